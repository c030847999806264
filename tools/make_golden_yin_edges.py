"""Writes tests/golden/yin_edges.npz and tests/golden/yin_edges.json: the fixture that pins tests/yin_edges_ref.py (the float64
truth of tests/test_pitch_edges_gpu.py) to the reference's own YIN at every row of the edge-case table, and carries the tolerances
those tests use.

    python tools/make_golden_yin_edges.py path/to/reference/util/yin.py

Runs where the reference checkout is present (its util/yin.py is loaded by path: torch + numpy only). The two
files hold data only. Signals are regenerated from seeds (yin_edges_ref.signal); per case the fixture keeps the chosen seed, a
probe of up to 256 samples, the reference's float64 hard and soft f0, up to 512 sampled entries (flat index, float64 value) of the
reference's float64 CMDF and, for the backward cases, of its float64 gradient with each row's max |gradient|, and
    E_ref32 / E_plain32    max abs CMDF error of the reference / of the helper run in fp32 against float64
    S_ref32                max relative soft-f0 error of the fp32 reference on the non-excused frames
    Eg_ref32 / Eg_plain32  the same pair for the row-normalised gradient
    tol = 4 * min(E_ref32, E_plain32), tol_g = 4 * min(Eg_ref32, Eg_plain32): the project's rule (tools/make_golden_yin.py,
                           make_golden_yin_grad.py) on new inputs; nothing is taken from the kernel
    on / voiced / excused share of the frames, the smallest |min_k c - threshold| over all frames.

The first seed of SEEDS that meets every condition is kept. Asserted here and again by tests/test_pitch_edges_cpu.py:
  - helper(float64) == reference(float64): hard f0 exact, CMDF within 1e-12, gradient within 1e-9 (row-normalised) with the same
    zero rows;
  - excused frames (yin_ref.margins <= 2*tol) are at most 5 % of the case;
  - EVERY frame's |min_k c - threshold| exceeds 2*tol: the on/off decision is out of an fp32 kernel's reach and the backward
    excuses nothing;
  - the share of frames that are on is within [0.1, 0.9]; at least one frame is hard-voiced where n >= 4 (one33 is exempt from
    both: a single sample gives frames that are non-periodic or all zero, so none is hard-voiced and the on frames are the zero ones);
  - backward cases have at least one live row, and tol_g <= 1e-4. The cap keeps the bound from going vacuous: with few lags the
    theta = 100 softmax saturates, and a row made only of saturated frames has a tiny, badly conditioned gradient. Such seeds are
    rejected, not tolerated.
"""
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import yin_ref as YR  # noqa: E402
import yin_grad_ref as GR  # noqa: E402
import yin_edges_ref as ER  # noqa: E402

SEEDS = range(64)
TOL_G_CAP = 1e-4


def load_reference(path):
    spec = importlib.util.spec_from_file_location('reference_yin', path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_kw(s):
    """Arguments from which `estimate` derives exactly (tau_min, tau_max, stride): the half keeps int() off a rounding edge."""
    kw = dict(sample_rate=ER.SR, pitch_min=ER.SR / (s['tau_max'] + 0.5), pitch_max=ER.SR / (s['tau_min'] + 0.5),
              frame_stride=(s['stride'] + 0.5) / ER.SR)
    assert YR.params(ER.SR, kw['pitch_min'], kw['pitch_max'], kw['frame_stride']) == (s['tau_min'], s['tau_max'], s['stride'])
    return dict(kw, threshold=ER.THR)


def reference_cmdf(ref, x, s):
    return ref._diff(ref._frame(x, 2 * s['tau_max'], s['stride']), s['tau_max'])[..., s['tau_min']:]


def build_forward(ref, name, seed):
    s = ER.settings(name)
    kw = reference_kw(s)
    x = ER.signal(name, seed)
    assert x.dtype == torch.float32 and tuple(x.shape) == (s['B'], s['T'])
    hard64 = ref.estimate(x.double(), **kw)
    soft64 = ref.estimate(x.double(), soft=True, **kw)
    soft32 = ref.estimate(x, soft=True, **kw)
    c_ref64, c_ref32 = reference_cmdf(ref, x.double(), s), reference_cmdf(ref, x, s)
    h = ER.forward64(x, name)
    c_h32 = YR.cmdf(x, s['tau_min'], s['tau_max'], s['stride'])
    assert hard64.shape == (s['B'], s['n_frames']) and h['cmdf'].shape == c_ref64.shape == (s['B'], s['n_frames'], s['n'])
    E_ref32 = float((c_ref32.double() - c_ref64).abs().max())
    E_plain32 = float((c_h32.double() - h['cmdf']).abs().max())
    tol = 4 * min(E_ref32, E_plain32)
    ok = h['margin'] > 2 * tol
    rel = (soft32.double() - soft64).abs() / soft64.abs().clamp_min(1e-30)
    rel = torch.where((soft64 == 0) & (soft32 == 0), torch.zeros_like(rel), rel)
    pick = np.sort(np.random.default_rng(seed + 1).choice(c_ref64.numel(), min(ER.N_SAMPLED, c_ref64.numel()), replace=False))
    probe = ER.probe_idx(name)
    stats = dict(**s, seed=seed, E_ref32=E_ref32, E_plain32=E_plain32, tol=tol, S_ref32=float(rel[ok].max()) if bool(ok.any()) else 0.0,
                 helper_hard_equals_reference=bool(torch.equal(h['hard'], hard64)),
                 helper_cmdf_max_abs_diff=float((h['cmdf'] - c_ref64).abs().max()),
                 helper_soft_max_abs_diff=float((h['soft'] - soft64).abs().max()),
                 on_frac=float(h['on'].double().mean()), voiced_frac=float((hard64 > 0).double().mean()),
                 excused_frac=float((~ok).double().mean()), min_margin=float(h['thr_margin'].min()))
    arrays = {'probe_idx': probe, 'probe_val': x.reshape(-1).numpy()[probe], 'f0_hard': hard64.numpy(), 'f0_soft': soft64.numpy(),
              'cmdf_idx': pick.astype(np.int32), 'cmdf_val': c_ref64.reshape(-1).numpy()[pick]}
    return x, stats, arrays


def check_forward(name, s):
    assert s['helper_hard_equals_reference'], 'hard f0 differs from the reference'
    assert s['helper_cmdf_max_abs_diff'] <= 1e-12, ('helper CMDF', s['helper_cmdf_max_abs_diff'])
    assert s['excused_frac'] <= 0.05, ('excused', s['excused_frac'])
    assert s['min_margin'] > 2 * s['tol'], ('on/off margin', s['min_margin'], s['tol'])
    if name != 'one33':
        assert 0.1 <= s['on_frac'] <= 0.9, ('on share', s['on_frac'])
    if s['n'] >= 4 and name != 'one33':      # one sample cannot be periodic: its frames are non-periodic or all zero (first crossing at index 0)
        assert s['voiced_frac'] > 0, 'no hard-voiced frame'
    if name == 'one33':
        assert s['voiced_frac'] == 0.0 and 0 < s['on_frac'] < 1


def build_backward(ref, name, x):
    s = ER.settings(name)
    kw = reference_kw(s)

    def ref_estimate(xb):
        return ref.estimate(xb, soft=True, **kw)
    g_ref64 = ER.grad64(x, name, estimate=ref_estimate)
    g_ref32 = ER.grad64(x, name, dtype=torch.float32, estimate=ref_estimate)
    g_h64 = ER.grad64(x, name)
    g_h32 = ER.grad64(x, name, dtype=torch.float32)
    assert g_ref64.shape == tuple(x.shape) and bool(torch.isfinite(g_ref64).all()) and bool(torch.isfinite(g_h64).all())
    row_max = g_ref64.abs().amax(-1)
    Eg_ref32, Eg_plain32 = GR.row_error(g_ref32, g_h64), GR.row_error(g_h32, g_h64)
    pick = np.sort(np.random.default_rng(2000 + len(name)).choice(g_ref64.numel(), min(ER.N_SAMPLED, g_ref64.numel()), replace=False))
    stats = dict(Eg_ref32=Eg_ref32, Eg_plain32=Eg_plain32, tol_g=4 * min(Eg_ref32, Eg_plain32),
                 helper_grad_vs_reference=GR.row_error(g_h64, g_ref64),
                 helper_zero_rows_match=bool(torch.equal(g_h64.abs().amax(-1) == 0, row_max == 0)),
                 zero_rows=[int(i) for i in torch.nonzero(row_max == 0).flatten()],
                 upstream_zero_frac=float((ER.upstream(name) == 0).double().mean()))
    arrays = {'grad_idx': pick.astype(np.int32), 'grad_val': g_ref64.reshape(-1).numpy()[pick], 'row_max': row_max.numpy()}
    return stats, arrays


def check_backward(name, s):
    assert s['helper_grad_vs_reference'] <= 1e-9 and s['helper_zero_rows_match'], ('helper gradient', s['helper_grad_vs_reference'])
    assert len(s['zero_rows']) < s['B'], 'no live row'
    assert 0 < s['tol_g'] <= TOL_G_CAP, ('tol_g', s['tol_g'])
    if name in ER.GY_ZERO_SHARE:
        assert 0.3 <= s['upstream_zero_frac'] <= 0.7


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    cases, arrays = {}, {}
    for name in ER.CASES:
        t0 = time.time()
        chosen, passed = None, []
        for seed in SEEDS:
            if seed >= 12 and chosen is not None:      # seeds 0 .. 11 are all tried, to report how many pass
                break
            try:
                x, stats, arr = build_forward(ref, name, seed)
                check_forward(name, stats)
                if name in ER.BACKWARD_CASES:
                    gs, ga = build_backward(ref, name, x)
                    stats.update(gs); arr.update(ga)
                    check_backward(name, stats)
            except AssertionError as e:
                if seed < 12:
                    print(f'{name}: seed {seed} rejected: {e}')
                continue
            passed.append(seed)
            if chosen is None:
                chosen = (stats, arr)
        assert chosen is not None, f'{name}: no seed meets the fixture conditions'
        stats, arr = chosen
        cases[name] = stats
        arrays.update({f'{name}_{k}': v for k, v in arr.items()})
        print(name, f'{time.time() - t0:.1f}s', 'seeds that pass among those tried:', passed, json.dumps(stats))
    out = os.path.join(ROOT, 'tests', 'golden')
    np.savez_compressed(os.path.join(out, 'yin_edges.npz'), **arrays)
    with open(os.path.join(out, 'yin_edges.json'), 'w') as f:
        json.dump({'sample_rate': ER.SR, 'threshold': ER.THR, 'cases': cases}, f, indent=1)
    size = sum(os.path.getsize(os.path.join(out, n)) for n in ('yin_edges.npz', 'yin_edges.json'))
    print(f'wrote yin_edges.npz + yin_edges.json: {size} bytes')
    assert size <= 300 * 1024


if __name__ == '__main__':
    main()
