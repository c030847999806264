"""Writes tests/golden/yin_grad.npz and tests/golden/yin_grad.json: the fixture that pins tests/yin_grad_ref.py (the float64 truth
of the GPU tests of tdvc_yin_soft_bwd) to the gradient of the reference's own soft YIN, and carries the tolerances those tests use.

    python tools/make_golden_yin_grad.py [path/to/reference/util/yin.py]

Runs where the reference checkout is present (default /root/reference/util/yin.py, loaded by path: torch + numpy only) and needs
tests/golden/yin.npz (tools/make_golden_yin.py). The two files hold data only. Per case of yin_grad_ref.CASES and for `long`: the
seed of the upstream gradient; up to 2048 sampled entries (flat index, float64 value) of the REFERENCE's float64 gradient
d sum(gy * f0) / d signal; each row's max |gradient|; E_ref32 / E_plain32 = the largest row-normalised error of the reference /
of the helper differentiated in fp32 against float64; tol_g = 4 * min(E_ref32, E_plain32) (the kernel has to be as accurate as an
fp32 evaluation of the same formulas, 4x for a different summation order); the share of frames that are on and the smallest
|min_k c - threshold| over all frames. The `faint` signal (the scale is a choice made here) is stored; the others derive from yin.npz.

Asserted here and again by tests/test_pitch_grad_cpu.py:
  - helper gradient == reference gradient within 1e-9 (row-normalised), rows that are zero in one are zero in the other;
  - where a case has frames that are on, EVERY frame's |min_k c - threshold| exceeds twice the forward CMDF tolerance of the
    matching case of yin.json: the on/off decision of an fp32 kernel cannot differ, so no frame is excused from the comparison;
  - `default` row 1, `short` and `silence` have an all-zero gradient; `silence` has every frame on;
  - `faint`: in every frame that is on, the floor is active at some lag m >= tau_min + 1 and inactive at another, and no S_m is
    closer to the floor than 1e-3 of it; the first scale of yin_grad_ref.FAINT_SCALES that achieves this is kept.
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


def load_reference(path):
    spec = importlib.util.spec_from_file_location('reference_yin', path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build_case(ref, name, x, meta):
    sr, thr = meta['sample_rate'], meta['threshold']
    s = GR.settings(name)
    B, T = x.shape
    nf = YR.num_frames(T, s['tau_max'], s['stride'])
    gy = GR.upstream(name, B, nf)
    a = (s['tau_min'], s['tau_max'], s['stride'], thr, sr)

    def ref_estimate(xb):
        return ref.estimate(xb, sr, pitch_min=s['pitch_min'], pitch_max=s['pitch_max'], frame_stride=s['stride'] / sr, threshold=thr, soft=True)
    g_ref64, f0_ref64, _ = GR.grad(x, gy, *a, dtype=torch.float64, estimate=ref_estimate)
    g_ref32, _, _ = GR.grad(x, gy, *a, dtype=torch.float32, estimate=ref_estimate)
    g_h64, f0_h64, c = GR.grad(x, gy, *a, dtype=torch.float64)
    g_h32, _, _ = GR.grad(x, gy, *a, dtype=torch.float32)
    assert g_ref64.shape == (B, T) and bool(torch.isfinite(g_ref64).all()) and bool(torch.isfinite(g_h64).all())
    row_max = g_ref64.abs().amax(-1)
    zero_rows = row_max == 0
    E_ref32, E_plain32 = GR.row_error(g_ref32, g_h64), GR.row_error(g_h32, g_h64)
    on = GR.on_frames(c, thr)
    margin = (c.amin(-1) - thr).abs()
    cmdf_case = 'long' if name == 'long' else GR.CASES[name][2]
    cmdf_tol = (meta['long'] if name == 'long' else meta['cases'][cmdf_case])['tol']
    pick = np.sort(np.random.default_rng(1000 + len(name)).choice(g_ref64.numel(), min(GR.N_SAMPLED, g_ref64.numel()), replace=False))
    stats = dict(B=B, T=T, n_frames=nf, **s, E_ref32=E_ref32, E_plain32=E_plain32, tol_g=4 * min(E_ref32, E_plain32),
                 helper_vs_reference=GR.row_error(g_h64, g_ref64),
                 helper_zero_rows_match=bool(torch.equal(g_h64.abs().amax(-1) == 0, zero_rows)),
                 f0_helper_vs_reference=float((f0_h64 - f0_ref64).abs().max()),
                 zero_rows=[int(i) for i in torch.nonzero(zero_rows).flatten()],
                 on_frac=float(on.double().mean()), on_frames=int(on.sum()), min_margin=float(margin.min()),
                 cmdf_tol_case=cmdf_case, cmdf_tol=cmdf_tol, upstream_zero_frac=float((gy == 0).double().mean()))
    arrays = {'grad_idx': pick.astype(np.int32), 'grad_val': g_ref64.reshape(-1).numpy()[pick], 'row_max': row_max.numpy()}
    return stats, arrays


def check(name, s):
    assert s['helper_vs_reference'] <= 1e-9 and s['helper_zero_rows_match'], (name, s['helper_vs_reference'])
    if s['on_frames'] > 0 and name != 'silence':      # silence: c == 0 exactly in every dtype, the decision cannot differ
        assert s['min_margin'] > 2 * s['cmdf_tol'], (name, s['min_margin'], s['cmdf_tol'])
    if name in ('short', 'silence'):
        assert s['zero_rows'] == list(range(s['B'])) and s['tol_g'] == 0.0, name
    if name == 'short':
        assert s['on_frames'] == 0
    if name == 'silence':
        assert s['on_frac'] == 1.0
    if name == 'default':
        assert s['zero_rows'] == [1], s['zero_rows']
    if name == 'speech':
        assert 0.35 <= s['upstream_zero_frac'] <= 0.65


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else '/root/reference/util/yin.py')
    meta, _ = YR.fixture()
    thr = meta['threshold']
    cases, arrays = {}, {}
    for name in list(GR.CASES) + ['long']:
        t0 = time.time()
        x = GR.base_signal(name)
        extra = {}
        if name == 'faint':
            s = GR.settings(name)
            for scale in GR.FAINT_SCALES:
                xs = (x.double() * scale).float()
                mixed, dist, n_on = GR.floor_facts(xs, s['tau_min'], s['tau_max'], s['stride'], thr)
                print(f'faint: scale {scale}: frames on {n_on}, floor mixed in every one: {mixed}, min |S - floor| / floor {dist:.3e}')
                if mixed and dist >= 1e-3:
                    x, extra = xs, dict(scale=scale, floor_mixed_in_every_on_frame=mixed, floor_min_rel_distance=dist)
                    break
            assert extra, 'faint: no scale meets the floor conditions'
            arrays['faint_signal'] = x.numpy()
        stats, arr = build_case(ref, name, x, meta)
        stats.update(extra)
        check(name, stats)
        cases[name] = stats
        arrays.update({f'{name}_{k}': v for k, v in arr.items()})
        print(name, f'{time.time() - t0:.1f}s', json.dumps(stats))
    out = os.path.join(ROOT, 'tests', 'golden')
    np.savez_compressed(os.path.join(out, 'yin_grad.npz'), **arrays)
    with open(os.path.join(out, 'yin_grad.json'), 'w') as f:
        json.dump({'sample_rate': meta['sample_rate'], 'threshold': thr, 'cases': cases}, f, indent=1)
    size = sum(os.path.getsize(os.path.join(out, n)) for n in ('yin_grad.npz', 'yin_grad.json'))
    print(f'wrote yin_grad.npz + yin_grad.json: {size} bytes')
    assert size <= 300 * 1024


if __name__ == '__main__':
    main()
