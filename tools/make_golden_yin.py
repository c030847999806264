"""Writes tests/golden/yin.npz and tests/golden/yin.json: the fixture that pins tests/yin_ref.py (the float64 truth of the GPU
tests of tdvc_yin_f0) to the reference's own YIN, and carries the tolerances those tests use.

    python tools/make_golden_yin.py [path/to/reference/util/yin.py]

Runs where the reference checkout is present (default /root/reference/util/yin.py, loaded by path: torch + numpy only). The two
files hold data only. Per case: the fp32 signal; the reference's hard and soft f0 computed in float64; 2048 sampled CMDF entries
(flat index, float64 value); E_ref32 / E_plain32 = max abs CMDF error of the reference / of the helper run in fp32 against
float64; S_ref32 = max relative soft-f0 error of the fp32 reference; a per-frame decision margin m (yin_ref.margins). The
inference-length case (1 x 71680) keeps its measured tolerances and a probe of its samples only: the test regenerates it from the seed.
tol = 4 * min(E_ref32, E_plain32): the kernel has to be as accurate as an fp32 evaluation of the same formula, and the 4x covers
a different summation order. Frames with m <= 2*tol are excused from the exact-decision checks.

Asserted here and again by tests/test_pitch_cpu.py: helper(float64) == reference(float64) (hard f0 exact, sampled CMDF within
1e-12); every case but `short` and `silence` has >= 15 % voiced and >= 15 % unvoiced frames; excused frames <= 5 %.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import yin_ref as YR  # noqa: E402

SR = 16000
THRESHOLD = 0.1
N_SAMPLED = 2048
# name, B, T, pitch_min, pitch_max, stride, seeds to try in order
CASES = [('speech', 2, 4000, 60, 500, 64), ('default', 2, 4000, 20, 20000, 64), ('short', 2, 300, 60, 500, 64),
         ('odd', 3, 4037, 50, 400, 160), ('silence', 1, 2000, 60, 500, 64)]
SEEDS = [1234, 7] + list(range(100, 140))


def load_reference(path):
    spec = importlib.util.spec_from_file_location('reference_yin', path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_cmdf(ref, x, tau_min, tau_max, stride):
    return ref._diff(ref._frame(x, 2 * tau_max, stride), tau_max)[..., tau_min:]


def build_case(ref, name, B, T, pmin, pmax, stride, seed):
    frame_stride = stride / SR
    tau_min, tau_max, stride_i = YR.params(SR, pmin, pmax, frame_stride)
    assert stride_i == stride, (stride_i, stride)
    rng = np.random.default_rng(seed)
    x32 = np.zeros((B, T), np.float32) if name == 'silence' else np.stack([YR.make_signal(rng, T, SR) for _ in range(B)])
    x = torch.from_numpy(x32)
    kw = dict(sample_rate=SR, pitch_min=pmin, pitch_max=pmax, frame_stride=frame_stride, threshold=THRESHOLD)
    hard64 = ref.estimate(x.double(), **kw)
    soft64 = ref.estimate(x.double(), soft=True, **kw)
    soft32 = ref.estimate(x, soft=True, **kw)
    c_ref64 = reference_cmdf(ref, x.double(), tau_min, tau_max, stride)
    c_ref32 = reference_cmdf(ref, x, tau_min, tau_max, stride)
    h_hard64, c_h64 = YR.estimate(x, SR, tau_min, tau_max, stride, THRESHOLD, dtype=torch.float64)
    h_hard32, c_h32 = YR.estimate(x, SR, tau_min, tau_max, stride, THRESHOLD, dtype=torch.float32)
    nf = YR.num_frames(T, tau_max, stride)
    assert hard64.shape == (B, nf) and c_h64.shape == c_ref64.shape == (B, nf, tau_max - 1 - tau_min)

    E_ref32 = float((c_ref32.double() - c_ref64).abs().max())
    E_plain32 = float((c_h32.double() - c_h64).abs().max())
    tol = 4 * min(E_ref32, E_plain32)
    m = YR.margins(c_h64, THRESHOLD)
    ok = m > 2 * tol
    rel = (soft32.double() - soft64).abs() / soft64.abs().clamp_min(1e-30)
    rel = torch.where((soft64 == 0) & (soft32 == 0), torch.zeros_like(rel), rel)
    S_ref32 = float(rel[ok].max()) if bool(ok.any()) else 0.0
    pick = np.sort(np.random.default_rng(seed + 1).choice(c_ref64.numel(), min(N_SAMPLED, c_ref64.numel()), replace=False))
    stats = dict(B=B, T=T, pitch_min=pmin, pitch_max=pmax, stride=stride, tau_min=tau_min, tau_max=tau_max, n_frames=nf, seed=seed,
                 E_ref32=E_ref32, E_plain32=E_plain32, S_ref32=S_ref32, tol=tol,
                 helper_hard_equals_reference=bool(torch.equal(h_hard64, hard64)),
                 helper_cmdf_max_abs_diff=float((c_h64 - c_ref64).abs().max()),
                 helper32_hard_disagreements=int(((h_hard32.double() - hard64).abs() > 1e-6 * hard64).sum()),
                 voiced_frac=float((hard64 > 0).double().mean()), excused_frac=float((~ok).double().mean()))
    arrays = {'signal': x32, 'f0_hard': hard64.numpy(), 'f0_soft': soft64.numpy(), 'cmdf_idx': pick.astype(np.int32),
              'cmdf_val': c_ref64.reshape(-1).numpy()[pick], 'margin': m.numpy()}
    return stats, arrays


def check(name, s):
    assert s['helper_hard_equals_reference'], name
    assert s['helper_cmdf_max_abs_diff'] <= 1e-12, (name, s['helper_cmdf_max_abs_diff'])
    assert s['excused_frac'] <= 0.05, (name, s['excused_frac'])
    if name not in ('short', 'silence'):
        assert 0.15 <= s['voiced_frac'] <= 0.85, (name, s['voiced_frac'])
    if name == 'silence':
        assert s['voiced_frac'] == 0.0


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else '/root/reference/util/yin.py')
    meta, arrays = {}, {}
    for name, B, T, pmin, pmax, stride in CASES:
        chosen = None
        for seed in SEEDS:
            stats, arr = build_case(ref, name, B, T, pmin, pmax, stride, seed)
            try:
                check(name, stats)
            except AssertionError as e:
                print(f'{name}: seed {seed} rejected: {e}')
                continue
            if chosen is None:
                chosen = (stats, arr)
            if name != 'short' or stats['voiced_frac'] > 0:      # `short`: prefer a seed with a voiced frame, if one exists
                chosen = (stats, arr)
                break
        assert chosen is not None, f'{name}: no seed meets the fixture conditions'
        stats, arr = chosen
        check(name, stats)
        meta[name] = stats
        arrays.update({f'{name}_{k}': v for k, v in arr.items()})
        print(name, json.dumps(stats))
    # inference length (test.max_segment): too long to store, so the test regenerates the signal from the seed (yin_ref.make_signal);
    # kept here: the tolerances measured on it and a probe of its samples
    stats, arr = build_case(ref, 'long', 1, YR.LONG_T, 60, 500, 64, YR.LONG_SEED)
    check('long', stats)
    probe = np.arange(0, YR.LONG_T, YR.LONG_T // 256)
    arrays.update({'long_probe_idx': probe.astype(np.int32), 'long_probe_val': arr['signal'][0, probe]})
    print('long', json.dumps(stats))
    out = os.path.join(ROOT, 'tests', 'golden')
    np.savez_compressed(os.path.join(out, 'yin.npz'), **arrays)
    with open(os.path.join(out, 'yin.json'), 'w') as f:
        json.dump({'sample_rate': SR, 'threshold': THRESHOLD, 'cases': meta, 'long': stats}, f, indent=1)
    size = sum(os.path.getsize(os.path.join(out, n)) for n in ('yin.npz', 'yin.json'))
    print(f'wrote yin.npz + yin.json: {size} bytes')


if __name__ == '__main__':
    main()
