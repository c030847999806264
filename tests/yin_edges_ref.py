"""Edge cases of tdvc_yin_f0 and tdvc_yin_soft_bwd: the case table, the signal generator and the float64 truth per case. Test
helper in the style of yin_ref.py / yin_grad_ref.py; all the maths comes from those two (yin_ref.cmdf / hard_tau / soft_tau /
margins, yin_grad_ref.grad). The fixture tests/golden/yin_edges.npz + yin_edges.json (tools/make_golden_yin_edges.py) pins the
truth to the reference's own YIN at every row of the table and carries the tolerances of tests/test_pitch_edges_gpu.py.

The fixtures yin.npz and yin_grad.npz only hold tau_max 266, 320 and 800, stride 64 and 160 and T >= 300. This table reaches what
they do not: odd tau_max (L = 2*tau_max with L % 4 == 2: the staged frame ends inside a float4, the backward's padded row
length differs from L and its last group of four positions holds two beyond the frame), the cap tau_max = 1024 and 1023, two and
four-or-more j slices per row of the difference function, fewer tau groups than a wave, the smallest n the ABI takes, stride > L
(positions no frame covers), stride 1 (up to L frames on one sample), T < L and T = 1.

All cases: sample rate 16000, threshold 0.1. `plan` mirrors the host code's split of the work (csrc/pitch_yin.hip,
pitch_yin_bwd.hip) so that tests/test_pitch_edges_cpu.py can assert that the table still reaches that list; it is a mirror, not
checked against the library.
"""
import functools
import json
import os

import numpy as np
import torch

import yin_grad_ref as GR
import yin_ref as YR

SR, THR = 16000, 0.1
GOLDEN = YR.GOLDEN
N_PROBE = 256
N_SAMPLED = 512

# name -> (tau_min, tau_max, stride, B, T)
CASES = {
    'odd267': (32, 267, 64, 2, 2200),
    'cap1024': (0, 1024, 1500, 1, 8200),
    'odd1023': (40, 1023, 1100, 2, 6200),
    'nc4_255': (16, 255, 96, 2, 2100),
    'nc2_401': (20, 401, 128, 1, 3300),
    'gap64': (8, 64, 300, 2, 1300),
    'dense21': (2, 21, 1, 2, 97),
    'n2_133': (130, 133, 50, 2, 900),
    'short101': (10, 101, 37, 3, 150),
    'tiny7': (1, 7, 2, 2, 60),
    'tiny5': (0, 5, 1, 2, 40),
    'tiny3': (0, 3, 1, 2, 30),
    'one33': (4, 33, 16, 1, 1),
}
# tiny3: two lags on an alternating signal, the float64 gradient is ill-conditioned beyond use (an fp32 evaluation is off by 1e9
# relative). one33: the CMDF does not depend on the single sample's amplitude, the true gradient is zero only by cancellation.
FORWARD_ONLY = ('tiny3', 'one33')
BACKWARD_CASES = tuple(n for n in CASES if n not in FORWARD_ONLY)
GY_ZERO_SHARE = {'odd267': 0.5}      # the gy == 0 early exit runs beside live frames


def settings(name):
    tau_min, tau_max, stride, B, T = CASES[name]
    return dict(tau_min=tau_min, tau_max=tau_max, stride=stride, B=B, T=T, L=2 * tau_max, n=tau_max - 1 - tau_min,
                n_frames=YR.num_frames(T, tau_max, stride))


def plan(tau_max):
    """The split the host code makes: NG groups of four tau and NC j slices per row in the difference function; in the backward's
    correlation NGn groups of four positions, NCm slices of m with mslice lags each, run in `rounds` rounds of 256 work items."""
    L = 2 * tau_max
    Lp, M4 = (L + 3) & ~3, (tau_max + 3) & ~3
    NG = (tau_max + 3) // 4
    NGn = Lp // 4
    best, best_num, best_den = 1, 0, 1
    for s in range(1, min(8, 4096 // Lp, M4 // 4) + 1):
        items = NGn * s
        rounds = (items + 255) // 256
        if items * best_den > best_num * rounds:
            best, best_num, best_den = s, items, rounds
    return dict(L=L, Lp=Lp, M4=M4, NG=NG, NC=256 // NG, NGn=NGn, NCm=best, mslice=((M4 // 4 + best - 1) // best) * 4,
                rounds=(NGn * best + 255) // 256)


def make_signal(rng, name):
    """fp32 [T] of one row. Segments of L .. 2L samples: with probability 0.3 noise 0.3 N(0, 1), else a three-partial tone
    sum_h sin(h phi + phase_h) / h whose period is uniform in [tau_min + 3, max(tau_min + 4, 0.45 tau_max)] samples, plus
    0.01 N(0, 1); everything scaled by 0.03. tiny3 (lags 1 and 2 only): (-1)^t (1 + 0.02 N) on the first half, noise on the second.
    one33 (T = 1): the sample 0.02."""
    tau_min, tau_max, _, _, T = CASES[name]
    if name == 'one33':
        return np.full(T, 0.02, np.float32)
    if name == 'tiny3':
        h = T // 2
        alt = (-1.0) ** np.arange(h) * (1 + 0.02 * rng.standard_normal(h))
        return (0.03 * np.concatenate([alt, 0.3 * rng.standard_normal(T - h)])).astype(np.float32)
    L = 2 * tau_max
    x = np.zeros(T)
    t = 0
    while t < T:
        n = min(int(rng.integers(L, 2 * L + 1)), T - t)
        if rng.random() < 0.3:
            seg = 0.3 * rng.standard_normal(n)
        else:
            period = rng.uniform(tau_min + 3, max(tau_min + 4, 0.45 * tau_max))
            phase = rng.uniform(0, 2 * np.pi, 3)
            phi = 2 * np.pi * np.arange(n) / period
            seg = sum(np.sin(h * phi + phase[h - 1]) / h for h in (1, 2, 3)) + 0.01 * rng.standard_normal(n)
        x[t:t + n] = seg
        t += n
    return (0.03 * x).astype(np.float32)


def signal(name, seed):
    """fp32 [B, T]: the rows drawn one after the other from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([make_signal(rng, name) for _ in range(CASES[name][3])]))


def upstream(name):
    """float64 [B, n_frames] standard normal from the case's own seed, rounded to fp32 (the kernel takes exactly these values);
    odd267 has half of its entries zeroed."""
    s = settings(name)
    rng = np.random.default_rng(5000 + list(CASES).index(name))
    gy = rng.standard_normal((s['B'], s['n_frames'])).astype(np.float32).astype(np.float64)
    share = GY_ZERO_SHARE.get(name, 0.0)
    if share > 0:
        gy = gy * (rng.random(gy.shape) >= share)
    return torch.from_numpy(gy)


def probe_idx(name):
    B, T = CASES[name][3:]
    return np.unique(np.linspace(0, B * T - 1, min(N_PROBE, B * T)).astype(np.int64))


def forward64(x, name):
    """dict(cmdf, hard, soft f0, margin = yin_ref.margins, thr_margin = |min c - threshold|, on) in float64."""
    s = settings(name)
    c = YR.cmdf(x.double(), s['tau_min'], s['tau_max'], s['stride'])
    return dict(cmdf=c, hard=YR.to_f0(YR.hard_tau(c, THR), s['tau_min'], SR), soft=YR.to_f0(YR.soft_tau(c, THR), s['tau_min'], SR),
                margin=YR.margins(c, THR), thr_margin=(c.amin(-1) - THR).abs(), on=GR.on_frames(c, THR))


def grad64(x, name, dtype=torch.float64, estimate=None):
    s = settings(name)
    return GR.grad(x, upstream(name), s['tau_min'], s['tau_max'], s['stride'], THR, SR, dtype=dtype, estimate=estimate)[0]


@functools.lru_cache(maxsize=None)
def fixture():
    meta = json.load(open(os.path.join(GOLDEN, 'yin_edges.json')))
    return meta, np.load(os.path.join(GOLDEN, 'yin_edges.npz'))


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict(meta = the case's record in yin_edges.json, settings, x fp32 [B, T] regenerated from the recorded seed and checked
    against the stored probe, cmdf / hard / soft / margin / thr_margin / on in float64, ok = non-excused frames, and for the
    backward cases gy and dx in float64, else None). Computed once, left unchanged."""
    meta, g = fixture()
    m = meta['cases'][name]
    x = signal(name, m['seed'])
    assert np.array_equal(g[f'{name}_probe_idx'], probe_idx(name))
    assert float(np.abs(x.reshape(-1).numpy()[g[f'{name}_probe_idx']] - g[f'{name}_probe_val']).max()) <= 1e-6, name
    t = dict(meta=m, settings=settings(name), x=x, **forward64(x, name))
    t['ok'] = t['margin'] > 2 * m['tol']
    backward = name in BACKWARD_CASES
    t['gy'] = upstream(name) if backward else None
    t['dx'] = grad64(x, name) if backward else None
    return t
