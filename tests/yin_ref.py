"""Plain torch restatement of the YIN definitions behind tdvc_yin_f0 (include/tdvc.h), in a caller-chosen dtype. Test helper:
the GPU tests take their float64 truth from here, and tests/golden/yin.npz pins it to the reference's own `estimate`.

Written from the formulae, with the difference function summed directly (one term-wise sum per tau):
    L = 2*tau_max; the signal is zero-extended to L if shorter, then zero-padded by L/2 left and L/2 - 1 right;
    frame f = padded[f*stride : f*stride + L];
    d[tau]  = sum_{j=0}^{L-1-tau} (u[j] - u[j+tau])^2,              tau = 0 .. tau_max-1
    c[k]    = d[k+1] * (k+1) / max(sum_{i=1}^{k+1} d[i], 1e-5),     k = 0 .. tau_max-2, then the first tau_min entries dropped
    hard:   fb = first index with c < threshold; none, or index 0 -> non-periodic; else tau = first index >= fb with
            c[k+1] - c[k] >= 0 (the last index always qualifies)
    soft:   tau = sum_k softmax(-100 c)[k] * k, times 1 if any c < threshold else 0
    f0      = sample_rate / (tau + tau_min + 1) where tau > 0, else 0
The floor 1e-5 is the float32 number nearest to 1e-5 in every dtype (a float32 constant in the reference and in the kernel).
"""
import functools
import json
import os

import numpy as np
import torch

THETA = 100.0
FLOOR = float(np.float32(1e-5))


def params(sample_rate, pitch_min, pitch_max, frame_stride):
    """(tau_min, tau_max, stride) exactly as `estimate` computes them."""
    return int(sample_rate / pitch_max), int(sample_rate / pitch_min), int(frame_stride * sample_rate)


def num_frames(T, tau_max, stride):
    return (max(T, 2 * tau_max) - 1) // stride + 1


def frames(x, tau_max, stride):
    """x [..., T] -> [..., n_frames, L]"""
    L = 2 * tau_max
    T = x.shape[-1]
    padded = torch.zeros(*x.shape[:-1], max(T, L) + L - 1, dtype=x.dtype)
    padded[..., L // 2:L // 2 + T] = x
    return padded.unfold(-1, L, stride)


def cmdf(x, tau_min, tau_max, stride):
    """x [..., T] -> c [..., n_frames, tau_max - 1 - tau_min] in x's dtype."""
    u = frames(x, tau_max, stride)
    L = 2 * tau_max
    d = torch.stack([(u[..., :L - tau] - u[..., tau:]).square().sum(-1) for tau in range(1, tau_max)], -1)
    k1 = torch.arange(1, tau_max, dtype=x.dtype)
    c = d * k1 / d.cumsum(-1).clamp_min(FLOOR)
    return c[..., tau_min:]


def hard_tau(c, threshold):
    n = c.shape[-1]
    below = c < threshold
    idx = torch.arange(n)
    fb = torch.where(below, idx, n).amin(-1, keepdim=True)                  # n = no crossing
    periodic = (fb > 0) & (fb < n)
    rising = torch.cat([c[..., 1:] - c[..., :-1] >= 0, torch.ones_like(below[..., :1])], -1)
    tau = torch.where(rising & (idx >= fb), idx, n).amin(-1)
    return torch.where(periodic[..., 0], tau, 0)


def soft_tau(c, threshold):
    alpha = torch.softmax(-THETA * c, -1)
    tau = (alpha * torch.arange(c.shape[-1], dtype=c.dtype)).sum(-1)
    return tau * (c < threshold).any(-1).to(c.dtype)


def to_f0(tau, tau_min, sample_rate):
    t = tau.to(torch.float64) if not tau.is_floating_point() else tau
    return torch.where(tau > 0, sample_rate / (t + tau_min + 1), torch.zeros_like(t))


def estimate(x, sample_rate, tau_min, tau_max, stride, threshold=0.1, soft=False, dtype=torch.float64):
    """-> (f0 [..., n_frames], c [..., n_frames, n]) computed in `dtype`."""
    c = cmdf(torch.as_tensor(x).to(dtype), tau_min, tau_max, stride)
    tau = soft_tau(c, threshold) if soft else hard_tau(c, threshold)
    return to_f0(tau, tau_min, sample_rate).to(dtype), c


def margins(c, threshold):
    """Per frame, how far the float64 CMDF is from changing the hard decision: the smallest of |c - threshold| over the indices
    up to the first crossing fb (all indices when there is none) and |c[k+1] - c[k]| over fb .. tau."""
    n = c.shape[-1]
    idx = torch.arange(n)
    below = c < threshold
    fb = torch.where(below, idx, n).amin(-1, keepdim=True)
    inf = torch.full_like(c, float('inf'))
    m_thr = torch.where(idx <= fb, (c - threshold).abs(), inf).amin(-1)
    tau = hard_tau(c, threshold).unsqueeze(-1)
    step = torch.cat([(c[..., 1:] - c[..., :-1]).abs(), inf[..., :1]], -1)
    periodic = (fb > 0) & (fb < n)
    m_step = torch.where(periodic & (idx >= fb) & (idx <= tau), step, inf).amin(-1)
    return torch.minimum(m_thr, m_step)


def make_signal(rng, T, sample_rate=16000):
    """Harmonic tone (4 partials) on a smoothed piecewise 90-300 Hz contour, about 30 % unvoiced segments; noise sigma 0.01 on
    voiced and 0.3 on unvoiced stretches; overall scale 0.03 (the project's -30 dB convention)."""
    f = np.zeros(T)
    voiced = np.zeros(T, bool)
    t = 0
    while t < T:
        n = int(rng.integers(T // 8 + 1, T // 3 + 2))
        f[t:t + n] = rng.uniform(90.0, 300.0)
        voiced[t:t + n] = rng.random() >= 0.3
        t += n
    w = max(1, min(200, T // 4))
    f = np.convolve(np.pad(f, (w // 2, w - 1 - w // 2), mode='edge'), np.ones(w) / w, mode='valid')
    phase = 2 * np.pi * np.cumsum(f) / sample_rate
    tone = sum(np.sin(h * phase) / h for h in range(1, 5))
    noise = rng.standard_normal(T)
    return (0.03 * np.where(voiced, tone + 0.01 * noise, 0.3 * noise)).astype(np.float32)


# ---- the fixture (tests/golden/yin.npz + yin.json, tools/make_golden_yin.py) and the float64 truth per case, computed once
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('speech', 'default', 'short', 'odd', 'silence')
LONG_T, LONG_SEED = 71680, 4321      # inference length: regenerated from the seed, tolerances in yin.json['long']


@functools.lru_cache(maxsize=None)
def fixture():
    meta = json.load(open(os.path.join(GOLDEN, 'yin.json')))
    return meta, np.load(os.path.join(GOLDEN, 'yin.npz'))


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict(meta, x fp32 [B, T], hard, soft f0 and cmdf in float64 from this helper, margin, ok = non-excused frames)."""
    meta, g = fixture()
    s = meta['cases'][name]
    x = torch.from_numpy(g[f'{name}_signal'])
    thr, sr = meta['threshold'], meta['sample_rate']
    c = cmdf(x.double(), s['tau_min'], s['tau_max'], s['stride'])
    hard, soft = to_f0(hard_tau(c, thr), s['tau_min'], sr), to_f0(soft_tau(c, thr), s['tau_min'], sr)
    m = margins(c, thr)
    return dict(meta=s, x=x, hard=hard, soft=soft, cmdf=c, margin=m, ok=m > 2 * s['tol'])


@functools.lru_cache(maxsize=None)
def long_truth():
    """The inference-length case (B = 1, T = 71680, speech settings): the signal regenerated from its seed, checked against the
    probe the fixture keeps; float64 truth and margins computed here, tolerances from the fixture."""
    meta, g = fixture()
    s = meta['long']
    x = torch.from_numpy(make_signal(np.random.default_rng(LONG_SEED), LONG_T, meta['sample_rate']))[None]
    assert float((x[0, g['long_probe_idx']] - torch.from_numpy(g['long_probe_val'])).abs().max()) <= 1e-6
    thr, sr = meta['threshold'], meta['sample_rate']
    c = cmdf(x.double(), s['tau_min'], s['tau_max'], s['stride'])
    hard, soft = to_f0(hard_tau(c, thr), s['tau_min'], sr), to_f0(soft_tau(c, thr), s['tau_min'], sr)
    m = margins(c, thr)
    return dict(meta=s, x=x, hard=hard, soft=soft, cmdf=c, margin=m, ok=m > 2 * s['tol'])
