"""float64 truth for the gradient of the soft YIN track: autograd through yin_ref.estimate(soft=True). Test helper; the fixture
tests/golden/yin_grad.npz + yin_grad.json (tools/make_golden_yin_grad.py) pins it to the gradient of the reference's own `estimate`
and carries the tolerances of the GPU tests (tests/test_pitch_grad_gpu.py).

Gradient cases (all at threshold 0.1, sample rate 16000): the signals of yin.npz where they exist, plus
    min      speech_signal[1][1000:1600]: T = 600 just above L = 532, the edge frames are mostly padding
    faint    speech_signal[1][:1400] scaled down until the 1e-5 floor of the CMDF denominator is active at some lags and not at
             others inside the frames that are on (tau_min = 1)
    long     1 x 71680 regenerated from yin_ref.LONG_SEED
The upstream gradient of a case is regenerated from its seed (`upstream`); `speech` has it zeroed on about half the frames, as
the masked loss produces.

Errors are row-normalised: max |g - truth| over a row [T] divided by that row's max |truth|. Rows whose truth is all zero are not
normalised; the tests require exact zeros there.
"""
import functools
import json
import os

import numpy as np
import torch

import yin_ref as YR

# name -> (signal source in yin.npz, settings source in yin.json or explicit (pitch_min, pitch_max, stride), case of yin.json whose
# CMDF tolerance bounds the on/off margin, seed of the upstream gradient, share of upstream entries zeroed)
CASES = {
    'speech': ('speech', 'speech', 'speech', 11, 0.5),
    'default': ('default', 'default', 'default', 12, 0.0),
    'odd': ('odd', 'odd', 'odd', 13, 0.0),
    'min': ('min', (60, 500, 64), 'speech', 14, 0.0),
    'short': ('short', 'short', 'short', 15, 0.0),
    'silence': ('silence', 'silence', 'silence', 16, 0.0),
    'faint': ('faint', (60, 16000, 64), 'speech', 17, 0.0),
}
FAINT_SCALES = (1e-2, 3e-3, 1e-3)
N_SAMPLED = 2048


def settings(name):
    """dict(pitch_min, pitch_max, stride, tau_min, tau_max) of a gradient case."""
    meta, _ = YR.fixture()
    src = 'speech' if name == 'long' else CASES[name][1]
    if isinstance(src, str):
        s = meta['long'] if name == 'long' else meta['cases'][src]
        pmin, pmax, stride = s['pitch_min'], s['pitch_max'], s['stride']
    else:
        pmin, pmax, stride = src
    tau_min, tau_max, stride_i = YR.params(meta['sample_rate'], pmin, pmax, stride / meta['sample_rate'])
    assert stride_i == stride
    return dict(pitch_min=pmin, pitch_max=pmax, stride=stride, tau_min=tau_min, tau_max=tau_max)


def base_signal(name):
    """fp32 [B, T] of the cases whose signal derives from yin.npz without a choice (`faint` comes scaled from the gradient fixture)."""
    _, g = YR.fixture()
    if name == 'min':
        return torch.from_numpy(g['speech_signal'][1:2, 1000:1600].copy())
    if name == 'faint':
        return torch.from_numpy(g['speech_signal'][1:2, :1400].copy())
    if name == 'long':
        return torch.from_numpy(YR.make_signal(np.random.default_rng(YR.LONG_SEED), YR.LONG_T, YR.fixture()[0]['sample_rate']))[None]
    return torch.from_numpy(g[f'{CASES[name][0]}_signal'])


def upstream(name, B, n_frames):
    """float64 [B, n_frames] standard normal from the case's seed, rounded to fp32 (the kernel takes exactly these values);
    entries zeroed where the case asks for it."""
    seed, zero_share = (18, 0.0) if name == 'long' else CASES[name][3:]
    rng = np.random.default_rng(seed)
    gy = rng.standard_normal((B, n_frames)).astype(np.float32).astype(np.float64)
    if zero_share > 0:
        gy = gy * (rng.random((B, n_frames)) >= zero_share)
    return torch.from_numpy(gy)


def grad(x, gy, tau_min, tau_max, stride, threshold, sample_rate, dtype=torch.float64, estimate=None):
    """d sum(gy * f0_soft(x)) / dx by autograd in `dtype`, one batch row at a time -> (dx [B, T], f0 [B, n_frames], cmdf) float64.
    estimate: a callable x -> f0 to differentiate instead of yin_ref.estimate (the generator passes the reference's)."""
    dxs, f0s, cs = [], [], []
    for b in range(x.shape[0]):
        xb = x[b:b + 1].to(dtype).clone().requires_grad_()
        if estimate is None:
            f0, c = YR.estimate(xb, sample_rate, tau_min, tau_max, stride, threshold, soft=True, dtype=dtype)
        else:
            f0, c = estimate(xb), None
        (f0 * gy[b:b + 1].to(dtype)).sum().backward()
        dxs.append(xb.grad.double())
        f0s.append(f0.detach().double())
        cs.append(None if c is None else c.detach().double())
    return torch.cat(dxs), torch.cat(f0s), (None if cs[0] is None else torch.cat(cs))


def row_error(g, truth):
    """Largest row-normalised error over the rows whose truth is not all zero (0.0 if there is none)."""
    g, truth = g.double(), truth.double()
    scale = truth.abs().amax(-1)
    live = scale > 0
    if not bool(live.any()):
        return 0.0
    return float(((g - truth).abs().amax(-1)[live] / scale[live]).max())


def on_frames(c, threshold):
    return (c < threshold).any(-1)


def floor_facts(x, tau_min, tau_max, stride, threshold):
    """For `faint`: over the frames that are on, whether every one has a lag m >= tau_min + 1 with S_m below and one with S_m above the
    floor, and the smallest |S_m - floor| / floor over those lags."""
    u = YR.frames(x.double(), tau_max, stride)
    L = 2 * tau_max
    d = torch.stack([(u[..., :L - tau] - u[..., tau:]).square().sum(-1) for tau in range(1, tau_max)], -1)
    S = d.cumsum(-1)[..., tau_min:]
    c = (d * torch.arange(1, tau_max, dtype=d.dtype) / d.cumsum(-1).clamp_min(YR.FLOOR))[..., tau_min:]
    on = on_frames(c, threshold)
    S = S[on]
    mixed = bool(((S < YR.FLOOR).any(-1) & (S > YR.FLOOR).any(-1)).all()) and S.shape[0] > 0
    dist = float(((S - YR.FLOOR).abs() / YR.FLOOR).min()) if S.numel() else float('inf')
    return mixed, dist, int(on.sum())


GOLDEN = YR.GOLDEN


@functools.lru_cache(maxsize=None)
def fixture():
    meta = json.load(open(os.path.join(GOLDEN, 'yin_grad.json')))
    return meta, np.load(os.path.join(GOLDEN, 'yin_grad.npz'))


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict(meta = the case's record in yin_grad.json, settings, x fp32 [B, T], gy float64 [B, n_frames], dx, f0, cmdf float64 from
    this helper, on [B, n_frames], margin = per-frame |min c - threshold|). Computed once, left unchanged."""
    meta, g = fixture()
    s = settings(name)
    x = torch.from_numpy(g['faint_signal']) if name == 'faint' else base_signal(name)
    thr, sr = meta['threshold'], meta['sample_rate']
    gy = upstream(name, x.shape[0], YR.num_frames(x.shape[1], s['tau_max'], s['stride']))
    dx, f0, c = grad(x, gy, s['tau_min'], s['tau_max'], s['stride'], thr, sr)
    return dict(meta=meta['cases'][name], settings=s, x=x, gy=gy, dx=dx, f0=f0, cmdf=c, on=on_frames(c, thr),
                margin=(c.amin(-1) - thr).abs())
