"""Times tdvc_yin_f0 (pitch.yin_f0, hard search) on the GPU beside the FFT formulation of the same tracker written with stock
torch ops, which is what a user would otherwise run on the device.

    python tools/bench_yin.py [--iters 200] [--warmup 20]

Shapes: 16 x 16000 with speech settings (60-500 Hz, hop 64) and with `estimate`'s defaults (20-20000 Hz, 10 ms), and 1 x 71680
with speech settings (one inference utterance). Device time from events around `iters` back-to-back calls after a warm-up, the two
implementations alternating in rounds so that drift hits both; the median round is reported, with the spread. One JSON line per
shape: microseconds per call for both, their ratio, the kernel's share of a 52 ms train step, and the direct sum's arithmetic
rate (subtract + FMA per term = 3 flop, terms counted from the shape).
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdvc_amd as P  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402

STEP_MS = 52.0


def fft_yin(x, sample_rate, pitch_min, pitch_max, frame_stride, threshold=0.1):
    """YIN with the difference function from an FFT autocorrelation: d[tau] = sum_{j<L-tau} u[j]^2 + sum_{j>=tau} u[j]^2 - 2 r[tau]."""
    tau_min, tau_max, stride = int(sample_rate / pitch_max), int(sample_rate / pitch_min), int(frame_stride * sample_rate)
    L, T = 2 * tau_max, x.shape[-1]
    u = F.pad(x, (L // 2, L // 2 - 1 + max(0, L - T))).unfold(-1, L, stride)
    nfft = 1 << (2 * L - 1).bit_length()
    spec = torch.fft.rfft(u, nfft)
    r = torch.fft.irfft(spec.real.square() + spec.imag.square(), nfft)[..., :tau_max]
    cs = F.pad(u.square().cumsum(-1), (1, 0))
    tau = torch.arange(tau_max, device=x.device)
    d = cs[..., L - tau] + cs[..., L:] - cs[..., tau] - 2 * r
    d1 = d[..., 1:]
    c = (d1 * tau[1:] / d1.cumsum(-1).clamp_min(1e-5))[..., tau_min:]
    n = c.shape[-1]
    idx = torch.arange(n, device=x.device)
    fb = torch.where(c < threshold, idx, n).amin(-1, keepdim=True)
    rising = F.pad(c[..., 1:] - c[..., :-1] >= 0, (0, 1), value=True)
    t = torch.where(rising & (idx >= fb), idx, n).amin(-1)
    t = torch.where((fb[..., 0] > 0) & (fb[..., 0] < n), t, 0)
    return torch.where(t > 0, sample_rate / (t + tau_min + 1).float(), 0.0)


def main():
    a = parse_args('bench_yin', iters=200, warmup=20, rounds=5)
    dev = torch.device('cuda:0')
    shapes = [('16x16000 speech', 16, 16000, 60, 500, 64 / 16000), ('16x16000 default', 16, 16000, 20, 20000, 0.01),
              ('1x71680 speech', 1, 71680, 60, 500, 64 / 16000)]
    for name, B, T, pmin, pmax, fs in shapes:
        g = torch.Generator().manual_seed(0)
        x = (0.03 * torch.randn(B, T, generator=g)).to(dev)
        kw = dict(sample_rate=16000, pitch_min=pmin, pitch_max=pmax, frame_stride=fs)
        fns = {'hip': (lambda: P.pitch.yin_f0(x, **kw), a.iters), 'torch_fft': (lambda: fft_yin(x, **kw), a.iters)}
        med, mm = measure(fns, a.warmup, a.rounds)
        tau_max, stride = int(16000 / pmin), int(fs * 16000)
        L = 2 * tau_max
        nf = (max(T, L) - 1) // stride + 1
        terms = B * nf * sum(L - tau for tau in range(tau_max))
        mh, mf = med['hip'], med['torch_fft']
        print(json.dumps({'shape': name, 'frames': B * nf, 'tau_max': tau_max, **report(med, mm, 2),
                          'fft_over_hip': round(mf / mh, 2), 'hip_share_of_52ms_step': round(mh / (STEP_MS * 1e3), 5),
                          'direct_sum_terms': terms, 'hip_tflops_direct_sum': round(3 * terms / mh / 1e6, 2)}), flush=True)


if __name__ == '__main__':
    main()
