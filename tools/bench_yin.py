"""Times tdvc_yin_f0 (pitch.yin_f0, hard search) on the GPU beside the FFT formulation of the same tracker written with stock
torch ops, which is what a user would otherwise run on the device.

    python tools/bench_yin.py [--iters 200] [--warmup 20]

Shapes: 16 x 16000 with speech settings (60-500 Hz, hop 64) and with `estimate`'s defaults (20-20000 Hz, 10 ms), and 1 x 71680
with speech settings (one inference utterance). Device time from events around `iters` back-to-back calls after a warm-up, the two
implementations alternating in rounds so that drift hits both; the median round is reported, with the spread. One JSON line per
shape: microseconds per call for both, their ratio, the kernel's share of a 52 ms train step, and the direct sum's arithmetic
rate (subtract + FMA per term = 3 flop, terms counted from the shape).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdvc_amd as P  # noqa: E402

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


def time_calls(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_yin: needs a GPU (a CPU timing says nothing about the kernel)')
    dev = torch.device('cuda:0')
    shapes = [('16x16000 speech', 16, 16000, 60, 500, 64 / 16000), ('16x16000 default', 16, 16000, 20, 20000, 0.01),
              ('1x71680 speech', 1, 71680, 60, 500, 64 / 16000)]
    for name, B, T, pmin, pmax, fs in shapes:
        g = torch.Generator().manual_seed(0)
        x = (0.03 * torch.randn(B, T, generator=g)).to(dev)
        kw = dict(sample_rate=16000, pitch_min=pmin, pitch_max=pmax, frame_stride=fs)
        hip = lambda: P.pitch.yin_f0(x, **kw)
        fft = lambda: fft_yin(x, **kw)
        for _ in range(a.warmup):
            hip(); fft()
        torch.cuda.synchronize()
        th, tf = [], []
        for _ in range(a.rounds):
            th.append(time_calls(hip, a.iters))
            tf.append(time_calls(fft, a.iters))
        tau_max, stride = int(16000 / pmin), int(fs * 16000)
        L = 2 * tau_max
        nf = (max(T, L) - 1) // stride + 1
        terms = B * nf * sum(L - tau for tau in range(tau_max))
        mh, mf = statistics.median(th), statistics.median(tf)
        print(json.dumps({'shape': name, 'frames': B * nf, 'tau_max': tau_max, 'hip_us': round(mh, 2), 'hip_us_min_max': [round(min(th), 2), round(max(th), 2)],
                          'torch_fft_us': round(mf, 2), 'torch_fft_us_min_max': [round(min(tf), 2), round(max(tf), 2)],
                          'fft_over_hip': round(mf / mh, 2), 'hip_share_of_52ms_step': round(mh / (STEP_MS * 1e3), 5),
                          'direct_sum_terms': terms, 'hip_tflops_direct_sum': round(3 * terms / mh / 1e6, 2)}), flush=True)


if __name__ == '__main__':
    main()
