"""Times the soft-YIN backward (tdvc_yin_soft_bwd) and the whole lambda_f0 term (losses.f0_yin_loss, forward + backward) on the GPU
beside the forward alone (tdvc_yin_f0, soft search) of the same run.

    python tools/bench_yin_bwd.py [--iters 200] [--warmup 20] [--rounds 5]

Shapes: 16 x 16000 with speech settings (60-500 Hz, hop 64) and with `estimate`'s defaults (20-20000 Hz, 10 ms), and 1 x 71680
with speech settings. The signal is a harmonic tone on a slowly moving 100-250 Hz contour with a little noise, so that nearly every
frame is on and pays for the full backward (a frame that is off, or has no upstream gradient, leaves the kernel at once); the
share of frames that are on is reported. Device time from events around `iters` back-to-back calls after a warm-up, the variants
alternating in rounds so that drift hits all of them; the median round is reported, with the spread. One JSON line per shape:
microseconds for the forward, for the backward's two launches (upstream gradient of ones), their ratio (target <= 4), for
forward + backward of f0_yin_loss, and that term's share of a 52 ms train step (target < 1 %; speech hop only: the loss works on the
[B, 1, T // hop + 1] track layout).
"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdvc_amd as P  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402

STEP_MS = 52.0


def tone(B, T, sr=16000, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)
    f = 175.0 + 75.0 * torch.sin(2 * math.pi * t[None] / sr * torch.rand(B, 1, generator=g, dtype=torch.float64) + 6.28 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    ph = 2 * math.pi * f.cumsum(-1) / sr
    x = sum(torch.sin(h * ph) / h for h in range(1, 5)) + 0.01 * torch.randn(B, T, generator=g, dtype=torch.float64)
    return (0.03 * x).float()


def main():
    a = parse_args('bench_yin_bwd', iters=200, warmup=20, rounds=5)
    dev = torch.device('cuda:0')
    L, lib = P._lib, P._lib.lib()
    shapes = [('16x16000 speech', 16, 16000, 60, 500, 64), ('16x16000 default', 16, 16000, 20, 20000, 160), ('1x71680 speech', 1, 71680, 60, 500, 64)]
    for name, B, T, pmin, pmax, stride in shapes:
        x = tone(B, T).to(dev)
        sr = 16000
        tau_min, tau_max = int(sr / pmax), int(sr / pmin)
        kw = dict(sample_rate=sr, pitch_min=pmin, pitch_max=pmax, frame_stride=stride / sr)
        f0 = P.pitch.yin_f0(x, soft=True, **kw)
        nf = f0.shape[-1]
        gy = torch.ones(B, nf, device=dev)
        dx = torch.empty(B, T, device=dev)
        nb = lib.tdvc_yin_soft_bwd_workspace(B, T, tau_max, stride)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        fwd = lambda: P.pitch.yin_f0(x, soft=True, **kw)
        bwd = lambda: L.check(lib.tdvc_yin_soft_bwd(x.data_ptr(), T, B, T, tau_min, tau_max, stride, 0.1, float(sr), gy.data_ptr(), dx.data_ptr(),
                                                    ws.data_ptr(), nb, st))
        variants = {'fwd': (fwd, a.iters), 'bwd': (bwd, a.iters)}
        if stride == 64:
            xr = x[:, None].clone().requires_grad_()
            tgt = torch.full((B, 1, T // 64 + 1), 150.0, device=dev)

            def term():
                xr.grad = None
                P.losses.f0_yin_loss(xr, tgt, pitch_min=pmin, pitch_max=pmax).backward()
            variants['term'] = (term, a.iters)
        med, mm = measure(variants, a.warmup, a.rounds)
        out = {'shape': name, 'frames': B * nf, 'tau_max': tau_max, 'frames_on': round(float((f0 > 0).float().mean()), 3),
               'workspace_mb': round(nb / 1e6, 2), **report(med, mm, 2, ('fwd', 'bwd')), 'bwd_over_fwd': round(med['bwd'] / med['fwd'], 2)}
        if 'term' in med:
            out.update({'term_fwd_bwd_us': round(med['term'], 2), 'term_us_min_max': [round(v, 2) for v in mm['term']],
                        'term_share_of_52ms_step': round(med['term'] / (STEP_MS * 1e3), 5)})
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
