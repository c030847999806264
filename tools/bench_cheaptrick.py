"""Times WORLD's CheapTrick spectral envelope on the GPU (td-vc-gan_amd/evaluate.py; csrc/eval_cheaptrick.hip), per call:

    cheaptrick            evaluate.cheaptrick alone (envelope out)
    mc_fused              mel_cepstrum(envelope='cheaptrick') with a given F0 track: the same launch, mel-cepstra out, no envelope stored
    mcd_cheaptrick        mcd(envelope='cheaptrick') whole: two waveforms in, YIN, two envelopes, the alignment

beside comparators measured in the same session:

    torch_cheaptrick      the same algorithm in stock torch float64 ops on the device (`torch_cheaptrick` below: gathered windows of
                          the fixed width N - 3 with a mask, torch.fft.rfft, cumsum, gathers for the two interpolations, two more
                          transforms); its envelope is compared with the kernel's
    mc_stft, mcd_stft     mel_cepstrum / mcd with the default STFT envelope (what the package computed before this envelope existed)
    generator_forward     one infer.convert forward of the same audio (config/conv_enc-stage1.yaml, weights as initialised)

    python tools/bench_cheaptrick.py [--iters 20] [--warmup 3] [--rounds 5] [--torch-iters 3]

Shapes: 16 x 4.48 s (71680 samples, 896 frames at the 5 ms hop) and 1 x 20 s (4000 frames) at 16 kHz, n_fft = 1024; the signals of
tools/bench_mcd.py. Device time from events around `iters` back-to-back calls after a warm-up, the implementations alternating in
rounds; the median round is reported with the spread. One JSON line per shape, microseconds per call.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from _timing import measure, parse_args, report  # noqa: E402


def _lin(y, p):
    j = p.floor().long().clamp(0, y.shape[-1] - 2)
    a, b = y.gather(-1, j), y.gather(-1, j + 1)
    return a + (b - a) * (p - j)


def torch_cheaptrick(x, f0, fs, n_fft, hop, q1=-0.15, floor=1e-16):
    """include/tdvc.h's definition in stock torch float64 ops: x [B, T], f0 [B, F] -> (env float64 [B, F, h + 1], c [B, F, h + 1])."""
    B, T = x.shape
    F = f0.shape[1]
    N, h, df, dev = n_fft, n_fft // 2, fs / n_fft, x.device
    f = f0.double()
    f = torch.where(torch.isfinite(f) & (f > 3.0 * fs / (N - 3.0)) & (f <= fs / 4.0), f, torch.full_like(f, 500.0))[..., None]      # [B, F, 1]
    half = torch.floor(1.5 * fs / f + 0.5)
    k = torch.arange(-(N - 4) // 2, (N - 4) // 2 + 1, device=dev, dtype=torch.float64)                                    # N - 3 taps
    inside = k.abs() <= half
    pos = torch.arange(F, device=dev)[None, :, None] * hop
    idx = (pos + k.long()).clamp(0, T - 1).expand(B, F, -1)
    seg = x.double()[:, None, :].expand(B, F, T).gather(2, idx)
    w = (0.5 * torch.cos(math.pi * f * k / (1.5 * fs)) + 0.5) * inside
    w = w / (w * w).sum(-1, keepdim=True).sqrt()
    s = seg * w
    s = s - w * (s.sum(-1, keepdim=True) / w.sum(-1, keepdim=True))
    P = torch.fft.rfft(s, N).abs() ** 2                                                                                     # a shift of the window does not move |.|
    i = torch.arange(h + 1, device=dev, dtype=torch.float64)
    P = P + torch.where(i < 1 + torch.floor(f * N / fs), _lin(P, ((f - i * df) / df).clamp(min=0.0)), torch.zeros_like(P))
    wd = 2.0 * f / 3.0
    bd = torch.floor(wd * N / fs).long() + 1
    j = torch.arange(h + 2 * (N // 6 + 1) + 1, device=dev)
    src = (j - bd).abs()
    src = torch.where(src > h, 2 * h - src, src).clamp(0, h)
    m = torch.where(j <= h + 2 * bd, P.gather(-1, src), torch.zeros((), dtype=torch.float64, device=dev))
    seg = torch.cumsum(m * df, -1)
    off = wd / (2.0 * df)
    S = (_lin(seg, i + off + bd - 0.5) - _lin(seg, i - off + bd - 0.5)) / wd
    L = torch.log(S.clamp(min=floor) + 2.2e-16)
    C = torch.fft.rfft(torch.cat([L, L[..., 1:h].flip(-1)], -1)).real
    q = i / fs
    sl = torch.where(i == 0, torch.ones_like(f * q), torch.sin(math.pi * f * q) / (math.pi * f * q).clamp(min=1e-300))
    c = C * sl * ((1 - 2 * q1) + 2 * q1 * torch.cos(2 * math.pi * f * q)) / N
    return torch.exp(torch.fft.rfft(torch.cat([c, c[..., 1:h].flip(-1)], -1)).real), c


def main():
    a = parse_args('bench_cheaptrick', iters=20, warmup=3, rounds=5, torch_iters=3)
    import tdvc_amd as P
    from bench_mcd import voiced_signal
    dev = torch.device('cuda:0')
    E = P.evaluate
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    fs, n_fft, hop = 16000, 1024, 80
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000)):
        rng = np.random.default_rng(B)
        test, ref = voiced_signal(rng, B, T).to(dev), voiced_signal(rng, B, T).to(dev)
        f0 = P.yin_f0(test[:, 0], fs, pitch_min=50, pitch_max=500, frame_stride=hop / fs)
        c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
        f0_conv = P.track_f0(test)
        noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
        phi0 = torch.tensor([0.5], device=dev)
        stock = lambda: torch_cheaptrick(test[:, 0], f0, fs, n_fft, hop)
        fns = {'cheaptrick': (lambda: E.cheaptrick(test, f0, fs, n_fft), a.iters),
               'mc_fused': (lambda: E.mel_cepstrum(test, fs, n_fft, hop, envelope='cheaptrick', f0=f0), a.iters),
               'mcd_cheaptrick': (lambda: E.mcd(test, ref, envelope='cheaptrick'), a.iters),
               'torch_cheaptrick': (stock, a.torch_iters),
               'mc_stft': (lambda: E.mel_cepstrum(test, fs, n_fft, hop), a.iters),
               'mcd_stft': (lambda: E.mcd(test, ref), a.iters),
               'generator_forward': (lambda: P.infer.convert(G, test, c_tgt, f0_conv, noise=noise, start_phase=phi0), max(1, a.iters // 4))}
        env = E.cheaptrick(test, f0, fs, n_fft).double()
        gap = float(((env - stock()[0]).abs() / env).max())
        r_ct, r_st = E.mcd(test, ref, envelope='cheaptrick'), E.mcd(test, ref)
        med, mm = measure(fns, a.warmup, a.rounds, once=('torch_cheaptrick',))
        out = {'shape': name, 'B': B, 'frames': f0.shape[1], 'n_fft': n_fft, 'voiced_frames': [int(v) for v in (f0 > 0).sum(1).tolist()][:4],
               'torch_env_rel_gap': float(f'{gap:.2e}'), 'mcd_cheaptrick': [round(float(v), 4) for v in r_ct['mcd'].tolist()][:4],
               'mcd_stft': [round(float(v), 4) for v in r_st['mcd'].tolist()][:4], **report(med, mm, 1)}
        out['us_per_frame'] = round(med['cheaptrick'] / (B * f0.shape[1]), 3)
        out['torch_over_cheaptrick'] = round(med['torch_cheaptrick'] / med['cheaptrick'], 1)
        out['mc_fused_over_mc_stft'] = round(med['mc_fused'] / med['mc_stft'], 2)
        out['mcd_cheaptrick_over_mcd_stft'] = round(med['mcd_cheaptrick'] / med['mcd_stft'], 2)
        out['mcd_cheaptrick_over_generator_forward'] = round(med['mcd_cheaptrick'] / med['generator_forward'], 3)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
