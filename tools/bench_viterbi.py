"""Times the Viterbi-decoded F0 track (tdvc_viterbi_path, csrc/pitch_viterbi.hip) on the GPU: the decode alone on the CMDF of the
shape, and the whole call (`track_f0(decoder='viterbi')`, or `yin_f0(decoder='viterbi')` for `estimate`'s default range), each
beside two things measured in the same session: the per-frame tracker as it is without the decoder, and the same recursion
written frame by frame with stock torch ops (dense n x n transition, max over predecessors, renormalisation, back-pointer gather),
which is what a user would otherwise run on the device.

    python tools/bench_viterbi.py [--iters 50] [--warmup 5] [--rounds 5] [--torch-iters 2]

Shapes: 16 x 16000 with speech settings (60-500 Hz, hop 64: n = 233, W = 64, F = 250) and with `estimate`'s defaults (20-20000 Hz,
10 ms: n = 799, W = 194), and 1 x 71680 with speech settings (one inference utterance, F = 1120). At the last shape one
`infer.convert` generator forward of the same utterance (config/conv_enc-stage1.yaml, weights as initialised) is timed too: the
decoded track has to cost less than that, or inference time doubles. Device time from events around `iters` back-to-back calls
after a warm-up, the implementations alternating in rounds so that drift hits all of them; the median round is reported with
the spread. One JSON line per shape, microseconds per call.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdvc_amd as P  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402


def torch_viterbi(x, logw, lo, scale, prior, jump):
    """The recursion of include/tdvc.h in stock torch ops, frame by frame. x [B, F, n] -> path [B, F]."""
    B, F, n = x.shape
    W = logw.shape[1]
    t = torch.full((n, n), -jump, device=x.device)
    t.scatter_(1, (lo[:, None] + torch.arange(W, device=x.device)[None, :]).long(), logw.clamp_min(-jump))
    obs = scale * x + prior
    d = obs[:, 0]
    bp = torch.empty(B, F, n, dtype=torch.int64, device=x.device)
    for f in range(1, F):
        best, bp[:, f] = (d[:, None, :] + t[None]).max(-1)
        d = obs[:, f] + best
        d = d - d.amax(-1, keepdim=True)
    path = torch.empty(B, F, dtype=torch.int64, device=x.device)
    path[:, F - 1] = d.argmax(-1)
    for f in range(F - 1, 0, -1):
        path[:, f - 1] = bp[:, f].gather(1, path[:, f, None])[:, 0]
    return path


def main():
    a = parse_args('bench_viterbi', iters=50, warmup=5, rounds=5, torch_iters=2)
    dev = torch.device('cuda:0')
    Pt = P.pitch
    shapes = [('16x16000 speech', 16, 16000, 60, 500, 64), ('16x16000 default', 16, 16000, 20, 20000, 160), ('1x71680 speech', 1, 71680, 60, 500, 64)]
    for name, B, T, pmin, pmax, hop in shapes:
        g = torch.Generator().manual_seed(0)
        x = (0.03 * torch.randn(B, 1, T, generator=g)).to(dev)
        speech = pmax == 500
        tau_min, tau_max = int(16000 / pmax), int(16000 / pmin)
        if speech:
            kw = dict(hop=hop, sample_rate=16000, pitch_min=pmin, pitch_max=pmax)
            plain = lambda: Pt.track_f0(x, **kw)
            whole = lambda: Pt.track_f0(x, decoder='viterbi', **kw)
        else:
            kw = dict(sample_rate=16000, pitch_min=pmin, pitch_max=pmax, frame_stride=hop / 16000)
            plain = lambda: Pt.yin_f0(x[:, 0], **kw)
            whole = lambda: Pt.yin_f0(x[:, 0], decoder='viterbi', **kw)
        _, cmdf = Pt.yin_f0(x[:, 0], 16000, pmin, pmax, hop / 16000, return_cmdf=True)
        n = cmdf.shape[-1]
        logw, lo = Pt.viterbi_transition(tau_min, tau_max)
        prior = torch.from_numpy((-np.log2((np.arange(n) + tau_min + 1.0) / (tau_min + 1))).astype(np.float32)).to(dev)
        decode = lambda: Pt.viterbi_path(cmdf, logw, lo, scale=-100.0, prior=prior, jump=16.0)
        stock = lambda: torch_viterbi(cmdf, logw, lo, -100.0, prior, 16.0)
        fns = {'decode': (decode, a.iters), 'track_viterbi': (whole, a.iters), 'track_plain': (plain, a.iters), 'torch_decode': (stock, a.torch_iters)}
        agree = float((decode() == stock()).float().mean())
        if name.startswith('1x'):
            hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
            G = P.infer.build_generator(hp.model.generator, 16, dev)
            c_tgt = torch.zeros(1, 16, device=dev); c_tgt[0, 3] = 1.0
            f0 = whole()
            noise = (torch.randn(1, 1, T, device=dev), torch.randn(1, 1, T, device=dev))
            phi0 = torch.tensor([0.5], device=dev)
            fns['generator_forward'] = (lambda: P.infer.convert(G, x, c_tgt, f0, noise=noise, start_phase=phi0), a.iters)
        med, mm = measure(fns, a.warmup, a.rounds, once=('torch_decode',))
        out = {'shape': name, 'B': B, 'frames': cmdf.shape[1], 'n': n, 'W': logw.shape[1], 'torch_path_agreement': round(agree, 4),
               **report(med, mm, 1)}
        out['decode_us_per_frame'] = round(med['decode'] / cmdf.shape[1], 3)
        out['viterbi_over_plain'] = round(med['track_viterbi'] / med['track_plain'], 2)
        out['torch_over_decode'] = round(med['torch_decode'] / med['decode'], 1)
        if 'generator_forward' in med:
            out['track_viterbi_over_generator_forward'] = round(med['track_viterbi'] / med['generator_forward'], 3)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
