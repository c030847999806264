"""Times the objective evaluation (td-vc-gan_amd/evaluate.py) on the GPU: `dtw` alone on mel-cepstrum-sized sequences (D = 25) and
`mcd` whole (two waveforms in, the reference's figures out), beside two comparators measured in the same session:

    torch_dtw   the same recursion in stock torch ops on the device: torch.cdist, then one step per anti-diagonal (index tensors
                built outside the timed region, cost only: no length, no path)
    host_dtw    tests/dtw_ref.py (numpy float64, cost + length + directions) on one host core, wall clock

and one `infer.convert` generator forward of the same utterances (config/conv_enc-stage1.yaml, weights as initialised), which is
what produced the files an evaluation scores.

    python tools/bench_mcd.py [--iters 20] [--warmup 3] [--rounds 5] [--torch-iters 1] [--host-rounds 3]

Shapes: 16 pairs x 4.48 s (the reference's test.max_segment: 71680 samples, 897 frames at the 5 ms hop) and 1 pair x 20 s (4001
frames). The signals are harmonic tones with vibrato, voiced throughout, so nearly every frame survives the voicing mask and the
alignment inside `mcd` is close to full size. Device time from events around `iters` back-to-back calls after a warm-up, the
implementations alternating in rounds; the median round is reported with the spread. One JSON line per shape, microseconds per call.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tdvc_amd as P  # noqa: E402
import dtw_ref as DR  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402


def torch_dtw_plan(N, M, device):
    """Per anti-diagonal the row and column indices into the padded cost array, as device tensors."""
    plan = []
    for k in range(N + M - 1):
        i = torch.arange(max(0, k - M + 1), min(k, N - 1) + 1, device=device)
        plan.append((i, k - i))
    return plan


def torch_dtw(x, y, plan):
    """C(n-1, m-1) of full pairs x [B, N, D], y [B, M, D] in stock torch ops: cdist, then one step per anti-diagonal."""
    B, N, _ = x.shape
    M = y.shape[1]
    d = torch.cdist(x, y)
    C = torch.full((B, N + 1, M + 1), float('inf'), dtype=torch.float64, device=x.device)
    C[:, 0, 0] = 0.0
    for i, j in plan:
        best = torch.minimum(torch.minimum(C[:, i, j + 1], C[:, i + 1, j]), C[:, i, j])
        C[:, i + 1, j + 1] = d[:, i, j].double() + best
    return C[:, N, M]


def host_dtw(x, y):
    """tests/dtw_ref.py on the host, the distances in row blocks so that the [n, m, D] difference array stays small."""
    out = []
    for xb, yb in zip(x, y):
        d = np.concatenate([DR.distance(xb[r:r + 128], yb) for r in range(0, len(xb), 128)])
        C, Ln, _ = DR.accumulate(d)
        out.append((C[-1, -1], Ln[-1, -1]))
    return out


def voiced_signal(rng, B, T, sr=16000):
    t = np.arange(T) / sr
    rows = []
    for _ in range(B):
        f0 = rng.uniform(100.0, 220.0) * (1 + 0.05 * np.sin(2 * np.pi * rng.uniform(0.3, 0.8) * t + rng.uniform(0, 6)))
        phase = 2 * np.pi * np.cumsum(f0) / sr
        fm = rng.uniform(500.0, 900.0) + 300.0 * np.sin(2 * np.pi * rng.uniform(1.0, 3.0) * t)
        x = sum(np.sin(h * phase) / (1 + ((h * f0 - fm) / 400.0) ** 2) for h in range(1, 16))
        rows.append(0.05 * x + 0.001 * rng.standard_normal(T))
    return torch.from_numpy(np.stack(rows).astype(np.float32))[:, None]


def main():
    a = parse_args('bench_mcd', iters=20, warmup=3, rounds=5, torch_iters=1, host_rounds=3)
    dev = torch.device('cuda:0')
    E = P.evaluate
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000)):
        rng = np.random.default_rng(B)
        test, ref = voiced_signal(rng, B, T).to(dev), voiced_signal(rng, B, T).to(dev)
        mt, mr = E.mel_cepstrum(test), E.mel_cepstrum(ref)
        N = mt.shape[1]
        plan = torch_dtw_plan(N, N, dev)
        dtw = lambda: E.dtw(mt, mr)
        dtw_path = lambda: E.dtw(mt, mr, return_path=True)
        whole = lambda: E.mcd(test, ref)
        stock = lambda: torch_dtw(mt, mr, plan)
        cepstra = lambda: (E.mel_cepstrum(test), E.mel_cepstrum(ref))
        c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
        f0 = P.track_f0(test)
        noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
        phi0 = torch.tensor([0.5], device=dev)
        forward = lambda: P.infer.convert(G, test, c_tgt, f0, noise=noise, start_phase=phi0)
        fns = {'dtw': (dtw, a.iters), 'dtw_with_path': (dtw_path, a.iters), 'mcd': (whole, a.iters), 'mel_cepstrum_x2': (cepstra, a.iters),
               'torch_dtw': (stock, a.torch_iters), 'generator_forward': (forward, max(1, a.iters // 4))}
        cost, length = dtw()
        agree = float((cost - stock()).abs().max() / cost.abs().max())
        r = whole()
        med, mm = measure(fns, a.warmup, a.rounds, once=('torch_dtw',))
        xh, yh = mt.cpu().numpy(), mr.cpu().numpy()
        host = []
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            hres = host_dtw(xh, yh)
            host.append((time.perf_counter() - t0) * 1e6)
        host_gap = max(abs(float(cost[b]) - hres[b][0]) / hres[b][0] for b in range(B))
        out = {'shape': name, 'B': B, 'frames': N, 'D': mt.shape[2], 'voiced_frames_test': [int(v) for v in r['n_test'].tolist()][:4],
               'torch_cost_rel_gap': float(f'{agree:.2e}'), 'host_cost_rel_gap': float(f'{host_gap:.2e}'),
               'path_len_equals_host': all(int(length[b]) == int(hres[b][1]) for b in range(B)), **report(med, mm, 1)}
        out['host_dtw_us'] = round(statistics.median(host), 1)
        out['host_dtw_us_min_max'] = [round(min(host), 1), round(max(host), 1)]
        out['torch_over_dtw'] = round(med['torch_dtw'] / med['dtw'], 1)
        out['host_over_dtw'] = round(out['host_dtw_us'] / med['dtw'], 1)
        out['mcd_over_generator_forward'] = round(med['mcd'] / med['generator_forward'], 3)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
