"""Times `fastdtw` (td-vc-gan_amd/evaluate.py, csrc/eval_fastdtw.hip) on mel-cepstrum sequences (D = 25, radius 1) beside `dtw`, the
exact programme, in the same session, `mcd(align='fastdtw')` whole beside `mcd()` whole, and the numpy restatement
tests/fastdtw_ref.py on one host core (wall clock).

    python tools/bench_fastdtw.py [--iters 20] [--warmup 3] [--rounds 5] [--host-rounds 1]

Shapes: 16 pairs x 4.48 s (897 frames at the 5 ms hop), 1 pair x 20 s (4001 frames) and 1 pair x 80 s (16001 frames, beyond what `dtw`
and `mcd()` take: only the FastDTW routes are timed there). The signals are tools/bench_mcd.py's voiced tones. Device time from
events around `iters` back-to-back calls after a warm-up, the implementations alternating in rounds; the median round is reported
with the spread. One JSON line per shape, microseconds per call.
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
import fastdtw_ref as FR  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402
from bench_mcd import voiced_signal  # noqa: E402


def main():
    a = parse_args('bench_fastdtw', iters=20, warmup=3, rounds=5, host_rounds=1)
    dev = torch.device('cuda:0')
    E = P.evaluate
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000), ('1 x 80 s', 1, 1280000)):
        rng = np.random.default_rng(B)
        test, ref = voiced_signal(rng, B, T).to(dev), voiced_signal(rng, B, T).to(dev)
        mt, mr = E.mel_cepstrum(test), E.mel_cepstrum(ref)
        N = mt.shape[1]
        exact_fits = N <= E.DTW_MAX_LEN
        fns = {'fastdtw': (lambda: E.fastdtw(mt, mr), a.iters), 'fastdtw_with_path': (lambda: E.fastdtw(mt, mr, return_path=True), a.iters),
               'mcd_fastdtw': (lambda: E.mcd(test, ref, align='fastdtw'), a.iters)}
        if exact_fits:
            fns.update({'dtw': (lambda: E.dtw(mt, mr), a.iters), 'mcd': (lambda: E.mcd(test, ref), a.iters)})
        cost, length = E.fastdtw(mt, mr)
        r = E.mcd(test, ref, align='fastdtw')
        med, mm = measure(fns, a.warmup, a.rounds)
        xh, yh = mt.cpu().numpy(), mr.cpu().numpy()
        host = []
        for _ in range(a.host_rounds):
            t0 = time.perf_counter()
            hres = [FR.fastdtw(xb, yb, 1, 'l2') for xb, yb in zip(xh, yh)]
            host.append((time.perf_counter() - t0) * 1e6)
        out = {'shape': name, 'B': B, 'frames': N, 'D': mt.shape[2], 'radius': 1, 'levels': len(hres[0]['levels']),
               'window_cells_all_levels': [sum(lv['cells'] for lv in h['levels']) for h in hres][:4],
               'voiced_frames_test': [int(v) for v in r['n_test'].tolist()][:4],
               'host_cost_rel_gap': float(f'{max(abs(float(cost[b]) - hres[b]["cost"]) / hres[b]["cost"] for b in range(B)):.2e}'),
               'path_len_equals_host': all(int(length[b]) == hres[b]['length'] for b in range(B)), **report(med, mm, 1)}
        out['host_fastdtw_us'] = round(statistics.median(host), 1)
        out['host_over_fastdtw'] = round(out['host_fastdtw_us'] / med['fastdtw'], 1)
        if exact_fits:
            exact = E.dtw(mt, mr)[0]
            out['fastdtw_cost_over_exact'] = [round(float(v), 6) for v in (cost / exact).tolist()][:4]
            out['dtw_over_fastdtw'] = round(med['dtw'] / med['fastdtw'], 2)
            out['mcd_over_mcd_fastdtw'] = round(med['mcd'] / med['mcd_fastdtw'], 2)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
