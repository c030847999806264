"""Times corrupt.random_eq (tdvc_peq_sos + tdvc_sos_filter, RMS-matched) on the GPU beside the reference's own route on this host:
params2sos, float64 scipy.signal.sosfilt and eq_rms_signals per row on the CPU (restated with numpy / scipy, one process, as one
DataLoader worker runs it), plus the host-to-device copy of the result.

    python tools/bench_corrupt.py [--iters 200] [--warmup 20] [--rounds 5] [--out profiles/corrupt_bench.txt]

Shapes: 16 x 16000 (one training batch) and 1 x 71680 (one inference-length utterance). Device time from events around `iters`
back-to-back calls after a warm-up; the median of `rounds` such measurements is reported with the spread. The draws are made once
and passed in, so the device figure is the two launches and their glue ops (the default path adds two torch.rand calls). The CPU
route is timed with a wall clock over whole batches, median of `rounds`. One JSON line per shape, also appended to --out:
microseconds per call for both, their ratio, the device call's share of a 52 ms train step, and the audio seconds per second of
one GPU / one CPU worker.
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
import peq_ref as PR  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402

STEP_MS = 52.0
SR = 16000


def cpu_route(x, G, z, dev):
    """The reference's route for one batch: coefficients, float64 sosfilt and RMS match row by row, then the copy to the device."""
    import scipy.signal as sps
    out = np.empty_like(x)
    for b in range(len(x)):
        sos = PR.peq_sos(G[b], PR.q_of_z(z[b]))
        y = sps.sosfilt(sos, x[b].astype(np.float64))
        out[b] = PR.match_rms(y, x[b])
    t = torch.from_numpy(out).to(dev)
    torch.cuda.synchronize()
    return t


def main():
    a = parse_args('bench_corrupt', iters=200, warmup=20, rounds=5, out=os.path.join(ROOT, 'profiles', 'corrupt_bench.txt'))
    try:
        import scipy.signal  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    dev = torch.device('cuda:0')
    lines = []
    for name, B, T in (('16x16000', 16, 16000), ('1x71680', 1, 71680)):
        rng = np.random.default_rng(0)
        x = np.stack([PR.make_signal(rng, T, SR) for _ in range(B)])
        G, z = rng.uniform(-12, 12, (B, 10)), rng.uniform(0, 1, (B, 10))
        xd, Gd, zd = torch.from_numpy(x).to(dev), torch.from_numpy(G).to(dev), torch.from_numpy(z).to(dev)
        sos = P.corrupt.peq_sos(Gd, torch.from_numpy(PR.q_of_z(z)).to(dev))
        fns = {'random_eq': (lambda: P.corrupt.random_eq(xd, gains_db=Gd, z=zd), a.iters),
               'sos_filter': (lambda: P.corrupt.sos_filter(xd, sos, match_rms=True), a.iters)}
        med, mm = measure(fns, a.warmup, a.rounds)
        mf = med['random_eq']
        rec = {'shape': name, **report(med, mm, 2), 'share_of_52ms_step': round(mf / (STEP_MS * 1e3), 5), 'gpu_audio_s_per_s': round(B * T / SR / (mf * 1e-6), 1)}
        if have_scipy:
            cpu_route(x, G, z, dev)
            tc = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                cpu_route(x, G, z, dev)
                tc.append((time.perf_counter() - t0) * 1e6)
            mc = statistics.median(tc)
            rec.update({'cpu_scipy_us': round(mc, 1), 'cpu_scipy_us_min_max': [round(min(tc), 1), round(max(tc), 1)],
                        'cpu_over_gpu': round(mc / mf, 1), 'cpu_worker_audio_s_per_s': round(B * T / SR / (mc * 1e-6), 1)})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_corrupt.py --iters {a.iters} --warmup {a.warmup} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
