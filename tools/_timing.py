"""What the operator benchmarks (bench_yin, bench_yin_bwd, bench_viterbi, bench_corrupt, bench_resample, bench_mcd, bench_cheaptrick)
share: the command line, the exit without a GPU, and the measurement. Device time from events around `iters` back-to-back calls
after a warm-up, the implementations alternating in rounds so that drift hits all of them; the median round is reported, with
the spread."""
import argparse
import statistics

import torch


def parse_args(who, iters, warmup, rounds, torch_iters=None, host_rounds=None, out=None, more=None):
    """--iters / --warmup / --rounds with the tool's defaults; --torch-iters, --host-rounds and --out where a default is given;
    more(parser) adds a tool's own arguments. Exits when there is no GPU."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=iters)
    ap.add_argument('--warmup', type=int, default=warmup)
    ap.add_argument('--rounds', type=int, default=rounds)
    if torch_iters is not None:
        ap.add_argument('--torch-iters', type=int, default=torch_iters, help='calls per round of the stock-torch route')
    if host_rounds is not None:
        ap.add_argument('--host-rounds', type=int, default=host_rounds)
    if out is not None:
        ap.add_argument('--out', default=out)
    if more is not None:
        more(ap)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f'{who}: needs a GPU (a CPU timing says nothing about the kernel)')
    return a


def time_calls(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # microseconds per call


def measure(fns, warmup, rounds, once=()):
    """fns: name -> (fn, iters). `warmup` calls of each (one call for the names in `once`: the slow stock-torch routes), then
    `rounds` rounds that time every fn in turn, microseconds per call -> (med: name -> median round, mm: name -> [min, max])."""
    for k, (fn, _) in fns.items():
        for _ in range(1 if k in once else warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (fn, iters) in fns.items():
            times[k].append(time_calls(fn, iters))
    return {k: statistics.median(v) for k, v in times.items()}, {k: [min(v), max(v)] for k, v in times.items()}


def report(med, mm, digits, names=None):
    """{'<name>_us': median, '<name>_us_min_max': [min, max]} rounded, for `names` (default: all, in order)."""
    out = {}
    for k in names or med:
        out[f'{k}_us'] = round(med[k], digits)
        out[f'{k}_us_min_max'] = [round(v, digits) for v in mm[k]]
    return out
