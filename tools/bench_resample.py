"""Times resample.resample (tdvc_resample) and resample.load_segments (tdvc_resample + the start draw + tdvc_segment) on the GPU beside
the same polyphase bank applied with stock torch ops on the same GPU: float64 F.conv1d with stride M, one filter per phase, the L
phase outputs interleaved (what one would write without a kernel), and beside the same kernel reading a phase-major bank (a
per-lane gather instead of the product's coalesced tap-major layout).

    python tools/bench_resample.py [--iters 100] [--warmup 10] [--rounds 5] [--step-ms MS] [--out profiles/resample_bench.txt]

Shapes: 16 rows x 3 s of 48 kHz -> 16 kHz, 16 rows x 3 s of 44.1 kHz -> 16 kHz, 1 row x 10 s of 48 kHz -> 16 kHz. Device time from
events around `iters` back-to-back calls after a warm-up; the median of `rounds` such measurements is reported with the minimum and
maximum. The variants are timed interleaved, round by round, in one process. --step-ms is the train step to relate the
figures to: measure it with bench.py in the same session and pass its ms_per_step (without it no share is reported). One JSON line
per shape, also written to --out.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tdvc_amd as P  # noqa: E402
import resample_ref as RR  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402

SR = 16000


def torch_route(x, bk, n_out):
    """The bank with stock ops: x [B, T] fp32 -> float64 conv1d per phase (stride M), interleaved -> fp32 [B, n_out]. Full-length
    rows only (no per-row lengths), which is all the timing needs."""
    bank = torch.tensor(bk.bank).to(x.device)      # [L, W]
    Lp, W = bank.shape
    per_phase = -(-n_out // Lp)

    def run():
        xd = x.double()
        cols = []
        for p in range(Lp):          # output t = p_idx + Lp * k with phase (t*M) % Lp: one stride-M conv per residue of t
            t0 = p
            n0, ph = divmod(t0 * bk.M, Lp)
            lo = n0 - bk.left + 1
            need = lo + (per_phase - 1) * bk.M + W
            xp = F.pad(xd, (max(0, -lo), max(0, need - xd.shape[1])))[:, max(0, lo):]
            cols.append(F.conv1d(xp[:, None], bank[ph][None, None], stride=bk.M)[:, 0, :per_phase])
        return torch.stack(cols, 2).reshape(x.shape[0], -1)[:, :n_out].float()
    return run


def gather_route(x, bk, lengths, n_out):
    """tdvc_resample with the bank phase-major, bank[q][j] (tap stride 1, column stride W): every lane walks its own row, the layout
    the product does not use. Same kernel, same arithmetic, only the weight addresses differ."""
    R, lib = P.resample, P._lib.lib()
    dev, (B, T) = x.device, x.shape
    order = (np.arange(bk.L, dtype=np.int64) * bk.M) % bk.L
    bank = torch.tensor(bk.bank[order]).to(dev)      # [L, W]
    W = bank.shape[1]
    n_in_d, n_out_d = R._device_lengths(lengths, dev), R._device_lengths([n_out] * B, dev)
    nbytes = lib.tdvc_resample_workspace(B, n_out)

    def run():
        y = torch.empty(B, n_out, dtype=torch.float32, device=dev)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        P._lib.check(lib.tdvc_resample(x.data_ptr(), x.stride(0), n_in_d.data_ptr(), n_out_d.data_ptr(), B, T, n_out, bank.data_ptr(), 1, W,
                                       bk.L, bk.M, W, bk.left, y.data_ptr(), n_out, ws.data_ptr(), nbytes,
                                       torch.cuda.current_stream(dev).cuda_stream))
        return y
    return run


def main():
    a = parse_args('bench_resample', iters=100, warmup=10, rounds=5, torch_iters=5, out=os.path.join(ROOT, 'profiles', 'resample_bench.txt'),
                   more=lambda ap: ap.add_argument('--step-ms', type=float, default=None,
                                                   help='ms per train step from bench.py, measured in the same session'))
    dev = torch.device('cuda:0')
    lines = []
    for name, B, sr, secs in (('16x3s_48k', 16, 48000, 3.0), ('16x3s_44k1', 16, 44100, 3.0), ('1x10s_48k', 1, 48000, 10.0)):
        T = int(sr * secs)
        rng = np.random.default_rng(0)
        x = torch.from_numpy(np.stack([RR.make_signal(rng, T, sr) for _ in range(B)])).to(dev)
        lengths = [T] * B
        bk = P.resample.resample_bank(sr, SR)
        n_out = P.resample.num_out(T, sr, SR)
        gen = torch.Generator(device=dev).manual_seed(0)
        res = lambda: P.resample(x, sr, SR, lengths=lengths)
        seg = lambda: P.load_segments(x, lengths, sr, sample_rate=SR, generator=gen)
        stock = torch_route(x, bk, n_out)
        gather = gather_route(x, bk, lengths, n_out)
        y = res()[0]
        assert torch.equal(gather(), y)
        diff = float((stock() - y).abs().max() / y.abs().max())          # the two routes compute the same thing
        fns = {'resample': (res, a.iters), 'load_segments': (seg, a.iters), 'torch_fp64_conv1d': (stock, a.torch_iters),
               'resample_phase_major_bank': (gather, a.iters)}
        med, mm = measure(fns, a.warmup, a.rounds, once=('torch_fp64_conv1d',))
        mr, ms_, mt = med['resample'], med['load_segments'], med['torch_fp64_conv1d']
        rec = {'shape': name, 'L': bk.L, 'M': bk.M, 'W': int(bk.bank.shape[1]), **report(med, mm, 2, ('resample', 'load_segments', 'torch_fp64_conv1d')),
               'torch_over_hip': round(mt / mr, 2), 'torch_vs_hip_max_rel_diff': diff, **report(med, mm, 2, ('resample_phase_major_bank',)),
               'audio_s_per_s': round(B * secs / (ms_ * 1e-6), 1)}
        if a.step_ms:
            rec.update({'step_ms': a.step_ms, 'resample_share_of_step': round(mr / (a.step_ms * 1e3), 5),
                        'load_segments_share_of_step': round(ms_ / (a.step_ms * 1e3), 5)})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_resample.py --iters {a.iters} --warmup {a.warmup} --rounds {a.rounds} --torch-iters {a.torch_iters}'
                f'{f" --step-ms {a.step_ms}" if a.step_ms else ""} on {torch.cuda.get_device_name(0)}\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
