"""Times WORLD's DIO and StoneMask on the GPU (td-vc-gan_amd/pitch.py; csrc/pitch_dio.hip), per call:

    dio                   pitch.dio alone (seven launches: tables, row mean, low-cut, the band filter twice, candidates, the fix steps)
    stonemask             pitch.stonemask on DIO's track (one launch, a block per frame)
    world_f0              stonemask(dio(x)): the F0 step of the reference's world_analyze
    mcd_world             mcd(f0_method='dio', envelope='cheaptrick', align='fastdtw') whole: two waveforms in, the reference's pipeline

beside comparators measured in the same session:

    yin_f0                pitch.yin_f0 at the same settings (50..500 Hz, 5 ms hop): what `mcd` tracks F0 with by default
    torch_fir_crossings   DIO's FIR and zero-crossing front end in stock torch float64 ops on the device (`torch_front_end` below:
                          conv1d for the low-cut and the seven Nuttall filters, the four crossing masks, their fine positions and
                          running counts); no interpolation, no candidates, no fix steps: less than `dio` does
    numpy_world_f0_ms     the float64 restatement tests/dio_ref.py (dio + stonemask) of ONE row on one host core, milliseconds, once
    mcd_yin               mcd(envelope='cheaptrick', align='fastdtw') with the default YIN track
    generator_forward     one infer.convert forward of the same audio (config/conv_enc-stage1.yaml, weights as initialised)

    python tools/bench_dio.py [--iters 20] [--warmup 3] [--rounds 5] [--torch-iters 3] [--out profiles/dio_bench.txt]

Shapes: 16 x 4.48 s (71680 samples, 897 frames at the 5 ms hop) and 1 x 20 s (4001 frames) at 16 kHz; the signals of
tools/bench_mcd.py. Device time from events around `iters` back-to-back calls after a warm-up, the implementations alternating in
rounds; the median round is reported with the spread. One JSON line per shape, microseconds per call, printed and written to --out.
"""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _timing import measure, parse_args, report  # noqa: E402


def torch_front_end(x, fs, f0_floor=50.0, f0_ceil=500.0, cpo=2.0):
    """x [B, T] -> the four crossing masks' running counts and fine positions per band, float64 on the device."""
    conv = torch.nn.functional.conv1d
    x = x.double()
    y = (x - x.mean(1, keepdim=True))[:, None]
    c = int(fs / 50.0 + 0.5)
    n = 2 * c + 1
    h = 0.5 - 0.5 * torch.cos(torch.arange(1, n + 1, device=x.device, dtype=torch.float64) * (2 * math.pi / (n + 1)))
    h = -h / h.sum()
    h[c] += 1.0
    y = conv(y, h.flip(0)[None, None], padding=c)
    out = []
    for k in range(1 + int(math.log2(f0_ceil / f0_floor) * cpo)):
        hal = int(fs / (f0_floor * 2.0 ** ((k + 1) / cpo)) / 2.0 + 0.5)
        u = torch.arange(4 * hal, device=x.device, dtype=torch.float64) / (4 * hal - 1.0)
        w = 0.355768 - 0.487396 * torch.cos(2 * math.pi * u) + 0.144232 * torch.cos(4 * math.pi * u) - 0.012604 * torch.cos(6 * math.pi * u)
        f = conv(torch.nn.functional.pad(y, (2 * hal - 1, 2 * hal)), w.flip(0)[None, None])[:, 0]
        d = f[:, 1:] - f[:, :-1]
        for g in (f, -f, -d, d):
            m = (g[:, :-1] > 0) & (g[:, 1:] <= 0)
            fine = torch.arange(1, g.shape[1], device=x.device, dtype=torch.float64) - g[:, :-1] / (g[:, 1:] - g[:, :-1])
            out.append((m.cumsum(1), torch.where(m, fine, torch.zeros_like(fine))))
    return out


def main():
    a = parse_args('bench_dio', iters=20, warmup=3, rounds=5, torch_iters=3, out=os.path.join(ROOT, 'profiles', 'dio_bench.txt'))
    import dio_ref as R
    import tdvc_amd as P
    from bench_mcd import voiced_signal
    dev = torch.device('cuda:0')
    E = P.evaluate
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    fs, hop = 16000, 80
    lines = []
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000)):
        rng = np.random.default_rng(B)
        test, ref = voiced_signal(rng, B, T).to(dev), voiced_signal(rng, B, T).to(dev)
        x = test[:, 0]
        d = P.dio(x, fs, hop)
        c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
        f0_conv = P.track_f0(test)
        noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
        phi0 = torch.tensor([0.5], device=dev)
        kw = dict(envelope='cheaptrick', align='fastdtw')
        fns = {'dio': (lambda: P.dio(x, fs, hop), a.iters),
               'stonemask': (lambda: P.stonemask(x, d, fs, hop), a.iters),
               'world_f0': (lambda: P.world_f0(x, fs, hop), a.iters),
               'mcd_world': (lambda: E.mcd(test, ref, f0_method='dio', **kw), a.iters),
               'yin_f0': (lambda: P.yin_f0(x, fs, pitch_min=50, pitch_max=500, frame_stride=hop / fs), a.iters),
               'torch_fir_crossings': (lambda: torch_front_end(x, fs), a.torch_iters),
               'mcd_yin': (lambda: E.mcd(test, ref, **kw), a.iters),
               'generator_forward': (lambda: P.infer.convert(G, test, c_tgt, f0_conv, noise=noise, start_phase=phi0), max(1, a.iters // 4))}
        try:
            torch_front_end(x, fs)
        except RuntimeError as e:                                              # a build of torch without float64 convolutions on the device
            print(f'torch_fir_crossings left out: {str(e)[:120]}', flush=True)
            del fns['torch_fir_crossings']
        row = x[0].cpu().numpy()
        t0 = time.perf_counter()
        w_ref, d_ref = R.world_f0(row, fs, hop)
        host_ms = (time.perf_counter() - t0) * 1e3
        w_dev = P.world_f0(x, fs, hop)
        g, v = w_dev[0].cpu().numpy().astype(np.float64), w_ref > 0
        same = bool(np.array_equal(g > 0, v))
        gap = float((np.abs(g - w_ref)[v & (g > 0)] / w_ref[v & (g > 0)]).max())
        r_w, r_y = E.mcd(test, ref, f0_method='dio', **kw), E.mcd(test, ref, **kw)
        med, mm = measure(fns, a.warmup, a.rounds, once=('torch_fir_crossings',))
        out = {'shape': name, 'B': B, 'frames': d.shape[1], 'voiced_frames_world': [int(n) for n in (w_dev > 0).sum(1).tolist()][:4],
               'row0_voiced_set_equals_numpy': same, 'row0_rel_gap_to_numpy': float(f'{gap:.2e}'), 'numpy_world_f0_ms': round(host_ms, 1),
               'mcd_world': [round(float(t), 4) for t in r_w['mcd'].tolist()][:4], 'mcd_yin': [round(float(t), 4) for t in r_y['mcd'].tolist()][:4],
               'f0_ratio_world': [round(float(t), 4) for t in r_w['f0_ratio'].tolist()][:4], **report(med, mm, 1)}
        out['world_f0_us_per_frame'] = round(med['world_f0'] / (B * d.shape[1]), 3)
        if 'torch_fir_crossings' in med:
            out['torch_front_end_over_dio'] = round(med['torch_fir_crossings'] / med['dio'], 1)
        out['numpy_row_over_world_f0_batch'] = round(host_ms * 1e3 / med['world_f0'], 1)
        out['world_f0_over_yin_f0'] = round(med['world_f0'] / med['yin_f0'], 2)
        out['mcd_world_over_mcd_yin'] = round(med['mcd_world'] / med['mcd_yin'], 2)
        out['mcd_world_over_generator_forward'] = round(med['mcd_world'] / med['generator_forward'], 3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_dio.py on one MI355X (defaults: {a.iters} calls per timing, warm-up {a.warmup}, {a.rounds} rounds alternating the\n'
                '# implementations, median and [min, max] in microseconds per call; torch_fir_crossings '
                f'{a.torch_iters} calls per round), 16 kHz, 5 ms hop,\n# 50..500 Hz, 2 channels per octave. The names are explained at the top of the tool.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
