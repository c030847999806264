"""Times the CREPE pitch tracker on the GPU (td-vc-gan_amd/crepe.py; csrc/pitch_crepe.hip), per call, with seeded weights
(tests/crepe_ref.state_dict):

    frames                the front end alone (tdvc_crepe_frames, one launch)
    conv1 .. conv6        one conv block each: conv + bias + ReLU + folded BatchNorm + max-pool 2 (one tdvc_crepe_conv launch)
    head                  the position-major flatten, Linear(., 360) and the sigmoid (tdvc_crepe_head)
    decode_argmax         tdvc_crepe_decode, one launch; decode_weighted the same with the weighted argmax
    decode_viterbi        the lattice launch, tdvc_viterbi_path on the 209 in-range states, and the launch that reads the path
    activations           waveform in, activations [B, 360, F] out (eight launches)
    filtered_pitch_*      waveform in, pitch out, with each decoder: what the reference's util/crepe.py filtered_pitch returns

beside comparators measured in the same session:

    torch_network         the same network in stock torch fp32 ops on the same device on the same frames (tests/crepe_ref.py's
                          restatement: F.pad, F.conv2d, F.batch_norm, F.max_pool2d, F.linear), frames to activations
    network               conv1 .. conv6 and head, frames to activations: what torch_network is compared with
    track_f0              the YIN tracker this project has used in CREPE's place (one launch)
    generator_forward     one infer.convert forward of the same audio (config/conv_enc-stage1.yaml, weights as initialised)

    python tools/bench_crepe.py [--iters 10] [--warmup 2] [--rounds 5] [--torch-iters 3] [--step-ms MS] [--out profiles/crepe_bench.txt]

Shapes: 16 x 16000 and 1 x 71680 samples for `tiny`, 1 x 16000 for `full`, hop 64, 16 kHz. Device time from events around `iters`
back-to-back calls after a warm-up, the implementations alternating in rounds; the median round is reported with the spread.
--step-ms is the train step to relate activations to: measure it with bench.py in the same session and pass its ms_per_step
(without it no share is reported). One JSON line per shape, microseconds per call, printed and written to --out.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _timing import measure, parse_args, report  # noqa: E402


def flop_per_frame(R, capacity):
    """2 x multiply-adds of the six convs and the classifier, per frame."""
    out = R.CAPACITIES[capacity]
    cin = [1] + out[:-1]
    pos = (256, 128, 64, 32, 16, 8)
    per_layer = [2.0 * cin[i] * R.KERNELS[i] * out[i] * pos[i] for i in range(6)]
    return per_layer, sum(per_layer) + 2.0 * 4 * out[5] * 360


def main():
    a = parse_args('bench_crepe', iters=10, warmup=2, rounds=5, torch_iters=3, out=os.path.join(ROOT, 'profiles', 'crepe_bench.txt'),
                   more=lambda ap: ap.add_argument('--step-ms', type=float, default=None,
                                                   help='ms per train step from bench.py, measured in the same session'))
    import crepe_ref as R
    import tdvc_amd as P
    from bench_mcd import voiced_signal
    dev = torch.device('cuda:0')
    K = P.crepe
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    lines = []
    for name, cap, B, T in (('tiny 16 x 16000', 'tiny', 16, 16000), ('tiny 1 x 71680', 'tiny', 1, 71680), ('full 1 x 16000', 'full', 1, 16000)):
        sd = R.state_dict(11, cap)
        m = K.load_crepe(sd, cap, device=dev)
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        fold = m._fold(dev)
        rng = np.random.default_rng(B)
        x = voiced_signal(rng, B, T).to(dev)
        frames = K.crepe_frames(x)
        F = frames.shape[1]
        N = B * F
        flat = frames.view(N, 1024)
        ins = [flat.view(N, 1, 1024)]
        for i in range(1, 7):
            conv = getattr(m, f'conv{i}')
            ins.append(K.crepe_conv(ins[-1], conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0]))
        act = m.activations(x)

        def conv_fn(i):
            conv = getattr(m, f'conv{i}')
            out = torch.empty_like(ins[i])
            return lambda: K.crepe_conv(ins[i - 1], conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0], out=out)

        def network():
            return K.crepe_head(m.embed_frames(flat), m.classifier.weight, m.classifier.bias, frames_per_row=F)

        def torch_network():
            return R.network(sd_dev, flat, torch.float32)

        fns = {'frames': (lambda: K.crepe_frames(x), a.iters)}
        fns.update({f'conv{i}': (conv_fn(i), a.iters) for i in range(1, 7)})
        fns.update({'head': (lambda: K.crepe_head(ins[6], m.classifier.weight, m.classifier.bias, frames_per_row=F), a.iters),
                    'decode_argmax': (lambda: K.crepe_decode(act), a.iters),
                    'decode_weighted': (lambda: K.crepe_decode(act, decoder='weighted_argmax'), a.iters),
                    'decode_viterbi': (lambda: K.crepe_decode(act, decoder='viterbi'), a.iters),
                    'network': (network, a.iters),
                    'activations': (lambda: m.activations(x), a.iters),
                    'filtered_pitch_argmax': (lambda: m.filtered_pitch(x, 'argmax'), a.iters),
                    'filtered_pitch_weighted_argmax': (lambda: m.filtered_pitch(x, 'weighted_argmax'), a.iters),
                    'filtered_pitch_viterbi': (lambda: m.filtered_pitch(x, 'viterbi'), a.iters),
                    'torch_network': (torch_network, a.torch_iters),
                    'track_f0': (lambda: P.track_f0(x), a.iters)})
        if T % 320 == 0 and T >= 8320:
            c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
            f0_conv = P.track_f0(x)
            noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
            phi0 = torch.tensor([0.5], device=dev)
            fns['generator_forward'] = (lambda: P.infer.convert(G, x, c_tgt, f0_conv, noise=noise, start_phase=phi0), max(1, a.iters // 4))
        gap = float((torch_network() - network().reshape(B, 360, F).permute(0, 2, 1).reshape(N, 360)).abs().max())
        med, mm = measure(fns, a.warmup, a.rounds)
        per_layer, total = flop_per_frame(R, cap)
        out = {'shape': name, 'capacity': cap, 'B': B, 'T': T, 'frames': N, 'mflop_per_frame': round(total * 1e-6, 1),
               'max_gap_to_torch': float(f'{gap:.2e}'), **report(med, mm, 1)}
        out['conv_tflops'] = {f'conv{i}': round(per_layer[i - 1] * N / med[f'conv{i}'] * 1e-6, 1) for i in range(1, 7)}
        out['network_tflops'] = round(total * N / med['network'] * 1e-6, 1)
        out['torch_over_hip_network'] = round(med['torch_network'] / med['network'], 2)
        out['activations_over_track_f0'] = round(med['activations'] / med['track_f0'], 1)
        if 'generator_forward' in med:
            out['filtered_pitch_viterbi_over_generator_forward'] = round(med['filtered_pitch_viterbi'] / med['generator_forward'], 3)
        if a.step_ms:
            out.update({'step_ms': a.step_ms, 'activations_share_of_step': round(med['activations'] / (a.step_ms * 1e3), 4)})
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_crepe.py on {torch.cuda.get_device_name(0)} (defaults: {a.iters} calls per timing, warm-up {a.warmup}, {a.rounds} rounds\n'
                f'# alternating the implementations, median and [min, max] in microseconds per call; torch_network {a.torch_iters} calls per round),\n'
                f'# 16 kHz, hop 64, seeded weights{f", --step-ms {a.step_ms}" if a.step_ms else ""}. The names are explained at the top of the tool.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
