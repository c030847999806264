"""Times the ECAPA-TDNN speaker-recognition metric on the GPU (td-vc-gan_amd/ecapa.py; csrc/eval_ecapa.hip), per call, with the
shipped widths (C = 1024, 3C = 3072, 192-dimensional embedding) and seeded weights:

    fbank                 the front end alone (two launches: float64 DFT, mel sums and dB; floor, mean, store)
    tdnn_80_1024_k5       blocks[0]'s convolution with its ReLU + BatchNorm epilogue (one tdvc_tdnn_fwd launch)
    tdnn_1024_1024_k1     a tdnn1 / tdnn2 layer
    tdnn_128_128_k3_d2    one Res2Net branch (a channel slice in, the previous branch added, a channel slice out)
    tdnn_3072_3072_k1     the MFA layer
    se_block              mean, gate and g x + residual on [B, 1024, F] (three launches)
    asp_pool              attentive statistics pooling on [B, 3072, F] (statistics, row bias, two tdvc_tdnn_fwd launches, pooling)
    ecapa_head            asp_bn + fc
    embed_features        the network from features to embeddings
    embed                 waveform in, embeddings out

beside comparators measured in the same session:

    torch_embed_features  the same network in stock torch fp32 ops on the same device on the same features (tests/ecapa_ref.py's
                          restatement; every row is full, so one batched evaluation is the row-alone result)
    generator_forward     one infer.convert forward of the same audio (config/conv_enc-stage1.yaml, weights as initialised)

    python tools/bench_ecapa.py [--iters 10] [--warmup 2] [--rounds 5] [--torch-iters 5] [--out profiles/ecapa_bench.txt]

Shapes: 16 x 4.48 s (71680 samples, 449 frames) and 1 x 20 s (2001 frames) at 16 kHz; the signals of tools/bench_mcd.py. Device time
from events around `iters` back-to-back calls after a warm-up, the implementations alternating in rounds; the median round is
reported with the spread. One JSON line per shape, microseconds per call, printed and written to --out.
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


def main():
    a = parse_args('bench_ecapa', iters=10, warmup=2, rounds=5, torch_iters=5, out=os.path.join(ROOT, 'profiles', 'ecapa_bench.txt'))
    import ecapa_ref as R
    import tdvc_amd as P
    from bench_mcd import voiced_signal
    dev = torch.device('cuda:0')
    ec = P.ecapa
    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    G = P.infer.build_generator(hp.model.generator, 16, dev)
    sd = R.state_dict(21, R.FULL)
    enc = ec.EcapaTdnn()
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    fold = enc._fold(dev)
    lines = []
    for name, B, T in (('16 x 4.48 s', 16, 71680), ('1 x 20 s', 1, 320000)):
        rng = np.random.default_rng(B)
        test = voiced_signal(rng, B, T).to(dev)
        feats, frames = enc.features(test)
        F = feats.shape[2]
        act = lambda ch: torch.randn(B, ch, F, device=dev)
        x1k, x3k, y1k = act(1024), act(3072), act(1024)
        o1k, o3k = torch.empty_like(x1k), torch.empty_like(x3k)
        pooled = torch.randn(B, 6144, device=dev)
        b2, se = enc.blocks[2], enc.blocks[2].se_block

        def torch_embed():
            return R.embed_full(sd_dev, feats)

        c_tgt = torch.zeros(B, 16, device=dev); c_tgt[:, 3] = 1.0
        f0_conv = P.track_f0(test)
        noise = (torch.randn(B, 1, T, device=dev), torch.randn(B, 1, T, device=dev))
        phi0 = torch.tensor([0.5], device=dev)
        fns = {'fbank': (lambda: ec.fbank(test), a.iters),
               'tdnn_80_1024_k5': (lambda: enc._tdnn(fold, 'blocks.0', enc.blocks[0], feats, frames, out=o1k), a.iters),
               'tdnn_1024_1024_k1': (lambda: enc._tdnn(fold, 'blocks.2.tdnn1', b2.tdnn1, x1k, frames, out=o1k), a.iters),
               'tdnn_128_128_k3_d2': (lambda: enc._tdnn(fold, 'blocks.1.res2net_block.blocks.1', enc.blocks[1].res2net_block.blocks[1], x1k[:, 256:384],
                                                        frames, out=o1k[:, 256:384], x2=o1k[:, 128:256]), a.iters),
               'tdnn_3072_3072_k1': (lambda: enc._tdnn(fold, 'mfa', enc.mfa, x3k, frames, out=o3k), a.iters),
               'se_block': (lambda: ec.se_block(x1k, y1k, se.conv1.conv.weight, se.conv1.conv.bias, se.conv2.conv.weight, se.conv2.conv.bias,
                                                frames=frames, out=o1k), a.iters),
               'asp_pool': (lambda: ec.asp_pool(x3k, enc.asp.tdnn.conv.conv.weight, enc.asp.tdnn.conv.conv.bias, *fold['asp.tdnn.norm'],
                                                enc.asp.conv.conv.weight, enc.asp.conv.conv.bias, frames=frames), a.iters),
               'ecapa_head': (lambda: ec.ecapa_head(pooled, *fold['asp_bn'], enc.fc.conv.weight, enc.fc.conv.bias), a.iters),
               'embed_features': (lambda: enc.embed_features(feats, frames), a.iters),
               'embed': (lambda: enc.embed(test), a.iters),
               'torch_embed_features': (torch_embed, a.torch_iters),
               'generator_forward': (lambda: P.infer.convert(G, test, c_tgt, f0_conv, noise=noise, start_phase=phi0), max(1, a.iters // 4))}
        gap = float((torch_embed() - enc.embed_features(feats, frames)).abs().max())
        med, mm = measure(fns, a.warmup, a.rounds)
        out = {'shape': name, 'B': B, 'frames': F, 'max_gap_to_torch': float(f'{gap:.2e}'), **report(med, mm, 1)}
        out['torch_over_hip_embed_features'] = round(med['torch_embed_features'] / med['embed_features'], 2)
        out['embed_over_generator_forward'] = round(med['embed'] / med['generator_forward'], 3)
        flop = 2.0 * B * F * 3072 * 3072
        out['mfa_tflops'] = round(flop / med['tdnn_3072_3072_k1'] * 1e-6, 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_ecapa.py on one MI355X (defaults: {a.iters} calls per timing, warm-up {a.warmup}, {a.rounds} rounds alternating the\n'
                f'# implementations, median and [min, max] in microseconds per call; torch_embed_features {a.torch_iters} calls per round), 16 kHz,\n'
                '# shipped widths (C = 1024), seeded weights. The names are explained at the top of the tool.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
