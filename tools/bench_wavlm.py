"""Times the WavLM feature extractor on the GPU (td-vc-gan_amd/wavlm.py; csrc/ssl_wavlm.hip) with the WavLM-Large shape (7 convs of
512 channels, 24 layers of width 1024, 16 heads, FFN 4096, conv_pos 128 in 16 groups) and seeded weights, per call:

    extract_features      waveform in, [B, L', 1024] out (all launches)
    conv0                 the first convolution with its LayerNorm and GELU (tdvc_wavlm_conv0)
    conv1_gemm, conv1_ln  the second convolution (512 -> 512, k 3, stride 2) as a GEMM, and its LayerNorm + GELU
    proj                  post_extract_proj (512 -> 1024), written into the padded buffer
    posconv               the grouped k-128 convolution + GELU + residual
    ln_gates              a layer's first LayerNorm with the gates of the relative position bias (two launches)
    qkv, out_proj, fc1, fc2   a layer's four GEMMs (q|k|v fused: 1024 -> 3072)
    attention             a layer's attention
    ln                    a layer's second LayerNorm

beside the comparator measured in the same session:

    torch_extract_features   the same network and weights in stock torch fp32 ops on the same device (tests/wavlm_ref.py with
                             F.layer_norm, F.gelu and F.scaled_dot_product_attention put in place of its literal formulas; the
                             bias table is built once, outside the timing)

    python tools/bench_wavlm.py [--iters 5] [--warmup 2] [--rounds 5] [--torch-iters 3] [--out profiles/wavlm_bench.txt]

Shapes: 8 x 32160 samples (the shape of config/wavlm-stage2_2.yaml's step: 8 x 2 s with SSLEncoder's 160 samples of padding, 100
frames) and 1 x 320160 (20 s, 1000 frames). Device time from events around `iters` back-to-back calls after a warm-up, the
implementations alternating in rounds; the median round is reported with the spread. One JSON line per shape, microseconds per call,
with the achieved TFLOP/s of the GEMMs; the first shape also carries the ratio to the 25.3 ms of the stock-torch stand-in
(synth.WavLMShapedExtractor) and the share of config #5's 93.9 ms step.
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _timing import measure, parse_args, report  # noqa: E402

STAND_IN_MS, STEP_MS = 25.3, 93.9


def stock_attention(q, k, v, gate, table):
    B, T, heads, d = q.shape
    pos = torch.arange(T, device=q.device)
    mask = gate[..., None] * table[:, pos[None, :] - pos[:, None] + T - 1][None]
    out = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask, scale=1.0)
    return out.transpose(1, 2).reshape(B, T, heads * d)


def main():
    a = parse_args('bench_wavlm', iters=5, warmup=2, rounds=5, torch_iters=3, out=os.path.join(ROOT, 'profiles', 'wavlm_bench.txt'))
    import tdvc_amd as P
    import wavlm_ref as R
    dev = torch.device('cuda:0')
    w = P.wavlm
    sd = R.state_dict(31, R.LARGE)
    m = w.WavLM()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    del sd
    R.layer_norm = lambda x, g, b: F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)          # the stock ops in place of the literal formulas
    R.gelu = F.gelu
    R.attention = stock_attention
    lay, pk = m.encoder.layers[3], m._pack(dev)
    at, pl = lay.self_attn, pk['layers'][3]
    cl = m.feature_extractor.conv_layers
    lines = []
    for name, B, n in (('8 x 32160', 8, 32160), ('1 x 320160', 1, 320160)):
        x = R.wave(B, n, seed=B).to(dev)
        T = m.num_frames(n)
        table_t = R.bias_table(sd_dev, R.LARGE, T).contiguous()
        got = m.extract_features(x)[0]
        want = R.extract(sd_dev, R.LARGE, x, table=table_t)
        gap = float((got - want).abs().max())
        ws = m._workspace(B, n, dev)
        f0, f1 = ws['feats'][0], ws['feats'][1]
        xp, xx, h, qkv, att, ffn = ws['xp'], ws['x'], ws['h'], ws['qkv'], ws['att'], ws['ffn']
        inner = xp[:, 64:64 + T]
        table = m.bias_table(T, dev)
        gate = torch.full((B, 16, T), 1.75, device=dev)
        wo, w1, w2, wp = (t.detach().contiguous() for t in (at.out_proj.weight, lay.fc1.weight, lay.fc2.weight, m.post_extract_proj.weight))
        fns = {'extract_features': (lambda: m.extract_features(x), a.iters),
               'conv0': (lambda: w.wavlm_conv0(x, pk['conv0'], cl[0][2][1].weight, cl[0][2][1].bias, 5, out=f0), a.iters),
               'conv1_gemm': (lambda: w.wavlm_gemm(f0, pk['convs'][0], kernel=3, stride=2, out=f1), a.iters),
               'conv1_ln': (lambda: w.wavlm_layernorm(f1, cl[1][2][1].weight, cl[1][2][1].bias, gelu=True, out=f1), a.iters),
               'proj': (lambda: w.wavlm_gemm(ws['feats'][-1], wp, m.post_extract_proj.bias, out=inner), a.iters),
               'posconv': (lambda: w.wavlm_posconv(xp, pk['pos'], m.encoder.pos_conv[0].bias, 128, 16, out=xx), a.iters),
               'ln_gates': (lambda: w.wavlm_layernorm(xx, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias, out=h,
                                                      grep=(at.grep_linear.weight, at.grep_linear.bias, pl['grep_a'])), a.iters),
               'qkv': (lambda: w.wavlm_gemm(h, pl['w'], pl['b'], scale=(0, 1024, 0.125), out=qkv), a.iters),
               'attention': (lambda: w.wavlm_attention(qkv, 16, gate, table, out=att), a.iters),
               'out_proj': (lambda: w.wavlm_gemm(att, wo, at.out_proj.bias, residual=h, out=h), a.iters),
               'ln': (lambda: w.wavlm_layernorm(xx, lay.final_layer_norm.weight, lay.final_layer_norm.bias, out=h), a.iters),
               'fc1': (lambda: w.wavlm_gemm(h, w1, lay.fc1.bias, epilogue=w.EPI_GELU, out=ffn), a.iters),
               'fc2': (lambda: w.wavlm_gemm(ffn, w2, lay.fc2.bias, residual=h, out=h), a.iters),
               'torch_extract_features': (lambda: R.extract(sd_dev, R.LARGE, x, table=table_t), a.torch_iters)}
        med, mm = measure(fns, a.warmup, a.rounds)
        out = {'shape': name, 'B': B, 'frames': T, 'max_gap_to_torch': float(f'{gap:.2e}'), 'scale': round(float(want.abs().max()), 2), **report(med, mm, 1)}
        out['torch_over_hip_extract_features'] = round(med['torch_extract_features'] / med['extract_features'], 2)
        tok = B * T
        T1 = (((n - 10) // 5 + 1) - 3) // 2 + 1
        for key, flop in (('conv1_gemm', 2.0 * B * T1 * 512 * 1536), ('qkv', 2.0 * tok * 1024 * 3072), ('out_proj', 2.0 * tok * 1024 * 1024),
                          ('fc1', 2.0 * tok * 1024 * 4096), ('fc2', 2.0 * tok * 1024 * 4096), ('posconv', 2.0 * tok * 1024 * 8192)):
            out[key + '_tflops'] = round(flop / med[key] * 1e-6, 1)
        if B == 8:
            out['extract_features_over_stand_in_25.3ms'] = round(med['extract_features'] * 1e-3 / STAND_IN_MS, 2)
            out['share_of_step_with_it'] = round(med['extract_features'] * 1e-3 / (STEP_MS - STAND_IN_MS + med['extract_features'] * 1e-3), 3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(f'# tools/bench_wavlm.py on one MI355X (defaults: {a.iters} calls per timing, warm-up {a.warmup}, {a.rounds} rounds alternating the\n'
                f'# implementations, median and [min, max] in microseconds per call; torch_extract_features {a.torch_iters} calls per round), 16 kHz,\n'
                '# WavLM-Large shape, seeded weights. The names are explained at the top of the tool.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
