"""Writes tests/golden/wavlm_small.npz from the REFERENCE's own wavlm/WavLM.py and wavlm/modules.py on the CPU: the fixture that pins
td-vc-gan_amd/wavlm.py's definition (and tests/wavlm_ref.py) to the reference's code. Run by hand, never by a test:

    python tools/make_golden_wavlm.py --reference /path/to/the/reference/checkout

Configuration: 7 conv layers of 32 channels, C = 64, 4 heads, FFN 128, 2 layers, conv_pos = 16 in 4 groups, num_buckets = 320,
max_distance = 800, layer-norm extractor, layer_norm_first, gated relative position bias. The reference's seeded init, then a seeded
perturbation of every LayerNorm, bias, grep_linear and grep_a parameter (at their init values, ones and zeros, a swapped gate or a
dropped bias would pass). Contents: the state dict (sd/<key>, fp32), cfg (JSON), an input of 2 x 8160 samples at -30 dB, the float64
evaluation of extract_features: the final output (out), output_layer = 1 and 2 (layer1, layer2), ret_conv=True (conv), and the
reference's bucket indices for s - t in -2047..2047 (buckets). It then records, in tests/golden/wavlm_small_pinning.json (a file of
its own in the style of PINNING.json), how far the float64 restatement tests/wavlm_ref.py is from what it stored.

Float64: the module is converted with .double(). Two places of the reference cast to float32 whatever they are given, Fp32LayerNorm
in the front end and the FFN's gelu(x.float()); for the float64 evaluation those two are replaced, on the instances, by
torch.nn.LayerNorm.forward and torch.nn.functional.gelu: the same functions without the cast."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(extractor_mode='layer_norm', encoder_layers=2, encoder_embed_dim=64, encoder_ffn_embed_dim=128, encoder_attention_heads=4,
           activation_fn='gelu', layer_norm_first=True, conv_feature_layers='[(32,10,5)] + [(32,3,2)] * 4 + [(32,2,2)] * 2', conv_bias=False,
           normalize=False, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, encoder_layerdrop=0.0, dropout_input=0.0,
           dropout_features=0.0, conv_pos=16, conv_pos_groups=4, relative_position_embedding=True, num_buckets=320, max_distance=800,
           gru_rel_pos=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='the reference checkout (holds wavlm/WavLM.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'wavlm_small.npz'))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from wavlm.WavLM import WavLM, WavLMConfig
    from wavlm import modules as M

    torch.manual_seed(20261020)
    np.random.seed(20261020)
    model = WavLM(WavLMConfig(CFG)).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in model.named_parameters():
            norm = any(s in name for s in ('layer_norm', '.2.1.'))
            if norm or name.endswith('.bias') or 'grep_linear' in name or name.endswith('grep_a'):
                p.add_(0.3 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone().float() for k, v in model.state_dict().items()}
    x = (torch.randn(2, 8160, generator=g, dtype=torch.float64) * 10.0 ** (-30.0 / 20.0)).float()

    model = model.double()
    for m in model.modules():
        if isinstance(m, M.Fp32LayerNorm):
            m.__class__ = torch.nn.LayerNorm
        if hasattr(m, 'activation_fn') and getattr(m, 'activation_name', None) == 'gelu':
            m.activation_fn = torch.nn.functional.gelu
    xd = x.double()
    with torch.no_grad():
        out = model.extract_features(xd)[0]
        l1 = model.extract_features(xd, output_layer=1)[0]
        l2 = model.extract_features(xd, output_layer=2)[0]
        conv = model.extract_features(xd, ret_conv=True)[0]
        buckets = model.encoder.layers[0].self_attn._relative_positions_bucket(torch.arange(-2047, 2048), bidirectional=True)
    assert out.dtype == torch.float64 and l2.shape == out.shape and not torch.equal(l2, out)
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    arrays.update(cfg=np.array(json.dumps(CFG)), input=x.numpy(), out=out.numpy(), layer1=l1.numpy(), layer2=l2.numpy(), conv=conv.numpy(),
                  buckets=buckets.numpy().astype(np.int64))
    np.savez_compressed(args.out, **arrays)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes, out {tuple(out.shape)} max|out| {float(out.abs().max()):.3f}')
    # how far the float64 restatement the GPU tests measure against is from what was just stored -> wavlm_small_pinning.json
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import wavlm_ref as R
    sdd = R.cast(sd, torch.float64)
    want = dict(out=(out, {}), layer1=(l1, dict(output_layer=1)), layer2=(l2, dict(output_layer=2)), conv=(conv, dict(ret_conv=True)))
    pin = {k: float((R.extract(sdd, R.SMALL, xd, **kw) - v).abs().max() / v.abs().max()) for k, (v, kw) in want.items()}
    pin['bucket_mismatches'] = int((R.buckets(torch.arange(-2047, 2048), 320, 800) != buckets).sum())
    pin_path = os.path.join(os.path.dirname(args.out), 'wavlm_small_pinning.json')
    json.dump({'wavlm_small': pin}, open(pin_path, 'w'), indent=1)
    print('pinned:', pin)


if __name__ == '__main__':
    main()
