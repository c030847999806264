"""A literal restatement of the WavLM feature extractor (the definition in include/tdvc.h and td-vc-gan_amd/wavlm.py) in stock torch
ops on the CPU, in whatever dtype it is given: float64 is what the GPU tests measure against, float32 is the "stock torch fp32 CPU
evaluation" whose error against float64 sets their network-level bars. tests/test_wavlm_cpu.py pins the float64 evaluation to the
reference's own output (tests/golden/wavlm_small.npz). `trace`, a dict, receives the intermediate of every launch."""
import math

import numpy as np
import torch
import torch.nn.functional as F

LARGE = dict(conv_feature_layers='[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2', encoder_layers=24, encoder_embed_dim=1024,
             encoder_ffn_embed_dim=4096, encoder_attention_heads=16, conv_pos=128, conv_pos_groups=16, num_buckets=320, max_distance=800)
SMALL = dict(conv_feature_layers='[(32,10,5)] + [(32,3,2)] * 4 + [(32,2,2)] * 2', encoder_layers=2, encoder_embed_dim=64,
             encoder_ffn_embed_dim=128, encoder_attention_heads=4, conv_pos=16, conv_pos_groups=4, num_buckets=320, max_distance=800)
WIDE = dict(SMALL, encoder_embed_dim=128, encoder_attention_heads=2, conv_pos_groups=2)                 # d = 64
SSL = dict(conv_feature_layers='[(16,10,5)] + [(16,3,2)] * 4 + [(16,2,2)] * 2', encoder_layers=1, encoder_embed_dim=1024,
           encoder_ffn_embed_dim=64, encoder_attention_heads=16, conv_pos=16, conv_pos_groups=16, num_buckets=320, max_distance=800)
FIXED = dict(extractor_mode='layer_norm', layer_norm_first=True, relative_position_embedding=True, gru_rel_pos=True, conv_bias=False,
             activation_fn='gelu', normalize=False)


def full_cfg(cfg):
    return dict(FIXED, **cfg)


def layers_of(cfg):
    return [tuple(cl) for cl in eval(cfg['conv_feature_layers'])]


def frames(n, cfg):
    for _, k, s in layers_of(cfg):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def expected_shapes(cfg):
    c, f, h, kp, g = (cfg[k] for k in ('encoder_embed_dim', 'encoder_ffn_embed_dim', 'encoder_attention_heads', 'conv_pos', 'conv_pos_groups'))
    out, cin = {'mask_emb': (c,)}, 1
    for i, (dim, k, _) in enumerate(layers_of(cfg)):
        out[f'feature_extractor.conv_layers.{i}.0.weight'] = (dim, cin, k)
        out[f'feature_extractor.conv_layers.{i}.2.1.weight'] = out[f'feature_extractor.conv_layers.{i}.2.1.bias'] = (dim,)
        cin = dim
    out['layer_norm.weight'] = out['layer_norm.bias'] = (cin,)
    out['post_extract_proj.weight'], out['post_extract_proj.bias'] = (c, cin), (c,)
    out['encoder.pos_conv.0.bias'], out['encoder.pos_conv.0.weight_g'], out['encoder.pos_conv.0.weight_v'] = (c,), (1, 1, kp), (c, c // g, kp)
    out['encoder.layer_norm.weight'] = out['encoder.layer_norm.bias'] = (c,)
    for li in range(cfg['encoder_layers']):
        p = f'encoder.layers.{li}.'
        for name in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            out[p + f'self_attn.{name}.weight'], out[p + f'self_attn.{name}.bias'] = (c, c), (c,)
        out[p + 'self_attn.grep_linear.weight'], out[p + 'self_attn.grep_linear.bias'], out[p + 'self_attn.grep_a'] = (8, c // h), (8,), (1, h, 1, 1)
        if li == 0:
            out[p + 'self_attn.relative_attention_bias.weight'] = (cfg['num_buckets'], h)
        for name in ('self_attn_layer_norm', 'final_layer_norm'):
            out[p + name + '.weight'] = out[p + name + '.bias'] = (c,)
        out[p + 'fc1.weight'], out[p + 'fc1.bias'], out[p + 'fc2.weight'], out[p + 'fc2.bias'] = (f, c), (f,), (c, f), (c,)
    return out


def state_dict(seed, cfg):
    """Seeded fp32 weights of our own: matrices N(0, 1 / fan_in) (q and k twice that each, so that the softmax is far from flat),
    LayerNorm gains 1 + 0.3 N, every bias 0.3 N, grep_a 1 + N (some negative), the bias table N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in sorted(expected_shapes(cfg).items()):
        r = torch.randn(*shape, generator=g)
        if k.endswith('grep_a'):
            v = 1.0 + r
        elif k.endswith('weight_g'):
            v = 1.0 + 0.3 * r
        elif k.endswith('relative_attention_bias.weight') or k == 'mask_emb':
            v = r
        elif len(shape) == 1:
            v = 1.0 + 0.3 * r if k.endswith('weight') else 0.3 * r
        else:
            fan_in = int(np.prod(shape[1:]))
            v = r * (fan_in ** -0.5) * (2.0 if '.q_proj.' in k or '.k_proj.' in k else 1.0) * (1.4 if 'conv_layers' in k else 1.0)
        sd[k] = v.float()
    return sd


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def buckets(rel, num_buckets, max_distance):
    """bucket(s - t) of modules.py's _relative_positions_bucket(bidirectional=True): float32 logarithm, truncation toward zero."""
    rel = torch.as_tensor(rel, dtype=torch.long)
    n = num_buckets // 2
    side = (rel > 0).long() * n
    dist = rel.abs()
    exact = n // 2
    log_part = torch.log(dist.to(torch.float32) / exact) / math.log(max_distance / exact) * (n - exact)
    far = torch.clamp(exact + log_part.to(torch.long), max=n - 1)
    return side + torch.where(dist < exact, dist, far)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def conv_block(sd, i, h, stride):
    """h [B, T, Cin] token-major -> gelu(LN(conv)) [B, T', Cout]; also the raw convolution."""
    p = f'feature_extractor.conv_layers.{i}.'
    raw = F.conv1d(h.transpose(1, 2), sd[p + '0.weight'], stride=stride).transpose(1, 2)
    return gelu(layer_norm(raw, sd[p + '2.1.weight'], sd[p + '2.1.bias'])), raw


def fold_pos(sd):
    v = sd['encoder.pos_conv.0.weight_v']
    return sd['encoder.pos_conv.0.weight_g'] * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))


def pos_conv(sd, cfg, x):
    k = cfg['conv_pos']
    y = F.conv1d(x.transpose(1, 2), fold_pos(sd), sd['encoder.pos_conv.0.bias'], padding=k // 2, groups=cfg['conv_pos_groups'])
    if k % 2 == 0:
        y = y[:, :, :-1]
    return x + gelu(y).transpose(1, 2)


def gates(h, w, b, a, heads):
    """h [B, T, C] -> gate [B, H, T]"""
    B, T, c = h.shape
    u = h.reshape(B, T, heads, c // heads) @ w.t() + b                       # [B, T, H, 8]
    ga, gb = torch.sigmoid(u[..., :4].sum(-1)), torch.sigmoid(u[..., 4:].sum(-1))
    return (ga * (gb * a.reshape(1, 1, heads) - 1.0) + 2.0).permute(0, 2, 1)


def bias_table(sd, cfg, T):
    """[H, 2 T - 1], indexed by s - t + T - 1"""
    idx = buckets(torch.arange(-(T - 1), T), cfg['num_buckets'], cfg['max_distance'])
    return sd['encoder.layers.0.self_attn.relative_attention_bias.weight'][idx].t()


def attention(q, k, v, gate, table):
    """q (scaled), k, v [B, T, H, d], gate [B, H, T], table [H, 2 T - 1] -> [B, T, H d]"""
    B, T, heads, d = q.shape
    pos = torch.arange(T, device=q.device)
    rel = pos[None, :] - pos[:, None] + T - 1                                # [t, s]
    scores = torch.einsum('bthd,bshd->bhts', q, k) + gate[..., None] * table[:, rel][None]
    return torch.einsum('bhts,bshd->bthd', torch.softmax(scores, dim=-1), v).reshape(B, T, heads * d)


def encoder_layer(sd, cfg, li, x, table, trace=None):
    p, heads = f'encoder.layers.{li}.', cfg['encoder_attention_heads']
    B, T, c = x.shape
    d = c // heads
    h = layer_norm(x, sd[p + 'self_attn_layer_norm.weight'], sd[p + 'self_attn_layer_norm.bias'])
    lin = lambda t, name: t @ sd[p + name + '.weight'].t() + sd[p + name + '.bias']
    q = lin(h, 'self_attn.q_proj') * d ** -0.5
    k, v = lin(h, 'self_attn.k_proj'), lin(h, 'self_attn.v_proj')
    gate = gates(h, sd[p + 'self_attn.grep_linear.weight'], sd[p + 'self_attn.grep_linear.bias'], sd[p + 'self_attn.grep_a'], heads)
    att = attention(q.reshape(B, T, heads, d), k.reshape(B, T, heads, d), v.reshape(B, T, heads, d), gate, table)
    x1 = x + lin(att, 'self_attn.out_proj')
    h2 = layer_norm(x1, sd[p + 'final_layer_norm.weight'], sd[p + 'final_layer_norm.bias'])
    f1 = gelu(lin(h2, 'fc1'))
    x2 = x1 + lin(f1, 'fc2')
    if trace is not None:
        trace[f'l{li}'] = dict(h=h, qkv=torch.cat([q, k, v], -1), gate=gate, att=att, x1=x1, h2=h2, f1=f1, x2=x2)
    return x2


def extract(sd, cfg, source, output_layer=None, ret_conv=False, trace=None, table=None):
    """source [B, L] in the dtype of sd -> [B, L', C]: extract_features(source, ret_conv=, output_layer=)[0] of the definition."""
    h = source[:, :, None]
    for i, (_, _, s) in enumerate(layers_of(cfg)):
        h, raw = conv_block(sd, i, h, s)
        if trace is not None:
            trace[f'conv{i}'], trace[f'conv{i}_raw'] = h, raw
    h = layer_norm(h, sd['layer_norm.weight'], sd['layer_norm.bias'])
    feats = h @ sd['post_extract_proj.weight'].t() + sd['post_extract_proj.bias']
    if trace is not None:
        trace['norm'], trace['proj'] = h, feats
    if ret_conv:
        return feats
    x = pos_conv(sd, cfg, feats)
    if trace is not None:
        trace['pos'] = x
    table = bias_table(sd, cfg, x.shape[1]) if table is None else table
    for li in range(cfg['encoder_layers']):
        x = encoder_layer(sd, cfg, li, x, table, trace)
        if output_layer is not None and li + 1 == output_layer:
            return x
    return layer_norm(x, sd['encoder.layer_norm.weight'], sd['encoder.layer_norm.bias'])


def wave(B, n, seed, db=-30.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, n, generator=g, dtype=torch.float64) * 10.0 ** (db / 20.0)).float()
