"""The WavLM feature extractor on the device: what the reference's model/ssl_encoder.py:141-145 calls as
`WavLM.extract_features(source)[0]`, from the reference's vendored wavlm/WavLM.py (W) and wavlm/modules.py (M). `WavLM(cfg)` has the
reference's state-dict keys and shapes and loads a `{'cfg', 'model'}` checkpoint strictly; `SSLEncoder(cmodel=WavLM(...))` and
`Generator(encoder_model='wavlm', cmodel=WavLM(...))` take it as they take any extractor, and `infer.convert_audio` then runs waveform
to waveform. The reference ships the code but not the 1.2 GB checkpoint, so the definition (also in include/tdvc.h) is pinned to the
reference's code by a fixture of its own float64 output on a small seeded configuration (tests/golden/wavlm_small.npz, written by
tools/make_golden_wavlm.py) and restated in float64 in tests/wavlm_ref.py; **parity with a real WavLM-Large.pt is unchecked (the
checkpoint is absent)**. No weights are shipped.

Definition: eval mode, padding_mask=None, mask=False, the layer-norm feature extractor, layer_norm_first=True, relative position
embedding with gru_rel_pos=True. WavLM-Large is expected to be 7 convs (512,10,5) + (512,3,2) x 4 + (512,2,2) x 2 without bias, 24
layers of width 1024 with 16 heads and FFN 4096, conv_pos=128, conv_pos_groups=16, num_buckets=320, max_distance=800; the checkpoint's
own cfg dict rules, these are the constructor defaults only.
  1. Input: the waveform as it is: the reference never applies cfg.normalize (its caller would have to, and SSLEncoder does not).
     Rows are full length: there are no per-row lengths. A row's result does not depend on its batch.
  2. Front end (W:378-504): per layer Conv1d without bias, LayerNorm over the channels (eps 1e-5, affine), erf-GELU; frame counts
     (L - k) // s + 1 per layer; L' = 0 (L < 400) is refused. Then WavLM.layer_norm, then post_extract_proj (ret_conv=True returns this).
  3. Positional convolution (W:514-527, 577-580): grouped Conv1d(C, C, 128, padding 64, groups 16), weight norm over dim=2
     (w = g v / ||v||, the norm over dims 0 and 1, one norm per tap), the last output frame dropped, GELU, x = x + pos.
  4. Layer l (W:690-715, M:504-564): h = LN(x); q = (h Wq^T + bq) d^-1/2, k, v; per head n: u = grep_linear_l(h[t, n d:(n+1) d]),
     a = sigmoid(u0+..+u3), b = sigmoid(u4+..+u7), gate = a (b grep_a_l[n] - 1) + 2; scores q_t . k_s + gate[b,n,t] bias[n][bucket(s - t)],
     softmax over s, times v, out_proj, + x; then x = x + fc2(gelu(fc1(LN(x)))). relative_attention_bias exists in layer 0 only.
  5. Bias buckets (M:417-455): on the host exactly as the reference evaluates them (float32 logarithm, truncation toward zero), as a
     device table bias_rel[H][2 T' - 1] indexed by s - t, cached per T'.
  6. Output: encoder.layer_norm -> [B, L', C]; output_layer=k returns layer k's output without that norm, as the reference does.

Everything runs in csrc/ssl_wavlm.hip (tdvc_wavlm_conv0, tdvc_wavlm_gemm, tdvc_wavlm_layernorm, tdvc_wavlm_posconv,
tdvc_wavlm_attention): no CPU or ATen fallback, no host synchronisation, no atomics, fixed summation orders (bit-identical from call to
call), every launch capturable into a graph once the per-(B, L) workspace and the per-T' bias table exist (one eager call).
"""
import ctypes as C
import math

import torch

from . import _host as H
from . import _lib as L

EPI_NONE, EPI_GELU = L.WAVLM_NONE, L.WAVLM_GELU
LARGE = dict(extractor_mode='layer_norm', encoder_layers=24, encoder_embed_dim=1024, encoder_ffn_embed_dim=4096, encoder_attention_heads=16,
             layer_norm_first=True, conv_feature_layers='[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2', conv_bias=False, normalize=True,
             conv_pos=128, conv_pos_groups=16, relative_position_embedding=True, num_buckets=320, max_distance=800, gru_rel_pos=True)


class WavLMConfig:
    """The reference's WavLMConfig field for field (W:162-217), so that WavLMConfig(checkpoint['cfg']) works; the defaults are
    WavLM-Large's instead of the reference's base model."""

    def __init__(self, cfg=None):
        self.extractor_mode = 'layer_norm'
        self.encoder_layers = 24
        self.encoder_embed_dim = 1024
        self.encoder_ffn_embed_dim = 4096
        self.encoder_attention_heads = 16
        self.activation_fn = 'gelu'
        self.layer_norm_first = True
        self.conv_feature_layers = '[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2'
        self.conv_bias = False
        self.feature_grad_mult = 1.0
        self.normalize = True
        self.dropout = 0.0
        self.attention_dropout = 0.0
        self.activation_dropout = 0.0
        self.encoder_layerdrop = 0.0
        self.dropout_input = 0.0
        self.dropout_features = 0.0
        self.mask_length = 10
        self.mask_prob = 0.8
        self.mask_selection = 'static'
        self.mask_other = 0
        self.no_mask_overlap = False
        self.mask_min_space = 1
        self.mask_channel_length = 10
        self.mask_channel_prob = 0.0
        self.mask_channel_selection = 'static'
        self.mask_channel_other = 0
        self.no_mask_channel_overlap = False
        self.mask_channel_min_space = 1
        self.conv_pos = 128
        self.conv_pos_groups = 16
        self.relative_position_embedding = True
        self.num_buckets = 320
        self.max_distance = 800
        self.gru_rel_pos = True
        if cfg is not None:
            self.update(cfg)

    def update(self, cfg):
        self.__dict__.update(cfg.__dict__ if isinstance(cfg, WavLMConfig) else cfg)


def conv_layers(cfg):
    """cfg.conv_feature_layers ('[(512,10,5)] + [(512,3,2)] * 4 + ...', the reference evaluates the string) -> [(dim, k, stride), ...]."""
    spec = cfg.conv_feature_layers
    if isinstance(spec, str):
        if not set(spec) <= set('0123456789[]()+*, '):
            raise ValueError(f'WavLM: conv_feature_layers holds more than a list expression: {spec!r}')
        spec = eval(spec, {'__builtins__': {}})      # digits, brackets, + and * only
    return [tuple(int(v) for v in cl) for cl in spec]


def frame_count(n, layers):
    """Frames of a row of n samples after the convolutions [(dim, k, stride), ...]: (L - k) // s + 1 each, 0 once a kernel does not fit."""
    for _, k, s in layers:
        n = (n - k) // s + 1 if n >= k else 0
    return n


def relative_buckets(rel, num_buckets, max_distance):
    """M:417-442 (bidirectional) line for line: int64 offsets s - t -> bucket indices. The logarithm is float32 and the cast to long
    truncates toward zero, as in the reference."""
    rel = torch.as_tensor(rel, dtype=torch.long)
    num_buckets = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * num_buckets
    rel = torch.abs(rel)
    max_exact = num_buckets // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(is_small, rel, large)


def fold_pos_conv(weight_g, weight_v):
    """weight_norm(dim=2) of the positional convolution: g [1, 1, K], v [C, C / G, K] -> w = g v / ||v|| with the norm over dims 0 and
    1 (one per tap), in float64, permuted to [C][K][C / G] and rounded once."""
    v = weight_v.detach().double()
    w = weight_g.detach().double() * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    return w.permute(0, 2, 1).contiguous().float()


def permute_conv(weight):
    """Conv1d weight [Cout, Cin, k] -> [Cout, k Cin]: the row the GEMM multiplies with k consecutive tokens of Cin channels."""
    return weight.detach().float().permute(0, 2, 1).contiguous().reshape(weight.shape[0], -1)


# ------------------------------------------------------------------------------------------------------------------ operators
def _tok3(who, t, name='x'):
    """fp32 [B, T, C] with dense channels -> (tensor, batch stride, token stride); a token or channel slice of a wider buffer stays a view."""
    H.need_device(who, t)
    if t.dim() != 3 or t.dtype != torch.float32 or (t.shape[2] > 1 and t.stride(2) != 1):
        raise ValueError(f'{who}: {name} must be fp32 [B, T, C] with dense channels, got {tuple(t.shape)} {t.dtype} strides {t.stride()}')
    B, T, Cc = t.shape
    ts = t.stride(1) if T > 1 else Cc
    return t, (t.stride(0) if B > 1 else max(T, 1) * ts), ts


def _gemm(who, B, T, N, K, x, x_bs, x_ts, w, bias, y, y_bs, y_ts, epilogue=EPI_NONE, res=None, r_bs=0, r_ts=0, scale=None, dev=None):
    a = L.WavlmGemmArgs()
    a.B, a.T, a.N, a.K, a.groups, a.seg_len, a.epilogue = B, T, N, K, 1, 0, int(epilogue)
    if scale is not None:
        a.scale_lo, a.scale_hi, a.scale = int(scale[0]), int(scale[1]), float(scale[2])
    a.x, a.x_bs, a.x_ts = x, x_bs, x_ts
    a.w, a.bias = w.data_ptr(), H.ptr(bias)
    if res is not None:
        a.res, a.r_bs, a.r_ts = res, r_bs, r_ts
    a.y, a.y_bs, a.y_ts = y, y_bs, y_ts
    H.check(who, L.lib().tdvc_wavlm_gemm(C.byref(a), H.stream(w)))


def wavlm_gemm(x, weight, bias=None, epilogue=EPI_NONE, residual=None, out=None, scale=None, kernel=1, stride=1):
    """tdvc_wavlm_gemm: x [B, T, Cin] (a view with dense channels), weight [N, kernel Cin] -> out [B, T', N] =
    epilogue((A W^T + bias) scale) [+ residual], T' = (T - kernel) // stride + 1; row t' of A is the kernel consecutive tokens from
    stride t' (kernel > 1 needs a token stride of exactly Cin). epilogue EPI_NONE | EPI_GELU; scale = (lo, hi, value) multiplies the
    columns lo <= n < hi; residual may be `out` itself; `out` may be a view into a wider (padded) buffer."""
    who = 'wavlm_gemm'
    x, x_bs, x_ts = _tok3(who, x)
    B, T, Cin = x.shape
    H.need_device(who, weight)
    kernel, stride = int(kernel), int(stride)
    if weight.dim() != 2 or weight.dtype != torch.float32 or not weight.is_contiguous() or weight.shape[1] != kernel * Cin:
        raise ValueError(f'{who}: weight must be contiguous fp32 [N, {kernel * Cin}], got {tuple(weight.shape)}')
    if kernel < 1 or stride < 1 or (kernel > 1 and T > 1 and x_ts != Cin):
        raise ValueError(f'{who}: a kernel of {kernel} tokens needs kernel, stride >= 1 and consecutive tokens (token stride {Cin})')
    if T < kernel:
        raise ValueError(f'{who}: {T} tokens are fewer than the kernel {kernel}')
    N, To = weight.shape[0], (T - kernel) // stride + 1
    bias = None if bias is None else H.vec(who, bias, N, 'bias')
    if out is None:
        out = torch.empty(B, To, N, dtype=torch.float32, device=x.device)
    out, y_bs, y_ts = _tok3(who, out, 'out')
    if tuple(out.shape) != (B, To, N):
        raise ValueError(f'{who}: out must be [{B}, {To}, {N}], got {tuple(out.shape)}')
    r = (None, 0, 0)
    if residual is not None:
        residual, r_bs, r_ts = _tok3(who, residual, 'residual')
        if residual.shape != out.shape:
            raise ValueError(f'{who}: residual must have the shape of out')
        r = (residual.data_ptr(), r_bs, r_ts)
    _gemm(who, B, To, N, kernel * Cin, x.data_ptr(), x_bs, stride * x_ts, weight, bias, out.data_ptr(), y_bs, y_ts, epilogue, *r, scale=scale)
    return out


def wavlm_conv0(signal, weight_t, gamma, beta, stride, out=None):
    """tdvc_wavlm_conv0: signal [B, L] | [B, 1, L] | [L], weight_t [k, C] (the Conv1d weight [C, 1, k] transposed) ->
    gelu(LN(conv)) fp32 [B, (L - k) // stride + 1, C]."""
    who = 'wavlm_conv0'
    H.need_device(who, signal, weight_t)
    x2, bs, _ = H.rows2(who, signal)
    B, Ln = x2.shape
    if weight_t.dim() != 2 or weight_t.dtype != torch.float32 or not weight_t.is_contiguous():
        raise ValueError(f'{who}: weight_t must be contiguous fp32 [k, C]')
    k, Cc = weight_t.shape
    if Ln < k:
        raise ValueError(f'{who}: a row of {Ln} samples is shorter than the kernel {k}')
    T = (Ln - k) // int(stride) + 1
    gamma, beta = H.vec(who, gamma, Cc, 'gamma'), H.vec(who, beta, Cc, 'beta')
    if out is None:
        out = torch.empty(B, T, Cc, dtype=torch.float32, device=x2.device)
    out, y_bs, y_ts = _tok3(who, out, 'out')
    if tuple(out.shape) != (B, T, Cc):
        raise ValueError(f'{who}: out must be [{B}, {T}, {Cc}]')
    H.check(who, L.lib().tdvc_wavlm_conv0(x2.data_ptr(), bs, B, Ln, weight_t.data_ptr(), k, int(stride), Cc, gamma.data_ptr(), beta.data_ptr(),
                                          out.data_ptr(), y_bs, y_ts, H.stream(x2)))
    return out


def wavlm_layernorm(x, gamma, beta, gelu=False, out=None, grep=None):
    """tdvc_wavlm_layernorm: x [B, T, C] -> LN(x) (eps 1e-5), with gelu the erf-GELU of it; `out` may be x. grep = (grep_linear weight
    [8, d], bias [8], grep_a [H]) also returns the gates fp32 [B, H, T] of the relative position bias."""
    who = 'wavlm_layernorm'
    x, x_bs, x_ts = _tok3(who, x)
    B, T, Cc = x.shape
    gamma, beta = H.vec(who, gamma, Cc, 'gamma'), H.vec(who, beta, Cc, 'beta')
    if out is None:
        out = torch.empty(B, T, Cc, dtype=torch.float32, device=x.device)
    out, y_bs, y_ts = _tok3(who, out, 'out')
    if out.shape != x.shape:
        raise ValueError(f'{who}: out must have the shape of x')
    Hh, gw, gb, ga, gate = 0, None, None, None, None
    if grep is not None:
        Hh = grep[2].numel()
        if Hh < 1 or Cc % Hh:
            raise ValueError(f'{who}: {Cc} channels do not divide into {Hh} heads')
        gw, gb, ga = H.vec(who, grep[0], 8 * (Cc // Hh), 'grep_linear.weight'), H.vec(who, grep[1], 8, 'grep_linear.bias'), H.vec(who, grep[2], Hh, 'grep_a')
        gate = torch.empty(B, Hh, T, dtype=torch.float32, device=x.device)
    H.check(who, L.lib().tdvc_wavlm_layernorm(x.data_ptr(), x_bs, x_ts, B, T, Cc, gamma.data_ptr(), beta.data_ptr(), int(bool(gelu)), out.data_ptr(),
                                              y_bs, y_ts, Hh, H.ptr(gw), H.ptr(gb), H.ptr(ga), H.ptr(gate), H.stream(x)))
    return out if grep is None else (out, gate)


def wavlm_posconv(xp, weight, bias, kernel, groups, out=None):
    """tdvc_wavlm_posconv: xp [B, T + kernel - 1, C] contiguous rows (the row behind kernel // 2 zero tokens, kernel // 2 - 1 behind
    it), weight [C, kernel, C / groups] from fold_pos_conv -> out[b, t] = xp[b, t + kernel // 2] + gelu(conv + bias), [B, T, C]."""
    who = 'wavlm_posconv'
    xp, x_bs, x_ts = _tok3(who, xp, 'xp')
    B, Tp, Cc = xp.shape
    kernel, groups = int(kernel), int(groups)
    T = Tp - kernel + 1
    if T < 0 or (Tp > 1 and x_ts != Cc):
        raise ValueError(f'{who}: xp must hold T + {kernel - 1} consecutive tokens')
    H.need_device(who, weight)
    if weight.dtype != torch.float32 or not weight.is_contiguous() or groups < 1 or Cc % groups or tuple(weight.shape) != (Cc, kernel, Cc // groups):
        raise ValueError(f'{who}: weight must be contiguous fp32 [{Cc}, {kernel}, C / groups], got {tuple(weight.shape)}')
    bias = H.vec(who, bias, Cc, 'bias')
    if out is None:
        out = torch.empty(B, T, Cc, dtype=torch.float32, device=xp.device)
    out, y_bs, y_ts = _tok3(who, out, 'out')
    if tuple(out.shape) != (B, T, Cc):
        raise ValueError(f'{who}: out must be [{B}, {T}, {Cc}]')
    H.check(who, L.lib().tdvc_wavlm_posconv(xp.data_ptr(), x_bs, B, T, Cc, kernel, groups, weight.data_ptr(), bias.data_ptr(), out.data_ptr(), y_bs, y_ts,
                                            H.stream(xp)))
    return out


def wavlm_attention(qkv, heads, gate, bias_rel, out=None):
    """tdvc_wavlm_attention: qkv [B, T, 3 C] (q | k | v, q already scaled), gate [B, H, T], bias_rel [H, 2 T - 1] -> [B, T, C]."""
    who = 'wavlm_attention'
    qkv, bs, ts = _tok3(who, qkv, 'qkv')
    B, T, C3 = qkv.shape
    heads = int(heads)
    if heads < 1 or C3 % (3 * heads):
        raise ValueError(f'{who}: qkv of width {C3} does not hold 3 x {heads} heads')
    Cc = C3 // 3
    H.need_device(who, gate, bias_rel)
    if tuple(gate.shape) != (B, heads, T) or gate.dtype != torch.float32 or not gate.is_contiguous():
        raise ValueError(f'{who}: gate must be contiguous fp32 [{B}, {heads}, {T}]')
    if tuple(bias_rel.shape) != (heads, max(2 * T - 1, 0)) or bias_rel.dtype != torch.float32 or not bias_rel.is_contiguous():
        raise ValueError(f'{who}: bias_rel must be contiguous fp32 [{heads}, {2 * T - 1}]')
    if out is None:
        out = torch.empty(B, T, Cc, dtype=torch.float32, device=qkv.device)
    out, o_bs, o_ts = _tok3(who, out, 'out')
    if tuple(out.shape) != (B, T, Cc):
        raise ValueError(f'{who}: out must be [{B}, {T}, {Cc}]')
    p = qkv.data_ptr()
    H.check(who, L.lib().tdvc_wavlm_attention(p, p + 4 * Cc, p + 8 * Cc, bs, ts, B, T, heads, Cc // heads, gate.data_ptr(), bias_rel.data_ptr(),
                                              out.data_ptr(), o_bs, o_ts, H.stream(qkv)))
    return out


# -------------------------------------------------------------------------------------------------------------------- module
class _PosConv(torch.nn.Module):
    """nn.utils.weight_norm(nn.Conv1d(C, C, K, padding=K // 2, groups=G), name='weight', dim=2): bias, weight_g [1, 1, K], weight_v."""

    def __init__(self, c, k, groups):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.zeros(c))
        self.weight_g = torch.nn.Parameter(torch.ones(1, 1, k))
        self.weight_v = torch.nn.Parameter(torch.empty(c, c // groups, k).normal_(0.0, math.sqrt(4.0 / (k * c))))


class _Attn(torch.nn.Module):
    def __init__(self, c, heads, num_buckets, has_bias):
        super().__init__()
        if has_bias:
            self.relative_attention_bias = torch.nn.Embedding(num_buckets, heads)
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (torch.nn.Linear(c, c) for _ in range(4))
        self.grep_linear = torch.nn.Linear(c // heads, 8)
        self.grep_a = torch.nn.Parameter(torch.ones(1, heads, 1, 1))


class _Layer(torch.nn.Module):
    def __init__(self, c, ffn, heads, num_buckets, has_bias):
        super().__init__()
        self.self_attn = _Attn(c, heads, num_buckets, has_bias)
        self.self_attn_layer_norm = torch.nn.LayerNorm(c)
        self.fc1 = torch.nn.Linear(c, ffn)
        self.fc2 = torch.nn.Linear(ffn, c)
        self.final_layer_norm = torch.nn.LayerNorm(c)


class _Encoder(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c = cfg.encoder_embed_dim
        self.pos_conv = torch.nn.Sequential(_PosConv(c, cfg.conv_pos, cfg.conv_pos_groups))
        self.layers = torch.nn.ModuleList([_Layer(c, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.num_buckets, i == 0)
                                           for i in range(cfg.encoder_layers)])
        self.layer_norm = torch.nn.LayerNorm(c)


class _Extractor(torch.nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.conv_layers = torch.nn.ModuleList()
        cin = 1
        for dim, k, s in layers:      # the reference's block: conv, dropout, (transpose, LayerNorm, transpose), GELU -> keys 0.weight, 2.1.*
            self.conv_layers.append(torch.nn.Sequential(torch.nn.Conv1d(cin, dim, k, stride=s, bias=False), torch.nn.Identity(),
                                                        torch.nn.Sequential(torch.nn.Identity(), torch.nn.LayerNorm(dim), torch.nn.Identity()),
                                                        torch.nn.Identity()))
            cin = dim


def _outside(cfg):
    """What of cfg lies outside the definition, as a list of strings."""
    bad = []
    for name, want in (('extractor_mode', 'layer_norm'), ('layer_norm_first', True), ('relative_position_embedding', True), ('gru_rel_pos', True),
                       ('conv_bias', False), ('activation_fn', 'gelu')):
        if getattr(cfg, name) != want:
            bad.append(f'{name}={getattr(cfg, name)!r} (only {want!r})')
    layers = conv_layers(cfg)
    c, heads = cfg.encoder_embed_dim, cfg.encoder_attention_heads
    if any(dim % 16 or dim > 1024 for dim, _, _ in layers):
        bad.append('convolution widths that are not multiples of 16 up to 1024')
    if layers and layers[0][1] > 64:
        bad.append('a first convolution of more than 64 taps')
    if layers and layers[-1][0] == c:
        bad.append('a front end as wide as the encoder (no post_extract_proj)')
    if c % 16 or c > 1024 or cfg.encoder_ffn_embed_dim % 16:
        bad.append('encoder widths that are not multiples of 16 (encoder_embed_dim up to 1024)')
    if heads < 1 or c % heads or c // heads not in (16, 32, 64):
        bad.append(f'a head width of {c / max(heads, 1):g} (only 16, 32, 64)')
    if cfg.conv_pos % 2 or cfg.conv_pos_groups < 1 or c % cfg.conv_pos_groups or (c // cfg.conv_pos_groups) % 16:
        bad.append('conv_pos odd, or encoder_embed_dim / conv_pos_groups not a multiple of 16')
    return bad


class WavLM(torch.nn.Module):
    """The reference's WavLM (W:220): the same state_dict keys and shapes, mask_emb, encoder.pos_conv.0.weight_g/_v and layer 0's
    relative_attention_bias included, so that checkpoint['model'] loads with strict=True. The stock modules are containers for the
    parameters and are never called: `extract_features` runs csrc/ssl_wavlm.hip. The packed weights (q|k|v, permuted convolutions,
    the folded positional convolution) are derived, per device, rebuilt after load_state_dict or a move, and not in the state dict.
    Inference only; parity with a real WavLM-Large.pt is unchecked (the checkpoint is absent)."""

    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg if isinstance(cfg, WavLMConfig) else WavLMConfig(cfg)
        bad = _outside(cfg)
        if bad:
            raise NotImplementedError('WavLM: outside the definition: ' + '; '.join(bad))
        self.cfg = cfg
        self.conv_spec = conv_layers(cfg)
        self.embed = self.conv_spec[-1][0]
        c = cfg.encoder_embed_dim
        self.feature_extractor = _Extractor(self.conv_spec)
        self.post_extract_proj = torch.nn.Linear(self.embed, c)
        self.mask_emb = torch.nn.Parameter(torch.empty(c).uniform_())
        self.encoder = _Encoder(cfg)
        self.layer_norm = torch.nn.LayerNorm(self.embed)
        self._packed, self._tables, self._work = {}, {}, {}
        self.eval()

    def _forget(self):
        self._packed, self._tables, self._work = {}, {}, {}

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._forget()
        return out

    def _apply(self, fn, *args, **kwargs):
        self._forget()
        return super()._apply(fn, *args, **kwargs)

    def num_frames(self, n):
        return frame_count(int(n), self.conv_spec)

    # ---- derived buffers
    def _pack(self, device):
        key = H.dev_key(device)
        if key not in self._packed:
            f = lambda t: t.detach().float().contiguous()
            cl = self.feature_extractor.conv_layers
            p = dict(conv0=f(cl[0][0].weight[:, 0, :].t()), convs=[permute_conv(m[0].weight) for m in list(cl)[1:]],
                     pos=fold_pos_conv(self.encoder.pos_conv[0].weight_g, self.encoder.pos_conv[0].weight_v), layers=[])
            for lay in self.encoder.layers:
                a = lay.self_attn
                p['layers'].append(dict(w=f(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])),
                                        b=f(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])), grep_a=f(a.grep_a.reshape(-1))))
            self._packed[key] = p
        return self._packed[key]

    def bias_table(self, T, device):
        """bias_rel fp32 [H, 2 T - 1] on the device: relative_attention_bias.weight[bucket(s - t)][n] at [n][s - t + T - 1]."""
        key = (int(T), H.dev_key(device))
        if key not in self._tables:
            idx = relative_buckets(torch.arange(-(T - 1), T), self.cfg.num_buckets, self.cfg.max_distance).to(device)
            w = self.encoder.layers[0].self_attn.relative_attention_bias.weight.detach().float()
            self._tables[key] = w[idx].t().contiguous()
        return self._tables[key]

    def _workspace(self, B, Ln, device):
        key = (B, Ln, H.dev_key(device))
        if key not in self._work:
            counts, n = [], Ln
            for _, k, s in self.conv_spec:
                n = (n - k) // s + 1 if n >= k else 0
                counts.append(n)
            T, c, kp = counts[-1], self.cfg.encoder_embed_dim, self.cfg.conv_pos
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)
            self._work[key] = dict(counts=counts, feats=[new(B, counts[i], self.conv_spec[i][0]) for i in range(len(counts))],
                                   xp=torch.zeros(B, T + kp - 1, c, dtype=torch.float32, device=device), x=new(B, T, c), h=new(B, T, c),
                                   qkv=new(B, T, 3 * c), att=new(B, T, c), ffn=new(B, T, self.cfg.encoder_ffn_embed_dim))
        return self._work[key]

    # ---- the call
    def extract_features(self, source, padding_mask=None, mask=False, ret_conv=False, output_layer=None, ret_layer_results=False):
        """source [B, L] (device fp32) -> (features fp32 [B, L', C], None), the reference's signature (W:324). mask=True, a padding_mask
        and ret_layer_results=True raise NotImplementedError. ret_conv=True returns post_extract_proj's output; output_layer=k the
        output of layer k (1-based) without the final norm. The result is a new tensor; the intermediates live in a workspace cached
        per (B, L)."""
        who = 'WavLM.extract_features'
        if mask:
            raise NotImplementedError(f'{who}: mask=True (masking is a training-time step; the definition is eval mode with mask=False)')
        if padding_mask is not None:
            raise NotImplementedError(f'{who}: a padding_mask (rows are full length: there are no per-row lengths)')
        if ret_layer_results:
            raise NotImplementedError(f'{who}: ret_layer_results=True (ask for one layer with output_layer=k)')
        nl = len(self.encoder.layers)
        if output_layer is not None and not 1 <= int(output_layer) <= nl:
            raise NotImplementedError(f'{who}: output_layer={output_layer} (layers are 1..{nl})')
        H.need_device(who, source, self.mask_emb)
        if source.dim() != 2:
            raise ValueError(f'{who}: source must be [B, L], got {tuple(source.shape)}')
        x2, _, _ = H.rows2(who, source)
        B, Ln = x2.shape
        cfg, spec = self.cfg, self.conv_spec
        T = frame_count(Ln, spec)
        if T < 1:
            raise ValueError(f'{who}: a row of {Ln} samples has no frame (the front end needs {self.min_samples()})')
        if T > 4096:
            raise ValueError(f'{who}: {T} frames; the attention kernel takes up to 4096 (82 s)')
        c, heads, kp = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.conv_pos
        if B == 0:
            return torch.empty(0, T, c, dtype=torch.float32, device=x2.device), None
        pk, ws = self._pack(x2.device), self._workspace(B, Ln, x2.device)
        cl = self.feature_extractor.conv_layers
        feats = ws['feats']
        wavlm_conv0(x2, pk['conv0'], cl[0][2][1].weight, cl[0][2][1].bias, spec[0][2], out=feats[0])
        for i in range(1, len(spec)):
            wavlm_gemm(feats[i - 1], pk['convs'][i - 1], kernel=spec[i][1], stride=spec[i][2], out=feats[i])
            wavlm_layernorm(feats[i], cl[i][2][1].weight, cl[i][2][1].bias, gelu=True, out=feats[i])
        f = wavlm_layernorm(feats[-1], self.layer_norm.weight, self.layer_norm.bias, out=feats[-1])
        xp = ws['xp']
        inner = xp[:, kp // 2:kp // 2 + T]
        wavlm_gemm(f, self.post_extract_proj.weight.detach().float().contiguous(), self.post_extract_proj.bias, out=inner)
        if ret_conv:
            return inner.clone(), None
        pc = self.encoder.pos_conv[0]
        x, h = ws['x'], ws['h']
        wavlm_posconv(xp, pk['pos'], pc.bias, kp, cfg.conv_pos_groups, out=x)
        table = self.bias_table(T, x2.device)
        scale = (0, c, float(c // heads) ** -0.5)
        for li, lay in enumerate(self.encoder.layers):
            a, pl = lay.self_attn, pk['layers'][li]
            _, gate = wavlm_layernorm(x, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias, out=h,
                                      grep=(a.grep_linear.weight, a.grep_linear.bias, pl['grep_a']))
            wavlm_gemm(h, pl['w'], pl['b'], scale=scale, out=ws['qkv'])
            wavlm_attention(ws['qkv'], heads, gate, table, out=ws['att'])
            wavlm_gemm(ws['att'], a.out_proj.weight.detach().float().contiguous(), a.out_proj.bias, residual=x, out=x)
            wavlm_layernorm(x, lay.final_layer_norm.weight, lay.final_layer_norm.bias, out=h)
            wavlm_gemm(h, lay.fc1.weight.detach().float().contiguous(), lay.fc1.bias, epilogue=EPI_GELU, out=ws['ffn'])
            wavlm_gemm(ws['ffn'], lay.fc2.weight.detach().float().contiguous(), lay.fc2.bias, residual=x, out=x)
            if output_layer is not None and li + 1 == int(output_layer):
                return x.clone(), None
        return wavlm_layernorm(x, self.encoder.layer_norm.weight, self.encoder.layer_norm.bias), None

    def min_samples(self):
        n = 1
        for _, k, s in reversed(self.conv_spec):
            n = (n - 1) * s + k
        return n

    def forward(self, source, **kwargs):
        return self.extract_features(source, **kwargs)[0]


def load_wavlm(path, device='cpu'):
    """The reference's checkpoint {'cfg': dict, 'model': state dict} (wavlm/WavLM-Large.pt) -> WavLM(WavLMConfig(cfg)) with the state
    dict loaded strictly, in eval mode on `device`."""
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(ckpt, dict) or 'cfg' not in ckpt or 'model' not in ckpt:
        raise ValueError("load_wavlm: a WavLM checkpoint is a dict with 'cfg' and 'model'")
    model = WavLM(WavLMConfig(ckpt['cfg']))
    model.load_state_dict(ckpt['model'], strict=True)
    return model.to(device).eval()
