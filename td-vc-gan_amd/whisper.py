"""The Whisper ASR metric on the device: the intelligibility score of the reference's test_scripts/common/test_asr.py, which takes
greedy transcripts from HF `WhisperForConditionalGeneration("openai/whisper-medium").generate` with a forced language and task and
then WER and CER over them. `Whisper(cfg)` has HF's state-dict keys and shapes (`model.encoder.*`, `model.decoder.*`; a tied
`proj_out.weight` is accepted and checked) and loads strictly; `whisper_log_mel` is WhisperFeatureExtractor's numpy path; `encode`,
`generate` and `transcribe` run csrc/asr_whisper.hip on top of tdvc_wavlm_gemm and tdvc_wavlm_layernorm; `asr_wer`, `asr_cer` and
`asr_report` are host functions on strings. The definition (include/tdvc.h, "The Whisper ASR metric") is pinned to HF's own float64
output on a small seeded configuration (tests/golden/whisper_small.npz, tools/make_golden_whisper.py) and restated in float64 in
tests/whisper_ref.py. No checkpoint is available and none is shipped: **parity with a real whisper-medium checkpoint is unchecked**.

What is not here: the tokenizer and Whisper's text normaliser (ids in, ids out; `transcribe` returns strings only through a caller's
object with `.decode`), beam search, temperature fallback, timestamps, long-form chunking (audio past chunk_length is truncated, as in
the reference), scale_embedding=True, and d_model above 1024 (whisper-large, d = 1280, is refused); head widths are 16, 32 or 64.

The decoder step reads its position from a device counter: one step is the same launch sequence at every position, `generate` never
synchronises with the host (check_every=k opts into one flag read every k steps) and replays one captured graph per step by default.
A launch takes up to 16 rows; larger batches are split on the host. No CPU or ATen fallback, no atomics, fixed summation orders."""
import ctypes as C

import numpy as np
import torch

from . import _host as H
from . import _lib as L
from .wavlm import EPI_GELU, EPI_NONE, _gemm, _tok3, permute_conv, wavlm_gemm, wavlm_layernorm

SAMPLE_RATE, N_FFT, HOP, BINS, STEP_ROWS = 16000, 400, 160, 201, 16
MEDIUM = dict(vocab_size=51865, num_mel_bins=80, d_model=1024, encoder_layers=24, decoder_layers=24, encoder_attention_heads=16,
              decoder_attention_heads=16, encoder_ffn_dim=4096, decoder_ffn_dim=4096, max_source_positions=1500, max_target_positions=448,
              activation_function='gelu', scale_embedding=False, pad_token_id=50257, bos_token_id=50257, eos_token_id=50257,
              decoder_start_token_id=50258)


class WhisperConfig:
    """HF's WhisperConfig field names, so that WhisperConfig(json.load(open('config.json'))) works; unknown fields are kept. The
    defaults are whisper-medium's."""

    def __init__(self, cfg=None, **kw):
        self.__dict__.update(MEDIUM)
        if cfg is not None:
            self.__dict__.update(cfg.__dict__ if isinstance(cfg, WhisperConfig) else cfg)
        self.__dict__.update(kw)


def _outside(cfg):
    bad = []
    d = cfg.d_model
    if cfg.activation_function != 'gelu':
        bad.append(f'activation_function={cfg.activation_function!r} (only gelu)')
    if cfg.scale_embedding:
        bad.append('scale_embedding=True')
    if d % 16 or d > 1024:
        bad.append(f'd_model={d} (a multiple of 16 up to 1024; whisper-large is outside)')
    for h in (cfg.encoder_attention_heads, cfg.decoder_attention_heads):
        if h < 1 or d % h or d // h not in (16, 32, 64):
            bad.append(f'a head width of {d / max(h, 1):g} (only 16, 32, 64)')
    if cfg.encoder_ffn_dim % 16 or cfg.decoder_ffn_dim % 16 or cfg.num_mel_bins % 16 or cfg.num_mel_bins > 128:
        bad.append('FFN widths or mel bands that are not multiples of 16 (mel bands up to 128)')
    if cfg.max_source_positions > 4096:
        bad.append('more than 4096 encoder positions')
    return bad


# ------------------------------------------------------------------------------------------------------------------ features
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), 200.0 * m / 3.0)


def whisper_mel_filters(n_mels=80):
    """float64 [201, n_mels]: HF's mel_filter_bank(201, n_mels, 0, 8000, 16000, norm='slaney', mel_scale='slaney')."""
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(8000.0), n_mels + 2))
    bins = np.linspace(0.0, SAMPLE_RATE // 2, BINS)
    width = np.diff(edges)
    slopes = edges[None, :] - bins[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / width[:-1], slopes[:, 2:] / width[1:]))
    return fb * (2.0 / (edges[2:] - edges[:-2]))[None, :]


def _mel_table(n_mels, device):
    build = lambda: np.concatenate([H.dft_tables(N_FFT, (0.5, 0.5)), whisper_mel_filters(n_mels).T.reshape(-1)])
    return H.device_table(device, ('whisper_mel', int(n_mels)), build)


def whisper_log_mel(signal, lengths=None, chunk_length=30, n_mels=80, out=None):
    """tdvc_whisper_log_mel: signal [B, L] | [L] at 16 kHz -> input_features fp32 [B, n_mels, chunk_length 100]. The row is zero-padded
    or truncated to chunk_length seconds; lengths [B] (device) mark where the zeros start, and samples behind them are never read.
    `out` may be any fp32 [B, n_mels, frames] view (the encoder passes a token-major one)."""
    who = 'whisper_log_mel'
    H.need_device(who, signal)
    x2, bs, _ = H.rows2(who, signal)
    B, Ln = x2.shape
    n_samples = int(chunk_length) * SAMPLE_RATE
    if chunk_length < 1 or n_samples > (1 << 28):
        raise ValueError(f'{who}: chunk_length must be 1 .. 16777 seconds')
    lengths = H.device_lengths(who, lengths, B, x2.device)
    frames = n_samples // HOP
    if out is None:
        out = torch.empty(B, n_mels, frames, dtype=torch.float32, device=x2.device)
    H.need_device(who, out)
    if tuple(out.shape) != (B, n_mels, frames) or out.dtype != torch.float32:
        raise ValueError(f'{who}: out must be fp32 [{B}, {n_mels}, {frames}]')
    table = _mel_table(n_mels, x2.device)
    nbytes = L.lib().tdvc_whisper_log_mel_workspace(B, n_samples, n_mels)
    ws = H.scratch(nbytes, x2.device)
    H.check(who, L.lib().tdvc_whisper_log_mel(x2.data_ptr(), bs, H.ptr(lengths), B, Ln, n_samples, table.data_ptr(), n_mels, out.data_ptr(),
                                              out.stride(0) if B > 1 else 0, out.stride(1), out.stride(2), ws.data_ptr(), nbytes, H.stream(x2)))
    return out


# ----------------------------------------------------------------------------------------------------------------- operators
def whisper_attention(qkv, heads, out=None):
    """tdvc_whisper_attention: qkv [B, T, 3 C] (q | k | v, q already scaled) -> softmax(q k^T) v, [B, T, C]."""
    who = 'whisper_attention'
    qkv, bs, ts = _tok3(who, qkv, 'qkv')
    B, T, C3 = qkv.shape
    heads = int(heads)
    if heads < 1 or C3 % (3 * heads):
        raise ValueError(f'{who}: qkv of width {C3} does not hold 3 x {heads} heads')
    Cc = C3 // 3
    if out is None:
        out = torch.empty(B, T, Cc, dtype=torch.float32, device=qkv.device)
    out, o_bs, o_ts = _tok3(who, out, 'out')
    if tuple(out.shape) != (B, T, Cc):
        raise ValueError(f'{who}: out must be [{B}, {T}, {Cc}]')
    p = qkv.data_ptr()
    H.check(who, L.lib().tdvc_whisper_attention(p, p + 4 * Cc, p + 8 * Cc, bs, ts, B, T, heads, Cc // heads, out.data_ptr(), o_bs, o_ts, H.stream(qkv)))
    return out


def _rows(who, t, name, width=None):
    """fp32 [B, N] with a dense last axis -> (tensor, row stride)."""
    H.need_device(who, t)
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or (width is not None and t.shape[1] != width):
        raise ValueError(f'{who}: {name} must be fp32 [B, {width if width is not None else "N"}] with a dense last axis, got {tuple(t.shape)} {t.dtype}')
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _counter(who, pos):
    H.need_device(who, pos)
    if pos.dtype != torch.int32 or pos.numel() != 1:
        raise ValueError(f'{who}: the position counter is one int32 on the device')
    return pos


def whisper_embed(ids, pos, embed_tokens, embed_positions, out=None):
    """tdvc_whisper_embed: ids int32 [B, L], pos the device counter -> embed_tokens[ids[:, p]] + embed_positions[p], [B, d]."""
    who = 'whisper_embed'
    H.need_device(who, ids, embed_tokens, embed_positions)
    _counter(who, pos)
    if ids.dim() != 2 or ids.dtype != torch.int32 or (ids.shape[1] > 1 and ids.stride(1) != 1):
        raise ValueError(f'{who}: ids must be int32 [B, L] with a dense last axis')
    B, Lm = ids.shape
    V, d = embed_tokens.shape
    if not (embed_tokens.is_contiguous() and embed_positions.is_contiguous() and embed_tokens.dtype == embed_positions.dtype == torch.float32):
        raise ValueError(f'{who}: the embeddings must be contiguous fp32')
    if embed_positions.shape[1] != d or embed_positions.shape[0] < Lm:
        raise ValueError(f'{who}: embed_positions must be [>= {Lm}, {d}]')
    if out is None:
        out = torch.empty(B, d, dtype=torch.float32, device=ids.device)
    out, x_bs = _rows(who, out, 'out', d)
    H.check(who, L.lib().tdvc_whisper_embed(ids.data_ptr(), ids.stride(0) if B > 1 else Lm, pos.data_ptr(), Lm, embed_tokens.data_ptr(),
                                            embed_positions.data_ptr(), B, d, V, out.data_ptr(), x_bs, H.stream(ids)))
    return out


def whisper_linear_step(x, weight, bias=None, norm=None, epilogue=EPI_NONE, residual=None, out=None, scale=None, cache=None):
    """tdvc_whisper_linear_step: x [B <= 16, K], weight [N, K] -> epilogue((LN?(x) W^T + bias) scale) [+ residual], [B, N].
    norm = (gamma, beta): the LayerNorm prologue. scale = (lo, hi, value) multiplies the columns lo <= n < hi. cache = (k_cache, v_cache,
    pos, first): the columns from `first` are k | v and go to cache[b, p] (caches fp32 [B, len, w] contiguous per row, pos the device
    counter) instead of `out`, which then is [B, first]. residual may be `out`."""
    who = 'whisper_linear_step'
    x, x_bs = _rows(who, x, 'x')
    B, K = x.shape
    H.need_device(who, weight)
    if weight.dim() != 2 or weight.dtype != torch.float32 or not weight.is_contiguous() or weight.shape[1] != K:
        raise ValueError(f'{who}: weight must be contiguous fp32 [N, {K}], got {tuple(weight.shape)}')
    N = weight.shape[0]
    a = L.WhisperLinearArgs()
    a.B, a.N, a.K, a.epilogue = B, N, K, int(epilogue)
    if scale is not None:
        a.scale_lo, a.scale_hi, a.scale = int(scale[0]), int(scale[1]), float(scale[2])
    a.x, a.x_bs, a.w = x.data_ptr(), x_bs, weight.data_ptr()
    keep = [x, weight]
    if bias is not None:
        keep.append(H.vec(who, bias, N, 'bias'))
        a.bias = keep[-1].data_ptr()
    if norm is not None:
        keep += [H.vec(who, norm[0], K, 'gamma'), H.vec(who, norm[1], K, 'beta')]
        a.gamma, a.beta = keep[-2].data_ptr(), keep[-1].data_ptr()
    ny = N
    if cache is not None:
        kc, vc, pos, first = cache
        H.need_device(who, kc, vc)
        _counter(who, pos)
        ny = int(first)
        w = (N - ny) // 2
        if kc.shape != vc.shape or kc.dim() != 3 or kc.shape[0] != B or kc.shape[2] != w or kc.dtype != torch.float32 or vc.dtype != torch.float32 \
                or kc.stride()[1:] != (w, 1) or vc.stride() != kc.stride():
            raise ValueError(f'{who}: the caches must be fp32 [{B}, len, {w}] with contiguous rows and equal strides')
        a.cache_lo, a.cache_len, a.pos, a.k_cache, a.v_cache = ny, kc.shape[1], pos.data_ptr(), kc.data_ptr(), vc.data_ptr()
        a.c_bs = kc.stride(0) if B > 1 else kc.shape[1] * w
    if out is None:
        out = torch.empty(B, ny, dtype=torch.float32, device=x.device)
    out, y_bs = _rows(who, out, 'out', ny)
    if out.shape[0] != B:
        raise ValueError(f'{who}: out must have {B} rows')
    a.y, a.y_bs = out.data_ptr(), y_bs
    if residual is not None:
        residual, r_bs = _rows(who, residual, 'residual', N)
        a.res, a.r_bs = residual.data_ptr(), r_bs
    H.check(who, L.lib().tdvc_whisper_linear_step(C.byref(a), H.stream(x)))
    return out


def whisper_attn_step(q, k, v, heads, pos=None, out=None):
    """tdvc_whisper_attn_step: q [B <= 16, C], k, v [B, len, C] views with dense channels and equal strides -> [B, C]: one query per
    (row, head) against the keys 0 .. p (pos, the device counter) or all len keys (pos None). Keys behind them are never read."""
    who = 'whisper_attn_step'
    q, q_bs = _rows(who, q, 'q')
    B, Cc = q.shape
    k, kv_bs, kv_ts = _tok3(who, k, 'k')
    v, v_bs, v_ts = _tok3(who, v, 'v')
    if k.shape != v.shape or k.shape[0] != B or k.shape[2] != Cc or (v_bs, v_ts) != (kv_bs, kv_ts):
        raise ValueError(f'{who}: k and v must be [{B}, len, {Cc}] with equal strides')
    heads = int(heads)
    if heads < 1 or Cc % heads:
        raise ValueError(f'{who}: {Cc} channels do not divide into {heads} heads')
    if k.shape[1] < 1:
        raise ValueError(f'{who}: no key')
    if pos is not None:
        _counter(who, pos)
    if out is None:
        out = torch.empty(B, Cc, dtype=torch.float32, device=q.device)
    out, o_bs = _rows(who, out, 'out', Cc)
    H.check(who, L.lib().tdvc_whisper_attn_step(q.data_ptr(), q_bs, k.data_ptr(), v.data_ptr(), kv_bs, kv_ts, H.ptr(pos), k.shape[1], B, heads, Cc // heads,
                                                out.data_ptr(), o_bs, H.stream(q)))
    return out


def partial_count(vocab):
    """Partials per row that tdvc_whisper_logits writes for a vocabulary: its workgroups."""
    off = (C.c_int64 * 4)()
    L.lib().tdvc_whisper_workspace(16, 1, int(vocab), 1, 1, 1, off)
    return int(off[3])


def whisper_logits(x, gamma, beta, embed_tokens, pos, n_prompt, partials, mask=None, logits=None):
    """tdvc_whisper_logits: x [B <= 16, d] -> LN(x) embed_tokens^T. `logits` (fp32 [B, vocab] or None) receives the raw values;
    `partials` (uint8, 16 partial_count(vocab) 8 bytes) the per-workgroup (max, argmax) after the mask (uint8 [vocab]: bit 0 suppressed at
    every step, bit 1 at the step pos == n_prompt - 1)."""
    who = 'whisper_logits'
    x, x_bs = _rows(who, x, 'x')
    B, d = x.shape
    H.need_device(who, embed_tokens, partials)
    _counter(who, pos)
    if embed_tokens.dim() != 2 or embed_tokens.shape[1] != d or embed_tokens.dtype != torch.float32 or not embed_tokens.is_contiguous():
        raise ValueError(f'{who}: embed_tokens must be contiguous fp32 [vocab, {d}]')
    V = embed_tokens.shape[0]
    gamma, beta = H.vec(who, gamma, d, 'gamma'), H.vec(who, beta, d, 'beta')
    if mask is not None:
        H.need_device(who, mask)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (V,) or not mask.is_contiguous():
            raise ValueError(f'{who}: mask must be uint8 [{V}]')
    l_bs = 0
    if logits is not None:
        logits, l_bs = _rows(who, logits, 'logits', V)
    H.check(who, L.lib().tdvc_whisper_logits(x.data_ptr(), x_bs, gamma.data_ptr(), beta.data_ptr(), embed_tokens.data_ptr(), B, d, V, H.ptr(mask),
                                             pos.data_ptr(), int(n_prompt), H.ptr(logits), l_bs, partials.data_ptr(), partials.numel() * partials.element_size(),
                                             H.stream(x)))
    return logits


def whisper_pick(partials, vocab, ids, n_prompt, eos, pad, pos, n_tokens, finished, all_done):
    """tdvc_whisper_pick: the partials of tdvc_whisper_logits -> ids[:, p + 1] (int32 [B, total]), n_tokens, finished, all_done (int32
    on the device), and the counter advanced."""
    who = 'whisper_pick'
    H.need_device(who, partials, ids, n_tokens, finished, all_done)
    _counter(who, pos)
    B, total = ids.shape
    if ids.dtype != torch.int32 or (total > 1 and ids.stride(1) != 1) or any(t.dtype != torch.int32 or not t.is_contiguous() for t in (n_tokens, finished, all_done)):
        raise ValueError(f'{who}: ids, n_tokens, finished and all_done must be int32')
    if n_tokens.numel() != B or finished.numel() != B or all_done.numel() != 1:
        raise ValueError(f'{who}: n_tokens and finished are [{B}], all_done [1]')
    H.check(who, L.lib().tdvc_whisper_pick(partials.data_ptr(), partials.numel() * partials.element_size(), int(vocab), B, ids.data_ptr(),
                                           ids.stride(0) if B > 1 else total, int(n_prompt), total, int(eos), int(pad), pos.data_ptr(), n_tokens.data_ptr(),
                                           finished.data_ptr(), all_done.data_ptr(), H.stream(ids)))


# -------------------------------------------------------------------------------------------------------------------- module
class _Attn(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj = torch.nn.Linear(d, d, bias=False)
        self.v_proj, self.q_proj, self.out_proj = (torch.nn.Linear(d, d) for _ in range(3))


class _Layer(torch.nn.Module):
    def __init__(self, d, ffn, cross):
        super().__init__()
        self.self_attn = _Attn(d)
        self.self_attn_layer_norm = torch.nn.LayerNorm(d)
        if cross:
            self.encoder_attn = _Attn(d)
            self.encoder_attn_layer_norm = torch.nn.LayerNorm(d)
        self.fc1 = torch.nn.Linear(d, ffn)
        self.fc2 = torch.nn.Linear(ffn, d)
        self.final_layer_norm = torch.nn.LayerNorm(d)


class _Encoder(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.d_model
        self.conv1 = torch.nn.Conv1d(cfg.num_mel_bins, d, 3, padding=1)
        self.conv2 = torch.nn.Conv1d(d, d, 3, stride=2, padding=1)
        self.embed_positions = torch.nn.Embedding(cfg.max_source_positions, d)
        self.layers = torch.nn.ModuleList([_Layer(d, cfg.encoder_ffn_dim, False) for _ in range(cfg.encoder_layers)])
        self.layer_norm = torch.nn.LayerNorm(d)


class _Decoder(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        d = cfg.d_model
        self.embed_tokens = torch.nn.Embedding(cfg.vocab_size, d)
        self.embed_positions = torch.nn.Embedding(cfg.max_target_positions, d)
        self.layers = torch.nn.ModuleList([_Layer(d, cfg.decoder_ffn_dim, True) for _ in range(cfg.decoder_layers)])
        self.layer_norm = torch.nn.LayerNorm(d)


class _Model(torch.nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.encoder, self.decoder = _Encoder(cfg), _Decoder(cfg)


class _Step:
    """The buffers of one generate shape (B <= 16 rows, T_enc, total positions) and, once captured, the graph of one step."""

    def __init__(self, cfg, B, T_enc, total, device):
        d, nl, V = cfg.d_model, cfg.decoder_layers, cfg.vocab_size
        off = (C.c_int64 * 4)()
        nbytes = L.lib().tdvc_whisper_workspace(d, nl, V, B, T_enc, total, off)
        self.work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        if self.work.numel() < nbytes:
            raise ValueError('Whisper: workspace too small')
        f32 = lambda lo, n, *shape: self.work[lo:lo + 4 * n].view(torch.float32).view(*shape)
        self.cache = f32(int(off[0]), 2 * nl * B * total * d, nl, 2, B, total, d)
        self.cross = f32(int(off[1]), 2 * nl * B * T_enc * d, nl, B, T_enc, 2 * d)
        self.partials = self.work[int(off[2]):]
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=device)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)
        self.ids, self.pos, self.n_tokens, self.finished, self.all_done = i32(B, total), i32(1), i32(B), i32(B), i32(1)
        self.x, self.q, self.att, self.ffn = new(B, d), new(B, d), new(B, d), new(B, cfg.decoder_ffn_dim)
        self.mask = torch.zeros(V, dtype=torch.uint8, device=device)
        self.logits = None
        self.graphs = {}


class Whisper(torch.nn.Module):
    """HF's WhisperForConditionalGeneration in eval mode: the same state_dict keys and shapes (`model.encoder.*`, `model.decoder.*`),
    loaded strictly both ways; a `proj_out.weight` in the incoming dict must equal `model.decoder.embed_tokens.weight` (the tied output
    projection) and is dropped. The stock modules are containers for the parameters and are never called: everything runs in
    csrc/asr_whisper.hip and csrc/ssl_wavlm.hip. The packed weights (permuted convolutions, q|k|v with a zero bias block for k, the
    cross k|v) are derived per device and rebuilt after load_state_dict or a move. Inference only, greedy only; parity with a real
    whisper-medium checkpoint is unchecked (no checkpoint is available)."""

    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg if isinstance(cfg, WhisperConfig) else WhisperConfig(cfg)
        bad = _outside(cfg)
        if bad:
            raise NotImplementedError('Whisper: outside the definition: ' + '; '.join(bad))
        self.cfg = cfg
        self.model = _Model(cfg)
        self._packed, self._steps, self._work = {}, {}, {}
        self.eval()

    def _forget(self):
        self._packed, self._steps, self._work = {}, {}, {}

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        sd = dict(state_dict)
        if 'proj_out.weight' in sd:
            tied = sd.pop('proj_out.weight')
            emb = sd.get('model.decoder.embed_tokens.weight')
            if emb is None or tied.shape != emb.shape or not torch.equal(tied.to(emb.dtype).cpu(), emb.cpu()):
                raise RuntimeError('Whisper: proj_out.weight is not model.decoder.embed_tokens.weight (the output projection is tied)')
        out = super().load_state_dict(sd, strict=strict, **kwargs)
        self._forget()
        return out

    def _apply(self, fn, *args, **kwargs):
        self._forget()
        return super()._apply(fn, *args, **kwargs)

    # ---- derived buffers
    def _pack(self, device):
        key = H.dev_key(device)
        if key not in self._packed:
            f = lambda t: t.detach().float().contiguous()
            enc, dec = self.model.encoder, self.model.decoder

            def qkv(a):
                zero = torch.zeros_like(a.q_proj.bias)
                return f(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])), f(torch.cat([a.q_proj.bias, zero, a.v_proj.bias]))

            def kv(a):
                return f(torch.cat([a.k_proj.weight, a.v_proj.weight])), f(torch.cat([torch.zeros_like(a.v_proj.bias), a.v_proj.bias]))
            self._packed[key] = dict(conv1=permute_conv(enc.conv1.weight), conv2=permute_conv(enc.conv2.weight), enc=[qkv(l.self_attn) for l in enc.layers],
                                     dec=[qkv(l.self_attn) for l in dec.layers], cross=[kv(l.encoder_attn) for l in dec.layers])
        return self._packed[key]

    @staticmethod
    def _w(lin):
        return lin.weight.detach()

    # ---- encoder
    def encode(self, features=None, _padded=None):
        """input_features fp32 [B, n_mels, 2 max_source_positions] (device) -> encoder output fp32 [B, max_source_positions, d]."""
        who = 'Whisper.encode'
        cfg = self.cfg
        d, T, nm, heads = cfg.d_model, cfg.max_source_positions, cfg.num_mel_bins, cfg.encoder_attention_heads
        enc = self.model.encoder
        H.need_device(who, enc.conv1.weight)
        if _padded is None:
            H.need_device(who, features)
            if features.dim() != 3 or tuple(features.shape[1:]) != (nm, 2 * T):
                raise ValueError(f'{who}: features must be [B, {nm}, {2 * T}], got {tuple(features.shape)}')
            B = features.shape[0]
            _padded = torch.zeros(B, 2 * T + 2, nm, dtype=torch.float32, device=features.device)
            _padded[:, 1:2 * T + 1] = features.detach().float().transpose(1, 2)
        B, dev = _padded.shape[0], _padded.device
        if B == 0:
            return torch.empty(0, T, d, dtype=torch.float32, device=dev)
        pk = self._pack(dev)
        key = (B, H.dev_key(dev))
        if key not in self._work:
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
            self._work[key] = dict(hp=torch.zeros(B, 2 * T + 2, d, dtype=torch.float32, device=dev), x=new(B, T, d), h=new(B, T, d), qkv=new(B, T, 3 * d),
                                   att=new(B, T, d), ffn=new(B, T, cfg.encoder_ffn_dim))
        ws = self._work[key]
        hp, x, h = ws['hp'], ws['x'], ws['h']
        wavlm_gemm(_padded, pk['conv1'], enc.conv1.bias, epilogue=EPI_GELU, kernel=3, stride=1, out=hp[:, 1:2 * T + 1])
        pos = enc.embed_positions.weight.detach()
        _gemm(who, B, T, d, 3 * d, hp.data_ptr(), hp.stride(0), 2 * d, pk['conv2'], H.vec(who, enc.conv2.bias, d, 'bias'), x.data_ptr(), x.stride(0), d,
              EPI_GELU, pos.data_ptr(), 0, d)
        scale = (0, d, float(d // heads) ** -0.5)
        for li, lay in enumerate(enc.layers):
            a = lay.self_attn
            wavlm_layernorm(x, lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias, out=h)
            wavlm_gemm(h, pk['enc'][li][0], pk['enc'][li][1], scale=scale, out=ws['qkv'])
            whisper_attention(ws['qkv'], heads, out=ws['att'])
            wavlm_gemm(ws['att'], self._w(a.out_proj), a.out_proj.bias, residual=x, out=x)
            wavlm_layernorm(x, lay.final_layer_norm.weight, lay.final_layer_norm.bias, out=h)
            wavlm_gemm(h, self._w(lay.fc1), lay.fc1.bias, epilogue=EPI_GELU, out=ws['ffn'])
            wavlm_gemm(ws['ffn'], self._w(lay.fc2), lay.fc2.bias, residual=x, out=x)
        return wavlm_layernorm(x, enc.layer_norm.weight, enc.layer_norm.bias)

    # ---- decoder
    def _state(self, B, T_enc, total, device):
        key = (B, T_enc, total, H.dev_key(device))
        if key not in self._steps:
            self._steps[key] = _Step(self.cfg, B, T_enc, total, device)
        return self._steps[key]

    def _project_cross(self, st, enc):
        pk = self._pack(enc.device)
        for li in range(self.cfg.decoder_layers):
            wavlm_gemm(enc, pk['cross'][li][0], pk['cross'][li][1], out=st.cross[li])

    def _step(self, st, n_prompt, eos, pad, logits):
        """The launches of one decoder step; the position is the device counter st.pos."""
        cfg, dec = self.cfg, self.model.decoder
        d, heads = cfg.d_model, cfg.decoder_attention_heads
        pk = self._pack(st.x.device)
        scale = (0, d, float(d // heads) ** -0.5)
        x, q, att, ffn, pos = st.x, st.q, st.att, st.ffn, st.pos
        whisper_embed(st.ids, pos, dec.embed_tokens.weight.detach(), dec.embed_positions.weight.detach(), out=x)
        for li, lay in enumerate(dec.layers):
            sa, ca = lay.self_attn, lay.encoder_attn
            kc, vc = st.cache[li, 0], st.cache[li, 1]
            whisper_linear_step(x, pk['dec'][li][0], pk['dec'][li][1], norm=(lay.self_attn_layer_norm.weight, lay.self_attn_layer_norm.bias), scale=scale,
                                cache=(kc, vc, pos, d), out=q)
            whisper_attn_step(q, kc, vc, heads, pos=pos, out=att)
            whisper_linear_step(att, self._w(sa.out_proj), sa.out_proj.bias, residual=x, out=x)
            whisper_linear_step(x, self._w(ca.q_proj), ca.q_proj.bias, norm=(lay.encoder_attn_layer_norm.weight, lay.encoder_attn_layer_norm.bias), scale=scale,
                                out=q)
            whisper_attn_step(q, st.cross[li][:, :, :d], st.cross[li][:, :, d:], heads, out=att)
            whisper_linear_step(att, self._w(ca.out_proj), ca.out_proj.bias, residual=x, out=x)
            whisper_linear_step(x, self._w(lay.fc1), lay.fc1.bias, norm=(lay.final_layer_norm.weight, lay.final_layer_norm.bias), epilogue=EPI_GELU, out=ffn)
            whisper_linear_step(ffn, self._w(lay.fc2), lay.fc2.bias, residual=x, out=x)
        whisper_logits(x, dec.layer_norm.weight, dec.layer_norm.bias, dec.embed_tokens.weight.detach(), pos, n_prompt, st.partials, mask=st.mask, logits=logits)
        whisper_pick(st.partials, cfg.vocab_size, st.ids, n_prompt, eos, pad, pos, st.n_tokens, st.finished, st.all_done)

    def _run(self, enc, ids0, n_prompt, eos, pad, mask, graph, check_every, want_logits):
        """ids0 int32 [B, total] on the device (prompt or teacher tokens in place) -> (ids, n_tokens, logits or None) for B <= 16 rows."""
        B, T_enc, _ = enc.shape
        total, dev = ids0.shape[1], enc.device
        st = self._state(B, T_enc, total, dev)
        st.ids.copy_(ids0)
        st.pos.zero_(), st.finished.zero_(), st.all_done.zero_(), st.n_tokens.fill_(n_prompt)
        st.mask.copy_(mask)
        self._project_cross(st, enc)
        if want_logits and st.logits is None:
            st.logits = torch.empty(B, self.cfg.vocab_size, dtype=torch.float32, device=dev)
        step_logits = st.logits if want_logits else None
        out = torch.empty(B, total, self.cfg.vocab_size, dtype=torch.float32, device=dev) if want_logits else None
        replay = None
        if graph:
            gkey = (n_prompt, eos, pad, want_logits)
            if gkey not in st.graphs:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._step(st, n_prompt, eos, pad, step_logits)
                st.graphs[gkey] = g
            replay = st.graphs[gkey].replay
        for p in range(total if want_logits else total - 1):
            if replay is not None:
                replay()
            else:
                self._step(st, n_prompt, eos, pad, step_logits)
            if want_logits:
                out[:, p].copy_(step_logits)
            if check_every and (p + 1) % check_every == 0 and p + 1 >= n_prompt and int(st.all_done.item()):
                break
        return st.ids.clone(), st.n_tokens.clone(), out

    def _check_enc(self, who, enc):
        H.need_device(who, enc, self.model.decoder.embed_tokens.weight)
        if enc.dim() != 3 or enc.shape[2] != self.cfg.d_model or enc.dtype != torch.float32:
            raise ValueError(f'{who}: the encoder output must be fp32 [B, T_enc, {self.cfg.d_model}]')
        if not 1 <= enc.shape[1] <= 4096:
            raise ValueError(f'{who}: 1 to 4096 encoder positions')
        return enc.contiguous()

    def step_logits(self, enc, ids, graph=False):
        """Teacher-forced logits fp32 [B, L, vocab] at every position of ids [B, L] through the step kernels (for tests)."""
        who = 'Whisper.step_logits'
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.shape[0] != enc.shape[0]:
            raise ValueError(f'{who}: ids must be [{enc.shape[0]}, L]')
        Lm = ids.shape[1]
        if not 1 <= Lm <= self.cfg.max_target_positions:
            raise ValueError(f'{who}: {Lm} positions; max_target_positions is {self.cfg.max_target_positions}')
        enc = self._check_enc(who, enc)
        ids = ids.to(enc.device).to(torch.int32)
        mask = torch.zeros(self.cfg.vocab_size, dtype=torch.uint8, device=enc.device)
        outs = [self._run(enc[b0:b0 + STEP_ROWS], ids[b0:b0 + STEP_ROWS].contiguous(), Lm, 0, 0, mask, graph, 0, True)[2] for b0 in range(0, enc.shape[0], STEP_ROWS)]
        return torch.cat(outs) if outs else torch.empty(0, Lm, self.cfg.vocab_size, dtype=torch.float32, device=enc.device)

    def generate(self, features, prompt_ids, max_new_tokens, suppress=None, begin_suppress=None, eos=None, pad=None, graph=True, check_every=0,
                 encoder_output=None):
        """Greedy decoding: features fp32 [B, n_mels, frames] (or encoder_output [B, T_enc, d]) and prompt_ids [P] ->
        (ids int32 [B, P + max_new_tokens], n_tokens int32 [B], prompt and eos included), on the device. suppress / begin_suppress: token
        lists set to -inf at every step / at the first generated step; a row that has emitted eos emits pad. graph=True captures one
        step once per shape and replays it. check_every=k reads one "all rows finished" flag every k steps (a host synchronisation,
        opt-in); the default never synchronises."""
        who = 'Whisper.generate'
        cfg = self.cfg
        prompt = [int(v) for v in (prompt_ids.tolist() if torch.is_tensor(prompt_ids) else prompt_ids)]
        P, V = len(prompt), cfg.vocab_size
        eos = cfg.eos_token_id if eos is None else int(eos)
        pad = cfg.pad_token_id if pad is None else int(pad)
        if P < 1 or max_new_tokens < 0:
            raise ValueError(f'{who}: an empty prompt or a negative max_new_tokens')
        if P + int(max_new_tokens) > cfg.max_target_positions:
            raise ValueError(f'{who}: {P} prompt tokens + {max_new_tokens} new tokens exceed max_target_positions {cfg.max_target_positions}')
        lists = [list(map(int, s)) if s is not None else [] for s in (suppress, begin_suppress)]
        if any(not 0 <= t < V for t in prompt + lists[0] + lists[1] + [eos, pad]):
            raise ValueError(f'{who}: a token outside the vocabulary of {V}')
        if check_every < 0:
            raise ValueError(f'{who}: check_every must be >= 0')
        enc = self.encode(features) if encoder_output is None else encoder_output
        enc = self._check_enc(who, enc)
        B, dev, total = enc.shape[0], enc.device, P + int(max_new_tokens)
        m = np.zeros(V, dtype=np.uint8)
        m[lists[0]] |= 1
        m[lists[1]] |= 2
        mask = torch.from_numpy(m).to(dev)
        row = torch.tensor(prompt + [pad] * (total - P), dtype=torch.int32, device=dev)
        ids, n_tokens = [], []
        for b0 in range(0, B, STEP_ROWS):
            e = enc[b0:b0 + STEP_ROWS]
            i, n, _ = self._run(e, row.expand(e.shape[0], total), P, eos, pad, mask, graph, int(check_every), False)
            ids.append(i), n_tokens.append(n)
        if not ids:
            return torch.empty(0, total, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        return torch.cat(ids), torch.cat(n_tokens)

    def transcribe(self, signal, lengths, prompt_ids, max_new_tokens, tokenizer=None, chunk_length=None, **kw):
        """Waveforms [B, L] at 16 kHz with per-row lengths (or None) -> generate(...) on their log-mel features. With a `tokenizer` (any
        object with .decode(list of ids, skip_special_tokens=True)) also the strings of the new tokens, eos excluded: (ids, n_tokens,
        texts). Whisper's text normaliser is the caller's."""
        who = 'Whisper.transcribe'
        cfg = self.cfg
        H.need_device(who, signal)
        frames = 2 * cfg.max_source_positions
        if chunk_length is None:
            chunk_length = frames * HOP // SAMPLE_RATE
        if int(chunk_length) * SAMPLE_RATE != frames * HOP:
            raise ValueError(f'{who}: a chunk of {chunk_length} s is not the {frames} frames of max_source_positions')
        x2, _, _ = H.rows2(who, signal)
        padded = torch.zeros(x2.shape[0], frames + 2, cfg.num_mel_bins, dtype=torch.float32, device=x2.device)
        whisper_log_mel(x2, lengths, chunk_length, cfg.num_mel_bins, out=padded[:, 1:frames + 1].transpose(1, 2))
        ids, n_tokens = self.generate(None, prompt_ids, max_new_tokens, encoder_output=self.encode(_padded=padded), **kw)
        if tokenizer is None:
            return ids, n_tokens
        P = len(prompt_ids)
        eos = cfg.eos_token_id if kw.get('eos') is None else int(kw['eos'])
        host, n = ids.tolist(), n_tokens.tolist()
        texts = [tokenizer.decode([t for t in host[b][P:n[b]] if t != eos], skip_special_tokens=True) for b in range(len(host))]
        return ids, n_tokens, texts

    def forward(self, features, prompt_ids, max_new_tokens, **kw):
        return self.generate(features, prompt_ids, max_new_tokens, **kw)


def load_whisper(path_or_state_dict, config=None, device='cpu'):
    """A state dict (or the path of one saved with torch.save) and HF's config (a WhisperConfig, a config.json dict or its path) ->
    Whisper(config) with the state dict loaded strictly, in eval mode on `device`."""
    sd = path_or_state_dict
    if not isinstance(sd, dict):
        sd = torch.load(sd, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict) or 'model.decoder.embed_tokens.weight' not in sd:
        raise ValueError("load_whisper: a Whisper state dict holds 'model.encoder.*' and 'model.decoder.*'")
    if isinstance(config, str):
        import json
        config = json.load(open(config))
    model = Whisper(config)
    model.load_state_dict(sd, strict=True)
    return model.to(device).eval()


# ----------------------------------------------------------------------------------------------------------------- WER / CER
def _edits(ref, hyp):
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i] + [0] * len(hyp)
        for j, h in enumerate(hyp, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r != h))
        prev = cur
    return prev[-1]


def _rate(who, predictions, references, units):
    predictions, references = list(predictions), list(references)
    if len(predictions) != len(references):
        raise ValueError(f'{who}: {len(predictions)} predictions for {len(references)} references')
    total = sum(len(units(r)) for r in references)
    if total == 0:
        raise ValueError(f'{who}: the references are empty')
    return sum(_edits(units(r), units(p)) for p, r in zip(predictions, references)) / total


def asr_wer(predictions, references):
    """evaluate.load('wer') (jiwer): substitutions + deletions + insertions over the whole corpus divided by the reference words
    (split on whitespace). Not the mean of the per-sentence rates."""
    return _rate('asr_wer', predictions, references, str.split)


def asr_cer(predictions, references):
    """evaluate.load('cer'): the same over characters, spaces included, per pair, with the corpus totals."""
    return _rate('asr_cer', predictions, references, list)


def asr_report(converted, originals, references):
    """The aggregation of test_asr.py:94-120 on plain dicts. converted[src][tgt], originals[src], references[src]: lists of transcripts,
    one per utterance of the source speaker. A conversion is scored against the transcript of its ORIGINAL audio, an original against
    the reference text. Returns wer_pair / cer_pair [src][tgt], wer / cer over all pairs, orig_wer_single / orig_cer_single [src] and
    orig_wer / orig_cer over all originals."""
    spks = list(converted)
    out = dict(wer_pair={}, cer_pair={}, orig_wer_single={}, orig_cer_single={})
    hyp, ref, ohyp, oref = [], [], [], []
    for s in spks:
        for t in spks:
            out['wer_pair'].setdefault(s, {})[t] = asr_wer(converted[s][t], originals[s])
            out['cer_pair'].setdefault(s, {})[t] = asr_cer(converted[s][t], originals[s])
            hyp += list(converted[s][t])
            ref += list(originals[s])
        out['orig_wer_single'][s], out['orig_cer_single'][s] = asr_wer(originals[s], references[s]), asr_cer(originals[s], references[s])
        ohyp += list(originals[s])
        oref += list(references[s])
    out.update(wer=asr_wer(hyp, ref), cer=asr_cer(hyp, ref), orig_wer=asr_wer(ohyp, oref), orig_cer=asr_cer(ohyp, oref))
    return out
