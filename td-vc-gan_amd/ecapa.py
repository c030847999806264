"""Speaker recognition on the device: the speechbrain path of the reference's test_scripts/mls-pt/test_speaker_rec.py (lines
58-186; the vctk script is wired the same way). Each file gets speechbrain Fbank features, sentence mean normalisation, an
ECAPA-TDNN embedding (sb_classifier_hparams.yaml) and a cosine classifier over the training speakers; the script reports the
predicted class, the probability of the target speaker and the cosine similarity of each converted utterance to the target speaker's
mean embedding (that last step is what speaker.speaker_similarity already computes). Neither speechbrain nor torchaudio is
available here and the reference ships no embedding_model.ckpt, so the definition below (also in include/tdvc.h), written from
knowledge of speechbrain 0.5's lobes/features.py, processing/features.py, nnet/CNN.py and lobes/models/ECAPA_TDNN.py, is the
contract and tests/ecapa_ref.py restates it in float64; **parity with an installed speechbrain is unchecked**, and so are the
state-dict keys against a real embedding_model.ckpt. Every quirk below is speechbrain's and is kept.

Definition. The input is a 16 kHz waveform row of n samples; samples at and past n are never read and count as zero.
  Features (Fbank(n_mels=80), InputNormalization(norm_type='sentence', std_norm=False)):
    STFT: n_fft = win = 400, hop 160, periodic Hamming window (torch.hamming_window(400)), center=True, pad_mode='constant' (zeros),
      one-sided 201 bins; frame count F = 1 + n // 160.
    Power: re^2 + im^2 (speechbrain's spectral_magnitude(power=1) returns the power spectrum, not its root).
    Filterbank: HTK mel scale mel = 2595 log10(1 + hz/700); hz[0..81] the image of 82 points equally spaced in mel on 0..8000 Hz;
      f_c[i] = hz[i+1]; band[i] = hz[i+1] - hz[i] (the left width only); bin frequencies linspace(0, 8000, 201); filter i at bin
      frequency f is max(0, min((f - f_c[i])/band[i] + 1, -(f - f_c[i])/band[i] + 1)): a symmetric triangle of half-width band[i]
      with peak 1 and no area normalisation.
    dB: 10 log10(max(x, 1e-10)), then max(., M - 80) with M the largest dB value of that row over its own F frames and 80 bands.
    Normalisation: subtract, per band, the mean over the row's F frames.
  Network: ECAPA_TDNN(input_size=80, channels=[1024,1024,1024,1024,3072], kernel_sizes=[5,3,3,3,1], dilations=[1,2,3,4,1],
  attention_channels=128, lin_neurons=192) with res2net_scale=8, se_channels=128, global_context=True, in eval mode.
    Conv1d: every Conv1d is "same"-padded with reflect padding, (k - 1) d / 2 per side, the edge sample not repeated; the reflection
      is about the row's own first and last frame, not the buffer's.
    TDNNBlock(x) = BatchNorm(ReLU(conv(x))); BatchNorm uses running statistics and eps 1e-5.
    blocks[0] = TDNNBlock(80 -> C, k5, d1). blocks[1..3] = SERes2NetBlock(C -> C, k3, d = 2, 3, 4): tdnn1 (k1); Res2Net over 8 channel
      chunks: y0 = x0, y1 = B0(x1), yi = B(i-1)(xi + y(i-1)), each B a TDNNBlock(C/8 -> C/8, k3, d); tdnn2 (k1); SE: s = mean over the
      row's frames, g = sigmoid(conv2(relu(conv1(s)))), output g x; then + the block's input.
    MFA: x = cat(blocks[1..3] outputs) -> mfa = TDNNBlock(3C -> 3C, k1).
    Attentive statistics pooling over the row's frames: uniform-weight mean m, sd = sqrt(clamp(sum w (x - m)^2, 1e-12));
      a = conv(tanh(TDNNBlock_{9C -> 128, k1}(cat[x, m, sd]))); softmax over the row's frames; weighted m, sd by the same formula -> [6C].
    Head: asp_bn -> fc (1x1 conv, 6C -> 192) -> the embedding [192].
  State-dict keys (speechbrain's): blocks.0.conv.conv.weight|bias, blocks.0.norm.norm.weight|bias|running_mean|running_var|
    num_batches_tracked, blocks.{1,2,3}.tdnn1.*, blocks.{1,2,3}.res2net_block.blocks.{0..6}.*, blocks.{1,2,3}.tdnn2.*,
    blocks.{1,2,3}.se_block.conv{1,2}.conv.weight|bias, mfa.*, asp.tdnn.*, asp.conv.conv.weight|bias, asp_bn.norm.*,
    fc.conv.weight|bias.
  Classifier(input_size=192, out_neurons) has the single key weight [S, 192]: logits = normalize(e) normalize(weight)^T; the script
    takes softmax over S, the argmax class and the target speaker's probability (`speaker_classify`).
  Embedding normalisation quirk: mean_var_norm_emb is InputNormalization('global', std_norm=False) and is never put in eval mode, so
    the script subtracts from the k-th embedding it computes the running mean of embeddings 1..k; the first becomes all zeros and the
    result depends on file order. `running_mean_norm` offers this, opt-in, as the reference's behaviour.
  Stated deviations and limits: a row is evaluated as if alone (the reference passes one file with lengths=[1.0]): a batch of rows
    with per-row lengths gives each row exactly the result it gets alone. Rows of fewer than 5 frames (n < 640) are refused: a reflect
    pad of 4 needs 5 frames (a padded width below 640 is refused on the host; a device length below 640 cannot be refused without a
    synchronisation and gives an unspecified result for that row). Every channel count must be a multiple of 16 and C a multiple of
    128. Inference only, no backward. The vctk script's 48 kHz resampling of a 16 kHz file is not reproduced: the input is 16 kHz
    (`resample` exists for other rates).

Everything runs in csrc/eval_ecapa.hip (tdvc_fbank, tdvc_tdnn_fwd, tdvc_se_block, tdvc_asp_pool, tdvc_ecapa_head): no CPU or ATen
fallback, no host synchronisation, frame counts stay on the device as int32, no atomics, fixed summation orders (bit-identical from
call to call), every launch capturable into a graph. `speaker_classify` and `running_mean_norm` are a few hundred elements of stock
torch ops on whatever device their inputs live on, as speaker.speaker_similarity is.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _host as H
from . import _lib as L

SR, N_FFT, HOP, BINS, MIN_SAMPLES = 16000, 400, 160, 201, 640
EPI_NONE, EPI_RELU_BN, EPI_RELU_BN_TANH = L.TDNN_NONE, L.TDNN_RELU_BN, L.TDNN_RELU_BN_TANH
BN_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------- host definitions
def hz_to_mel(hz):
    """HTK mel scale."""
    return 2595.0 * np.log10(1.0 + np.asarray(hz, dtype=np.float64) / 700.0)


def mel_to_hz(mel):
    return 700.0 * (10.0 ** (np.asarray(mel, dtype=np.float64) / 2595.0) - 1.0)


def fbank_matrix(n_mels=80):
    """float64 [n_mels, 201], read-only, cached: speechbrain's triangular Filterbank (left band width on both sides, peak 1)."""
    n_mels = int(n_mels)

    def build():
        hz = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(SR / 2.0), n_mels + 2))
        f_c, band = hz[1:-1], hz[1:-1] - hz[:-2]
        f = np.linspace(0.0, SR / 2.0, BINS)
        slope = (f[None, :] - f_c[:, None]) / band[:, None]
        fb = np.maximum(0.0, np.minimum(slope + 1.0, -slope + 1.0))
        fb.setflags(write=False)
        return fb
    return H.host_table(f'ecapa_fbank_{n_mels}', build)


def _tables(device, n_mels):
    """float64 [400 cos | 400 sin | 400 Hamming | n_mels x 201 filterbank] on the device, uploaded once."""
    return H.device_table(device, f'ecapa_tables_{n_mels}',
                          lambda: np.concatenate([H.dft_tables(N_FFT, (0.54, 0.46)), fbank_matrix(n_mels).reshape(-1)]))


# ------------------------------------------------------------------------------------------------------------------ operators
def _fbank(who, signal, lengths, n_mels):
    """-> (feats [B, n_mels, F], frames int32 [B])"""
    H.need_device(who, signal)
    x2, bs, _ = H.rows2(who, signal)
    B, T = x2.shape
    lengths = H.device_lengths(who, lengths, B, x2.device)
    n_mels = int(n_mels)
    if n_mels < 16 or n_mels > 128 or n_mels % 16:
        raise ValueError(f'{who}: n_mels must be a multiple of 16 up to 128, got {n_mels}')
    if T < MIN_SAMPLES:
        raise ValueError(f'{who}: rows of fewer than {MIN_SAMPLES} samples (5 frames) are refused, got {T}')
    lib = L.lib()
    F = 1 + T // HOP
    feats = torch.empty(B, n_mels, F, dtype=torch.float32, device=x2.device)
    frames = torch.empty(B, dtype=torch.int32, device=x2.device)
    ws_bytes = lib.tdvc_fbank_workspace(B, T, n_mels)
    ws = H.scratch(ws_bytes, x2.device)
    H.check(who, lib.tdvc_fbank(x2.data_ptr(), bs, H.ptr(lengths), T, B, n_mels, _tables(x2.device, n_mels).data_ptr(), feats.data_ptr(),
                                n_mels * F, F, F, frames.data_ptr(), ws.data_ptr(), ws_bytes, H.stream(x2)))
    return feats, frames


def fbank(signal, lengths=None, n_mels=80, return_frames=False):
    """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz) -> the normalised log-mel features fp32 [B, n_mels, F], F = 1 + T // 160
    (tdvc_fbank, two launches); with return_frames also the per-row frame counts 1 + lengths // 160, device int32 [B]. lengths:
    device integers [B]; samples at and past them are never read, and a row's frames at and past its count are zeros. Rows are
    strided views (nothing is copied unless the last axis is not dense)."""
    feats, frames = _fbank('fbank', signal, lengths, n_mels)
    return (feats, frames) if return_frames else feats


def _act3(who, t):
    """[B, C, F] fp32 with dense frames -> (tensor, batch stride, channel stride); a channel slice of a wider buffer stays a view."""
    H.need_device(who, t)
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f'{who}: activations must be fp32 [B, C, F], got {tuple(t.shape)} {t.dtype}')
    if t.shape[2] > 1 and t.stride(2) != 1:
        t = t.contiguous()
    B, Cc, F = t.shape
    return t, (t.stride(0) if B > 1 else Cc * max(t.stride(1), F)), (t.stride(1) if Cc > 1 else F)


def tdnn_fwd(x, weight, bias=None, dilation=1, epilogue=EPI_NONE, scale=None, shift=None, x2=None, row_bias=None, frames=None, out=None):
    """The reflect-padded, length-aware Conv1d (tdvc_tdnn_fwd): x [B, Cin, F] (+ x2, added before the convolution), weight
    [Cout, Cin, K] -> out [B, Cout, F] (given, possibly a channel slice, or new). Frames at and past frames[b] are neither read nor
    written (a new `out` holds zeros there)."""
    who = 'tdnn_fwd'
    x, x_bs, x_cs = _act3(who, x)
    B, Cin, F = x.shape
    H.need_device(who, weight)
    if weight.dim() != 3:
        raise ValueError(f'{who}: weight must be [Cout, Cin, K]')
    w = weight.detach().float().contiguous()
    Cout, Wc, K = w.shape
    if Wc != Cin:
        raise ValueError(f'{who}: x has {Cin} channels, the weight takes {Wc}')
    a = L.TdnnArgs()
    a.B, a.Cin, a.Cout, a.F, a.K, a.dilation, a.epilogue = B, Cin, Cout, F, K, int(dilation), int(epilogue)
    a.x, a.x_bs, a.x_cs = x.data_ptr(), x_bs, x_cs
    if x2 is not None:
        x2, b2, c2 = _act3(who, x2)
        if x2.shape != x.shape:
            raise ValueError(f'{who}: x2 must have the shape of x')
        a.x2, a.x2_bs, a.x2_cs = x2.data_ptr(), b2, c2
    a.w = w.data_ptr()
    keep = [w, x, x2]
    for name, t, n in (('bias', bias, Cout), ('scale', scale, Cout), ('shift', shift, Cout), ('row_bias', row_bias, B * Cout)):
        if t is not None:
            t = H.vec(who, t, n, name)
            keep.append(t)
            setattr(a, name, t.data_ptr())
    if frames is not None:
        H.need_device(who, frames)
        if frames.shape != (B,) or frames.dtype != torch.int32:
            raise ValueError(f'{who}: frames must be int32 [{B}]')
        frames = frames.contiguous()
        a.frames = frames.data_ptr()
    if out is None:
        out = torch.zeros(B, Cout, F, dtype=torch.float32, device=x.device)
    H.need_device(who, out)
    if tuple(out.shape) != (B, Cout, F) or out.dtype != torch.float32 or (F > 1 and out.stride(2) != 1):
        raise ValueError(f'{who}: out must be fp32 [{B}, {Cout}, {F}] with dense frames')
    a.y, a.y_bs, a.y_cs = out.data_ptr(), (out.stride(0) if B > 1 else Cout * max(out.stride(1), F)), (out.stride(1) if Cout > 1 else F)
    H.check(who, L.lib().tdvc_tdnn_fwd(C.byref(a), H.stream(x)))
    return out


def se_block(x, residual, w1, b1, w2, b2, frames=None, out=None, return_gate=False):
    """tdvc_se_block: x, residual [B, C, F], w1 [S, C(, 1)], w2 [C, S(, 1)] -> out = sigmoid(w2 relu(w1 mean_f(x) + b1) + b2) x + residual."""
    who = 'se_block'
    x, x_bs, x_cs = _act3(who, x)
    residual, r_bs, r_cs = _act3(who, residual)
    B, Cc, F = x.shape
    if residual.shape != x.shape:
        raise ValueError(f'{who}: residual must have the shape of x')
    H.need_device(who, w1, w2)
    S = w1.shape[0]
    w1, w2 = H.vec(who, w1, S * Cc), H.vec(who, w2, S * Cc)
    b1, b2 = H.vec(who, b1, S), H.vec(who, b2, Cc)
    if frames is not None:
        H.need_device(who, frames)
        frames = frames.to(torch.int32).contiguous()
    if out is None:
        out = torch.zeros(B, Cc, F, dtype=torch.float32, device=x.device)
    H.need_device(who, out)
    if tuple(out.shape) != (B, Cc, F) or out.dtype != torch.float32 or (F > 1 and out.stride(2) != 1):
        raise ValueError(f'{who}: out must be fp32 [{B}, {Cc}, {F}] with dense frames')
    gate = torch.empty(B, Cc + S, dtype=torch.float32, device=x.device)
    o_bs, o_cs = (out.stride(0) if B > 1 else Cc * max(out.stride(1), F)), (out.stride(1) if Cc > 1 else F)
    H.check(who, L.lib().tdvc_se_block(x.data_ptr(), x_bs, x_cs, residual.data_ptr(), r_bs, r_cs, B, Cc, F, H.ptr(frames), S, w1.data_ptr(),
                                       b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), gate.data_ptr(), out.data_ptr(), o_bs, o_cs, H.stream(x)))
    return (out, gate[:, :Cc]) if return_gate else out


def asp_pool(x, w_tdnn, b_tdnn, scale, shift, w_conv, b_conv, frames=None):
    """tdvc_asp_pool: x [B, C, F], w_tdnn [A, 3C(, 1)] with bias and folded BatchNorm scale / shift [A], w_conv [C, A(, 1)], b_conv [C]
    -> (weighted mean | weighted sd) fp32 [B, 2C]."""
    who = 'asp_pool'
    x, x_bs, x_cs = _act3(who, x)
    B, Cc, F = x.shape
    H.need_device(who, w_tdnn, w_conv)
    A = w_tdnn.shape[0]
    w_tdnn, w_conv = H.vec(who, w_tdnn, A * 3 * Cc), H.vec(who, w_conv, A * Cc)
    b_tdnn, scale, shift, b_conv = H.vec(who, b_tdnn, A), H.vec(who, scale, A), H.vec(who, shift, A), H.vec(who, b_conv, Cc)
    if frames is not None:
        H.need_device(who, frames)
        frames = frames.to(torch.int32).contiguous()
    lib = L.lib()
    ws_bytes = lib.tdvc_asp_pool_workspace(B, Cc, A, F)
    ws = H.scratch(ws_bytes, x.device)
    pooled = torch.empty(B, 2 * Cc, dtype=torch.float32, device=x.device)
    H.check(who, lib.tdvc_asp_pool(x.data_ptr(), x_bs, x_cs, B, Cc, F, H.ptr(frames), A, w_tdnn.data_ptr(), b_tdnn.data_ptr(), scale.data_ptr(),
                                   shift.data_ptr(), w_conv.data_ptr(), b_conv.data_ptr(), pooled.data_ptr(), ws.data_ptr(), ws_bytes,
                                   H.stream(x)))
    return pooled


def ecapa_head(pooled, scale, shift, weight, bias):
    """tdvc_ecapa_head: pooled [B, N], folded asp_bn scale / shift [N], fc weight [E, N(, 1)], bias [E] -> fp32 [B, E]."""
    who = 'ecapa_head'
    H.need_device(who, pooled, weight)
    if pooled.dim() != 2:
        raise ValueError(f'{who}: pooled must be [B, N]')
    pooled = pooled.detach().float().contiguous()
    B, N = pooled.shape
    E = weight.shape[0]
    weight, bias, scale, shift = H.vec(who, weight, E * N), H.vec(who, bias, E), H.vec(who, scale, N), H.vec(who, shift, N)
    emb = torch.empty(B, E, dtype=torch.float32, device=pooled.device)
    H.check(who, L.lib().tdvc_ecapa_head(pooled.data_ptr(), B, N, scale.data_ptr(), shift.data_ptr(), weight.data_ptr(), bias.data_ptr(), E,
                                         emb.data_ptr(), H.stream(pooled)))
    return emb


def fold_bn(bn):
    """nn.BatchNorm1d in eval mode as (scale, shift) fp32: scale = gamma / sqrt(var + eps), shift = beta - mean scale, evaluated in
    float64 and rounded once."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


# -------------------------------------------------------------------------------------------------------------------- module
class _Conv(torch.nn.Module):
    """speechbrain.nnet.CNN.Conv1d: the parameters live under `.conv`."""

    def __init__(self, cin, cout, k, dilation=1):
        super().__init__()
        self.conv = torch.nn.Conv1d(cin, cout, k, dilation=dilation)


class _Norm(torch.nn.Module):
    """speechbrain.nnet.normalization.BatchNorm1d: the parameters live under `.norm`."""

    def __init__(self, c):
        super().__init__()
        self.norm = torch.nn.BatchNorm1d(c, eps=BN_EPS)


class _Tdnn(torch.nn.Module):
    def __init__(self, cin, cout, k, dilation):
        super().__init__()
        self.conv = _Conv(cin, cout, k, dilation)
        self.norm = _Norm(cout)


class _Res2Net(torch.nn.Module):
    def __init__(self, c, scale, k, dilation):
        super().__init__()
        self.blocks = torch.nn.ModuleList([_Tdnn(c // scale, c // scale, k, dilation) for _ in range(scale - 1)])


class _SE(torch.nn.Module):
    def __init__(self, c, se):
        super().__init__()
        self.conv1 = _Conv(c, se, 1)
        self.conv2 = _Conv(se, c, 1)


class _SERes2Net(torch.nn.Module):
    def __init__(self, c, scale, se, k, dilation):
        super().__init__()
        self.tdnn1 = _Tdnn(c, c, 1, 1)
        self.res2net_block = _Res2Net(c, scale, k, dilation)
        self.tdnn2 = _Tdnn(c, c, 1, 1)
        self.se_block = _SE(c, se)


class _Asp(torch.nn.Module):
    def __init__(self, c, att):
        super().__init__()
        self.tdnn = _Tdnn(3 * c, att, 1, 1)
        self.conv = _Conv(att, c, 1)


class EcapaTdnn(torch.nn.Module):
    """speechbrain's ECAPA_TDNN: the same state_dict keys and shapes (the module docstring lists them), so that an
    embedding_model.ckpt loads with strict=True. The stock modules are containers for the parameters and are never called: `embed`
    runs csrc/eval_ecapa.hip. The BatchNorms are folded to scale / shift once per device and again after load_state_dict or a move."""

    def __init__(self, input_size=80, channels=(1024, 1024, 1024, 1024, 3072), kernel_sizes=(5, 3, 3, 3, 1), dilations=(1, 2, 3, 4, 1),
                 attention_channels=128, res2net_scale=8, se_channels=128, lin_neurons=192):
        super().__init__()
        channels, kernel_sizes, dilations = list(channels), list(kernel_sizes), list(dilations)
        who = 'EcapaTdnn'
        if len(channels) != 5 or len(kernel_sizes) != 5 or len(dilations) != 5:
            raise ValueError(f'{who}: five entries each in channels, kernel_sizes and dilations (one TDNN block, three SE-Res2Net blocks, MFA)')
        Cc = channels[0]
        if any(c != Cc for c in channels[:4]) or channels[4] != 3 * Cc:
            raise ValueError(f'{who}: channels must be [C, C, C, C, 3C], got {channels}')
        if res2net_scale != 8:
            raise ValueError(f'{who}: res2net_scale must be 8')
        if Cc % 128:
            raise ValueError(f'{who}: C must be a multiple of 128 (C / 8 a multiple of 16), got {Cc}')
        for name, v in (('input_size', input_size), ('attention_channels', attention_channels), ('se_channels', se_channels), ('lin_neurons', lin_neurons)):
            if v < 16 or v % 16:
                raise ValueError(f'{who}: {name} must be a multiple of 16, got {v}')
        if any(k not in (1, 3, 5) for k in kernel_sizes) or kernel_sizes[4] != 1:
            raise ValueError(f'{who}: kernel sizes must be 1, 3 or 5 (1 for the MFA layer), got {kernel_sizes}')
        if any(not 1 <= d <= 4 for d in dilations):
            raise ValueError(f'{who}: dilations must be 1..4, got {dilations}')
        self.input_size, self.channels, self.lin_neurons = input_size, Cc, lin_neurons
        self.blocks = torch.nn.ModuleList([_Tdnn(input_size, Cc, kernel_sizes[0], dilations[0])] +
                                          [_SERes2Net(Cc, res2net_scale, se_channels, kernel_sizes[i], dilations[i]) for i in (1, 2, 3)])
        self.mfa = _Tdnn(3 * Cc, 3 * Cc, kernel_sizes[4], dilations[4])
        self.asp = _Asp(3 * Cc, attention_channels)
        self.asp_bn = _Norm(6 * Cc)
        self.fc = _Conv(6 * Cc, lin_neurons, 1)
        self._folded = {}

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._folded = {}
        return out

    def _apply(self, fn, *args, **kwargs):
        self._folded = {}
        return super()._apply(fn, *args, **kwargs)

    def _fold(self, device):
        k = H.dev_key(device)
        if k not in self._folded:
            self._folded[k] = {name: fold_bn(m.norm) for name, m in self.named_modules() if isinstance(m, _Norm)}
        return self._folded[k]

    def _tdnn(self, fold, name, m, x, frames, out=None, rows=None, x2=None, epilogue=EPI_RELU_BN):
        """TDNNBlock `m` (named `name`) on x; rows = (lo, hi): only those output channels."""
        w, b = m.conv.conv.weight, m.conv.conv.bias
        scale, shift = fold[name + '.norm']
        if rows is not None:
            lo, hi = rows
            w, b, scale, shift = w[lo:hi], b[lo:hi], scale[lo:hi], shift[lo:hi]
        return tdnn_fwd(x, w, b, m.conv.conv.dilation[0], epilogue, scale, shift, x2=x2, frames=frames, out=out)

    def features(self, signal, lengths=None):
        """-> (normalised log-mel [B, input_size, F], frame counts int32 [B]): the front end alone."""
        return _fbank('EcapaTdnn.features', signal, lengths, self.input_size)

    def embed_features(self, feats, frames=None):
        """feats [B, input_size, F] (device fp32) with frame counts int32 [B] or None -> the embeddings fp32 [B, lin_neurons]."""
        who = 'EcapaTdnn.embed'
        H.need_device(who, feats, self.fc.conv.weight)
        if feats.dim() != 3 or feats.shape[1] != self.input_size:
            raise ValueError(f'{who}: features must be [B, {self.input_size}, F], got {tuple(feats.shape)}')
        fold = self._fold(feats.device)
        B, _, F = feats.shape
        Cc, c8 = self.channels, self.channels // 8
        new = lambda ch: torch.empty(B, ch, F, dtype=torch.float32, device=feats.device)
        x = self._tdnn(fold, 'blocks.0', self.blocks[0], feats, frames, out=new(Cc))
        cat, r, y, t2 = new(3 * Cc), new(Cc), new(Cc), new(Cc)
        for i in (1, 2, 3):
            blk, name = self.blocks[i], f'blocks.{i}'
            # tdnn1: chunk 0 goes straight into the Res2Net output (y0 = x0), the other chunks into r
            self._tdnn(fold, name + '.tdnn1', blk.tdnn1, x, frames, out=y[:, :c8], rows=(0, c8))
            self._tdnn(fold, name + '.tdnn1', blk.tdnn1, x, frames, out=r[:, c8:], rows=(c8, Cc))
            for jx in range(1, 8):
                self._tdnn(fold, f'{name}.res2net_block.blocks.{jx - 1}', blk.res2net_block.blocks[jx - 1], r[:, jx * c8:(jx + 1) * c8], frames,
                           out=y[:, jx * c8:(jx + 1) * c8], x2=y[:, (jx - 1) * c8:jx * c8] if jx > 1 else None)
            self._tdnn(fold, name + '.tdnn2', blk.tdnn2, y, frames, out=t2)
            se = blk.se_block
            out = cat[:, (i - 1) * Cc:i * Cc]
            se_block(t2, x, se.conv1.conv.weight, se.conv1.conv.bias, se.conv2.conv.weight, se.conv2.conv.bias, frames=frames, out=out)
            x = out
        m = self._tdnn(fold, 'mfa', self.mfa, cat, frames, out=new(3 * Cc))
        a_scale, a_shift = fold['asp.tdnn.norm']
        pooled = asp_pool(m, self.asp.tdnn.conv.conv.weight, self.asp.tdnn.conv.conv.bias, a_scale, a_shift, self.asp.conv.conv.weight,
                          self.asp.conv.conv.bias, frames=frames)
        h_scale, h_shift = fold['asp_bn']
        return ecapa_head(pooled, h_scale, h_shift, self.fc.conv.weight, self.fc.conv.bias)

    def embed(self, signal, lengths=None):
        """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz), lengths device integers [B] or None -> the embeddings fp32
        [B, lin_neurons]. Samples at and past lengths are never read; a row's embedding does not depend on the rows beside it. No
        host synchronisation: the buffers are sized from the padded width T alone."""
        feats, frames = _fbank('EcapaTdnn.embed', signal, lengths, self.input_size)
        return self.embed_features(feats, frames)

    forward = embed


def read_label_encoder(path):
    """The reference's label_encoder.txt (speechbrain's CategoricalEncoder): lines `'p293' => 0` up to the `====` rule ->
    (lab2ind, ind2lab)."""
    lab2ind = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith('===='):
                break
            m = re.fullmatch(r"'(.*)' => (-?\d+)", line)
            if not m:
                if line:
                    raise ValueError(f'read_label_encoder: cannot parse {line!r}')
                continue
            lab2ind[m.group(1)] = int(m.group(2))
    return lab2ind, {v: k for k, v in lab2ind.items()}


def _load_weights(path):
    if str(path).endswith('.npz'):
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in z.files}
    return torch.load(path, map_location='cpu', weights_only=True)


def load_ecapa(embedding_ckpt=None, classifier_ckpt=None, label_encoder=None, device='cpu', **config):
    """-> dict(model: an EcapaTdnn(**config) with embedding_ckpt loaded strictly (None without one), weight: the classifier's
    [S, 192] (None without classifier_ckpt), lab2ind / ind2lab from label_encoder.txt (None without)). Checkpoints are state dicts
    read with torch.load(weights_only=True), or .npz files of the same keys."""
    model = weight = lab2ind = ind2lab = None
    if embedding_ckpt is not None:
        model = EcapaTdnn(**config)
        model.load_state_dict(_load_weights(embedding_ckpt), strict=True)
        model = model.to(device).eval()
    if classifier_ckpt is not None:
        sd = _load_weights(classifier_ckpt)
        if set(sd) != {'weight'} or sd['weight'].dim() != 2:
            raise ValueError(f'load_ecapa: a Classifier checkpoint has the single key weight [S, E], got {sorted(sd)}')
        weight = sd['weight'].float().to(device)
    if label_encoder is not None:
        lab2ind, ind2lab = read_label_encoder(label_encoder)
    return dict(model=model, weight=weight, lab2ind=lab2ind, ind2lab=ind2lab)


def speaker_classify(emb, weight, target=None):
    """speechbrain's Classifier and the script's softmax: emb [B, E], weight [S, E] -> (prob [B, S] = softmax(normalize(emb)
    normalize(weight)^T), pred [B] = argmax, target_prob [B] = prob[b, target[b]] or None). Stock torch ops, no host synchronisation."""
    e = torch.nn.functional.normalize(emb.float(), dim=1)
    w = torch.nn.functional.normalize(weight.float(), dim=1)
    prob = torch.softmax(e @ w.t(), dim=1)
    pred = prob.argmax(dim=1)
    tp = None if target is None else prob.gather(1, torch.as_tensor(target, device=prob.device).long()[:, None])[:, 0]
    return prob, pred, tp


def running_mean_norm(emb):
    """The reference's embedding normalisation as it runs (a 'global' InputNormalization left in training mode): row k, in call
    order, becomes e_k - mean(e_1..e_k); the first row becomes zeros and the result depends on the order. Opt-in."""
    e = emb.float()
    k = torch.arange(1, e.shape[0] + 1, device=e.device, dtype=e.dtype)[:, None]
    return e - torch.cumsum(e, dim=0) / k
