"""Speaker similarity on the device: the live path of the reference's test_scripts/common/test_speaker_rec.py (lines 120-180),
which embeds every original and converted file with Resemblyzer's VoiceEncoder.embed_utterance, builds per-speaker mean
embeddings, and reports the cosine similarity of each converted utterance to its target speaker's mean and a nearest-centroid
classification. Resemblyzer, librosa and webrtcvad are not available here, so the definition below (also in include/tdvc.h) is
the contract and tests/speaker_ref.py restates it in float64; **parity with an installed resemblyzer / librosa is unchecked**.

Definition (Resemblyzer's VoiceEncoder, hparams as shipped): sr = 16000, n_fft = 400 (25 ms), hop = 160 (10 ms), n_mels = 40,
partials_n_frames = 160, hidden size 256, embedding size 256, 3 layers.
  Mel front end (librosa.feature.melspectrogram(y, sr, n_fft=400, hop_length=160, n_mels=40), transposed): centred frames, frame f
  covers padded samples [160 f - 200, 160 f + 200), 1 + L' // 160 frames for a row of padded length L'; pad_mode='reflect' (the edge
  sample is not repeated; librosa < 0.10's default and the default here) or 'constant' (zeros; librosa 0.10 and later changed its
  default to this); periodic Hann window of 400 points; power |DFT|^2 on 201 bins; no logarithm; the filterbank
  librosa.filters.mel(sr, 400, n_mels=40, fmin=0, fmax=sr/2, htk=False, norm='slaney') (`mel_filterbank`: Slaney scale, 42 edges
  equally spaced in mel on 0..8000 Hz, triangles at f_k = k sr / n_fft, each row scaled by 2 / (e_{i+2} - e_i)); it is not the
  HTK-scale table of losses._mel_filterbank.
  Partial windows (compute_partial_slices(n, rate=1.3, min_coverage=0.75)): `partial_slices` is the literal loop,
  `window_count` the closed form the kernels use. The row is zero-padded to L' = max(n, last window's end); the mel
  spectrogram is that of the padded row (reflect padding mirrors about sample L' - 1; samples at and past n count as zero).
  Network: torch.nn.LSTM(40, 256, 3, batch_first=True) (gate order i, f, g, o; both biases; zero initial state), the top layer's
  hidden state after the 160th frame, e = relu(linear(h)), e / ||e||_2 without an epsilon (an all-zero e gives NaN as in the
  reference). Utterance embedding: the mean over the row's kept windows of their normalised embeddings, normalised again.
  Stated deviation: preprocess_wav's silence trimming uses webrtcvad, a third-party C library; **it is not reproduced, trimming is
  left to the caller**. Its volume step normalize_volume(wav, -30 dBFS, increase_only=True) is normalize=True (default False).
  Resampling to 16 kHz is `resample`'s job.

Everything runs in csrc/eval_speaker.hip (tdvc_voice_windows, tdvc_voice_gain, tdvc_voice_mel, tdvc_lstm_fwd, tdvc_voice_embed):
no CPU or ATen fallback, no host synchronisation, lengths stay on the device as int32, no atomics, fixed summation orders
(bit-identical from call to call), every launch capturable into a graph. `speaker_similarity` is a few hundred elements of
stock torch ops on whatever device its inputs live on, as infer.shift_f0 is.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _host as H
from . import _lib as L

SR, N_FFT, HOP, N_MELS, PARTIAL_FRAMES, HIDDEN, EMBED, LAYERS = 16000, 400, 160, 40, 160, 256, 256, 3
PAD_MODES = ('reflect', 'constant')


# ---------------------------------------------------------------------------------------------------------- host definitions
def hz_to_mel(f):
    """Slaney mel scale (librosa.hz_to_mel(htk=False)): linear below 1000 Hz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_edges():
    """The 42 band edges in Hz."""
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(SR / 2.0), N_MELS + 2))


def mel_filterbank():
    """float64 [40, 201]: librosa.filters.mel(16000, 400, n_mels=40, htk=False, norm='slaney')."""
    def build():
        e = mel_edges()
        fk = np.arange(N_FFT // 2 + 1, dtype=np.float64) * SR / N_FFT
        lower = (fk[None, :] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None]
        upper = (e[2:, None] - fk[None, :]) / (e[2:] - e[1:-1])[:, None]
        fb = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (e[2:] - e[:-2]))[:, None]
        fb.setflags(write=False)
        return fb
    return H.host_table('speaker_mel_fb', build)


def _tables(device):
    """float64 [400 cos | 400 sin | 400 Hann | 40 x 201 filterbank] on the device, uploaded once."""
    return H.device_table(device, 'speaker_tables', lambda: np.concatenate([H.dft_tables(N_FFT, (0.5, 0.5)), mel_filterbank().reshape(-1)]))


def frame_step(rate=1.3):
    """int(round((sr / rate) / 160)): 77 at the default rate."""
    if not (rate > 0 and math.isfinite(rate)):
        raise ValueError('speaker: rate must be positive and finite')
    step = int(np.round((SR / rate) / HOP))
    if step < 1:
        raise ValueError(f'speaker: rate {rate} gives a frame step of 0')
    return step


def partial_slices(n_samples, rate=1.3, min_coverage=0.75):
    """Resemblyzer's compute_partial_slices, the literal loop -> (wav_slices, mel_slices). It documents the definition and serves
    the tests; the kernels use `window_count`."""
    assert 0 < rate and 0 < min_coverage <= 1
    n_frames = int(np.ceil((n_samples + 1) / HOP))
    step = int(np.round((SR / rate) / HOP))
    assert 0 < step
    steps = max(1, n_frames - PARTIAL_FRAMES + step + 1)
    wav_slices, mel_slices = [], []
    for i in range(0, steps, step):
        mel_range = np.array([i, i + PARTIAL_FRAMES])
        wav_range = mel_range * HOP
        mel_slices.append(slice(*mel_range))
        wav_slices.append(slice(*wav_range))
    last = wav_slices[-1]
    coverage = (n_samples - last.start) / (last.stop - last.start)
    if coverage < min_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


def window_count(n_samples, rate=1.3, min_coverage=0.75):
    """(number of kept windows, padded length L') of a row of n_samples: tdvc_voice_window_count, the closed form the kernels
    evaluate from the device lengths. Window j starts at mel frame j * frame_step(rate)."""
    padded = C.c_int64(0)
    cnt = L.lib().tdvc_voice_window_count(int(n_samples), frame_step(rate), float(min_coverage), C.byref(padded))
    if cnt < 1:
        raise ValueError(f'speaker: {n_samples} samples at rate {rate} are outside what the kernels take')
    return cnt, padded.value


# ------------------------------------------------------------------------------------------------------------------ operators
def _front(who, signal, lengths, rate, min_coverage, normalize, pad_mode):
    """-> (mel [B, F, 40], lengths int32 or None, frame step, P_max)"""
    H.need_device(who, signal)
    if pad_mode not in PAD_MODES:
        raise ValueError(f'{who}: unknown pad_mode {pad_mode!r} (known: {PAD_MODES})')
    if not (min_coverage == min_coverage):
        raise ValueError(f'{who}: min_coverage is NaN')
    x2, bs, _ = H.rows2(who, signal)
    B, T = x2.shape
    lengths = H.device_lengths(who, lengths, B, x2.device)
    step = frame_step(rate)
    if pad_mode == 'reflect' and T <= N_FFT // 2:
        raise ValueError(f'{who}: reflect padding needs T > 200 samples')
    P_max, padded = window_count(T, rate, min_coverage)
    F = 1 + padded // HOP
    lib = L.lib()
    gain = None
    if normalize:
        gain = torch.empty(B, dtype=torch.float64, device=x2.device)
        H.check(who, lib.tdvc_voice_gain(x2.data_ptr(), bs, H.ptr(lengths), T, B, gain.data_ptr(), H.stream(x2)))
    mel = torch.empty(B, F, N_MELS, dtype=torch.float32, device=x2.device)
    H.check(who, lib.tdvc_voice_mel(x2.data_ptr(), bs, H.ptr(lengths), T, B, F, step, float(min_coverage), int(pad_mode == 'constant'),
                                    H.ptr(gain), _tables(x2.device).data_ptr(), mel.data_ptr(), H.stream(x2)))
    return mel, lengths, step, P_max


def voice_mel(signal, lengths=None, pad_mode='reflect', normalize=False):
    """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz) -> the encoder's mel power spectrogram, fp32 [B, F, 40] with
    F = 1 + L'(T) // 160: tdvc_voice_mel, one launch (two with normalize). lengths: device integers [B]; samples at and past them
    are never read, and a row's frames at and past 1 + L'(lengths[b]) // 160 are zeros. Rows are strided views (nothing is
    copied unless the last axis is not dense). The windows are those of the default rate and min_coverage."""
    return _front('voice_mel', signal, lengths, 1.3, 0.75, normalize, pad_mode)[0]


def lstm_fwd(frames, slots, weights, counts=None, P_max=0, T_steps=PARTIAL_FRAMES):
    """The recurrence alone: frames [B, F, I] (device fp32, I <= 256, any batch and frame stride), slots int32 [P, 2] = (row, start
    frame), weights = [(w_ih, w_hh, b_ih, b_hh)] for 1 to 3 layers of 256 units -> the top layer's hidden state after T_steps <= 160
    frames, fp32 [P, 256]. With counts (device int32 [B]) slot p is used when p % P_max < counts[row]; unused slots are zeroed and
    frames no used window covers are never used. tdvc_lstm_fwd."""
    who = 'lstm_fwd'
    H.need_device(who, frames, slots)
    if frames.dim() != 3:
        raise ValueError(f'{who}: frames must be [B, F, I]')
    f3, f_bs, f_fs = H.frames3(who, frames)
    B, F, I = f3.shape
    if slots.dim() != 2 or slots.shape[1] != 2:
        raise ValueError(f'{who}: slots must be [P, 2]')
    slots = slots.to(torch.int32).contiguous()
    P = slots.shape[0]
    layers = len(weights)
    flat = []
    for l, ws in enumerate(weights):
        want = [(4 * HIDDEN, I if l == 0 else HIDDEN), (4 * HIDDEN, HIDDEN), (4 * HIDDEN,), (4 * HIDDEN,)]
        if len(ws) != 4:
            raise ValueError(f'{who}: layer {l} needs (w_ih, w_hh, b_ih, b_hh)')
        for w, shape in zip(ws, want):
            H.need_device(who, w)
            if tuple(w.shape) != shape:
                raise ValueError(f'{who}: layer {l} weight of shape {tuple(w.shape)}, expected {shape}')
            flat.append(w.detach().float().contiguous())
    if counts is not None:
        H.need_device(who, counts)
        if counts.shape != (B,):
            raise ValueError(f'{who}: counts must be [{B}]')
        counts = counts.to(torch.int32).contiguous()
    lib = L.lib()
    wptr = (C.c_void_p * max(len(flat), 1))(*[w.data_ptr() for w in flat])
    ws_bytes = lib.tdvc_lstm_workspace(B, F, I, P, T_steps, layers)
    ws = H.scratch(ws_bytes, f3.device)
    out = torch.empty(P, HIDDEN, dtype=torch.float32, device=f3.device)
    H.check(who, lib.tdvc_lstm_fwd(f3.data_ptr(), f_bs, f_fs, B, F, I, slots.data_ptr(), H.ptr(counts), P, int(P_max), int(T_steps), layers,
                                   wptr, out.data_ptr(), ws.data_ptr(), ws_bytes, H.stream(f3)))
    return out


def _embed(who, h, B, P_max, counts, weight, bias, want_partial, want_utt):
    partial = torch.empty(B * P_max, EMBED, dtype=torch.float32, device=h.device) if want_partial else None
    utt = torch.empty(B, EMBED, dtype=torch.float32, device=h.device) if want_utt else None
    H.check(who, L.lib().tdvc_voice_embed(h.data_ptr(), B, P_max, H.ptr(counts), weight.data_ptr(), bias.data_ptr(), H.ptr(partial),
                                          H.ptr(utt), H.stream(h)))
    return partial, utt


class VoiceEncoder(torch.nn.Module):
    """Resemblyzer's VoiceEncoder: the same state_dict keys and shapes (lstm.weight_ih_l{0,1,2}, lstm.weight_hh_l{k},
    lstm.bias_ih_l{k}, lstm.bias_hh_l{k}, linear.weight, linear.bias). The stock modules are containers for the parameters and
    are never called: forward and embed_utterance run csrc/eval_speaker.hip."""

    def __init__(self):
        super().__init__()
        self.lstm = torch.nn.LSTM(N_MELS, HIDDEN, LAYERS, batch_first=True)
        self.linear = torch.nn.Linear(HIDDEN, EMBED)

    def _weights(self):
        return [tuple(getattr(self.lstm, f'{n}_l{k}') for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')) for k in range(LAYERS)]

    def _linear(self, who):
        w, b = self.linear.weight.detach().float().contiguous(), self.linear.bias.detach().float().contiguous()
        H.need_device(who, w, b)
        return w, b

    def forward(self, mels):
        """mels [P, 160, 40] (device fp32) -> the normalised window embeddings [P, 256]."""
        who = 'VoiceEncoder.forward'
        H.need_device(who, mels)
        if mels.dim() != 3 or mels.shape[1] != PARTIAL_FRAMES or mels.shape[2] != N_MELS:
            raise ValueError(f'{who}: mels must be [P, {PARTIAL_FRAMES}, {N_MELS}], got {tuple(mels.shape)}')
        P = mels.shape[0]
        slots = torch.zeros(P, 2, dtype=torch.int32, device=mels.device)
        slots[:, 0] = torch.arange(P, dtype=torch.int32, device=mels.device)
        h = lstm_fwd(mels, slots, self._weights())
        w, b = self._linear(who)
        return _embed(who, h, P, 1, None, w, b, True, False)[0]

    def embed_utterance(self, signal, lengths=None, rate=1.3, min_coverage=0.75, normalize=False, pad_mode='reflect', return_partials=False):
        """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz), lengths device integers [B] or None -> the utterance embeddings
        fp32 [B, 256]; with return_partials also the window embeddings [B, P_max, 256] (zeros behind a row's count) and the
        per-row window counts, device int32 [B]. Samples at and past lengths are never read. No host synchronisation: the buffers
        are sized from the padded width T alone."""
        who = 'embed_utterance'
        mel, lengths, step, P_max = _front(who, signal, lengths, rate, min_coverage, normalize, pad_mode)
        B, T = mel.shape[0], signal.shape[-1]
        counts = torch.empty(B, dtype=torch.int32, device=mel.device)
        slots = torch.empty(B * P_max, 2, dtype=torch.int32, device=mel.device)
        H.check(who, L.lib().tdvc_voice_windows(H.ptr(lengths), T, B, step, float(min_coverage), P_max, counts.data_ptr(), slots.data_ptr(),
                                                H.stream(mel)))
        h = lstm_fwd(mel, slots, self._weights(), counts=counts, P_max=P_max)
        w, b = self._linear(who)
        partial, utt = _embed(who, h, B, P_max, counts, w, b, return_partials, True)
        if return_partials:
            return utt, partial.view(B, P_max, EMBED), counts
        return utt


def load_voice_encoder(path, device):
    """A VoiceEncoder on `device` with the weights of `path`: a plain state dict or Resemblyzer's {'model_state': ...} checkpoint
    (its pretrained.pt), read with torch.load(weights_only=True). similarity_weight / similarity_bias (the GE2E loss's scale) are
    ignored, as Resemblyzer's own strict=False load does."""
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if isinstance(sd, dict) and 'model_state' in sd:
        sd = sd['model_state']
    sd = {k: v for k, v in sd.items() if k not in ('similarity_weight', 'similarity_bias')}
    enc = VoiceEncoder()
    enc.load_state_dict(sd, strict=True)
    return enc.to(device).eval()


def speaker_similarity(test_emb, test_target, ref_emb, ref_speaker, num_speakers):
    """What test_speaker_rec.py:163-180 computes. test_emb [N, 256] with target speakers test_target [N] int64, ref_emb [M, 256] with
    speakers ref_speaker [M] int64 -> dict(centroids [S, 256]: the plain mean of each speaker's reference embeddings, not
    re-normalised (NaN for a speaker without any); cos [N]: the cosine similarity of each test embedding to its target's centroid;
    pred [N]: the argmin over speakers of the Euclidean distance to the centroids, the lowest index winning ties; accuracy: the
    mean of pred == test_target). Stock torch ops on the inputs' device, no host synchronisation."""
    S = int(num_speakers)
    ref = ref_emb.float()
    onehot = torch.nn.functional.one_hot(ref_speaker.long(), S).to(ref.dtype)               # [M, S]
    centroids = (onehot.t() @ ref) / onehot.sum(0)[:, None]
    t = test_emb.float()
    tc = centroids[test_target.long()]
    cos = (t * tc).sum(1) / (t.norm(dim=1) * tc.norm(dim=1))
    d2 = ((t[:, None, :] - centroids[None, :, :]) ** 2).sum(-1)
    big = torch.where(torch.isnan(d2), torch.full_like(d2, float('inf')), d2)
    pred = (big == big.min(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # the first minimum
    return dict(centroids=centroids, cos=cos, pred=pred, accuracy=(pred == test_target.long()).float().mean())
