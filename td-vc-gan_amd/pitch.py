"""F0 extraction on the device: the reference's YIN pitch tracker (util/yin.py, `estimate` and its `soft` variant; the calls
train.py:238, :548 and :634 keep commented out) as one HIP launch per call (csrc/pitch_yin.hip, tdvc_yin_f0).

`yin_f0` has `estimate`'s signature and return value; `track_f0` gives the [B, 1, T/hop + 1] layout that `infer.convert`,
`infer.shift_f0` and `TrainStep` take. The difference function is summed directly in fp32 instead of through the reference's FFT
autocorrelation: same quantity, without the cancellation at its minimum.

The soft variant is differentiable: with `soft=True`, an input that requires grad and grad mode on, the F0 track carries a
`grad_fn` whose backward is tdvc_yin_soft_bwd (csrc/pitch_yin_bwd.hip: per-frame gradient, then a gather; no atomics). The hard
search is piecewise constant and the CMDF of `return_cmdf=True` is a diagnostic output: neither is differentiable.

`decoder='viterbi'` decodes the track over time instead of frame by frame: the counterpart of the reference's inference call
util.crepe.filtered_pitch(signal, "viterbi") (generate_with_target.py:139), whose torchcrepe decoder is a max-sum dynamic programme
with a triangular +-240 cent transition. Here the lattice is the CMDF the YIN launch already produces, decoded by
tdvc_viterbi_path (csrc/pitch_viterbi.hip); `viterbi_transition` builds the band table and `viterbi_path` is the raw decoder for a
caller with a lattice of its own; crepe.py is one: `crepe.crepe_decode(decoder='viterbi')` decodes the CREPE network's activations with
it, which is the reference's call itself (`crepe.Crepe.filtered_pitch(signal, 'viterbi')`).

`dio`, `stonemask` and `world_f0` are WORLD's F0 estimator and its refinement, the pyworld.dio + pyworld.stonemask step of the
reference's objective evaluation (test_scripts/common/test_mcd.py world_analyze), as HIP kernels in float64 (csrc/pitch_dio.hip,
tdvc_dio / tdvc_stonemask; the definition is written out in include/tdvc.h). Parity with pyworld is unchecked.
"""
import math
import weakref

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _host as H
from . import _lib as L


class _YinSoftFn(torch.autograd.Function):
    """Soft YIN on x2 [B, T] (rows x_bs apart, last axis dense). The forward is the plain tdvc_yin_f0 call (same bits as without
    autograd); the backward recomputes the forward's intermediates on the device from x2, which is all it keeps."""

    @staticmethod
    def forward(ctx, x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, return_cmdf):
        f0, cmdf = _launch(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, True, return_cmdf)
        ctx.save_for_backward(x2)
        ctx.args = (x_bs, sample_rate, tau_min, tau_max, stride, threshold)
        if not return_cmdf:
            return f0
        ctx.mark_non_differentiable(cmdf)
        return f0, cmdf

    @staticmethod
    @once_differentiable                    # the backward is a raw library call: a second derivative raises instead of returning a graph-less tensor
    def backward(ctx, gy, *_):
        (x2,) = ctx.saved_tensors
        x_bs, sample_rate, tau_min, tau_max, stride, threshold = ctx.args
        B, T = x2.shape
        gy = gy.contiguous().float()
        lib = L.lib()
        nbytes = lib.tdvc_yin_soft_bwd_workspace(B, T, tau_max, stride)
        ws = H.scratch(nbytes, x2.device)
        dx = torch.empty(B, T, dtype=torch.float32, device=x2.device)      # the kernel writes every element
        L.check(lib.tdvc_yin_soft_bwd(x2.data_ptr(), x_bs, B, T, tau_min, tau_max, stride, float(threshold), float(sample_rate),
                                      gy.data_ptr(), dx.data_ptr(), ws.data_ptr(), nbytes, H.stream(x2)))
        return (dx,) + (None,) * 7


def _launch(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf):
    """x2 [B, T] -> (f0 [B, n_frames], cmdf [B, n_frames, n] or None): one tdvc_yin_f0 call."""
    B, T = x2.shape
    lib = L.lib()
    nf = lib.tdvc_yin_num_frames(T, tau_max, stride)
    n = tau_max - 1 - tau_min
    f0 = torch.empty(B, max(nf, 0), dtype=torch.float32, device=x2.device)
    cmdf = torch.empty(B, max(nf, 0), max(n, 0), dtype=torch.float32, device=x2.device) if return_cmdf else None
    L.check(lib.tdvc_yin_f0(x2.data_ptr(), x_bs, B, T, tau_min, tau_max, stride, float(threshold), int(bool(soft)), float(sample_rate),
                            f0.data_ptr(), H.ptr(cmdf), H.stream(x2)))
    return f0, cmdf


def _yin(x, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf):
    """x [..., T] (device tensor, last axis dense) -> f0 [..., n_frames] (, cmdf [..., n_frames, tau_max - 1 - tau_min])."""
    H.need_device('yin_f0', x)
    x2, x_bs, lead = H.rows2('yin_f0', x, any_lead=True, keep_grad=True)
    if soft and x2.requires_grad and torch.is_grad_enabled():
        # differentiable path: the layout steps of rows2 are torch ops, so the gradient returns in the input's shape
        out = _YinSoftFn.apply(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, bool(return_cmdf))
        f0, cmdf = out if return_cmdf else (out, None)
    else:
        f0, cmdf = _launch(x2.detach(), x_bs, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf)
    nf, n = f0.shape[-1], tau_max - 1 - tau_min
    f0 = f0.reshape(*lead, nf)
    return (f0, cmdf.reshape(*lead, nf, n)) if return_cmdf else f0


DECODERS = (None, 'viterbi')
THETA = 100.0      # the reference's own sharpness of the CMDF (util/yin.py:132, _softsearch)
_checked_bands = {}      # id(lo tensor) -> (version, n, W) it was found in range for; the entry goes when the tensor does


def _mark_band_checked(lo, n, W):
    if id(lo) not in _checked_bands:
        weakref.finalize(lo, _checked_bands.pop, id(lo), None)
    _checked_bands[id(lo)] = (lo._version, n, W)


def _transition_host(tau_min, tau_max, half_width_cents):
    """(logw float64 [n, W], lo int64 [n]) in numpy; see viterbi_transition."""
    key = (int(tau_min), int(tau_max), float(half_width_cents))

    def build():
        n = key[1] - 1 - key[0]
        if n < 1 or not key[2] > 0:
            raise ValueError('viterbi_transition: needs tau_max - 1 - tau_min >= 1 states and a positive half width')
        c = 1200.0 * np.log2(np.arange(n, dtype=np.float64) + key[0] + 1)
        w = np.maximum(1.0 - np.abs(c[None, :] - c[:, None]) / key[2], 0.0)          # w[j, i], symmetric
        first = (w > 0).argmax(1)
        W = int((w > 0).sum(1).max())
        lo = np.minimum(first, n - W)                                                 # bands at the upper end are shifted down, not cut
        band = np.take_along_axis(w, lo[:, None] + np.arange(W)[None, :], 1)
        with np.errstate(divide='ignore'):
            logw = np.where(band > 0, np.log(band), -np.inf)
        logw.setflags(write=False); lo.setflags(write=False)
        return logw, lo
    return H.host_table(('viterbi_transition',) + key, build)


def viterbi_transition(tau_min, tau_max, half_width_cents=240.0, device=None):
    """Band table of the triangular pitch transition on the YIN lag lattice -> (logw [n, W] fp32, lo [n] int32) on `device` (default:
    the current CUDA/ROCm device), n = tau_max - 1 - tau_min states, state s = lag s + tau_min + 1.
        c_s = 1200 * log2(s + tau_min + 1);  w(i, j) = max(1 - |c_i - c_j| / half_width_cents, 0);  logw = log(w) where w > 0
    Slot k of row j is predecessor i = lo[j] + k; slots outside the triangle hold -inf; W is the widest band. The table is symmetric
    and NOT row-normalised: the lag lattice is not uniform in cents, so normalising rows in the lag domain would favour short or
    long lags. Built in numpy float64, rounded once, cached per argument tuple and device."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(tau_min), int(tau_max), float(half_width_cents))

    def upload(host, device):
        logw, lo = host
        t = (torch.from_numpy(logw.astype(np.float32)).to(device), torch.from_numpy(lo.astype(np.int32)).to(device))
        _mark_band_checked(t[1], logw.shape[0], logw.shape[1])      # in range by construction
        return t
    return H.device_table(device, ('viterbi_transition',) + key, lambda: _transition_host(*key), upload)


def viterbi_path(x, logw, lo, scale=1.0, prior=None, jump=math.inf):
    """Best path through a lattice x [..., F, n] (device tensor, last axis dense) -> int64 [..., F] state indices: the banded
    max-sum decoder tdvc_viterbi_path (include/tdvc.h has the recursion and the tie rules: lowest predecessor, lowest final state).
        obs[f][j] = scale * x[f][j] + prior[j];  transition max(logw[j][i - lo[j]], -jump) inside the band, -jump outside it
    logw [n, W] fp32 and lo [n] int32 are a band table such as `viterbi_transition` returns; prior [n] or None; jump = inf
    disables the floor. A lo tensor that did not come from `viterbi_transition` is checked on the host the first time it is seen (one
    synchronisation; pass the same int32 device tensor again and it is not repeated): a band that leaves [0, n) raises ValueError. One launch; not differentiable."""
    H.need_device('viterbi_path', x)
    x3, x_bs, x_fs = H.frames3('viterbi_path', x)
    lead, (B, F, n) = x.shape[:-2], x3.shape
    if logw.dim() != 2 or logw.shape[0] != n or lo.shape != (n,):
        raise ValueError(f'viterbi_path: band table {tuple(logw.shape)} / {tuple(lo.shape)} does not match {n} states')
    logw = logw.to(device=x.device, dtype=torch.float32).contiguous()
    lo = lo.to(device=x.device, dtype=torch.int32).contiguous()
    W = logw.shape[1]
    if _checked_bands.get(id(lo)) != (lo._version, n, W):
        if n > 0 and W > 0 and (int(lo.min()) < 0 or int(lo.max()) + W > n):
            raise ValueError(f'viterbi_path: a band of {W} slots leaves [0, {n})')
        _mark_band_checked(lo, n, W)
    if prior is not None:
        prior = prior.to(device=x.device, dtype=torch.float32).contiguous()
        if prior.shape != (n,):
            raise ValueError(f'viterbi_path: prior must be [{n}]')
    lib = L.lib()
    path = torch.empty(B, F, dtype=torch.int32, device=x.device)
    nbytes = lib.tdvc_viterbi_workspace(B, F, n)
    ws = H.scratch(nbytes, x.device)
    L.check(lib.tdvc_viterbi_path(x3.data_ptr(), x_bs, x_fs, float(scale), H.ptr(prior), logw.data_ptr(), lo.data_ptr(), W, float(jump),
                                  B, F, n, path.data_ptr(), F, ws.data_ptr(), nbytes, H.stream(x)))
    return path.reshape(*lead, F).long()


def _check_decoder(who, decoder, soft):
    if decoder not in DECODERS:
        raise ValueError(f'{who}: unknown decoder {decoder!r} (known: {DECODERS})')
    if decoder is not None and soft:
        raise ValueError(f"{who}: decoder='viterbi' gives a path, which is not differentiable; it cannot be combined with soft=True")


def _viterbi_f0(x, sample_rate, tau_min, tau_max, stride, threshold, octave_cost, jump_cost, return_cmdf):
    """The hard YIN call with its CMDF, then the decoded lag on the frames the hard track calls voiced."""
    hard, cmdf = _yin(x, sample_rate, tau_min, tau_max, stride, threshold, False, True)
    n = cmdf.shape[-1]
    logw, lo = viterbi_transition(tau_min, tau_max, device=cmdf.device)
    prior = H.device_table(cmdf.device, ('viterbi prior', tau_min, tau_max, float(octave_cost)), lambda: (
        -float(octave_cost) * np.log2((np.arange(n, dtype=np.float64) + tau_min + 1) / (tau_min + 1))).astype(np.float32))
    path = viterbi_path(cmdf, logw, lo, scale=-THETA, prior=prior, jump=float(jump_cost))
    f0 = torch.where(hard != 0, sample_rate / (path + (tau_min + 1)).to(torch.float32), torch.zeros_like(hard))
    return (f0, cmdf) if return_cmdf else f0


def yin_f0(signal, sample_rate, pitch_min=20, pitch_max=20000, frame_stride=0.01, threshold=0.1, soft=False, return_cmdf=False,
           decoder=None, octave_cost=1.0, jump_cost=16.0):
    """YIN pitch of a signal [T], [B, T] or [..., T] -> [..., n_frames] in Hz, 0 = non-periodic frame (reference: util/yin.py:24-85,
    same arguments). Frames of 2*sample_rate/pitch_min samples every frame_stride seconds; n_frames = (max(T, L) - 1) // stride + 1.
    return_cmdf=True also returns the cumulative-mean-normalised difference [..., n_frames, tau_max - 1 - tau_min].
    soft=True on a signal that requires grad gives a differentiable track (the gradient has the signal's shape); the hard track
    and the CMDF carry no grad_fn.
    decoder='viterbi' replaces the per-frame lag by the best path through the CMDF of the same launch (see `track_f0`)."""
    _check_decoder('yin_f0', decoder, soft)
    tau_min = int(sample_rate / pitch_max)
    tau_max = int(sample_rate / pitch_min)
    stride = int(frame_stride * sample_rate)
    if decoder == 'viterbi':
        return _viterbi_f0(signal, sample_rate, tau_min, tau_max, stride, threshold, octave_cost, jump_cost, return_cmdf)
    return _yin(signal, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf)


def track_f0(signal, hop=64, sample_rate=16000, pitch_min=60, pitch_max=500, threshold=0.1, soft=False, decoder=None, octave_cost=1.0,
             jump_cost=16.0):
    """signal [B, 1, T] -> F0 track [B, 1, T // hop + 1] in Hz, 0 = unvoiced: the frame count of the reference's CREPE front end
    (pad=True; `crepe.Crepe.filtered_pitch` is that tracker itself), which is what `infer.convert`, `infer.shift_f0` and `TrainStep` take. YIN yields T // hop frames for an utterance
    of whole hops, so the last frame is repeated once; `f0_to_excitation` drops that frame, as the reference does.
    soft=True selects the softmax-weighted period, differentiable with respect to a signal that requires grad.
    decoder='viterbi' (the reference's inference setting, generate_with_target.py:139) decodes the lag over time: the best path
    through obs = -100 * CMDF - octave_cost * log2(lag / lag_min) under the triangular +-240 cent transition of
    `viterbi_transition` with a uniform floor of -jump_cost, so that a pitch reset costs jump_cost instead of being impossible.
    f0 = sample_rate / lag of the path on the frames the hard tracker calls voiced and 0 elsewhere: voicing decisions are
    exactly those of decoder=None. octave_cost = 1 and jump_cost = 16 were chosen on synthetic signals (a glide whose fundamental
    fades against its second harmonic under noise, and the pitch resets of the test fixtures), not on speech; 0.5 .. 1 and
    10 .. 16 gave the same tracks there. Not differentiable: with soft=True it raises ValueError."""
    if signal.dim() != 3 or signal.shape[1] != 1:
        raise ValueError('track_f0: signal must be [B, 1, T]')
    _check_decoder('track_f0', decoder, soft)
    T = signal.shape[-1]
    tau_min, tau_max = int(sample_rate / pitch_max), int(sample_rate / pitch_min)
    if decoder == 'viterbi':
        f0 = _viterbi_f0(signal[:, 0], sample_rate, tau_min, tau_max, int(hop), threshold, octave_cost, jump_cost, False)
    else:
        f0 = _yin(signal[:, 0], sample_rate, tau_min, tau_max, int(hop), threshold, soft, False)
    idx = torch.arange(T // int(hop) + 1, device=f0.device).clamp_(max=f0.shape[-1] - 1)
    return f0.index_select(-1, idx).unsqueeze(1)


# ------------------------------------------------------------------------------------------------------------ WORLD's DIO + StoneMask
def _world_rows(who, signal, lengths):
    H.need_device(who, signal)
    x2, x_bs, lead = H.rows2(who, signal)
    return x2, x_bs, lead, H.device_lengths(who, lengths, x2.shape[0], x2.device, move=True, any_shape=True)


def dio(signal, sample_rate=16000, hop=80, f0_floor=50.0, f0_ceil=500.0, channels_in_octave=2.0, allowed_range=0.1, lengths=None,
        return_candidates=False):
    """WORLD's DIO F0 track of signal [T], [B, T] or [B, 1, T] (device fp32, last axis dense) -> fp32 [..., T // hop + 1] in Hz, 0 =
    unvoiced: the counterpart of pyworld.dio(x, fs, f0_floor, f0_ceil, channels_in_octave, frame_period = 1000 hop / fs,
    allowed_range) without decimation (speed = 1); tdvc_dio (csrc/pitch_dio.hip), the definition in include/tdvc.h. Frame i is at
    sample i * hop. lengths: device integers, valid samples per row; samples at and past them are never read, and frames past
    lengths[b] // hop are 0. Rows of a wider buffer go in as views. return_candidates=True also returns the per-band candidates and
    scores, float64 [..., n_bands, T // hop + 1] each. Float64 arithmetic, seven launches, no host synchronisation.
    **Parity with pyworld is unchecked**; both band-limiting filters are linear convolutions where WORLD's FFT product is circular.
    At most 16 bands, 2^21 samples per row, filters of 2048 taps (any fs up to 51 kHz with f0_floor >= fs / 1449)."""
    x2, x_bs, lead, ln = _world_rows('dio', signal, lengths)
    B, T = x2.shape
    hop, fs = int(hop), int(sample_rate)
    if hop < 1 or fs != sample_rate:
        raise ValueError('dio: needs an integer sample rate and hop >= 1')
    par = (float(f0_floor), float(f0_ceil), float(channels_in_octave))
    lib = L.lib()
    F = T // hop + 1
    nb = lib.tdvc_dio_num_bands(*par)
    f0 = torch.empty(B, F, dtype=torch.float32, device=x2.device)
    cand = torch.empty(B, max(nb, 0), F, dtype=torch.float64, device=x2.device) if return_candidates else None
    score = torch.empty_like(cand) if return_candidates else None
    nbytes = lib.tdvc_dio_workspace(B, T, F, hop, fs, *par)
    ws = H.scratch(nbytes, x2.device)
    H.check('dio', lib.tdvc_dio(x2.data_ptr(), x_bs, 1, H.ptr(ln), T, B, F, hop, fs, *par, float(allowed_range), f0.data_ptr(), F, H.ptr(cand),
                                H.ptr(score), ws.data_ptr(), nbytes, H.stream(x2)))
    f0 = f0.reshape(*lead, F)
    return (f0, cand.reshape(*lead, nb, F), score.reshape(*lead, nb, F)) if return_candidates else f0


def stonemask(signal, f0, sample_rate=16000, hop=80, lengths=None):
    """WORLD's StoneMask refinement of the track f0 [..., F] (Hz; any strides) on signal [T], [B, T] or [B, 1, T] -> fp32 [..., F]: the
    counterpart of pyworld.stonemask(x, f0, t, fs) with frame i at sample i * hop; tdvc_stonemask (csrc/pitch_dio.hip), one launch,
    the definition in include/tdvc.h. Frames with f0 not finite, <= 40 Hz or > fs / 12 give 0; a refinement more than 20 % off
    returns its input. lengths as in `dio` (the window repeats the first and the last valid sample). **Parity with pyworld is
    unchecked**; the track is fp32 where WORLD's is float64."""
    x2, x_bs, lead, ln = _world_rows('stonemask', signal, lengths)
    H.need_device('stonemask', f0)
    B, T = x2.shape
    if f0.dim() < 1 or tuple(f0.shape[:-1]) != lead:
        raise ValueError(f'stonemask: the track must be {list(lead)} + [n_frames], one row per signal row')
    hop, fs = int(hop), int(sample_rate)
    if hop < 1 or fs != sample_rate:
        raise ValueError('stonemask: needs an integer sample rate and hop >= 1')
    F = f0.shape[-1]
    f = f0.detach().float()
    f2 = f if f.dim() == 2 else f.reshape(B, F)
    out = torch.empty(B, F, dtype=torch.float32, device=x2.device)
    H.check('stonemask', L.lib().tdvc_stonemask(x2.data_ptr(), x_bs, 1, H.ptr(ln), T, f2.data_ptr(), f2.stride(0) if B > 1 else F,
                                                 f2.stride(1) if F > 1 else 1, B, F, hop, fs, out.data_ptr(), F, H.stream(x2)))
    return out.reshape(*lead, F)


def world_f0(signal, sample_rate=16000, hop=80, f0_floor=50.0, f0_ceil=500.0, channels_in_octave=2.0, allowed_range=0.1, lengths=None):
    """stonemask(signal, dio(signal, ...)): the F0 track of the reference's world_analyze, -> fp32 [..., T // hop + 1]. DIO's track
    passes through one fp32 rounding between the two steps, where WORLD keeps float64. **Parity with pyworld is unchecked.**"""
    f0 = dio(signal, sample_rate, hop, f0_floor, f0_ceil, channels_in_octave, allowed_range, lengths)
    return stonemask(signal, f0, sample_rate, hop, lengths)
