"""The CREPE pitch tracker on the device: the reference's util/crepe.py `filtered_pitch` (train.py:239, :549, :635;
generate_with_target.py:139, :161 with "viterbi"; generate_from_list.py:101, :104), which runs torchcrepe's `tiny` network at hop 64,
masks the bins to 50-550 Hz, decodes, and thresholds the periodicity at 0.21. torchcrepe is not available here and no weights are
shipped, so the definition below (also in include/tdvc.h), written from torchcrepe's published source, is the contract and
tests/crepe_ref.py restates it in float64 with stock torch ops; **parity with an installed torchcrepe and with its shipped
`tiny.pth` is unchecked**, and so are the state-dict keys against a real file and `full` beyond one row.

Definition.
  Constants: 360 bins of 20 cents; cents(bin) = 20 bin + 1997.3794084376191; hz(cents) = 10 2^(cents / 1200);
    bin(hz, q) = q((1200 log2(hz / 10) - 1997.3794084376191) / 20), q = floor unless stated. Sample rate 16000 (any other rate is
    refused: `resample` exists), window 1024.
  Front end (preprocess, pad=True): the row is zero-padded by 512 on both sides; F = 1 + T // hop frames of 1024 samples every hop
    samples; each frame loses its mean and is divided by max(1e-10, std), std the unbiased (n - 1) standard deviation.
  Network (capacity 'tiny' | 'full'): output channels [128, 16, 16, 16, 32, 64] | [1024, 128, 128, 128, 256, 512]; six layers, each
    zero-pad -> conv -> ReLU -> BatchNorm in eval mode (eps 0.0010000000474974513) -> max-pool 2. Layer 1: 1 -> C1, kernel 512, stride
    4, pad (254, 254): 1024 -> 256 -> 128 positions; layers 2-6: kernel 64, stride 1, pad (31, 32): 128 -> 64 -> 32 -> 16 -> 8 -> 4
    positions after each pool. The BatchNorm comes after the ReLU and its scale may be negative: the pool cannot be moved in front of
    the affine. The result [N, C6, 4] is flattened position-major (permute(0, 2, 1), index l C6 + c), then Linear(., 360) and a sigmoid.
  State-dict keys (torchcrepe's): conv1..conv6 .weight [Cout, Cin, K, 1] and .bias; conv1_BN..conv6_BN .weight, .bias, .running_mean,
    .running_var, .num_batches_tracked; classifier.weight, classifier.bias. Load is strict both ways.
  Post-processing (postprocess and util/crepe.py:55-84) on activations [B, 360, F]: bins below minidx = bin(fmin) and from maxidx =
    bin(fmax, ceil) on are excluded (39 and 248 for 50 and 550 Hz; float64 on the host).
    argmax: the lowest index on ties; pitch hz(cents(bin)).
    weighted_argmax: the window [max(0, b - 4), min(360, b + 5)) around the argmax bin b; weights sigmoid(activation) inside the window
      and the range, 0 outside (torchcrepe's second sigmoid on values that are already probabilities, kept); hz(sum w cents / sum w).
    viterbi: observation = log-softmax over the in-range bins; transition max(12 - |i - j|, 0), row-normalised over all 360 bins;
      uniform initial distribution; decoded by `pitch.viterbi_path` on the maxidx - minidx in-range states with jump = inf. This
      equals librosa's programme whenever that avoids its `tiny`-floored transitions, which it always does: staying on a state is
      always possible at finite cost.
    Periodicity = the activation at the chosen bin; pitch = 0 where periodicity < threshold (0.21).
    get_shift(src, tgt) = bin(tgt) - bin(src).
  Stated deviation: torchcrepe adds a random triangular dither of +-20 cents to every bin -> cents conversion; here the conversion is
    deterministic (the dither's mean).
  Decisions where the source leaves room: with per-row `lengths` a row is framed as if it were alone (samples at and past its length
    are never read and count as zero); its frames past 1 + length // hop are zero frames, the activations there are those of a zero
    frame, and `crepe_decode(lengths=frame counts)` gives pitch 0 and periodicity 0 there. The Viterbi decoder looks at the whole row,
    so it refuses per-row frame counts: decode such rows one at a time. The threshold comparison is made in fp32.

Out of scope: the activation-MSE `lambda_f0` term of train.py:439-470 (a backward pass through this network, `roll_batches`),
`TrainStep`, `bench.py` and `smoke()`: forward and inference only.

Everything runs in csrc/pitch_crepe.hip (tdvc_crepe_frames, tdvc_crepe_conv, tdvc_crepe_head, tdvc_crepe_decode) and, for the Viterbi
decoder, csrc/pitch_viterbi.hip: no CPU or ATen fallback, no host synchronisation, no atomics, fixed summation orders (bit-identical
from call to call, a row's result does not depend on its batch), every launch capturable into a graph.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _host as H
from . import _lib as L

SR, WINDOW, BINS, CENTS_PER_BIN, CENTS0 = 16000, 1024, 360, 20, 1997.3794084376191
BN_EPS = 0.0010000000474974513
CAPACITIES = {'tiny': (128, 16, 16, 16, 32, 64), 'full': (1024, 128, 128, 128, 256, 512)}
DECODERS = ('argmax', 'weighted_argmax', 'viterbi')
FMIN, FMAX, THRESHOLD, HOP = 50.0, 550.0, 0.21, 64
BAND = 23      # predecessors of a state under max(12 - |i - j|, 0)


# ---------------------------------------------------------------------------------------------------------- host definitions
def bins_to_cents(bins):
    return CENTS_PER_BIN * np.asarray(bins, dtype=np.float64) + CENTS0


def cents_to_hz(cents):
    return 10.0 * 2.0 ** (np.asarray(cents, dtype=np.float64) / 1200.0)


def hz_to_bins(hz, quantize=np.floor):
    """bin(hz, q) in float64 -> int64 (numpy scalar or array)."""
    cents = 1200.0 * np.log2(np.asarray(hz, dtype=np.float64) / 10.0)
    return quantize((cents - CENTS0) / CENTS_PER_BIN).astype(np.int64)


def bin_range(fmin=FMIN, fmax=FMAX):
    """-> (minidx, maxidx): the bins [minidx, maxidx) stay in range. Refuses fmin >= fmax and a range with no bin."""
    fmin, fmax = float(fmin), float(fmax)
    if not (0.0 < fmin < fmax) or not math.isfinite(fmax):
        raise ValueError(f'crepe: needs 0 < fmin < fmax, got {fmin}, {fmax}')
    lo, hi = max(int(hz_to_bins(fmin)), 0), min(int(hz_to_bins(fmax, np.ceil)), BINS)
    if lo >= hi:
        raise ValueError(f'crepe: no bin between {fmin} and {fmax} Hz')
    return lo, hi


def num_frames(T, hop=HOP):
    return 1 + int(T) // int(hop)


def get_shift(pitch_source, pitch_target):
    """util/crepe.py get_shift: bin(target) - bin(source), floor-quantised; tensors (any device, stock torch ops) or numbers in Hz."""
    if torch.is_tensor(pitch_source) or torch.is_tensor(pitch_target):
        q = lambda f: torch.floor((1200.0 * torch.log2(torch.as_tensor(f).double() / 10.0) - CENTS0) / CENTS_PER_BIN).long()
        return q(pitch_target) - q(pitch_source)
    return hz_to_bins(pitch_target) - hz_to_bins(pitch_source)


def _transition_host(minidx, maxidx):
    """(logw float64 [n, W], lo int64 [n]) of the states minidx..maxidx - 1, W = min(23, n); see crepe_transition."""
    key = (int(minidx), int(maxidx))

    def build():
        lo_bin, hi_bin = key
        if not 0 <= lo_bin < hi_bin <= BINS:
            raise ValueError(f'crepe_transition: the states [{lo_bin}, {hi_bin}) must lie in [0, {BINS})')
        i = np.arange(BINS)
        tri = np.maximum(12.0 - np.abs(i[:, None] - i[None, :]), 0.0)          # tri[i, j]: from bin i to bin j
        trans = tri / tri.sum(1, keepdims=True)                                 # rows normalised over all 360 bins
        n = hi_bin - lo_bin
        W = min(BAND, n)
        j = np.arange(n) + lo_bin
        lo = np.clip(j - BAND // 2 - lo_bin, 0, n - W)                          # bands at both ends are shifted, not cut
        pred = lo[:, None] + np.arange(W)[None, :] + lo_bin                     # predecessor bin of slot k of state j
        p = trans[pred, j[:, None]]
        with np.errstate(divide='ignore'):
            logw = np.where(p > 0, np.log(p), -np.inf)
        logw.setflags(write=False); lo.setflags(write=False)
        return logw, lo
    return H.host_table(('crepe_transition',) + key, build)


def crepe_transition(minidx=0, maxidx=BINS, device=None):
    """Band table of torchcrepe's Viterbi transition for `pitch.viterbi_path` -> (logw [n, W] fp32, lo [n] int32) on `device`: the n =
    maxidx - minidx in-range states (state s is bin s + minidx), W = min(23, n) slots, slot k of state j is predecessor lo[j] + k,
    logw = log(max(12 - |i - j|, 0) / sum_j' max(12 - |i - j'|, 0)) with the sum over ALL 360 bins (the row of the source bin i), -inf
    outside the triangle. Built in float64, rounded once, cached per range and device."""
    from .pitch import _mark_band_checked
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(minidx), int(maxidx))

    def upload(host, device):
        logw, lo = host
        t = (torch.from_numpy(logw.astype(np.float32)).to(device), torch.from_numpy(lo.astype(np.int32)).to(device))
        _mark_band_checked(t[1], logw.shape[0], logw.shape[1])      # in range by construction
        return t
    return H.device_table(device, ('crepe_transition',) + key, lambda: _transition_host(*key), upload)


# ------------------------------------------------------------------------------------------------------------------ operators
def _check_rate(who, sample_rate):
    if sample_rate != SR:
        raise ValueError(f'{who}: the network takes {SR} Hz audio, got {sample_rate} (resample first: tdvc_amd.resample)')


def crepe_frames(signal, hop=HOP, lengths=None, sample_rate=SR):
    """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz) -> the normalised frames fp32 [B, F, 1024], F = 1 + T // hop
    (tdvc_crepe_frames, one launch). lengths: device integers [B]; samples at and past them are never read, and a row's frames past
    1 + length // hop are zeros. Rows are strided views (nothing is copied unless the last axis is not dense)."""
    who = 'crepe_frames'
    _check_rate(who, sample_rate)
    H.need_device(who, signal)
    x2, bs, _ = H.rows2(who, signal)
    B, T = x2.shape
    lengths = H.device_lengths(who, lengths, B, x2.device)
    hop = int(hop)
    if hop < 1:
        raise ValueError(f'{who}: hop must be at least 1, got {hop}')
    if T < 1:
        raise ValueError(f'{who}: rows with no sample are refused')
    F = num_frames(T, hop)
    frames = torch.empty(B, F, WINDOW, dtype=torch.float32, device=x2.device)
    H.check(who, L.lib().tdvc_crepe_frames(x2.data_ptr(), bs, H.ptr(lengths), T, B, hop, F, frames.data_ptr(), H.stream(x2)))
    return frames


def crepe_conv(x, weight, bias, scale, shift, stride=1, out=None):
    """One conv block (tdvc_crepe_conv): x [N, Cin, Lin] dense fp32, weight [Cout, Cin, K(, 1)] -> maxpool2(relu(conv(x) + bias) scale +
    shift) fp32 [N, Cout, Lc / 2]; (Cin 1, K 512, stride 4, Lin 1024: Lc = 256) or (K 64, stride 1, Lin in 128, 64, 32, 16, 8: Lc =
    Lin); Cout and (K 64) Cin multiples of 16."""
    who = 'crepe_conv'
    H.need_device(who, x, weight)
    if x.dim() != 3 or weight.dim() not in (3, 4) or (weight.dim() == 4 and weight.shape[3] != 1):
        raise ValueError(f'{who}: x must be [N, Cin, Lin] and weight [Cout, Cin, K(, 1)]')
    x = x.detach().float().contiguous()
    N, Cin, Lin = x.shape
    Cout, Wc, K = weight.shape[:3]
    if Wc != Cin:
        raise ValueError(f'{who}: x has {Cin} channels, the weight takes {Wc}')
    w = H.vec(who, weight, Cout * Cin * K, 'weight')
    bias, scale, shift = H.vec(who, bias, Cout, 'bias'), H.vec(who, scale, Cout, 'scale'), H.vec(who, shift, Cout, 'shift')
    lout = (Lin // int(stride) if stride else 0) // 2
    if out is None:
        out = torch.empty(N, Cout, lout, dtype=torch.float32, device=x.device)
    H.need_device(who, out)
    if tuple(out.shape) != (N, Cout, lout) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f'{who}: out must be contiguous fp32 [{N}, {Cout}, {lout}]')
    a = L.CrepeConvArgs()
    a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = N, Cin, Cout, Lin, K, int(stride)
    a.x, a.w, a.bias, a.scale, a.shift, a.y = x.data_ptr(), w.data_ptr(), bias.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr()
    H.check(who, L.lib().tdvc_crepe_conv(C.byref(a), H.stream(x)))
    return out


def crepe_head(x, weight, bias, frames_per_row=1):
    """tdvc_crepe_head: x [N, C, P] (the last block's output), weight [O, P C] over the position-major flatten, bias [O] ->
    sigmoid(Linear(x.permute(0, 2, 1).reshape(N, P C))) as fp32 [N / frames_per_row, O, frames_per_row] ([N, O] for 1)."""
    who = 'crepe_head'
    H.need_device(who, x, weight)
    if x.dim() != 3 or weight.dim() != 2:
        raise ValueError(f'{who}: x must be [N, C, P] and weight [O, P C]')
    x = x.detach().float().contiguous()
    N, Cc, P = x.shape
    O = weight.shape[0]
    Fr = int(frames_per_row)
    if Fr < 1 or N % Fr:
        raise ValueError(f'{who}: {N} frames are not whole rows of {Fr}')
    w, bias = H.vec(who, weight, O * P * Cc, 'weight'), H.vec(who, bias, O, 'bias')
    act = torch.empty((N // Fr, O, Fr) if Fr > 1 else (N, O), dtype=torch.float32, device=x.device)
    H.check(who, L.lib().tdvc_crepe_head(x.data_ptr(), N, Cc, P, w.data_ptr(), bias.data_ptr(), O, Fr, act.data_ptr(), H.stream(x)))
    return act


def _decode_call(who, act, lo, hi, mode, threshold, frames=None, bins=None):
    B, nb, F = act.shape
    dev = act.device
    lattice = pitch = per = None
    if mode == L.CREPE_LATTICE:
        lattice = torch.empty(B, F, hi - lo, dtype=torch.float32, device=dev)
    else:
        pitch, per = torch.empty(B, F, dtype=torch.float32, device=dev), torch.empty(B, F, dtype=torch.float32, device=dev)
    a_bs, a_cs = (act.stride(0) if B > 1 else nb * max(act.stride(1), F)), (act.stride(1) if nb > 1 else F)
    H.check(who, L.lib().tdvc_crepe_decode(act.data_ptr(), a_bs, a_cs, B, F, nb, lo, hi, mode, float(threshold), H.ptr(frames), H.ptr(bins),
                                           H.ptr(pitch), H.ptr(per), H.ptr(lattice), H.stream(act)))
    return lattice if mode == L.CREPE_LATTICE else (pitch, per)


def crepe_lattice(activations, fmin=FMIN, fmax=FMAX):
    """activations [B, 360, F] -> the Viterbi observations fp32 [B, F, maxidx - minidx]: the log-softmax over the in-range bins."""
    act, lo, hi = _decode_args('crepe_lattice', activations, fmin, fmax)
    return _decode_call('crepe_lattice', act, lo, hi, L.CREPE_LATTICE, 0.0)


def _decode_args(who, activations, fmin, fmax):
    lo, hi = bin_range(fmin, fmax)
    H.need_device(who, activations)
    if activations.dim() != 3 or activations.shape[1] != BINS:
        raise ValueError(f'{who}: activations must be [B, {BINS}, F], got {tuple(activations.shape)}')
    act = activations.detach().float()
    if act.shape[2] > 1 and act.stride(2) != 1:
        act = act.contiguous()
    return act, lo, hi


def crepe_decode(activations, fmin=FMIN, fmax=FMAX, decoder='argmax', threshold=THRESHOLD, lengths=None):
    """activations [B, 360, F] (device fp32; a view with dense frames stays a view) -> (pitch [B, F] in Hz, 0 = periodicity below the
    threshold; periodicity [B, F]): tdvc_crepe_decode, one launch ('viterbi': the lattice launch, `pitch.viterbi_path`, and the
    launch that reads the path). lengths: device integers [B], the rows' FRAME counts; frames at and past them give 0 and 0 (not with
    'viterbi', which looks at the whole row: ValueError)."""
    who = 'crepe_decode'
    if decoder not in DECODERS:
        raise ValueError(f'{who}: unknown decoder {decoder!r} (known: {DECODERS})')
    act, lo, hi = _decode_args(who, activations, fmin, fmax)
    frames = H.device_lengths(who, lengths, act.shape[0], act.device)
    if decoder == 'viterbi':
        if frames is not None:
            raise ValueError(f"{who}: decoder='viterbi' decodes a whole row; decode rows of different lengths one at a time")
        from .pitch import viterbi_path
        lattice = _decode_call(who, act, lo, hi, L.CREPE_LATTICE, 0.0)
        logw, band_lo = crepe_transition(lo, hi, device=act.device)
        bins = (viterbi_path(lattice, logw, band_lo) + lo).to(torch.int32)
        return _decode_call(who, act, lo, hi, L.CREPE_ARGMAX, threshold, bins=bins)
    return _decode_call(who, act, lo, hi, L.CREPE_WEIGHTED if decoder == 'weighted_argmax' else L.CREPE_ARGMAX, threshold, frames=frames)


def fold_bn(bn):
    """BatchNorm in eval mode as (scale, shift) fp32: scale = gamma / sqrt(var + eps), shift = beta - mean scale, evaluated in float64
    and rounded once."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


# -------------------------------------------------------------------------------------------------------------------- module
class Crepe(torch.nn.Module):
    """torchcrepe's Crepe(model): the same state_dict keys and shapes (the module docstring lists them), so that a tiny.pth / full.pth
    loads with strict=True. The stock modules are containers for the parameters and are never called: `activations` runs
    csrc/pitch_crepe.hip. The BatchNorms are folded to scale / shift once per device and again after load_state_dict or a move."""

    def __init__(self, capacity='tiny'):
        super().__init__()
        if capacity not in CAPACITIES:
            raise ValueError(f'Crepe: unknown capacity {capacity!r} (known: {tuple(CAPACITIES)})')
        self.capacity = capacity
        out = CAPACITIES[capacity]
        cin = (1,) + out[:-1]
        for i in range(6):
            k, s = (512, 4) if i == 0 else (64, 1)
            setattr(self, f'conv{i + 1}', torch.nn.Conv2d(cin[i], out[i], (k, 1), stride=(s, 1)))
            setattr(self, f'conv{i + 1}_BN', torch.nn.BatchNorm2d(out[i], eps=BN_EPS))
        self.in_features = 4 * out[-1]
        self.classifier = torch.nn.Linear(self.in_features, BINS)
        self._folded = {}
        self.eval()

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
            self._folded[k] = [fold_bn(getattr(self, f'conv{i}_BN')) for i in range(1, 7)]
        return self._folded[k]

    def embed_frames(self, frames):
        """Normalised frames [N, 1024] (device fp32) -> the last conv block's output fp32 [N, C6, 4]: six tdvc_crepe_conv launches."""
        who = 'Crepe.activations'
        H.need_device(who, frames, self.classifier.weight)
        fold = self._fold(frames.device)
        x = frames.reshape(-1, 1, WINDOW)
        for i in range(1, 7):
            conv = getattr(self, f'conv{i}')
            x = crepe_conv(x, conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0])
        return x

    @torch.no_grad()
    def activations(self, signal, hop=HOP, lengths=None, sample_rate=SR):
        """signal [B, 1, T] | [B, T] | [T] (device fp32, 16 kHz), lengths device integers [B] or None -> the activations fp32
        [B, 360, F], F = 1 + T // hop: tdvc_crepe_frames, six tdvc_crepe_conv, tdvc_crepe_head. No host synchronisation: the buffers
        are sized from the padded width T alone."""
        who = 'Crepe.activations'
        _check_rate(who, sample_rate)
        H.need_device(who, signal, self.classifier.weight)
        frames = crepe_frames(signal, hop, lengths)
        B, F, _ = frames.shape
        x = self.embed_frames(frames.view(B * F, WINDOW))
        return crepe_head(x, self.classifier.weight, self.classifier.bias, frames_per_row=F).view(B, BINS, F)

    forward = activations

    @torch.no_grad()
    def filtered_pitch(self, signal, decoder='argmax'):
        """util/crepe.py filtered_pitch: signal [B, 1, T] or [B, T] -> (pitches [B, 1, F] or [B, F] in Hz, 0 where the periodicity is below
        0.21; activations [B, 360, F]), F = 1 + T // 64, bins masked to 50-550 Hz, decoder 'argmax' | 'weighted_argmax' | 'viterbi'."""
        if decoder not in DECODERS:
            raise ValueError(f'Crepe.filtered_pitch: unknown decoder {decoder!r} (known: {DECODERS})')
        if signal.dim() not in (2, 3) or (signal.dim() == 3 and signal.shape[1] != 1):
            raise ValueError('Crepe.filtered_pitch: signal must be [B, 1, T] or [B, T]')
        act = self.activations(signal, HOP)
        pitch, _ = crepe_decode(act, FMIN, FMAX, decoder, THRESHOLD)
        return (pitch.unsqueeze(1) if signal.dim() == 3 else pitch), act


def _load_weights(path):
    if str(path).endswith('.npz'):
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in z.files}
    return torch.load(path, map_location='cpu', weights_only=True)


def load_crepe(path_or_state_dict, capacity='tiny', device='cpu'):
    """-> a Crepe(capacity) with the state dict (or the file: torch.load(weights_only=True), or an .npz of the same keys) loaded
    strictly, on `device`, in eval mode."""
    sd = path_or_state_dict if isinstance(path_or_state_dict, dict) else _load_weights(path_or_state_dict)
    model = Crepe(capacity)
    model.load_state_dict(sd, strict=True)
    return model.to(device).eval()
