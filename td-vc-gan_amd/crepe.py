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

The activation-MSE `lambda_f0` term of train.py:439-470 (g_loss_f0 = mse(activations(fake), target activations), :482) is
`activation_mse` / `losses.f0_crepe_loss`, and `Crepe.activations_with_grad` is the differentiable forward: the network is fixed, so
only d / d signal exists, and the backward keeps nothing of the forward but one byte per pooled output (which of the two positions
won, and whether its ReLU was on: tdvc_crepe_conv_train) and the activations. Backward: tdvc_crepe_head_bwd (the loss gradient and
the sigmoid fused), six tdvc_crepe_conv_bwd (unpool, mask, BatchNorm scale and the conv's input gradient in one launch each, from a
transposed tap-flipped weight packing cached next to the folded BatchNorms), tdvc_crepe_frames_bwd. `roll_bins` and
`conversion_target` build the target of train.py:245-252. Per-row `lengths` are refused on the differentiable path. The reference's
dither is absent (above), so the target activations are the deterministic ones. Out of scope: `bench.py` and `smoke()`.

Everything runs in csrc/pitch_crepe.hip (tdvc_crepe_frames, tdvc_crepe_conv, tdvc_crepe_head, tdvc_crepe_decode), csrc/pitch_crepe_bwd.hip
and, for the Viterbi decoder, csrc/pitch_viterbi.hip: no CPU or ATen fallback, no host synchronisation, no atomics, fixed summation orders (bit-identical
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


def crepe_conv(x, weight, bias, scale, shift, stride=1, out=None, train=False):
    """One conv block (tdvc_crepe_conv): x [N, Cin, Lin] dense fp32, weight [Cout, Cin, K(, 1)] -> maxpool2(relu(conv(x) + bias) scale +
    shift) fp32 [N, Cout, Lc / 2]; (Cin 1, K 512, stride 4, Lin 1024: Lc = 256) or (K 64, stride 1, Lin in 128, 64, 32, 16, 8: Lc =
    Lin); Cout and (K 64) Cin multiples of 16. train=True (tdvc_crepe_conv_train): -> (the same bits, code uint8 [N, Cout, Lc / 2]: 0 the
    winner of the pooled pair has its ReLU off, 1 the even position won and is on, 2 the odd one)."""
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
    if train:
        code = torch.empty(N, Cout, lout, dtype=torch.uint8, device=x.device)
        H.check(who, L.lib().tdvc_crepe_conv_train(C.byref(a), code.data_ptr(), H.stream(x)))
        return out, code
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


# ------------------------------------------------------------------------------------------------------------------- backward
L1_U = 136     # csrc/pitch_crepe.h CR_L1_U: the layer-1 backward reduces over 136 tap offsets per output channel, 132 of them live


def pack_bwd_weight(weight):
    """The weight of a conv block as tdvc_crepe_conv_bwd reads it (include/tdvc.h), fp32 contiguous on the weight's device: K 64:
    wt[ci][co][k'] = w[co][ci][63 - k']; K 512 (Cin 1): wt[r][co][i] = w[co][r + 510 - 4 i] where that tap exists, else 0, r < 16, i < 136."""
    w = weight.detach().float()
    if w.dim() == 4 and w.shape[3] == 1:
        w = w[..., 0]
    if w.dim() != 3 or not ((w.shape[2] == 64) or (w.shape[2] == 512 and w.shape[1] == 1)):
        raise ValueError(f'pack_bwd_weight: weight must be [Cout, Cin, 64(, 1)] or [Cout, 1, 512(, 1)], got {tuple(weight.shape)}')
    if w.shape[2] == 64:
        return w.flip(2).permute(1, 0, 2).contiguous()
    tap = torch.arange(16, device=w.device)[:, None] + 510 - 4 * torch.arange(L1_U, device=w.device)[None, :]
    live = (tap >= 0) & (tap < 512)
    packed = w[:, 0, :][:, tap.clamp(0, 511)] * live                           # [Cout, 16, 136]
    return packed.permute(1, 0, 2).contiguous()


def crepe_conv_bwd(dy, code, scale, wt, Cin, Lin, K=64, stride=1, out=None):
    """The backward of one conv block with respect to its input (tdvc_crepe_conv_bwd, one launch): dy fp32 and code uint8 [N, Cout, Lc / 2],
    scale [Cout], wt = pack_bwd_weight(weight) -> dx fp32 [N, Cin, Lin]."""
    who = 'crepe_conv_bwd'
    H.need_device(who, dy, code, wt)
    if dy.dim() != 3 or code.shape != dy.shape or code.dtype != torch.uint8:
        raise ValueError(f'{who}: dy must be [N, Cout, Lc / 2] and code uint8 of that shape')
    dy, code = dy.detach().float().contiguous(), code.contiguous()
    N, Cout, lout = dy.shape
    Cin, Lin, K, stride = int(Cin), int(Lin), int(K), int(stride)
    if lout != (Lin // stride if stride else 0) // 2:
        raise ValueError(f'{who}: {Lin} input positions at stride {stride} pool to {(Lin // stride if stride else 0) // 2} outputs, dy has {lout}')
    scale = H.vec(who, scale, Cout, 'scale')
    wt = H.vec(who, wt, (16 * Cout * L1_U) if K == 512 else Cin * Cout * K, 'the packed weight')
    if out is None:
        out = torch.empty(N, Cin, Lin, dtype=torch.float32, device=dy.device)
    H.need_device(who, out)
    if tuple(out.shape) != (N, Cin, Lin) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f'{who}: out must be contiguous fp32 [{N}, {Cin}, {Lin}]')
    a = L.CrepeConvBwdArgs()
    a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = N, Cin, Cout, Lin, K, stride
    a.dy, a.code, a.scale, a.wt, a.dx = dy.data_ptr(), code.data_ptr(), scale.data_ptr(), wt.data_ptr(), out.data_ptr()
    H.check(who, L.lib().tdvc_crepe_conv_bwd(C.byref(a), H.stream(dy)))
    return out


def _act3(who, act, weight, Cc, P):
    H.need_device(who, act, weight)
    if act.dim() == 2:
        act = act[:, :, None]
    if act.dim() != 3 or weight.dim() != 2 or weight.shape != (act.shape[1], P * Cc):
        raise ValueError(f'{who}: act must be [B, O, F] (or [N, O]) and weight [O, {P * Cc}]')
    return act.detach().float().contiguous()


def _target_strides(who, act, target):
    H.need_device(who, target)
    if target.dim() == 2:
        target = target[:, :, None]
    if tuple(target.shape) != tuple(act.shape):
        raise ValueError(f'{who}: the target must have the shape of the activations {tuple(act.shape)}, got {tuple(target.shape)}')
    target = target.detach()
    if target.dtype != torch.float32:
        target = target.float()
    return target, target.stride()


def crepe_head_bwd(act, weight, Cc, P=4, target=None, gL=None, dact=None):
    """The backward of the head (tdvc_crepe_head_bwd, one launch): act [B, O, F] from the forward, weight [O, P C] -> dx fp32 [B F, C, P].
    Either the loss form, target [B, O, F] (any strides) and gL (a 1-element DEVICE tensor, the upstream gradient of mean((act -
    target)^2); never read on the host), or the plain form dact [B, O, F]."""
    who = 'crepe_head_bwd'
    act = _act3(who, act, weight, Cc, P)
    B, O, F = act.shape
    w = H.vec(who, weight, O * P * Cc, 'weight')
    if (dact is None) == (target is None) or (target is None) != (gL is None):
        raise ValueError(f'{who}: takes either target and gL or dact')
    ts = (0, 0, 0)
    if dact is not None:
        H.need_device(who, dact)
        if dact.numel() != act.numel():
            raise ValueError(f'{who}: dact must have the shape of the activations')
        dact = dact.detach().float().contiguous()
    else:
        target, ts = _target_strides(who, act, target)
        gL = H.vec(who, gL, 1, 'gL')
    dx = torch.empty(B * F, Cc, P, dtype=torch.float32, device=act.device)
    H.check(who, L.lib().tdvc_crepe_head_bwd(act.data_ptr(), H.ptr(target), ts[0], ts[1], ts[2], H.ptr(gL), H.ptr(dact), w.data_ptr(), B * F, Cc, P,
                                             O, F, dx.data_ptr(), H.stream(act)))
    return dx


def crepe_act_mse(act, target):
    """mean((act - target)^2) over act [B, O, F] as a 1-element fp32 tensor (tdvc_crepe_act_mse: float64 partial sums in a fixed order,
    no atomics: the same bits eagerly and from a graph replay). target: any strides."""
    who = 'crepe_act_mse'
    H.need_device(who, act)
    if act.dim() not in (2, 3):
        raise ValueError(f'{who}: act must be [B, O, F] or [N, O]')
    act = (act if act.dim() == 3 else act[:, :, None]).detach().float().contiguous()
    target, ts = _target_strides(who, act, target)
    B, O, F = act.shape
    lib = L.lib()
    nbytes = lib.tdvc_crepe_act_mse_workspace()
    ws = H.scratch(nbytes, act.device)
    out = torch.empty(1, dtype=torch.float32, device=act.device)
    H.check(who, lib.tdvc_crepe_act_mse(act.data_ptr(), target.data_ptr(), ts[0], ts[1], ts[2], B, O, F, out.data_ptr(), ws.data_ptr(), nbytes,
                                        H.stream(act)))
    return out


def crepe_frames_bwd(signal, g, hop=HOP):
    """The backward of crepe_frames (tdvc_crepe_frames_bwd, two launches): signal [B, T] | [B, 1, T] | [T] as the forward took it (rows of
    full length), g [B, F, 1024] the gradient of the normalised frames -> d signal, fp32 in the signal's shape."""
    who = 'crepe_frames_bwd'
    H.need_device(who, signal, g)
    x2, bs, lead = H.rows2(who, signal)
    B, T = x2.shape
    hop = int(hop)
    if hop < 1 or T < 1:
        raise ValueError(f'{who}: hop must be at least 1 and rows need a sample')
    F = num_frames(T, hop)
    if g.numel() != B * F * WINDOW:
        raise ValueError(f'{who}: g must be [{B}, {F}, {WINDOW}], got {tuple(g.shape)}')
    g = g.detach().float().contiguous()
    lib = L.lib()
    nbytes = lib.tdvc_crepe_frames_bwd_workspace(B, F)
    ws = H.scratch(nbytes, x2.device)
    dx = torch.empty(B, T, dtype=torch.float32, device=x2.device)
    H.check(who, lib.tdvc_crepe_frames_bwd(x2.data_ptr(), bs, T, B, hop, F, g.data_ptr(), dx.data_ptr(), T, ws.data_ptr(), nbytes, H.stream(x2)))
    return dx.reshape(lead + (T,))


def roll_bins(act, shift):
    """util.roll_batches(act, shift, 1) of the reference (util/__init__.py:91-102) on act [B, C, F] (device fp32, any strides): row b is
    rolled along the bin axis by shift[b] (integers, any shape of B elements, either sign): out[b, k] = act[b, (k - shift[b]) mod C]
    (tdvc_roll_bins, one launch)."""
    who = 'roll_bins'
    H.need_device(who, act)
    if act.dim() != 3:
        raise ValueError(f'{who}: act must be [B, C, F], got {tuple(act.shape)}')
    act = act.detach().float()
    B, Cb, F = act.shape
    if F > 1 and act.stride(2) != 1:
        act = act.contiguous()
    shift = torch.as_tensor(shift, device=act.device)
    if shift.is_floating_point() or shift.numel() != B:
        raise ValueError(f'{who}: shift must hold {B} integers')
    shift = shift.reshape(-1).to(torch.int64).contiguous()
    out = torch.empty(B, Cb, F, dtype=torch.float32, device=act.device)
    H.check(who, L.lib().tdvc_roll_bins(act.data_ptr(), act.stride(0), act.stride(1), shift.data_ptr(), out.data_ptr(), B, Cb, F, H.stream(act)))
    return out


def conversion_target(f0_src, act_src, perm):
    """train.py:245-252: the F0 track and the target activations of a conversion towards the speakers f0_src[perm]. f0_src [B, 1, F] or
    [B, F] in Hz (0 = unvoiced), act_src [B, 360, F], perm [B] -> (f0_conv_tgt, act_tgt): the log-F0 mean shift of `infer.shift_f0`
    (mu = sum(voiced log(f0 + 1e-6)) / (voiced frames + 1e-6); a row without a voiced frame has mu = 0, i.e. a mean of 1 Hz, as in the
    reference) and the source activations rolled along the bins by get_shift(exp(mu_src), exp(mu_tgt))."""
    from .infer import shift_f0
    f0_tgt = f0_src[perm]

    def mu(f):
        v = f > 0
        return torch.sum(v * torch.log(f + 1e-6), -1, keepdim=True) / (torch.sum(v, -1, keepdim=True) + 1e-6)
    shift = get_shift(torch.exp(mu(f0_src)), torch.exp(mu(f0_tgt)))
    return shift_f0(f0_src, f0_tgt), roll_bins(act_src, shift)


class _ActivationsFn(torch.autograd.Function):
    """Crepe.activations_with_grad. Saved for the backward: the signal, the activations and one byte per pooled output."""

    @staticmethod
    def forward(ctx, x2, model, hop, target):
        act, codes = model._forward_train(x2, hop)
        ctx.model, ctx.hop, ctx.with_loss = model, hop, target is not None
        if target is None:
            ctx.save_for_backward(x2, act, *codes)
            return act
        ctx.save_for_backward(x2, act, target, *codes)
        ctx.mark_non_differentiable(act)
        return crepe_act_mse(act, target), act

    @staticmethod
    def backward(ctx, g, *unused):
        m = ctx.model
        x2, act = ctx.saved_tensors[:2]
        c6 = CAPACITIES[m.capacity][-1]
        if ctx.with_loss:      # the loss gradient, the sigmoid and the classifier in one launch; g stays on the device
            target, codes = ctx.saved_tensors[2], ctx.saved_tensors[3:]
            dx = crepe_head_bwd(act, m.classifier.weight, c6, 4, target=target, gL=g)
        else:
            codes = ctx.saved_tensors[2:]
            dx = crepe_head_bwd(act, m.classifier.weight, c6, 4, dact=g)
        gfr = m._backward_blocks(dx, codes)
        return crepe_frames_bwd(x2, gfr, ctx.hop), None, None, None


def _grad_rows(who, signal, model, hop, lengths, sample_rate):
    _check_rate(who, sample_rate)
    if lengths is not None:
        raise ValueError(f'{who}: per-row lengths are not part of the differentiable path (rows are full length)')
    H.need_device(who, signal, model.classifier.weight)
    hop = int(hop)
    if hop < 1:
        raise ValueError(f'{who}: hop must be at least 1, got {hop}')
    x2, _, _ = H.rows2(who, signal, keep_grad=True)
    if x2.shape[1] < 1:
        raise ValueError(f'{who}: rows with no sample are refused')
    return x2, hop


def activation_mse(signal, target_activ, model, hop=HOP, sample_rate=SR):
    """The reference's F0 term (train.py:439-470): mean((model.activations(signal) - target_activ)^2) as a 1-element tensor that is
    differentiable in signal [B, 1, T] | [B, T] | [T]; target_activ [B, 360, F] (a view is fine) gets no gradient. -> (loss,
    activations). The value comes from tdvc_crepe_act_mse; the backward is tdvc_crepe_head_bwd with the loss gradient fused, six
    tdvc_crepe_conv_bwd and tdvc_crepe_frames_bwd."""
    who = 'activation_mse'
    x2, hop = _grad_rows(who, signal, model, hop, None, sample_rate)
    H.need_device(who, target_activ)
    want = (x2.shape[0], BINS, num_frames(x2.shape[1], hop))
    if tuple(target_activ.shape) != want:
        raise ValueError(f'{who}: target_activ must be {list(want)} for this signal, got {list(target_activ.shape)}')
    return _ActivationsFn.apply(x2, model, hop, target_activ.detach().float())


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
        self._packed = {}
        self.eval()

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._folded, self._packed = {}, {}
        return out

    def _apply(self, fn, *args, **kwargs):
        self._folded, self._packed = {}, {}
        return super()._apply(fn, *args, **kwargs)

    def _pack(self, device):
        """The six weights as the backward reads them (pack_bwd_weight), once per device like the folded BatchNorms."""
        k = H.dev_key(device)
        if k not in self._packed:
            self._packed[k] = [pack_bwd_weight(getattr(self, f'conv{i}').weight) for i in range(1, 7)]
        return self._packed[k]

    def _forward_train(self, x2, hop):
        """x2 [B, T] -> (activations [B, 360, F], the six code tensors): `activations` with tdvc_crepe_conv_train."""
        frames = crepe_frames(x2, hop)
        B, F, _ = frames.shape
        fold = self._fold(frames.device)
        x, codes = frames.view(B * F, 1, WINDOW), []
        for i in range(1, 7):
            conv = getattr(self, f'conv{i}')
            x, code = crepe_conv(x, conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0], train=True)
            codes.append(code)
        return crepe_head(x, self.classifier.weight, self.classifier.bias, frames_per_row=F).view(B, BINS, F), codes

    def _backward_blocks(self, dx, codes):
        """dx [N, C6, 4] (the gradient of the last block's output) -> the gradient of the normalised frames [N, 1, 1024]: six
        tdvc_crepe_conv_bwd launches."""
        fold, packed = self._fold(dx.device), self._pack(dx.device)
        for i in range(6, 0, -1):
            conv = getattr(self, f'conv{i}')
            dx = crepe_conv_bwd(dx, codes[i - 1], fold[i - 1][0], packed[i - 1], conv.in_channels, WINDOW if i == 1 else 256 >> (i - 1),
                                conv.kernel_size[0], conv.stride[0])
        return dx

    def activations_with_grad(self, signal, hop=HOP, lengths=None, sample_rate=SR):
        """`activations` (the same bits) as a tensor that is differentiable in signal; the weights are fixed and get no gradient.
        Only the codes of tdvc_crepe_conv_train and the activations are kept for the backward. lengths: refused."""
        x2, hop = _grad_rows('Crepe.activations_with_grad', signal, self, hop, lengths, sample_rate)
        return _ActivationsFn.apply(x2, self, hop, None)

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
