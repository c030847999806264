"""Sample-rate conversion and segment loading on the device: what data/dataset.py:106-150 load_audio does to a file after reading it
(resampy.resample with its defaults, util.eq_rms, gain / sign augmentation, random crop, zero pad, additive noise), for a padded
batch of raw utterances that is already on the GPU. `load_segments` followed by corrupt.device_batch is the whole path from "raw
utterances at their native rate" to a TrainStep batch; `resample` alone serves infer.convert_audio users whose input is not at the
model's rate.

The resampler is resampy's table-interpolated windowed sinc, written from its published description (resampy is not a dependency
and parity with an installed resampy has not been checked; `filter=(table, precision)` takes resampy's own shipped table):

    table   n = num_zeros * 2^precision;  win = rolloff * sinc(rolloff * linspace(0, num_zeros, n + 1)) * kaiser(2n + 1, beta)[n:]
    setup   ratio = sr_new / sr_orig; win *= ratio if ratio < 1; delta = diff(win, append=win[-1]); scale = min(1, ratio);
            index_step = int(scale * 2^precision)  (an integer, truncated, as resampy has it)
    output t at time tr = t / ratio:  n = int(tr), frac = scale * (tr - n)
      left wing   idx = frac * 2^precision, off = int(idx), eta = idx - off;
                  sum over i < min(n + 1, (len(win) - off) // index_step) of (win[off + i*step] + eta * delta[off + i*step]) * x[n - i]
      right wing  the same with frac = scale - frac, over k < min(n_in - n - 1, ...) and x[n + 1 + k]

The truncated index_step makes the taps slightly denser than the filter's zero crossings ask for, which shows as a small gain
(1.0027 at DC for 48 kHz -> 16 kHz). resampy has it, eq_rms removes it, and it is kept.

On the device the time register is exact: sr_new / sr_orig = L / M in lowest terms, n = (t*M) div L, phase p = (t*M) mod L, and the
weights depend on p only. `resample_bank` tabulates them in numpy float64, bank[p] = the left wing reversed followed by the right
wing, zero-filled to the widest phase, so that y[t] = sum_j bank[p][j] * x[n - left + 1 + j] with x zero outside the row reproduces
both min(...) truncations. tdvc_resample (csrc/audio_resample.hip) applies it in float64 and rounds once. Against the float time
register of the description the exact phase moves the result by <= 4.5e-13 of the row maximum (the interpolated filter is
continuous where int() flips). Nothing here is differentiable.
"""
import collections
import hashlib
import sys
import types
from fractions import Fraction

import numpy as np
import torch

from . import _host as H
from . import _lib as L

FILTERS = {      # name -> (num_zeros, precision, beta, rolloff): the parameters resampy's two shipped tables were made with
    'kaiser_best': (64, 9, 14.769656459379492, 0.9475937167399596),
    'kaiser_fast': (16, 9, 8.555504641634386, 0.85),
}
BANK_MAX_BYTES = 8 << 20
MIN_SEGMENT = 10 * 8 * 2 * 2 * 16      # data/dataset.py:40 min_segment_size
SEGMENT_MULTI = 10 * 8 * 2 * 2         # data/dataset.py:41 segment_multi
TO = L.RESAMPLE_TO

Bank = collections.namedtuple('Bank', 'bank L M left')           # bank float64 [L][W]
Lengths = collections.namedtuple('Lengths', 'dev host')          # int32 device tensor [B], list of int

_len_cache = {}


def resample_filter(filter='kaiser_best'):
    """(win, precision): the half window of the interpolation filter, float64 [num_zeros * 2^precision + 1], and the log2 of its
    samples per zero crossing. `filter` is 'kaiser_best', 'kaiser_fast' or a (table, precision) pair that is passed through."""
    if not isinstance(filter, str):
        table, precision = filter
        win = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
        if win.size < 2 or int(precision) != precision or not 0 <= precision <= 20:
            raise ValueError('resample_filter: (table, precision) needs a table of at least two samples and an integer precision')
        return win, int(precision)
    if filter not in FILTERS:
        raise ValueError(f'resample_filter: unknown filter {filter!r} (known: {sorted(FILTERS)}, or a (table, precision) pair)')

    def build():
        num_zeros, precision, beta, rolloff = FILTERS[filter]
        n = num_zeros * 2 ** precision
        win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, n + 1)) * np.kaiser(2 * n + 1, beta)[n:]
        win.setflags(write=False)
        return win, precision
    return H.host_table(('resample_filter', filter), build)


def _filter_key(filter):
    if isinstance(filter, str):
        return filter
    win, precision = resample_filter(filter)
    return (hashlib.sha1(win.tobytes()).hexdigest(), precision)


def _rates(sr_orig, sr_new):
    if sr_orig <= 0 or sr_new <= 0 or int(sr_orig) != sr_orig or int(sr_new) != sr_new:
        raise ValueError(f'resample: sample rates must be positive integers, got {sr_orig} -> {sr_new}')
    return int(sr_orig), int(sr_new)


def num_out(length, sr_orig, sr_new):
    """Output samples for `length` input samples: int(length * (float(sr_new) / sr_orig)), in double, as resampy sizes its output."""
    return int(length * (float(sr_new) / sr_orig))


def resample_bank(sr_orig, sr_new, filter='kaiser_best'):
    """Bank(bank, L, M, left) for a rate pair: sr_new / sr_orig = L / M in lowest terms and bank float64 [L][W], row p the weights
    of phase p = (t*M) mod L, so that y[t] = sum_j bank[p][j] * x[(t*M) div L - left + 1 + j] with x zero outside the row.
    ValueError when the bank would exceed 8 MiB."""
    sr_orig, sr_new = _rates(sr_orig, sr_new)
    return H.host_table(('resample_bank', sr_orig, sr_new, _filter_key(filter)), lambda: _build_bank(sr_orig, sr_new, filter))


def _build_bank(sr_orig, sr_new, filter):
    win, precision = resample_filter(filter)
    fr = Fraction(sr_new, sr_orig)
    Lp, M = fr.numerator, fr.denominator
    ratio = sr_new / sr_orig
    if ratio < 1:
        win = win * ratio
    delta = np.diff(win, append=win[-1])
    scale = min(1.0, ratio)
    num_table = 2 ** precision
    step = int(scale * num_table)
    if step < 1:
        raise ValueError(f'resample: {sr_orig} -> {sr_new} is beyond the filter table (index_step = 0)')
    nwin = len(win)
    frac = scale * (np.arange(Lp, dtype=np.float64) / Lp)
    wings = []
    for f in (frac, scale - frac):
        idx = f * num_table
        off = idx.astype(np.int64)
        wings.append((off, idx - off, (nwin - off) // step))
    left, right = int(wings[0][2].max()), int(wings[1][2].max())
    W = left + right
    if Lp * W * 8 > BANK_MAX_BYTES:
        raise ValueError(f'resample: the polyphase bank of {sr_orig} -> {sr_new} ({Lp} phases x {W} taps) exceeds 8 MiB')
    bank = np.zeros((Lp, W), np.float64)
    for p in range(Lp):
        (off, eta, cnt), (off2, eta2, cnt2) = [(int(o[p]), float(e[p]), int(c[p])) for o, e, c in wings]
        i = off + step * np.arange(cnt)
        bank[p, left - cnt:left] = (win[i] + eta * delta[i])[::-1]
        k = off2 + step * np.arange(cnt2)
        bank[p, left:left + cnt2] = win[k] + eta2 * delta[k]
    bank.setflags(write=False)
    return Bank(bank, Lp, M, left)


def _device_bank(sr_orig, sr_new, filter, device):
    """The bank in the kernel's layout, float64 [W][L] with column q = t mod L holding phase (q*M) mod L, uploaded once per rate
    pair, filter and device: a repeated call copies nothing from the host."""
    def upload(bk, device):
        order = (np.arange(bk.L, dtype=np.int64) * bk.M) % bk.L
        return torch.from_numpy(np.ascontiguousarray(bk.bank[order].T)).to(device), bk
    return H.device_table(device, ('resample_bank', sr_orig, sr_new, _filter_key(filter)), lambda: _build_bank(sr_orig, sr_new, filter), upload)


def _device_lengths(values, device):
    """Host lengths as an int32 device tensor. Cached by value, so a batch geometry that comes back (every fixed-length batch, and a
    captured graph's warm-up) uploads nothing the second time."""
    key = (H.dev_key(device), tuple(values))
    t = _len_cache.get(key)
    if t is None:
        if len(_len_cache) >= 1024:
            _len_cache.clear()
        t = _len_cache[key] = torch.tensor(list(values), dtype=torch.int32).to(device)
    return t


def _host_lengths(lengths, B, T, what):
    if lengths is None:
        return [T] * B
    if torch.is_tensor(lengths):
        if lengths.is_cuda:
            raise ValueError(f'{what}: lengths is a host sequence (a device tensor would need a synchronisation to size the output)')
        lengths = lengths.tolist()
    lengths = [int(v) for v in lengths]
    if len(lengths) != B or any(v < 0 or v > T for v in lengths):
        raise ValueError(f'{what}: lengths must be {B} values in [0, {T}]')
    return lengths


def _resample_rows(x2, x_bs, n_in, sr_orig, sr_new, filter):
    """-> (y [B, max n_out] fp32, Lengths n_out, tile sums float64 [B, tiles] or None when there is nothing to compute)"""
    dev = x2.device
    B, T = x2.shape
    bank_d, bk = _device_bank(sr_orig, sr_new, filter, dev)
    n_out = [num_out(v, sr_orig, sr_new) for v in n_in]
    n_max = max(n_out, default=0)
    n_out_d = _device_lengths(n_out, dev)
    y = torch.empty(B, n_max, dtype=torch.float32, device=dev)      # the kernel writes every element
    if B == 0 or n_max == 0:
        return y, Lengths(n_out_d, n_out), None
    lib = L.lib()
    nbytes = lib.tdvc_resample_workspace(B, n_max)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    W = bank_d.shape[0]
    H.check('resample', lib.tdvc_resample(x2.data_ptr(), x_bs, _device_lengths(n_in, dev).data_ptr(), n_out_d.data_ptr(), B, T, n_max,
                                          bank_d.data_ptr(), bk.L, 1, bk.L, bk.M, W, bk.left, y.data_ptr(), n_max, ws.data_ptr(), nbytes,
                                          H.stream(y)))
    return y, Lengths(n_out_d, n_out), ws.view(B, -1)


def resample(signal, sr_orig, sr_new, lengths=None, filter='kaiser_best'):
    """signal [T], [B, T] or [B, 1, T] (fp32, device; rows may be strided) at sr_orig -> (y, n_out) at sr_new: y [.., max(n_out)]
    fp32, zero past n_out[b]; n_out = Lengths(dev int32 tensor [B], host list) with n_out[b] = int(lengths[b] * (sr_new / sr_orig)).
    lengths: host sequence of valid samples per row (default: all T); samples past a row's length are never read.
    filter: 'kaiser_best' (resampy's default), 'kaiser_fast', or a (table, precision) pair. Equal rates return the input itself with
    no launch. float64 accumulation, rounded once; bit-identical from call to call; no host synchronisation."""
    H.need_device('resample', signal)
    sr_orig, sr_new = _rates(sr_orig, sr_new)
    x2, x_bs, lead = H.rows2('resample', signal)
    n_in = _host_lengths(lengths, x2.shape[0], x2.shape[1], 'resample')
    if sr_orig == sr_new:
        return signal, Lengths(_device_lengths(n_in, signal.device), n_in)
    y, n_out, _ = _resample_rows(x2, x_bs, n_in, sr_orig, sr_new, filter)
    return y.reshape(lead + (y.shape[1],)), n_out


def segment_size(max_segment):
    """The static length of a batch of segments: max_segment raised to at least 5120 and then to a multiple of 320 (the reference's
    min_segment_size and segment_multi)."""
    return -SEGMENT_MULTI * (-max(int(max_segment), MIN_SEGMENT) // SEGMENT_MULTI)


def valid_start_mask(y, n, max_segment):
    """y [B, N] (N > max_segment), n [B] valid samples per row -> bool [B, N - max_segment]: start s is allowed (s < n - max_segment,
    the range of the reference's randint) and its window [s, s + max_segment) holds a non-zero sample, which is the set the
    reference's redraw loop samples uniformly. From a prefix count of the non-zero samples; works on any device."""
    B, N = y.shape
    K = N - max_segment
    n = n.to(device=y.device, dtype=torch.int64)[:, None]
    nz = (y != 0) & (torch.arange(N, device=y.device)[None] < n)
    c = torch.nn.functional.pad(torch.cumsum(nz, 1, dtype=torch.int32), (1, 0))
    count = c[:, max_segment:max_segment + K] - c[:, :K]
    return (count > 0) & (torch.arange(K, device=y.device)[None] < n - max_segment)


def draw_start(y, n, max_segment, generator=None):
    """One crop start per row, int32 [B], uniform over valid_start_mask; 0 for rows with n <= max_segment. A longer row with no
    non-zero sample at all (the reference would redraw for ever) draws uniformly from the whole range. No host synchronisation."""
    valid = valid_start_mask(y, n, max_segment)
    K = valid.shape[1]
    allowed = torch.arange(K, device=y.device)[None] < (n.to(device=y.device, dtype=torch.int64)[:, None] - max_segment)
    w = torch.where(valid.any(1, keepdim=True), valid, allowed).float()
    w[:, 0] += (w.sum(1) == 0).float()
    return torch.multinomial(w, 1, generator=generator)[:, 0].to(torch.int32)


@torch.no_grad()
def load_segments(signals, lengths, sr_orig, sample_rate=16000, normalization_db=-30, max_segment=16000, data_augment=True,
                  augment_noise=None, generator=None, aug_gain=None, aug_sign=None, start=None, noise=None):
    """load_audio for a batch: signals [B, Tmax] (fp32, device, padded) with host `lengths` at sr_orig -> (signal_real [B, 1, S], info),
    ready for corrupt.device_batch. S = segment_size(max_segment) is static; shorter rows are zero-padded as collate_fn pads them.
    In the reference's order: resample to sample_rate (skipped at equal rates); gain 10^(db/20) / rms over the whole resampled row
    (normalization_db None or 0: none); with data_augment a gain U(0.3, 1) and a random sign; crop [start, start + max_segment) when
    the row is longer than max_segment (strictly); zero pad; + noise * augment_noise when augment_noise is given. A row whose rms is
    0 gives zeros (the reference divides by zero there and its warnings filter turns that into a crash).
    The draws are optional inputs, aug_gain, aug_sign [B] (sign: negative = flip), start [B] int, noise [B, S] or [B, 1, S] standard
    normal; by default they are drawn on the device with `generator`, the start uniformly among the windows that hold a non-zero
    sample. info: n_out (host list), n_out_dev, start, gain (float64 [B], the rms gain), aug_gain, aug_sign, noise. One resample
    launch and one tdvc_segment launch; no host synchronisation."""
    H.need_device('load_segments', signals)
    if signals.dim() != 2:
        raise ValueError('load_segments: signals must be a padded [B, Tmax] batch')
    sr_orig, sample_rate = _rates(sr_orig, sample_rate)
    dev = signals.device
    x2, x_bs, _ = H.rows2('load_segments', signals)
    B = x2.shape[0]
    n_in = _host_lengths(lengths, B, x2.shape[1], 'load_segments')
    if sr_orig == sample_rate:
        y, y_bs, n, tile_sq = x2, x_bs, Lengths(_device_lengths(n_in, dev), n_in), None
    else:
        y, n, tile_sq = _resample_rows(x2, x_bs, n_in, sr_orig, sample_rate, 'kaiser_best')
        y_bs = y.shape[1]
    n_max = max(n.host, default=0)
    ms = int(max_segment) if max_segment else 0
    S = segment_size(ms if ms else n_max)
    if data_augment:
        if aug_gain is None:
            aug_gain = 0.3 + 0.7 * torch.rand(B, device=dev, generator=generator)
        if aug_sign is None:
            aug_sign = 1.0 - 2.0 * torch.randint(0, 2, (B,), device=dev, generator=generator).float()
        aug_gain = aug_gain.to(device=dev, dtype=torch.float32).contiguous()
        aug_sign = aug_sign.to(device=dev, dtype=torch.float32).contiguous()
        if aug_gain.shape != (B,) or aug_sign.shape != (B,):
            raise ValueError(f'load_segments: aug_gain and aug_sign must be [{B}]')
    else:
        aug_gain = aug_sign = None
    if ms and n_max > ms:
        if start is None:
            start = draw_start(y[:, :n_max], n.dev, ms, generator)
        start = start.to(device=dev, dtype=torch.int32).contiguous()
        if start.shape != (B,):
            raise ValueError(f'load_segments: start must be [{B}]')
    else:
        start = None
    if augment_noise is not None:
        if noise is None:
            noise = torch.randn(B, S, device=dev, generator=generator)
        noise = noise.to(device=dev, dtype=torch.float32).reshape(B, S).contiguous()
    else:
        noise = None
    out = torch.empty(B, 1, S, dtype=torch.float32, device=dev)      # the kernel writes every element
    gain = torch.ones(B, dtype=torch.float64, device=dev)
    L.check(L.lib().tdvc_segment(y.data_ptr() if y.numel() else out.data_ptr(), y_bs, n.dev.data_ptr(), B, n_max, H.ptr(tile_sq),
                                 tile_sq.shape[1] if tile_sq is not None else 0, H.ptr(start), H.ptr(aug_gain), H.ptr(aug_sign),
                                 H.ptr(noise), S, float(augment_noise) if augment_noise is not None else 0.0,
                                 int(bool(normalization_db)), float(normalization_db or 0.0), ms, S, out.data_ptr(), gain.data_ptr(),
                                 H.stream(out)))
    return out, dict(n_out=n.host, n_out_dev=n.dev, start=start, gain=gain, aug_gain=aug_gain, aug_sign=aug_sign, noise=noise)


class _CallableModule(types.ModuleType):
    """The package exports the function `resample` under the name of this module, and importing a submodule binds the module to that
    name on the package. So the module itself is callable: tdvc_amd.resample(signal, 48000, 16000) is the function,
    tdvc_amd.resample.resample_bank the module's attribute."""

    def __call__(self, *args, **kwargs):
        return resample(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
