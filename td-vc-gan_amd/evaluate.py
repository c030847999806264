"""Objective evaluation on the device: the reference's test_scripts/common/test_mcd.py (mfcc_dist + f0_ratio) as library calls.

    reference                                            here
    pyworld.dio / stonemask (F0, voicing)                pitch.world_f0: tdvc_dio + tdvc_stonemask (csrc/pitch_dio.hip), the definition in
                                                         include/tdvc.h; opt-in (f0_method='dio' in `mcd`); the default stays
                                                         pitch.yin_f0(pitch_min=50, pitch_max=500, frame_stride=0.005); or the caller's tracks
    pyworld.cheaptrick (spectral envelope)               cheaptrick: tdvc_cheaptrick (csrc/eval_cheaptrick.hip), the definition in include/tdvc.h;
                                                         opt-in (envelope='cheaptrick' in `mel_cepstrum` / `mcd`, which then take the mel-cepstrum
                                                         from the same launch); the default stays a plain Hann STFT power spectrum
    pysptk.sp2mc(sp, 24, 0.42)                           sp2mc: tdvc_sp2mc (csrc/eval_mcep.hip), the definition in include/tdvc.h
    fastdtw(test, ref, dist=2) -> dist / len(path)       fastdtw: tdvc_fastdtw (csrc/eval_fastdtw.hip), the same algorithm, opt-in in `mcd`
                                                         (align='fastdtw'); the default stays dtw: tdvc_dtw (csrc/eval_dtw.hip), the EXACT programme

With f0_method='dio', envelope='cheaptrick' and align='fastdtw', `mcd` runs the reference's whole pipeline as the same algorithms.
Four parities are NOT checked, because none of pyworld, pysptk and fastdtw is available to this repository: **parity of `dio` and
`stonemask` with pyworld is unchecked** (they follow WORLD's dio.cpp, stonemask.cpp and matlabfunctions.cpp with pyworld's defaults
as restated in include/tdvc.h, with two stated deviations: the low-cut and the band filters are linear convolutions where WORLD
multiplies the spectra of one zero-padded FFT, which wraps into the first few hundred samples when the padding is tight; and
StoneMask reads DIO's track after one fp32 rounding where WORLD keeps float64), **parity of
`cheaptrick` with pyworld is still unchecked** (it follows WORLD's cheaptrick.cpp as restated in include/tdvc.h, with two stated
deviations: a deterministic floor, S = max(S, floor) + 2.2e-16, where WORLD adds noise from its own generator, so frames of digital
silence differ; and an F0 above fs/4 counts as unvoiced, where WORLD has no cap and reads out of range), `sp2mc` is believed to be
pysptk's, and `dtw` is exact where fastdtw is an approximation with radius 1, so its cost is a lower bound on fastdtw's (the
tie order up, left, diagonal is believed to be fastdtw's tuple order). The alignment of the reference is now available as the
same algorithm: `fastdtw` restates the package (recursion, halving, window expansion, windowed programme; include/tdvc.h), but
**parity with the installed fastdtw package is still unchecked**, its pyramid of halved sequences is fp32 where the package
averages in float64 (a stated deviation: one fp32 rounding per level), and the radius is limited to 1..8.

Nothing here synchronises with the host: lengths and voicing stay on the device, the voiced frames are compacted by a prefix
sum and a scatter, and the per-pair lengths go into the kernel as device int32.
"""
import math

import numpy as np
import torch

from . import _host as H
from . import _lib as L
from . import ops
from .arena import ConvSlot
from .ops import ConvSpec

METRICS = {'l2': L.DTW_L2, 'l1': L.DTW_L1, 'sq': L.DTW_SQ}
DTW_MAX_LEN, DTW_MAX_D = 4096, 64      # csrc/eval_dtw.hip
FASTDTW_MAX_LEN, FASTDTW_MAX_RADIUS = 16384, 8      # csrc/eval_fastdtw.hip
POWER_FLOOR = 1e-10                    # default floor under the logarithm: -100 dB against a full-scale bin of power 1
# default floor under CheapTrick's smoothed spectrum. Its window has sum w^2 = 1, so white noise of variance v gives P = v per bin: 1e-16
# is the rounding noise of an fp32 waveform at full scale (2^-48 / 12 = 3e-16), below which nothing in an fp32 signal is information,
# and it is the size of WORLD's own safeguard (2.2e-16 |randn| added to S), so only frames WORLD would fill with its noise are floored
CHEAPTRICK_FLOOR = 1e-16
CHEAPTRICK_N_FFT = (512, 1024, 2048)   # the compiled instances of csrc/eval_cheaptrick.hip
ENVELOPES = ('stft', 'cheaptrick')
F0_METHODS = ('yin', 'dio')
ALIGNMENTS = ('exact', 'fastdtw')

_stft_cache = {}


def _signal3(who, signal):
    H.need_device(who, signal)
    if signal.dim() != 3 or signal.shape[1] != 1:
        raise ValueError(f'{who}: signal must be [B, 1, T]')


# ------------------------------------------------------------------------------------------------------------ mel-cepstrum
def _freqt(c, order, alpha):
    """SPTK's frequency transform of c [..., m1 + 1] -> [..., order + 1] (float64; the recursion of include/tdvc.h)."""
    b = 1.0 - alpha * alpha
    g = np.zeros(c.shape[:-1] + (order + 1,), np.float64)
    for i in range(c.shape[-1] - 1, -1, -1):
        d = g.copy()
        g[..., 0] = c[..., i] + alpha * d[..., 0]
        if order >= 1:
            g[..., 1] = b * d[..., 0] + alpha * d[..., 1]
        for j in range(2, order + 1):
            g[..., j] = d[..., j - 1] + alpha * (d[..., j] - g[..., j - 1])
    return g


def _mc_table(who, n_fft, order, alpha):
    """(key, build) of `who`'s matrix for _host.host_table / device_table: freqt of the unit vectors, for sp2mc_matrix after irfft and c[0] / 2."""
    n_fft, order, alpha = int(n_fft), int(order), float(alpha)
    if n_fft < 2 or n_fft % 2 or not 0 <= order <= n_fft // 2 or not abs(alpha) < 1:
        raise ValueError(f'{who}: needs an even n_fft >= 2, 0 <= order <= n_fft/2 and |alpha| < 1')

    def build():
        nb = n_fft // 2 + 1
        c = np.eye(nb)
        if who == 'sp2mc_matrix':
            c = np.fft.irfft(c, n=n_fft, axis=1)[:, :nb].copy()      # row k: the cepstrum of the k-th unit vector of log P
            c[:, 0] *= 0.5
        m = np.ascontiguousarray(_freqt(c, order, alpha).T)
        m.setflags(write=False)
        return m
    return (who, n_fft, order, alpha), build


def sp2mc_matrix(n_fft, order=24, alpha=0.42):
    """float64 [order + 1, n_fft/2 + 1] with mc = matrix @ log(P): the unit vectors of log P pushed through irfft, c[0] / 2 and
    the frequency-transform recursion. Host numpy, cached per argument tuple (read-only)."""
    return H.host_table(*_mc_table('sp2mc_matrix', n_fft, order, alpha))


def sp2mc(power, order=24, alpha=0.42, floor=POWER_FLOOR, layout='fn'):
    """Mel-cepstrum of a power spectrum (device fp32) -> fp32 [..., n_frames, order + 1]; tdvc_sp2mc, one launch.
    layout='fn': power is [n_frames, n_bins] or [B, n_frames, n_bins], the layout of a WORLD envelope (pysptk.sp2mc's argument);
    layout='nf': [B, n_bins, n_frames], the layout of this package's conv STFT. Any strides: nothing is copied. n_bins = n_fft/2 + 1."""
    H.need_device('sp2mc', power)
    if layout not in ('fn', 'nf') or power.dim() not in (2, 3):
        raise ValueError("sp2mc: power must be [F, N] / [B, F, N] with layout='fn' or [B, N, F] with layout='nf'")
    p = power.detach().float()
    p3 = p[None] if p.dim() == 2 else p
    if layout == 'nf':
        p3 = p3.transpose(1, 2)
    B, F, nb = p3.shape
    mat = H.device_table(p.device, *_mc_table('sp2mc_matrix', 2 * (nb - 1), order, alpha))
    mc = torch.empty(B, F, order + 1, dtype=torch.float32, device=p.device)
    L.check(L.lib().tdvc_sp2mc(p3.data_ptr(), p3.stride(0), p3.stride(1), p3.stride(2), mat.data_ptr(), B, F, nb, order, float(floor),
                               mc.data_ptr(), H.stream(p)))
    return mc[0] if power.dim() == 2 else mc


class _Stft:
    """Periodic-Hann windowed DFT as Conv1d(1 -> 2 Fp, K = n_fft, stride = hop) on the HIP conv kernels (losses.MelSpec's front end
    with a free hop); Fp = n_fft/2 + 1 padded to a multiple of 4, real parts in channels [0, F), imaginary in [Fp, Fp + F)."""

    def __init__(self, n_fft, hop, device):
        F = n_fft // 2 + 1
        self.F, self.Fp, self.n_fft, self.hop = F, (F + 3) // 4 * 4, n_fft, hop
        n = np.arange(n_fft)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
        ang = 2 * np.pi * np.outer(np.arange(F), n) / n_fft
        basis = np.zeros((2 * self.Fp, 1, n_fft), np.float64)
        basis[:F, 0] = np.cos(ang) * win
        basis[self.Fp:self.Fp + F, 0] = -np.sin(ang) * win
        self.basis = torch.from_numpy(basis.astype(np.float32)).to(device)
        self.spec = ConvSpec(1, 2 * self.Fp, n_fft, stride=hop)
        self.spec.slot = ConvSlot(self.basis.data_ptr(), 0, 0, 0, trainable=False)

    def power(self, x):
        """x [B, 1, T] -> |STFT|^2 [B, Fp, 1 + T // hop] (centred frames, reflect padding)."""
        x = x.contiguous()
        B, _, T = x.shape
        pad = self.n_fft // 2
        lib = L.lib()
        xp = torch.empty((B, 1, T + 2 * pad), dtype=torch.float32, device=x.device)
        L.check(lib.tdvc_reflect_pad_fwd(x.data_ptr(), xp.data_ptr(), B, T, pad, H.stream(x)))
        spec = ops.conv_fwd_raw(self.spec, xp, ops._xf())
        pw = torch.empty((B, self.Fp, spec.shape[2]), dtype=torch.float32, device=x.device)
        L.check(lib.tdvc_power_fwd(spec.data_ptr(), pw.data_ptr(), B, self.Fp, spec.shape[2], H.stream(x)))
        return pw


def cheaptrick_mc_matrix(n_fft, order=24, alpha=0.42):
    """float64 [order + 1, n_fft/2 + 1], G = freqt of the unit vectors: the mel-cepstrum of a CheapTrick frame is G @ c' with c' the
    liftered cepstrum, c[0] halved (include/tdvc.h). Host numpy, cached per argument tuple (read-only)."""
    return H.host_table(*_mc_table('cheaptrick_mc_matrix', n_fft, order, alpha))


def _cheaptrick(who, signal, f0, sample_rate, n_fft, hop, q1, lengths, floor, want_env, mc_args):
    """One tdvc_cheaptrick launch -> (env or None, mc or None); mc_args = (order, alpha) or None. The caller has checked signal."""
    H.need_device(who, f0)
    B, _, T = signal.shape
    if f0.dim() != 2 or f0.shape[0] != B:
        raise ValueError(f'{who}: an F0 track must be [B, n_frames]')
    if n_fft not in CHEAPTRICK_N_FFT:
        raise ValueError(f'{who}: the CheapTrick envelope needs n_fft in {CHEAPTRICK_N_FFT}')
    hop = int(round(sample_rate / 200)) if hop is None else int(hop)
    x, f = signal.detach().float(), f0.detach().float()
    F, nb, dev = f.shape[1], n_fft // 2 + 1, x.device
    ln = H.device_lengths(who, lengths, B, dev, move=True)
    env = torch.empty(B, F, nb, dtype=torch.float32, device=dev) if want_env else None
    mc = mat = None
    order = 0
    if mc_args is not None:
        order, alpha = mc_args
        mat = H.device_table(dev, *_mc_table('cheaptrick_mc_matrix', n_fft, order, alpha))
        mc = torch.empty(B, F, order + 1, dtype=torch.float32, device=dev)
    L.check(L.lib().tdvc_cheaptrick(x.data_ptr(), x.stride(0), x.stride(2), H.ptr(ln), T, f.data_ptr(), f.stride(0), f.stride(1), B, F, hop,
                                    int(sample_rate), int(n_fft), float(q1), float(floor), H.ptr(mat), int(order), H.ptr(env), H.ptr(mc), H.stream(x)))
    return env, mc


def cheaptrick(signal, f0, sample_rate=16000, n_fft=1024, hop=None, q1=-0.15, lengths=None, floor=CHEAPTRICK_FLOOR):
    """WORLD's CheapTrick spectral envelope of signal [B, 1, T] (device fp32) under the F0 track f0 [B, F] (Hz; 0, NaN, anything at
    or under 3 fs/(n_fft - 3) or above fs/4 = unvoiced) -> env fp32 [B, F, n_fft/2 + 1], the counterpart of
    pyworld.cheaptrick(x, f0, t, fs, fft_size=n_fft) with t = 5 ms frames: tdvc_cheaptrick, one launch, the definition in
    include/tdvc.h. Frame f is centred on sample f * hop, hop = sample_rate / 200 by default (the frame grid of `yin_f0` with
    frame_stride=0.005). lengths: device integers [B], valid samples per row; samples at and past them are never read (the
    window repeats the last valid sample, as WORLD does at the end of its input). Any strides: nothing is copied. q1 is the
    lifter's spectral-recovery weight; floor > 0 replaces WORLD's random safeguard (CHEAPTRICK_FLOOR has the reason).
    **Parity with pyworld is unchecked.** n_fft is 512, 1024 or 2048."""
    _signal3('cheaptrick', signal)
    return _cheaptrick('cheaptrick', signal, f0, sample_rate, n_fft, hop, q1, lengths, floor, True, None)[0]


def mel_cepstrum(signal, sample_rate=16000, n_fft=1024, hop=80, order=24, alpha=0.42, lengths=None, floor=None, envelope='stft', f0=None,
                 q1=-0.15):
    """signal [B, 1, T] (device fp32) -> mel-cepstra fp32 [B, 1 + T // hop, order + 1]: periodic Hann window of n_fft samples, frame f
    centred on sample f * hop (reflect padding of n_fft/2, as torch.stft(center=True)), power spectrum through the conv STFT and
    tdvc_power_fwd, then `sp2mc`. hop is in samples (80 = the reference's 5 ms at 16 kHz); sample_rate is recorded in the
    signature for symmetry with `mcd` and does not enter the arithmetic. floor defaults to POWER_FLOOR.
    With lengths (device integers [B], valid samples per row) the result is (mc, n_frames) with n_frames = 1 + lengths // hop as
    device int32; frames whose window reaches past lengths[b] see whatever the row holds there (zero padding, usually).
    envelope='cheaptrick': the mel-cepstra of WORLD's CheapTrick envelope instead (`cheaptrick`, whose launch also yields them:
    no envelope is stored), fp32 [B, F, order + 1] on the frames of the F0 track f0 [B, F]; f0=None runs
    yin_f0(pitch_min=50, pitch_max=500, frame_stride=hop / sample_rate), as `mcd` does. sample_rate enters the arithmetic, floor
    defaults to CHEAPTRICK_FLOOR, n_fft is 512, 1024 or 2048, and samples at and past lengths[b] are never read."""
    _signal3('mel_cepstrum', signal)
    if envelope not in ENVELOPES:
        raise ValueError(f'mel_cepstrum: unknown envelope {envelope!r} (known: {ENVELOPES})')
    if envelope == 'cheaptrick':
        if f0 is None:
            from . import pitch
            f0 = pitch.yin_f0(signal.detach().float()[:, 0], sample_rate, pitch_min=50, pitch_max=500, frame_stride=hop / sample_rate)
        mc = _cheaptrick('mel_cepstrum', signal, f0, sample_rate, n_fft, hop, q1, lengths, CHEAPTRICK_FLOOR if floor is None else floor,
                         False, (order, alpha))[1]
    else:
        if n_fft % 2 or n_fft < 4 or hop < 1 or signal.shape[-1] <= n_fft // 2:
            raise ValueError('mel_cepstrum: needs an even n_fft, hop >= 1 and more than n_fft/2 samples (reflect padding)')
        key = (int(n_fft), int(hop), H.dev_key(signal.device))
        if key not in _stft_cache:
            _stft_cache[key] = _Stft(int(n_fft), int(hop), signal.device)
        st = _stft_cache[key]
        pw = st.power(signal.detach().float())
        mc = sp2mc(pw[:, :st.F], order, alpha, POWER_FLOOR if floor is None else floor, layout='nf')
    if lengths is None:
        return mc
    return mc, (1 + torch.div(lengths.to(signal.device), int(hop), rounding_mode='floor')).clamp(0, mc.shape[1]).to(torch.int32)


# ------------------------------------------------------------------------------------------------------------ DTW
def dtw(x, y, x_len=None, y_len=None, metric='l2', return_path=False):
    """Exact dynamic time warping of x [B, N, D] against y [B, M, D] (device fp32; [N, D] / [M, D] for one pair) ->
    (cost float64 [B], length int32 [B][, path int64 [B, N + M - 1, 2]]); tdvc_dtw, one launch, no host synchronisation.
    x_len / y_len: device integers [B], the valid frames of each pair (None = all); frames past them are never read.
    metric: 'l2' Euclidean norm (fastdtw's dist=2), 'l1', 'sq' squared Euclidean, each in fp32 from direct differences; the
    accumulated cost is float64. Ties: the first minimum in the order up (i-1, j), left (i, j-1), diagonal. length is the number
    of cells of that path, so cost / length is the reference's figure. The path starts at (0, 0) and is padded with -1.
    A pair with a length of 0 gives cost NaN, length 0 and a path of -1. N, M <= 4096 and D <= 64."""
    H.need_device('dtw', x, y)
    if metric not in METRICS:
        raise ValueError(f'dtw: unknown metric {metric!r} (known: {sorted(METRICS)})')
    if x.dim() != y.dim() or x.dim() not in (2, 3):
        raise ValueError('dtw: x and y must both be [N, D] or both [B, N, D]')
    single = x.dim() == 2
    x3, x_bs, x_fs = H.frames3('dtw', x)
    y3, y_bs, y_fs = H.frames3('dtw', y)
    B, N, D = x3.shape
    if y3.shape[0] != B or y3.shape[2] != D:
        raise ValueError(f'dtw: x {tuple(x3.shape)} and y {tuple(y3.shape)} differ in batch or feature size')
    M = y3.shape[1]
    dev = x3.device
    xl, yl = H.device_lengths('dtw', x_len, B, dev, move=True), H.device_lengths('dtw', y_len, B, dev, move=True)
    lib = L.lib()
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    P = N + M - 1
    path = torch.full((B, max(P, 0), 2), -1, dtype=torch.int32, device=dev) if return_path else None
    nbytes = lib.tdvc_dtw_workspace(B, N, M, int(return_path)) if B > 0 else 0
    ws = H.scratch(nbytes, dev)
    L.check(lib.tdvc_dtw(x3.data_ptr(), x_bs, x_fs, y3.data_ptr(), y_bs, y_fs, H.ptr(xl), H.ptr(yl), B, N, M, D, METRICS[metric],
                         cost.data_ptr(), length.data_ptr(), H.ptr(path), 2 * P, ws.data_ptr(), nbytes, H.stream(x3)))
    if single:
        cost, length, path = cost[0], length[0], (path[0] if return_path else None)
    return (cost, length, path.long()) if return_path else (cost, length)


def fastdtw(x, y, x_len=None, y_len=None, radius=1, metric='l2', return_path=False):
    """FastDTW of x [B, N, D] against y [B, M, D] (device fp32; [N, D] / [M, D] for one pair) -> (cost float64 [B], length int32 [B]
    [, path int64 [B, N + M - 1, 2]]): the reference's fastdtw(x, y, radius=1, dist=2) as the same algorithm; tdvc_fastdtw, one
    launch with the whole pyramid inside it, no host synchronisation. Layouts, strides, lengths, metrics, tie rule and return
    values are exactly `dtw`'s; the definition (recursion, halving, window) is written out in include/tdvc.h. The cost is an
    approximation from above of `dtw`'s exact optimum, in O((N + M) radius) work.
    **Parity with the installed fastdtw package is unchecked**, and the pyramid of halved sequences is fp32 (one rounding per
    level) where the package averages in float64. N, M <= 16384, D <= 64, 1 <= radius <= 8."""
    H.need_device('fastdtw', x, y)
    if metric not in METRICS:
        raise ValueError(f'fastdtw: unknown metric {metric!r} (known: {sorted(METRICS)})')
    if x.dim() != y.dim() or x.dim() not in (2, 3):
        raise ValueError('fastdtw: x and y must both be [N, D] or both [B, N, D]')
    radius = int(radius)
    if radius < 1:
        raise ValueError('fastdtw: the radius must be at least 1')
    single = x.dim() == 2
    x3, x_bs, x_fs = H.frames3('fastdtw', x)
    y3, y_bs, y_fs = H.frames3('fastdtw', y)
    B, N, D = x3.shape
    if y3.shape[0] != B or y3.shape[2] != D:
        raise ValueError(f'fastdtw: x {tuple(x3.shape)} and y {tuple(y3.shape)} differ in batch or feature size')
    M = y3.shape[1]
    dev = x3.device
    xl, yl = H.device_lengths('fastdtw', x_len, B, dev, move=True), H.device_lengths('fastdtw', y_len, B, dev, move=True)
    lib = L.lib()
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    P = N + M - 1
    path = torch.full((B, max(P, 0), 2), -1, dtype=torch.int32, device=dev) if return_path else None
    nbytes = lib.tdvc_fastdtw_workspace(B, N, M, D, radius, int(return_path)) if B > 0 else 0
    ws = H.scratch(nbytes, dev)
    L.check(lib.tdvc_fastdtw(x3.data_ptr(), x_bs, x_fs, y3.data_ptr(), y_bs, y_fs, H.ptr(xl), H.ptr(yl), B, N, M, D, METRICS[metric], radius,
                             cost.data_ptr(), length.data_ptr(), H.ptr(path), 2 * P, ws.data_ptr(), nbytes, H.stream(x3)))
    if single:
        cost, length, path = cost[0], length[0], (path[0] if return_path else None)
    return (cost, length, path.long()) if return_path else (cost, length)


# ------------------------------------------------------------------------------------------------------------ MCD
def f0_stats(f0_test, f0_ref):
    """The F0 statistics of test_mcd.py:83-84 and :116 from two tracks [..., F] in Hz (0 = unvoiced; the two may differ in F) ->
    dict of float64 tensors [...]: over the voiced frames v of each track,
        diff_f0_mean = mean(log f_test[v]) - mean(log f_ref[v])
        diff_f0_var  = log(var f_test[v]) - log(var f_ref[v])      (population variance, numpy's default)
        f0_ratio     = mean f_ref[v] / mean f_test[v]
    Plain tensor arithmetic in float64 on whichever device holds the tracks; a track without voiced frames gives NaN."""
    def moments(f):
        f = f.double()
        v = f > 0
        n = v.sum(-1).double()
        mean = torch.where(v, f, torch.zeros_like(f)).sum(-1) / n
        mlog = torch.where(v, torch.log(torch.where(v, f, torch.ones_like(f))), torch.zeros_like(f)).sum(-1) / n
        var = torch.where(v, (f - mean[..., None]) ** 2, torch.zeros_like(f)).sum(-1) / n
        return mean, mlog, var
    mt, lt, vt = moments(f0_test)
    mr, lr, vr = moments(f0_ref)
    return dict(diff_f0_mean=lt - lr, diff_f0_var=torch.log(vt) - torch.log(vr), f0_ratio=mr / mt)


def compact_voiced(mc, voiced):
    """mc [B, F, D], voiced bool [B, F] -> (the voiced frames of each row moved to its front, in order, [B, F, D]; their count
    int32 [B]). A prefix sum and a scatter: no host synchronisation. Rows past the count hold NaN."""
    B, F, D = mc.shape
    dest = torch.where(voiced, voiced.cumsum(1) - 1, torch.full_like(voiced, F, dtype=torch.int64))      # unvoiced frames go to a spare row
    out = torch.full((B, F + 1, D), float('nan'), dtype=mc.dtype, device=mc.device)
    out.scatter_(1, dest[..., None].expand(B, F, D), mc)
    out[:, F] = float('nan')
    return out[:, :F], voiced.sum(1).to(torch.int32)


def _voiced_cepstra(who, sig, length, f0, sample_rate, hop, drop_c0, envelope, mel_kwargs, f0_method='yin'):
    """Mel-cepstra of the voiced frames of sig [B, 1, T], compacted, their count, and the F0 track used."""
    B, _, T = sig.shape
    cheap = envelope == 'cheaptrick'
    if not cheap:
        mc = mel_cepstrum(sig, sample_rate=sample_rate, hop=hop, **mel_kwargs)
    if f0 is None:
        from . import pitch
        if f0_method == 'dio':
            f0 = pitch.world_f0(sig[:, 0], sample_rate, hop, 50.0, 500.0, lengths=length)
        else:
            f0 = pitch.yin_f0(sig[:, 0], sample_rate, pitch_min=50, pitch_max=500, frame_stride=hop / sample_rate)
    elif f0.dim() != 2 or f0.shape[0] != B:
        raise ValueError(f'{who}: an F0 track must be [B, n_frames]')
    if cheap:                                                                     # one F0 track for the envelope and for the voicing
        mc = mel_cepstrum(sig, sample_rate=sample_rate, hop=hop, envelope='cheaptrick', f0=f0, lengths=length, **mel_kwargs)
        mc = mc[0] if length is not None else mc
    F = min(mc.shape[1], f0.shape[1])
    mc, f0 = mc[:, :F], f0[:, :F]
    if length is None:
        valid = torch.ones(B, F, dtype=torch.bool, device=sig.device)
    else:
        ln = length.to(sig.device)
        if cheap or f0_method == 'dio':                                           # WORLD's frame grid: f * hop <= length, 1 + length // hop frames
            nfr = 1 + torch.div(ln, hop, rounding_mode='floor')
        else:                                                                     # frames centred inside the row: f * hop < length
            nfr = torch.div(ln + (hop - 1), hop, rounding_mode='floor')
        valid = torch.arange(F, device=sig.device)[None, :] < nfr[:, None]
    f0 = torch.where(valid, f0, torch.zeros_like(f0))
    if drop_c0:
        mc = mc[:, :, 1:]
    seq, count = compact_voiced(mc, f0 > 0)
    return seq, count, f0


def mcd(test, ref, test_len=None, ref_len=None, sample_rate=16000, f0_test=None, f0_ref=None, drop_c0=False, db=False, min_voiced=10,
        envelope='stft', align='exact', radius=1, f0_method='yin', **mel_kwargs):
    """Mel-cepstral distortion of test [B, 1, T1] against ref [B, 1, T2] (device waveforms; *_len: valid samples per row as device
    integers [B]) -> dict of device tensors [B]: the counterpart of test_mcd.py's mfcc_dist + f0_ratio.

    Mel-cepstra at a 5 ms hop (hop = sample_rate / 200 samples; mel_kwargs go to `mel_cepstrum`: n_fft, order, alpha, floor, q1).
    envelope='stft' (the default) takes them from a plain Hann STFT; envelope='cheaptrick' from WORLD's CheapTrick envelope, as the
    reference does: the F0 track is obtained first and serves both the envelope and the voicing, frame f of the cepstra IS frame f
    of the track, and samples at and past a length are never read.
    Voicing from yin_f0(pitch_min=50, pitch_max=500, frame_stride=0.005) or from the caller's f0_test / f0_ref [B, n_frames].
    f0_method='dio' takes it from pitch.world_f0(f0_floor=50, f0_ceil=500) instead: WORLD's DIO refined by StoneMask, as the reference
    does (samples at and past a length are never read; parity with pyworld is unchecked). With envelope='cheaptrick' and
    align='fastdtw' the call is then the reference's pipeline, step for step, as the same algorithms.
    Frame alignment: STFT frame f and YIN frame f are both centred on sample f * hop (the STFT reflects n_fft/2 samples, YIN
    zero-pads half a frame), so frame f of one is frame f of the other; the STFT has one frame more when T is a multiple of
    hop, and the common frames are kept. With a length, the frames centred inside the row, f * hop < length, count. Where a WORLD
    component supplies the frame grid (f0_method='dio' or envelope='cheaptrick') the frame set is WORLD's, f * hop <= length: the
    1 + length // hop frames of `world_f0` and of `mel_cepstrum`'s n_frames, so a length that is a multiple of hop keeps the frame
    centred on sample `length` (its window repeats the last valid sample), and a row gives the same numbers with length = T as
    without a length.
    The voiced frames of each side are compacted on the device and aligned with metric 'l2': align='exact' (the default) by `dtw`,
    the exact programme (at most 4096 frames, 20.5 s); align='fastdtw' by `fastdtw` with `radius`, the reference's alignment as the
    same algorithm (at most 16384 frames; parity with the installed fastdtw package is unchecked, and its pyramid is fp32 here).
        mcd = cost / path_len      plain Euclidean distance including c0: the reference's number
        drop_c0=True leaves c0 out; db=True multiplies by 10 / ln(10) * sqrt(2): together the conventional MCD in dB
        path_len, n_test, n_ref    cells of the path, voiced frames of each side
        diff_f0_mean, diff_f0_var, f0_ratio      `f0_stats` of the two tracks
    Every entry is float64, and every entry is NaN for a pair with fewer than min_voiced voiced frames on either side (the
    reference returns NaN under 10 on the test side). Nothing synchronises with the host."""
    H.need_device('mcd', test, ref)
    for s in (test, ref):
        if s.dim() != 3 or s.shape[1] != 1 or s.shape[0] != test.shape[0]:
            raise ValueError('mcd: waveforms must be [B, 1, T] with one batch size')
    if envelope not in ENVELOPES:
        raise ValueError(f'mcd: unknown envelope {envelope!r} (known: {ENVELOPES})')
    if align not in ALIGNMENTS:
        raise ValueError(f'mcd: unknown align {align!r} (known: {ALIGNMENTS})')
    if f0_method not in F0_METHODS:
        raise ValueError(f'mcd: unknown f0_method {f0_method!r} (known: {F0_METHODS})')
    hop = int(round(sample_rate * 0.005))
    a, na, f0a = _voiced_cepstra('mcd', test.detach().float(), test_len, f0_test, sample_rate, hop, drop_c0, envelope, mel_kwargs, f0_method)
    b, nb, f0b = _voiced_cepstra('mcd', ref.detach().float(), ref_len, f0_ref, sample_rate, hop, drop_c0, envelope, mel_kwargs, f0_method)
    max_len = FASTDTW_MAX_LEN if align == 'fastdtw' else DTW_MAX_LEN
    if a.shape[1] > max_len or b.shape[1] > max_len:
        raise ValueError(f'mcd: more than {max_len} frames ({max_len * 0.005:.1f} s); evaluate shorter segments')
    cost, length = fastdtw(a, b, na, nb, radius=radius, metric='l2') if align == 'fastdtw' else dtw(a, b, na, nb, metric='l2')
    ok = (na >= min_voiced) & (nb >= min_voiced)
    nan = torch.full_like(cost, float('nan'))
    scale = 10.0 / math.log(10.0) * math.sqrt(2.0) if db else 1.0
    out = dict(mcd=scale * cost / length.double(), path_len=length.double(), n_test=na.double(), n_ref=nb.double(), **f0_stats(f0a, f0b))
    return {k: torch.where(ok, v, nan) for k, v in out.items()}
