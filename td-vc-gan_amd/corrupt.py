"""Signal corruption on the device: the `signal_corrupted` member of a training batch, which the reference makes in DataLoader
workers with scipy (data/dataset.py:68-86 corrupt_audio -> util/contentvec/audio_corruption.py random_eq -> util.eq_rms_signals).

corrupt_audio first calls the Praat formant / pitch perturbation and then overwrites its result: line 84 filters `signal`, not the
Praat output. What it returns is therefore a random ten-band parametric EQ of the clean signal, RMS-matched to it, and that is
what this module computes: `peq_sos` (tdvc_peq_sos, the reference's params2sos in float64 on the device), `sos_filter`
(tdvc_sos_filter, per-row float64 biquad cascades parallel over time, csrc/audio_eq.hip) and `random_eq` / `corrupt_audio` on top.
`device_batch` builds the whole batch dict TrainStep reads from a device waveform batch and labels. Nothing here is differentiable.
"""
import math

import numpy as np
import torch

from . import _host as H
from . import _lib as L
from .infer import shift_f0
from .pitch import track_f0
from .util import f0_to_excitation

Q_MIN, Q_MAX = 2.0, 5.0
GAIN_DB = 12.0
N_BANDS = 10
FC = tuple(math.exp(math.log(60.0) + (math.log(7600.0) - math.log(60.0)) * k / (N_BANDS - 1)) for k in range(N_BANDS))
F0_HOP = 64

def peq_sos(gains_db, q, sample_rate=16000, fc=None):
    """Second-order sections of a parametric EQ: gains_db, q [B, n] (dB, Q factor) -> float64 [B, n, 6] on the device, rows
    b0 b1 b2 1 a1 a2. Band 0 is a low shelf, band n-1 a high shelf, the others peaking filters (the reference's params2sos).
    fc: n centre frequencies in Hz, default the reference's ten log-spaced centres."""
    H.need_device('peq_sos', gains_db)
    dev = gains_db.device
    g = gains_db.detach().to(torch.float32).contiguous()
    qq = q.detach().to(device=dev, dtype=torch.float32).contiguous()
    if g.dim() != 2 or qq.shape != g.shape:
        raise ValueError('peq_sos: gains_db and q must both be [B, n_bands]')
    B, n = g.shape
    fc_t = H.device_table(dev, 'peq centres', lambda: np.array(FC)) if fc is None else torch.as_tensor(fc, dtype=torch.float64).to(dev).contiguous()
    if fc_t.shape != (n,):
        raise ValueError(f'peq_sos: {n} bands need {n} centre frequencies, got {tuple(fc_t.shape)}')
    if n < 2:
        raise ValueError('peq_sos: needs at least two bands (a low and a high shelf)')
    sos = torch.empty(B, n, 6, dtype=torch.float64, device=dev)
    L.check(L.lib().tdvc_peq_sos(g.data_ptr(), qq.data_ptr(), fc_t.data_ptr(), n, float(sample_rate), B, sos.data_ptr(), H.stream(sos)))
    return sos


def sos_filter(signal, sos, match_rms=False):
    """signal [T], [B, T] or [B, 1, T] (fp32, device) through the biquad cascades sos [B, S, 6] (float64, scipy's layout, a0 = 1;
    one cascade per row, zero initial state) -> the same shape: scipy.signal.sosfilt per row, computed in float64 and rounded once.
    match_rms=True scales each row to the RMS of its input row (util.eq_rms_signals) before that rounding. Rows may be strided;
    only a signal whose last axis is not dense is copied."""
    H.need_device('sos_filter', signal, sos)
    x2, x_bs, lead = H.rows2('sos_filter', signal)
    B, T = x2.shape
    sos = sos.detach().to(torch.float64).contiguous()
    if sos.dim() == 2:
        sos = sos.unsqueeze(0)
    if sos.dim() != 3 or sos.shape[0] != B or sos.shape[2] != 6:
        raise ValueError(f'sos_filter: sos must be [B = {B}, n_sections, 6], got {tuple(sos.shape)}')
    S = sos.shape[1]
    lib = L.lib()
    y = torch.empty(B, T, dtype=torch.float32, device=x2.device)      # the kernel writes every element
    nbytes = lib.tdvc_sos_filter_workspace(B, T, S)
    ws = H.scratch(nbytes, x2.device)
    H.check('sos_filter', lib.tdvc_sos_filter(x2.data_ptr(), x_bs, sos.data_ptr(), B, T, S, int(bool(match_rms)), y.data_ptr(), T,
                                              ws.data_ptr(), nbytes, H.stream(x2)))
    return y.reshape(lead + (T,))


def random_eq(signal, sample_rate=16000, gains_db=None, z=None, generator=None, match_rms=True):
    """Random parametric EQ of signal [T], [B, T] or [B, 1, T] (reference: audio_corruption.random_eq, per row): ten bands at the
    log-spaced centres, gains G ~ U(-12, 12) dB, Q = 2 * 2.5^z with z ~ U(0, 1). The draws are optional inputs, gains_db and z
    [B, 10]; by default they are drawn on the device with `generator`. No host synchronisation anywhere in the call."""
    H.need_device('random_eq', signal)
    dev = signal.device
    B = 1 if signal.dim() == 1 else signal.shape[0]
    if gains_db is None:
        gains_db = (torch.rand(B, N_BANDS, device=dev, generator=generator) * 2.0 - 1.0) * GAIN_DB
    if z is None:
        z = torch.rand(B, N_BANDS, device=dev, generator=generator)
    gains_db, z = gains_db.to(dev), z.to(dev)
    if gains_db.shape != (B, N_BANDS) or z.shape != (B, N_BANDS):
        raise ValueError(f'random_eq: gains_db and z must be [{B}, {N_BANDS}]')
    q = Q_MIN * torch.pow(Q_MAX / Q_MIN, z.double())      # float64 until tdvc_peq_sos takes it: one rounding to fp32
    return sos_filter(signal, peq_sos(gains_db, q, sample_rate), match_rms=match_rms)


def corrupt_audio(signal, sample_rate=16000, gains_db=None, z=None, generator=None):
    """What data/dataset.py:68 corrupt_audio returns: random_eq of the clean signal, RMS-matched to it. (The Praat step before it
    in the reference is overwritten by line 84 and contributes nothing.)"""
    return random_eq(signal, sample_rate, gains_db=gains_db, z=z, generator=generator, match_rms=True)


def pair_targets(label_src, num_spk, conversion=True, perm=None, generator=None):
    """In-batch target pairing of train.py:215-226 on the device: perm (a random permutation of the batch when converting, the
    identity with no_conv), label_tgt = label_src[perm] and the two one-hot codes. -> (perm, label_tgt, c_src, c_tgt)"""
    B, dev = label_src.shape[0], label_src.device
    if perm is None:
        perm = torch.randperm(B, device=dev, generator=generator) if conversion else torch.arange(B, device=dev)
    perm = perm.to(device=dev, dtype=torch.int64)
    label_tgt = label_src[perm]
    onehot = lambda l: torch.nn.functional.one_hot(l, num_spk).to(torch.float32)
    return perm, label_tgt, onehot(label_src), onehot(label_tgt)


@torch.no_grad()
def device_batch(signal_real, label_src, num_spk, conversion=True, generator=None, sample_rate=16000, gains_db=None, z=None,
                 perm=None, noise_src=None, noise_conv=None, start_phase_src=None, start_phase_conv=None, f0_tracker=None):
    """The batch dict of train.py:214-256 from a device waveform batch signal_real [B, 1, T] and labels label_src [B] (int64):
    signal_corrupted = corrupt_audio(signal_real); the in-batch target pairing; F0 tracks from track_f0 (YIN), shifted towards the
    target speaker with infer.shift_f0 when converting; the two excitations from util.f0_to_excitation. Returns the keys TrainStep
    reads: signal_real, signal_corrupted, label_src, label_tgt, c_src, c_tgt, c_f0_src, c_f0_conv, f0_conv, perm.
    Every random draw is an optional input (gains_db, z [B, 10]; perm [B]; noise_* = (voiced, unvoiced) normal tensors [B, 1, T];
    start_phase_* 1-element tensors), drawn on the device with `generator` otherwise. T must be a multiple of the F0 hop (64).
    f0_tracker: a crepe.Crepe replaces YIN by the reference's own tracker (train.py:239, filtered_pitch with the argmax decoder), and
    the dict gains f0_conv_activ [B, 360, T/64 + 1]: the target activations of TrainStep's f0_loss='activation', i.e. the source
    activations rolled towards the target speaker (crepe.conversion_target, train.py:245-252), or the source activations themselves
    with conversion=False (:242-243). With f0_tracker=None nothing changes."""
    H.need_device('device_batch', signal_real)
    if signal_real.dim() != 3 or signal_real.shape[1] != 1:
        raise ValueError('device_batch: signal_real must be [B, 1, T]')
    B, _, T = signal_real.shape
    if T % F0_HOP:
        raise ValueError(f'device_batch: T = {T} is not a multiple of the F0 hop {F0_HOP}')
    dev = signal_real.device
    signal_real = signal_real.float()
    label_src = label_src.to(device=dev, dtype=torch.int64)
    perm, label_tgt, c_src, c_tgt = pair_targets(label_src, num_spk, conversion, perm, generator)
    corrupted = corrupt_audio(signal_real, sample_rate, gains_db=gains_db, z=z, generator=generator)
    extra = {}
    if f0_tracker is None:
        f0_src = track_f0(signal_real, hop=F0_HOP, sample_rate=sample_rate)
        f0_conv = shift_f0(f0_src, f0_src[perm]) if conversion else f0_src
    else:
        from .crepe import conversion_target
        if sample_rate != 16000:
            raise ValueError(f'device_batch: the CREPE tracker takes 16000 Hz audio, got {sample_rate}')
        f0_src, act_src = f0_tracker.filtered_pitch(signal_real, 'argmax')
        f0_conv, act_conv = conversion_target(f0_src, act_src, perm) if conversion else (f0_src, act_src)
        extra['f0_conv_activ'] = act_conv

    def draws(noise, phase):
        if noise is None:
            noise = (torch.randn(B, 1, T, device=dev, generator=generator), torch.randn(B, 1, T, device=dev, generator=generator))
        if phase is None:
            phase = torch.rand(1, device=dev, generator=generator) * (2 * math.pi)
        return noise, phase
    n_c, p_c = draws(noise_conv, start_phase_conv)
    n_s, p_s = draws(noise_src, start_phase_src)
    c_f0_conv = f0_to_excitation(f0_conv, F0_HOP, sampling_rate=sample_rate, noise=n_c, start_phase=p_c)
    c_f0_src = f0_to_excitation(f0_src, F0_HOP, sampling_rate=sample_rate, noise=n_s, start_phase=p_s)
    return dict(signal_real=signal_real, signal_corrupted=corrupted, label_src=label_src, label_tgt=label_tgt, c_src=c_src, c_tgt=c_tgt,
                c_f0_src=c_f0_src, c_f0_conv=c_f0_conv, f0_conv=f0_conv, perm=perm, **extra)
