"""No GPU: what tests/test_dio_gpu.py relies on, proved on the host. pyworld is not available: nothing here is a parity test against
WORLD; the definition of include/tdvc.h, restated in tests/dio_ref.py, is pinned to facts that do not come from the code under test.

1. Symbols: tdvc_dio, tdvc_dio_workspace, tdvc_dio_num_bands and tdvc_stonemask are declared, exported, bound and re-exported.
2. Refusals through the raw C ABI with a null stream (nothing is launched, the pointers are never dereferenced), and the workspace
   query returns 0 on refused arguments.
3. The restatement on steady harmonic tones (7 harmonics, 1/k amplitudes, -60 dB noise, 0.5 s) at 60, 100, 220 and 480 Hz: every
   frame more than vrm frames from the ends is voiced, and `dio`, then `stonemask`, lie within TONE_BAR of the true frequency there.
   Measured worst relative error of the restatement over the four tones: dio 1.05e-04 (480 Hz), stonemask 2.74e-04 (220 Hz);
   TONE_BAR = 4 x 2.74e-04 = 1.1e-03. Zeros, a constant, F <= vrm, a 1500-sample row, tones outside [floor, ceil], a 100 -> 200 Hz step.
   StoneMask: 0, 40.0, fs/12 + 1 and NaN give 0; a track 5 % off a harmonic tone is pulled to within TONE_BAR (measured 5.6e-04); a
   track 30 % above a pure sinusoid returns the input. (On the HARMONIC tones a track 30 % off does not: its first two bins sit
   between harmonics, and the refinement lands within the 20 % clamp of the input on 42 to 101 of the 101 frames, so the rule that is
   true of every frame is asserted there instead: the output is the input or within 20 % of it.)
4. Decision stability: for every waveform of the GPU tests, the restatement on x and on x (1 + 1e-12 xi) agrees on which frames are
   voiced and which candidates are zero, and voiced values agree to 1e-10 relative. Measured: no flip, f0 within 9.5e-14, StoneMask
   within 5.8e-14; candidates within 6.4e-10 (they are not asserted to 1e-10: a candidate of a band that loses is not a voiced value).
5. world_f0's fp32 round trip: the restatement's stonemask on the fp32 DIO track nudged by +-1 ulp moves no voiced frame by more
   than 4 * 2^-24 relative on the waveforms of the end-to-end GPU test. Measured: 0 of 822 frame-nudges. (The 100 -> 200 Hz step has
   1 of 198, 5.2e-05 at the jump, and is therefore not among the end-to-end inputs.)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dio_ref as R
from common import ROOT, pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
TONE_BAR = 4 * 2.74e-4
WORLD_INPUTS = ('glide4000', 'glide8000', 'glide16040', 'lastframe', 'tile-1', 'tile+1', 'glide24')      # test_dio_gpu.py's end to end


def test_symbols_in_header_binding_library_and_package():
    P = pkg()
    L = P._lib
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = L.lib()
    for name in ('tdvc_dio', 'tdvc_dio_workspace', 'tdvc_dio_num_bands', 'tdvc_stonemask'):
        assert re.search(rf'\b{name}\(', header), name
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.tdvc_dio_workspace.restype is C.c_size_t
    assert len(L.SIGNATURES['tdvc_dio'][1]) == 20 and len(L.SIGNATURES['tdvc_stonemask'][1]) == 15
    assert os.path.exists(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'pitch_dio.hip'))
    assert 'pitch_dio.hip' in open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert P.dio is P.pitch.dio and P.stonemask is P.pitch.stonemask and P.world_f0 is P.pitch.world_f0
    assert P.evaluate.F0_METHODS == ('yin', 'dio') and P.evaluate.ENVELOPES == ('stft', 'cheaptrick')
    assert P.evaluate.ALIGNMENTS == ('exact', 'fastdtw')
    assert lib.tdvc_dio_num_bands(50.0, 500.0, 2.0) == 7 == R.num_bands(50.0, 500.0, 2.0)
    assert lib.tdvc_dio_num_bands(71.0, 800.0, 4.0) == 14 == R.num_bands(71.0, 800.0, 4.0)
    for bad in ((0.0, 500.0, 2.0), (500.0, 50.0, 2.0), (50.0, 500.0, 0.0), (50.0, 500.0, 5.0), (50.0, float('nan'), 2.0)):
        assert lib.tdvc_dio_num_bands(*bad) == 0, bad


def test_dio_refusals_through_the_raw_abi_before_any_launch():
    lib = pkg()._lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 44
    B, T, hop, fs = 2, 4000, 80, 16000
    F = T // hop + 1

    def query(B=B, T=T, F=F, hop=hop, fs=fs, floor=50.0, ceil=500.0, cpo=2.0):
        return lib.tdvc_dio_workspace(B, T, F, hop, fs, floor, ceil, cpo)

    def call(B=B, T=T, F=F, hop=hop, fs=fs, floor=50.0, ceil=500.0, cpo=2.0, allowed=0.1, x=p, f0=p, s_bs=T, s_ts=1, f0_bs=F, cand=None,
             score=None, ws=p, ws_bytes=big):
        return lib.tdvc_dio(x, s_bs, s_ts, None, T, B, F, hop, fs, floor, ceil, cpo, allowed, f0, f0_bs, cand, score, ws, ws_bytes, None)
    need = query()
    assert need >= B * T * 8 * (1 + 2 * 7) and query(B=1) < need
    cases = [
        (dict(B=-1), EINVAL), (dict(T=-1), EINVAL), (dict(F=-1), EINVAL), (dict(hop=0), EINVAL), (dict(fs=0), EINVAL),
        (dict(floor=0.0), EINVAL), (dict(floor=-5.0), EINVAL), (dict(ceil=50.0), EINVAL), (dict(ceil=40.0), EINVAL),
        (dict(ceil=float('inf')), EINVAL), (dict(floor=float('nan')), EINVAL), (dict(cpo=0.0), EINVAL), (dict(cpo=float('nan')), EINVAL),
        (dict(ceil=20000.0, cpo=1.0), EINVAL),                                       # a band above fs
        (dict(cpo=5.0), EUNSUPPORTED), (dict(ceil=4000.0, cpo=3.0), EUNSUPPORTED),        # 17 and 19 bands
        (dict(T=(1 << 21) + 1, F=(1 << 21) // hop + 2), EUNSUPPORTED), (dict(B=65536), EUNSUPPORTED),
        (dict(fs=52000), EUNSUPPORTED),                                             # low-cut of 2081 taps
        (dict(floor=10.0), EUNSUPPORTED),                                           # lowest band of 2264 taps
    ]
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert b'dio' in lib.tdvc_last_error(), kw
        assert query(**{k: v for k, v in kw.items() if k in ('B', 'T', 'F', 'hop', 'fs', 'floor', 'ceil', 'cpo')}) == 0, kw
    late = [
        (dict(allowed=0.0), EINVAL), (dict(allowed=float('nan')), EINVAL), (dict(s_bs=-1), EINVAL), (dict(s_ts=-1), EINVAL),
        (dict(f0_bs=-1), EINVAL), (dict(F=F - 1), EINVAL), (dict(f0_bs=F - 1), EINVAL), (dict(x=None), EINVAL), (dict(f0=None), EINVAL),
        (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE), (dict(ws_bytes=need - 1), EWORKSPACE),
    ]
    for kw, want in late:
        assert call(**kw) == want, (kw, want)
        assert b'dio' in lib.tdvc_last_error(), kw
    assert query(F=F - 1) == 0 and query(B=0) == 0
    assert call(B=0) == 0 and call(B=0, x=None, f0=None, ws=None, ws_bytes=0) == 0 and call(F=0, T=0) == 0      # no-ops
    assert call(B=0, cpo=5.0) == EUNSUPPORTED                                       # the arguments are still checked
    assert not any(buf)


def test_stonemask_refusals_through_the_raw_abi_before_any_launch():
    lib = pkg()._lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    B, T, F = 2, 4000, 51

    def call(B=B, T=T, F=F, hop=80, fs=16000, x=p, fi=p, fo=p, s_bs=T, s_ts=1, fi_bs=F, fi_fs=1, fo_bs=F):
        return lib.tdvc_stonemask(x, s_bs, s_ts, None, T, fi, fi_bs, fi_fs, B, F, hop, fs, fo, fo_bs, None)
    cases = [
        (dict(B=-1), EINVAL), (dict(T=-1), EINVAL), (dict(F=-1), EINVAL), (dict(hop=0), EINVAL), (dict(fs=0), EINVAL),
        (dict(s_bs=-1), EINVAL), (dict(s_ts=-1), EINVAL), (dict(fi_bs=-1), EINVAL), (dict(fi_fs=-1), EINVAL), (dict(fo_bs=-1), EINVAL),
        (dict(fo_bs=F - 1), EINVAL), (dict(x=None), EINVAL), (dict(fi=None), EINVAL), (dict(fo=None), EINVAL),
        (dict(fs=55000), EUNSUPPORTED), (dict(B=1 << 16, F=1 << 15), EUNSUPPORTED), (dict(F=1 << 25, hop=80, B=1), EUNSUPPORTED),
    ]
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert b'stonemask' in lib.tdvc_last_error(), kw
    assert call(B=0) == 0 and call(F=0) == 0 and call(B=0, x=None, fi=None, fo=None) == 0
    assert call(B=0, fs=55000) == EUNSUPPORTED
    assert not any(buf)


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('f', (60, 100, 220, 480))
def test_steady_tones_are_tracked_within_the_bar(f):
    x = R.tone(f)
    r = R.dio(x)
    F, vrm = len(r['f0']), r['vrm']
    assert F == 101 and vrm == 9 and r['nb'] == 7
    inner = slice(vrm + 1, F - vrm - 1)
    assert (r['f0'][inner] > 0).all()
    e_dio = np.abs(r['f0'][inner] - f).max() / f
    s = R.stonemask(x, R.f32(r['f0']))
    e_sm = np.abs(s[inner] - f).max() / f
    s5 = R.stonemask(x, np.full(F, f * 1.05))
    e_5 = np.abs(s5[inner] - f).max() / f
    print(f'\n{f} Hz: worst relative error dio {e_dio:.3e}, stonemask {e_sm:.3e}, from a track 5 % off {e_5:.3e} (bar {TONE_BAR:.2e})')
    assert e_dio <= TONE_BAR and e_sm <= TONE_BAR and e_5 <= TONE_BAR
    for m in (1.3, 0.7):                                                        # the clamp, true of every frame
        s30 = R.stonemask(x, np.full(F, f * m))
        assert ((s30 == f * m) | (np.abs(s30 - f * m) <= 0.2 * f * m)).all()


@pytest.mark.parametrize('f', (60, 100, 220, 480))
def test_stonemask_returns_a_track_30_percent_off_a_sinusoid(f):
    n = 8000
    x = (0.1 * np.sin(2 * np.pi * f * np.arange(n) / R.FS) + 1e-4 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)
    F = n // R.HOP + 1
    track = np.full(F, f * 1.3)
    s = R.stonemask(x, track)
    edge = int(1.5 * R.FS / (f * 1.3) + 1) // R.HOP + 1                         # frames whose window is clamped at a row end
    assert (s[edge:F - edge] == track[edge:F - edge]).all()
    assert ((s == track) | (np.abs(s - track) <= 0.2 * track)).all()


def test_stonemask_special_values_give_zero():
    x = R.tone(220)
    s = R.stonemask(x, np.array([0.0, 40.0, R.FS / 12 + 1, np.nan, np.inf, -100.0, 40.001, R.FS / 12]))
    assert (s[:6] == 0).all() and (s[6:] > 0).all()
    assert (R.stonemask(np.zeros(0), np.array([100.0, 200.0])) == 0).all()


def test_silence_constant_and_short_rows_give_zeros():
    for x in (np.zeros(4000, np.float32), np.full(4000, 0.3, np.float32)):
        r = R.dio(x)
        assert (r['f0'] == 0).all() and (r['cand'] == 0).all() and (r['score'] == R.BIG / R.EPS).all()
    r = R.dio_of('short')
    assert len(r['f0']) == r['vrm'] == 9 and (r['f0'] == 0).all() and (r['cand'] != 0).any()      # candidates exist, the fix refuses
    assert (R.dio(np.zeros(0))['f0'] == 0).all() and len(R.dio(np.zeros(0))['f0']) == 1


def test_1500_samples_leave_the_lowest_band_without_candidates():
    r = R.dio_of('row1500')
    assert len(r['f0']) == 19 and (r['cand'][0] == 0).all() and (r['score'][0] == R.BIG / R.EPS).all()
    used = r['best'] != 0
    assert used.sum() >= 10 and (np.abs(r['best'][used][2:-2] - 220) < 220 * 0.02).all()      # the other bands are used


@pytest.mark.parametrize('f', (45, 520))
def test_tones_outside_floor_and_ceil_are_rejected(f):
    r = R.dio(R.tone(f))
    assert (r['f0'] == 0).all()
    inner = slice(r['vrm'] + 1, len(r['f0']) - r['vrm'] - 1)
    assert (np.abs(r['cand'][:, inner] - f) > 0.02 * f).all()                   # no band keeps a candidate at the tone


def test_step_is_zeroed_then_regrown_up_to_the_jump():
    r = R.dio_of('step')
    jump = 4000 // R.HOP                                                         # frame 50
    assert (r['s2'][jump - 4:jump + 5] == 0).all()                              # step 1 zeroes the jump, step 2 widens it
    f0 = r['f0']
    assert (f0[jump - 4:jump] > 0).all() and (f0[jump + 1:jump + 5] > 0).all()  # re-grown from both sides
    assert (np.abs(f0[20:jump] - 100) < 10).all() and (np.abs(f0[jump + 1:80] - 200) < 20).all()
    assert f0[jump] == 0                                                         # and not across it


# ------------------------------------------------------------------------------------------------------------ licences for the GPU test
@pytest.mark.parametrize('name', R.GPU_WAVEFORMS)
def test_decisions_are_stable_under_rounding_level_noise(name):
    x, p = R.waveform(name).astype(np.float64), R.params(name)
    rng = np.random.default_rng(11)
    a = R.dio_of(name)
    b = R.dio(x * (1 + 1e-12 * rng.standard_normal(len(x))), **p)
    va, vb = a['f0'] > 0, b['f0'] > 0
    assert np.array_equal(va, vb) and np.array_equal(a['cand'] == 0, b['cand'] == 0)
    rel = float((np.abs(a['f0'] - b['f0'])[va] / a['f0'][va]).max()) if va.any() else 0.0
    wa, _ = R.world_of(name)
    wb = R.stonemask(x * (1 + 1e-12 * rng.standard_normal(len(x))), R.f32(b['f0']), p['fs'], p['hop'])
    assert np.array_equal(wa > 0, wb > 0)
    wrel = float((np.abs(wa - wb)[wa > 0] / wa[wa > 0]).max()) if (wa > 0).any() else 0.0
    print(f'\n{name}: voiced {int(va.sum())} of {len(va)}, no flips; relative difference dio {rel:.1e}, stonemask {wrel:.1e}')
    assert rel <= 1e-10 and wrel <= 1e-10


@pytest.mark.parametrize('name', WORLD_INPUTS)
def test_fp32_round_trip_moves_no_voiced_frame(name):
    x, p = R.waveform(name).astype(np.float64), R.params(name)
    want, d = R.world_of(name)
    f32 = d.astype(np.float32)
    v = want > 0
    assert v.any()
    for sign in (-1.0, 1.0):
        nudged = np.nextafter(f32, np.float32(sign * np.inf)).astype(np.float64)
        nudged[f32 == 0] = 0
        got = R.stonemask(x, nudged, p['fs'], p['hop'])
        assert (np.abs(got - want)[v] <= 4 * 2.0 ** -24 * want[v]).all()
