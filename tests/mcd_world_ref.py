"""The float64 chain behind mcd(f0_method='dio', envelope='cheaptrick', align='fastdtw'), from the waveform to the number, and the
pairs that tests/test_mcd_world_cpu.py (which shows the chain fit on them) and tests/test_mcd_world_gpu.py (which runs them) share.
Test helper: it composes the restatements dio_ref, cheaptrick_ref, fastdtw_ref and dtw_ref and imports nothing from the package.
It is the reference's test_scripts/common/test_mcd.py:29-91 as those restatements state its steps; none of pyworld, pysptk and
fastdtw is available, so it is NOT a parity statement against them.

    chain(x, length)   f0 = stonemask(x[:length], fp32(dio(x[:length])))      dio_ref.world_f0: 1 + length // 80 frames, frame f on sample 80 f
                       f0 = fp32(f0)                                           the device emits an fp32 track
                       c  = cheaptrick(x[:length], f0, n_fft=1024, hop=80)     cheaptrick_ref, float64
                       mc = mc_from_c(c, 24, 0.42)                             on the frames with f0 > 0: "remove silence"
    pipeline(t, r)     fastdtw(fp32(mc_t), fp32(mc_r), radius, 'l2') -> cost / length, and the F0 statistics of test_mcd.py:83-84 and :116

Waveforms: dio_ref.harmonic on f(t) = base (1 + 0.4 sin(2 pi (0.9 + 0.2 (seed % 5)) t) + 0.2 t) with two silent stretches and noise
30 dB down (at dio_ref's 60 dB the float64 CheapTrick is 3.5e-7 from its long double evaluation: not fit as a reference; at 30 dB
1.3e-9, tests/test_mcd_world_cpu.py). The figures of every pair, as the chain gives them, are printed by the CPU test.
"""
import functools

import numpy as np

import cheaptrick_ref as CR
import dio_ref as DIO
import dtw_ref as DR
import fastdtw_cases as FC
import fastdtw_ref as FR

FS, HOP, N_FFT, ORDER, ALPHA = 16000, 80, 1024, 24, 0.42
D = ORDER + 1
MIN_VOICED = 10

#        row      T     seed  base   length (the row is cut there: samples at and past it are padding)
ROWS = {
    'a_test': (8000, 1, 120.0, 8000),      # a multiple of the hop, the last frame (on sample 8000) voiced
    'a_ref':  (7600, 1, 200.0, 7600),      # the same
    'b_test': (8000, 3, 110.0, 8000),
    'b_ref':  (6400, 4, 220.0, 6400),      # the last frame unvoiced
    'c_test': (6400, 5, 100.0, 6400),      # the last frame unvoiced
    'c_ref':  (7200, 6, 260.0, 7200),
    'd_test': (4000, 2, 180.0, 3270),      # 1 voiced frame: under MIN_VOICED (from 3280 samples on DIO keeps a stretch of 13)
    'e_test': (8000, 1, 120.0, 7641),      # a_test cut where no frame sits: 96 frames, the last on sample 7600
}
#         pair  test      ref       radii of the device calls   radii at which the path must be the chain's (margin ratio >= 4)
PAIRS = {
    'A': ('a_test', 'a_ref', (1, 2), (1, 2)),
    'B': ('b_test', 'b_ref', (1, 2), ()),       # kept for the comparison of exact, radius 1 and radius 2 only: its margins are too small
    'C': ('c_test', 'c_ref', (1, 2), (1, 2)),
    'D': ('d_test', 'a_ref', (1, 2), ()),       # NaN: under MIN_VOICED on the test side
    'E': ('e_test', 'a_ref', (1, 2), (1, 2)),
}
ORDERED = ('A', 'B', 'C', 'D', 'E')            # the batch order of the device buffers
RADII = (1, 2)
EPS = FC.EPS                                    # (D + 2) 2^-24 at D = 25 with c0: the relative error of one fp32 'l2' distance
assert FC.D_REAL == D


@functools.lru_cache(maxsize=None)
def waveform(name):
    """fp32 [T] of ROWS[name], read-only; samples at and past the row's length exist and are never to be looked at."""
    T, seed, base, _ = ROWS[name]
    rng = np.random.default_rng(seed)
    t = np.arange(T) / FS
    f = base * (1 + 0.4 * np.sin(2 * np.pi * (0.9 + 0.2 * (seed % 5)) * t) + 0.2 * t)
    f[int(0.30 * T):int(0.42 * T)] = 0
    f[int(0.70 * T):int(0.78 * T)] = 0
    x = DIO.harmonic(f, FS, rng, noise_db=-30.0).astype(np.float32)
    x.setflags(write=False)
    return x


def length_of(name):
    return ROWS[name][3]


@functools.lru_cache(maxsize=None)
def _frame_mc(name, fr, f0_bits):
    """Mel-cepstrum float64 [D] of frame fr of the row under the fp32 F0 value with these bits: one CheapTrick frame, then mc_from_c."""
    f0 = float(np.array(f0_bits, np.uint32).view(np.float32))
    x = waveform(name)[:length_of(name)]
    mc = CR.mc_from_c(CR.frame(x, fr * HOP, f0, FS, N_FFT)['c'], ORDER, ALPHA)
    mc.setflags(write=False)
    return mc


def cepstra(name, f0_32, frames):
    """float64 [len(frames), D]: cheaptrick_ref -> mc_from_c of the named frames of the row under the fp32 track f0_32 [F]. Frame by
    frame and cached, so the device's own track costs nothing where it has the chain's bits."""
    bits = np.ascontiguousarray(f0_32, np.float32).view(np.uint32)
    return np.stack([_frame_mc(name, int(f), int(bits[f])) for f in frames]) if len(frames) else np.zeros((0, D))


def chain(x, length, name=None):
    """x [T], length -> dict(f0 fp32 [F] as float64, F = 1 + length // 80; dio: the fp32 DIO track; voiced bool [F]; mc float64
    [n_voiced, D]). With a row's name its per-frame cache is used; the arithmetic is the same."""
    x = np.asarray(x)[:length]
    refined, d = DIO.world_f0(x, FS, HOP)
    assert len(refined) == 1 + length // HOP
    f0 = DIO.f32(refined)
    voiced = f0 > 0
    if name is None:
        _, c = CR.cheaptrick(x, f0, FS, N_FFT, HOP)
        mc = CR.mc_from_c(c[voiced], ORDER, ALPHA)
    else:
        mc = cepstra(name, f0, np.nonzero(voiced)[0])
    for a in (f0, d, voiced, mc):
        a.setflags(write=False)
    return dict(f0=f0, dio=d, voiced=voiced, mc=mc)


@functools.lru_cache(maxsize=None)
def chain_of(name):
    return chain(waveform(name), length_of(name), name)


def f0_statistics(f_test, f_ref):
    """test_mcd.py:83-84 and :116 on two tracks (0 = unvoiced)."""
    vt, vr = f_test[f_test > 0], f_ref[f_ref > 0]
    return dict(diff_f0_mean=np.mean(np.log(vt)) - np.mean(np.log(vr)), diff_f0_var=np.log(np.var(vt)) - np.log(np.var(vr)),
                f0_ratio=np.mean(vr) / np.mean(vt))


def pipeline(test, ref, radius=1):
    """Two chain() results -> dict(mcd = cost / length, cost, length, path, levels, n_test, n_ref, the three statistics), or
    dict(mcd=nan, n_test, n_ref) under MIN_VOICED voiced frames on either side, as `mcd` answers."""
    n_test, n_ref = len(test['mc']), len(ref['mc'])
    if min(n_test, n_ref) < MIN_VOICED:
        return dict(mcd=float('nan'), n_test=n_test, n_ref=n_ref)
    w = FR.fastdtw(test['mc'].astype(np.float32), ref['mc'].astype(np.float32), radius, 'l2')
    return dict(mcd=w['cost'] / w['length'], cost=w['cost'], length=w['length'], path=w['path'], levels=w['levels'], n_test=n_test, n_ref=n_ref,
                **f0_statistics(test['f0'], ref['f0']))


@functools.lru_cache(maxsize=None)
def pipeline_of(pair, radius=1):
    t, r = PAIRS[pair][:2]
    return pipeline(chain_of(t), chain_of(r), radius)


@functools.lru_cache(maxsize=None)
def exact_of(pair):
    """The exact programme (dtw_ref) on the chain's fp32 cepstra: what align='exact' restates."""
    t, r = PAIRS[pair][:2]
    return DR.dtw(chain_of(t)['mc'].astype(np.float32), chain_of(r)['mc'].astype(np.float32), 'l2')


margin_ratio = FC.margin_ratio                 # min over levels of (smallest back-traced margin) / (4 * 2 eps cost of that level)
