"""Numpy restatement of the CheapTrick spectral envelope behind tdvc_cheaptrick (include/tdvc.h), frame by frame. Test helper,
written from the definition; it imports nothing from the package.

With N = n_fft, h = N/2, df = fs/N and frame fr centred on sample pos = fr * hop of a row of `length` valid samples:
    f      = f0 if it is finite and 3 fs/(N - 3) < f0 <= fs/4, else 500                      (the fs/4 cap is this project's)
    half   = floor(1.5 fs/f + 0.5);  k = -half .. half;  idx = clamp(pos + k, 0, length - 1)
    w      = 0.5 cos(pi f k / (1.5 fs)) + 0.5;  w /= sqrt(sum w^2);  s = x[idx] w;  s -= w sum(s)/sum(w)
    P      = |rfft(s, N)|^2;  P[i] += lin(P, (f - i df)/df) for i < 1 + floor(f N/fs)          (from the uncorrected P)
    m      = [P[bd] .. P[1], P[0] .. P[h], P[h-1] .. P[h-bd]],  bd = floor(wd N/fs) + 1,  wd = 2 f/3;  seg = cumsum(m df)
    S[i]   = (lin(seg, i + wd/(2 df) + bd - 0.5) - lin(seg, i - wd/(2 df) + bd - 0.5)) / wd;  S = max(S, floor) + 2.2e-16
    C      = Re rfft(even extension of log S);  c[n] = C[n] sinc(f n/fs) ((1 - 2 q1) + 2 q1 cos(2 pi f n/fs)) / N
    env    = exp(Re rfft(even extension of c))
where lin(y, p) = y[j] + (y[j+1] - y[j]) (p - j), j = floor(p) (kept inside the array). The mel-cepstrum of the frame is
freqt(c with c[0] halved): irfft(log env)[0 .. h] IS c.

Two arithmetic back ends: F64 (numpy float64, numpy's FFT) is the reference; LD evaluates the same statements in numpy's long
double with a direct DFT from an exactly reduced table, and is what the sensitivity test compares F64 against.
"""
import functools

import numpy as np

DEFAULT_F0 = 500.0
EPS = 2.2e-16
FLOOR = 1e-16          # evaluate.CHEAPTRICK_FLOOR


class F64:
    dtype = np.float64
    pi = np.pi

    @staticmethod
    def rfft(x, n):
        X = np.fft.rfft(x, n)
        return X.real, X.imag

    @staticmethod
    def rfft_even(v, n):
        """Re rfft of the even extension of v [n/2 + 1]."""
        return np.fft.rfft(even(v), n).real


@functools.lru_cache(maxsize=None)
def _ld_tables(n):
    ld = np.longdouble
    ang = 2 * LD.pi * np.arange(n, dtype=ld) / ld(n)
    idx = (np.arange(n, dtype=np.int64)[:, None] * np.arange(n // 2 + 1, dtype=np.int64)[None, :]) % n      # j k mod n: exact reduction
    return np.cos(ang)[idx], np.sin(ang)[idx]


class LD:
    dtype = np.longdouble
    pi = np.longdouble(4) * np.arctan(np.longdouble(1))

    @staticmethod
    def rfft(x, n):
        cm, sm = _ld_tables(n)
        x = np.asarray(x, np.longdouble)
        return x @ cm[:len(x)], -(x @ sm[:len(x)])

    @staticmethod
    def rfft_even(v, n):
        """The cosine sum v[0] + (-1)^k v[h] + 2 sum_{0 < j < h} v[j] cos(2 pi j k/n): half the terms of the extended sequence."""
        cm, _ = _ld_tables(n)
        h = n // 2
        v = np.asarray(v, np.longdouble)
        return v[0] + v[h] * cm[h] + 2 * (v[1:h] @ cm[1:h])


def f0_floor(fs, n_fft):
    return 3.0 * fs / (n_fft - 3.0)


def effective_f0(f0, fs, n_fft):
    f = float(f0)
    return f if np.isfinite(f) and f0_floor(fs, n_fft) < f <= fs / 4.0 else DEFAULT_F0


def half_width(f, fs):
    return int(np.floor(1.5 * fs / f + 0.5))          # halves away from zero (the argument is positive)


def lin(y, p):
    j = np.clip(np.floor(p).astype(np.int64), 0, len(y) - 2)
    return y[j] + (y[j + 1] - y[j]) * (p - j)


def window(x, pos, f, fs, be=F64):
    """Row x (its valid samples) -> (w normalised, s windowed and freed of its mean), both [2 half + 1] in be.dtype."""
    T = be.dtype
    half = half_width(f, fs)
    k = np.arange(-half, half + 1)
    seg = np.asarray(x, T)[np.clip(pos + k, 0, len(x) - 1)] if len(x) else np.zeros(len(k), T)
    w = T(0.5) * np.cos(be.pi * T(f) * k.astype(T) / T(1.5 * fs)) + T(0.5)
    w = w / np.sqrt((w * w).sum())
    s = seg * w
    return w, s - w * (s.sum() / w.sum())


def dc_correct(P, f, fs, n_fft):
    T = P.dtype.type
    df = T(fs) / T(n_fft)
    i = np.arange(1 + int(np.floor(f * n_fft / fs)))
    out = P.copy()
    out[i] = P[i] + lin(P, (T(f) - i.astype(P.dtype) * df) / df)
    return out


def mirrored(P, bd):
    h = len(P) - 1
    return np.concatenate([P[bd:0:-1], P, P[h - 1:h - bd - 1:-1]])


def smooth(P, f, fs, n_fft):
    """Mean of the mirrored staircase over [i df - wd/2, i df + wd/2], wd = 2 f/3, from its running integral."""
    T = P.dtype.type
    h = n_fft // 2
    df, wd = T(fs) / T(n_fft), T(2) * T(f) / T(3)
    bd = int(np.floor(wd * T(n_fft) / T(fs))) + 1
    seg = np.cumsum(mirrored(P, bd) * df)
    i = np.arange(h + 1).astype(P.dtype)
    off = wd / (T(2) * df)
    return (lin(seg, i + off + T(bd) - T(0.5)) - lin(seg, i - off + T(bd) - T(0.5))) / wd


def even(v):
    return np.concatenate([v, v[-2:0:-1]])


def lifter(S, f, fs, n_fft, q1, be=F64):
    """Smoothed spectrum S [h + 1] -> liftered cepstrum c [h + 1] (= irfft(log env)[0 .. h])."""
    T = be.dtype
    h = n_fft // 2
    C = be.rfft_even(np.log(S), n_fft)
    q = np.arange(h + 1).astype(T) / T(fs)
    sl = np.ones(h + 1, T)
    sl[1:] = np.sin(be.pi * T(f) * q[1:]) / (be.pi * T(f) * q[1:])
    cl = (T(1) - T(2) * T(q1)) + T(2) * T(q1) * np.cos(T(2) * be.pi * T(f) * q)
    return C * sl * cl / T(n_fft)


def frame(x, pos, f0, fs, n_fft, q1=-0.15, floor=FLOOR, be=F64):
    """One frame -> dict(f, w, s, P raw power, S smoothed with the safeguard, c liftered cepstrum, env)."""
    T = be.dtype
    f = effective_f0(f0, fs, n_fft)
    w, s = window(x, pos, f, fs, be)
    re, im = be.rfft(s, n_fft)
    P = re * re + im * im
    S = np.maximum(smooth(dc_correct(P, f, fs, n_fft), f, fs, n_fft), T(floor)) + T(EPS)
    c = lifter(S, f, fs, n_fft, q1, be)
    env = np.exp(be.rfft_even(c, n_fft))
    return dict(f=f, w=w, s=s, P=P, S=S, c=c, env=env)


def cheaptrick(x, f0, fs, n_fft, hop, q1=-0.15, floor=FLOOR, length=None, be=F64):
    """x [T], f0 [F] -> (env [F, h + 1], c [F, h + 1]) in be.dtype; samples at and past `length` are not looked at."""
    x = np.asarray(x)[:len(x) if length is None else length]
    fr = [frame(x, i * hop, f0[i], fs, n_fft, q1, floor, be) for i in range(len(f0))]
    return np.stack([r['env'] for r in fr]), np.stack([r['c'] for r in fr])


def freqt(c, order, alpha):
    """SPTK's frequency transform of c [m1 + 1] -> [order + 1] (the recursion of include/tdvc.h)."""
    b = 1.0 - alpha * alpha
    g = np.zeros(order + 1)
    for v in c[::-1]:
        d = g.copy()
        g[0] = v + alpha * d[0]
        if order >= 1:
            g[1] = b * d[0] + alpha * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


def mc_from_c(c, order, alpha):
    """Liftered cepstra [..., h + 1] -> mel-cepstra [..., order + 1]: c[0] halved, then freqt."""
    c = np.array(c, np.float64)
    c[..., 0] *= 0.5
    flat = c.reshape(-1, c.shape[-1])
    return np.stack([freqt(r, order, alpha) for r in flat]).reshape(c.shape[:-1] + (order + 1,))


# ------------------------------------------------------------------------------------------------------------ shared inputs
FS, HOP, T_CASE, F_CASE = 16000, 80, 2401, 34          # frame 30 sits on the last sample, frames 31 .. 33 past the row end


def voiced(rng, T, f0, fs=FS, noise_db=-30.0):
    """Harmonics of f0 (with a slow vibrato) under a formant-shaped envelope, scaled to unit RMS, plus white noise noise_db down.
    The noise sets the depth of the valleys of the smoothed spectrum, and the smoothing is a difference of running sums: in float64
    an element 10^(r/10) under the frame's peak carries a relative error of some 4e-15 * 10^(r/10) (measured against the long double
    evaluation: 2.6e-6 with the noise 60 dB down, where the envelopes span 95 dB; 1.2e-8 at 40 dB; 2.1e-9 at 30 dB, where they
    span 69 dB). 30 dB keeps the float64 reference 7 times inside 2^-24 / 4."""
    t = np.arange(T) / fs
    phase = 2 * np.pi * np.cumsum(f0 * (1 + 0.02 * np.sin(2 * np.pi * 4.0 * t))) / fs
    x = sum(np.sin(k * phase + 0.3 * k) / (1 + ((k * f0 - 700.0) / 600.0) ** 2) for k in range(1, int(0.45 * fs / f0)))
    x = x / np.sqrt(np.mean(x * x))
    return 0.1 * (x + 10 ** (noise_db / 20) * rng.standard_normal(T))


def special_f0(fs, n_fft):
    """The per-frame F0 values whose handling the definition spells out, as fp32."""
    lo, cap = np.float32(f0_floor(fs, n_fft)), np.float32(fs / 4.0)
    up = lambda v: np.nextafter(v, np.float32(np.inf))
    below = lo if float(lo) <= f0_floor(fs, n_fft) else np.nextafter(lo, np.float32(0))
    return np.array([0.0, np.nan, -120.0, below, up(below), cap, up(cap), 55.0, 140.0, 480.0, 384.0, 500.0, np.inf, 231.7], np.float32)


@functools.lru_cache(maxsize=None)
def case(n_fft):
    """The inputs of the device tests: dict(x fp32 [2, T], f0 fp32 [2, F], lengths, fs, hop, n_fft). Row 0 runs through the special
    F0 values (twice, so that each meets an interior and an edge position) and plain ones; row 1 follows its own pitch and is cut
    short by `lengths`."""
    rng = np.random.default_rng(n_fft)
    x = np.stack([voiced(rng, T_CASE, 140.0), 0.3 * voiced(rng, T_CASE, 210.0)]).astype(np.float32)
    sp = special_f0(FS, n_fft)
    f0 = np.empty((2, F_CASE), np.float32)
    f0[0] = np.resize(np.concatenate([sp[7:], sp]), F_CASE)
    f0[1] = 210.0 * (1 + 0.02 * np.sin(np.arange(F_CASE)))
    f0[1, ::9] = 0.0
    for a in (x, f0):
        a.setflags(write=False)
    return dict(x=x, f0=f0, lengths=np.array([T_CASE, 1999], np.int32), fs=FS, hop=HOP, n_fft=n_fft)


@functools.lru_cache(maxsize=None)
def case_ref(n_fft, with_lengths=True):
    """float64 (env [2, F, h + 1], c [2, F, h + 1]) of case(n_fft); computed once and shared, read-only."""
    k = case(n_fft)
    out = [cheaptrick(k['x'][b], k['f0'][b], k['fs'], n_fft, k['hop'], length=int(k['lengths'][b]) if with_lengths else None) for b in range(2)]
    env, c = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    env.setflags(write=False)
    c.setflags(write=False)
    return env, c


def harmonic_sum(f0, T, fs=FS):
    """Equal-amplitude, zero-phase sum of all harmonics of f0 below Nyquist -> (x [T], number of harmonics)."""
    nh = int(np.ceil(fs / 2.0 / f0)) - 1
    t = np.arange(T) / fs
    return sum(np.cos(2 * np.pi * k * f0 * t) for k in range(1, nh + 1)), nh


RECOVERY_F0 = (100.0, 250.0)
# peak-to-peak of log env over [3 f0, (nh - 3) f0], the largest over the 8 frame positions of recovery_case, as the float64 reference
# measures it (tests/test_cheaptrick_cpu.py prints the figures); the bar of the CPU and of the device test is 4 x this
RECOVERY_FLATNESS = {100.0: 8.61e-4, 250.0: 3.35e-4}


@functools.lru_cache(maxsize=None)
def recovery_case(f0, n_fft=1024, fs=FS):
    """dict(x [T] float64, hop, frames: 8 frame indices one eighth of a period apart from sample 2000 on, band: the bins inside
    [3 f0, (nh - 3) f0])."""
    x, nh = harmonic_sum(f0, 4000, fs)
    hop = int(round(fs / f0)) // 8
    first = 2000 // hop
    assert first * hop == 2000
    k = np.arange(n_fft // 2 + 1) * fs / n_fft
    x.setflags(write=False)
    return dict(x=x, hop=hop, frames=np.arange(first, first + 8), band=(k >= 3 * f0) & (k <= (nh - 3) * f0), n_fft=n_fft, fs=fs)
