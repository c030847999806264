"""Float64 numpy restatement of the DIO and StoneMask definitions of include/tdvc.h (WORLD's dio.cpp, stonemask.cpp and
matlabfunctions.cpp with pyworld's defaults), written for the eye: loop for loop and tie for tie, nothing shared with the kernels.
It is NOT pyworld, which is not available to this repository; tests/test_dio_cpu.py pins it to facts that do not come from the code
under test. Also the waveforms that the CPU and the GPU tests share, and their cached references (read-only)."""
import functools
import math

import numpy as np

EPS = 1e-12
BIG = 100000.0
FS, HOP = 16000, 80


def mround(v):
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def num_bands(f0_floor, f0_ceil, cpo):
    return 1 + int(math.log2(f0_ceil / f0_floor) * cpo)


def vrm_of(fs, hop, f0_floor):
    return int(0.5 + fs / hop / f0_floor) * 2 + 1


def lowcut(x, fs):
    """y = x - mean, then the zero-phase low-cut FIR of 2 c + 1 taps as a linear convolution with zeros outside the row."""
    c = mround(fs / 50.0)
    n = 2 * c + 1
    h = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 1) / (n + 1)) for i in range(n)])
    h = -h / h.sum()
    h[c] += 1.0
    y = x - x.mean()
    return np.convolve(y, h)[c:c + len(x)]


def nuttall(n):
    u = np.arange(n) / (n - 1.0)
    return 0.355768 - 0.487396 * np.cos(2 * np.pi * u) + 0.144232 * np.cos(4 * np.pi * u) - 0.012604 * np.cos(6 * np.pi * u)


def events(g, fs):
    """(locations, values) of the intervals between consecutive negative-going crossings of g."""
    fine = []
    for i in range(len(g) - 1):
        if 0 < g[i] and g[i + 1] <= 0:
            fine.append((i + 1) - g[i] / (g[i + 1] - g[i]))
    if len(fine) < 2:
        return np.zeros(0), np.zeros(0)
    fine = np.array(fine)
    return (fine[:-1] + fine[1:]) / 2 / fs, fs / (fine[1:] - fine[:-1])


def interp1(x, y, xi):
    """WORLD's histc + interp1: the line through intervals k - 1 and k, k = the number of locations <= xi clipped to [1, n - 1]."""
    out = np.zeros(len(xi))
    for i, t in enumerate(xi):
        k = min(max(int(np.searchsorted(x, t, side='right')), 1), len(x) - 1)
        s = (t - x[k - 1]) / (x[k] - x[k - 1])
        out[i] = y[k - 1] + s * (y[k] - y[k - 1])
    return out


def dio(x, fs=FS, hop=HOP, f0_floor=50.0, f0_ceil=500.0, cpo=2.0, allowed=0.1):
    """x: the valid samples of one row -> dict: f0 [F_b] float64 (before the fp32 rounding), cand / score [nb, F_b], and the
    intermediate tracks best, s1, s2, s3 of the fix steps."""
    x = np.asarray(x, np.float64)
    n = len(x)
    F = n // hop + 1
    t = np.array([i * hop / fs for i in range(F)])
    nb = num_bands(f0_floor, f0_ceil, cpo)
    bf = [f0_floor * 2.0 ** ((k + 1) / cpo) for k in range(nb)]
    cand = np.zeros((nb, F))
    score = np.full((nb, F), BIG / EPS)
    if n > 0:
        y = lowcut(x, fs)
        for k in range(nb):
            hal = mround(fs / bf[k] / 2.0)
            f = np.convolve(y, nuttall(4 * hal))[2 * hal:2 * hal + n]
            d = f[1:] - f[:-1]
            lists = [events(f, fs), events(-f, fs), events(-d, fs), events(d, fs)]
            if min(len(e[0]) for e in lists) <= 2:
                continue
            v = [interp1(e[0], e[1], t) for e in lists]
            for i in range(F):
                c = (((v[0][i] + v[1][i]) + v[2][i]) + v[3][i]) / 4.0
                q = 0.0
                for m in range(4):
                    q += (v[m][i] - c) * (v[m][i] - c)
                s = math.sqrt(q / 3.0)
                if c > bf[k] or c < bf[k] / 2.0 or c > f0_ceil or c < f0_floor:
                    c, s = 0.0, BIG
                cand[k, i], score[k, i] = c, s / (c + EPS)
    best = np.zeros(F)
    for i in range(F):
        bs = score[0, i]
        best[i] = cand[0, i]
        for k in range(1, nb):
            if score[k, i] < bs:
                bs, best[i] = score[k, i], cand[k, i]
    out = dict(cand=cand, score=score, best=best, nb=nb, vrm=vrm_of(fs, hop, f0_floor))
    vrm = out['vrm']
    if F <= vrm:
        out.update(f0=np.zeros(F), s1=np.zeros(F), s2=np.zeros(F), s3=np.zeros(F))
        return out
    base = best.copy()
    base[:vrm] = 0
    base[F - vrm:] = 0
    s1 = np.zeros(F)
    for i in range(vrm, F):
        s1[i] = base[i] if abs((base[i] - base[i - 1]) / (EPS + base[i])) < allowed else 0.0
    s2 = s1.copy()
    c = (vrm - 1) // 2
    for i in range(c, F - c):
        for j in range(-c, c + 1):
            if s1[i + j] == 0:
                s2[i] = 0
    neg = [i - 1 for i in range(1, F) if s2[i] == 0 and s2[i - 1] != 0]
    pos = [i for i in range(1, F) if s2[i - 1] == 0 and s2[i] != 0]

    def select(cur, past, fr):
        ref = (cur * 3.0 - past) / 2.0
        v, err = cand[0, fr], abs(ref - cand[0, fr])
        for k in range(1, nb):
            if abs(ref - cand[k, fr]) < err:
                v, err = cand[k, fr], abs(ref - cand[k, fr])
        return 0.0 if abs(1.0 - v / ref) > allowed else v
    s3 = s2.copy()
    for n_, start in enumerate(neg):
        lim = F - 1 if n_ == len(neg) - 1 else neg[n_ + 1]
        for j in range(start, lim):
            s3[j + 1] = select(s3[j], s3[j - 1], j + 1)
            if s3[j + 1] == 0:
                break
    s4 = s3.copy()
    for n_ in range(len(pos) - 1, -1, -1):
        lim = 1 if n_ == 0 else pos[n_ - 1]
        for j in range(pos[n_], lim, -1):
            s4[j - 1] = select(s4[j], s4[j + 1], j - 1)
            if s4[j - 1] == 0:
                break
    out.update(f0=s4, s1=s1, s2=s2, s3=s3)
    return out


def stonemask(x, f0, fs=FS, hop=HOP):
    """x: the valid samples of one row, f0 [F] (the fp32 track, as float64) -> refined track float64 [F]."""
    x = np.asarray(x, np.float64)
    n = len(x)
    out = np.zeros(len(f0))
    for fr, f in enumerate(np.asarray(f0, np.float64)):
        if not np.isfinite(f) or f <= 40.0 or f > fs / 12.0 or n == 0:
            continue
        t = fr * hop / fs
        half = int(1.5 * fs / f + 1)
        N = 2 ** (2 + int(math.log2(2 * half + 1)))
        raw = np.array([mround((t + k / fs) * fs + 0.001) for k in range(-half, half + 1)])
        u = ((raw - 1.0) / fs - t) / ((2 * half + 1.0) / fs)
        mw = 0.42 + 0.5 * np.cos(2 * np.pi * u) + 0.08 * np.cos(4 * np.pi * u)
        dw = np.zeros_like(mw)
        dw[1:-1] = -(mw[2:] - mw[:-2]) / 2
        dw[0] = -mw[1] / 2
        dw[-1] = mw[-2] / 2
        seg = x[np.clip(raw - 1, 0, n - 1)]
        M, D = np.fft.fft(seg * mw, N), np.fft.fft(seg * dw, N)
        P = M.real ** 2 + M.imag ** 2
        num = M.real * D.imag - M.imag * D.real

        def fix(g, nh):
            a = d = 0.0
            for h in range(1, nh + 1):
                idx = mround(g * N / fs * h)
                p_, n_ = P[idx % N], num[idx % N]
                inst = 0.0 if p_ == 0 else idx * fs / N + n_ / p_ * fs / 2 / math.pi
                amp = math.sqrt(p_)
                a += amp * inst
                d += amp * h
            return a / (d + EPS)
        tent = fix(f, 2)
        r = 0.0 if (tent <= 0 or tent > f * 2) else fix(tent, min(int(fs / 2.0 / f), 6))
        if abs(r - f) > 0.2 * f:
            r = f
        out[fr] = r
    return out


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def world_f0(x, fs=FS, hop=HOP, **kw):
    """stonemask on DIO's track after its one fp32 rounding -> (refined float64, the fp32 DIO track as float64)."""
    d = f32(dio(x, fs, hop, **kw)['f0'])
    return stonemask(x, d, fs, hop), d


# ------------------------------------------------------------------------------------------------------------ shared waveforms
def harmonic(f_inst, fs, rng, noise_db=-60.0, amp=0.1):
    """7 harmonics with 1/k amplitudes on the instantaneous frequency f_inst (0 = silence), plus white noise."""
    ph = 2 * np.pi * np.cumsum(f_inst) / fs
    x = sum(np.sin(k * ph) / k for k in range(1, 8)) * amp * (f_inst > 0)
    return x + amp * 10 ** (noise_db / 20) * rng.standard_normal(len(f_inst))


def tone(f, fs=FS, dur=0.5, seed=0):
    n = int(dur * fs)
    return harmonic(np.full(n, float(f)), fs, np.random.default_rng(seed)).astype(np.float32)


def glide(T, seed, fs=FS):
    """A harmonic glide with two unvoiced gaps (noise only) and -60 dB noise, fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / fs
    f = 150 + 60 * np.sin(2 * np.pi * (0.9 + 0.2 * seed) * t) + 30 * t
    f[int(0.30 * T):int(0.42 * T)] = 0
    f[int(0.70 * T):int(0.78 * T)] = 0
    return harmonic(f, fs, rng).astype(np.float32)


def step_tone(fs=FS, n=8000, seed=3):
    f = np.where(np.arange(n) < n // 2, 100.0, 200.0)
    return harmonic(f, fs, np.random.default_rng(seed)).astype(np.float32)


GLIDE_LENGTHS = (4000, 8000, 16040)
P2 = dict(fs=24000, hop=120, f0_floor=71.0, f0_ceil=800.0, cpo=4.0)      # the second parameter set


def glide24(T=6000, seed=7):
    rng = np.random.default_rng(seed)
    t = np.arange(T) / 24000
    return harmonic(220 + 80 * np.sin(2 * np.pi * 2.0 * t), 24000, rng).astype(np.float32)


@functools.lru_cache(maxsize=None)
def waveform(name):
    """Every waveform the GPU tests use, by name (read-only fp32)."""
    if name == 'glide24':
        x = glide24()
    elif name.startswith('glide'):
        T = int(name[5:])
        x = glide(T, GLIDE_LENGTHS.index(T) if T in GLIDE_LENGTHS else 5)
    elif name == 'zeros':
        x = np.zeros(4000, np.float32)
    elif name == 'short':                     # F <= vrm
        x = glide(8000, 1)[2000:2000 + 8 * HOP + 5]
    elif name == 'row1500':
        x = tone(220, dur=1.0)[:1500]
    elif name == 'step':
        x = step_tone()
    elif name == 'lastframe':                 # the last frame sits on the final sample
        x = glide(8000, 1)[:77 * HOP + 1]
    elif name == 'tile-1':
        x = glide(8000, 2)[:4 * 1024 - 1]
    elif name == 'tile+1':
        x = glide(8000, 2)[:4 * 1024 + 1]
    elif name == 'ev-1':                      # the band kernels' tiles hold the events of 1022 samples
        x = glide(8000, 3)[:4 * 1022 - 1]
    elif name == 'ev+1':
        x = glide(8000, 3)[:4 * 1022 + 1]
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def params(name):
    return P2 if name == 'glide24' else dict(fs=FS, hop=HOP)


GPU_WAVEFORMS = ('glide4000', 'glide8000', 'glide16040', 'zeros', 'short', 'row1500', 'step', 'lastframe', 'tile-1', 'tile+1', 'ev-1', 'ev+1',
                 'glide24')


@functools.lru_cache(maxsize=None)
def dio_of(name):
    r = dio(waveform(name), **params(name))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def world_of(name):
    p = params(name)
    r, d = world_f0(waveform(name), **p)
    r.setflags(write=False)
    d.setflags(write=False)
    return r, d
