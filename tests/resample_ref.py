"""Plain numpy float64 restatement of what tdvc_resample / tdvc_segment compute (include/tdvc.h): resampy's table-interpolated windowed
sinc as its per-sample loop with the FLOAT time register (not the polyphase bank the product builds), util.eq_rms, and the
segment steps of data/dataset.py load_audio. Test helper: the GPU tests take their truth from here, and test_resample_cpu.py pins
the loop itself to analytic tones. Written from the algorithm's description; resampy is not needed and was not compared against.

    table   n = num_zeros * 2^precision;  win = rolloff * sinc(rolloff * linspace(0, num_zeros, n + 1)) * kaiser(2n + 1, beta)[n:]
    setup   ratio = sr_new / sr_orig; win *= ratio if ratio < 1; delta = diff(win, append=win[-1]); scale = min(1, ratio);
            index_step = int(scale * 2^precision); n_out = int(n_in * ratio)
    output t, tr = t * (1 / ratio): n = int(tr), frac = scale * (tr - n)
      left    idx = frac * 2^precision, off = int(idx), eta = idx - off; i < min(n + 1, (len(win) - off) // index_step):
              y[t] += (win[off + i*step] + eta * delta[off + i*step]) * x[n - i]
      right   frac = scale - frac, same off / eta; k < min(n_in - n - 1, (len(win) - off) // index_step): ... * x[n + 1 + k]
"""
import functools

import numpy as np

U24 = 2.0 ** -24
BOUND_FACTOR = 4.0      # |y - truth| <= 4 * 2^-24 * max|truth_row|, the bar of tests/peq_ref.py: one rounding is a quarter of it
FILTERS = {'kaiser_best': (64, 9, 14.769656459379492, 0.9475937167399596), 'kaiser_fast': (16, 9, 8.555504641634386, 0.85)}
MIN_SEGMENT, SEGMENT_MULTI = 5120, 320
UP = ((8000, 16000), (16000, 24000))
DOWN = ((48000, 16000), (44100, 16000), (24000, 16000), (22050, 16000))


@functools.lru_cache(maxsize=None)
def sinc_window(name):
    num_zeros, precision, beta, rolloff = FILTERS[name]
    n = num_zeros * 2 ** precision
    win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, n + 1)) * np.kaiser(2 * n + 1, beta)[n:]
    win.setflags(write=False)
    return win, precision


def num_out(n_in, sr_orig, sr_new):
    return int(n_in * (float(sr_new) / sr_orig))


def resample_loop(x, sr_orig, sr_new, filter='kaiser_best'):
    """x [n_in] -> float64 [int(n_in * ratio)]: the per-sample loop, every product and sum in float64."""
    win, precision = sinc_window(filter) if isinstance(filter, str) else filter
    x = np.asarray(x, np.float64)
    ratio = float(sr_new) / sr_orig
    n_in = len(x)
    n_out = int(n_in * ratio)
    if ratio < 1:
        win = win * ratio
    delta = np.diff(win, append=win[-1])
    scale = min(1.0, ratio)
    time_increment = 1.0 / ratio
    num_table = 2 ** precision
    step = int(scale * num_table)
    nwin = len(win)
    y = np.zeros(n_out, np.float64)
    for t in range(n_out):
        tr = t * time_increment
        n = int(tr)
        frac = scale * (tr - n)
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        i = np.arange(min(n + 1, (nwin - off) // step))
        w = win[off + i * step] + eta * delta[off + i * step]
        acc = float(np.dot(w, x[n - i]))
        frac = scale - frac
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        k = np.arange(min(n_in - n - 1, (nwin - off) // step))
        w = win[off + k * step] + eta * delta[off + k * step]
        y[t] = acc + float(np.dot(w, x[n + 1 + k]))
    return y


def resample_rows(x, lengths, sr_orig, sr_new, filter='kaiser_best'):
    """padded x [B, T] with lengths -> (float64 [B, max n_out] zero past each row's n_out, list n_out)"""
    rows = [resample_loop(r[:n], sr_orig, sr_new, filter) for r, n in zip(x, lengths)]
    out = np.zeros((len(rows), max((len(r) for r in rows), default=0)), np.float64)
    for o, r in zip(out, rows):
        o[:len(r)] = r
    return out, [len(r) for r in rows]


def apply_bank(bank, L, M, left, x, n_out):
    """The polyphase bank as a zero-extended FIR: y[t] = sum_j bank[(t*M) % L][j] * x[(t*M) // L - left + 1 + j], x = 0 outside."""
    W = bank.shape[1]
    x = np.asarray(x, np.float64)
    xp = np.concatenate([np.zeros(W), x, np.zeros(W + M + 1)])
    y = np.zeros(n_out)
    for t in range(n_out):
        n, p = divmod(t * M, L)
        a = n - left + 1 + W
        y[t] = np.dot(bank[p], xp[a:a + W])
    return y


def eq_rms(signal, db):
    """util.eq_rms; a silent signal stays silent (the reference divides by zero)"""
    signal = np.asarray(signal, np.float64)
    ms = (signal ** 2).mean() if len(signal) else 0.0
    return signal * (10 ** (db / 20) / np.sqrt(ms)) if ms > 0 else np.zeros_like(signal)


def segment_size(max_segment):
    return -SEGMENT_MULTI * (-max(max_segment, MIN_SEGMENT) // SEGMENT_MULTI)


def segment(y, normalization_db=-30, data_augment=True, aug_gain=1.0, aug_sign=1.0, start=0, max_segment=16000, noise=None,
            augment_noise=None):
    """load_audio's steps after the resampler on one float64 row y -> float64 [segment_size(max_segment)]"""
    sig = np.asarray(y, np.float64)
    if normalization_db:
        sig = eq_rms(sig, normalization_db)
    if data_augment:
        sig = sig * float(aug_gain)
        if aug_sign < 0:
            sig = -sig
    if max_segment and len(sig) > max_segment:
        sig = sig[start:start + max_segment]
        assert len(sig) == max_segment
    out = np.zeros(segment_size(max_segment), np.float64)
    out[:len(sig)] = sig
    if augment_noise is not None:
        out = out + np.asarray(noise, np.float64) * augment_noise
    return out


def bound(ref):
    """per-row absolute bound of the GPU tests"""
    return BOUND_FACTOR * U24 * np.abs(ref).max(-1, keepdims=True)


def make_signal(rng, T, sr):
    """A few harmonics of a 90-250 Hz fundamental plus white noise, about -30 dB RMS, fp32."""
    t = np.arange(T) / sr
    f0 = rng.uniform(90, 250)
    x = sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t + rng.uniform(0, 2 * np.pi)) for k, a in enumerate((1.0, 0.6, 0.4, 0.25, 0.15)))
    x = x + 0.2 * rng.standard_normal(T)
    return (x * (10 ** (-30 / 20) / max(np.sqrt((x ** 2).mean()), 1e-30))).astype(np.float32)


def padded(rng, lengths, sr, fill=0.0, T=None):
    """rows of make_signal in one [B, T] fp32 buffer, `fill` past each row's length"""
    T = max(lengths) if T is None else T
    x = np.full((len(lengths), T), fill, np.float32)
    for r, n in zip(x, lengths):
        r[:n] = make_signal(rng, n, sr)
    return x


def length_for(n_out, sr_orig, sr_new):
    """the smallest n_in with num_out(n_in) == n_out"""
    n = max(0, int(n_out * sr_orig / sr_new) - 2)
    while num_out(n, sr_orig, sr_new) < n_out:
        n += 1
    assert num_out(n, sr_orig, sr_new) == n_out, (n_out, sr_orig, sr_new)
    return n
