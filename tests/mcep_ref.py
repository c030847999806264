"""Float64 numpy restatement of the mel-cepstrum behind tdvc_sp2mc and evaluate.mel_cepstrum (include/tdvc.h). Test helper.

    c = irfft(log(max(P, floor)));  c[0] /= 2;  mc = freqt(c[0 .. n_fft/2], order, alpha)
    freqt (SPTK's frequency transform): b = 1 - alpha^2, g = 0; for i = -m1 .. 0:
        d = g;  g[0] = c[-i] + alpha d[0];  g[1] = b d[0] + alpha d[1];  g[j] = d[j-1] + alpha (d[j] - g[j-1]),  j >= 2

`warped_spectrum` is the analytic check: a spectrum whose mel-cepstrum is known in closed form.
"""
import numpy as np


def freqt(c, order, alpha):
    """c [m1 + 1] -> [order + 1], one vector, written as the recursion reads."""
    c = np.asarray(c, np.float64)
    m1 = len(c) - 1
    b = 1.0 - alpha * alpha
    g = np.zeros(order + 1)
    for i in range(-m1, 1):
        d = g.copy()
        g[0] = c[-i] + alpha * d[0]
        if order >= 1:
            g[1] = b * d[0] + alpha * d[1]
        for j in range(2, order + 1):
            g[j] = d[j - 1] + alpha * (d[j] - g[j - 1])
    return g


def sp2mc(power, order, alpha, floor=0.0):
    """power [..., n_fft/2 + 1] -> float64 [..., order + 1]."""
    p = np.asarray(power, np.float64)
    nb = p.shape[-1]
    lp = np.log(np.maximum(p, floor)) if floor > 0 else np.log(p)
    c = np.fft.irfft(lp, n=2 * (nb - 1), axis=-1)[..., :nb].copy()
    c[..., 0] *= 0.5
    flat = c.reshape(-1, nb)
    return np.stack([freqt(r, order, alpha) for r in flat]).reshape(p.shape[:-1] + (order + 1,))


def warped_spectrum(m, n_fft, alpha):
    """Power spectrum on the n_fft/2 + 1 bins with log P(w) = 2 sum_k m[k] cos(k w~), w~ = w + 2 atan(alpha sin w / (1 - alpha cos w)):
    the spectrum whose mel-cepstrum (c[0] halved, as above) is m."""
    w = 2 * np.pi * np.arange(n_fft // 2 + 1) / n_fft
    wt = w + 2 * np.arctan(alpha * np.sin(w) / (1 - alpha * np.cos(w)))
    k = np.arange(len(m))
    return np.exp(2 * (np.asarray(m, np.float64)[None, :] * np.cos(k[None, :] * wt[:, None])).sum(1))


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)


def stft_power(x, n_fft, hop, dtype):
    """x [T] -> power [1 + T // hop, n_fft/2 + 1] in `dtype`: centred frames (reflect padding of n_fft/2), periodic Hann, the direct
    windowed DFT as one matrix product against the cos / -sin basis rounded to `dtype`, |.|^2. The formulation of the device path."""
    x = np.asarray(x, dtype)
    F = n_fft // 2 + 1
    xp = np.pad(x, n_fft // 2, mode='reflect')
    nfr = 1 + len(x) // hop
    frames = np.stack([xp[f * hop:f * hop + n_fft] for f in range(nfr)])
    ang = 2 * np.pi * np.outer(np.arange(F), np.arange(n_fft)) / n_fft
    re = (np.cos(ang) * hann(n_fft)).astype(dtype)
    im = (-np.sin(ang) * hann(n_fft)).astype(dtype)
    a, b = frames @ re.T, frames @ im.T
    return a * a + b * b


def mel_cepstrum(x, n_fft, hop, order, alpha, floor, dtype=np.float64):
    """The whole chain from one fp32 signal [T]: the front end in `dtype`, everything from the logarithm on in float64 (as the
    device does) -> float64 [n_frames, order + 1]."""
    return sp2mc(stft_power(x, n_fft, hop, dtype), order, alpha, floor)
