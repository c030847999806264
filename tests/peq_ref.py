"""Plain numpy restatement of the random parametric EQ behind tdvc_peq_sos / tdvc_sos_filter (include/tdvc.h), in a caller-chosen
dtype. Test helper: the GPU tests take their float64 truth from here, and tests/golden/peq.npz pins it to the reference's own
`random_eq` + `eq_rms_signals` (tools/make_golden_peq.py). No scipy: the GPU tests must not need it.

Written from the RBJ cookbook formulae, as the reference's `params2sos` evaluates them:
    g = 10^(G/20), A = max(0, sqrt(g)), w = 2*pi*max(fc, 2)/fs
    low shelf (band 0), high shelf (last band): beta = sin(w)*sqrt(A)/Q, the cookbook's shelf polynomials in A, cos(w), beta
    peaking (the bands between):                alpha = sin(w)/(2Q); b = (1 + alpha*A, -2cos(w), 1 - alpha*A), a = (1 + alpha/A, -2cos(w), 1 - alpha/A)
    every section divided by its a0; rows are b0 b1 b2 1 a1 a2 (scipy's sos layout)
    cascade: each section in transposed direct form II from a zero state, y = b0*x + s1; s1 = b1*x - a1*y + s2; s2 = b2*x - a2*y
    RMS match: y * rms(x) / (rms(y) + 1e-8)
With dtype=float32 every coefficient, state and product is rounded to fp32: what a naive fp32 port computes.
"""
import functools
import json
import os

import numpy as np

from yin_ref import make_signal  # noqa: F401  (speech-like test signal; re-exported)

QMIN, QMAX = 2.0, 5.0
FC = np.exp(np.linspace(np.log(60), np.log(7600), 10))      # the reference's ten log-spaced centres
SR = 16000
U24 = 2.0 ** -24
BOUND_FACTOR = 4.0                                            # |y - truth| <= 4 * 2^-24 * max|truth_row|


def q_of_z(z):
    return QMIN * (QMAX / QMIN) ** np.asarray(z)


def _section(kind, G, fc, Q, fs, dt):
    G, fc, Q, fs = dt(G), dt(fc), dt(Q), dt(fs)
    one, two = dt(1), dt(2)
    g = np.power(dt(10), G / dt(20))
    A = np.maximum(dt(0), np.sqrt(g))
    w = (two * dt(np.pi) * np.maximum(fc, two)) / fs
    co, si = np.cos(w), np.sin(w)
    if kind == 'peak':
        alpha = si / (Q * two)
        c2 = -two * co
        b0, b1, b2 = one + alpha * A, c2, one - alpha * A
        a0, a1, a2 = one + alpha / A, c2, one - alpha / A
    else:
        am, ap = A - one, A + one
        beta = si * np.sqrt(A) / Q
        amc = am * co
        if kind == 'low':
            b0, b1, b2 = A * (ap - amc + beta), A * two * (am - ap * co), A * (ap - amc - beta)
            a0, a1, a2 = ap + amc + beta, -two * (am + ap * co), ap + amc - beta
        else:
            b0, b1, b2 = A * (ap + amc + beta), A * -two * (am + ap * co), A * (ap + amc - beta)
            a0, a1, a2 = ap - amc + beta, two * (am - ap * co), ap - amc - beta
    return np.array([b0 / a0, b1 / a0, b2 / a0, one, a1 / a0, a2 / a0], dtype=dt)


def peq_sos(G, Q, fc=FC, fs=SR, dtype=np.float64):
    """G, Q [..., n] -> sos [..., n, 6]: band 0 low shelf, band n-1 high shelf, peaking between."""
    G, Q = np.asarray(G), np.asarray(Q)
    n = G.shape[-1]
    assert n >= 2 and Q.shape == G.shape and len(fc) == n
    out = np.empty(G.shape + (6,), dtype)
    for idx in np.ndindex(*G.shape):
        k = idx[-1]
        kind = 'low' if k == 0 else 'high' if k == n - 1 else 'peak'
        out[idx] = _section(kind, G[idx], fc[k], Q[idx], fs, dtype)
    return out


def sosfilt(sos, x, dtype=np.float64):
    """sos [S, 6], x [T] -> y [T]: the sections one after another, each a plain sequential recurrence in `dtype`."""
    dt = dtype
    y = np.asarray(x).astype(dt)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos).astype(dt):
        assert a0 == 1
        if dt is np.float64:      # python floats are IEEE doubles and several times faster than numpy scalars
            b0, b1, b2, a1, a2 = float(b0), float(b1), float(b2), float(a1), float(a2)
            s1 = s2 = 0.0
            seq = y.tolist()
        else:
            s1 = s2 = dt(0)
            seq = list(y)
        out = []
        for v in seq:
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            out.append(o)
        y = np.array(out, dtype=dt)
    return y


def sosfilt_rows(sos, x, dtype=np.float64):
    """sos [B, S, 6], x [B, T] -> [B, T]"""
    return np.stack([sosfilt(s, r, dtype) for s, r in zip(sos, x)]) if len(x) else np.zeros(np.shape(x), dtype)


def match_rms(y, x):
    """rows of y scaled to the RMS of the rows of x (util.eq_rms_signals), float64."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    rms_y = np.sqrt((y ** 2).mean(-1, keepdims=True))
    rms_x = np.sqrt((x ** 2).mean(-1, keepdims=True))
    return y * rms_x / (rms_y + 1e-8)


def random_eq(x, G, z, fs=SR, match=True):
    """x [B, T] fp32, G, z [B, 10] -> (sos, y) in float64: what the reference's corrupt_audio returns for these draws."""
    sos = peq_sos(G, q_of_z(z), FC, fs)
    y = sosfilt_rows(sos, x)
    return sos, (match_rms(y, x) if match else y)


def bound(ref):
    """per-row absolute bound of the GPU tests: the float64 result rounded once to fp32, x4 for another operation order."""
    return BOUND_FACTOR * U24 * np.abs(ref).max(-1, keepdims=True)


# ---- the fixture (tests/golden/peq.npz + peq.json, tools/make_golden_peq.py) and the cases of the GPU tests, computed once
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LONG_T, LONG_SEED = 71680, 4321
ODD_B, ODD_T, ODD_SEED, ODD_PITCH = 3, 4037, 77, 4100      # `odd`: rows of a wider buffer, ODD_PITCH floats apart
SPEECH_LIKE = ('speech', 'boost', 'cut', 'mixed_rows', 'odd', 'long')
CASES = SPEECH_LIKE + ('step', 'impulse', 'short1', 'short5', 'silence')


@functools.lru_cache(maxsize=None)
def fixture():
    meta = json.load(open(os.path.join(GOLDEN, 'peq.json')))
    return meta, np.load(os.path.join(GOLDEN, 'peq.npz'))


def _probe_ok(x, g, name):
    return float(np.abs(x.reshape(-1)[g[f'{name}_probe_idx']] - g[f'{name}_probe_val']).max()) <= 1e-6


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x fp32 [B, T], G fp32 [B, 10], Q fp32 [B, 10]): the kernel's inputs for a case. The draws are rounded to fp32 here, as
    tdvc_peq_sos takes them, so the truth and the kernel start from the same numbers."""
    _, g = fixture()
    sp = g['speech_signal']
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    full = lambda B, G, Q: (np.full((B, 10), G, np.float32), np.full((B, 10), Q, np.float32))
    if name == 'speech':
        return sp, f32(g['speech_G']), f32(q_of_z(g['speech_z']))
    if name == 'boost':
        return (sp[:1],) + full(1, 12.0, 5.0)
    if name == 'cut':
        return (sp[1:],) + full(1, -12.0, 2.0)
    if name == 'mixed_rows':
        G, Q = full(2, 12.0, 5.0)
        G[1], Q[1] = -12.0, 2.0
        return sp, G, Q
    if name in ('odd', 'long'):
        B, T, seed = (ODD_B, ODD_T, ODD_SEED) if name == 'odd' else (1, LONG_T, LONG_SEED)
        rng = np.random.default_rng(seed)
        x = np.stack([make_signal(rng, T, SR) for _ in range(B)])
        assert _probe_ok(x, g, name), f'{name}: the regenerated signal differs from the probe in the fixture'
        return x, f32(rng.uniform(-12, 12, (B, 10))), f32(q_of_z(rng.uniform(0, 1, (B, 10))))
    rng = np.random.default_rng({'step': 1, 'impulse': 2, 'short1': 3, 'short5': 4, 'silence': 5}[name])
    T = {'step': 4096, 'impulse': 4096, 'short1': 1, 'short5': 5, 'silence': 2000}[name]
    x = np.zeros((1, T), np.float32)
    if name == 'step':
        x[:] = 1.0
    elif name == 'impulse':
        x[0, 0] = x[0, 2049] = 1.0
    elif name.startswith('short'):
        x[:] = (0.03 * rng.standard_normal((1, T))).astype(np.float32)
    return x, f32(rng.uniform(-12, 12, (1, 10))), f32(q_of_z(rng.uniform(0, 1, (1, 10))))


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict(x, G, Q (fp32, as the kernel gets them), sos, y = plain cascade, y_rms = RMS-matched; float64)."""
    x, G, Q = inputs(name)
    sos = peq_sos(G.astype(np.float64), Q.astype(np.float64))
    y = sosfilt_rows(sos, x)
    return dict(x=x, G=G, Q=Q, sos=sos, y=y, y_rms=match_rms(y, x))


@functools.lru_cache(maxsize=None)
def fp32_run(name):
    """The same cascade with fp32 coefficients and fp32 state, on the case's input: [B, T] float32."""
    t = truth(name)
    return sosfilt_rows(t['sos'].astype(np.float32), t['x'], np.float32)
