"""Dense float64 numpy restatement of the banded max-sum decoder behind tdvc_viterbi_path (include/tdvc.h). Test helper: the CPU
and GPU tests take their truth from here; nothing is imported from the package.

    obs[f][j] = scale * x[f][j] + prior[j]
    t(i, j)   = max(logw[j][i - lo[j]], -jump) for lo[j] <= i < lo[j] + W, -jump outside the band      (an n x n matrix here)
    d_0 = obs[0];  d_f[j] = obs[f][j] + max_i (d_{f-1}[i] + t(i, j)), the lowest i among equal maxima
    the path ends in the lowest j among the maxima of d_{F-1} and follows the predecessors back
numpy's argmax returns the first maximum, which is both tie rules. No renormalisation: float64 does not need it at these lengths.

`transition` is the triangular pitch transition on the YIN lag lattice, from its formula; `hard_case` the two-second glide whose
fundamental fades against its second harmonic under noise.
"""
import functools
import itertools

import numpy as np


def dense_transition(logw, lo, jump, n):
    """t[j, i] in float64."""
    logw = np.asarray(logw, np.float64)
    t = np.full((n, n), -float(jump))
    cols = np.asarray(lo, np.int64)[:, None] + np.arange(logw.shape[1])[None, :]
    t[np.arange(n)[:, None], cols] = np.maximum(logw, -float(jump))
    return t


def observations(x, scale=1.0, prior=None):
    obs = float(scale) * np.asarray(x, np.float64)
    return obs if prior is None else obs + np.asarray(prior, np.float64)


def decode(x, logw, lo, scale=1.0, prior=None, jump=np.inf, t=None):
    """x [F, n] or [B, F, n] -> path int64 [F] or [B, F]. t: the dense transition when the caller already has it."""
    x = np.asarray(x)
    t = dense_transition(logw, lo, jump, x.shape[-1]) if t is None else t
    if x.ndim == 3:
        return np.stack([decode(r, logw, lo, scale, prior, jump, t) for r in x])
    F, n = x.shape
    obs = observations(x, scale, prior)
    bp = np.zeros((F, n), np.int64)
    d = obs[0]
    for f in range(1, F):
        cand = d[None, :] + t                       # [j, i]
        bp[f] = cand.argmax(1)
        d = obs[f] + cand.max(1)
    path = np.zeros(F, np.int64)
    path[-1] = d.argmax()
    for f in range(F - 1, 0, -1):
        path[f - 1] = bp[f, path[f]]
    return path


def score(path, x, logw, lo, scale=1.0, prior=None, jump=np.inf, t=None):
    """Float64 score of one path through x [F, n]."""
    x = np.asarray(x)
    obs = observations(x, scale, prior)
    t = dense_transition(logw, lo, jump, x.shape[1]) if t is None else t
    path = np.asarray(path)
    return float(obs[np.arange(len(path)), path].sum() + t[path[1:], path[:-1]].sum())


def brute_force(x, logw, lo, scale=1.0, prior=None, jump=np.inf):
    """Every one of the n^F paths scored; among equal scores the one the two tie rules select: lowest final state, then the lowest
    predecessor frame by frame from the end, i.e. the path smallest in reversed lexicographic order."""
    x = np.asarray(x)
    F, n = x.shape
    obs = observations(x, scale, prior)
    t = dense_transition(logw, lo, jump, n)
    best, best_path = None, None
    for rev in itertools.product(range(n), repeat=F):        # rev = (p_{F-1}, ..., p_0) ascending in the order the tie rules use
        p = rev[::-1]
        s = sum(obs[f, p[f]] for f in range(F)) + sum(t[p[f], p[f - 1]] for f in range(1, F))
        if best is None or s > best:
            best, best_path = s, p
    return np.array(best_path, np.int64)


def transition(tau_min, tau_max, half_width_cents=240.0):
    """(logw float64 [n, W], lo int64 [n]): c_s = 1200 log2(s + tau_min + 1), w(i, j) = max(1 - |c_i - c_j| / half_width, 0),
    logw = log w where w > 0 and -inf elsewhere; row j holds predecessors lo[j] .. lo[j] + W - 1, W the widest band, a band at the
    upper end shifted down to stay inside [0, n)."""
    n = tau_max - 1 - tau_min
    c = [1200.0 * np.log2(s + tau_min + 1) for s in range(n)]
    w = np.zeros((n, n))
    for j in range(n):
        for i in range(n):
            w[j, i] = max(1.0 - abs(c[i] - c[j]) / half_width_cents, 0.0)
    counts = (w > 0).sum(1)
    W = int(counts.max())
    lo = np.zeros(n, np.int64)
    logw = np.full((n, W), -np.inf)
    for j in range(n):
        lo[j] = min(int(np.flatnonzero(w[j] > 0)[0]), n - W)
        for k in range(W):
            if w[j, lo[j] + k] > 0:
                logw[j, k] = np.log(w[j, lo[j] + k])
    return logw, lo


def octave_prior(tau_min, n, octave_cost=1.0):
    lag = np.arange(n, dtype=np.float64) + tau_min + 1
    return -octave_cost * np.log2(lag / (tau_min + 1))


HARD_T, HARD_SR, HARD_HOP = 32000, 16000, 64


@functools.lru_cache(maxsize=None)
def hard_case():
    """(x float32 [T], true pitch per frame k = f[min(64 k, T - 1)] for k = 0 .. T // 64)."""
    T, sr = HARD_T, HARD_SR
    rng = np.random.default_rng(7)
    t = np.arange(T) / sr
    f = 110 + 60 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f) / sr
    a1 = 0.15 + 0.85 * (np.sin(2 * np.pi * 1.3 * t) > 0)
    x = a1 * np.sin(ph) + np.sin(2 * ph + 0.3) + 0.4 * np.sin(3 * ph + 1.0) + 0.25 * rng.standard_normal(T)
    x = (x * (0.03 / np.sqrt(np.mean(x * x)))).astype(np.float32)
    k = np.minimum(HARD_HOP * np.arange(T // HARD_HOP + 1), T - 1)
    return x, f[k]
