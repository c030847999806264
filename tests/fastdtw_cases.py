"""The inputs shared by tests/test_fastdtw_cpu.py (which proves they are fit for exact comparison) and tests/test_fastdtw_gpu.py
(which runs them): lattice pairs for tdvc_fastdtw and the real-valued pairs, each with its float64 reference computed once.

Lattices hold integers |v| <= V = 3, so level L of the fp32 pyramid holds multiples of 2^-L and every fp32 distance is exact when
    'l1'          log2(2 V D) + L <= 24 bits
    'sq', 'l2'    2 (log2(2 V) + L) + log2(D) <= 24 bits   ('l2' only with D = 1, where sqrt(e^2) = |e| is exact)
with L the deepest level of the pair. D and the metric of each case are chosen under that budget; deep pyramids use 'l1'.
"""
import functools
import math

import numpy as np

import dtw_ref as DR
import fastdtw_ref as FR

V = 3
#        name           N      M      D   B  metric radius  kind
EXACT = {
    '1x1':          (1,     1,     1,  1, 'l2', 1, 'random'),
    '1x7':          (1,     7,     1,  5, 'l2', 1, 'random'),
    '7x1':          (7,     1,     1,  5, 'l2', 1, 'random'),
    '2x500':        (2,     500,   1,  1, 'l2', 1, 'random'),       # the base case at level 0, the other side long
    '500x2':        (500,   2,     1,  1, 'l2', 1, 'random'),
    '3x3':          (3,     3,     1,  5, 'l2', 1, 'random'),       # the first real recursion
    '4x4':          (4,     4,     1,  5, 'l2', 1, 'random'),
    '63x64':        (63,    64,    1,  5, 'l2', 1, 'random'),
    '64x65':        (64,    65,    1,  5, 'l2', 1, 'random'),
    '65x63':        (65,    63,    1,  5, 'l2', 1, 'random'),
    '65x63d64':     (65,    63,    64, 5, 'sq', 1, 'random'),
    '255x256':      (255,   256,   25, 1, 'sq', 1, 'random'),       # odd and even sizes at different levels
    '256x257':      (256,   257,   25, 5, 'l1', 1, 'random'),
    '257x255':      (257,   255,   64, 1, 'l1', 2, 'random'),
    'plateau':      (101,   700,   1,  1, 'l1', 1, 'plateau'),      # one row of x against 500 equal frames of y: rows wider than 256
    'plateau_t':    (700,   101,   1,  1, 'l1', 1, 'plateau_t'),    # the transposed pair: a long vertical run
    '40x1500':      (40,    1500,  1,  1, 'l2', 1, 'random'),
    '1500x40':      (1500,  40,    1,  1, 'l2', 1, 'random'),
    '1024x1024':    (1024,  1024,  1,  1, 'l2', 1, 'random'),
    '16384x16001':  (16384, 16001, 1,  1, 'l1', 1, 'random'),
    'identical':    (130,   130,   25, 1, 'sq', 1, 'identical'),    # all ties on the diagonal
    'constant':     (100,   77,    1,  5, 'l2', 1, 'constant'),     # all ties everywhere
    '65x63r2':      (65,    63,    1,  5, 'l2', 2, 'random'),
    '129x200r3':    (129,   200,   25, 1, 'l1', 3, 'random'),
    '300x280r8':    (300,   280,   1,  1, 'l1', 8, 'random'),
    '40x300r8':     (40,    300,   25, 5, 'sq', 8, 'random'),
    'constant_r8':  (90,    150,   1,  1, 'l1', 8, 'constant'),
}
BIG = ('16384x16001',)                                              # reference through the closed-form window (test_fastdtw_cpu proves it equal)


def pair_lengths(N, M, B):
    """Full, empty x, one frame of x, one frame of y, empty y."""
    if B == 1:
        return [N], [M]
    return [N, 0, 1, max(1, N // 2), N], [M, M, max(1, M // 3), 1, 0]


def depth(n, m, radius):
    """The deepest level of the pyramid of an n x m pair (0 = the pair itself is solved in full)."""
    L = 0
    while n >= radius + 2 and m >= radius + 2:
        n, m, L = n // 2, m // 2, L + 1
    return L


def bits_needed(D, metric, L):
    if metric == 'l1':
        return math.log2(2 * V * D) + L
    return 2 * (math.log2(2 * V) + L) + math.log2(D)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """dict(x [B, N, D], y [B, M, D] fp32 with NaN past the lengths, n, m, metric, radius, want = per-pair references or None)."""
    N, M, D, B, metric, radius, kind = EXACT[name]
    rng = np.random.default_rng(sorted(EXACT).index(name) + 11)
    x = rng.integers(-V, V + 1, (B, N, D)).astype(np.float32)
    y = rng.integers(-V, V + 1, (B, M, D)).astype(np.float32)
    if kind in ('plateau', 'plateau_t'):
        short, long_ = (x, y) if kind == 'plateau' else (y, x)
        ns, nl = short.shape[1], long_.shape[1]
        short[:] = np.where(np.arange(ns) < ns // 2, -V, V)[None, :, None]
        short[:, ns // 2] = 0
        long_[:] = np.where(np.arange(nl) < 100, -V, V)[None, :, None]
        long_[:, 100:nl - 100] = 0
    elif kind == 'identical':
        y = x.copy()
    elif kind == 'constant':
        x[:], y[:] = 1, 1
    n, m = pair_lengths(N, M, B)
    want = []
    for b in range(B):
        want.append(FR.fastdtw(x[b, :n[b]], y[b, :m[b]], radius, metric, 'closed' if name in BIG else 'literal') if n[b] and m[b] else None)
        x[b, n[b]:] = np.nan
        y[b, m[b]:] = np.nan
    return dict(x=x, y=y, n=np.asarray(n, np.int32), m=np.asarray(m, np.int32), metric=metric, radius=radius, want=want)


# real-valued pairs (dtw_ref.warped_pair, D = 25, 'l2'): the device computes every distance within eps relative
D_REAL = 25
EPS = (D_REAL + 2) * 2.0 ** -24
IDENTITY = [(60, 45, 0), (60, 45, 1), (60, 45, 2), (200, 150, 0), (200, 150, 1), (200, 150, 2)]      # (n, m, seed - n - m)
LOOSE = (900, 700, 0)


@functools.lru_cache(maxsize=None)
def real_case(n, m, k):
    x, y = DR.warped_pair(np.random.default_rng(n + m + k), n, m, D_REAL)
    return x, y, FR.fastdtw(x, y, 1, 'l2')


def margin_ratio(want):
    """min over levels of (smallest back-traced margin) / (4 * 2 eps cost of that level): above 1 the device must take the same path."""
    return min(lv['margin'] / (4 * 2 * EPS * lv['cost']) for lv in want['levels'])
