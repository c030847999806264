"""The reflect fold of conv_lean_kernel (conv_lean.hip: fold_taps and the three fold loops): the INPUT-GRAD of a reflect-padded conv
adds the gradient of the mirrored halo columns to the columns they mirror, in a second pass over the staged gradient tile. The pass
runs over the LIVE taps of each 16-column sub-tile only, and on the 16-row tiles over the sub-tiles that hold mirrored columns only;
the fold as it was (every tap, every sub-tile of the 16-row tiles) stays behind tdvc_debug_knob(10, 1).

A step the live range leaves out multiplied zeros (the staging writes zeros outside [0, T)) into a sum that started at +0, and the
steps that stay keep their operands and their order, so no bit moves. Each GPU case, at each of its tiles, checks

  * both float64 bars of the lean edge suite (edge_support.assert_bars; the rules are in test_lean_conv_edges_gpu.py's docstring) on the
    forward and the input-grad, with the knob off and on,
  * the instance of each call by trace: the name the tile table of lean_cases.py gives, unchanged by the live ranges,
  * torch.equal between knob 10 off (live taps) and on (every tap) on dx (and y; dgb with the FiLM epilogue),
  * and all of it once more with NaN bit patterns in the LDS of every CU in front of every call: a live tap left out breaks the bars
    and the equality, a read of a column that was never staged turns the result into NaN.

THE LIVE RANGE (restated in fold_taps below and checked against brute force on the CPU). At tap j the mirrored column u reads the
staged tile at position base - u + j * d, with base = -pad on the left side (mirrored columns 1 .. mirror) and 2 (T - 1) - pad on the
right side (T - 1 - mirror .. T - 2); pad is the input-grad's own, (K - 1) d - pad of the conv. For the mirrored columns [ua, ub] of
a sub-tile the taps that can read inside [0, T) are ceil((ua - base) / d) .. floor((T - 1 - base + ub) / d), clamped to [0, K - 1].
The kernel divides in fp32, (n + 0.5) * (1 / d) with n <= K * d: test_live_range_in_fp32_equals_the_integer_one evaluates that
expression in numpy float32 for every d the trunk has and beyond.

ROWS, all reflect, pre = 1 (LeakyReLU mask epilogue), add = True, B = 2:
  SMALL   tiles 3 and 6 (16 x 64, 32 x 64: the per-tap ring). K = 11 d = 5 (pad 25: two sub-tiles per side, the second with 2 live
          taps of 11), K = 11 d = 1, K = 7 d = 3, K = 3 d = 5; 4 and 36 channels (a 32 + 4 chunk split: the fold runs per chunk);
          T = 52 (both mirrors in one tile), 50 (scalar epilogue), 72 (the right mirror across two tiles), 132 (mirrors in different tiles).
  WIDE16  tile 0 (16 x 256, the plain loop): the same kernels at 16 channels, T = 84 and 260.
  ROWS    tiles 1, 5, 2 (32 / 48 / 64 x 256: the double-buffered loop into a temporary accumulator): 32, 40 (a partly filled 48- and
          64-row tile) and 64 channels, K = 11 d = 5 and K = 7 d = 1, T = 84 (both mirrors in one block, on different waves) and 260
          (the right mirror spans two blocks, the second 4 columns wide).
  FILM    K = 3 on tile 6 with the FiLM prologue / epilogue pair (film=True stands in place of pre = 1, as Edge requires).
"""
import contextlib

import numpy as np
import pytest
import torch

from conv_edge import Edge, _g
from edge_support import assert_bars, forced_tile, lib, poison_lds
from lean_cases import GENERIC, LEAN_CFG, expected_instance, lean_call, tile_rows_cols

KERNELS = ((11, 5), (11, 1), (7, 3), (3, 5))      # (K, dilation); 'same' padding (K - 1) d / 2
OPTS = dict(B=2, pre=1, add=True)


def _row(tag, c, k, d, T, opts=OPTS):
    return _g(f'fold_{tag}_c{c}_k{k}_d{d}_T{T}', c, c, k, (k - 1) * d // 2, d, True, T), opts


SMALL = [_row('small', c, k, d, T) for k, d in KERNELS for c in (4, 36) for T in (52, 50, 72, 132)]
WIDE16 = [_row('wide16', 16, k, d, T) for k, d in KERNELS for T in (84, 260)]
ROWS = [_row('rows', c, k, d, T) for k, d in ((11, 5), (7, 1)) for c in (32, 40, 64) for T in (84, 260)]
FILM = [_row('film', 16, 3, 1, 132, dict(B=2, film=True, add=True))]
# (tiles, rows)
GROUPS = [((3, 6), SMALL), ((0,), WIDE16), ((1, 5, 2), ROWS), ((6,), FILM)]
GPU_CASES = [(cfg, row) for tiles, rows in GROUPS for row in rows for cfg in tiles]
GPU_IDS = [f'tile{cfg}_' + 'x'.join(map(str, LEAN_CFG[cfg])) + '-' + row[0][0] for cfg, row in GPU_CASES]


# ------------------------------------------------------------------------------------------------ the live range (CPU)
def mirrored(side, ca, mirror, T):
    """First and last mirrored column of the 16-column sub-tile that starts at `ca` (first > last: none)."""
    if side == 0:
        return max(ca, 1), min(ca + 15, mirror, T - 1)
    return max(ca, T - 1 - mirror, 0), min(ca + 15, T - 2)


def fold_base(side, pad, T):
    return -pad if side == 0 else 2 * (T - 1) - pad


def fold_taps(side, ca, K, d, pad, mirror, T, div=None):
    """conv_lean.hip's fold_taps: (jlo, jhi), or None where the sub-tile is skipped. `div(n)`: floor(n / d) for 0 <= n <= K * d."""
    div = div or (lambda n: n // d)
    ua, ub = mirrored(side, ca, mirror, T)
    base = fold_base(side, pad, T)
    nlo, nhi, kd = ua - base, T - 1 - base + ub, (K - 1) * d
    jlo = 0 if nlo <= 0 else div(min(nlo, kd + d) + d - 1)
    jhi = -1 if nhi < 0 else div(min(nhi, kd))
    return (jlo, jhi) if ua <= ub and jlo <= jhi else None


def live(side, u, j, d, pad, T):
    return 0 <= fold_base(side, pad, T) - u + j * d < T


def sub_tile_starts(side, mirror, T, step=16):
    """Starts of the 16-column sub-tiles that hold a mirrored column. The kernel's are multiples of 16; step = 1 gives every start the
    formula can be asked about."""
    lo, hi = (1, min(mirror, T - 1)) if side == 0 else (max(T - 1 - mirror, 0), T - 2)
    return [ca for ca in range(-16 + step, T + 16, step) if ca <= hi and ca + 15 >= lo]


def test_live_range_against_brute_force():
    """CPU. K in {3, 5, 7, 11}, d in {1, 3, 5}, 'same' padding, both sides, every sub-tile start that can hold a mirrored column (the
    kernel's multiples of 16 and every start between them: with multiples of 16 alone the first mirrored column is 1 or 16, and
    pad + 1, pad + 16 are multiples of no d > 1 here), six sequence lengths: the range contains every live tap of every mirrored
    column, its first tap is live for the first mirrored column and its last tap for the last one, and a sub-tile is skipped only
    where no tap is live. Both divisions are met exact and inexact for every d > 1: pad + u a multiple of d for the first mirrored
    column of the left side (the ceil), pad + u - (T - 1) for the last one of the right side (the floor)."""
    exact, inexact, second = set(), set(), False
    for K in (3, 5, 7, 11):
        for d in (1, 3, 5):
            pad = (K - 1) * d // 2
            for T in (50, 52, 72, 84, 132, 260):
                for side in (0, 1):
                    assert sub_tile_starts(side, pad, T)
                    for ca in sub_tile_starts(side, pad, T, step=1):
                        ua, ub = mirrored(side, ca, pad, T)
                        assert ua <= ub
                        alive = {j for j in range(K) for u in range(ua, ub + 1) if live(side, u, j, d, pad, T)}
                        r = fold_taps(side, ca, K, d, pad, pad, T)
                        what = (K, d, T, side, ca, r, sorted(alive))
                        if r is None:
                            assert not alive, what
                            continue
                        jlo, jhi = r
                        assert 0 <= jlo <= jhi <= K - 1, what
                        assert alive and min(alive) == jlo and max(alive) == jhi, what
                        assert live(side, ua, jlo, d, pad, T) and live(side, ub, jhi, d, pad, T), what
                        assert jhi - jlo + 1 <= max((K - 1) // 2, 1), what      # at most (K - 1) / 2 of the K taps per side
                        (exact if (pad + ua if side == 0 else pad + ub - (T - 1)) % d == 0 else inexact).add((side, d))
                        second |= (K, d, side, ca, r) == (11, 5, 0, 16, (9, 10))      # second sub-tile of pad 25: 2 live taps of 11
    assert exact == {(s, d) for s in (0, 1) for d in (1, 3, 5)} and inexact == {(s, d) for s in (0, 1) for d in (3, 5)} and second


def test_live_range_without_same_padding():
    """CPU. Nothing in the range assumes 2 pad = (K - 1) d: with a shorter or longer input-grad pad than the mirror it is still the
    hull of the live taps, clamped to [0, K - 1], and empty where no tap is live."""
    empty = 0
    for K, d, pad, mirror in ((7, 3, 4, 9), (7, 3, 14, 9), (11, 5, 0, 25), (3, 1, 2, 1), (5, 5, 20, 3), (3, 1, 0, 20)):
        for T in (50, 72, 132):
            for side in (0, 1):
                for ca in sub_tile_starts(side, mirror, T):
                    ua, ub = mirrored(side, ca, mirror, T)
                    alive = {j for j in range(K) for u in range(ua, ub + 1) if live(side, u, j, d, pad, T)}
                    r = fold_taps(side, ca, K, d, pad, mirror, T)
                    assert (r is None) == (not alive), (K, d, pad, mirror, T, side, ca, r)
                    empty += r is None
                    if r:
                        assert r == (min(alive), max(alive)), (K, d, pad, mirror, T, side, ca, r, sorted(alive))
    assert empty > 0


def test_live_range_in_fp32_equals_the_integer_one():
    """CPU. The kernel's division, (int)((n + 0.5f) * (1.0f / d)) in fp32, is floor(n / d) for every numerator it meets (0 .. K d)."""
    f = np.float32
    for d in range(1, 65):
        inv = f(1.0) / f(d)
        for n in range(0, 64 * d + d):
            assert int((f(n) + f(0.5)) * inv) == n // d, (n, d)
    for K, d in KERNELS:
        pad = (K - 1) * d // 2
        inv = f(1.0) / f(d)
        for T in (50, 52, 260):
            for side in (0, 1):
                for ca in sub_tile_starts(side, pad, T):
                    assert fold_taps(side, ca, K, d, pad, pad, T, div=lambda n: int((f(n) + f(0.5)) * inv)) == fold_taps(side, ca, K, d, pad, pad, T)


def test_fold_tables_stay_on_the_lean_kernel():
    """CPU. Every GPU row runs on the lean kernel at each of its tiles, both ways, with the mirror of an input-grad; the 256-column
    rows are long enough for those tiles; on the small tiles K = 11, d = 5 folds two sub-tiles per side and the 36-channel rows
    split into 32 + 4."""
    for cfg, (geom, opts) in GPU_CASES:
        assert tile_rows_cols(cfg)[1] == 64 or geom[-1] > 80, (cfg, geom[0])
        for what in ('fwd', 'dgrad'):
            assert expected_instance(geom, opts, what, cfg) != GENERIC, (geom[0], what, cfg)
        red, k, d, pad, mirror, _, _ = lean_call(geom, opts, 'dgrad')
        assert mirror == pad == (k - 1) * d // 2 and mirror > 0, geom[0]
    assert len(sub_tile_starts(0, 25, 52)) == 2 and len(sub_tile_starts(1, 25, 132)) == 3


# ------------------------------------------------------------------------------------------------ GPU
@contextlib.contextmanager
def full_fold(on):
    """tdvc_debug_knob(10, 1): the reflect fold runs every tap and, on the 16-row tiles, every sub-tile."""
    lib().tdvc_debug_knob(10, int(on))
    try:
        yield
    finally:
        lib().tdvc_debug_knob(10, 0)


def run(row, dev, cfg, knob, poison):
    """One forward and one input-grad of a fresh Edge -> Edge."""
    e = Edge(row[0], dev, **{**dict(wt=True, nan_spare=True), **row[1]})

    def calls():
        if poison:
            poison_lds(dev)
        res = e.fwd()
        if poison:
            poison_lds(dev)
        res.update(e.dgrad())
        return res
    with full_fold(knob):
        res = forced_tile(cfg, calls)
    assert_bars(res, f'{e.geom[0]} tile {cfg} ' + ('every tap' if knob else 'live taps') + (' (poisoned LDS)' if poison else ''))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,row', GPU_CASES, ids=GPU_IDS)
def test_live_taps_equal_every_tap(cfg, row, dev):
    name = row[0][0]
    for poison in (False, True):
        lean, full = run(row, dev, cfg, 0, poison), run(row, dev, cfg, 1, poison)
        for e in (lean, full):
            for what in ('fwd', 'dgrad'):
                assert e.names[what] == {expected_instance(row[0], row[1], what, cfg)}, (name, what, sorted(e.names[what]))
        for key in ('yv', 'dxv') + (('dgbv',) if lean.film else ()):
            a, b = getattr(lean, key), getattr(full, key)
            assert torch.equal(a, b), f'{name} tile {cfg}' + (' (poisoned LDS)' if poison else '') + \
                f': {key[:-1]} differs between the live taps and every tap in {int((a != b).sum())} elements'
            assert float(a.abs().max()) > 0
