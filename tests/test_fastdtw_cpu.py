"""No GPU: what tests/test_fastdtw_gpu.py relies on, proved on the host.

1. Window: the closed form the kernel uses equals the package's set-and-scan construction at every level of random lattice pairs
   (radius 1, 2, 3; sides of 1..5 frames, powers of two +- 1, n >> m and m >> n), and a window has at most 4 r + 2 rows on an
   anti-diagonal (the bound csrc/eval_fastdtw.hip derives and lays its lanes out by).
2. Ordering: fastdtw >= exact DTW on every case and > on some: the reference is not secretly exact.
3. Exactness budget: on every lattice case of the GPU suite the fp32 and the float64 evaluation of every window distance at every
   level are equal, and the pyramid itself is exact in fp32.
4. Workspace: tdvc_fastdtw_workspace covers the cells, rows and diagonals the reference needs on staircase, L-shaped and diagonal paths.
5. Symbols and refusals through the raw C ABI with a null stream (nothing is launched, the pointers are never dereferenced).
6. Margins: the real-valued GPU cases satisfy the condition under which path identity may be asserted.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dtw_ref as DR
import fastdtw_cases as FC
import fastdtw_ref as FR
from common import ROOT, pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


def lattice(rng, n, m, D=1):
    return rng.integers(-3, 4, (n, D)).astype(np.float32), rng.integers(-3, 4, (m, D)).astype(np.float32)


def window_sizes():
    rng = np.random.default_rng(5)
    sizes = [(n, m) for n in (1, 2, 3, 4, 5) for m in (1, 2, 3, 4, 5, 9, 33)] + [(m, n) for n in (1, 2, 3, 4, 5) for m in (9, 33)]
    sizes += [(a, b) for a in (15, 16, 17, 31, 33, 63, 65) for b in (16, 17, 64, 63)]
    sizes += [(200, 7), (7, 200), (150, 12), (12, 150), (129, 40), (40, 129)]
    sizes += [tuple(int(v) for v in rng.integers(1, 80, 2)) for _ in range(40)]
    return sizes


@pytest.mark.parametrize('radius', [1, 2, 3])
def test_closed_form_window_equals_the_literal_construction(radius):
    rng = np.random.default_rng(radius)
    levels = 0
    for n, m in window_sizes():
        x, y = lattice(rng, n, m)
        if (n + m) % 3 == 0:                                          # runs of equal frames: long horizontal and vertical stretches
            x, y = np.repeat(x, 3, 0)[:n], np.repeat(y, 5, 0)[:m]
        w = FR.fastdtw(x, y, radius, 'l1')
        for fine, coarse in zip(w['levels'][:-1], w['levels'][1:]):
            lit = FR.literal_window(coarse['path'], fine['n'], fine['m'], radius)
            assert lit == FR.closed_window(coarse['path'], fine['n'], fine['m'], radius), (n, m, fine['n'], fine['m'])
            assert FR.max_rows_on_a_diagonal(lit) <= 4 * radius + 2
            assert fine['cells'] == sum(map(len, lit)) <= (4 * radius + 2) * (fine['n'] + fine['m'] - 1)
            levels += 1
        assert DR.is_warping_path(w['path'], n, m) and w['length'] == len(w['path'])
        assert w['cost'] == DR.score(w['path'], x, y, 'l1')
    assert levels > 150


def test_fastdtw_is_never_below_exact_dtw_and_sometimes_above():
    rng = np.random.default_rng(9)
    above = total = 0
    for _ in range(60):
        n, m = (int(v) for v in rng.integers(1, 70, 2))
        x, y = lattice(rng, n, m)
        for radius in (1, 3):
            f, e = FR.fastdtw(x, y, radius, 'l1')['cost'], DR.dtw(x, y, 'l1')['cost']
            assert f >= e
            above, total = above + (f > e), total + 1
    for name in FC.EXACT:
        if name in FC.BIG or max(FC.EXACT[name][:2]) > 600:
            continue
        c = FC.exact_case(name)
        for b, w in enumerate(c['want']):
            if w is not None:
                assert w['cost'] >= DR.dtw(c['x'][b, :c['n'][b]], c['y'][b, :c['m'][b]], c['metric'])['cost']
    assert 0 < above < total, (above, total)


def f32_distance(x, y, metric):
    """dtw_ref.distance in np.float32 arithmetic, summed in order of d (every partial sum is exact when the budget holds)."""
    s = np.zeros((len(x), len(y)), np.float32)
    for d in range(x.shape[1]):
        e = x[:, None, d] - y[None, :, d]
        s = s + (np.abs(e) if metric == 'l1' else e * e)
    return np.sqrt(s) if metric == 'l2' else s


@pytest.mark.parametrize('name', sorted(FC.EXACT))
def test_lattice_cases_are_exact_in_fp32(name):
    N, M, D, B, metric, radius, _ = FC.EXACT[name]
    L = FC.depth(N, M, radius)
    assert FC.bits_needed(D, metric, L) <= 24 and (metric != 'l2' or D == 1), (name, L)
    c = FC.exact_case(name)
    for b, w in enumerate(c['want']):
        if w is None:
            continue
        x, y = c['x'][b, :c['n'][b]], c['y'][b, :c['m'][b]]
        assert len(w['levels']) == FC.depth(len(x), len(y), radius) + 1
        for lv, level in enumerate(w['levels']):
            if lv:
                x64, y64 = x.astype(np.float64), y.astype(np.float64)
                x64, y64 = 0.5 * (x64[0:len(x) // 2 * 2:2] + x64[1::2]), 0.5 * (y64[0:len(y) // 2 * 2:2] + y64[1::2])
                x, y = FR.halve(x), FR.halve(y)
                assert np.array_equal(x, x64) and np.array_equal(y, y64)                  # the fp32 pyramid is exact here
            assert (len(x), len(y)) == (level['n'], level['m'])
            rows = np.unique(level['path'][:, 0])[:: max(1, level['n'] // 64)]              # distances along the path's rows, a band around it
            for i in rows:
                js = level['path'][level['path'][:, 0] == i, 1]
                j0, j1 = max(int(js.min()) - 4 * radius - 2, 0), int(js.max()) + 4 * radius + 3
                assert np.array_equal(f32_distance(x[i:i + 1], y[j0:j1], metric).astype(np.float64), DR.distance(x[i:i + 1], y[j0:j1], metric))
        assert w['cost'] == DR.score(w['path'], c['x'][b], c['y'][b], metric) and DR.is_warping_path(w['path'], c['n'][b], c['m'][b])


def test_plateau_cases_have_rows_wider_than_a_wave_and_than_256_columns():
    for name, axis in (('plateau', 0), ('plateau_t', 1)):
        path = FC.exact_case(name)['want'][0]['levels'][1]['path']
        n, m = FC.EXACT[name][:2]
        widths = [len(r) for r in FR.closed_window(path, n, m, 1)]
        runs = np.bincount(FC.exact_case(name)['want'][0]['path'][:, axis])
        if axis == 0:
            assert max(widths) > 256 and runs.max() > 256, (max(widths), runs.max())
        else:
            assert runs.max() > 256, runs.max()


def shaped_path(kind, n, m):
    if kind == 'L':                                                   # all of row 0, then all of the last column
        return [(0, j) for j in range(m)] + [(i, m - 1) for i in range(1, n)]
    if kind == 'diagonal':
        k = min(n, m)
        return [(i, i) for i in range(k)] + [(i, k - 1) for i in range(k, n)] + [(k - 1, j) for j in range(k, m)]
    cells, i, j = [(0, 0)], 0, 0                                      # staircase: right, down, right, ...
    while (i, j) != (n - 1, m - 1):
        if (len(cells) % 2 and j < m - 1) or i == n - 1:
            j += 1
        else:
            i += 1
        cells.append((i, j))
    return cells


@pytest.mark.parametrize('kind', ['staircase', 'L', 'diagonal'])
def test_workspace_covers_what_the_reference_needs(kind):
    """Per level the kernel keeps: the fp32 frames of both halved sequences, four int32 per row, and per anti-diagonal one int32 and
    2 bits for each of its cells. Summed over the levels of a pair this must fit the size the query returns, for every radius."""
    lib = pkg()._lib.lib()
    for N, M, D in ((100, 100, 25), (64, 300, 1), (301, 77, 64), (2048, 1999, 3)):
        for radius in (1, 3, 8):
            need_frames = need_level = 0
            n, m = N, M
            while n >= radius + 2 and m >= radius + 2:
                nc, mc = n // 2, m // 2
                rows = FR.closed_window(shaped_path(kind, nc, mc), n, m, radius)
                assert max(n, m) > 600 or rows == FR.literal_window(shaped_path(kind, nc, mc), n, m, radius)
                cells, diags = sum(map(len, rows)), n + m - 1
                assert cells <= (4 * radius + 2) * diags and FR.max_rows_on_a_diagonal(rows) <= 4 * radius + 2
                need_level = max(need_level, 4 * 4 * n + 4 * diags + (2 * cells + 7) // 8)
                need_frames += 4 * D * (nc + mc)
                n, m = nc, mc
            for B in (1, 3):
                got = lib.tdvc_fastdtw_workspace(B, N, M, D, radius, 1)
                assert got >= B * (need_frames + need_level) and got == lib.tdvc_fastdtw_workspace(B, N, M, D, radius, 0), (N, M, D, radius)
    assert lib.tdvc_fastdtw_workspace(1, 16384, 16384, 64, 8, 1) > 0
    for bad in ((0, 8, 8, 1, 1), (1, 0, 8, 1, 1), (1, 8, 0, 1, 1), (1, 8, 8, 0, 1), (1, 8, 8, 1, 0), (1, 16385, 8, 1, 1), (1, 8, 16385, 1, 1),
                (1, 8, 8, 65, 1), (1, 8, 8, 1, 9), (-1, 8, 8, 1, 1)):
        assert lib.tdvc_fastdtw_workspace(*bad, 1) == 0, bad


def test_symbols_in_header_binding_library_and_package():
    P = pkg()
    L = P._lib
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = L.lib()
    for name in ('tdvc_fastdtw', 'tdvc_fastdtw_workspace'):
        assert re.search(rf'\b{name}\(', header), name
        assert name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.tdvc_fastdtw_workspace.restype is C.c_size_t and len(L.SIGNATURES['tdvc_fastdtw'][1]) == 21
    assert os.path.exists(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'eval_fastdtw.hip'))
    assert 'eval_fastdtw.hip' in open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert P.fastdtw is P.evaluate.fastdtw and P.evaluate.ALIGNMENTS == ('exact', 'fastdtw')


def test_refusals_through_the_raw_abi_before_any_launch():
    """The table of include/tdvc.h. A null stream and host memory: a call that got past its checks would launch, so only refused
    calls and the B == 0 no-op are made here."""
    lib = pkg()._lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    B, N, M, D = 2, 8, 9, 3
    P = 2 * (N + M - 1)
    big = 1 << 40

    def call(B=B, N=N, M=M, D=D, metric=0, radius=1, x=p, y=p, cost=p, length=p, path=p, path_bs=P, x_bs=N * D, x_fs=D, y_bs=M * D, y_fs=D,
             ws=p, ws_bytes=big):
        return lib.tdvc_fastdtw(x, x_bs, x_fs, y, y_bs, y_fs, None, None, B, N, M, D, metric, radius, cost, length, path, path_bs, ws, ws_bytes, None)
    cases = [
        (dict(B=-1), EINVAL), (dict(N=0), EINVAL), (dict(M=0), EINVAL), (dict(D=0), EINVAL), (dict(N=-4), EINVAL),
        (dict(metric=3), EINVAL), (dict(metric=-1), EINVAL), (dict(radius=0), EINVAL), (dict(radius=-2), EINVAL),
        (dict(x_fs=D - 1), EINVAL), (dict(y_fs=0), EINVAL), (dict(x_bs=-1), EINVAL), (dict(y_bs=-1), EINVAL),
        (dict(path_bs=P - 1), EINVAL), (dict(path_bs=-1), EINVAL), (dict(B=1, path_bs=P - 1), EINVAL),
        (dict(x=None), EINVAL), (dict(y=None), EINVAL), (dict(cost=None), EINVAL), (dict(length=None), EINVAL),
        (dict(N=16385, path_bs=1 << 20), EUNSUPPORTED), (dict(M=16385, path_bs=1 << 20), EUNSUPPORTED),
        (dict(D=65, x_fs=65, y_fs=65), EUNSUPPORTED), (dict(radius=9), EUNSUPPORTED),
        (dict(ws=None), EWORKSPACE), (dict(ws_bytes=0), EWORKSPACE),
        (dict(ws_bytes=lib.tdvc_fastdtw_workspace(B, N, M, D, 1, 1) - 1), EWORKSPACE),
    ]
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert b'fastdtw' in lib.tdvc_last_error()
    assert call(B=0) == 0 and call(B=0, x=None, ws=None) == 0                       # a no-op
    assert call(B=0, N=16385, path_bs=1 << 20) == EUNSUPPORTED                      # the arguments are still checked
    assert call(path=None, path_bs=0, radius=9) == EUNSUPPORTED                     # without a path its stride does not matter
    assert not any(buf)


def test_real_valued_cases_meet_the_margin_condition():
    """The condition is on the inputs: where every level's smallest back-traced margin exceeds 4 x the rounding bound of that
    level's cost, a solver with distances within eps relative takes the same path. (200 x 150 with seed n + m + 3 and 900 x 700
    fail it and are not used for identity.)"""
    for n, m, k in FC.IDENTITY:
        _, _, w = FC.real_case(n, m, k)
        ratio = FC.margin_ratio(w)
        print(f'{n}x{m} seed +{k}: margin / bound {ratio:.1f}, levels {len(w["levels"])}')
        assert ratio > 1, (n, m, k, ratio)
        x, y, _ = FC.real_case(n, m, k)
        assert w['cost'] >= DR.dtw(x, y, 'l2')['cost']
