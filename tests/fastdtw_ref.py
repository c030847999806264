"""Literal restatement of FastDTW (Salvador & Chan) in the form of the `fastdtw` Python package, as include/tdvc.h defines
tdvc_fastdtw. Test helper: the CPU suite checks its two window constructions against each other, the GPU suite checks the kernel
against it. The package itself is not available to this repository, so parity with it is NOT checked here either.

    recursion   n < r + 2 or m < r + 2: the full programme; otherwise halve, recurse, expand the coarse path into a window, solve inside it
    halving     fp32: np.float32(0.5) * (x[2i] + x[2i+1]) in np.float32 arithmetic (the package averages in float64: a stated deviation)
    window      `literal_window`: the package's sets and its row scan; `closed_window`: the closed form the kernel uses
    programme   a dict of cells, float64 costs, distances by dtw_ref.distance (float64 from direct differences of the fp32 level),
                C = d + the FIRST minimum in the order up, left, diagonal; the path is traced back along the chosen predecessors
"""
import numpy as np

import dtw_ref as DR


def halve(x):
    """x fp32 [n, D] -> fp32 [n // 2, D]; an odd last frame is dropped."""
    x = np.asarray(x, np.float32)
    n2 = len(x) // 2
    return (np.float32(0.5) * (x[0:2 * n2:2] + x[1:2 * n2:2])).astype(np.float32)


def literal_window(path, n, m, radius):
    """The package's __expand_window: coarse path -> the columns of every fine row (a list of lists)."""
    path = [tuple(int(v) for v in c) for c in path]
    path_ = set(path)
    for i, j in path:
        for a in range(-radius, radius + 1):
            for b in range(-radius, radius + 1):
                path_.add((i + a, j + b))                    # cells outside the coarse grid, negative ones included
    window_ = set()
    for i, j in path_:
        for cell in ((i * 2, j * 2), (i * 2, j * 2 + 1), (i * 2 + 1, j * 2), (i * 2 + 1, j * 2 + 1)):
            window_.add(cell)
    rows, start_j = [], 0
    for i in range(n):
        new_start_j, cols = None, []
        for j in range(start_j, m):
            if (i, j) in window_:
                cols.append(j)
                if new_start_j is None:
                    new_start_j = j
            elif new_start_j is not None:
                break
        assert new_start_j is not None, (i, n, m, radius)    # the package would fail on range(None, ...)
        start_j = new_start_j
        rows.append(cols)
    return rows


def closed_window(path, n, m, radius):
    """The same window in closed form: with jmin(a) / jmax(a) the first / last column of the coarse path in row a and n_c coarse
    rows, fine row i (c = i // 2) gets [max(2 (jmin(max(c - r, 0)) - r), 0), min(2 (jmax(min(c + r, n_c - 1)) + r) + 1, m - 1)]."""
    path = np.asarray(path, np.int64)
    nc = int(path[-1, 0]) + 1
    jmin = np.full(nc, np.iinfo(np.int64).max)
    jmax = np.full(nc, -1)
    np.minimum.at(jmin, path[:, 0], path[:, 1])
    np.maximum.at(jmax, path[:, 0], path[:, 1])
    rows = []
    for i in range(n):
        c = i // 2
        lo = max(2 * (int(jmin[max(c - radius, 0)]) - radius), 0)
        hi = min(2 * (int(jmax[min(c + radius, nc - 1)]) + radius) + 1, m - 1)
        rows.append(list(range(lo, hi + 1)))
    return rows


def windowed_dtw(x, y, rows, metric):
    """The programme over the cells rows[i] = columns of row i -> dict(cost, path [L, 2], cells, margin). margin: the smallest gap
    between the best and the second-best predecessor among the cells of the back-traced path (+inf where a cell has one)."""
    n, m = len(x), len(y)
    inf = float('inf')
    C = {(-1, -1): (0.0, None, inf)}                        # cell -> (cost, chosen predecessor, margin)
    cells = 0
    for i, cols in enumerate(rows):
        if not cols:
            continue
        d = DR.distance(x[i:i + 1], y[cols[0]:cols[-1] + 1], metric)[0]
        assert cols[-1] - cols[0] + 1 == len(cols)
        for j, dt in zip(cols, d):
            cand = ((i - 1, j), (i, j - 1), (i - 1, j - 1))              # up, left, diagonal
            costs = [C[c][0] if c in C else inf for c in cand]
            if i == 0 and j == 0:
                costs = [inf, inf, 0.0]
            k = int(np.argmin(costs))                                    # the FIRST minimum
            rest = sorted(costs[:k] + costs[k + 1:])
            C[i, j] = (float(dt) + costs[k], cand[k], rest[0] - costs[k] if np.isfinite(rest[0]) else inf)
            cells += 1
    path, margin = [], inf
    cell = (n - 1, m - 1)
    while cell != (-1, -1):
        path.append(cell)
        margin = min(margin, C[cell][2])
        cell = C[cell][1] if cell != (0, 0) else (-1, -1)
    return dict(cost=C[n - 1, m - 1][0], path=np.asarray(path[::-1], np.int64), cells=cells, margin=margin)


def fastdtw(x, y, radius=1, metric='l2', window='literal'):
    """x [n, D], y [m, D] -> dict(cost, length, path [L, 2], levels): levels[0] is the finest; each level is
    dict(n, m, cost, path, cells, margin, windowed). window: 'literal' (the package's construction) or 'closed' (the closed form)."""
    expand = {'literal': literal_window, 'closed': closed_window}[window]
    xs, ys = [np.asarray(x, np.float32)], [np.asarray(y, np.float32)]
    while len(xs[-1]) >= radius + 2 and len(ys[-1]) >= radius + 2:
        xs.append(halve(xs[-1]))
        ys.append(halve(ys[-1]))
    levels, path = [], None
    for lx, ly in zip(xs[::-1], ys[::-1]):
        n, m = len(lx), len(ly)
        rows = [list(range(m))] * n if path is None else expand(path, n, m, radius)
        r = windowed_dtw(lx, ly, rows, metric)
        levels.append(dict(n=n, m=m, windowed=path is not None, **r))
        path = r['path']
    levels = levels[::-1]
    return dict(cost=levels[0]['cost'], length=len(path), path=path, levels=levels)


def max_rows_on_a_diagonal(rows):
    """The largest number of rows with a cell on one anti-diagonal i + j = k of a window."""
    count = {}
    for i, cols in enumerate(rows):
        for j in cols:
            count[i + j] = count.get(i + j, 0) + 1
    return max(count.values())
