"""Float64 numpy restatement of the exact dynamic time warping behind tdvc_dtw (include/tdvc.h). Test helper: the CPU suite checks
it against brute-force enumeration of every warping path, the GPU suite checks the kernel against it.

    d(i, j)   'l2' sqrt(sum (x - y)^2), 'l1' sum |x - y|, 'sq' sum (x - y)^2
    C(0, 0) = d(0, 0);  C(i, j) = d(i, j) + min(C(i-1, j), C(i, j-1), C(i-1, j-1)), the FIRST minimum in the order up, left, diagonal
    len(0, 0) = 1;      len(i, j) = len(chosen predecessor) + 1          (carried forward with the cost)

The programme is evaluated one anti-diagonal at a time (every cell of a diagonal depends only on the two before it), so a
1024 x 1024 pair is 2047 vector steps. `backtrace` walks the stored directions from (n-1, m-1) to (0, 0).
"""
import numpy as np

METRICS = ('l2', 'l1', 'sq')
UP, LEFT, DIAG = 0, 1, 2


def distance(x, y, metric='l2'):
    """x [n, D], y [m, D] -> float64 [n, m], from direct differences."""
    e = np.asarray(x, np.float64)[:, None, :] - np.asarray(y, np.float64)[None, :, :]
    if metric == 'l1':
        return np.abs(e).sum(-1)
    s = (e * e).sum(-1)
    if metric == 'sq':
        return s
    if metric == 'l2':
        return np.sqrt(s)
    raise ValueError(metric)


def accumulate(d):
    """Local distances d [n, m] -> (C [n, m] float64, length [n, m] int64, direction [n, m] int8), (0, 0) marked DIAG."""
    n, m = d.shape
    C = np.full((n + 1, m + 1), np.inf)              # C[i + 1, j + 1] = cost of cell (i, j); row 0 and column 0 are the +inf border
    Ln = np.zeros((n + 1, m + 1), np.int64)
    Dr = np.full((n, m), DIAG, np.int8)
    for k in range(n + m - 1):
        i = np.arange(max(0, k - m + 1), min(k, n - 1) + 1)
        j = k - i
        cand = np.stack([C[i, j + 1], C[i + 1, j], C[i, j]])          # up, left, diagonal
        lens = np.stack([Ln[i, j + 1], Ln[i + 1, j], Ln[i, j]])
        pick = cand.argmin(0)                                           # numpy's argmin is the FIRST minimum
        best = np.take_along_axis(cand, pick[None], 0)[0]
        bl = np.take_along_axis(lens, pick[None], 0)[0]
        if k == 0:
            best, bl, pick = np.zeros(1), np.zeros(1, np.int64), np.full(1, DIAG)
        C[i + 1, j + 1] = d[i, j] + best
        Ln[i + 1, j + 1] = bl + 1
        Dr[i, j] = pick
    return C[1:, 1:], Ln[1:, 1:], Dr


def backtrace(Dr):
    """Directions [n, m] -> path int64 [L, 2] from (0, 0) to (n-1, m-1)."""
    i, j = Dr.shape[0] - 1, Dr.shape[1] - 1
    cells = [(i, j)]
    while i > 0 or j > 0:
        dr = Dr[i, j]
        i, j = i - (dr != LEFT), j - (dr != UP)
        cells.append((i, j))
    return np.asarray(cells[::-1], np.int64)


def dtw(x, y, metric='l2'):
    """x [n, D], y [m, D] -> dict(cost float, length int (carried forward), path [L, 2] (back-traced))."""
    C, Ln, Dr = accumulate(distance(x, y, metric))
    return dict(cost=float(C[-1, -1]), length=int(Ln[-1, -1]), path=backtrace(Dr))


def score(path, x, y, metric='l2'):
    """Sum of the float64 local distances along a path [L, 2]."""
    path = np.asarray(path)
    x, y = np.asarray(x, np.float64)[path[:, 0]], np.asarray(y, np.float64)[path[:, 1]]
    e = x - y
    if metric == 'l1':
        return float(np.abs(e).sum())
    s = (e * e).sum(-1)
    return float(s.sum() if metric == 'sq' else np.sqrt(s).sum())


def is_warping_path(path, n, m):
    """Starts at (0, 0), ends at (n-1, m-1), every step is one of (1, 0), (0, 1), (1, 1)."""
    path = np.asarray(path)
    if path.ndim != 2 or path.shape[1] != 2 or len(path) < 1:
        return False
    if tuple(path[0]) != (0, 0) or tuple(path[-1]) != (n - 1, m - 1):
        return False
    step = np.diff(path, axis=0)
    return bool(np.all((step >= 0) & (step <= 1)) and np.all(step.sum(1) >= 1))


def all_paths(n, m):
    """Every warping path of an n x m lattice as a list of cell tuples (brute force: small lattices only)."""
    out = []

    def walk(i, j, acc):
        acc = acc + [(i, j)]
        if i == n - 1 and j == m - 1:
            out.append(acc)
            return
        for di, dj in ((1, 0), (0, 1), (1, 1)):
            if i + di < n and j + dj < m:
                walk(i + di, j + dj, acc)
    walk(0, 0, [])
    return out


def brute_force(d):
    """Minimum over every warping path of the summed local distance d [n, m] -> (cost, the set of lengths of the minimal paths)."""
    n, m = d.shape
    best, lens = np.inf, set()
    for p in all_paths(n, m):
        c = sum(d[i, j] for i, j in p)
        if c < best:
            best, lens = c, {len(p)}
        elif c == best:
            lens.add(len(p))
    return best, lens


def warped_pair(rng, n, m, D, noise=0.1):
    """A smooth random sequence x [n, D] and a time-warped noisy copy y [m, D] (float32): the real-valued test pair."""
    base = np.cumsum(rng.standard_normal((n, D)), 0) * 0.3
    t = np.sort(rng.uniform(0, n - 1, m))
    t[0], t[-1] = 0, n - 1
    lo = np.floor(t).astype(int)
    hi = np.minimum(lo + 1, n - 1)
    fr = (t - lo)[:, None]
    y = base[lo] * (1 - fr) + base[hi] * fr + noise * rng.standard_normal((m, D))
    return base.astype(np.float32), y.astype(np.float32)

