"""GPU: tdvc_fastdtw (csrc/eval_fastdtw.hip) through the package and the raw C ABI against the literal float64 restatement
tests/fastdtw_ref.py, and `mcd(align='fastdtw')`. The inputs and their references live in tests/fastdtw_cases.py;
tests/test_fastdtw_cpu.py proves what is assumed of them here.

1. Exact lattices (integers |v| <= 3 under the bit budget of fastdtw_cases, so every fp32 distance at every level is exact): cost,
   length and EVERY path cell equal the reference. 1 x 1, one row, one column, the base case at level 0 against a long other side,
   the first recursions, 63/64/65 and 255/256/257 mixes, rows wider than a wave and than 256 columns, 40 x 1500, 1024 x 1024,
   16384 x 16001, identical and constant sequences (all ties), radius 1, 2, 3, 8, D = 1, 25, 64, B = 1 and 5 with per-pair lengths
   0, 1 and full, NaN in all padding, strided views, a workspace pre-filled with 0x5A, with and without the path.
2. Real-valued pairs (dtw_ref.warped_pair, D = 25, 'l2'), eps = (D + 2) 2^-24. Where the inputs meet the margin condition
   (fastdtw_cases.IDENTITY; checked on the host) the device must take the reference's path and |cost - C_ref| <= 2 eps C_ref.
   900 x 700 does not meet it: there the result must be a valid warping path of `length` cells whose float64 re-score is the
   cost within 2 eps, and the cost is at least the exact optimum (1 - 2 eps); the distance to the reference is printed.
3. The kernel by trace; `dtw` still launches only its own.
4. mcd(align='fastdtw'): identical signals, a pair of different vowels, 30 s of audio (where mcd() refuses), graph capture.
"""
import numpy as np
import pytest
import torch

import dtw_ref as DR
import fastdtw_cases as FC
from common import pkg, traced

pytestmark = pytest.mark.gpu
NAN = float('nan')


def vowel(rng, T, f0, sr=16000):
    """A harmonic tone under a fixed formant-like envelope with a slow vibrato, a little noise; 0.1 s of near-silence at either end
    (the signal of tests/test_mcd_gpu.py)."""
    t = np.arange(T) / sr
    phase = 2 * np.pi * np.cumsum(f0 * (1 + 0.03 * np.sin(2 * np.pi * 3.0 * t))) / sr
    x = sum(np.sin(h * phase) / (1 + ((h * f0 - 700.0) / 400.0) ** 2) for h in range(1, 20))
    x = 0.05 * x + 0.001 * rng.standard_normal(T)
    x[:sr // 10] *= 0.001
    x[-sr // 10:] *= 0.001
    return x.astype(np.float32)


def check_against(c, cost, length, path=None):
    cost, length = cost.cpu().numpy(), length.cpu().numpy()
    path = None if path is None else path.cpu().numpy()
    for b, w in enumerate(c['want']):
        if w is None:
            assert np.isnan(cost[b]) and length[b] == 0
            assert path is None or (path[b] == -1).all()
            continue
        assert cost[b] == w['cost'] and length[b] == w['length'], (b, cost[b], w['cost'], length[b], w['length'])
        if path is not None:
            L = w['length']
            assert np.array_equal(path[b, :L], w['path']), (b, int((path[b, :L] != w['path']).any(1).argmax()))
            assert (path[b, L:] == -1).all(), b


@pytest.mark.parametrize('name', sorted(FC.EXACT))
def test_exact_lattice_equals_the_reference(dev, name):
    E = pkg().evaluate
    c = FC.exact_case(name)
    t = lambda a: torch.from_numpy(a).to(dev)
    x, y, n, m = t(c['x']), t(c['y']), t(c['n']), t(c['m'])
    kw = dict(radius=c['radius'], metric=c['metric'])
    with traced() as tr:
        cost, length, path = E.fastdtw(x, y, n, m, return_path=True, **kw)
    assert tr.names == {'fastdtw_kernel'}, tr.names
    assert cost.dtype == torch.float64 and length.dtype == torch.int32 and path.dtype == torch.int64
    assert path.shape == (x.shape[0], x.shape[1] + y.shape[1] - 1, 2)
    check_against(c, cost, length, path)
    cost2, length2 = E.fastdtw(x, y, n, m, **kw)                                  # without the path: the same figures
    assert torch.equal(cost2.nan_to_num(-1), cost.nan_to_num(-1)) and torch.equal(length2, length)
    again = E.fastdtw(x, y, n, m, return_path=True, **kw)                         # two calls, the same bits
    assert torch.equal(again[0].nan_to_num(-1), cost.nan_to_num(-1)) and torch.equal(again[2], path)


@pytest.mark.parametrize('metric', DR.METRICS)
def test_all_metrics_a_single_pair_and_dtw_keeps_its_own_kernel(dev, metric):
    import fastdtw_ref as FR
    P = pkg()
    E = P.evaluate
    rng = np.random.default_rng(3)
    D = 1 if metric == 'l2' else 7
    x, y = rng.integers(-3, 4, (50, D)).astype(np.float32), rng.integers(-3, 4, (77, D)).astype(np.float32)
    w = FR.fastdtw(x, y, 1, metric)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    cost, length, path = P.fastdtw(xd, yd, metric=metric, return_path=True)
    assert cost.shape == () and length.shape == () and path.shape == (126, 2)
    assert float(cost) == w['cost'] and int(length) == w['length'] and np.array_equal(path[:w['length']].cpu().numpy(), w['path'])
    with traced() as tr:
        exact = E.dtw(xd, yd, metric=metric)
    assert tr.names == {'dtw_kernel<4,1024>' if D == 1 else 'dtw_kernel<16,1024>'}, tr.names
    assert float(exact[0]) == DR.dtw(x, y, metric)['cost'] <= float(cost)


def test_strided_views_with_nan_in_the_spare_elements(dev):
    E = pkg().evaluate
    c = FC.exact_case('256x257')
    B, N, D = c['x'].shape
    M = c['y'].shape[1]
    wx = torch.full((2 * B, N + 2, D + 3), NAN, device=dev)
    wy = torch.full((B, M + 1, D + 5), NAN, device=dev)
    wx[::2, 1:1 + N, :D] = torch.from_numpy(c['x']).to(dev)
    wy[:, 1:, :D] = torch.from_numpy(c['y']).to(dev)
    vx, vy = wx[::2, 1:1 + N, :D], wy[:, 1:, :D]
    assert not vx.is_contiguous() and vx.stride() == (2 * (N + 2) * (D + 3), D + 3, 1)
    n, m = torch.from_numpy(c['n']).to(dev), torch.from_numpy(c['m']).to(dev)
    cost, length, path = E.fastdtw(vx, vy, n, m, radius=c['radius'], metric=c['metric'], return_path=True)
    check_against(c, cost, length, path)
    assert bool(torch.isnan(wx[1::2]).all())                                       # nothing was written to the inputs


def test_raw_abi_poisoned_workspace_strided_path_and_null_lengths(dev):
    """Through ctypes: a workspace pre-filled with 0x5A (a read of workspace the kernel has not written would change the result),
    path rows 2 (N + M - 1) + 6 apart with the elements between them untouched, and NULL lengths meaning full pairs."""
    import fastdtw_ref as FR
    lib = pkg()._lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    for name in ('64x65', '40x300r8', 'constant'):
        c = FC.exact_case(name)
        B, N, D = c['x'].shape
        M = c['y'].shape[1]
        P = 2 * (N + M - 1)
        t = {k: torch.from_numpy(c[k]).to(dev) for k in ('x', 'y', 'n', 'm')}
        nbytes = lib.tdvc_fastdtw_workspace(B, N, M, D, c['radius'], 1)
        outs = []
        for fill in (0x5A, 0x00):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
            cost = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
            length = torch.full((B,), -7, dtype=torch.int32, device=dev)
            path = torch.full((B, P + 6), -7, dtype=torch.int32, device=dev)
            rc = lib.tdvc_fastdtw(t['x'].data_ptr(), N * D, D, t['y'].data_ptr(), M * D, D, t['n'].data_ptr(), t['m'].data_ptr(), B, N, M, D,
                                  {'l2': 0, 'l1': 1, 'sq': 2}[c['metric']], c['radius'], cost.data_ptr(), length.data_ptr(), path.data_ptr(), P + 6,
                                  ws.data_ptr(), nbytes, st)
            torch.cuda.synchronize()
            assert rc == 0 and bool((path[:, P:] == -7).all())
            check_against(c, cost, length, path[:, :P].reshape(B, P // 2, 2))
            outs.append((cost, length, path))
        assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][1], outs[1][1])
    c = FC.exact_case('63x64')
    x, y = np.nan_to_num(c['x']), np.nan_to_num(c['y'])
    B, N, D = x.shape
    M = y.shape[1]
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.tdvc_fastdtw_workspace(B, N, M, D, 1, 0)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    assert lib.tdvc_fastdtw(xd.data_ptr(), N * D, D, yd.data_ptr(), M * D, D, None, None, B, N, M, D, 0, 1, cost.data_ptr(), length.data_ptr(), None, 0,
                            ws.data_ptr(), nbytes, st) == 0
    torch.cuda.synchronize()
    for b in range(B):
        w = FR.fastdtw(x[b], y[b], 1, 'l2')
        assert float(cost[b]) == w['cost'] and int(length[b]) == w['length']


# ------------------------------------------------------------------------------------------------------------ real-valued pairs
@pytest.mark.parametrize('n,m,k', FC.IDENTITY)
def test_real_valued_pair_takes_the_reference_path(dev, n, m, k):
    E = pkg().evaluate
    x, y, w = FC.real_case(n, m, k)
    assert FC.margin_ratio(w) > 1                                                  # the condition on the inputs (test_fastdtw_cpu)
    cost, length, path = E.fastdtw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), return_path=True)
    cost, length, path = float(cost), int(length), path.cpu().numpy()
    print(f'\nfastdtw {n}x{m}+{k}: C_ref {w["cost"]:.6f}, |cost - C_ref| {abs(cost - w["cost"]):.3e}, bound {2 * FC.EPS * w["cost"]:.3e}')
    assert length == w['length'] and np.array_equal(path[:length], w['path']) and (path[length:] == -1).all()
    assert abs(cost - w['cost']) <= 2 * FC.EPS * w['cost']


def test_real_valued_900x700_is_a_valid_scored_path(dev):
    E = pkg().evaluate
    n, m, k = FC.LOOSE
    x, y, w = FC.real_case(n, m, k)
    exact = DR.dtw(x, y, 'l2')['cost']
    cost, length, path = E.fastdtw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), return_path=True)
    cost, length, path = float(cost), int(length), path.cpu().numpy()
    p = path[:length]
    rescored = DR.score(p, x, y, 'l2')
    ref_cells = {tuple(cell) for cell in w['path']}
    off = sum(tuple(cell) not in ref_cells for cell in p)
    print(f'\nfastdtw {n}x{m}: C_ref {w["cost"]:.6f}, exact {exact:.6f}, |cost - C_ref| {abs(cost - w["cost"]):.3e}, '
          f'|cost - re-scored| {abs(cost - rescored):.3e}, bound {2 * FC.EPS * rescored:.3e}, cells off the reference path {off} of {length}')
    assert DR.is_warping_path(p, n, m) and (path[length:] == -1).all()
    assert abs(cost - rescored) <= 2 * FC.EPS * rescored
    assert cost >= exact * (1 - 2 * FC.EPS)


# ------------------------------------------------------------------------------------------------------------ mcd
def test_mcd_fastdtw_identical_signals_and_a_pair_of_vowels(dev):
    P = pkg()
    rng = np.random.default_rng(4)
    T = 9600
    a, b = vowel(rng, T, 140.0), vowel(rng, T, 180.0)
    test = torch.from_numpy(np.stack([a, a]))[:, None].to(dev)
    ref = torch.from_numpy(np.stack([a, b]))[:, None].to(dev)
    with traced() as tr:
        fast = P.mcd(test, ref, align='fastdtw')
    assert 'fastdtw_kernel' in tr.names and not any(k.startswith('dtw_kernel') for k in tr.names), tr.names
    exact = P.mcd(test, ref)
    assert set(fast) == set(exact) and all(v.dtype == torch.float64 and v.shape == (2,) for v in fast.values())
    assert float(fast['mcd'][0]) == 0.0 == float(exact['mcd'][0]) and torch.equal(fast['path_len'][0], exact['path_len'][0])
    for k in ('n_test', 'n_ref', 'diff_f0_mean', 'diff_f0_var', 'f0_ratio'):
        assert torch.equal(fast[k], exact[k]), k
    # cost = mcd * path_len: FastDTW's path is one of the paths the exact programme minimises over, and both kernels see distances
    # within eps = (D + 2) 2^-24 relative of the true ones, so cost_fast >= cost_exact (1 - 2 eps) (the bound; the figures mcd differ in path_len)
    cf, ce = float(fast['mcd'][1] * fast['path_len'][1]), float(exact['mcd'][1] * exact['path_len'][1])
    print(f'\nmcd: fastdtw cost {cf:.6f} over {int(fast["path_len"][1])} cells, exact cost {ce:.6f} over {int(exact["path_len"][1])} cells')
    assert ce > 0 and cf >= ce * (1 - 2 * FC.EPS)
    assert torch.equal(P.mcd(test, ref, align='fastdtw', radius=1)['mcd'], fast['mcd'])
    wide = P.mcd(test, ref, align='fastdtw', radius=8)
    assert float(wide['mcd'][1] * wide['path_len'][1]) >= ce * (1 - 2 * FC.EPS) and float(wide['mcd'][0]) == 0.0
    with pytest.raises(ValueError):
        P.mcd(test, ref, align='bogus')
    with pytest.raises(ValueError):
        P.evaluate.fastdtw(test[0], ref[0], radius=0)


def test_mcd_fastdtw_on_30_seconds_where_exact_refuses(dev):
    P = pkg()
    rng = np.random.default_rng(6)
    T = 30 * 16000
    test = torch.from_numpy(vowel(rng, T, 130.0))[None, None].to(dev)
    ref = torch.from_numpy(vowel(rng, T - 4000, 150.0))[None, None].to(dev)
    with pytest.raises(ValueError):
        P.mcd(test, ref)                                                          # 6001 frames: beyond the exact kernel's 4096
    r = P.mcd(test, ref, align='fastdtw')
    nt, nr, pl = int(r['n_test'][0]), int(r['n_ref'][0]), int(r['path_len'][0])
    assert nt > 4096 and nr > 4096 and max(nt, nr) <= pl <= nt + nr - 1 and float(r['mcd'][0]) > 0


def test_mcd_fastdtw_under_graph_capture(dev):
    """No host synchronisation on the new route either: the whole call is captured, and a replay follows its inputs."""
    P = pkg()
    rng = np.random.default_rng(12)
    T = 6400
    test = torch.from_numpy(vowel(rng, T, 130.0))[None, None].to(dev)
    ref = torch.from_numpy(vowel(rng, T, 160.0))[None, None].to(dev)
    tl = torch.tensor([T], device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        P.mcd(test, ref, tl, tl, align='fastdtw')                                 # warm-up
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = P.mcd(test, ref, tl, tl, align='fastdtw')
    graph.replay()
    torch.cuda.synchronize(dev)
    eager = P.mcd(test, ref, tl, tl, align='fastdtw')
    assert all(torch.equal(r[k], eager[k]) for k in r) and float(r['mcd'][0]) > 0
    ref.copy_(test)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert float(r['mcd'][0]) == 0.0
