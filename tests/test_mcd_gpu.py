"""GPU: objective evaluation on the device (td-vc-gan_amd/evaluate.py; csrc/eval_dtw.hip, csrc/eval_mcep.hip) through the package and
through the raw C ABI, against the float64 helpers tests/dtw_ref.py and tests/mcep_ref.py.

1. Exact lattices: inputs are integers of magnitude <= 3 (D = 1 for 'l2', D up to 64 for 'sq' and 'l1'), so every fp32 distance is
   exact and every sum stays far below 2^24: cost, length and EVERY path cell must equal the float64 reference; the inputs are full
   of ties. The shapes reach every kernel instance by trace -- dtw_kernel<4,1024> (D <= 4), <16,1024>, <28,1024>, <64,512> -- and in
   each of them a second band of rows (N > 1024 / 512) and a wrap of the LDS ring of y (M > 1088 / 576), besides 1 x 1, one row,
   one column, 63/64/65 on either side, B = 1 and 5, per-pair lengths 0, 1 and full, NaN in all padding, strided views.
2. Real-valued pairs (a time-warped noisy copy, D = 25): with eps = (D + 2) 2^-24 the device solves the exact programme on
   distances within eps relative of the true ones, so |cost - C*| <= 2 eps C* and the device path re-scored in float64 is
   <= C* (1 + 2 eps); the path is a valid warping path of `length` cells.
   Measured on an MI355X (printed by the tests, run with -s):
       pair     metric  C*          |cost - C*|  re-scored path gap  bound 2 eps C*  cells off the float64 path
       200x150  l2      216.718410  3.772e-06    -5.684e-14          6.975e-04       0 of 216
       200x150  l1      870.864820  2.114e-06     0.000e+00          2.803e-03       0 of 217
       200x150  sq      272.723253  1.046e-06    -1.705e-13          8.778e-04       0 of 220
       900x700  l2      946.763035  1.059e-05     1.137e-13          3.047e-03       0 of 978
3. tdvc_sp2mc: every element within 4 * 2^-24 * max |mc of that frame| of the float64 reference; both layouts, the floor.
4. mel_cepstrum end to end against the float64 chain from the same fp32 signal; the bar is 4 x the error of a plain numpy fp32
   evaluation of the same windowed-DFT formulation on that input. Measured: device 4.383e-06, numpy fp32 4.253e-06, ratio 1.03.
5. mcd: identical signals, too few voiced frames, the F0 statistics, and the whole call under graph capture (no host sync).
6. Refusals, before any launch.
"""
import functools

import numpy as np
import pytest
import torch

import dtw_ref as DR
import mcep_ref as MR
from common import pkg, traced

pytestmark = pytest.mark.gpu
NAN = float('nan')
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


# ------------------------------------------------------------------------------------------------------------ exact lattices
#        name        N     M     D   B  metric  instance
EXACT = {
    '1x1':       (1,    1,    1,  1, 'l2', 'dtw_kernel<4,1024>'),
    '1x7':       (1,    7,    1,  5, 'l2', 'dtw_kernel<4,1024>'),
    '7x1':       (7,    1,    1,  5, 'l2', 'dtw_kernel<4,1024>'),
    '63x64':     (63,   64,   1,  5, 'l2', 'dtw_kernel<4,1024>'),
    '64x65':     (64,   65,   1,  5, 'l2', 'dtw_kernel<4,1024>'),
    '65x63':     (65,   63,   1,  5, 'l2', 'dtw_kernel<4,1024>'),
    '129x64':    (129,  64,   25, 5, 'sq', 'dtw_kernel<28,1024>'),
    '64x129':    (64,   129,  25, 5, 'l1', 'dtw_kernel<28,1024>'),
    '5x700':     (5,    700,  64, 5, 'l1', 'dtw_kernel<64,512>'),      # 700 columns wrap the 576-column ring
    '700x5':     (700,  5,    64, 5, 'sq', 'dtw_kernel<64,512>'),      # two bands of 512 rows
    '1024x1024': (1024, 1024, 1,  1, 'l2', 'dtw_kernel<4,1024>'),
    '1100x70':   (1100, 70,   1,  1, 'l2', 'dtw_kernel<4,1024>'),      # two bands of 1024 rows
    '3x1200':    (3,    1200, 1,  1, 'l2', 'dtw_kernel<4,1024>'),      # 1200 columns wrap the 1088-column ring
    '1030x40':   (1030, 40,   25, 1, 'l1', 'dtw_kernel<28,1024>'),     # two bands
    '70x1150':   (70,   1150, 25, 1, 'sq', 'dtw_kernel<28,1024>'),     # ring wrap
    '600x600':   (600,  600,  33, 1, 'sq', 'dtw_kernel<64,512>'),      # two bands and a wrap together
    '65x64d16':  (65,   64,   16, 5, 'l1', 'dtw_kernel<16,1024>'),
    '1030x70':   (1030, 70,   12, 1, 'sq', 'dtw_kernel<16,1024>'),     # two bands
    '3x1200d5':  (3,    1200, 5,  1, 'l1', 'dtw_kernel<16,1024>'),     # ring wrap
}


def pair_lengths(N, M, B):
    """Full, empty x, one frame of x, one frame of y, empty y."""
    if B == 1:
        return [N], [M]
    return [N, 0, 1, max(1, N // 2), N], [M, M, max(1, M // 3), 1, 0]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """dict(x [B, N, D], y [B, M, D] fp32 with NaN past the lengths, n, m, metric, want = per-pair float64 results or None)."""
    N, M, D, B, metric, inst = EXACT[name]
    rng = np.random.default_rng(sorted(EXACT).index(name) + 7)
    x = rng.integers(-3, 4, (B, N, D)).astype(np.float32)
    y = rng.integers(-3, 4, (B, M, D)).astype(np.float32)
    n, m = pair_lengths(N, M, B)
    want = []
    for b in range(B):
        want.append(DR.dtw(x[b, :n[b]], y[b, :m[b]], metric) if n[b] and m[b] else None)
        x[b, n[b]:] = np.nan
        y[b, m[b]:] = np.nan
    return dict(x=x, y=y, n=np.asarray(n, np.int32), m=np.asarray(m, np.int32), metric=metric, want=want, inst=inst)


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
            assert np.array_equal(path[b, :L], w['path']) and (path[b, L:] == -1).all(), b


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_lattice_equals_float64(dev, name):
    E = pkg().evaluate
    c = exact_case(name)
    t = lambda a: torch.from_numpy(a).to(dev)
    x, y, n, m = t(c['x']), t(c['y']), t(c['n']), t(c['m'])
    with traced() as tr:
        cost, length, path = E.dtw(x, y, n, m, metric=c['metric'], return_path=True)
    assert tr.names == {c['inst']}, tr.names
    assert cost.dtype == torch.float64 and length.dtype == torch.int32 and path.dtype == torch.int64
    assert path.shape == (x.shape[0], x.shape[1] + y.shape[1] - 1, 2)
    check_against(c, cost, length, path)
    cost2, length2 = E.dtw(x, y, n, m, metric=c['metric'])                      # without the path: same figures
    assert torch.equal(cost2.nan_to_num(-1), cost.nan_to_num(-1)) and torch.equal(length2, length)
    again = E.dtw(x, y, n, m, metric=c['metric'], return_path=True)              # two calls, the same bits
    assert torch.equal(again[0].nan_to_num(-1), cost.nan_to_num(-1)) and torch.equal(again[2], path)


@pytest.mark.parametrize('metric', DR.METRICS)
def test_all_metrics_on_one_lattice_and_a_single_pair(dev, metric):
    E = pkg().evaluate
    rng = np.random.default_rng(3)
    D = 1 if metric == 'l2' else 7
    x, y = rng.integers(-3, 4, (50, D)).astype(np.float32), rng.integers(-3, 4, (77, D)).astype(np.float32)
    w = DR.dtw(x, y, metric)
    cost, length, path = E.dtw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), metric=metric, return_path=True)
    assert cost.shape == () and length.shape == () and path.shape == (126, 2)
    assert float(cost) == w['cost'] and int(length) == w['length'] and np.array_equal(path[:w['length']].cpu().numpy(), w['path'])


def test_strided_views_with_nan_in_the_spare_elements(dev):
    E = pkg().evaluate
    c = exact_case('129x64')
    B, N, D = c['x'].shape
    M = c['y'].shape[1]
    wx = torch.full((2 * B, N + 2, D + 3), NAN, device=dev)
    wy = torch.full((B, M + 1, D + 5), NAN, device=dev)
    wx[::2, 1:1 + N, :D] = torch.from_numpy(c['x']).to(dev)
    wy[:, 1:, :D] = torch.from_numpy(c['y']).to(dev)
    vx, vy = wx[::2, 1:1 + N, :D], wy[:, 1:, :D]
    assert not vx.is_contiguous() and vx.stride() == (2 * (N + 2) * (D + 3), D + 3, 1)
    n, m = torch.from_numpy(c['n']).to(dev), torch.from_numpy(c['m']).to(dev)
    cost, length, path = E.dtw(vx, vy, n, m, metric=c['metric'], return_path=True)
    check_against(c, cost, length, path)
    assert bool(torch.isnan(wx[1::2]).all())                                       # nothing was written to the inputs


def raw_dtw(dev, c, cost, length, path, path_bs, *, B=None, N=None, M=None, D=None, metric=None, ws='query', nulls=(), x_fs=None,
            y_fs=None, x_bs=None):
    """tdvc_dtw through ctypes on device copies of case c; returns the status code."""
    L = pkg()._lib
    lib = L.lib()
    xb, xn, xd = c['x'].shape
    B, N, D = xb if B is None else B, xn if N is None else N, xd if D is None else D
    M = c['y'].shape[1] if M is None else M
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ('x', 'y', 'n', 'm')}
    t.update(cost=cost, length=length, path=path)
    ptr = lambda k: None if (k in nulls or t[k] is None) else t[k].data_ptr()
    if ws == 'query':
        nbytes = lib.tdvc_dtw_workspace(max(B, 1), max(min(N, 4096), 1), max(min(M, 4096), 1), int(path is not None))
        ws = (torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes)
    buf, nbytes = ws
    rc = lib.tdvc_dtw(ptr('x'), xn * xd if x_bs is None else x_bs, xd if x_fs is None else x_fs, ptr('y'), c['y'].shape[1] * xd,
                      xd if y_fs is None else y_fs, ptr('n'), ptr('m'), B, N, M, D,
                      {'l2': 0, 'l1': 1, 'sq': 2}[c['metric']] if metric is None else metric, ptr('cost'), ptr('length'), ptr('path'), path_bs,
                      None if buf is None else buf.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_raw_abi_strided_path_null_lengths_and_poisoned_lds(dev):
    """Path rows 2 (N + M - 1) + 6 apart, the elements between them untouched; NULL lengths mean full pairs; the same call after
    every CU's LDS has been filled with NaN bit patterns: a read of LDS the kernel has not written would change the result."""
    L = pkg()._lib
    for name in ('64x65', '700x5'):
        c = exact_case(name)
        B, N, _ = c['x'].shape
        M = c['y'].shape[1]
        P = 2 * (N + M - 1)
        outs = []
        for poison in (False, True):
            if poison:
                L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
            cost = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
            length = torch.full((B,), -7, dtype=torch.int32, device=dev)
            path = torch.full((B, P + 6), -7, dtype=torch.int32, device=dev)
            assert raw_dtw(dev, c, cost, length, path, P + 6) == 0
            assert bool((path[:, P:] == -7).all())
            for b, w in enumerate(c['want']):
                if w is None:                                                      # an empty pair: cost NaN, length 0, nothing else touched
                    assert bool(torch.isnan(cost[b])) and int(length[b]) == 0 and bool((path[b] == -7).all())
                else:
                    Lw = w['length']
                    assert float(cost[b]) == w['cost'] and int(length[b]) == Lw
                    assert np.array_equal(path[b, :2 * Lw].view(Lw, 2).cpu().numpy(), w['path']) and bool((path[b, 2 * Lw:P] == -1).all())
            outs.append((cost, length, path))
        assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][1], outs[1][1])
    c = exact_case('63x64')
    full = dict(c, x=np.nan_to_num(c['x']), y=np.nan_to_num(c['y']))
    B, N, _ = c['x'].shape
    M = c['y'].shape[1]
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    assert raw_dtw(dev, full, cost, length, None, 0, nulls=('n', 'm')) == 0
    for b in range(B):
        w = DR.dtw(full['x'][b], full['y'][b], c['metric'])
        assert float(cost[b]) == w['cost'] and int(length[b]) == w['length']


# ------------------------------------------------------------------------------------------------------------ real-valued pairs
REAL = {'200x150': (200, 150), '900x700': (900, 700)}
D_REAL = 25
EPS = (D_REAL + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def real_case(name):
    n, m = REAL[name]
    x, y = DR.warped_pair(np.random.default_rng(n + m), n, m, D_REAL)
    return x, y, {metric: DR.dtw(x, y, metric) for metric in (DR.METRICS if name == '200x150' else ('l2',))}


@pytest.mark.parametrize('name', sorted(REAL))
def test_real_valued_pair_within_the_rounding_bound(dev, name):
    E = pkg().evaluate
    x, y, want = real_case(name)
    n, m = len(x), len(y)
    for metric, w in want.items():
        cost, length, path = E.dtw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), metric=metric, return_path=True)
        cost, length, path = float(cost), int(length), path.cpu().numpy()
        p = path[:length]
        rescored = DR.score(p, x, y, metric)
        ref_cells = {tuple(cell) for cell in w['path']}
        off = sum(tuple(cell) not in ref_cells for cell in p)
        print(f'\ndtw {name} {metric}: C* {w["cost"]:.6f}, |cost - C*| {abs(cost - w["cost"]):.3e}, re-scored path gap {rescored - w["cost"]:.3e}, '
              f'bound {2 * EPS * w["cost"]:.3e}, cells off the float64 path {off} of {length}')
        assert DR.is_warping_path(p, n, m) and (path[length:] == -1).all()
        assert abs(cost - w['cost']) <= 2 * EPS * w['cost']
        assert rescored <= w['cost'] * (1 + 2 * EPS)


# ------------------------------------------------------------------------------------------------------------ tdvc_sp2mc
#          n_fft  order alpha  B  F
SP2MC = [(64,   0,  0.42, 2, 3), (64,   4,  0.42, 1, 1), (512,  24, 0.35, 2, 4), (1024, 24, 0.42, 2, 5), (1024, 34, 0.42, 1, 1),
         (2048, 34, 0.55, 1, 3), (2048, 4,  0.42, 2, 2)]
FLOOR = float(np.float32(1e-6))


@pytest.mark.parametrize('n_fft,order,alpha,B,F', SP2MC)
def test_sp2mc_both_layouts_and_the_floor(dev, n_fft, order, alpha, B, F):
    E = pkg().evaluate
    nb = n_fft // 2 + 1
    rng = np.random.default_rng(n_fft + order)
    p = np.exp(rng.standard_normal((B, F, nb)) * 2 - 3).astype(np.float32)
    p[:, :, ::7] = 1e-9                                                          # under the floor
    p[0, 0, 5] = 0.0
    assert (p < FLOOR).any() and (p > FLOOR).any()
    want = MR.sp2mc(p, order, alpha, FLOOR)
    tol = 4 * 2.0 ** -24 * np.abs(want).max(-1, keepdims=True)
    fn = torch.from_numpy(p).to(dev)
    got = E.sp2mc(fn, order, alpha, FLOOR)                                       # [B, F, nb]: a WORLD envelope's layout
    assert got.shape == (B, F, order + 1) and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert (err <= tol).all(), float((err / tol).max())
    wide = torch.full((B, nb + 3, 2 * F + 1), NAN, device=dev)                   # [B, nb, F] inside a larger buffer: the conv STFT's layout
    wide[:, :nb, 1::2] = fn.transpose(1, 2)
    got_nf = E.sp2mc(wide[:, :nb, 1::2], order, alpha, FLOOR, layout='nf')
    assert torch.equal(got_nf, got)
    assert torch.equal(E.sp2mc(fn[0], order, alpha, FLOOR), got[0])              # [F, nb]


# ------------------------------------------------------------------------------------------------------------ mel_cepstrum
def tones_in_noise(rng, T):
    t = np.arange(T) / 16000.0
    x = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in ((0.3, 220.0, 0.1), (0.2, 1330.0, 1.0), (0.1, 3105.0, 2.0), (0.05, 6150.0, 0.5)))
    return (x + 0.05 * rng.standard_normal(T)).astype(np.float32)                # a noise floor: no bin far under the frame's energy


def test_mel_cepstrum_end_to_end(dev):
    """Reference: the float64 chain from the same fp32 signal. Error measure: max over elements of |mc - ref| / max |ref of that frame|.
    The bar is 4 x what a plain numpy fp32 evaluation of the same windowed-DFT formulation shows on this input.
    Measured on an MI355X: device error 4.383e-06, numpy fp32 error 4.253e-06, ratio 1.03."""
    E = pkg().evaluate
    rng = np.random.default_rng(17)
    T, n_fft, hop, order, alpha = 2400, 1024, 80, 24, 0.42
    x = np.stack([tones_in_noise(rng, T), 0.1 * tones_in_noise(rng, T)])
    floor = float(np.float32(E.POWER_FLOOR))
    ref = np.stack([MR.mel_cepstrum(r, n_fft, hop, order, alpha, floor) for r in x])
    f32 = np.stack([MR.mel_cepstrum(r, n_fft, hop, order, alpha, floor, np.float32) for r in x])
    scale = np.abs(ref).max(-1, keepdims=True)
    bar = 4 * float((np.abs(f32 - ref) / scale).max())
    got = E.mel_cepstrum(torch.from_numpy(x)[:, None].to(dev), n_fft=n_fft, hop=hop, order=order, alpha=alpha)
    assert got.shape == (2, 1 + T // hop, order + 1) and got.dtype == torch.float32
    err = float((np.abs(got.cpu().numpy().astype(np.float64) - ref) / scale).max())
    print(f'\nmel_cepstrum: device error {err:.3e}, numpy fp32 error {bar / 4:.3e}, ratio {err / (bar / 4):.2f} (bar 4)')
    assert err <= bar
    mc, nfr = E.mel_cepstrum(torch.from_numpy(x)[:, None].to(dev), lengths=torch.tensor([T, 801], device=dev))
    assert torch.equal(mc, got) and nfr.tolist() == [1 + T // hop, 11] and nfr.dtype == torch.int32


# ------------------------------------------------------------------------------------------------------------ mcd
def vowel(rng, T, f0, sr=16000):
    """A harmonic tone under a fixed formant-like envelope with a slow vibrato, a little noise; 0.1 s of near-silence at either end."""
    t = np.arange(T) / sr
    phase = 2 * np.pi * np.cumsum(f0 * (1 + 0.03 * np.sin(2 * np.pi * 3.0 * t))) / sr
    x = sum(np.sin(h * phase) / (1 + ((h * f0 - 700.0) / 400.0) ** 2) for h in range(1, 20))
    x = 0.05 * x + 0.001 * rng.standard_normal(T)
    x[:sr // 10] *= 0.001
    x[-sr // 10:] *= 0.001
    return x.astype(np.float32)


def test_mcd_identical_signals_and_too_few_voiced_frames(dev):
    P = pkg()
    rng = np.random.default_rng(4)
    T = 9600
    v = vowel(rng, T, 140.0)
    noise = (0.01 * rng.standard_normal(T)).astype(np.float32)
    test = torch.from_numpy(np.stack([v, noise, v]))[:, None].to(dev)
    ref = torch.from_numpy(np.stack([v, v, noise]))[:, None].to(dev)
    r = P.mcd(test, ref)
    assert set(r) == {'mcd', 'path_len', 'n_test', 'n_ref', 'diff_f0_mean', 'diff_f0_var', 'f0_ratio'}
    assert all(t.shape == (3,) and t.dtype == torch.float64 for t in r.values())
    f0 = P.yin_f0(test[:1, 0], 16000, 50, 500, 0.005)
    nv = int((f0[0, :T // 80] > 0).sum())
    assert nv > 50
    assert float(r['mcd'][0]) == 0.0 and int(r['path_len'][0]) == nv and int(r['n_test'][0]) == nv and int(r['n_ref'][0]) == nv
    assert float(r['diff_f0_mean'][0]) == 0.0 and float(r['f0_ratio'][0]) == 1.0
    for b in (1, 2):                                                              # fewer than 10 voiced frames on the test / the reference side
        assert all(bool(torch.isnan(t[b])) for t in r.values()), {k: float(t[b]) for k, t in r.items()}


def test_mcd_f0_statistics_db_variant_and_caller_tracks(dev):
    P = pkg()
    rng = np.random.default_rng(8)
    T1, T2 = 9600, 8000
    a, b = vowel(rng, T1, 120.0), vowel(rng, T2, 180.0)
    test = torch.zeros(2, 1, T1, device=dev)
    test[0, 0] = torch.from_numpy(a).to(dev)
    test[1, 0, :T2] = torch.from_numpy(b).to(dev)
    ref = torch.zeros(2, 1, T1, device=dev)
    ref[0, 0, :T2] = torch.from_numpy(b).to(dev)
    ref[1, 0] = torch.from_numpy(a).to(dev)
    tl, rl = torch.tensor([T1, T2], device=dev), torch.tensor([T2, T1], device=dev)
    r = P.mcd(test, ref, tl, rl)
    ft = P.yin_f0(test[:, 0], 16000, 50, 500, 0.005).cpu().numpy().astype(np.float64)
    fr = P.yin_f0(ref[:, 0], 16000, 50, 500, 0.005).cpu().numpy().astype(np.float64)
    for i, (lt, lr) in enumerate(((T1, T2), (T2, T1))):
        vt, vr = ft[i, :(lt + 79) // 80], fr[i, :(lr + 79) // 80]
        vt, vr = vt[vt > 0], vr[vr > 0]
        assert int(r['n_test'][i]) == len(vt) and int(r['n_ref'][i]) == len(vr) and len(vt) > 50 and len(vr) > 50
        want = dict(diff_f0_mean=np.mean(np.log(vt)) - np.mean(np.log(vr)), diff_f0_var=np.log(np.var(vt)) - np.log(np.var(vr)),
                    f0_ratio=np.mean(vr) / np.mean(vt))
        for k, w in want.items():
            assert abs(float(r[k][i]) - w) <= 1e-12 * max(1.0, abs(w)), (i, k, float(r[k][i]), w)
        assert max(len(vt), len(vr)) <= int(r['path_len'][i]) <= len(vt) + len(vr) - 1 and float(r['mcd'][i]) > 0
    assert abs(float(r['f0_ratio'][0]) - 1.5) < 0.05 and abs(float(r['f0_ratio'][1]) - 1 / 1.5) < 0.05
    # the same pair the other way round: the same optimal cost (the paths may differ where the tie rule decides)
    assert abs(float(r['mcd'][0] * r['path_len'][0]) - float(r['mcd'][1] * r['path_len'][1])) <= 1e-6 * float(r['mcd'][0] * r['path_len'][0])
    # the caller's own tracks, and the conventional MCD in dB without c0
    f0t, f0r = torch.from_numpy(ft).float().to(dev), torch.from_numpy(fr).float().to(dev)
    r2 = P.mcd(test, ref, tl, rl, f0_test=f0t, f0_ref=f0r)
    assert all(torch.equal(r2[k], r[k]) for k in r)
    rdb = P.mcd(test, ref, tl, rl, drop_c0=True, db=True)
    mc_t, mc_r = P.mel_cepstrum(test), P.mel_cepstrum(ref)
    F = ft.shape[1]
    sel = lambda mc, f, ln: mc[:F][(f > 0) & (np.arange(F) < (ln + 79) // 80)]
    w = DR.dtw(sel(mc_t[0].cpu().numpy(), ft[0], T1)[:, 1:], sel(mc_r[0].cpu().numpy(), fr[0], T2)[:, 1:], 'l2')
    want_db = 10 / np.log(10) * np.sqrt(2) * w['cost'] / w['length']
    assert abs(float(rdb['mcd'][0]) - want_db) <= 1e-5 * want_db


def test_mcd_under_graph_capture(dev):
    """No component synchronises with the host: once the caches are warm (STFT basis, cepstrum matrix, allocator) the whole call is
    captured into a graph, and a replay follows its inputs."""
    P = pkg()
    rng = np.random.default_rng(12)
    T = 6400
    test = torch.from_numpy(vowel(rng, T, 130.0))[None, None].to(dev)
    ref = torch.from_numpy(vowel(rng, T, 160.0))[None, None].to(dev)
    tl = torch.tensor([T], device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        P.mcd(test, ref, tl, tl)                                                  # warm-up
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = P.mcd(test, ref, tl, tl)
    graph.replay()
    torch.cuda.synchronize(dev)
    eager = P.mcd(test, ref, tl, tl)
    assert all(torch.equal(r[k], eager[k]) for k in r) and float(r['mcd'][0]) > 0
    ref.copy_(test)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert float(r['mcd'][0]) == 0.0


# ------------------------------------------------------------------------------------------------------------ refusals
def test_dtw_refusals_before_any_launch(dev):
    L = pkg()._lib
    lib = L.lib()
    c = exact_case('64x65')
    B, N, D = c['x'].shape
    M = c['y'].shape[1]
    P = 2 * (N + M - 1)
    cost = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    length = torch.full((B,), -7, dtype=torch.int32, device=dev)
    path = torch.full((B, P), -7, dtype=torch.int32, device=dev)
    nbytes = lib.tdvc_dtw_workspace(B, N, M, 1)
    assert nbytes >= B * M * 12 + B * N * ((M + 15) // 16) * 4 and lib.tdvc_dtw_workspace(B, N, M, 0) >= B * M * 12
    wsbuf = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    ws = (wsbuf, nbytes)
    cases = [
        (dict(B=-1), EINVAL), (dict(N=0), EINVAL), (dict(M=0), EINVAL), (dict(D=0), EINVAL), (dict(N=-4), EINVAL),
        (dict(metric=3), EINVAL), (dict(metric=-1), EINVAL), (dict(x_fs=D - 1), EINVAL), (dict(y_fs=0), EINVAL), (dict(x_bs=-1), EINVAL),
        (dict(path_bs=P - 1), EINVAL), (dict(path_bs=-1), EINVAL),
        (dict(nulls=('x',)), EINVAL), (dict(nulls=('y',)), EINVAL), (dict(nulls=('cost',)), EINVAL), (dict(nulls=('length',)), EINVAL),
        (dict(N=4097, path_bs=20000), EUNSUPPORTED), (dict(M=4097, path_bs=20000), EUNSUPPORTED), (dict(D=65, x_fs=65, y_fs=65), EUNSUPPORTED),
        (dict(ws=(None, nbytes)), EWORKSPACE), (dict(ws=(wsbuf, nbytes - 1)), EWORKSPACE), (dict(ws=(wsbuf, 0)), EWORKSPACE),
    ]
    with traced() as tr:
        for kw, want in cases:
            kw = {'ws': ws, 'path_bs': P, **kw}
            path_bs = kw.pop('path_bs')
            rc = raw_dtw(dev, c, cost, length, path, path_bs, **kw)
            assert rc == want, (kw.keys(), rc, want)
            assert lib.tdvc_last_error()
            assert bool((path == -7).all()) and bool((cost == -7).all()) and bool((length == -7).all()) and bool((wsbuf == 0x5A).all()), kw.keys()
        assert raw_dtw(dev, c, cost, length, path, P, B=0, ws=ws) == 0           # a no-op
        assert bool((path == -7).all()) and bool((wsbuf == 0x5A).all())
    assert tr.names == set()
    assert lib.tdvc_dtw_workspace(B, 4097, M, 1) == 0 and lib.tdvc_dtw_workspace(B, N, 0, 0) == 0 and lib.tdvc_dtw_workspace(0, N, M, 0) == 0
    assert raw_dtw(dev, c, cost, length, path, P, ws=ws) == 0                      # and the same buffers do work
    check_against(c, cost, length)


def test_sp2mc_refusals_before_any_launch(dev):
    L = pkg()._lib
    lib = L.lib()
    nb, order, B, F = 33, 4, 2, 3
    p = torch.ones(B, F, nb, device=dev)
    mat = torch.zeros(order + 1, nb, dtype=torch.float64, device=dev)
    mc = torch.full((B, F, order + 1), -7.0, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(B=B, F=F, nb=nb, order=order, floor=1e-6, strides=(F * nb, nb, 1), p_=p, mat_=mat, mc_=mc):
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = lib.tdvc_sp2mc(ptr(p_), *strides, ptr(mat_), B, F, nb, order, floor, ptr(mc_), st)
        torch.cuda.synchronize()
        return rc
    cases = [(dict(B=-1), EINVAL), (dict(F=-1), EINVAL), (dict(nb=1), EINVAL), (dict(order=-1), EINVAL), (dict(order=nb), EINVAL),
             (dict(floor=0.0), EINVAL), (dict(floor=-1.0), EINVAL), (dict(floor=NAN), EINVAL), (dict(floor=float('inf')), EINVAL),
             (dict(strides=(-1, nb, 1)), EINVAL), (dict(strides=(F * nb, nb, -1)), EINVAL),
             (dict(p_=None), EINVAL), (dict(mat_=None), EINVAL), (dict(mc_=None), EINVAL),
             (dict(nb=2050, order=4), EUNSUPPORTED), (dict(nb=1025, order=256), EUNSUPPORTED)]
    for kw, want in cases:
        assert call(**kw) == want, (kw, want)
        assert lib.tdvc_last_error() and bool((mc == -7).all())
    assert call(B=0) == 0 and call(F=0) == 0 and bool((mc == -7).all())
    assert call() == 0 and bool((mc == 0).all())                                   # a zero matrix: every coefficient 0


def test_python_refusals(dev):
    P = pkg()
    E = P.evaluate
    x = torch.zeros(2, 10, 3, device=dev)
    with pytest.raises(RuntimeError):
        E.dtw(x.cpu(), x.cpu())                                                    # there is no CPU fallback
    with pytest.raises(ValueError):
        E.dtw(x, x, metric='cosine')
    with pytest.raises(ValueError):
        E.dtw(x, x[:, :, :2])
    with pytest.raises(ValueError):
        E.dtw(x, x, x_len=torch.tensor([3], device=dev))
    with pytest.raises(RuntimeError):
        E.dtw(torch.zeros(1, 4097, 1, device=dev), torch.zeros(1, 5, 1, device=dev))      # TDVC_EUNSUPPORTED from the library
    with pytest.raises(ValueError):
        E.mel_cepstrum(torch.zeros(2, 2, 4000, device=dev))
    with pytest.raises(ValueError):
        E.sp2mc(torch.ones(2, 3, 33, device=dev), layout='xy')
    with pytest.raises(ValueError):
        P.mcd(torch.zeros(2, 1, 4000, device=dev), torch.zeros(3, 1, 4000, device=dev))
    assert P.dtw is E.dtw and P.mcd is E.mcd and P.f0_stats is E.f0_stats and P.mel_cepstrum is E.mel_cepstrum
