"""GPU: the composed call mcd(test, ref, test_len, ref_len, f0_method='dio', envelope='cheaptrick', align='fastdtw') from the waveform
to the number, against the float64 chain tests/mcd_world_ref.py (dio_ref -> one fp32 rounding -> cheaptrick_ref -> mc_from_c ->
the frames with f0 > 0 -> fastdtw_ref -> cost / length, the F0 statistics). tests/test_mcd_world_cpu.py shows that chain fit on
exactly these rows: stable DIO decisions, a well-conditioned CheapTrick, no half-width ties, FastDTW margins of 4 and more. Every
kernel in the call has its own float64 test; what is held to account here is the glue of evaluate._voiced_cepstra and `mcd`: frame
validity from the lengths, frame f of the cepstra being frame f of the track, compact_voiced, the counts handed to `fastdtw`,
cost / length and the min_voiced gate. pyworld, pysptk and fastdtw are not available: nothing here is a parity test against them.

The five pairs of mcd_world_ref.PAIRS sit in one padded buffer per side, [5, 1, 8000 + 24] as a view of a wider one, NaN at and past
every length, lengths as device int32. Pair A has two lengths that are multiples of the hop with the last frame voiced on both sides
(the frame centred on sample `length` counts: WORLD's 1 + length // hop frames), B differs between exact, radius 1 and radius 2, C has
the shorter side first, D has 1 voiced frame on the test side (NaN), E has a length that is no multiple of the hop.

1. Every entry of every pair but D is finite (nothing at or past a length was read), every entry of D is NaN.
2. n_test and n_ref equal the chain's counts, and the voiced sets of the device's world_f0 are the chain's.
3. The call rebuilt from world_f0, mel_cepstrum(envelope='cheaptrick', f0=, lengths=), the WORLD frame set, compact_voiced,
   fastdtw(return_path=True) and f0_stats gives mcd's entries bit for bit; compact_voiced equals numpy's boolean indexing of the
   device cepstra with NaN behind the count; the statistics equal numpy's on the device track within 1e-12 (test_mcd_gpu.py).
4. The compacted device cepstra against cheaptrick_ref -> mc_from_c on the device's OWN fp32 track, frame by frame after compaction:
   4 * 2^-24 * max |mc64 of that frame| (test_cheaptrick_gpu.py). A shift of one frame between track and cepstra fails here.
5. fastdtw_ref on the device's own fp32 compacted cepstra: its margin ratio there is at least 1 (asserted) on pairs A, C and E, so
   path and length are identical and |cost - C_ref| <= 2 eps C_ref, eps = (25 + 2) 2^-24 (test_fastdtw_gpu.py). Pair B's margins are
   too small for that (1.69 on the chain's cepstra where the CPU test asks 4): it is held to the rule of test_fastdtw_gpu.py's
   900 x 700 pair instead: a valid warping path whose float64 re-score is the cost within 2 eps, not below the exact optimum.
6. The device path re-scored on the chain's float64 cepstra (dtw_ref.score): |mcd - score / length| <= e_cell, the error of one local
   distance as in test_cheaptrick_gpu.mcd_case: both frames within 4 * 2^-24 * max |mc| per element give 2 sqrt(D) of that, plus the
   fp32 evaluation of the distance, (D + 2) 2^-24 (d_max + that). Whether the chain's own path is the device's is printed, not
   asserted: near-ties between smooth cepstra make the reference's number discontinuous there.
7. Variants: on pair B exact < radius 2 < radius 1 as in the chain, the exact cost within (N + M - 1) e_cell of dtw_ref's; drop_c0=True,
   db=True against the rebuilt call (bits) and the chain's re-score with 10 / ln 10 * sqrt 2 (D = 24); min_voiced = 74 gives pair A's
   numbers, 75 NaN; dense rows without lengths give the bits of the call with len = T; two calls and a graph replay give the same bits.

Measured on an MI355X (printed by the tests, run with -s), the same at radius 1 and 2 except on pair B:
    pair  voiced    margin ratio on    |cost - C_ref|     mcd (device)   chain's cost / length   |mcd - re-score / length|
                    the device cepstra  over 2 eps C_ref                                          over e_cell (e_cell)
    A     79 / 74   8.44               0.003              1.751159955    1.751159974             0.0004 (1.61e-05)
    B r1  79 / 47   (loose rule) |cost - re-scored| 0.007 of 2 eps       2.033016585    2.033016632             0.0018 (1.78e-05)
    B r2  79 / 47   (loose rule) |cost - re-scored| 0.008 of 2 eps       2.024404563    2.024404617             0.0023 (1.78e-05)
    C     49 / 72   16.81              0.001              2.120911332    2.120911325             0.0014 (1.86e-05)
    E     57 / 74   7.14               0.002              1.589335319    1.589335329             0.0015 (1.56e-05)
    D     1 / 74    every entry NaN
The chain's own path was the device's on every pair, B included. The device's world_f0 track had the bits of the chain's fp32 track
on every row (0.000 of 4 * 2^-24); the compacted cepstra were within 0.242 of their bar (0.25 is the one rounding to fp32); the F0
statistics within 0.002 of the 1e-12 bar; pair B's costs exact 157.694710 (chain 157.694714), radius 2 159.927961 (159.927965),
radius 1 160.608310 (160.608314); pair A in dB without c0 10.155318132 against the re-score 10.155318277, 0.0023 of e_cell 6.20e-05.
With `mcd` counting the frames f * hop < length on this path, as it did before this file existed, assertion 2 fails on pair A:
n_test, n_ref = 78, 73 where the chain has 79, 74.
"""
import functools
import math

import numpy as np
import pytest
import torch

import dtw_ref as DR
import fastdtw_ref as FR
import mcd_world_ref as W
from common import pkg

pytestmark = pytest.mark.gpu
NAN = float('nan')
BAR = 4 * 2.0 ** -24
KW = dict(f0_method='dio', envelope='cheaptrick', align='fastdtw')
KEYS = ('mcd', 'path_len', 'n_test', 'n_ref', 'diff_f0_mean', 'diff_f0_var', 'f0_ratio')
DB = 10.0 / math.log(10.0) * math.sqrt(2.0)
LIVE = [b for b, p in enumerate(W.ORDERED) if p != 'D']
TAIL, LEAD = 24, 8


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def same_entries(a, b, rows=None):
    sel = (lambda v: v) if rows is None else (lambda v: v[rows])
    return set(a) == set(b) == set(KEYS) and all(bits_equal(sel(a[k]), sel(b[k])) for k in KEYS)


def padded(dev, names):
    """[B, 1, 8000 + 24] as a view of a wider buffer, NaN before it, behind it and at and past every length; lengths int32 [B]."""
    T = max(W.length_of(n) for n in W.ROWS) + TAIL
    buf = np.full((len(names), 1, LEAD + T + LEAD), np.nan, np.float32)
    for b, n in enumerate(names):
        buf[b, 0, LEAD:LEAD + W.length_of(n)] = W.waveform(n)[:W.length_of(n)]
    view = torch.from_numpy(buf).to(dev)[:, :, LEAD:LEAD + T]
    assert not view.is_contiguous() and view.shape == (len(names), 1, T)
    return view, torch.tensor([W.length_of(n) for n in names], dtype=torch.int32, device=dev)


def e_cell(mt, mr, D):
    """The error of one fp32 local distance between frames that are each within BAR * max |mc| per element of mt / mr (float64)."""
    e = 2 * np.sqrt(D) * BAR * max(np.abs(mt).max(), np.abs(mr).max())
    return e + (D + 2) * 2.0 ** -24 * (DR.distance(mt, mr, 'l2').max() + e)


def rebuilt(E, sides, radius, drop_c0=False, db=False):
    """mcd from the public operators -> (entries, path int64 [B, P, 2]); `sides` = two of side()'s results."""
    a, b = ((E.compact_voiced(s['mc_all'][:, :, 1:], s['f0v'] > 0)[0] if drop_c0 else s['mc']) for s in sides)
    (na, fa), (nb, fb) = ((s['count'], s['f0v']) for s in sides)
    cost, length, path = E.fastdtw(a, b, na, nb, radius=radius, metric='l2', return_path=True)
    out = dict(mcd=(DB if db else 1.0) * cost / length.double(), path_len=length.double(), n_test=na.double(), n_ref=nb.double(), **E.f0_stats(fa, fb))
    return out, path


def side(P, sig, lengths):
    """One side from the public operators: the track, the cepstra of every frame, WORLD's frame set, the compacted voiced frames."""
    E = P.evaluate
    f0 = P.world_f0(sig[:, 0], W.FS, W.HOP, 50.0, 500.0, lengths=lengths)
    mc_all, nfr = E.mel_cepstrum(sig, sample_rate=W.FS, hop=W.HOP, envelope='cheaptrick', f0=f0, lengths=lengths)
    assert mc_all.shape == (sig.shape[0], f0.shape[1], W.D) and nfr.tolist() == [1 + int(n) // W.HOP for n in lengths.tolist()]
    valid = torch.arange(f0.shape[1], device=sig.device)[None, :] < nfr[:, None]      # f * hop <= length
    f0v = torch.where(valid, f0, torch.zeros_like(f0))
    mc, count = E.compact_voiced(mc_all, f0v > 0)
    return dict(f0=f0, f0v=f0v, mc_all=mc_all, mc=mc, count=count)


@functools.lru_cache(maxsize=None)
def run(dev):
    """Everything the tests share, computed once: the buffers, one mcd call per radius, the rebuilt calls, host copies."""
    P = pkg()
    E = P.evaluate
    test, tl = padded(dev, [W.PAIRS[p][0] for p in W.ORDERED])
    ref, rl = padded(dev, [W.PAIRS[p][1] for p in W.ORDERED])
    got = {r: P.mcd(test, ref, tl, rl, radius=r, **KW) for r in W.RADII}
    sides = side(P, test, tl), side(P, ref, rl)
    re = {r: rebuilt(E, sides, r) for r in W.RADII}
    torch.cuda.synchronize(dev)
    host = lambda t: t.detach().cpu().numpy()
    return dict(test=test, ref=ref, tl=tl, rl=rl, got=got, sides=sides, rebuilt=re,
                h=[{k: host(v) for k, v in s.items()} for s in sides], hgot={r: {k: host(v) for k, v in g.items()} for r, g in got.items()},
                hpath={r: host(re[r][1]) for r in W.RADII})


def rows_of(b):
    return W.PAIRS[W.ORDERED[b]][:2]


def device_cepstra(k, b):
    """The compacted fp32 cepstra of pair b on the host: (test [n, D], ref [m, D])."""
    return tuple(k['h'][s]['mc'][b, :int(k['h'][s]['count'][b])] for s in (0, 1))


# ------------------------------------------------------------------------------------------------------------ 1, 2
def test_finite_where_a_result_is_due_and_nan_under_min_voiced(dev):
    k = run(dev)
    d = W.ORDERED.index('D')
    for r in W.RADII:
        g = k['hgot'][r]
        assert set(g) == set(KEYS) and all(v.shape == (len(W.ORDERED),) and v.dtype == np.float64 for v in g.values())
        for key in KEYS:
            assert np.isfinite(g[key][LIVE]).all(), (r, key, g[key])
            assert np.isnan(g[key][d]), (r, key, g[key][d])


def test_counts_and_voiced_sets_are_the_chains(dev):
    k = run(dev)
    for b, pair in enumerate(W.ORDERED):
        for s, name in enumerate(rows_of(b)):
            c = W.chain_of(name)
            f0 = k['h'][s]['f0'][b].astype(np.float64)
            Fb = len(c['f0'])
            assert Fb == 1 + W.length_of(name) // W.HOP and np.isfinite(f0).all() and (f0[Fb:] == 0).all(), (pair, name)
            assert np.array_equal(f0[:Fb] > 0, c['voiced']), (pair, name, np.nonzero((f0[:Fb] > 0) != c['voiced'])[0][:8])
            v = c['voiced']
            worst = float((np.abs(f0[:Fb] - c['f0'])[v] / (BAR * c['f0'][v])).max())
            print(f'\npair {pair} {name}: {int(v.sum())} voiced of {Fb} frames, last frame voiced {bool(v[-1])}; device track against the chain\'s '
                  f'{worst:.3f} of 4 * 2^-24 relative (printed, not asserted: test_dio_gpu.py holds world_f0 to its bar)')
            assert int(k['h'][s]['count'][b]) == int(v.sum()), (pair, name)
        if pair == 'D':
            continue
        for r in W.RADII:
            g = k['hgot'][r]
            want = (int(W.chain_of(rows_of(b)[0])['voiced'].sum()), int(W.chain_of(rows_of(b)[1])['voiced'].sum()))
            assert (g['n_test'][b], g['n_ref'][b]) == want, (pair, r, g['n_test'][b], g['n_ref'][b], want)


# ------------------------------------------------------------------------------------------------------------ 3
def test_mcd_is_its_public_operators_bit_for_bit(dev):
    k = run(dev)
    for r in W.RADII:
        assert same_entries(k['got'][r], k['rebuilt'][r][0], LIVE), r
    for s in (0, 1):
        h = k['h'][s]
        B, F, D = h['mc_all'].shape
        for b in range(B):
            want = h['mc_all'][b][h['f0v'][b] > 0]
            n = int(h['count'][b])
            assert n == len(want) and np.array_equal(h['mc'][b, :n].view(np.uint32), want.view(np.uint32)), (s, b)
            assert np.isnan(h['mc'][b, n:]).all() and h['mc'].shape == (B, F, D), (s, b)
    worst = 0.0
    for b in LIVE:
        want = W.f0_statistics(k['h'][0]['f0v'][b].astype(np.float64), k['h'][1]['f0v'][b].astype(np.float64))
        for key, w in want.items():
            got = float(k['hgot'][1][key][b])
            worst = max(worst, abs(got - w) / (1e-12 * max(1.0, abs(w))))
            assert abs(got - w) <= 1e-12 * max(1.0, abs(w)), (b, key, got, w)
    print(f'\nF0 statistics against numpy on the device track: {worst:.3f} of the 1e-12 bar')


# ------------------------------------------------------------------------------------------------------------ 4
def test_compacted_cepstra_against_float64_on_the_device_track(dev):
    k = run(dev)
    worst = 0.0
    for b, pair in enumerate(W.ORDERED):
        for s, name in enumerate(rows_of(b)):
            h = k['h'][s]
            frames = np.nonzero(h['f0v'][b] > 0)[0]
            want = W.cepstra(name, h['f0'][b], frames)
            got = h['mc'][b, :len(frames)].astype(np.float64)
            assert np.isfinite(got).all(), (pair, name)
            ratio = np.abs(got - want) / (BAR * np.abs(want).max(-1, keepdims=True))
            assert (ratio <= 1).all(), (pair, name, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
            worst = max(worst, float(ratio.max()))
    print(f'\ncompacted device cepstra against cheaptrick_ref on the device track: worst error over its bar {worst:.3f}')


# ------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize('radius', W.RADII)
def test_alignment_against_fastdtw_ref_on_the_device_cepstra(dev, radius):
    k = run(dev)
    for b, pair in enumerate(W.ORDERED):
        if pair == 'D':
            continue
        x, y = device_cepstra(k, b)
        w = FR.fastdtw(x, y, radius, 'l2')
        g = k['hgot'][radius]
        length, path = int(g['path_len'][b]), k['hpath'][radius][b]
        cost = float(g['mcd'][b]) * length
        assert (path[length:] == -1).all(), pair
        if radius in W.PAIRS[pair][3]:
            ratio = W.margin_ratio(w)
            print(f'\npair {pair} radius {radius}: margin ratio on the device cepstra {ratio:.2f}, C_ref {w["cost"]:.6f}, '
                  f'|cost - C_ref| over 2 eps C_ref {abs(cost - w["cost"]) / (2 * W.EPS * w["cost"]):.3f}')
            assert ratio >= 1, (pair, radius, ratio)
            assert length == w['length'] and np.array_equal(path[:length], w['path']), pair
            assert abs(cost - w['cost']) <= 2 * W.EPS * w['cost'], pair
        else:
            p = path[:length]
            rescored, exact = DR.score(p, x, y, 'l2'), DR.dtw(x, y, 'l2')['cost']
            print(f'\npair {pair} radius {radius} (no path identity): C_ref {w["cost"]:.6f}, cost {cost:.6f}, exact {exact:.6f}, '
                  f'|cost - re-scored| over 2 eps {abs(cost - rescored) / (2 * W.EPS * rescored):.3f}, the reference\'s path {np.array_equal(p, w["path"])}')
            assert DR.is_warping_path(p, len(x), len(y)), pair
            assert abs(cost - rescored) <= 2 * W.EPS * rescored and cost >= exact * (1 - 2 * W.EPS), pair


# ------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize('radius', W.RADII)
def test_the_number_against_the_pure_chain(dev, radius):
    k = run(dev)
    for b, pair in enumerate(W.ORDERED):
        if pair == 'D':
            continue
        mt, mr = (W.chain_of(n)['mc'] for n in rows_of(b))
        g = k['hgot'][radius]
        length = int(g['path_len'][b])
        path = k['hpath'][radius][b, :length]
        assert DR.is_warping_path(path, len(mt), len(mr)), pair
        want, bound = DR.score(path, mt, mr, 'l2') / length, e_cell(mt, mr, W.D)
        chain = W.pipeline_of(pair, radius)
        print(f'\npair {pair} radius {radius}: mcd {float(g["mcd"][b]):.9f}, the chain\'s cost / length {chain["mcd"]:.9f}, the chain\'s path is the '
              f'device\'s: {np.array_equal(path, chain["path"])}; |mcd - re-score / length| {abs(float(g["mcd"][b]) - want):.3e}, '
              f'{abs(float(g["mcd"][b]) - want) / bound:.4f} of e_cell {bound:.3e}')
        assert abs(float(g['mcd'][b]) - want) <= bound, pair


# ------------------------------------------------------------------------------------------------------------ 7
def test_exact_radius_1_and_radius_2_differ_as_the_chains_do(dev):
    P = pkg()
    k = run(dev)
    b = W.ORDERED.index('B')
    exact = P.mcd(k['test'], k['ref'], k['tl'], k['rl'], **{**KW, 'align': 'exact'})
    ce = float(exact['mcd'][b] * exact['path_len'][b])
    c1, c2 = (float(k['hgot'][r]['mcd'][b] * k['hgot'][r]['path_len'][b]) for r in (1, 2))
    w1, w2, we = W.pipeline_of('B', 1), W.pipeline_of('B', 2), W.exact_of('B')
    print(f'\npair B costs: exact {ce:.6f} (chain {we["cost"]:.6f}), radius 2 {c2:.6f} (chain {w2["cost"]:.6f}), radius 1 {c1:.6f} (chain {w1["cost"]:.6f})')
    assert we['cost'] < w2['cost'] < w1['cost'] and ce < c2 < c1
    mt, mr = (W.chain_of(n)['mc'] for n in rows_of(b))
    assert int(exact['path_len'][b]) == we['length'] and abs(ce - we['cost']) <= (len(mt) + len(mr) - 1) * e_cell(mt, mr, W.D)
    for key in ('n_test', 'n_ref', 'diff_f0_mean', 'diff_f0_var', 'f0_ratio'):
        assert bits_equal(exact[key], k['got'][1][key]), key


def test_drop_c0_and_db_against_the_rebuilt_call_and_the_chain(dev):
    P = pkg()
    k = run(dev)
    got = P.mcd(k['test'], k['ref'], k['tl'], k['rl'], drop_c0=True, db=True, **KW)
    re, path = rebuilt(P.evaluate, k['sides'], 1, drop_c0=True, db=True)
    assert same_entries(got, re, LIVE) and bool(torch.isnan(got['mcd'][W.ORDERED.index('D')]))
    b = W.ORDERED.index('A')
    mt, mr = (W.chain_of(n)['mc'][:, 1:] for n in rows_of(b))
    length = int(got['path_len'][b])
    p = path[b, :length].cpu().numpy()
    want, bound = DB * DR.score(p, mt, mr, 'l2') / length, DB * e_cell(mt, mr, W.D - 1)
    print(f'\npair A in dB without c0: mcd {float(got["mcd"][b]):.9f}, re-score {want:.9f}, difference {abs(float(got["mcd"][b]) - want) / bound:.4f} of e_cell {bound:.3e}')
    assert DR.is_warping_path(p, len(mt), len(mr)) and abs(float(got['mcd'][b]) - want) <= bound
    assert not bits_equal(got['mcd'][LIVE], k['got'][1]['mcd'][LIVE])


def test_min_voiced_gate_sits_on_the_smaller_count(dev):
    P = pkg()
    k = run(dev)
    b = W.ORDERED.index('A')
    n = min(int(W.chain_of(name)['voiced'].sum()) for name in rows_of(b))
    at, over = (P.mcd(k['test'], k['ref'], k['tl'], k['rl'], min_voiced=m, **KW) for m in (n, n + 1))
    for key in KEYS:
        assert bits_equal(at[key][b:b + 1], k['got'][1][key][b:b + 1]) and bool(torch.isfinite(at[key][b])), key
        assert bool(torch.isnan(over[key][b])), key


@pytest.mark.parametrize('pair', ('A', 'C'))
def test_dense_rows_without_lengths_equal_lengths_of_T(dev, pair):
    P = pkg()
    t, r = (torch.from_numpy(W.waveform(n)[:W.length_of(n)].copy()).to(dev)[None, None] for n in W.PAIRS[pair][:2])
    tl, rl = (torch.tensor([s.shape[-1]], dtype=torch.int32, device=dev) for s in (t, r))
    assert t.shape[-1] % W.HOP == 0 == r.shape[-1] % W.HOP
    plain, given = P.mcd(t, r, **KW), P.mcd(t, r, tl, rl, **KW)
    assert same_entries(plain, given) and bool(torch.isfinite(plain['mcd']).all())
    assert int(plain['n_test'][0]) == int(W.chain_of(W.PAIRS[pair][0])['voiced'].sum())


def test_two_calls_and_a_graph_replay_give_the_same_bits(dev):
    P = pkg()
    k = run(dev)
    call = lambda: P.mcd(k['test'], k['ref'], k['tl'], k['rl'], **KW)
    assert same_entries(call(), k['got'][1])
    side_stream = torch.cuda.Stream(dev)
    side_stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side_stream):
        call()                                                                 # warm-up
    torch.cuda.current_stream(dev).wait_stream(side_stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = call()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert same_entries(r, k['got'][1])
    first = {key: v.clone() for key, v in r.items()}
    graph.replay()
    torch.cuda.synchronize(dev)
    assert same_entries(r, first)
