"""CPU: what tests/test_mcd_world_gpu.py assumes of its reference. The float64 chain of tests/mcd_world_ref.py (dio_ref ->
cheaptrick_ref -> mc_from_c -> fastdtw_ref) is a fit reference for the composed `mcd` call only where its discrete decisions do
not hang on the last bits and its float64 arithmetic is well inside an fp32 rounding. Shown here on exactly the rows and pairs
the device test runs, in the forms the suite already has:

1. DIO's and StoneMask's decisions are stable under 1e-12 relative input noise: identical voiced sets, values within 1e-10
   (test_dio_cpu.test_decisions_are_stable_under_rounding_level_noise).
2. The fp32 round trip of the DIO track (one ulp either way) moves no frame of the refined track past 4 * 2^-24 relative.
3. Float64 CheapTrick under the chain's track is within 2^-24 / 4 of the long double back end on every row
   (test_cheaptrick_cpu.test_reference_sensitivity_on_the_device_test_inputs).
4. No voiced frame has 1.5 fs / f0 within 1e-6 of a half-integer: a change of one ulp in F0 cannot flip CheapTrick's half width.
5. The FastDTW margin ratio (fastdtw_cases.margin_ratio, eps = (25 + 2) 2^-24) on the chain's fp32 cepstra is at least 4 for every
   pair and radius at which the device test demands the path of fastdtw_ref. That test measures the ratio again on the device's
   own cepstra, where the condition is 1; the factor 4 here is the room for those cepstra to differ from the chain's by up to
   the CheapTrick bar, which moves the margins.
6. The chain has 1 + length // 80 frames; the shapes of the pairs (which last frames are voiced, which side is short) are as
   mcd_world_ref states them, and the three alignments of pair B differ.

The figures of the chain (printed with -s):
    pair  voiced     last frame voiced   FastDTW cost r1 / r2     exact DTW   margin ratio
    A     79 / 74    both                138.342 / 138.342        138.342     8.44
    B     79 / 47    test                160.608 / 159.928        157.695     1.69 (not used for path identity)
    C     49 / 72    ref                 152.706 / 152.706        152.706     16.81
    D     1 / 74     ref                 NaN: under 10 voiced frames on the test side
    E     57 / 74    ref                 117.611 / 117.611        117.611     7.14
"""
import numpy as np
import pytest

import cheaptrick_ref as CR
import dio_ref as DIO
import mcd_world_ref as W

ROWS = sorted(W.ROWS)


@pytest.mark.parametrize('name', ROWS)
def test_decisions_are_stable_under_rounding_level_noise(name):
    x = W.waveform(name)[:W.length_of(name)].astype(np.float64)
    rng = np.random.default_rng(11)
    k = W.chain_of(name)
    a = DIO.dio(x)
    assert np.array_equal(DIO.f32(a['f0']), k['dio'])
    b = DIO.dio(x * (1 + 1e-12 * rng.standard_normal(len(x))))
    va, vb = a['f0'] > 0, b['f0'] > 0
    assert np.array_equal(va, vb) and np.array_equal(a['cand'] == 0, b['cand'] == 0)
    rel = float((np.abs(a['f0'] - b['f0'])[va] / a['f0'][va]).max()) if va.any() else 0.0
    wa = DIO.stonemask(x, k['dio'])
    assert np.array_equal(DIO.f32(wa), k['f0'])
    wb = DIO.stonemask(x * (1 + 1e-12 * rng.standard_normal(len(x))), DIO.f32(b['f0']))
    assert np.array_equal(wa > 0, wb > 0) and np.array_equal(wa > 0, k['voiced'])
    wrel = float((np.abs(wa - wb)[wa > 0] / wa[wa > 0]).max())
    print(f'\n{name}: voiced {int(k["voiced"].sum())} of {len(va)}, no flips; relative difference dio {rel:.1e}, stonemask {wrel:.1e}')
    assert rel <= 1e-10 and wrel <= 1e-10


@pytest.mark.parametrize('name', ROWS)
def test_fp32_round_trip_of_the_dio_track_moves_no_frame(name):
    x = W.waveform(name)[:W.length_of(name)].astype(np.float64)
    k = W.chain_of(name)
    want = DIO.stonemask(x, k['dio'])
    f32 = k['dio'].astype(np.float32)
    v = want > 0
    assert v.any()
    worst = 0.0
    for sign in (-1.0, 1.0):
        nudged = np.nextafter(f32, np.float32(sign * np.inf)).astype(np.float64)
        nudged[f32 == 0] = 0
        got = DIO.stonemask(x, nudged)
        assert np.array_equal(got > 0, v)
        worst = max(worst, float((np.abs(got - want)[v] / (4 * 2.0 ** -24 * want[v])).max()))
    print(f'\n{name}: one ulp of the fp32 DIO track moves the refined track by {worst:.3f} of 4 * 2^-24 relative at most')
    assert worst <= 1


@pytest.mark.parametrize('name', ROWS)
def test_float64_cheaptrick_is_within_a_quarter_rounding_of_long_double(name):
    x, k = W.waveform(name), W.chain_of(name)
    kw = dict(fs=W.FS, n_fft=W.N_FFT, hop=W.HOP, length=W.length_of(name))
    env, _ = CR.cheaptrick(x, k['f0'], **kw)
    ld, _ = CR.cheaptrick(x, k['f0'], be=CR.LD, **kw)
    assert np.isfinite(env).all() and (env > 0).all()
    worst = float(np.abs((env.astype(np.longdouble) - ld) / ld).max())
    span = float((10 * np.log10(env.max(-1) / env.min(-1))).max())
    print(f'\n{name}: float64 against long double {worst:.2e} (bar {2.0 ** -26:.2e}), envelopes span up to {span:.0f} dB')
    assert worst <= 2.0 ** -24 / 4


def test_no_voiced_frame_sits_on_a_half_width_tie():
    worst = 1.0
    for name in ROWS:
        f0 = W.chain_of(name)['f0']
        f0 = f0[f0 > 0]
        assert ((f0 > CR.f0_floor(W.FS, W.N_FFT)) & (f0 <= W.FS / 4.0)).all()      # every voiced frame keeps its own F0 in CheapTrick
        v = 1.5 * W.FS / f0
        worst = min(worst, float(np.abs(v - np.floor(v) - 0.5).min()))              # half_width = floor(v + 0.5) steps where v is k + 0.5
    print(f'\nthe nearest 1.5 fs / f0 to a half-integer: {worst:.2e} away')
    assert worst > 1e-6


def test_frame_counts_and_the_shape_of_every_pair():
    for name in ROWS:
        k = W.chain_of(name)
        assert len(k['f0']) == len(k['voiced']) == 1 + W.length_of(name) // W.HOP and k['mc'].shape == (int(k['voiced'].sum()), W.D)
        assert np.isfinite(k['mc']).all()
    last = lambda n: bool(W.chain_of(n)['voiced'][-1])
    assert W.length_of('a_test') % W.HOP == 0 == W.length_of('a_ref') % W.HOP and last('a_test') and last('a_ref')      # the frame-count edge
    assert last('b_test') and not last('b_ref') and not last('c_test') and last('c_ref')
    assert 0 < W.chain_of('d_test')['voiced'].sum() < W.MIN_VOICED and np.isnan(W.pipeline_of('D')['mcd'])
    assert W.length_of('e_test') % W.HOP and W.length_of('d_test') % W.HOP
    assert set(W.ORDERED) == set(W.PAIRS) and max(W.length_of(n) for n in ROWS) <= 8000
    # with the name (the per-frame cache) and without it: the same chain
    plain = W.chain(W.waveform('d_test'), W.length_of('d_test'))
    assert all(np.array_equal(plain[key], W.chain_of('d_test')[key]) for key in plain)


def test_fastdtw_margins_and_the_figures_of_the_chain():
    for pair in W.ORDERED:
        t, r, radii, identity = W.PAIRS[pair]
        assert set(identity) <= set(radii) <= set(W.RADII)
        for radius in radii:
            w = W.pipeline_of(pair, radius)
            if pair == 'D':
                print(f'\npair D: voiced {w["n_test"]} / {w["n_ref"]}: NaN')
                assert not identity
                continue
            ratio, exact = W.margin_ratio(w), W.exact_of(pair)
            print(f'\npair {pair} radius {radius}: voiced {w["n_test"]} / {w["n_ref"]}, FastDTW cost {w["cost"]:.3f} over {w["length"]} cells, '
                  f'exact {exact["cost"]:.3f} over {exact["length"]}, margin ratio {ratio:.2f}, mcd {w["mcd"]:.6f}')
            assert w['cost'] >= exact['cost'] * (1 - 1e-12) and np.isfinite(w['mcd'])
            if radius in identity:
                assert ratio >= 4, (pair, radius, ratio)
    assert all(W.PAIRS[p][3] for p in 'ACE')                                      # the pairs that carry the path identity
    # pair B is there because its three alignments differ: `align` and `radius` reach the kernel
    b1, b2, bx = W.pipeline_of('B', 1), W.pipeline_of('B', 2), W.exact_of('B')
    assert bx['cost'] < b2['cost'] * (1 - 1e-3) and b2['cost'] < b1['cost'] * (1 - 1e-3)
