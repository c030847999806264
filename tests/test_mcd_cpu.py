"""CPU: the float64 helpers of the objective-evaluation tests (tests/dtw_ref.py, tests/mcep_ref.py) against independent statements of
the same definitions, and the host side of td-vc-gan_amd/evaluate.py (sp2mc_matrix, f0_stats). No GPU.

1. dtw_ref against brute-force enumeration of EVERY warping path, all shapes up to 4 x 4, real-valued and tied inputs, all metrics;
   the length carried forward equals the length of the back-traced path.
2. mcep_ref against the analytic warped-cepstrum spectrum. Residues measured here (max |mc - m|, float64):
       (1024, 24, 0.42) 1.11e-16   (512, 24, 0.35) 4.94e-17   (2048, 34, 0.55) 6.25e-17   (64, 4, 0.42) 1.93e-14
   The bar is 1e-12 for the three larger transforms and 4 x 1.93e-14 for the 64-point one (see BAR). alpha = 0 is the identity on c.
3. evaluate.sp2mc_matrix against the recursion; evaluate.f0_stats against the three formulas of test_mcd.py on a hand-made track.
"""
import numpy as np
import pytest
import torch

import dtw_ref as DR
import mcep_ref as MR
from common import pkg

SETTINGS = [(1024, 24, 0.42), (512, 24, 0.35), (2048, 34, 0.55), (64, 4, 0.42)]
# the residue at 64 points is aliasing of the unwarped cepstrum (it decays like alpha^n), not rounding; with the coefficients drawn here
# it measures 1.93e-14, so its bar is 4 x that instead of the 1e-12 of the three larger transforms
BAR = {SETTINGS[0]: 1e-12, SETTINGS[1]: 1e-12, SETTINGS[2]: 1e-12, SETTINGS[3]: 4 * 1.93e-14}


# ------------------------------------------------------------------------------------------------------------ DTW
@pytest.mark.parametrize('metric', DR.METRICS)
def test_dtw_ref_equals_brute_force_up_to_4x4(metric):
    rng = np.random.default_rng(5)
    for n in range(1, 5):
        for m in range(1, 5):
            for tied in (False, True):
                for D in (1, 3):
                    if tied:
                        x, y = rng.integers(-1, 2, (n, D)).astype(np.float64), rng.integers(-1, 2, (m, D)).astype(np.float64)
                    else:
                        x, y = rng.standard_normal((n, D)), rng.standard_normal((m, D))
                    d = DR.distance(x, y, metric)
                    want, lens = DR.brute_force(d)
                    r = DR.dtw(x, y, metric)
                    assert abs(r['cost'] - want) <= 1e-12 * max(1.0, want), (n, m, tied, D)
                    assert DR.is_warping_path(r['path'], n, m)
                    assert r['length'] == len(r['path']) and r['length'] in lens          # carried == back-traced, and a minimal path
                    assert abs(DR.score(r['path'], x, y, metric) - want) <= 1e-12 * max(1.0, want)


def test_dtw_ref_tie_rule_is_up_left_diagonal():
    """All distances equal: every predecessor ties, the first in the order up, left, diagonal wins, so the path runs along the first
    row to the last column and then down: n + m - 1 cells."""
    for n, m in ((3, 4), (4, 3), (1, 5), (5, 1)):
        r = DR.dtw(np.zeros((n, 2)), np.zeros((m, 2)))
        want = [(0, j) for j in range(m)] + [(i, m - 1) for i in range(1, n)]
        assert r['cost'] == 0 and r['length'] == n + m - 1 and [tuple(c) for c in r['path']] == want


def test_dtw_ref_carried_length_equals_backtraced_length_on_larger_lattices():
    rng = np.random.default_rng(6)
    for n, m, D in ((37, 50, 2), (64, 129, 1), (200, 150, 25)):
        x, y = rng.integers(-3, 4, (n, D)), rng.integers(-3, 4, (m, D))
        for metric in DR.METRICS:
            r = DR.dtw(x, y, metric)
            assert r['length'] == len(r['path']) and DR.is_warping_path(r['path'], n, m)
            got = DR.score(r['path'], x, y, metric)
            assert got == r['cost'] if metric != 'l2' else abs(got - r['cost']) <= 1e-13 * got      # integer sums are exact, roots are not


# ------------------------------------------------------------------------------------------------------------ mel-cepstrum
@pytest.mark.parametrize('n_fft,order,alpha', SETTINGS)
def test_mcep_ref_recovers_the_analytic_warped_cepstrum(n_fft, order, alpha):
    rng = np.random.default_rng(n_fft + order)
    m = rng.standard_normal(order + 1) * 0.5 ** np.arange(order + 1).clip(max=6)
    got = MR.sp2mc(MR.warped_spectrum(m, n_fft, alpha), order, alpha)
    err = float(np.abs(got - m).max())
    print(f'\nmcep_ref ({n_fft}, {order}, {alpha}): max |mc - m| = {err:.2e}')
    assert err <= BAR[(n_fft, order, alpha)]


def test_mcep_ref_alpha_zero_is_the_identity():
    rng = np.random.default_rng(9)
    c = rng.standard_normal(65)
    assert np.array_equal(MR.freqt(c, 64, 0.0), c)
    assert np.array_equal(MR.freqt(c, 10, 0.0), c[:11])
    lp = rng.standard_normal(65)
    want = np.fft.irfft(lp, n=128)[:11]
    want[0] *= 0.5
    assert np.abs(MR.sp2mc(np.exp(lp), 10, 0.0) - want).max() <= 1e-15          # log(exp(.)) in between: the last bit


@pytest.mark.parametrize('n_fft,order,alpha', SETTINGS + [(16, 0, 0.42), (16, 8, -0.3)])
def test_sp2mc_matrix_equals_the_recursion(n_fft, order, alpha):
    E = pkg().evaluate
    M = E.sp2mc_matrix(n_fft, order, alpha)
    assert M.shape == (order + 1, n_fft // 2 + 1) and M.dtype == np.float64 and not M.flags.writeable
    assert E.sp2mc_matrix(n_fft, order, alpha) is M                                        # cached
    rng = np.random.default_rng(3)
    lp = rng.standard_normal((5, n_fft // 2 + 1)) * 3
    want = MR.sp2mc(np.exp(lp), order, alpha)
    got = lp @ M.T
    scale = np.abs(M).sum(1).max() * np.abs(lp).max()
    assert np.abs(got - want).max() <= 1e-13 * scale, np.abs(got - want).max()
    if (n_fft, order, alpha) == (1024, 24, 0.42):
        assert abs(np.abs(M).sum(1).max() - 0.64) < 0.01                                   # max_row sum |M| at the default settings


def test_sp2mc_matrix_refuses_bad_arguments():
    E = pkg().evaluate
    for bad in ((1023, 24, 0.42), (1024, 600, 0.42), (1024, -1, 0.42), (1024, 24, 1.0)):
        with pytest.raises(ValueError):
            E.sp2mc_matrix(*bad)


# ------------------------------------------------------------------------------------------------------------ F0 statistics
def test_f0_stats_against_the_three_formulas():
    E = pkg().evaluate
    ft = np.array([0, 100.0, 110, 0, 121, 133.1, 0, 0, 146.41], np.float32)
    fr = np.array([200.0, 0, 0, 190, 180.5, 171.475, 150], np.float32)
    t64, r64 = ft.astype(np.float64), fr.astype(np.float64)
    vt, vr = t64[t64 > 0], r64[r64 > 0]
    want = dict(diff_f0_mean=np.mean(np.log(vt)) - np.mean(np.log(vr)), diff_f0_var=np.log(np.var(vt)) - np.log(np.var(vr)),
                f0_ratio=np.mean(vr) / np.mean(vt))
    got = E.f0_stats(torch.from_numpy(ft), torch.from_numpy(fr))
    for k, v in want.items():
        assert got[k].dtype == torch.float64 and abs(float(got[k]) - v) <= 1e-13 * abs(v), (k, float(got[k]), v)
    both = E.f0_stats(torch.from_numpy(np.stack([ft, np.zeros_like(ft)])), torch.from_numpy(np.stack([fr, fr])))
    assert abs(float(both['f0_ratio'][0]) - want['f0_ratio']) <= 1e-13 and all(bool(torch.isnan(v[1])) for v in both.values())
