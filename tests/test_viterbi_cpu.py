"""CPU: the float64 decoder of tests/viterbi_ref.py against brute force, the band table of pitch.viterbi_transition against the
formula, and the decoding design (obs = -100 CMDF - octave_cost log2(lag / lag_min), triangular +-240 cent band, jump floor) on
the YIN fixtures and on the hard case, all in float64. No GPU: the package contributes only the numpy side of its table."""
import numpy as np
import pytest
import torch

import viterbi_ref as VR
import yin_ref as YR
from common import pkg

OCTAVE_COST, JUMP_COST, THR, SR = 1.0, 16.0, 0.1, 16000


def eighths(rng, shape, lim=8.0):
    """Multiples of 1/8 in [-lim, lim]: every sum below is exact, so ties are real ties."""
    return rng.integers(-int(lim * 8), int(lim * 8) + 1, size=shape) / 8.0


@pytest.mark.parametrize('n,F', [(3, 4), (4, 3)])
@pytest.mark.parametrize('jump', [np.inf, 1.5])
def test_reference_equals_brute_force(n, F, jump):
    rng = np.random.default_rng(n * 10 + F)
    seen_tie = False
    for trial in range(40):
        W = int(rng.integers(1, n + 1))
        lo = rng.integers(0, n - W + 1, size=n)
        logw = eighths(rng, (n, W), 2.0)
        logw[rng.random((n, W)) < 0.2] = -np.inf
        if not np.isfinite(jump):
            logw[np.arange(n), 0] = np.where(np.isfinite(logw[:, 0]), logw[:, 0], 0.0)      # one finite predecessor per state
        x = eighths(rng, (F, n), 1.0 if trial % 2 else 0.25)                                 # the coarse half is full of ties
        prior = eighths(rng, n, 1.0) if trial % 3 else None
        scale = 2.0 if trial % 4 == 0 else 1.0
        got = VR.decode(x, logw, lo, scale, prior, jump)
        want = VR.brute_force(x, logw, lo, scale, prior, jump)
        assert np.array_equal(got, want), (trial, got, want)
        s = VR.score(got, x, logw, lo, scale, prior, jump)
        others = [VR.score(p, x, logw, lo, scale, prior, jump) for p in np.ndindex(*(n,) * F) if tuple(p) != tuple(got)]
        seen_tie |= max(others) == s
    assert seen_tie                                           # the tie rules were exercised, not just the maximum


def test_all_equal_lattice_decodes_to_zeros():
    logw, lo = np.zeros((5, 3)), np.array([0, 0, 1, 2, 2])
    assert not VR.decode(np.zeros((6, 5)), logw, lo, jump=2.0).any()
    assert not VR.decode(np.zeros((6, 5)), logw, lo).any()


@pytest.mark.parametrize('tau_min,tau_max,cmin,cmax', [(32, 266, 5, 64), (40, 320, 7, 77), (0, 800, 1, 194)])
def test_transition_table(tau_min, tau_max, cmin, cmax):
    logw, lo = pkg().pitch._transition_host(tau_min, tau_max, 240.0)
    ref_logw, ref_lo = VR.transition(tau_min, tau_max, 240.0)
    n = tau_max - 1 - tau_min
    assert logw.shape == (n, cmax) and lo.shape == (n,)
    counts = np.isfinite(logw).sum(1)
    assert counts.min() == cmin and counts.max() == cmax
    assert lo.min() >= 0 and (lo + cmax).max() <= n
    assert np.array_equal(lo, ref_lo)
    assert np.all((logw == -np.inf) == (ref_logw == -np.inf)) and not np.isnan(logw).any() and logw.max() <= 0
    fin = np.isfinite(ref_logw)
    assert np.all(np.abs(logw[fin] - ref_logw[fin]) <= 2.0 ** -30 * np.abs(ref_logw[fin]))      # far inside half an fp32 ulp
    assert np.all(np.abs(logw[fin].astype(np.float32) - ref_logw[fin]) <= 2.0 ** -24 * np.abs(ref_logw[fin]) + 2.0 ** -149)
    dense = VR.dense_transition(logw, lo, np.inf, n)
    assert np.array_equal(dense, dense.T)                     # symmetric, not row-normalised
    assert np.array_equal(np.diag(dense), np.zeros(n))        # self weight log 1


def design_decode(c, tau_min, tau_max):
    """c float64 [F, n] -> decoded state per frame under the package's defaults."""
    logw, lo = VR.transition(tau_min, tau_max)
    return VR.decode(c, logw, lo, -YR.THETA, VR.octave_prior(tau_min, c.shape[-1], OCTAVE_COST), JUMP_COST)


@pytest.mark.parametrize('name', ['speech', 'default', 'odd', 'long'])
def test_float64_design_on_fixtures(name):
    t = YR.long_truth() if name == 'long' else YR.truth(name)
    s = t['meta']
    hard = YR.hard_tau(t['cmdf'], THR).numpy()
    n_voiced = 0
    for b in range(hard.shape[0]):
        path = design_decode(t['cmdf'][b].numpy(), s['tau_min'], s['tau_max'])
        v = hard[b] > 0
        n_voiced += int(v.sum())
        assert np.all(np.abs(path[v] - hard[b][v]) <= 1), (name, b, int((np.abs(path[v] - hard[b][v]) > 1).sum()))
        f0 = np.where(v, SR / (path + s['tau_min'] + 1.0), 0.0)
        assert np.array_equal(f0 == 0, hard[b] == 0)
    assert n_voiced > 0
    if name == 'long':
        assert n_voiced == 620


def test_float64_design_on_silence():
    t = YR.truth('silence')
    hard = YR.hard_tau(t['cmdf'], THR).numpy()
    assert not hard.any()                                     # every frame unvoiced: the decoded track is 0 whatever the path


def test_float64_design_on_hard_case():
    x, true_f = VR.hard_case()
    tau_min, tau_max = int(SR / 500), int(SR / 60)
    c = YR.cmdf(torch.from_numpy(x)[None].double(), tau_min, tau_max, VR.HARD_HOP)[0]
    hard = YR.hard_tau(c, THR).numpy()
    path = design_decode(c.numpy(), tau_min, tau_max)
    v = hard > 0
    true_f = true_f[:len(hard)]
    cents = lambda lag: np.abs(1200 * np.log2(SR / (lag + tau_min + 1.0) / true_f))
    hard_err, dec_err = int((cents(hard)[v] > 100).sum()), int((cents(path)[v] > 100).sum())
    print(f'\nhard case: {int(v.sum())} voiced frames of {len(hard)}, errors > 100 cents: hard YIN {hard_err}, decoded {dec_err}')
    assert hard_err >= 10
    assert dec_err == 0
