"""CPU: the float64 CheapTrick reference of the device tests (tests/cheaptrick_ref.py) against independent statements of the same
definition, and the host side of evaluate.cheaptrick (cheaptrick_mc_matrix). pyworld is not available, so nothing here is a parity
test against WORLD. No GPU.

1. Recovery: on an equal-amplitude, zero-phase sum of all harmonics of f0 below Nyquist (fs = 16000, N = 1024) the log envelope over
   [3 f0, (nh - 3) f0] is flat, although the merely smoothed spectrum S is not. Measured with this reference at 8 frame positions one
   eighth of a period apart (printed by the test, run with -s):
       f0    max peak-to-peak of log env   peak-to-peak of log S   spread of log env across the positions
       100   8.61e-04                      0.72 .. 0.80            7.9e-03
       250   3.35e-04                      0.79 .. 0.87            9.1e-03
   Bars: 4 x the measured flatness for env; S alone must exceed 0.5 (a lifter that does nothing cannot pass); under 0.06 across the
   positions.
2. Smoothing against the brute-force mean of the mirrored staircase on a 64 x finer grid (width chosen so that the window's ends
   fall on grid points: the brute force is then exact).
3. Lifter and envelope against direct cosine sums at N = 64.
4. Window: sum w^2 = 1, sum s = 0, halves away from zero at a tie (fs = 16000: f = 480 gives 1.5 fs/f = 50 exactly, f = 384 gives
   62.5 -> 63 where rounding to even would give 62), the special F0 values.
5. The fused identity: freqt(c with c[0] halved) equals mcep_ref.sp2mc of the reference's own env within 1e-12.
6. The reference's own sensitivity on the inputs of the device tests: numpy float64 with numpy's FFT against the same statements
   in long double with a direct DFT; every env element within 2^-24 / 4 relative, the condition under which the device tests'
   one-rounding bar 4 * 2^-24 is meaningful. Measured: 9.4e-10 (N = 512), 2.1e-09 (1024), 1.6e-09 (2048); the envelopes of those
   inputs span up to 69 dB. (With the noise of the inputs 60 dB down instead of 30 the span is 95 dB and the float64 reference
   is off by 2.6e-06: see cheaptrick_ref.voiced. Exchanging ONLY the transforms for the long double DFT and keeping float64 elsewhere
   moves env by 8e-13 at either noise level: the transforms are not where float64 runs out, the running sum of the smoothing is,
   and a comparison that leaves it in float64 on both sides cannot see that. Hence the whole evaluation in long double here.)
"""
import numpy as np
import pytest

import cheaptrick_ref as R
import mcep_ref as MR
from common import pkg


@pytest.mark.parametrize('f0', R.RECOVERY_F0)
def test_recovery_of_a_flat_harmonic_spectrum(f0):
    k = R.recovery_case(f0)
    fr = [R.frame(k['x'], int(i) * k['hop'], f0, k['fs'], k['n_fft']) for i in k['frames']]
    le = np.stack([np.log(r['env'][k['band']]) for r in fr])
    ls = np.stack([np.log(r['S'][k['band']]) for r in fr])
    flat, s_lo, s_hi, across = np.ptp(le, axis=1).max(), np.ptp(ls, axis=1).min(), np.ptp(ls, axis=1).max(), np.ptp(le, axis=0).max()
    print(f'\nrecovery f0 {f0}: log env peak-to-peak {flat:.3e}, log S peak-to-peak {s_lo:.2f} .. {s_hi:.2f}, across positions {across:.2e}')
    assert flat <= 4 * R.RECOVERY_FLATNESS[f0]
    assert s_lo > 0.5
    assert across < 0.06


def test_smoothing_equals_the_brute_force_mean_of_the_mirrored_staircase():
    fs, N, G = 6400, 64, 64
    h, df = N // 2, fs / N
    rng = np.random.default_rng(1)
    for r in (150, 37, 64, 700):                                                  # half width of the window in 64ths of a bin
        f = 3.0 * r * df / G                                                      # wd / (2 df) = r / 64 exactly
        P = np.exp(2 * rng.standard_normal(h + 1))
        got = R.smooth(P, f, fs, N)
        g = np.arange(-r, r) + 0.5                                                # midpoints of the fine cells, in 64ths of a bin
        want = np.empty(h + 1)
        for i in range(h + 1):
            b = np.rint((i * G + g) / G).astype(int)                              # the bin whose step holds the midpoint (never a tie)
            b = np.abs(b)
            b = np.where(b > h, 2 * h - b, b)                                     # mirrored at 0 and at Nyquist
            want[i] = P[b].mean()
        assert np.abs(got / want - 1).max() <= 1e-12, (r, float(np.abs(got / want - 1).max()))


def test_lifter_and_envelope_equal_direct_cosine_sums():
    fs, N, q1 = 2000, 64, -0.15
    h = N // 2
    rng = np.random.default_rng(2)
    S = np.exp(rng.standard_normal(h + 1))
    for f in (140.0, 333.3):
        c = R.lifter(S, f, fs, N, q1)
        ext = np.concatenate([np.log(S), np.log(S)[h - 1:0:-1]])
        n = np.arange(h + 1)
        C = np.array([(ext * np.cos(2 * np.pi * np.arange(N) * m / N)).sum() for m in n])
        x = np.pi * f * n[1:] / fs
        want = C / N * np.concatenate([[1.0], np.sin(x) / x]) * ((1 - 2 * q1) + 2 * q1 * np.cos(2 * np.pi * f * n / fs))
        assert np.abs(c - want).max() <= 1e-13
        cext = np.concatenate([want, want[h - 1:0:-1]])
        env = np.exp(np.array([(cext * np.cos(2 * np.pi * np.arange(N) * m / N)).sum() for m in n]))
        assert np.abs(R.F64.rfft_even(c, N) - np.log(env)).max() <= 1e-12
        assert np.abs(np.fft.irfft(np.log(env), N)[:h + 1] - want).max() <= 1e-13      # irfft(log env) IS c


def test_window_normalisation_mean_removal_and_rounding():
    fs = 16000
    assert R.half_width(480.0, fs) == 50 and R.half_width(384.0, fs) == 63 and 1.5 * fs / 384.0 == 62.5
    assert R.half_width(1920.0, fs) == 13 and 1.5 * fs / 1920.0 == 12.5
    x = np.random.default_rng(3).standard_normal(3000) + 0.7
    for f, pos in ((480.0, 1000), (384.0, 5), (55.0, 2990), (500.0, 4000)):
        w, s = R.window(x, pos, f, fs)
        assert len(w) == len(s) == 2 * R.half_width(f, fs) + 1
        assert abs((w * w).sum() - 1) <= 1e-14 and abs(s.sum()) <= 1e-14 * w.sum() * np.abs(x).max()
        assert w[0] == w[-1] or abs(w[0] - w[-1]) < 1e-15
    w, s = R.window(x, 4000, 500.0, fs)                                           # every index clamped: a constant, nothing left
    assert np.abs(s).max() <= 1e-15
    assert R.window(np.zeros(0), 0, 500.0, fs)[1].tolist() == [0.0] * 97


@pytest.mark.parametrize('n_fft', (512, 1024, 2048))
def test_special_f0_values(n_fft):
    fs = R.FS
    sp = R.special_f0(fs, n_fft)
    eff = [R.effective_f0(v, fs, n_fft) for v in sp]
    lo = R.f0_floor(fs, n_fft)
    assert float(sp[3]) <= lo < float(sp[4]) and float(sp[5]) == fs / 4 < float(sp[6])
    assert eff[:4] == [500.0] * 4 and eff[4] == float(sp[4]) and eff[5] == fs / 4 and eff[6] == 500.0 and eff[12] == 500.0
    assert 2 * R.half_width(eff[4], fs) + 1 == n_fft - 3                          # the longest window: it nearly fills N
    assert eff[7] == (55.0 if lo < 55.0 else 500.0) and eff[9] == 480.0 and eff[10] == 384.0 and eff[11] == 500.0


def test_fused_identity_mel_cepstrum_of_c_equals_sp2mc_of_env():
    env, c = R.case_ref(1024)
    for order, alpha in ((24, 0.42), (34, 0.55), (0, 0.42)):
        got = R.mc_from_c(c[:, ::5], order, alpha)
        want = MR.sp2mc(env[:, ::5], order, alpha)
        assert np.abs(got - want).max() <= 1e-12, float(np.abs(got - want).max())


@pytest.mark.parametrize('n_fft', (512, 1024, 2048))
def test_reference_sensitivity_on_the_device_test_inputs(n_fft):
    k = R.case(n_fft)
    env, _ = R.case_ref(n_fft)
    assert np.isfinite(env).all() and (env > 0).all()
    worst = 0.0
    for b in range(2):
        ld, _ = R.cheaptrick(k['x'][b], k['f0'][b], k['fs'], n_fft, k['hop'], length=int(k['lengths'][b]), be=R.LD)
        worst = max(worst, float(np.abs((env[b].astype(np.longdouble) - ld) / ld).max()))
    span = float((10 * np.log10(env.max(-1) / env.min(-1))).max())
    print(f'\nsensitivity n_fft {n_fft}: float64 against long double {worst:.2e} (bar {2.0 ** -26:.2e}), envelopes span up to {span:.0f} dB')
    assert worst <= 2.0 ** -24 / 4


def test_mc_matrix_of_the_package_is_freqt_of_the_unit_vectors():
    E = pkg().evaluate
    for n_fft, order, alpha in ((64, 4, 0.42), (512, 24, 0.35), (1024, 24, 0.42)):
        G = E.cheaptrick_mc_matrix(n_fft, order, alpha)
        assert G.shape == (order + 1, n_fft // 2 + 1) and G.dtype == np.float64 and not G.flags.writeable
        assert E.cheaptrick_mc_matrix(n_fft, order, alpha) is G
        c = np.random.default_rng(n_fft).standard_normal(n_fft // 2 + 1)
        half = c.copy()
        half[0] *= 0.5
        want = R.mc_from_c(c, order, alpha)
        assert np.abs(G @ half - want).max() <= 1e-12 * np.abs(want).max()
    for bad in ((63, 4, 0.42), (64, 33, 0.42), (64, -1, 0.42), (64, 4, 1.0)):
        with pytest.raises(ValueError):
            E.cheaptrick_mc_matrix(*bad)
    assert E.CHEAPTRICK_FLOOR == R.FLOOR and pkg().cheaptrick is E.cheaptrick
