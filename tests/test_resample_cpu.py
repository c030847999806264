"""CPU: the float64 restatement of the resampler (tests/resample_ref.py) against analytic tones, the product's polyphase bank
(resample.resample_bank) against that restatement, the output-length rule and the crop-start mask of load_segments.

Tone checks: a 0.03-amplitude tone through the per-sample loop, compared away from the row's ends with the same tone sampled at the
new rate, in units of the amplitude. The margin is the filter's reach, 64 zero crossings / rolloff = 68 samples at the LOWER of the
two rates: 70 outputs when downsampling, 70 input samples (140 outputs at 8 -> 16 kHz, 105 at 16 -> 24 kHz) when upsampling. Inside
70 outputs of an upsampled row's end the truncated filter is still visible (1.6e-4 at 8 -> 16 kHz), as it is in resampy. Upsampling is accurate to 1e-6. Downsampling shows the
small gain of the truncated index_step (up to 2.8e-3 at 44.1 kHz -> 16 kHz), which a least-squares gain fit removes down to 5e-4;
a tone at 1.15 x the new Nyquist is rejected to 1e-3."""
import numpy as np
import pytest
import torch

import resample_ref as RR
from common import pkg

AMP = 0.03


def edge(so, sn):
    return -(-70 * max(so, sn) // so)      # 70 samples of the lower rate, in outputs


def tone(freq, n, sr):
    return AMP * np.sin(2 * np.pi * freq * np.arange(n) / sr)


@pytest.fixture(scope='module')
def tones():
    """ratio -> (resampled 1 kHz tone, the analytic tone at the new rate), interior only; computed once"""
    out = {}
    for so, sn in RR.UP + RR.DOWN:
        y = RR.resample_loop(tone(1000.0, int(0.035 * so), so), so, sn)
        e = edge(so, sn)
        assert len(y) > 3 * e
        out[so, sn] = (y[e:-e], tone(1000.0, len(y), sn)[e:-e])
    return out


@pytest.mark.parametrize('rates', RR.UP)
def test_upsampled_tone_matches_the_analytic_tone(tones, rates):
    y, ref = tones[rates]
    err = float(np.abs(y - ref).max()) / AMP
    print(f'[resample] {rates}: interior error {err:.2e} of the amplitude')
    assert err <= 1e-6


@pytest.mark.parametrize('rates', RR.DOWN)
def test_downsampled_tone_matches_up_to_the_index_step_gain(tones, rates):
    y, ref = tones[rates]
    err = float(np.abs(y - ref).max()) / AMP
    g = float(np.dot(y, ref) / np.dot(ref, ref))
    fit = float(np.abs(y - g * ref).max()) / AMP
    print(f'[resample] {rates}: interior error {err:.2e}, gain {g:.5f}, after the gain fit {fit:.2e} of the amplitude')
    assert err <= 4e-3
    assert fit <= 5e-4


@pytest.mark.parametrize('rates', RR.DOWN)
def test_tone_above_the_new_nyquist_is_rejected(rates):
    so, sn = rates
    y = RR.resample_loop(tone(1.15 * sn / 2, int(0.035 * so), so), so, sn)
    res = float(np.abs(y[edge(so, sn):-edge(so, sn)]).max()) / AMP
    print(f'[resample] {rates}: residual of a tone at 1.15 x Nyquist {res:.2e} of the amplitude')
    assert res <= 1e-3


@pytest.mark.parametrize('rates', RR.UP + RR.DOWN)
def test_bank_as_a_zero_extended_fir_equals_the_loop(rates):
    so, sn = rates
    bk = pkg().resample.resample_bank(so, sn)
    assert bk.bank.dtype == np.float64 and bk.bank.shape[0] == bk.L and bk.L * so == bk.M * sn
    rng = np.random.default_rng(so + sn)
    worst = 0.0
    for n_in in (1, 2, 3, 50, 383, 385, 1000):
        x = rng.standard_normal(n_in)
        ref = RR.resample_loop(x, so, sn)
        got = RR.apply_bank(bk.bank, bk.L, bk.M, bk.left, x, len(ref))
        if len(ref):
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print(f'[resample] {rates}: bank vs loop, worst {worst:.2e} of the row maximum (L = {bk.L}, W = {bk.bank.shape[1]})')
    assert worst <= 1e-11


def test_bank_geometry_and_cache():
    R = pkg().resample
    bk = R.resample_bank(48000, 16000)
    assert (bk.L, bk.M) == (1, 3) and R.resample_bank(48000, 16000) is bk
    assert abs(float(bk.bank.sum()) - 1.0027) < 2e-4                  # the DC gain of the truncated index_step, kept as resampy has it
    assert R.resample_bank(44100, 16000).L == 160 and R.resample_bank(22050, 16000).L == 320
    assert R.resample_bank(16000, 24000).L == 3 and R.resample_bank(8000, 16000).L == 2
    win, prec = R.resample_filter('kaiser_best')
    assert len(win) == 32769 and prec == 9 and np.array_equal(win, RR.sinc_window('kaiser_best')[0])
    fast = R.resample_bank(48000, 16000, 'kaiser_fast')
    assert fast.bank.shape[1] < 110
    assert np.array_equal(R.resample_bank(48000, 16000, R.resample_filter('kaiser_fast')).bank, fast.bank)      # (table, precision)
    with pytest.raises(ValueError):
        R.resample_bank(16000, 44101)                                   # 44101 phases: over 8 MiB
    with pytest.raises(ValueError):
        R.resample_filter('kaiser_worst')


def test_output_length_rule():
    R = pkg().resample
    assert [R.num_out(n, 48000, 16000) for n in (1, 2, 3, 50, 383, 385, 1000)] == [0, 0, 1, 16, 127, 128, 333]
    for so, sn in RR.UP + RR.DOWN:
        for n in (0, 1, 7, 441, 4097, 48000):
            assert R.num_out(n, so, sn) == int(n * (float(sn) / so)) == len(RR.resample_loop(np.zeros(n), so, sn))
    assert [R.segment_size(m) for m in (1, 5120, 5121, 16000, 16001)] == [5120, 5120, 5440, 16000, 16320]


def test_valid_start_mask_equals_brute_force():
    R = pkg().resample
    ms, N = 50, 400
    y = np.zeros((3, N), np.float32)
    y[0, 120:123] = 1.0                      # one burst between long zero runs
    y[0, 330] = -2.0
    y[1, :] = 1.0                            # all non-zero
    y[2, 10] = 1.0
    y[2, 390] = 1.0                          # past the row's length: must not count
    n = [400, 237, 300]
    got = R.valid_start_mask(torch.from_numpy(y), torch.tensor(n), ms).numpy()
    want = np.zeros((3, N - ms), bool)
    for b in range(3):
        for s in range(max(0, n[b] - ms)):
            want[b, s] = bool(np.any(y[b, s:min(s + ms, n[b])] != 0))
    assert got.shape == want.shape and np.array_equal(got, want)
    assert want[0].sum() < n[0] - ms and want[0].any()                  # the zero runs do exclude starts
    start = R.draw_start(torch.from_numpy(y), torch.tensor(n), ms, torch.Generator().manual_seed(0)).numpy()
    assert all(want[b, start[b]] for b in range(3))
    short = R.draw_start(torch.from_numpy(y), torch.tensor([400, 50, 20]), ms, torch.Generator().manual_seed(0)).numpy()
    assert short[1] == 0 and short[2] == 0                               # rows that are not cropped start at 0
