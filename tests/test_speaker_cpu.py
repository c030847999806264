"""CPU: the host side of the speaker-similarity evaluation (td-vc-gan_amd/speaker.py) and the float64 restatement the GPU tests
measure against (tests/speaker_ref.py). Resemblyzer and librosa are not available: nothing here is a parity test against them.

1. tdvc_voice_window_count, the closed form the kernels evaluate from the device lengths, equals the literal
   compute_partial_slices loop (count, window starts, padded length) for n = 1..120000 in steps of 7, at the boundaries of the
   window count, and for a second (rate, min_coverage) pair.
2. The Slaney filterbank: hz -> mel(1000) = 15, monotone edges, every row's area sum_k fb[i][k] sr/n_fft = 1 within the
   bin-sampling error (an HTK-scale or un-normalised table fails), the package's vectorised table equals the band-by-band one.
3. The float64 mel reference is within 2^-24 / 4 of a long double evaluation on the inputs the GPU test uses: the bar of
   4 * 2^-24 is meaningful.
4. state_dict keys and shapes are those of nn.LSTM(40, 256, 3) + Linear(256, 256) under lstm. / linear.; both ways strict.
5. load_voice_encoder takes {'model_state': ...} and ignores similarity_weight / similarity_bias.
6. speaker_similarity against the numpy lines of the reference.
7. Every wrapper refuses CPU tensors (no CPU fallback); the new symbols are declared, bound and built.
"""
import os
import re

import numpy as np
import pytest
import torch

import speaker_ref as R
from common import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDARIES = (25439, 25440, 31519, 31520, 43839, 43840, 56159, 56160, 71680, 320000)


def S():
    return pkg().speaker


@pytest.mark.parametrize('rate,cov', [(1.3, 0.75), (2.0, 0.5)])
def test_closed_form_windows_equal_the_literal_loop(rate, cov):
    sp = S()
    step = sp.frame_step(rate)
    for n in list(range(1, 120001, 7)) + list(BOUNDARIES):
        want = R.partial_slices(n, rate, cov)
        cnt, padded = sp.window_count(n, rate, cov)
        assert cnt == len(want), (n, cnt, len(want))
        assert [j * step for j in range(cnt)] == [w[0] for w in want], n
        assert padded == max(n, want[-1][2]), n
    wav, mel = sp.partial_slices(71680, rate, cov)
    assert [(m.start, w.start, w.stop) for w, m in zip(wav, mel)] == R.partial_slices(71680, rate, cov)


def test_window_counts_at_the_documented_boundaries():
    sp = S()
    got = {n: sp.window_count(n)[0] for n in BOUNDARIES}
    assert got == {25439: 1, 25440: 1, 31519: 1, 31520: 2, 43839: 2, 43840: 3, 56159: 3, 56160: 4, 71680: 5, 320000: 25}
    assert sp.frame_step() == 77


def test_slaney_filterbank():
    sp = S()
    assert R.hz_to_mel(1000.0) == 15.0 and float(sp.hz_to_mel(1000.0)) == 15.0
    e = R.mel_edges()
    assert e.shape == (42,) and e[0] == 0.0 and abs(e[-1] - 8000.0) < 1e-9 and (np.diff(e) > 0).all()
    assert np.allclose(np.diff(e[:10]), e[1] - e[0], rtol=1e-12)          # linear part: equal steps below 1 kHz
    fb = R.mel_filterbank()
    assert fb.shape == (40, 201) and (fb >= 0).all()
    # a triangle of height 2/(e2 - e0) on [e0, e2] has area 1; sampled every sr/n_fft = 40 Hz the trapezoid sum is off by at most
    # the kink terms: h^2/12 * sum |slope jumps| <= 40^2/12 * 2 * (2/(e2-e0)) * (1/(e1-e0) + 1/(e2-e1)); bands narrower than two
    # bins (the lowest ones: 2 (e2-e0) = 129 Hz) are bounded by one bin's height, 40 * 2/(e2 - e0)
    area = fb.sum(1) * (R.SR / R.N_FFT)
    for i in range(40):
        w = e[i + 2] - e[i]
        bound = min(40.0 * 2 / w, 1600.0 / 12 * 2 * (2 / w) * (1 / (e[i + 1] - e[i]) + 1 / (e[i + 2] - e[i + 1])))
        assert abs(area[i] - 1.0) <= bound, (i, area[i], bound)
    assert abs(area[20:] - 1.0).max() < 0.05
    peak = fb.argmax(1)
    assert (np.diff(peak) >= 0).all() and peak[0] <= 3 and peak[-1] >= 180
    # the two tables place their edges by different float64 expressions: a few ulp of 8000 Hz (1e-12 Hz) over the narrowest
    # band's 66.7 Hz is 2e-14 of a triangle's height
    assert sp.mel_filterbank().shape == fb.shape and np.abs(sp.mel_filterbank() - fb).max() <= 1e-13 * fb.max()


@pytest.mark.parametrize('n,pad_mode,normalize', [(1000, 'reflect', False), (25440, 'constant', False), (31520, 'reflect', True)])
def test_float64_mel_is_good_to_well_under_the_fp32_bar(n, pad_mode, normalize):
    x = R.tones(n, seed=n, amp=0.003 if normalize else 0.1)
    m64 = R.mel(x, pad_mode, normalize)
    mld = R.mel(x, pad_mode, normalize, dtype=np.longdouble)
    live = mld > 0                                                          # frames past the signal's reach are exact zeros in both
    assert live[:n // R.HOP].all() and np.array_equal(m64 == 0, ~live)
    err = np.abs(m64 - mld)[live] / mld[live]
    print(f'float64 mel against long double, n={n}: {float(err.max()):.3e} (bar 2^-24 / 4 = {2.0 ** -26:.3e})')
    assert err.max() <= 2.0 ** -26
    assert m64.shape == (1 + S().window_count(n)[1] // 160, 40)


def test_state_dict_is_resemblyzers():
    enc = pkg().VoiceEncoder()
    ref = R.Net()
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want
    assert want['lstm.weight_ih_l0'] == (1024, 40) and want['lstm.weight_ih_l2'] == (1024, 256) and want['linear.weight'] == (256, 256)
    assert len(want) == 14
    ref.load_state_dict(enc.state_dict(), strict=True)
    enc.load_state_dict(R.state_dict(1), strict=True)


def test_loader_takes_the_checkpoint_wrapping(tmp_path):
    sd = R.state_dict(2)
    ck = {'step': 1, 'model_state': dict(sd, similarity_weight=torch.tensor([10.0]), similarity_bias=torch.tensor([-5.0]))}
    torch.save(ck, tmp_path / 'pretrained.pt')
    torch.save(sd, tmp_path / 'plain.pt')
    for name in ('pretrained.pt', 'plain.pt'):
        enc = pkg().load_voice_encoder(str(tmp_path / name), 'cpu')
        got = enc.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    torch.save(dict(sd, extra=torch.zeros(1)), tmp_path / 'bad.pt')
    with pytest.raises(RuntimeError):
        pkg().load_voice_encoder(str(tmp_path / 'bad.pt'), 'cpu')


def test_speaker_similarity_against_the_reference_lines():
    te, tt, re_, rs = R.similarity_case()
    cent, cos, pred, acc = R.similarity_numpy(te.astype(np.float64), tt, re_.astype(np.float64), rs, 16)
    out = pkg().speaker_similarity(torch.from_numpy(te), torch.from_numpy(tt), torch.from_numpy(re_), torch.from_numpy(rs), 16)
    assert out['centroids'].shape == (16, 256) and out['cos'].shape == (48,) and out['pred'].dtype == torch.int64
    assert np.abs(out['centroids'].numpy() - cent).max() <= 8 * 2.0 ** -24
    assert np.abs(out['cos'].numpy() - cos).max() <= 64 * 2.0 ** -24
    assert np.array_equal(out['pred'].numpy(), pred) and abs(float(out['accuracy']) - acc) < 1e-6
    assert 0.5 < acc < 1.0                                                  # the case has both hits and misses
    two = torch.tensor([[1.0, 0.0], [0.0, 1.0]])                            # a tie: the lowest index wins
    tie = pkg().speaker_similarity(torch.tensor([[0.5, 0.5]]), torch.tensor([1]), two, torch.tensor([0, 1]), 2)
    assert int(tie['pred'][0]) == 0 and float(tie['accuracy']) == 0.0


def test_no_cpu_fallback():
    P = pkg()
    sp = P.speaker
    enc = P.VoiceEncoder()
    x = torch.zeros(2, 1, 26000)
    w = [tuple(torch.zeros(s) for s in ((1024, 40), (1024, 256), (1024,), (1024,)))]
    for fn in (lambda: sp.voice_mel(x), lambda: enc.embed_utterance(x), lambda: enc(torch.zeros(1, 160, 40)),
               lambda: sp.lstm_fwd(torch.zeros(1, 160, 40), torch.zeros(1, 2, dtype=torch.int32), w)):
        with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
            fn()
    for name in ('VoiceEncoder', 'load_voice_encoder', 'voice_mel', 'lstm_fwd', 'partial_slices', 'window_count', 'speaker_similarity'):
        assert getattr(P, name) is getattr(sp, name)


def test_symbols_are_declared_bound_and_built():
    names = ['tdvc_voice_window_count', 'tdvc_voice_windows', 'tdvc_voice_gain', 'tdvc_voice_mel', 'tdvc_lstm_workspace', 'tdvc_lstm_fwd',
             'tdvc_voice_embed']
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    for n in names:
        assert n in pkg()._lib.SIGNATURES and re.search(r'\b%s\(' % n, header), n
    mk = open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\beval_speaker\.hip\b', mk, re.M)
    assert 'parity with an installed resemblyzer / librosa is unchecked' in pkg().speaker.__doc__
    assert 'PARITY WITH AN INSTALLED RESEMBLYZER / LIBROSA IS UNCHECKED' in header
    lib = pkg()._lib.lib()
    assert lib.tdvc_lstm_workspace(1, 160, 257, 1, 160, 3) == 0 and lib.tdvc_lstm_workspace(1, 160, 40, 1, 161, 3) == 0
    assert lib.tdvc_lstm_workspace(1, 160, 40, 1, 160, 4) == 0 and True
    # packed W_hh and W_ih of three layers (input size 40 padded to 48), 160 projected frames of 1024 floats, 160 hidden states of 256
    assert lib.tdvc_lstm_workspace(1, 160, 40, 1, 160, 3) == 3 * 2 ** 20 + (48 + 256 + 256) * 4096 + 160 * 4096 + 160 * 1024
