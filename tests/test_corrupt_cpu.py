"""CPU: the random-EQ fixture (tests/golden/peq.npz + peq.json, tools/make_golden_peq.py) still pins tests/peq_ref.py to the reference's
own random_eq + eq_rms_signals output, and the host side of tdvc_peq_sos / tdvc_sos_filter / corrupt.py (argument checks happen before
any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import peq_ref as PR
from common import ROOT, pkg


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_restatement_reproduces_the_reference_output():
    """sos within 1e-13 (relative to the largest coefficient), the cascade and the RMS-matched signal within 1e-12 of the row maximum,
    against what the reference's random_eq / eq_rms_signals returned for the stored draws."""
    meta, g = PR.fixture()
    x, G, z = g['speech_signal'], g['speech_G'], g['speech_z']
    assert x.dtype == np.float32 and x.shape == (2, 4000) and G.shape == z.shape == (2, 10)
    assert (np.abs(G) <= 12).all() and ((z >= 0) & (z <= 1)).all()
    sos, y = PR.random_eq(x, G, z, match=False)
    assert relmax(sos, g['speech_sos']) <= 1e-13
    assert np.all(g['speech_sos'][..., 3] == 1.0)
    for b in range(2):
        assert relmax(y[b], g['speech_y'][b]) <= 1e-12
        assert relmax(PR.match_rms(y, x)[b], g['speech_y_rms'][b]) <= 1e-12
    s = meta['cases']['speech']
    assert max(s['helper_sos_rel'], s['helper_y_rel'], s['helper_y_rms_rel']) <= 1e-13      # recorded by the generator
    # rounding the draws to fp32, as tdvc_peq_sos takes them, stays well inside the GPU bound
    assert float((np.abs(PR.truth('speech')['y_rms'] - g['speech_y_rms']) / PR.bound(g['speech_y_rms'])).max()) <= 0.25
    assert np.allclose(PR.FC[[0, -1]], [60.0, 7600.0], rtol=1e-12) and np.allclose(np.diff(np.log(PR.FC)), np.log(7600 / 60) / 9, rtol=1e-12)


@pytest.mark.parametrize('name', [n for n in PR.CASES if n != 'long'])
def test_restatement_agrees_with_scipy(name):
    sps = pytest.importorskip('scipy.signal')
    t = PR.truth(name)
    for b in range(len(t['x'])):
        ref = sps.sosfilt(t['sos'][b], t['x'][b].astype(np.float64))
        assert float(np.abs(t['y'][b] - ref).max()) <= 1e-12 * max(float(np.abs(ref).max()), 1e-300), name
    _, g = PR.fixture()
    x0 = g['speech_signal'][0]
    for n in (1, 3):
        ref = sps.sosfilt(g['sections_sos'][:n], x0.astype(np.float64))
        assert relmax(PR.sosfilt(g['sections_sos'][:n], x0), ref) <= 1e-12


@pytest.mark.parametrize('name', ['speech', 'boost', 'cut', 'odd'])
def test_fp32_cascade_misses_the_gpu_bound(name):
    """The discrimination behind the GPU bound 4 * 2^-24 * max|row|: the float64 result rounded once sits inside it, the same cascade
    with fp32 coefficients and state misses it by 50x or more on every speech-like row."""
    t = PR.truth(name)
    bd = PR.bound(t['y'])
    assert float((np.abs(t['y'].astype(np.float32) - t['y']) / bd).max()) <= 0.25 + 1e-9
    ratio = (np.abs(PR.fp32_run(name) - t['y']) / bd).max(-1)
    print(name, 'fp32 cascade / bound per row:', ratio)
    assert float(ratio.min()) >= 50


def test_silence_and_fixture_size():
    t = PR.truth('silence')
    assert not t['y'].any() and not t['y_rms'].any() and np.isfinite(t['y_rms']).all()
    size = {n: os.path.getsize(os.path.join(PR.GOLDEN, n)) for n in ('peq.npz', 'peq.json', 'yin.npz')}
    assert size['peq.npz'] <= size['yin.npz'] and size['peq.json'] <= size['yin.npz'], size


def test_symbols_in_header_binding_and_library():
    L = pkg()._lib
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = L.lib()
    for name in ('tdvc_peq_sos', 'tdvc_sos_filter', 'tdvc_sos_filter_workspace'):
        assert re.search(rf'\b{name}\(', header), name
        assert name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert os.path.exists(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'audio_eq.hip'))
    assert 'audio_eq.hip' in open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()


def test_entry_points_validate_arguments_before_any_launch():
    """n_sections outside 1..16 and T < 0 are TDVC_EUNSUPPORTED (-4); B == 0 and T == 0 are no-ops; n_bands < 2 is TDVC_EINVAL (-1).
    Checked on the host with a null stream: nothing is launched, so this runs without a GPU (the pointers are never dereferenced)."""
    L = pkg()._lib
    lib = L.lib()
    buf = (C.c_double * 128)()
    p = C.cast(buf, C.c_void_p)

    def filt(B=1, T=8, S=10):
        return lib.tdvc_sos_filter(p, T, p, B, T, S, 1, p, T, None, 0, None)
    assert filt(S=17) == L.EUNSUPPORTED and b'n_sections' in lib.tdvc_last_error()
    assert filt(S=0) == L.EUNSUPPORTED and filt(T=-1) == L.EUNSUPPORTED
    assert filt(B=0) == 0 and filt(T=0) == 0
    assert filt(B=-1) == -1
    assert lib.tdvc_sos_filter(None, 8, p, 1, 8, 10, 0, p, 8, None, 0, None) == -1            # null input
    assert lib.tdvc_sos_filter(p, 8, p, 2, 8, 10, 0, p, 4, None, 0, None) == -1               # output rows would overlap
    assert lib.tdvc_sos_filter_workspace(16, 16000, 10) >= 0
    assert lib.tdvc_peq_sos(p, p, p, 1, 16000.0, 1, p, None) == -1 and b'n_bands' in lib.tdvc_last_error()
    assert lib.tdvc_peq_sos(p, p, p, 10, 0.0, 1, p, None) == -1
    assert lib.tdvc_peq_sos(p, p, p, 10, 16000.0, 0, p, None) == 0


def test_corrupt_needs_a_device_tensor():
    P = pkg()
    x = torch.zeros(2, 4000)
    sos = torch.zeros(2, 10, 6, dtype=torch.float64)
    for call in (lambda: P.corrupt.sos_filter(x, sos), lambda: P.corrupt.random_eq(x), lambda: P.corrupt.corrupt_audio(x),
                 lambda: P.corrupt.peq_sos(torch.zeros(2, 10), torch.ones(2, 10)),
                 lambda: P.corrupt.device_batch(x[:, None], torch.zeros(2, dtype=torch.int64), 16)):
        with pytest.raises(P._lib.TdvcError):
            call()
    assert P.corrupt_audio is P.corrupt.corrupt_audio and P.sos_filter is P.corrupt.sos_filter and P.device_batch is P.corrupt.device_batch
    assert np.allclose(P.corrupt.FC, PR.FC, rtol=1e-14, atol=0)


def test_pair_targets_on_the_host():
    """The pairing is plain tensor indexing: checkable on CPU tensors."""
    P = pkg()
    lbl = torch.tensor([3, 0, 7, 7])
    perm, tgt, c_src, c_tgt = P.corrupt.pair_targets(lbl, 16, perm=torch.tensor([2, 3, 0, 1]))
    assert tgt.tolist() == [7, 7, 3, 0] and c_src.shape == c_tgt.shape == (4, 16) and c_src.dtype == torch.float32
    assert torch.equal(c_src.argmax(1), lbl) and torch.equal(c_tgt.argmax(1), tgt) and float(c_src.sum()) == 4.0
    perm, tgt, *_ = P.corrupt.pair_targets(lbl, 16, conversion=False)
    assert perm.tolist() == [0, 1, 2, 3] and torch.equal(tgt, lbl)
    g = torch.Generator().manual_seed(5)
    perm, *_ = P.corrupt.pair_targets(lbl, 16, generator=g)
    assert sorted(perm.tolist()) == [0, 1, 2, 3]
