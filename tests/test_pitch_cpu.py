"""CPU: the YIN fixture (tests/golden/yin.npz + yin.json, tools/make_golden_yin.py) still pins tests/yin_ref.py to the reference's
float64 results, and the host side of tdvc_yin_num_frames / tdvc_yin_f0 / pitch.yin_f0 (argument checks happen before any launch)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import yin_ref as YR
from common import pkg


@pytest.mark.parametrize('name', YR.CASES)
def test_fixture_pins_helper_to_reference(name):
    """The float64 helper reproduces what the reference computed in float64: hard f0 exactly, the sampled CMDF entries within
    1e-12, the stored margins; and the fixture still meets the conditions its generator asserted."""
    meta, g = YR.fixture()
    t = YR.truth(name)
    s = t['meta']
    assert (s['tau_min'], s['tau_max'], s['stride']) == YR.params(meta['sample_rate'], s['pitch_min'], s['pitch_max'], s['stride'] / meta['sample_rate'])
    assert t['x'].dtype == torch.float32 and tuple(t['x'].shape) == (s['B'], s['T'])
    assert t['hard'].shape == (s['B'], s['n_frames']) == g[f'{name}_f0_hard'].shape
    assert torch.equal(t['hard'], torch.from_numpy(g[f'{name}_f0_hard']))
    idx, val = g[f'{name}_cmdf_idx'], g[f'{name}_cmdf_val']
    assert len(idx) == min(2048, t['cmdf'].numel())
    assert float(np.abs(t['cmdf'].reshape(-1).numpy()[idx] - val).max()) <= 1e-12
    assert float((t['soft'] - torch.from_numpy(g[f'{name}_f0_soft'])).abs().max()) <= 1e-9 * meta['sample_rate']
    assert np.allclose(t['margin'].numpy(), g[f'{name}_margin'], rtol=0, atol=1e-12)
    # recorded by the generator
    assert s['helper_hard_equals_reference'] and s['helper_cmdf_max_abs_diff'] <= 1e-12
    assert s['tol'] == 4 * min(s['E_ref32'], s['E_plain32'])
    voiced = float((t['hard'] > 0).double().mean())
    if name not in ('short', 'silence'):
        assert voiced >= 0.15 and 1 - voiced >= 0.15, voiced
    if name == 'silence':
        assert not bool(t['hard'].any()) and s['tol'] == 0.0
    assert float((~t['ok']).double().mean()) <= 0.05


def test_fixture_is_small():
    size = sum(os.path.getsize(os.path.join(YR.GOLDEN, n)) for n in ('yin.npz', 'yin.json'))
    assert size <= 300 * 1024, size


def test_yin_num_frames():
    lib = pkg()._lib.lib()
    meta, _ = YR.fixture()
    for name, s in meta['cases'].items():
        assert lib.tdvc_yin_num_frames(s['T'], s['tau_max'], s['stride']) == s['n_frames'] == YR.num_frames(s['T'], s['tau_max'], s['stride']), name
    assert lib.tdvc_yin_num_frames(71680, 266, 64) == 1120
    assert lib.tdvc_yin_num_frames(1, 266, 64) == (2 * 266 - 1) // 64 + 1          # shorter than a frame: extended to L first
    for bad in ((0, 266, 64), (-5, 266, 64), (4000, 0, 64), (4000, 266, 0), (4000, 266, -1)):
        assert lib.tdvc_yin_num_frames(*bad) <= 0, bad


def test_yin_f0_validates_arguments_before_any_launch():
    """T < 1, stride < 1 and fewer than two CMDF entries are TDVC_EINVAL (-1); tau_max > 1024 is TDVC_EUNSUPPORTED (-4). Checked on the
    host with a null stream: nothing is launched, so this runs without a GPU (the pointers are never dereferenced)."""
    L = pkg()._lib
    lib = L.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)

    def call(T=4000, tau_min=32, tau_max=266, stride=64):
        return lib.tdvc_yin_f0(p, T, 1, T, tau_min, tau_max, stride, 0.1, 0, 16000.0, p, None, None)
    assert call(T=0) == -1 and b'T' in lib.tdvc_last_error()
    assert call(stride=0) == -1 and b'stride' in lib.tdvc_last_error()
    assert call(tau_min=32, tau_max=34) == -1 and b'tau' in lib.tdvc_last_error()       # n = 1
    assert call(tau_min=0, tau_max=2) == -1
    assert call(tau_max=1025) == L.EUNSUPPORTED and b'1024' in lib.tdvc_last_error()
    assert call(T=-3) == -1 and call(stride=-64) == -1


def test_yin_f0_needs_a_device_tensor():
    P = pkg()
    with pytest.raises(P._lib.TdvcError):
        P.pitch.yin_f0(torch.zeros(2, 4000), 16000, 60, 500)
    with pytest.raises(P._lib.TdvcError):
        P.track_f0(torch.zeros(1, 1, 8960))
    assert P.yin_f0 is P.pitch.yin_f0 and P.infer.convert_audio
