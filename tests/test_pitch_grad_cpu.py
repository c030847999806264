"""CPU: the gradient fixture (tests/golden/yin_grad.npz + yin_grad.json, tools/make_golden_yin_grad.py) still pins
tests/yin_grad_ref.py to the reference's float64 gradient and still meets the conditions its generator asserted; the host side of
tdvc_yin_soft_bwd (declared, exported, signed; argument checks happen before any launch); the opt-in switch of the lambda_f0 term."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import yin_grad_ref as GR
import yin_ref as YR
from common import ROOT, pkg

CASES = tuple(GR.CASES)


@pytest.mark.parametrize('name', CASES)
def test_fixture_pins_helper_gradient_to_reference(name):
    """The float64 helper gradient reproduces the sampled entries of the reference's float64 gradient within 1e-9 of the row's
    max |gradient|, zero rows exactly; and the recorded conditions hold when recomputed."""
    meta, g = GR.fixture()
    t = GR.truth(name)
    s = t['meta']
    assert {k: s[k] for k in t['settings']} == t['settings']
    assert tuple(t['x'].shape) == (s['B'], s['T']) == tuple(t['dx'].shape) and t['x'].dtype == torch.float32
    assert tuple(t['gy'].shape) == (s['B'], s['n_frames']) and bool(torch.isfinite(t['dx']).all())
    idx, val, row_max = g[f'{name}_grad_idx'], g[f'{name}_grad_val'], g[f'{name}_row_max']
    assert len(idx) == min(GR.N_SAMPLED, t['dx'].numel()) and len(np.unique(idx)) == len(idx)
    rows = idx // s['T']
    err = np.abs(t['dx'].reshape(-1).numpy()[idx] - val)
    live = row_max[rows] > 0
    assert not err[~live].any() and not val[~live].any()
    assert float((err[live] / row_max[rows][live]).max(initial=0.0)) <= 1e-9
    assert np.allclose(t['dx'].abs().amax(-1).numpy(), row_max, rtol=1e-9, atol=0)
    assert [int(i) for i in np.nonzero(row_max == 0)[0]] == s['zero_rows']
    # recorded by the generator
    assert s['helper_vs_reference'] <= 1e-9 and s['helper_zero_rows_match']
    assert s['tol_g'] == 4 * min(s['E_ref32'], s['E_plain32'])
    assert s['on_frames'] == int(t['on'].sum())
    ymeta, _ = YR.fixture()
    assert s['cmdf_tol'] == ymeta['cases'][s['cmdf_tol_case']]['tol']
    if s['on_frames'] > 0 and name != 'silence':
        # EVERY frame's on/off decision is out of an fp32 kernel's reach: no frame is excused from the gradient comparison
        assert float(t['margin'].min()) > 2 * s['cmdf_tol']
        assert 1e-6 <= s['tol_g'] <= 2e-5, s['tol_g']
    if name in ('short', 'silence'):
        assert s['tol_g'] == 0.0 and not bool(t['dx'].any())
    if name == 'short':
        assert not bool(t['on'].any())
    if name == 'silence':
        assert bool(t['on'].all()) and not bool(t['cmdf'].any()) and bool((t['f0'] > 0).all())
    if name == 'default':
        assert s['zero_rows'] == [1] and not bool(t['on'][1].any()) and (s['tau_min'], s['tau_max']) == (0, 800)
    if name == 'min':
        assert s['T'] == 600 and 2 * s['tau_max'] == 532 and s['on_frames'] == 4 and s['n_frames'] == 10
    if name == 'speech':
        assert 0.35 <= float((t['gy'] == 0).double().mean()) <= 0.65


def test_faint_case_has_the_floor_active_and_inactive_inside_on_frames():
    t = GR.truth('faint')
    s = t['settings']
    mixed, dist, n_on = GR.floor_facts(t['x'], s['tau_min'], s['tau_max'], s['stride'], 0.1)
    assert s['tau_min'] <= 1 and mixed and dist >= 1e-3 and n_on == t['meta']['on_frames'] > 0
    assert t['meta']['scale'] in GR.FAINT_SCALES
    assert torch.equal(t['x'], (GR.base_signal('faint').double() * t['meta']['scale']).float())


def test_long_case_record():
    """The inference-length case is not recomputed on the CPU suite: its record must carry what the GPU test relies on."""
    meta, g = GR.fixture()
    s = meta['cases']['long']
    ymeta, _ = YR.fixture()
    assert (s['B'], s['T']) == (1, YR.LONG_T) and s['n_frames'] == 1120 and s['cmdf_tol'] == ymeta['long']['tol']
    assert s['helper_vs_reference'] <= 1e-9 and s['tol_g'] == 4 * min(s['E_ref32'], s['E_plain32']) and 1e-6 <= s['tol_g'] <= 2e-5
    assert s['min_margin'] > 2 * s['cmdf_tol'] and len(g['long_grad_idx']) == GR.N_SAMPLED


def test_fixture_is_small():
    size = sum(os.path.getsize(os.path.join(GR.GOLDEN, n)) for n in ('yin_grad.npz', 'yin_grad.json'))
    assert size <= 300 * 1024, size


def test_soft_bwd_is_declared_exported_and_signed():
    L = pkg()._lib
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = L.lib()
    for name in ('tdvc_yin_soft_bwd', 'tdvc_yin_soft_bwd_workspace'):
        assert name + '(' in header and name in L.SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.tdvc_yin_soft_bwd_workspace.restype is C.c_size_t and len(L.SIGNATURES['tdvc_yin_soft_bwd'][1]) == 14
    # du [B][n_frames][2 * tau_max] floats; the sizes DESIGN.md quotes
    assert lib.tdvc_yin_soft_bwd_workspace(16, 16000, 266, 64) == 16 * 250 * 532 * 4
    assert lib.tdvc_yin_soft_bwd_workspace(1, 71680, 266, 64) == 1120 * 532 * 4
    for bad in ((0, 4000, 266, 64), (2, 0, 266, 64), (2, 4000, 0, 64), (2, 4000, 266, 0)):
        assert lib.tdvc_yin_soft_bwd_workspace(*bad) == 0, bad


def test_soft_bwd_validates_arguments_before_any_launch():
    """The checks and status codes of tdvc_yin_f0, plus TDVC_EWORKSPACE (-2) for a null or too small workspace. Host only: with a bad
    argument nothing is launched and no pointer is dereferenced, so this runs without a GPU."""
    L = pkg()._lib
    lib = L.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    need = lib.tdvc_yin_soft_bwd_workspace(1, 4000, 266, 64)

    def call(T=4000, tau_min=32, tau_max=266, stride=64, B=1, x_bs=None, sr=16000.0, x=p, gy=p, dx=p, ws=p, ws_bytes=None):
        return lib.tdvc_yin_soft_bwd(x, T if x_bs is None else x_bs, B, T, tau_min, tau_max, stride, 0.1, sr, gy, dx, ws,
                                     need if ws_bytes is None else ws_bytes, None)
    assert call(T=0) == -1 and b'T' in lib.tdvc_last_error()
    assert call(stride=0) == -1 and b'stride' in lib.tdvc_last_error()
    assert call(tau_min=32, tau_max=34) == -1 and b'tau' in lib.tdvc_last_error()
    assert call(tau_min=0, tau_max=2) == -1 and call(tau_min=-1) == -1
    assert call(tau_max=1025) == L.EUNSUPPORTED and b'1024' in lib.tdvc_last_error()
    assert call(T=-3) == -1 and call(stride=-64) == -1 and call(B=0) == -1 and call(x_bs=-1) == -1 and call(sr=0.0) == -1
    for null in ('x', 'gy', 'dx'):
        assert call(**{null: None}) == -1 and b'null' in lib.tdvc_last_error(), null
    assert call(ws=None) == -2 and b'workspace' in lib.tdvc_last_error()
    assert call(ws_bytes=need - 1) == -2 and b'small' in lib.tdvc_last_error()
    assert call(ws_bytes=0) == -2


def _stage1_train():
    P = pkg()
    return P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml')).train


def test_from_hparams_default_still_warns_and_skips_the_term():
    SC = pkg().train_step.StepConfig
    with pytest.warns(UserWarning, match='lambda_f0'):
        cfg = SC.from_hparams(_stage1_train())
    assert cfg.f0_loss is None and cfg.lambda_f0 == 1000.0
    assert SC().f0_loss is None


def test_from_hparams_yin_turns_the_term_on_without_a_warning():
    SC = pkg().train_step.StepConfig
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        cfg = SC.from_hparams(_stage1_train(), f0_loss='yin')
    assert cfg.f0_loss == 'yin' and cfg.lambda_f0 == 1000.0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        base = SC.from_hparams(_stage1_train())
    assert {k: v for k, v in vars(cfg).items() if k != 'f0_loss'} == {k: v for k, v in vars(base).items() if k != 'f0_loss'}
    with pytest.raises(ValueError):
        SC.from_hparams(_stage1_train(), f0_loss='crepe')


def test_f0_yin_loss_and_soft_track_need_a_device_tensor():
    P = pkg()
    with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
        P.losses.f0_yin_loss(torch.zeros(2, 1, 8960, requires_grad=True), torch.zeros(2, 1, 141))
    with pytest.raises(P._lib.TdvcError):
        P.track_f0(torch.zeros(1, 1, 8960), soft=True)
