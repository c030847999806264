"""GPU: tdvc_yin_f0 (csrc/pitch_yin.hip) through pitch.yin_f0 / track_f0 / infer.convert_audio against the float64 helper
tests/yin_ref.py, which tests/golden/yin.npz pins to the reference's own YIN (tests/test_pitch_cpu.py).

Tolerances come from the fixture, not from the kernel: tol = 4 * min(E_ref32, E_plain32) on the CMDF (the error of an fp32 evaluation
of the same formula, 4x for a different summation order); hard f0 must agree (rel 1e-6) on every frame whose float64 decision
margin exceeds 2*tol; soft f0 within max(4 * S_ref32, 1e-6) relative on those frames.

Measured on an MI355X (printed by the tests, run with -s; hard f0 disagreements 0 and excused frames 0 in every case):
    case      CMDF max abs err   tol         soft f0 max rel err   bound
    speech    4.720e-07          1.386e-06   1.960e-07             7.074e-06
    default   6.433e-07          2.109e-06   3.020e-07             5.150e-06
    short     2.864e-07          1.337e-06   0                     1.000e-06
    odd       4.569e-07          1.275e-06   1.100e-07             6.137e-06
    silence   0                  0           2.575e-08             1.000e-06
    long      5.685e-07          1.596e-06   3.252e-07             9.291e-06
"""
import functools

import numpy as np
import pytest
import torch

import yin_ref as YR
from common import build_models, pkg

pytestmark = pytest.mark.gpu
SR, THR = 16000, 0.1


def settings(s):
    return dict(sample_rate=SR, pitch_min=s['pitch_min'], pitch_max=s['pitch_max'], frame_stride=s['stride'] / SR, threshold=THR)


@functools.lru_cache(maxsize=None)
def device_result(name, soft):
    """(f0, cmdf) of one fixture case from the device, computed once per session and left unchanged."""
    t = YR.long_truth() if name == 'long' else YR.truth(name)
    f0, c = pkg().pitch.yin_f0(t['x'].cuda(), soft=soft, return_cmdf=True, **settings(t['meta']))
    torch.cuda.synchronize()
    return f0.cpu(), c.cpu()


def check_against_truth(name, t):
    s = t['meta']
    f0, c = device_result(name, False)
    f0s, _ = device_result(name, True)
    assert f0.shape == t['hard'].shape and c.shape == t['cmdf'].shape and f0.dtype == c.dtype == torch.float32
    assert bool(torch.isfinite(c).all())
    err = float((c.double() - t['cmdf']).abs().max())
    ok = t['ok']
    excused = float((~ok).double().mean())
    hard_bad = ((f0.double() - t['hard']).abs() > 1e-6 * t['hard']) & ok
    rel = (f0s.double() - t['soft']).abs() / t['soft'].abs().clamp_min(1e-30)
    rel = torch.where((t['soft'] == 0) & (f0s == 0), torch.zeros_like(rel), rel)
    soft_err = float(rel[ok].max()) if bool(ok.any()) else 0.0
    soft_bound = max(4 * s['S_ref32'], 1e-6)
    print(f'\nyin {name}: CMDF max abs err {err:.3e} (tol {s["tol"]:.3e}), hard f0 disagreements {int(hard_bad.sum())} of {int(ok.sum())} '
          f'non-excused frames (excused {excused:.3f}), soft f0 max rel err {soft_err:.3e} (bound {soft_bound:.3e})')
    assert err <= s['tol'], (name, err, s['tol'])
    assert excused <= 0.05
    assert not bool(hard_bad.any()), (name, int(hard_bad.sum()))
    assert soft_err <= soft_bound, (name, soft_err, soft_bound)
    return f0


@pytest.mark.parametrize('name', YR.CASES)
def test_yin_vs_float64_helper(dev, name):
    """CMDF, hard f0 and soft f0 of every fixture case; hard f0 also against the reference's own float64 f0 stored in the fixture."""
    t = YR.truth(name)
    f0 = check_against_truth(name, t)
    _, g = YR.fixture()
    ref = torch.from_numpy(g[f'{name}_f0_hard'])
    assert not bool((((f0.double() - ref).abs() > 1e-6 * ref) & t['ok']).any())
    if name == 'silence':
        assert not bool(f0.any())                                      # every frame, excused or not


def test_yin_inference_length_vs_float64_helper(dev):
    """B = 1, T = 71680 (test.max_segment), speech settings: 1120 frames in one launch."""
    check_against_truth('long', YR.long_truth())


def test_yin_poisoned_lds(dev):
    """The LDS of every CU pre-filled with NaN bit patterns: a read of LDS the kernel has not written shows up as NaN in the CMDF."""
    L = pkg()._lib
    t = YR.truth('odd')
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
    f0, c = pkg().pitch.yin_f0(t['x'].to(dev), return_cmdf=True, **settings(t['meta']))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(f0).all())
    assert float((c.cpu().double() - t['cmdf']).abs().max()) <= t['meta']['tol']
    assert torch.equal(c.cpu(), device_result('odd', False)[1]) and torch.equal(f0.cpu(), device_result('odd', False)[0])


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
def test_yin_layouts_repeat_runs_and_optional_cmdf(dev, soft):
    """The same signal as [B, T], [B, 1, T], [T] and as a slice of a wider buffer (x_bs != T) gives identical bits; so do two runs;
    so does a call that does not ask for the CMDF."""
    Pt = pkg().pitch
    t = YR.truth('odd')
    kw = dict(soft=soft, **settings(t['meta']))
    x = t['x'].to(dev)
    B, T = x.shape
    f0, c = Pt.yin_f0(x, return_cmdf=True, **kw)
    f0_b, c_b = Pt.yin_f0(x, return_cmdf=True, **kw)
    assert torch.equal(f0, f0_b) and torch.equal(c, c_b)
    assert torch.equal(f0.cpu(), device_result('odd', soft)[0])
    plain = Pt.yin_f0(x, **kw)
    assert torch.is_tensor(plain) and torch.equal(plain, f0)
    f0_3, c_3 = Pt.yin_f0(x[:, None, :], return_cmdf=True, **kw)
    assert f0_3.shape == (B, 1, f0.shape[-1]) and c_3.shape == (B, 1) + tuple(c.shape[1:])
    assert torch.equal(f0_3[:, 0], f0) and torch.equal(c_3[:, 0], c)
    wide = torch.full((B, T + 37), float('nan'), device=dev)
    wide[:, 5:5 + T] = x
    sl = wide[:, 5:5 + T]
    assert sl.stride(0) == T + 37 and not sl.is_contiguous()
    assert torch.equal(Pt.yin_f0(sl, **kw), f0)
    one = Pt.yin_f0(x[1], **kw)
    assert one.shape == f0.shape[1:] and torch.equal(one, f0[1])
    assert torch.equal(Pt.yin_f0(x.t().contiguous().t(), **kw), f0)          # last axis not dense: copied, same result


def test_track_f0_layout(dev):
    """[B, 1, T] -> [B, 1, T/64 + 1]: YIN's T/64 frames with the last one repeated (the frame f0_to_excitation drops)."""
    P = pkg()
    T = 8960
    rng = np.random.default_rng(11)
    x = torch.from_numpy(np.stack([YR.make_signal(rng, T) for _ in range(2)]))[:, None].to(dev)
    f0 = P.track_f0(x)
    assert f0.shape == (2, 1, T // 64 + 1)
    assert torch.equal(f0[..., -1], f0[..., -2])
    ref = P.yin_f0(x[:, 0], SR, 60, 500, 64 / SR)
    assert ref.shape == (2, T // 64) and torch.equal(f0[:, 0, :-1], ref)
    assert 0.15 < float((f0 > 0).float().mean()) < 0.95
    exc = P.util.f0_to_excitation(f0, 64)
    assert exc.shape == (2, 1, T)


def test_convert_audio_end_to_end(dev):
    """Waveform in, waveform out at T = 8960: convert_audio == convert fed with track_f0's own output times the ratio."""
    P = pkg()
    G, _ = build_models(dev)
    T = 8960
    rng = np.random.default_rng(12)
    x = torch.from_numpy(YR.make_signal(rng, T))[None, None].to(dev)
    c_tgt = torch.zeros(1, 16, device=dev); c_tgt[0, 3] = 1.0
    noise = (torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev),
             torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev))
    phi0 = torch.tensor([0.5], device=dev)
    y = P.infer.convert_audio(G, x, c_tgt, f0_ratio=1.25, noise=noise, start_phase=phi0)
    f0 = P.track_f0(x)
    assert bool((f0 > 0).any())
    y_ref = P.infer.convert(G, x, c_tgt, f0 * 1.25, noise=noise, start_phase=phi0)
    torch.cuda.synchronize()
    assert y.shape == (1, 1, T) and bool(torch.isfinite(y).all())
    assert torch.equal(y, y_ref)
    y_other = P.infer.convert(G, x, c_tgt, f0, noise=noise, start_phase=phi0)
    assert not torch.equal(y, y_other)                                        # the ratio reaches the excitation
