"""GPU: tdvc_yin_f0 (csrc/pitch_yin.hip, pitch_yin.h) and tdvc_yin_soft_bwd (csrc/pitch_yin_bwd.hip) at the shapes the fixtures
yin.npz / yin_grad.npz never reach, against the float64 helper tests/yin_edges_ref.py, which tests/golden/yin_edges.npz pins to the
reference's own YIN (tests/test_pitch_edges_cpu.py): odd tau_max (L % 4 == 2), the cap tau_max = 1024 and 1023, NC = 2 and NC >= 4,
NG < 64, n = 2, stride > L, stride 1, T < L and T = 1. The table and what each row reaches: yin_edges_ref.CASES.

Every case goes in as a slice of a wider NaN-filled buffer (row stride T + 37, offset 5): a read outside [0, T) of a row shows up
as NaN. The lags are passed as integers (pitch._yin), so tau_min / tau_max / stride are exact.

Tolerances come from the fixture, not from the kernel, by the rule of the sibling tests: tol = 4 * min(E_ref32, E_plain32) on the
CMDF; hard f0 agrees (rel 1e-6) and soft f0 is within max(4 * S_ref32, 1e-6) relative on every frame whose float64 decision margin
exceeds 2*tol; the soft on/off decision agrees on EVERY frame (the fixture keeps every |min c - threshold| above 2*tol); every
element of dx is within tol_g * max |truth row|, tol_g = 4 * min(Eg_ref32, Eg_plain32) <= 1e-4, and rows whose truth is zero are
exactly zero. tiny3 and one33 are forward only (yin_edges_ref.FORWARD_ONLY has the reasons).

Measured on an MI355X (printed by the tests, run with -s; hard f0 disagreements, soft on/off disagreements and excused frames 0
in every case):
    case       CMDF max abs err   tol         soft f0 max rel err   bound       grad row-normalised max err   tol_g
    odd267     3.876e-07          1.180e-06   1.249e-07             5.578e-06   5.412e-07                     4.536e-06
    cap1024    5.425e-07          1.572e-06   2.208e-07             1.354e-06   8.113e-07                     4.548e-06
    odd1023    4.749e-07          1.705e-06   5.825e-08             2.436e-06   3.728e-07                     1.534e-05
    nc4_255    5.088e-07          1.751e-06   3.184e-07             8.675e-06   1.393e-06                     3.658e-06
    nc2_401    4.676e-07          1.231e-06   1.420e-07             3.711e-06   5.824e-07                     3.476e-06
    gap64      2.411e-07          7.747e-07   1.352e-07             8.726e-06   3.924e-07                     1.826e-06
    dense21    2.984e-07          1.022e-06   2.188e-07             4.481e-06   7.794e-06                     3.147e-05
    n2_133     1.297e-07          3.974e-07   6.009e-08             1.000e-06   1.689e-07                     2.381e-06
    short101   2.758e-07          1.019e-06   4.643e-08             1.000e-06   1.966e-05                     6.383e-05
    tiny7      2.182e-07          7.794e-07   0                     1.000e-06   5.837e-06                     8.430e-06
    tiny5      1.450e-07          6.409e-07   3.052e-08             1.000e-06   8.444e-06                     2.078e-05
    tiny3      1.300e-07          5.230e-07   0                     1.000e-06   forward only
    one33      1.550e-07          3.267e-07   3.815e-09             1.000e-06   forward only

What this table found. tiny5 first failed its gradient check: row 1, max |truth| 1.7e-16, came back with an element of -0.053. In
frame 9 of that row the softmax is saturated on k* = 3 (every other weight below 1e-26), yet the kernel's tau was 3 + 1 ulp, and
(k* - tau) * g_tau * 100 = -2.4e-7 * 4.3e4 was the frame's whole gradient (du of the frame = -0.01025 * d c[3] / d u, element
by element). Cause: the weight was exp(-100 c + 100 min c), the compiler contracted it into an FMA, so the minimum's own weight
was exp(-3.3e-7) = 1 - 6 * 2^-24 instead of 1, and fl(fl(3 e) / e) = 3 + 2^-22. The weight is now exp(100 (min c - c)), exactly 1
at the minimum (pitch_yin.h, yin_soft_weight); every other check here passed before and after.
"""
import functools

import pytest
import torch

import yin_edges_ref as ER
import yin_grad_ref as GR
from common import pkg
from edge_support import poison_lds

pytestmark = pytest.mark.gpu
SR, THR = ER.SR, ER.THR
SENT = -12345.0          # neither an f0, a CMDF entry (both >= 0) nor NaN
PAD = 19                 # sentinel floats before and after an output handed to the C entry points
WS_PAD = 68              # sentinel bytes around the workspace


def wide_slice(x, dev):
    """x [B, T] as a slice of a NaN-filled [B, T + 37] device buffer, offset 5."""
    B, T = x.shape
    wide = torch.full((B, T + 37), float('nan'), device=dev)
    wide[:, 5:5 + T] = x.to(dev)
    sl = wide[:, 5:5 + T]
    assert sl.stride(0) == T + 37 and sl.data_ptr() == wide.data_ptr() + 20
    return sl


def args(s):
    return SR, s['tau_min'], s['tau_max'], s['stride'], THR


def run_forward(name, soft, dev='cuda'):
    s = ER.settings(name)
    f0, c = pkg().pitch._yin(wide_slice(ER.truth(name)['x'], dev), *args(s), soft, True)
    torch.cuda.synchronize()
    return f0.cpu(), c.cpu()


def run_backward(name, gy=None, dev='cuda'):
    """(dx, f0) of the autograd path on the wide slice."""
    t = ER.truth(name)
    x = wide_slice(t['x'], dev).detach().requires_grad_()
    f0 = pkg().pitch._yin(x, *args(t['settings']), True, False)
    assert f0.grad_fn is not None
    f0.backward((t['gy'].float() if gy is None else gy).to(dev))
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape
    return x.grad.cpu(), f0.detach().cpu()


@functools.lru_cache(maxsize=None)
def device_forward(name, soft):
    """Computed once per session and left unchanged."""
    return run_forward(name, soft)


@functools.lru_cache(maxsize=None)
def device_backward(name):
    return run_backward(name)


def guarded(n, fill, dev, dtype=torch.float32, pad=PAD, sent=SENT):
    """(whole buffer, the n elements in its middle pre-filled with `fill`), `pad` sentinels on both sides."""
    big = torch.full((pad + n + pad,), sent, dtype=dtype, device=dev)
    mid = big[pad:pad + n]
    mid.fill_(fill)
    return big, mid


def guards_intact(big, n, pad=PAD, sent=SENT):
    return bool((big[:pad] == sent).all()) and bool((big[pad + n:] == sent).all())


@pytest.mark.parametrize('name', tuple(ER.CASES))
def test_yin_edges_forward_vs_float64_helper(dev, name):
    t = ER.truth(name)
    s = t['meta']
    f0, c = device_forward(name, False)
    f0s, cs = device_forward(name, True)
    assert f0.shape == f0s.shape == t['hard'].shape and c.shape == t['cmdf'].shape
    assert f0.dtype == f0s.dtype == c.dtype == torch.float32
    assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(f0).all()) and bool(torch.isfinite(f0s).all())
    assert torch.equal(c, cs)
    err = float((c.double() - t['cmdf']).abs().max())
    ok = t['ok']
    hard_bad = ((f0.double() - t['hard']).abs() > 1e-6 * t['hard']) & ok
    rel = (f0s.double() - t['soft']).abs() / t['soft'].abs().clamp_min(1e-30)
    rel = torch.where((t['soft'] == 0) & (f0s == 0), torch.zeros_like(rel), rel)
    soft_err = float(rel[ok].max()) if bool(ok.any()) else 0.0
    soft_bound = max(4 * s['S_ref32'], 1e-6)
    decision_bad = int(((f0s > 0) != t['on']).sum())
    print(f'\nyin edges {name}: CMDF max abs err {err:.3e} (tol {s["tol"]:.3e}), hard f0 disagreements {int(hard_bad.sum())} of {int(ok.sum())} '
          f'non-excused frames (excused {float((~ok).double().mean()):.3f}), soft f0 max rel err {soft_err:.3e} (bound {soft_bound:.3e}), '
          f'soft on/off disagreements {decision_bad} of {ok.numel()}')
    assert err <= s['tol'], (name, err, s['tol'])
    assert not bool(hard_bad.any()), (name, int(hard_bad.sum()))
    assert soft_err <= soft_bound, (name, soft_err, soft_bound)
    assert decision_bad == 0, (name, decision_bad)


@pytest.mark.parametrize('soft', [False, True], ids=['hard', 'soft'])
@pytest.mark.parametrize('name', tuple(ER.CASES))
def test_yin_edges_forward_c_entry_writes_all_and_nothing_else(dev, name, soft):
    """f0 and cmdf inside larger sentinel-filled buffers: every element written, same bits as the wrapper's, sentinels untouched."""
    L = pkg()._lib
    s = ER.settings(name)
    x = wide_slice(ER.truth(name)['x'], dev)
    nf0, nc = s['B'] * s['n_frames'], s['B'] * s['n_frames'] * s['n']
    big_f, f0 = guarded(nf0, SENT, dev)
    big_c, c = guarded(nc, SENT, dev)
    L.check(L.lib().tdvc_yin_f0(x.data_ptr(), s['T'] + 37, s['B'], s['T'], s['tau_min'], s['tau_max'], s['stride'], THR, int(soft), float(SR),
                                f0.data_ptr(), c.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert not bool((f0 == SENT).any()) and not bool((c == SENT).any())
    assert guards_intact(big_f, nf0) and guards_intact(big_c, nc)
    ref_f0, ref_c = device_forward(name, soft)
    assert torch.equal(f0.cpu(), ref_f0.reshape(-1)) and torch.equal(c.cpu(), ref_c.reshape(-1))


def check_rows(what, dx, truth, tol):
    """Element by element within tol * max |truth row|; zero rows exactly zero; everything finite."""
    assert dx.shape == truth.shape and dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    scale = truth.abs().amax(-1, keepdim=True)
    err = GR.row_error(dx, truth)
    print(f'\nyin edges grad {what}: row-normalised max err {err:.3e} (tol_g {tol:.3e}), zero rows {int((scale == 0).sum())} of {scale.numel()}')
    zero = (scale == 0).expand_as(truth)
    assert not bool(dx[zero].any()), what
    assert bool(((dx.double() - truth).abs() <= tol * scale).all()), (what, err, tol)


@pytest.mark.parametrize('name', ER.BACKWARD_CASES)
def test_yin_edges_backward_vs_float64_helper(dev, name):
    t = ER.truth(name)
    dx, f0 = device_backward(name)
    assert torch.equal(f0, device_forward(name, True)[0])              # the autograd path returns the plain call's bits
    assert torch.equal(f0 > 0, t['on'])
    check_rows(name, dx, t['dx'], t['meta']['tol_g'])


def c_backward(name, gy, dev):
    """tdvc_yin_soft_bwd on NaN-filled dx inside sentinels, the workspace exactly the queried byte count cut out of a larger
    sentinel-filled buffer -> dx [B, T] on the host, after checking that dx is fully written and every sentinel is intact."""
    L = pkg()._lib
    lib = L.lib()
    s = ER.settings(name)
    x = wide_slice(ER.truth(name)['x'], dev)
    B, T = s['B'], s['T']
    nb = lib.tdvc_yin_soft_bwd_workspace(B, T, s['tau_max'], s['stride'])
    assert nb == B * s['n_frames'] * s['L'] * 4
    big_dx, dx = guarded(B * T, float('nan'), dev)
    big_ws, ws = guarded(nb, 0x5A, dev, dtype=torch.uint8, pad=WS_PAD, sent=0xA5)
    gy = gy.float().to(dev).contiguous()
    L.check(lib.tdvc_yin_soft_bwd(x.data_ptr(), T + 37, B, T, s['tau_min'], s['tau_max'], s['stride'], THR, float(SR), gy.data_ptr(),
                                  dx.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dx).any()), name
    assert guards_intact(big_dx, B * T) and guards_intact(big_ws, nb, WS_PAD, 0xA5), name
    return dx.reshape(B, T).cpu()


@pytest.mark.parametrize('name', ER.BACKWARD_CASES)
def test_yin_edges_backward_c_entry_writes_all_and_nothing_else(dev, name):
    t = ER.truth(name)
    assert torch.equal(c_backward(name, t['gy'], dev), device_backward(name)[0])
    assert not bool(c_backward(name, torch.zeros_like(t['gy']), dev).any())          # gy all zero: dx all zero


@pytest.mark.parametrize('name', ['cap1024', 'odd1023', 'dense21', 'tiny5'])
def test_yin_edges_poisoned_lds(dev, name):
    """The LDS of every CU pre-filled with NaN bit patterns before the forward and before the backward: finite, and the clean run's
    bits. A read of LDS that the kernel has not written, landing anywhere but in a term a select discards, shows up as NaN."""
    for soft in (False, True):
        poison_lds(dev)
        f0, c = run_forward(name, soft)
        assert bool(torch.isfinite(f0).all()) and bool(torch.isfinite(c).all())
        assert torch.equal(f0, device_forward(name, soft)[0]) and torch.equal(c, device_forward(name, soft)[1])
    poison_lds(dev)
    dx, f0 = run_backward(name)
    assert bool(torch.isfinite(dx).all())
    assert torch.equal(dx, device_backward(name)[0]) and torch.equal(f0, device_backward(name)[1])


@pytest.mark.parametrize('name', ['odd267', 'cap1024'])
def test_yin_edges_repeat_runs_are_bit_identical(dev, name):
    for soft in (False, True):
        f0, c = run_forward(name, soft)
        assert torch.equal(f0, device_forward(name, soft)[0]) and torch.equal(c, device_forward(name, soft)[1])
    dx, f0 = run_backward(name)
    assert torch.equal(dx, device_backward(name)[0]) and torch.equal(f0, device_backward(name)[1])
