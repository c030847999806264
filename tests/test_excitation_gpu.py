"""tdvc_f0_to_excitation (f0_excitation_kernel, csrc/misc_kernels.hip) against the float64 reference tests/excitation_ref.py,
through util.f0_to_excitation with the draws passed in, at the lengths where the kernel's split of T samples over 256 threads
(per = ceil(T / 256), a serial scan over the 256 segment sums) changes shape: T = 1, T < 256, T = 256, T just above a multiple of
256 with trailing threads that own nothing, odd steps (lam == 0 in the middle of a frame), the product's T = 8960 and the
T = 71680 row whose phase passes 10^4 rad. Three rows with a different F0 pattern each per call; tests/test_loss_layer_cpu.py
asserts what the patterns are.

Bar, per element: |got - ref| <= 4 * 2^-24 * A, A = 0.1 + 0.003 |n_v| (voiced) or |(0.1 / 3) n_u| (unvoiced). It is derived, not
measured: the kernel forms the phase and its sine in float64 and then does at most three fp32 roundings of terms no larger than A
(voiced), or rounds 0.1f / 3.0f and one product (unvoiced); 4 is the project's usual factor. The draw of the other branch is NaN
on every sample and the dropped last frame is NaN in every row, so a finite output also shows that the voiced / unvoiced decision
agrees with the reference sample by sample and that frame n is never read.

Measured on an MI355X, worst error / bar per shape over both row sets and both start phases (voiced / unvoiced elements):
    (2, 1) 0.021 / 0.396     (2, 64) 0.360 / 0.458    (5, 64) 0.408 / 0.460     (6, 64) 0.432 / 0.464
    (86, 3) 0.429 / 0.457    (87, 3) 0.457 / 0.462    (141, 64) 0.463 / 0.467   (1121, 64) 0.467 / 0.467
    linear=False: (6, 64) 0.442 / 0.464, (87, 3) 0.457 / 0.462;  C ABI with the unaligned output: 0.367 / 0.462.
No case exceeds the bar. Tried and not kept: with exc_omega's `w0 > 0.0 && w1 > 0.0` turned into `||` every linear case from 4 kept
frames on fails (a sample the reference calls unvoiced takes the voiced branch and its NaN draw: the output is non-finite)."""
import numpy as np
import pytest
import torch

import excitation_ref as XR
from common import pkg
from edge_support import EINVAL, SENT, stream

pytestmark = pytest.mark.gpu
BAR = 4 * 2.0 ** -24
PHASES = [0.0, 6.28]


def _dev(c, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(c['f0']), (t(c['noise_v']), t(c['noise_u']))


def _run(c, phi0, dev, linear=True):
    f0, noise = _dev(c, dev)
    exc = pkg().util.f0_to_excitation(f0, c['step'], 16000, linear, noise=noise, start_phase=torch.tensor([phi0], device=dev))
    torch.cuda.synchronize()
    return exc


def _check(exc, c, phi0, linear, what):
    """Element-wise bar against the float64 reference; prints worst error / bar."""
    ref, unv, A = XR.excitation(c['f0'], c['noise_v'], c['noise_u'], float(np.float32(phi0)), c['step'], linear=linear)
    got = exc.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape == (len(c['patterns']), 1, c['T'])
    assert np.isfinite(got).all(), f'{what}: non-finite output -- a draw of the other branch or the dropped frame was read'
    ratio = np.abs(got - ref) / (BAR * A)
    live = A > 0
    worst = float(ratio[live].max()) if live.any() else 0.0
    print(f'[excitation] {what}: worst err/bar {worst:.3f} (voiced {float(ratio[live & ~unv].max()) if (live & ~unv).any() else 0.0:.3f}, '
          f'unvoiced {float(ratio[live & unv].max()) if (live & unv).any() else 0.0:.3f})')
    assert worst <= 1.0, (what, worst)
    assert (got[~live] == 0).all()
    for b, p in enumerate(c['patterns']):
        if p == 'unvoiced':            # the row is (0.1 / 3) n_u and nothing else
            want = (0.1 / 3.0) * c['noise_u'][b].astype(np.float64)
            assert (np.abs(got[b] - want) <= BAR * np.abs(want)).all()
    return worst


@pytest.mark.parametrize('shape', XR.SHAPES, ids=XR.SHAPE_IDS)
@pytest.mark.parametrize('patterns', [XR.PATTERNS_A, XR.PATTERNS_B], ids=['rows_A', 'rows_B'])
@pytest.mark.parametrize('phi0', PHASES, ids=['phase0', 'phase6.28'])
def test_excitation_vs_float64(shape, patterns, phi0, dev):
    c = XR.make_case(*shape, patterns)
    exc = _run(c, phi0, dev)
    _check(exc, c, phi0, True, f'{shape} {patterns} phi0={phi0}')
    assert torch.equal(exc, _run(c, phi0, dev)), 'two calls differ'


@pytest.mark.parametrize('shape', [(6, 64), (87, 3)], ids=['T320', 'T258_odd_step'])
@pytest.mark.parametrize('patterns', [XR.PATTERNS_A, XR.PATTERNS_B], ids=['rows_A', 'rows_B'])
def test_excitation_nearest_vs_float64(shape, patterns, dev):
    """linear=False: omega stays the nearest-upsampled frame value."""
    c = XR.make_case(*shape, patterns)
    _check(_run(c, 6.28, dev, linear=False), c, 6.28, False, f'nearest {shape} {patterns}')


@pytest.mark.parametrize('shape', [(6, 64), (87, 3), (141, 64)], ids=['T320', 'T258_odd_step', 'T8960'])
def test_excitation_row_alone_equals_row_in_batch(shape, dev):
    """One block per row and nothing shared between rows: every row computed alone has the bits it has inside the batch."""
    c = XR.make_case(*shape, XR.PATTERNS_B)
    full = _run(c, 6.28, dev)
    for b in range(len(c['patterns'])):
        one = dict(c, f0=c['f0'][b:b + 1], noise_v=c['noise_v'][b:b + 1], noise_u=c['noise_u'][b:b + 1], patterns=c['patterns'][b:b + 1])
        assert torch.equal(_run(one, 6.28, dev)[0], full[b]), (shape, b)


def test_excitation_c_abi_unaligned_output_guards(dev):
    """Through the C ABI with the output one float into a SENT-filled flat buffer (nothing 16-byte aligned, T = 258 odd rows): the
    values meet the bar and the floats in front of and behind the output stay untouched."""
    L = pkg()._lib
    c = XR.make_case(87, 3, XR.PATTERNS_B)
    B, T = len(c['patterns']), c['T']
    f0, (nv, nu) = _dev(c, dev)
    phi = torch.tensor([6.28], device=dev)
    buf = torch.full((1 + B * T + 3,), SENT, dtype=torch.float32, device=dev)
    out = buf[1:1 + B * T]
    L.check(L.lib().tdvc_f0_to_excitation(f0.data_ptr(), nv.data_ptr(), nu.data_ptr(), phi.data_ptr(), out.data_ptr(), B, 87, 3, 16000.0, 1,
                                          stream(dev)))
    torch.cuda.synchronize()
    _check(out.view(B, 1, T), c, 6.28, True, 'C ABI, unaligned output')
    h = buf.cpu()
    assert bool(h[0] == SENT) and bool((h[1 + B * T:] == SENT).all()), 'write outside the output'
    assert torch.equal(out.view(B, 1, T), _run(c, 6.28, dev))
    rc = L.lib().tdvc_f0_to_excitation(f0.data_ptr(), nv.data_ptr(), nu.data_ptr(), phi.data_ptr(), out.data_ptr(), B, 1, 3, 16000.0, 1, stream(dev))
    assert rc == EINVAL                    # n_frames = 1 leaves no frame once the last one is dropped: refused, no launch
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), h)


def test_excitation_refusals(dev):
    """n_frames = 1 and a 2-D f0 raise ValueError before any launch."""
    U = pkg().util
    with pytest.raises(ValueError, match='f0_to_excitation'):
        U.f0_to_excitation(torch.full((2, 1, 1), 120.0, device=dev), 64)
    with pytest.raises(ValueError, match='f0_to_excitation'):
        U.f0_to_excitation(torch.full((2, 9), 120.0, device=dev), 64)
