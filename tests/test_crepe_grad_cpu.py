"""CPU: the float64 restatement tests/crepe_grad_ref.py of the CREPE backward (the reference's activation-MSE F0 term, train.py:439-470) that
the GPU tests of tests/test_crepe_grad_gpu.py measure against, and the host side of the term.

1. `backward` under its own codes equals torch.autograd through crepe_ref.network, to 1e-12 of the largest element.
2. `frames_backward` equals autograd through the framing, including a constant frame (den = 1e-10) and frames that straddle the padding.
3. The weight packing of tdvc_crepe_conv_bwd (crepe.pack_bwd_weight) reproduces `block_backward` when the sums of include/tdvc.h are
   written out with it, for both geometries.
4. The literal restatements of util.roll_batches and train.py:245-252 behave as the source does: negative shifts, a row with no voiced
   frame (mu = 0: a mean of 1 Hz). The device `roll_bins` / `conversion_target` are held to them in the GPU file: there is no CPU path.
5. The decisions of the seeded network: the share of undecided pooled outputs and fp32 / float64 agreement (printed, run with -s).
6. Symbols, signatures, the StepConfig switch, refusals of CPU tensors."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crepe_grad_ref as GR
import crepe_ref as R
from common import ROOT, pkg


def Cr():
    return pkg().crepe


def seeded_rows(n_rows=3, T=2240):
    return [R.tones(T, seed=50 + b) for b in range(n_rows)]


def test_manual_backward_equals_autograd():
    sd = R.state_dict(7, 'tiny')
    fr = R.frames(R.tones(640, 3), 64)[2:6].clone().requires_grad_()
    g = torch.Generator().manual_seed(1)
    target = torch.rand(fr.shape[0], 360, generator=g, dtype=torch.float64)
    gL = 1.7
    act = R.network(sd, fr)
    (gL * F.mse_loss(act, target)).backward()
    layers, act2 = GR.codes(sd, fr.detach())
    assert float((act2 - act.detach()).abs().max()) < 1e-13             # the folded BatchNorm rounds differently from F.batch_norm
    got = GR.backward(sd, [d['code'] for d in layers], act2, target, gL)
    scale = float(fr.grad.abs().max())
    err = float((got - fr.grad).abs().max())
    print(f'\nmanual backward vs autograd: max|diff| {err:.3e}, largest element {scale:.3e}')
    assert scale > 0 and err <= 1e-12 * scale
    for d in layers:                                                           # every code occurs, so every branch of the backward ran
        assert set(d['code'].unique().tolist()) == {0, 1, 2}


def autograd_frames(x, hop):
    """crepe_ref.frames on a tensor that requires grad; max(1e-10, std) with a zero subgradient on the clamped side (torch's own std
    backward is 0 / 0 at a constant frame)."""
    n = x.shape[0]
    xp = F.pad(x, (512, 512))
    fr = torch.stack([xp[f * hop:f * hop + 1024] for f in range(1 + n // hop)])
    c = fr - fr.mean(1, keepdim=True)
    var = (c * c).sum(1, keepdim=True) / 1023
    on = var > 1e-20
    den = torch.where(on, torch.sqrt(torch.where(on, var, torch.ones_like(var))), torch.full_like(var, 1e-10))
    return c / den


@pytest.mark.parametrize('hop', [64, 160])
def test_frames_backward_equals_autograd(hop):
    g0 = torch.Generator().manual_seed(hop)
    rows = {'tones': torch.from_numpy(R.tones(1500, 4)).double(), 'constant': torch.full((2047,), 0.3).double(),
            'short': torch.from_numpy(R.tones(63, 5)).double()}
    for name, x in rows.items():
        x = x.clone().requires_grad_()
        fr = autograd_frames(x, hop)
        assert torch.allclose(fr.detach(), R.frames(x.detach().numpy(), hop), rtol=0, atol=1e-9 * float(fr.detach().abs().max()) + 1e-300)
        g = torch.randn(fr.shape, generator=g0, dtype=torch.float64)
        (fr * g).sum().backward()
        got = GR.frames_backward(x.detach(), g, hop)
        scale = float(x.grad.abs().max())
        err = float((got - x.grad).abs().max())
        print(f'\nframes backward hop {hop} {name}: max|diff| {err:.3e}, largest element {scale:.3e}')
        assert scale > 0 and err <= 1e-12 * scale
    n = 2047                                                                    # the constant row has frames of both kinds
    inside = [f for f in range(1 + n // hop) if f * hop - 512 >= 0 and f * hop + 512 <= n]
    assert inside and len(inside) < 1 + n // hop


@pytest.mark.parametrize('layer,Cin,Cout', [(1, 1, 32), (3, 16, 32)])
def test_weight_packing_reproduces_the_block_backward(layer, Cin, Cout):
    g = torch.Generator().manual_seed(layer)
    K = R.KERNELS[layer - 1]
    Lin = GR.LIN[layer - 1]
    Lc = Lin // R.STRIDES[layer - 1]
    w = torch.randn(Cout, Cin, K, 1, generator=g).double()                     # fp32 values: the packing is made from fp32 weights
    sd = {f'conv{layer}.weight': w}
    dy = torch.randn(2, Cout, Lc // 2, generator=g, dtype=torch.float64)
    code = torch.randint(0, 3, dy.shape, generator=g).to(torch.uint8)
    scale = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = GR.block_backward(sd, layer, dy, code, scale=scale)
    dz = GR.unpool(dy, code, scale)
    wt = Cr().pack_bwd_weight(w.float()).double()
    assert torch.equal(wt.float(), Cr().pack_bwd_weight(w[..., 0].float()))
    if layer == 1:
        assert wt.shape == (16, Cout, 136)
        dzp = F.pad(dz, (64, 72))                                               # dz[4 m + i - 64], i < 136
        cols = dzp.unfold(2, 136, 4)[:, :, :64]                                 # [N, Cout, m, i]
        got = torch.einsum('rci,ncmi->nmr', wt, cols).reshape(2, 1, 1024)       # s = 16 m + r
    else:
        assert wt.shape == (Cin, Cout, 64)
        cols = F.pad(dz, (32, 32)).unfold(2, 64, 1)[:, :, :Lin]                 # dzp[s + k']
        got = torch.einsum('ick,ncsk->nis', wt, cols)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_roll_and_conversion_target_restatements():
    g = torch.Generator().manual_seed(3)
    act = torch.rand(4, 360, 5, generator=g)
    shifts = torch.tensor([0, 7, -7, 365])
    out = GR.roll_batches(act, shifts, 1)
    for b, s in enumerate(shifts.tolist()):
        assert torch.equal(out[b], torch.roll(act[b], s, 0))
    f0 = torch.tensor([[[100.0, 0.0, 110.0, 120.0, 0.0]], [[0.0, 0.0, 0.0, 0.0, 0.0]], [[220.0, 230.0, 0.0, 210.0, 200.0]], [[150.0] * 5]])
    perm = torch.tensor([2, 0, 3, 1])
    f0c, actc = GR.conversion_target(f0, act, perm, Cr().get_shift)
    assert f0c.shape == f0.shape and bool(((f0c > 0) == (f0 > 0)).all())
    assert bool((f0c[1] == 0).all())                                            # no voiced frame: nothing to shift
    mean_hz = lambda f: float(torch.exp(torch.log(f[f > 0]).mean()))
    s0 = int(Cr().get_shift(mean_hz(f0[0]), mean_hz(f0[2])))
    assert s0 > 0 and torch.equal(actc[0], torch.roll(act[0], s0, 0))
    # row 1 has no voiced frame: mu_src = 0, a mean of 1 Hz, so the shift is that of 1 Hz -> row 0's mean; row 3's target is row 1: the other sign
    s1 = int(Cr().hz_to_bins(mean_hz(f0[0])) - Cr().hz_to_bins(1.0))
    s3 = int(Cr().hz_to_bins(1.0) - Cr().hz_to_bins(150.0))
    assert s1 > 360 and s3 < -200
    assert torch.equal(actc[1], torch.roll(act[1], s1 % 360, 0)) and torch.equal(actc[3], torch.roll(act[3], s3, 0))


def test_seeded_network_leaves_few_outputs_undecided():
    """crepe_ref.state_dict(7) on three `tones` rows of 2240 samples (108 frames): the share of pooled outputs whose decision is within
    4 x the fp32 CPU error of changing is far below the 0.5 % cap of the GPU tests, and fp32 and float64 disagree on none."""
    sd = R.state_dict(7, 'tiny')
    fr = torch.cat([R.frames(x, 64) for x in seeded_rows()])
    assert fr.shape == (108, 1024)
    l64, _ = GR.codes(sd, fr)
    l32, _ = GR.codes(sd, fr.float(), torch.float32)
    for i, (d64, d32) in enumerate(zip(l64, l32), 1):
        und = GR.undecided(d64, *GR.taus(d64, d32))
        share = float(und.double().mean())
        differ = int((d64['code'] != d32['code']).sum())
        print(f'\nlayer {i}: undecided {share:.2e} of {und.numel()}, fp32 and float64 codes differ on {differ}')
        assert share <= 0.005 and not bool((d64['code'] != d32['code'])[~und].any())


def test_library_exports_the_backward_symbols_with_their_signatures():
    L = pkg()._lib
    lib = L.lib()
    i32, i64, vp, sz = C.c_int32, C.c_int64, C.c_void_p, C.c_size_t
    want = {
        'tdvc_crepe_conv_train': (C.c_int, [C.POINTER(L.CrepeConvArgs), vp, vp]),
        'tdvc_crepe_conv_bwd': (C.c_int, [C.POINTER(L.CrepeConvBwdArgs), vp]),
        'tdvc_crepe_head_bwd': (C.c_int, [vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        'tdvc_crepe_act_mse_workspace': (sz, []),
        'tdvc_crepe_act_mse': (C.c_int, [vp, vp, i64, i64, i64, i32, i32, i32, vp, vp, sz, vp]),
        'tdvc_crepe_frames_bwd_workspace': (sz, [i32, i32]),
        'tdvc_crepe_frames_bwd': (C.c_int, [vp, i64, i32, i32, i32, i32, vp, vp, i64, vp, sz, vp]),
        'tdvc_roll_bins': (C.c_int, [vp, i64, i64, vp, vp, i32, i32, i32, vp]),
    }
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert L.SIGNATURES[name] == (res, args) and f' {name}(' in header, name
    assert [f[0] for f in L.CrepeConvBwdArgs._fields_] == ['N', 'Cin', 'Cout', 'Lin', 'K', 'stride', 'reserved0', 'reserved1', 'dy', 'code', 'scale',
                                                           'wt', 'dx']
    assert C.sizeof(L.CrepeConvBwdArgs) == 8 * 4 + 5 * 8
    assert lib.tdvc_crepe_frames_bwd_workspace(3, 36) == 3 * 36 * 32 and lib.tdvc_crepe_act_mse_workspace() > 0
    mk = open(os.path.join(os.path.dirname(L.LIB_PATH), 'Makefile')).read()
    assert 'pitch_crepe_bwd.hip' in mk and os.path.exists(os.path.join(os.path.dirname(L.LIB_PATH), 'pitch_crepe_bwd.hip'))
    for name in ('roll_bins', 'conversion_target', 'activation_mse', 'crepe_conv_bwd', 'crepe_head_bwd', 'crepe_frames_bwd', 'pack_bwd_weight'):
        assert callable(getattr(pkg(), name))
    assert callable(pkg().losses.f0_crepe_loss) and callable(Cr().Crepe.activations_with_grad)


def test_the_c_abi_refuses_before_any_launch():
    """A null stream and host or null pointers: a call that got past its checks would launch, so only refused calls are made."""
    L = pkg()._lib
    lib = L.lib()
    a = L.CrepeConvBwdArgs()
    cases = [(dict(Cin=24), -4), (dict(Cout=24), -4), (dict(Lin=100), -4), (dict(K=32), -4), (dict(stride=2), -4),
             (dict(Cin=16, K=512, stride=4, Lin=1024), -4), (dict(N=-1), -1), (dict(), -1), (dict(N=1 << 20, Cin=1024, Cout=1024), -4)]
    for kw, want in cases:
        g = dict(N=4, Cin=16, Cout=32, Lin=128, K=64, stride=1)
        g.update(kw)
        a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = g['N'], g['Cin'], g['Cout'], g['Lin'], g['K'], g['stride']
        assert lib.tdvc_crepe_conv_bwd(C.byref(a), None) == want and lib.tdvc_last_error(), kw      # dict(): null pointers
    assert lib.tdvc_crepe_conv_bwd(None, None) == -1
    assert lib.tdvc_crepe_conv_train(None, None, None) == -1
    fa = L.CrepeConvArgs()
    fa.N, fa.Cin, fa.Cout, fa.Lin, fa.K, fa.stride = 4, 16, 24, 128, 64, 1
    assert lib.tdvc_crepe_conv_train(C.byref(fa), None, None) == -4
    assert lib.tdvc_crepe_head_bwd(None, None, 0, 0, 0, None, None, None, 10, 16, 4, 360, 3, None, None) == -1      # N not a multiple of F
    assert lib.tdvc_crepe_head_bwd(None, None, 0, 0, 0, None, None, None, 9, 24, 4, 360, 3, None, None) == -4
    assert lib.tdvc_crepe_head_bwd(None, None, 0, 0, 0, None, None, None, 9, 16, 4, 360, 3, None, None) == -1       # null pointers
    assert lib.tdvc_crepe_frames_bwd(None, 2048, 2048, 2, 0, 33, None, None, 2048, None, 0, None) == -4
    assert lib.tdvc_crepe_frames_bwd(None, 2048, 2048, 2, 64, 32, None, None, 2048, None, 0, None) == -1
    assert lib.tdvc_crepe_frames_bwd(None, 2048, 2048, 2, 64, 33, None, None, 2048, None, 0, None) == -1
    assert lib.tdvc_crepe_act_mse(None, None, 0, 0, 0, 2, 360, 5, None, None, 0, None) == -1
    assert lib.tdvc_roll_bins(None, 0, 0, None, None, 2, 360, 5, None) == -1 and lib.tdvc_roll_bins(None, 0, 0, None, None, 2, 0, 5, None) == -1


def test_step_config_switch():
    SC = pkg().train_step.StepConfig
    train = dict(lambda_f0=1000, lambda_idt=5)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        cfg = SC.from_hparams(train, f0_loss='activation')
    assert cfg.f0_loss == 'activation' and cfg.lambda_f0 == 1000.0
    with pytest.raises(ValueError):
        SC.from_hparams(train, f0_loss='crepe')
    with pytest.warns(UserWarning, match='lambda_f0'):
        assert SC.from_hparams(train).f0_loss is None
    with pytest.raises(ValueError, match='f0_model'):                           # at construction, before anything is built
        pkg().train_step.TrainStep(None, None, SC(f0_loss='activation', lambda_f0=1.0), 'cpu')
    with pytest.raises(ValueError):
        pkg().train_step.TrainStep(None, None, SC(f0_loss='crepe'), 'cpu')


def test_cpu_tensors_are_refused():
    P = pkg()
    E = P._lib.TdvcError
    m = Cr().load_crepe(R.state_dict(3, 'tiny'))
    x = torch.zeros(2, 1, 2048)
    with pytest.raises(E):
        P.losses.f0_crepe_loss(x, torch.zeros(2, 360, 33), m)
    with pytest.raises(E):
        m.activations_with_grad(x)
    with pytest.raises(E):
        Cr().roll_bins(torch.zeros(2, 360, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(E):
        Cr().conversion_target(torch.zeros(2, 1, 4) + 100.0, torch.zeros(2, 360, 4), torch.tensor([1, 0]))
    with pytest.raises(E):
        Cr().crepe_frames_bwd(x, torch.zeros(2, 33, 1024))
    with pytest.raises(E):
        Cr().crepe_conv_bwd(torch.zeros(1, 16, 32), torch.zeros(1, 16, 32, dtype=torch.uint8), torch.zeros(16), torch.zeros(16, 16, 64), 16, 64)
    with pytest.raises(ValueError):                                             # per-row lengths are not part of the differentiable path
        m.activations_with_grad(x, lengths=torch.tensor([2048, 1000]))
