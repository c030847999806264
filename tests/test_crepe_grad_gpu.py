"""GPU: the backward of the CREPE tracker with respect to its signal (csrc/pitch_crepe_bwd.hip, tdvc_crepe_conv_train in pitch_crepe.hip,
crepe.py, losses.f0_crepe_loss, TrainStep(f0_loss='activation')) against the float64 restatement tests/crepe_grad_ref.py, which
tests/test_crepe_grad_cpu.py pins to torch.autograd. torchcrepe is not available: nothing here is a parity test against it.

1. Codes (tdvc_crepe_conv_train): every geometry of test_crepe_gpu.CONV_CASES, N = 1, 2, 17, 33. y has the bits of tdvc_crepe_conv. A
   pooled output is undecided when a float64 margin (|v_even - v_odd|, |z_winner|) is below tau = 4 x the largest difference between
   stock torch's fp32 CPU evaluation and float64 of v and z respectively; pairs with both z <= 0 are code 0 either way and never
   undecided. The device code equals the float64 code on every decided output; at most 0.5 % of a layer's outputs are undecided
   (asserted on the CPU side before the device is consulted).
2. Block backward (tdvc_crepe_conv_bwd) as the linear map it is: the float64 codes and a seeded dy go in, every element of dx is
   compared, bar 4 x the error of the fp32 CPU evaluation of the same formulae. NaN-filled spare frames stay NaN (dx) and are never
   read (dy); LDS poisoned first; the scale has negative entries; all codes 0 gives exact zeros; one nonzero dy per frame reproduces
   one weight row times fl(dy scale) exactly.
3. Head backward: C6 = 64 and 512, (N, F) = (1, 1), (17, 1), (17, 17), a strided target view with NaN spares, gL changed on the
   device between two calls; the plain form (d act given) as well.
4. Frames backward: hop 64 and 160, T = 63, 64, 1023, 1024, 1025, 2240, rows: tones, a constant row, an all-zero row, in a strided view
   with NaN spares; bar 4 * 2^-24 * max|row gradient| * covering frames.
5. End to end: f0_crepe_loss on 3 rows of 2240 samples with `tiny` and state_dict(7): value against float64; signal.grad element by
   element against `backward` under the device's own codes, bar 4 x the fp32 CPU evaluation's error; those codes agree with float64's
   on every decided output, under the cap; a row alone, a second call and a graph replay give the same bits; activations_with_grad
   gives the bits of activations and the same gradient; `full` on one row of 1024 samples.
6. roll_bins and conversion_target against the literal restatements of util.roll_batches and train.py:245-252.
7. TrainStep(f0_loss='activation'): the four tests of test_pitch_grad_gpu.py:189-286 mirrored, and device_batch(f0_tracker=).
8. Refusals before any launch.
Every test prints error / bar (run with -s).
Measured on an MI355X (error / bar): codes: no decided output off float64 on any geometry or N, undecided 0 .. 3.2e-5 of a layer's
outputs; tdvc_crepe_conv_bwd 0.22 (128 -> 1), 0.08 (16 -> 128), 0.08-0.17 (layers 3-5), 0.39 (64 -> 32 on 8), 0.21 (128 -> 128), 0.63
(1024 -> 1); tdvc_crepe_head_bwd 0.02-0.03; tdvc_crepe_frames_bwd at most 0.03 on all 36 rows; f0_crepe_loss tiny 3 x 2240: value 4.0e-11 from float64 (tolerance 1.6e-8), signal.grad
0.13 (max|g - g64| 2.7e-13 of 6.4e-7), the device's codes differ from float64's on 1 undecided output of layer 1 (undecided 1.3e-3
there, at most 7.2e-5 in layers 2-6); full on one row 0.24; step: |g(lambda) - g0 - lambda gf| / |g(lambda)| = 2.0e-7, eager and
replayed G_loss 2.303254700e+02 and g_loss_f0 7.365512429e-04, bit-equal."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import crepe_grad_ref as GR
import crepe_ref as R
import test_crepe_gpu as TG
from common import build_models, pkg, to_dev
from edge_support import EINVAL, EUNSUPPORTED, poison_lds

pytestmark = pytest.mark.gpu
NAN = float('nan')
U24 = 2.0 ** -24
GRAD_N = (1, 2, 17, 33)
CAP = 0.005


def K():
    return pkg().crepe


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------------------------------ 1. codes
@functools.lru_cache(maxsize=None)
def code_case(name):
    """The float64 and fp32 decisions of conv_case(name)'s 33 frames, the undecided outputs, and a seeded dy with the block backward in
    both precisions."""
    c = TG.conv_case(name)
    layer = c['layer']
    d64 = GR.layer_codes(c['sd'], layer, c['x'])
    d32 = GR.layer_codes(c['sd'], layer, c['x'], torch.float32)
    tau_v, tau_z = GR.taus(d64, d32)
    und = GR.undecided(d64, tau_v, tau_z)
    g = torch.Generator().manual_seed(sorted(TG.CONV_CASES).index(name) + 70)
    dy = torch.randn(d64['code'].shape, generator=g)
    b64 = GR.block_backward(c['sd'], layer, dy, d64['code'], torch.float64, scale=c['scale'])
    b32 = GR.block_backward(c['sd'], layer, dy, d64['code'], torch.float32, scale=c['scale'])
    return dict(code=d64['code'], und=und, share=float(und.double().mean()), tau=(tau_v, tau_z), dy=dy, b64=b64,
                bar=4 * float((b32.double() - b64).abs().max()), differ32=int((d64['code'] != d32['code'])[~und].sum()))


def conv_train_call(dev, c, name, N, y, code):
    layer, Cin, Cout, Lin = TG.CONV_CASES[name]
    L = pkg()._lib
    p = f'conv{layer}'
    a = L.CrepeConvArgs()
    a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = N, Cin, Cout, Lin, R.KERNELS[layer - 1], R.STRIDES[layer - 1]
    keep = [c['x'][:N].to(dev).contiguous(), c['sd'][p + '.weight'].to(dev).contiguous(), c['sd'][p + '.bias'].to(dev), c['scale'].to(dev), c['shift'].to(dev)]
    a.x, a.w, a.bias, a.scale, a.shift, a.y = [t.data_ptr() for t in keep] + [y.data_ptr()]
    rc = L.lib().tdvc_crepe_conv_train(C.byref(a), None if code is None else code.data_ptr(), stream(dev))
    torch.cuda.synchronize()
    return rc, keep


@pytest.mark.parametrize('name', sorted(TG.CONV_CASES))
def test_codes_against_float64(dev, name):
    c, cc = TG.conv_case(name), code_case(name)
    layer, Cin, Cout, Lin = TG.CONV_CASES[name]
    print(f'crepe_conv_train {name}: tau_v {cc["tau"][0]:.2e} tau_z {cc["tau"][1]:.2e}, undecided {cc["share"]:.2e} of {cc["und"].numel()}, '
          f'fp32 CPU codes differ from float64 on {cc["differ32"]} decided outputs')
    assert cc['share'] <= CAP and set(cc['code'].unique().tolist()) == {0, 1, 2}
    Nmax, Lout = max(GRAD_N), cc['code'].shape[2]
    wrong = 0
    for N in GRAD_N:
        y = torch.full((Nmax, Cout, Lout), NAN, device=dev)
        code = torch.full((Nmax, Cout, Lout), 77, dtype=torch.uint8, device=dev)
        poison_lds(dev)
        rc, keep = conv_train_call(dev, c, name, N, y, code)
        assert rc == 0, pkg()._lib.lib().tdvc_last_error()
        plain = torch.full((Nmax, Cout, Lout), NAN, device=dev)
        assert TG.conv_call(dev, keep[0], keep[1], keep[2], keep[3], keep[4], plain, N, Cin, Cout, Lin, R.KERNELS[layer - 1], R.STRIDES[layer - 1]) == 0
        assert torch.equal(y[:N], plain[:N]) and bool(torch.isnan(y[N:]).all()), f'N={N}: y differs from tdvc_crepe_conv'
        got = code.cpu()
        assert bool((got[N:] == 77).all()), f'N={N}: codes past N were written'
        bad = (got[:N] != cc['code'][:N]) & ~cc['und'][:N]
        wrong += int(bad.sum())
    assert wrong == 0, f'{wrong} decided outputs carry another code than float64'


# --------------------------------------------------------------------------------------------------------- 2. block backward
def conv_bwd_call(dev, name, N, dy, code, scale, wt, dx):
    layer, Cin, Cout, Lin = TG.CONV_CASES[name]
    L = pkg()._lib
    a = L.CrepeConvBwdArgs()
    a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = N, Cin, Cout, Lin, R.KERNELS[layer - 1], R.STRIDES[layer - 1]
    ptr = lambda t: None if t is None else t.data_ptr()
    a.dy, a.code, a.scale, a.wt, a.dx = ptr(dy), ptr(code), ptr(scale), ptr(wt), ptr(dx)
    rc = L.lib().tdvc_crepe_conv_bwd(C.byref(a), stream(dev))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('name', sorted(TG.CONV_CASES))
def test_block_backward_against_float64(dev, name):
    c, cc = TG.conv_case(name), code_case(name)
    layer, Cin, Cout, Lin = TG.CONV_CASES[name]
    assert bool((c['scale'] < 0).any()) and cc['bar'] > 0
    wt = K().pack_bwd_weight(c['sd'][f'conv{layer}.weight'].to(dev))
    scale = c['scale'].to(dev)
    Nmax = max(GRAD_N)
    worst = 0.0
    for N in GRAD_N:
        dy = torch.full(cc['dy'].shape, NAN, device=dev)
        dy[:N] = cc['dy'][:N].to(dev)
        code = cc['code'].to(dev)
        dx = torch.full((Nmax, Cin, Lin), NAN, device=dev)
        poison_lds(dev)
        assert conv_bwd_call(dev, name, N, dy, code, scale, wt, dx) == 0, pkg()._lib.lib().tdvc_last_error()
        got = dx.double().cpu()
        assert torch.isnan(got[N:]).all(), f'N={N}: frames past N were written'
        assert torch.isfinite(got[:N]).all(), f'N={N}'
        worst = max(worst, float((got[:N] - cc['b64'][:N]).abs().max()))
    print(f'crepe_conv_bwd {name} {Cout}->{Cin} on {Lin}: max|dx - dx64| {worst:.3e}, bar {cc["bar"]:.3e}, error / bar {worst / cc["bar"]:.3f}')
    assert worst <= cc['bar']
    # all codes 0: exact zeros, whatever dy holds
    N = 17
    dx = torch.full((N, Cin, Lin), NAN, device=dev)
    assert conv_bwd_call(dev, name, N, cc['dy'][:N].to(dev), torch.zeros(cc['code'][:N].shape, dtype=torch.uint8, device=dev), scale, wt, dx) == 0
    assert bool((dx == 0).all())
    # one nonzero dy per frame (NaN everywhere else, never selected): one weight row times fl(dy scale), exactly
    g = torch.Generator().manual_seed(layer)
    Lout = cc['code'].shape[2]
    dy1, code1 = torch.full((N, Cout, Lout), NAN), torch.zeros(N, Cout, Lout, dtype=torch.uint8)
    dyz = torch.zeros(N, Cout, Lout)
    for n in range(N):
        co, m = int(torch.randint(0, Cout, (1,), generator=g)), int(torch.randint(0, Lout, (1,), generator=g))
        if n == 0:
            co, m = 1, 0                                                        # a negative scale at the left edge
        if n == 1:
            co, m = Cout - 1, Lout - 1                                          # the odd position at the right edge
        dy1[n, co, m] = dyz[n, co, m] = float(torch.randn(1, generator=g))
        code1[n, co, m] = 2 if n % 2 else 1
    ref = GR.block_backward(c['sd'], layer, dyz, code1, torch.float32, scale=c['scale'])
    dx = torch.full((N, Cin, Lin), NAN, device=dev)
    assert conv_bwd_call(dev, name, N, dy1.to(dev), code1.to(dev), scale, wt, dx) == 0
    assert float(ref.abs().max()) > 0 and torch.equal(dx.cpu(), ref), 'one dy element must reproduce one weight row exactly'


# ---------------------------------------------------------------------------------------------------------- 3. head backward
@pytest.mark.parametrize('C6,N,F', [(64, 1, 1), (64, 17, 1), (64, 17, 17), (512, 1, 1), (512, 17, 1), (512, 17, 17)])
def test_head_backward_against_float64(dev, C6, N, F):
    g = torch.Generator().manual_seed(C6 + N + F)
    sd = {'classifier.weight': (2 * torch.rand(360, 4 * C6, generator=g) - 1) * math.sqrt(3.0 / (4 * C6))}
    act = 0.05 + 0.9 * torch.rand(N, 360, generator=g)                           # frame-major [N, 360]
    target = torch.rand(N, 360, generator=g)
    B = N // F
    lay = lambda t: t.reshape(B, F, 360).permute(0, 2, 1).contiguous()          # -> [B, 360, F]
    whole = torch.full((B, 362, F + 3), NAN, device=dev)
    whole[:, 1:361, :F] = lay(target).to(dev)
    tview = whole[:, 1:361, :F]
    assert not tview.is_contiguous()
    gl = torch.tensor([1.75], device=dev)
    ref = GR.head_backward(sd, act, target, 1.75)
    ref32 = GR.head_backward(sd, act, target, 1.75, torch.float32)
    bar = 4 * float((ref32.double() - ref).abs().max())
    poison_lds(dev)
    W = sd['classifier.weight'].to(dev)
    got = K().crepe_head_bwd(lay(act).to(dev), W, C6, 4, target=tview, gL=gl)
    assert got.shape == (N, C6, 4) and got.dtype == torch.float32
    err = float((got.double().cpu() - ref).abs().max())
    print(f'crepe_head_bwd C6={C6} N={N} F={F}: max|dx - dx64| {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}')
    assert bar > 0 and err <= bar
    gl.fill_(-3.5)                                                              # the same pointer, another value: gL is read on the device
    again = K().crepe_head_bwd(lay(act).to(dev), W, C6, 4, target=tview, gL=gl)
    assert float((again.double().cpu() - (-2.0) * ref).abs().max()) <= 2 * bar
    dact = torch.randn(N, 360, generator=g)
    plain = K().crepe_head_bwd(lay(act).to(dev), W, C6, 4, dact=lay(dact).to(dev))
    pref = GR.head_backward(sd, act, None, None, dact=dact)
    pbar = 4 * float((GR.head_backward(sd, act, None, None, torch.float32, dact=dact).double() - pref).abs().max())
    assert float((plain.double().cpu() - pref).abs().max()) <= pbar


# -------------------------------------------------------------------------------------------------------- 4. frames backward
FRAME_T = (63, 64, 1023, 1024, 1025, 2240)


@pytest.mark.parametrize('hop', [64, 160])
def test_frames_backward_against_float64(dev, hop):
    cover = -(-1024 // hop)
    for T in FRAME_T:
        rows = np.stack([R.tones(T, seed=T % 97), np.full(T, 0.3, np.float32), np.zeros(T, np.float32)])
        Fn = 1 + T // hop
        g = torch.randn(3, Fn, 1024, generator=torch.Generator().manual_seed(T + hop))
        whole = torch.full((6, T + 5), NAN, device=dev)
        whole[::2, :T] = torch.from_numpy(rows).to(dev)
        view = whole[::2, :T]
        poison_lds(dev)
        got = K().crepe_frames_bwd(view, g.to(dev), hop)
        assert got.shape == (3, T) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        for b, what in enumerate(('tones', 'constant', 'zero')):
            ref = GR.frames_backward(rows[b], g[b], hop)
            bar = 4 * U24 * float(ref.abs().max()) * cover
            err = float((got[b].double().cpu() - ref).abs().max())
            print(f'crepe_frames_bwd hop {hop} T={T} {what}: max|d - d64| {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}')
            assert bar > 0 and err <= bar, (T, what, err, bar)
        assert torch.equal(K().crepe_frames_bwd(view[0], g[:1].to(dev), hop), got[0])      # a row alone


# ------------------------------------------------------------------------------------------------------------- 5. end to end
def rows_grad(sd, code_list, act, target, xs, hop, dtype):
    """d mean((act - target)^2) / d signal for rows xs (equal lengths) under the given decisions; act, target [N, 360] frame-major."""
    gfr = GR.backward(sd, code_list, act, target, 1.0, dtype)
    Fn = gfr.shape[0] // len(xs)
    return torch.stack([GR.frames_backward(x, gfr[b * Fn:(b + 1) * Fn], hop, dtype) for b, x in enumerate(xs)])


def e2e_reference(capacity, seed, xs):
    sd = R.state_dict(seed, capacity)
    fr = torch.cat([R.frames(x, 64) for x in xs])
    l64, a64 = GR.codes(sd, fr)
    l32, a32 = GR.codes(sd, fr.float(), torch.float32)
    und = [GR.undecided(d64, *GR.taus(d64, d32)) for d64, d32 in zip(l64, l32)]
    for i, u in enumerate(und, 1):
        assert float(u.double().mean()) <= CAP, (i, float(u.double().mean()))
    target = torch.roll(a64, 5, 1).float() * 0.9 + 0.03                         # the kind of target the term has: the activations, rolled
    # the value: an error d in the activations moves mean((a - t)^2) by at most mean(2 |a - t|) max|d| to first order; max|d| <= 4 x the
    # fp32 CPU chain's error is the bar the forward test holds the activations to; 4 * 2^-24 for the fp32 result
    loss64 = float(((a64 - target.double()) ** 2).mean())
    tol_v = float((2 * (a64 - target.double()).abs()).mean()) * 4 * float((a32.double() - a64).abs().max()) + 4 * U24 * loss64
    return dict(sd=sd, l64=l64, a64=a64, a32=a32, und=und, target=target, loss64=loss64, tol_v=tol_v)


@functools.lru_cache(maxsize=None)
def e2e_case():
    xs = [R.tones(2240, seed=50 + b) for b in range(3)]
    return xs, e2e_reference('tiny', 7, xs)


@functools.lru_cache(maxsize=None)
def tiny7():
    return K().load_crepe(e2e_case()[1]['sd'], 'tiny', device='cuda')


def check_e2e(dev, m, xs, ref, what):
    P = pkg()
    B, T = len(xs), len(xs[0])
    Fn = 1 + T // 64
    lay = lambda t: t.reshape(B, Fn, 360).permute(0, 2, 1).contiguous()
    tgt = lay(ref['target']).to(dev)
    x = torch.from_numpy(np.stack(xs)).to(dev)[:, None].requires_grad_()
    poison_lds(dev)
    loss = P.losses.f0_crepe_loss(x, tgt, m)
    assert loss.shape == (1,) and loss.grad_fn is not None
    loss.backward()
    torch.cuda.synchronize()
    tol_v = ref['tol_v']
    print(f'f0_crepe_loss {what}: value {float(loss.detach()):.9e} vs {ref["loss64"]:.9e}, |diff| {abs(float(loss.detach()) - ref["loss64"]):.3e}, tol {tol_v:.3e}')
    assert abs(float(loss.detach()) - ref['loss64']) <= tol_v
    act, codes = m._forward_train(x.detach()[:, 0], 64)                          # the decisions the device took, read back
    assert torch.equal(act, m.activations(x.detach()))
    dev_codes = [c_.cpu() for c_ in codes]
    for i, (dc, d64, und) in enumerate(zip(dev_codes, ref['l64'], ref['und']), 1):
        off = dc != d64['code']
        print(f'  layer {i}: undecided {float(und.double().mean()):.2e}, device codes differ from float64 on {int(off.sum())} outputs, {int((off & ~und).sum())} of them decided')
        assert not bool((off & ~und).any()), i
    g64 = rows_grad(ref['sd'], dev_codes, ref['a64'], ref['target'], xs, 64, torch.float64)
    g32 = rows_grad(ref['sd'], dev_codes, ref['a32'], ref['target'], xs, 64, torch.float32)
    bar = 4 * float((g32.double() - g64).abs().max())
    got = x.grad[:, 0]
    assert got.shape == (B, T) and bool(torch.isfinite(got).all())
    err = float((got.double().cpu() - g64).abs().max())
    print(f'  signal.grad: max|g - g64| {err:.3e}, largest element {float(g64.abs().max()):.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}')
    assert bar > 0 and err <= bar
    return x, tgt, loss.detach().clone(), got.clone(), g64, bar


def test_f0_crepe_loss_end_to_end(dev):
    P = pkg()
    xs, ref = e2e_case()
    m = tiny7()
    x, tgt, loss, grad, g64, bar = check_e2e(dev, m, xs, ref, 'tiny, 3 rows of 2240')

    def run(xin, t):
        xin = xin.detach().clone().requires_grad_()
        l_ = P.losses.f0_crepe_loss(xin, t, m)
        l_.backward()
        return l_.detach(), xin.grad
    l2, g2 = run(x, tgt)                                                        # a second call
    assert torch.equal(l2, loss) and torch.equal(g2[:, 0], grad)
    # a row alone: the loss divides by the batch's element count, so the rows are compared through activations_with_grad and one d act
    a = m.activations_with_grad(x.detach().clone().requires_grad_())
    assert a.grad_fn is not None and torch.equal(a.detach(), m.activations(x.detach()))
    xa = x.detach().clone().requires_grad_()
    aa = m.activations_with_grad(xa)
    dact = (2.0 / aa.numel()) * (aa.detach() - tgt)
    aa.backward(dact)
    assert float((xa.grad[:, 0].double().cpu() - g64).abs().max()) <= bar       # the plain form of the head backward: the same bar
    x1 = x.detach()[1:2].clone().requires_grad_()
    a1 = m.activations_with_grad(x1)
    assert torch.equal(a1.detach(), aa.detach()[1:2])
    a1.backward(dact[1:2])
    assert torch.equal(x1.grad, xa.grad[1:2]), 'a row alone differs from the row in the batch'
    # graph replay
    torch.cuda.synchronize()
    xs_ = x.detach().clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs_.grad = None
            P.losses.f0_crepe_loss(xs_, tgt, m).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    xs_.grad = None
    with torch.cuda.graph(graph):
        lc = P.losses.f0_crepe_loss(xs_, tgt, m)
        lc.backward()
    gc = xs_.grad
    lc.detach().zero_(); gc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lc.detach(), loss) and torch.equal(gc[:, 0], grad)


def test_full_capacity_gradient_on_one_row(dev):
    xs = [R.tones(1024, seed=31)]
    ref = e2e_reference('full', 12, xs)
    m = K().load_crepe(ref['sd'], 'full', device=dev)
    check_e2e(dev, m, xs, ref, 'full, 1 row of 1024')


# -------------------------------------------------------------------------------------------------------- 6. roll and target
def test_roll_bins_and_conversion_target(dev):
    g = torch.Generator().manual_seed(3)
    act = torch.rand(4, 360, 7, generator=g)
    shifts = torch.tensor([0, 7, -7, 365])
    whole = torch.full((4, 362, 9), NAN, device=dev)
    whole[:, 1:361, :7] = act.to(dev)
    got = K().roll_bins(whole[:, 1:361, :7], shifts.to(dev))
    assert torch.equal(got.cpu(), GR.roll_batches(act, shifts, 1))
    assert torch.equal(K().roll_bins(act.to(dev), shifts.view(4, 1, 1).to(dev)).cpu(), got.cpu())
    f0 = torch.zeros(4, 1, 7)
    f0[0, 0, :5] = torch.tensor([100.0, 0.0, 110.0, 120.0, 0.0])
    f0[2, 0, :5] = torch.tensor([220.0, 230.0, 0.0, 210.0, 200.0])
    f0[3, 0] = 150.0                                                            # row 1 has no voiced frame
    perm = torch.tensor([2, 0, 3, 1])
    f0c, actc = K().conversion_target(f0.to(dev), act.to(dev), perm.to(dev))
    rf0, ract = GR.conversion_target(f0, act, perm, K().get_shift)
    # the track is exp(log f0 + mu_tgt - mu_src) in fp32 stock ops on both sides, with different log / exp routines: the exponent is the
    # result of four fp32 operations on values up to max|log f0|, each within 2 ulp on either side, and exp turns its absolute error
    # into a relative one: 16 * 2^-24 * max|log f0| * f0
    tol = 16 * U24 * float(torch.log(f0[f0 > 0]).abs().max()) * float(rf0.max())
    assert torch.equal(actc.cpu(), ract) and float((f0c.cpu() - rf0).abs().max()) <= tol
    assert bool((f0c[1] == 0).all()) and not torch.equal(ract[1], act[1])
    f2, a2 = K().conversion_target(f0[:, 0].to(dev), act.to(dev), perm.to(dev))  # [B, F] tracks
    assert torch.equal(a2, actc) and torch.equal(f2, f0c[:, 0])


# -------------------------------------------------------------------------------------------------------------- 7. the step
B_, T_ = 2, 8960


@functools.lru_cache(maxsize=None)
def step_inputs():
    P = pkg()
    dev = torch.device('cuda')
    bt = to_dev(P.synth.make_batch(B_, T_, seed=5), dev)
    m = tiny7()
    tgt = K().roll_bins(m.activations(bt['signal_real']), torch.tensor([3, -4], device=dev))
    assert tgt.shape == (B_, 360, T_ // 64 + 1)
    ix = P.synth.contrastive_indices(B_, T_ // 320, 100, 1).to(dev)
    iy = P.synth.contrastive_indices(B_, T_ // 320, 100, 2).to(dev)
    return bt, tgt, ix, iy


def g_pass(dev, bt, ix, iy, **cfg_kw):
    P = pkg()
    G, D = build_models(dev)
    ts = P.train_step.TrainStep(G, D, P.train_step.StepConfig(**cfg_kw), dev, f0_model=tiny7())
    log = {}
    ts._g_fwd_bwd(bt, log, ix, iy)
    torch.cuda.synchronize()
    return ts, log, G.arena.G[:G.arena.n_live].clone()


def test_step_logs_the_activation_term(dev):
    """(a)"""
    P = pkg()
    bt, tgt, ix, iy = step_inputs()
    ts, log, _ = g_pass(dev, {**bt, 'f0_conv_activ': tgt}, ix, iy, lambda_f0=1000.0, f0_loss='activation')
    assert 'g_loss_f0' in log and log['g_loss_f0'].grad_fn is None
    fake = ts._generate(bt)[0][0]
    again = P.losses.f0_crepe_loss(fake, tgt, tiny7())
    print(f'\nstep: g_loss_f0 {float(log["g_loss_f0"]):.6e}')
    assert torch.equal(log['g_loss_f0'], again.detach()) and float(again.detach()) > 0
    with pytest.raises(ValueError, match='f0_conv_activ'):
        ts._g_fwd_bwd(bt, {}, ix, iy)
    with pytest.raises(ValueError, match='f0_model'):
        P.train_step.TrainStep(ts.G, ts.D, P.train_step.StepConfig(f0_loss='activation'), dev)


def test_step_default_path_ignores_the_target_activations(dev):
    """(b)"""
    bt, tgt, ix, iy = step_inputs()
    _, log_a, g_a = g_pass(dev, bt, ix, iy, lambda_f0=1000.0)
    _, log_b, g_b = g_pass(dev, {**bt, 'f0_conv_activ': tgt}, ix, iy, lambda_f0=1000.0)
    assert 'g_loss_f0' not in log_a and 'g_loss_f0' not in log_b
    assert torch.equal(log_a['G_loss'], log_b['G_loss'])
    assert torch.equal(g_a, g_b) and float(g_a.abs().max()) > 0


def test_step_gradient_is_the_sum_of_both_parts(dev):
    """(c)"""
    P = pkg()
    bt, tgt, ix, iy = step_inputs()
    btf = {**bt, 'f0_conv_activ': tgt}
    ts, _, g0 = g_pass(dev, btf, ix, iy)
    ts.opt_g.zero_grad()
    fake = ts._generate(btf)[0][0]
    P.losses.f0_crepe_loss(fake, tgt, tiny7()).backward()
    torch.cuda.synchronize()
    gf = ts.G.arena.G[:ts.G.arena.n_live].clone()
    n0, nf = float(g0.double().norm()), float(gf.double().norm())
    assert nf > 0 and n0 > 0
    lam = n0 / nf
    _, log, gl = g_pass(dev, btf, ix, iy, lambda_f0=lam, f0_loss='activation')
    res = float((gl.double() - g0.double() - lam * gf.double()).norm())
    print(f'\nstep: |g0| {n0:.4e}, |gf| {nf:.4e}, lambda {lam:.4e}, |g(lambda) - g0 - lambda gf| / |g(lambda)| = {res / float(gl.double().norm()):.3e}')
    assert res <= 1e-3 * float(gl.double().norm())


def test_step_with_the_activation_term_under_graph_capture(dev):
    """(d)"""
    P = pkg()
    bt, tgt, ix, iy = step_inputs()
    btf = {**bt, 'f0_conv_activ': tgt}
    cfg = dict(lambda_f0=1000.0, f0_loss='activation')
    G, D = build_models(dev)
    ts = P.train_step.TrainStep(G, D, P.train_step.StepConfig(**cfg), dev, f0_model=tiny7())
    for _ in range(2):
        ts.run(btf, ix, iy)
    eager = {k: v.clone() for k, v in ts.run(btf, ix, iy).items()}
    torch.cuda.synchronize()
    G2, D2 = build_models(dev)
    ts2 = P.train_step.TrainStep(G2, D2, P.train_step.StepConfig(**cfg), dev, f0_model=tiny7())
    replay = ts2.capture(btf, ix, iy, warmup=2)
    log = replay()
    torch.cuda.synchronize()
    print(f'\nstep: eager G_loss {float(eager["G_loss"]):.9e} g_loss_f0 {float(eager["g_loss_f0"]):.9e}; '
          f'replay G_loss {float(log["G_loss"]):.9e} g_loss_f0 {float(log["g_loss_f0"]):.9e}')
    assert set(log) == set(eager) and float(log['g_loss_f0']) > 0
    for k in eager:
        assert torch.equal(log[k], eager[k]), k


def test_device_batch_with_the_tracker_feeds_a_step(dev):
    P = pkg()
    bt, _, ix, iy = step_inputs()
    m = tiny7()
    sig, lab = bt['signal_real'], bt['label_src']
    perm = torch.tensor([1, 0], device=dev)
    db = P.device_batch(sig, lab, 16, perm=perm, f0_tracker=m, generator=torch.Generator(device=dev).manual_seed(1))
    f0_src, act_src = m.filtered_pitch(sig)
    f0c, actc = K().conversion_target(f0_src, act_src, perm)
    assert db['f0_conv_activ'].shape == (B_, 360, T_ // 64 + 1) and torch.equal(db['f0_conv_activ'], actc) and torch.equal(db['f0_conv'], f0c)
    same = P.device_batch(sig, lab, 16, conversion=False, f0_tracker=m, generator=torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(same['f0_conv_activ'], act_src) and torch.equal(same['f0_conv'], f0_src)
    assert 'f0_conv_activ' not in P.device_batch(sig, lab, 16, perm=perm, generator=torch.Generator(device=dev).manual_seed(1))
    G, D = build_models(dev)
    ts = P.train_step.TrainStep(G, D, P.train_step.StepConfig(lambda_f0=1000.0, f0_loss='activation'), dev, f0_model=m)
    log = ts.run(db, ix, iy)
    torch.cuda.synchronize()
    assert float(log['g_loss_f0']) >= 0 and all(bool(torch.isfinite(v).all()) for v in log.values())


# -------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_before_any_launch(dev):
    P = pkg()
    L = P._lib
    lib = L.lib()
    m = tiny7()
    x = torch.zeros(2, 1, 2048, device=dev)
    tgt = torch.zeros(2, 360, 33, device=dev)
    for fn in (lambda: P.losses.f0_crepe_loss(x[:, 0], tgt, m), lambda: P.losses.f0_crepe_loss(x, tgt[:, :, :32], m), lambda: P.losses.f0_crepe_loss(x, tgt, None),
               lambda: P.losses.f0_crepe_loss(x, tgt, m, sample_rate=22050), lambda: m.activations_with_grad(x, lengths=torch.ones(2, device=dev)),
               lambda: m.activations_with_grad(x, hop=0), lambda: K().roll_bins(tgt, torch.zeros(3, dtype=torch.int64, device=dev)),
               lambda: K().roll_bins(tgt, torch.zeros(2, device=dev)), lambda: K().crepe_frames_bwd(x, torch.zeros(2, 32, 1024, device=dev)),
               lambda: K().crepe_head_bwd(tgt, m.classifier.weight, 64, 4), lambda: K().pack_bwd_weight(torch.zeros(16, 16, 32, device=dev)),
               lambda: K().crepe_conv_bwd(torch.zeros(1, 24, 32, device=dev), torch.zeros(1, 24, 32, dtype=torch.uint8, device=dev), torch.zeros(24, device=dev),
                                          torch.zeros(16 * 24 * 64, device=dev), 16, 64)):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: P.losses.f0_crepe_loss(x.cpu(), tgt, m), lambda: P.losses.f0_crepe_loss(x, tgt.cpu(), m), lambda: K().roll_bins(tgt.cpu(), [0, 0])):
        with pytest.raises(RuntimeError):
            fn()
    # the C ABI: the output stays untouched
    dx = torch.full((4, 16, 128), -7.0, device=dev)
    dy, code = torch.zeros(4, 32, 64, device=dev), torch.zeros(4, 32, 64, dtype=torch.uint8, device=dev)
    v, wt = torch.zeros(32, device=dev), torch.zeros(16 * 32 * 64, device=dev)
    cases = [(dict(Cin=24), EUNSUPPORTED), (dict(Cout=24), EUNSUPPORTED), (dict(Lin=100), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED), (dict(stride=2), EUNSUPPORTED),
             (dict(Cin=16, K=512, stride=4, Lin=1024), EUNSUPPORTED), (dict(N=-1), EINVAL), (dict(null='wt'), EINVAL), (dict(null='code'), EINVAL),
             (dict(null='dx'), EINVAL)]
    for kw, want in cases:
        g = dict(N=4, Cin=16, Cout=32, Lin=128, K=64, stride=1)
        g.update({k: val for k, val in kw.items() if k != 'null'})
        ops = dict(dy=dy, code=code, scale=v, wt=wt, dx=dx)
        if 'null' in kw:
            ops[kw['null']] = None
        a = L.CrepeConvBwdArgs()
        a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = g['N'], g['Cin'], g['Cout'], g['Lin'], g['K'], g['stride']
        a.dy, a.code, a.scale, a.wt, a.dx = [None if ops[k] is None else ops[k].data_ptr() for k in ('dy', 'code', 'scale', 'wt', 'dx')]
        assert lib.tdvc_crepe_conv_bwd(C.byref(a), stream(dev)) == want and lib.tdvc_last_error(), kw
    st = stream(dev)
    out = torch.full((2, 2048), -7.0, device=dev)
    gfr = torch.zeros(2, 33, 1024, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    fb = lambda T, hop, F, nb: lib.tdvc_crepe_frames_bwd(x.data_ptr(), 2048, T, 2, hop, F, gfr.data_ptr(), out.data_ptr(), 2048, ws.data_ptr(), nb, st)
    assert fb(2048, 0, 33, 4096) == EUNSUPPORTED and fb(0, 64, 1, 4096) == EUNSUPPORTED and fb(2048, 64, 32, 4096) == EINVAL and fb(2048, 64, 33, 8) == -2
    assert lib.tdvc_crepe_head_bwd(tgt.data_ptr(), tgt.data_ptr(), 360 * 33, 33, 1, None, None, tgt.data_ptr(), 66, 64, 4, 360, 33, dx.data_ptr(), st) == EINVAL
    assert lib.tdvc_crepe_head_bwd(tgt.data_ptr(), tgt.data_ptr(), 360 * 33, 33, 1, v.data_ptr(), None, tgt.data_ptr(), 66, 24, 4, 360, 33, dx.data_ptr(), st) == EUNSUPPORTED
    assert lib.tdvc_crepe_act_mse(tgt.data_ptr(), tgt.data_ptr(), 360 * 33, 33, 1, 2, 360, 33, out.data_ptr(), ws.data_ptr(), 8, st) == -2
    torch.cuda.synchronize()
    assert bool((dx == -7.0).all()) and bool((out == -7.0).all())
