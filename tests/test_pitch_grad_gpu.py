"""GPU: the backward of the soft YIN track (tdvc_yin_soft_bwd, csrc/pitch_yin_bwd.hip) through pitch.yin_f0(soft=True) autograd,
losses.f0_yin_loss and the opt-in lambda_f0 term of TrainStep, against the float64 helper tests/yin_grad_ref.py, which
tests/golden/yin_grad.npz pins to the gradient of the reference's own soft YIN (tests/test_pitch_grad_cpu.py).

The tolerance comes from the fixture, not from the kernel: tol_g = 4 * min(E_ref32, E_plain32), the row-normalised error of an fp32
autograd evaluation of the same formulas against float64, 4x for a different summation order. Every element of a row must be
within tol_g * max |truth row|; rows whose truth is zero must be exactly zero. No frame is excused: the fixture guarantees that
every frame's on/off decision is out of an fp32 kernel's reach.

Measured on an MI355X (printed by the tests, run with -s):
    case      row-normalised max err   tol_g
    speech    5.496e-07                4.716e-06
    default   7.225e-07                7.391e-06
    odd       2.014e-06                1.084e-05
    min       2.847e-07                5.857e-06
    short     0 (exact zeros)          0
    silence   0 (exact zeros)          0
    faint     7.404e-07                6.271e-06
    long      8.312e-07                5.176e-06
    f0_yin_loss on speech: value |diff| 7.7e-10 (tol 4.3e-07), gradient 6.228e-07 (tol 4.716e-06)
    step: |g(lambda) - g0 - lambda gf| / |g(lambda)| = 7.2e-07 (bound 1e-3); eager and replayed G_loss 2.683939209e+02 and
    g_loss_f0 3.602325544e-02, bit-equal
"""
import functools

import numpy as np
import pytest
import torch

import yin_grad_ref as GR
import yin_ref as YR
from common import build_models, pkg, to_dev

pytestmark = pytest.mark.gpu
SR, THR = 16000, 0.1


def kw(s):
    return dict(sample_rate=SR, pitch_min=s['pitch_min'], pitch_max=s['pitch_max'], frame_stride=s['stride'] / SR, threshold=THR)


def device_grad_of(x, gy, s, **extra):
    """(dx, f0) of yin_f0(x.requires_grad_(), soft=True).backward(gy) for a device tensor x of any accepted layout."""
    x = x.detach().requires_grad_()
    f0 = pkg().pitch.yin_f0(x, soft=True, **kw(s), **extra)
    assert f0.grad_fn is not None and f0.requires_grad
    f0.backward(gy)
    assert x.grad is not None and x.grad.shape == x.shape
    return x.grad, f0.detach()


@functools.lru_cache(maxsize=None)
def device_grad(name):
    """Computed once per session and left unchanged."""
    t = GR.truth(name)
    dx, f0 = device_grad_of(t['x'].cuda(), t['gy'].float().cuda(), t['settings'])
    torch.cuda.synchronize()
    return dx.cpu(), f0.cpu()


def check_rows(what, dx, truth, tol):
    """Element by element within tol * max |truth row|; zero rows exactly zero; everything finite."""
    assert dx.shape == truth.shape and dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    scale = truth.abs().amax(-1, keepdim=True)
    err = GR.row_error(dx, truth)
    print(f'\nyin grad {what}: row-normalised max err {err:.3e} (tol {tol:.3e}), zero rows {int((scale == 0).sum())} of {scale.numel()}')
    zero = (scale == 0).expand_as(truth)
    assert not bool(dx[zero].any()), what
    assert bool(((dx.double() - truth).abs() <= tol * scale).all()), (what, err, tol)
    return err


def check_case(name):
    t = GR.truth(name)
    dx, f0 = device_grad(name)
    plain = pkg().pitch.yin_f0(t['x'].cuda(), soft=True, **kw(t['settings']))
    assert plain.grad_fn is None and torch.equal(plain.cpu(), f0)      # the autograd path returns the plain call's bits
    assert torch.equal(f0 > 0, t['f0'] > 0)                            # same on/off decision as the float64 truth, every frame
    check_rows(name, dx, t['dx'], t['meta']['tol_g'])


@pytest.mark.parametrize('name', tuple(GR.CASES))
def test_soft_yin_grad_vs_float64_helper(dev, name):
    check_case(name)
    if name in ('short', 'silence'):
        assert not bool(device_grad(name)[0].any())


def test_soft_yin_grad_inference_length(dev):
    """B = 1, T = 71680, speech settings: 1120 frames in one call."""
    check_case('long')


def test_soft_yin_grad_layouts_repeat_runs_and_full_write(dev):
    """[B, T], [B, 1, T], [T] and a slice of a wider NaN-filled buffer (x_bs != T) give identical gradient bits; so do two runs; dx
    handed to the C entry point as NaN-filled memory comes back fully written."""
    P = pkg()
    t = GR.truth('odd')
    s = t['settings']
    x, gy = t['x'].to(dev), t['gy'].float().to(dev)
    B, T = x.shape
    dx, f0 = device_grad_of(x, gy, s)
    assert torch.equal(dx.cpu(), device_grad('odd')[0]) and torch.equal(f0.cpu(), device_grad('odd')[1])
    dx_b, _ = device_grad_of(x, gy, s)
    assert torch.equal(dx, dx_b)
    dx3, f03 = device_grad_of(x[:, None, :], gy[:, None, :], s)
    assert dx3.shape == (B, 1, T) and torch.equal(dx3[:, 0], dx) and torch.equal(f03[:, 0], f0)
    dx1, f01 = device_grad_of(x[1], gy[1], s)
    assert dx1.shape == (T,) and torch.equal(dx1, dx[1]) and torch.equal(f01, f0[1])
    wide = torch.full((B, T + 37), float('nan'), device=dev)
    wide[:, 5:5 + T] = x
    sl = wide[:, 5:5 + T]
    assert sl.stride(0) == T + 37 and not sl.is_contiguous()
    dxs, f0s = device_grad_of(sl, gy, s)
    assert torch.equal(dxs, dx) and torch.equal(f0s, f0)
    dxt, _ = device_grad_of(x.t().contiguous().t(), gy, s)              # last axis not dense: copied, same result
    assert torch.equal(dxt, dx)
    # the CMDF is returned next to a differentiable track, and is itself not differentiable
    xr = x.detach().requires_grad_()
    f0c, c = P.pitch.yin_f0(xr, soft=True, return_cmdf=True, **kw(s))
    assert f0c.grad_fn is not None and c.grad_fn is None and not c.requires_grad and torch.equal(f0c.detach(), f0)
    # the C entry point on NaN-filled dx
    lib, L = P._lib.lib(), P._lib
    nb = lib.tdvc_yin_soft_bwd_workspace(B, T, s['tau_max'], s['stride'])
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.full((B, T), float('nan'), device=dev)
    L.check(lib.tdvc_yin_soft_bwd(x.data_ptr(), T, B, T, s['tau_min'], s['tau_max'], s['stride'], THR, float(SR), gy.data_ptr(),
                                  out.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream(dev).cuda_stream))
    assert torch.equal(out, dx)


@pytest.mark.parametrize('name', ['odd', 'default'])
def test_soft_yin_grad_poisoned_lds(dev, name):
    """The LDS of every CU pre-filled with NaN bit patterns before a backward: same bits as the clean run. `odd` (L = 640) runs five
    m slices; `default` (tau_max = 800) is where the correlation's clamped window reads reach the end of the LDS image, beyond what
    the frame staging writes: what they fetch may only ever land in terms that a select discards."""
    L = pkg()._lib
    t = GR.truth(name)
    clean = device_grad(name)[0]
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
    dx, _ = device_grad_of(t['x'].to(dev), t['gy'].float().to(dev), t['settings'])
    assert bool(torch.isfinite(dx).all()) and torch.equal(dx.cpu(), clean)


def test_hard_track_has_no_grad_fn(dev):
    P = pkg()
    t = GR.truth('min')
    x = t['x'].to(dev).requires_grad_()
    assert P.pitch.yin_f0(x, soft=False, **kw(t['settings'])).grad_fn is None
    assert P.track_f0(x[:, None], soft=False).grad_fn is None and P.track_f0(x[:, None]).grad_fn is None
    assert P.track_f0(x[:, None], soft=True).grad_fn is not None
    with torch.no_grad():
        assert P.pitch.yin_f0(x, soft=True, **kw(t['settings'])).grad_fn is None


def test_f0_yin_loss_value_and_gradient(dev):
    """On `speech` with a target track from synth.make_f0, against the float64 helper composed with the loss formula.
    Gradient: the row rule above with the case's tol_g. Value: the loss is sum(v e^2) / n with e = (f - t) / scale, so an error df in
    f moves it by at most sum(v * 2 |e| |df| / scale) / n to first order; |df| <= max(4 * S_ref32, 1e-6) * f is the bound the
    forward test holds the soft track to (yin.json), and 1e-6 * loss covers the fp32 sum."""
    P = pkg()
    t = GR.truth('speech')
    s = t['settings']
    B, T = t['x'].shape
    scale, n_t = 400.0, T // 64
    tgt = torch.from_numpy(P.synth.make_f0(np.random.RandomState(21), B, T))
    assert tgt.shape == (B, 1, n_t + 1)
    # float64: loss of the helper's track, its derivative with respect to the track as upstream gradient of the helper
    f, tt = t['f0'][:, :n_t], tgt[:, 0, :-1].double()
    v = ((tt > 0) & (f > 0)).double()
    n = v.sum().clamp(min=1.0)
    assert float(v.sum()) >= 10
    loss64 = float((v * ((f - tt) / scale) ** 2).sum() / n)
    gy = torch.zeros_like(t['f0'])
    gy[:, :n_t] = v * 2 * (f - tt) / scale ** 2 / n
    dx64, _, _ = GR.grad(t['x'], gy, s['tau_min'], s['tau_max'], s['stride'], THR, SR)
    x = t['x'][:, None].to(dev).requires_grad_()
    loss = P.losses.f0_yin_loss(x, tgt.to(dev))
    assert loss.shape == (1,)
    loss.backward()
    torch.cuda.synchronize()
    soft_bound = max(4 * YR.truth('speech')['meta']['S_ref32'], 1e-6)
    tol_v = float((v * 2 * ((f - tt) / scale).abs() * soft_bound * f / scale).sum() / n) + 1e-6 * loss64
    print(f'\nf0_yin_loss speech: value {float(loss.detach()):.9e} vs {loss64:.9e} (|diff| {abs(float(loss.detach()) - loss64):.3e}, tol {tol_v:.3e}), frames in the mean {int(v.sum())}')
    assert abs(float(loss.detach()) - loss64) <= tol_v
    check_rows('f0_yin_loss speech', x.grad[:, 0].cpu(), dx64, t['meta']['tol_g'])


# ---- the lambda_f0 term in TrainStep: B = 2, T = 8960, deterministic weights
B_, T_ = 2, 8960


def _step_inputs(dev):
    P = pkg()
    bt = to_dev(P.synth.make_batch(B_, T_, seed=5), dev)
    f0_conv = torch.from_numpy(P.synth.make_f0(np.random.RandomState(5), B_, T_)).to(dev)
    ix = P.synth.contrastive_indices(B_, T_ // 320, 100, 1).to(dev)
    iy = P.synth.contrastive_indices(B_, T_ // 320, 100, 2).to(dev)
    return bt, f0_conv, ix, iy


def _g_pass(dev, bt, ix, iy, **cfg_kw):
    """A fresh seeded step, one G forward/backward: (step, log, flat G gradient)."""
    P = pkg()
    G, D = build_models(dev)
    ts = P.train_step.TrainStep(G, D, P.train_step.StepConfig(**cfg_kw), dev)
    log = {}
    ts._g_fwd_bwd(bt, log, ix, iy)
    torch.cuda.synchronize()
    return ts, log, G.arena.G[:G.arena.n_live].clone()


def test_step_logs_the_f0_term(dev):
    """(a) log['g_loss_f0'] equals f0_yin_loss recomputed on step._generate(batch)'s fake, bit for bit; the term is live."""
    P = pkg()
    bt, f0_conv, ix, iy = _step_inputs(dev)
    ts, log, _ = _g_pass(dev, {**bt, 'f0_conv': f0_conv}, ix, iy, lambda_f0=1000.0, f0_loss='yin')
    assert 'g_loss_f0' in log and log['g_loss_f0'].grad_fn is None
    fake = ts._generate(bt)[0][0]
    again = P.losses.f0_yin_loss(fake, f0_conv)
    f = P.pitch.yin_f0(fake[:, 0].detach(), SR, 60, 500, 64 / SR, soft=True)
    print(f'\nstep: g_loss_f0 {float(log["g_loss_f0"]):.6e}, frames on {float((f > 0).float().mean()):.3f}')
    assert torch.equal(log["g_loss_f0"], again.detach()) and float(again.detach()) > 0
    with pytest.raises(ValueError, match='f0_conv'):
        ts._g_fwd_bwd(bt, {}, ix, iy)


def test_step_default_path_ignores_f0_conv(dev):
    """(b) with f0_loss=None, G_loss and the flat G gradient have the same bits whether or not f0_conv is in the batch. (The logged
    loss values are bit-reproducible from run to run: their block partials are accumulated in fixed point, csrc/misc_kernels.hip
    loss_accumulate.)"""
    bt, f0_conv, ix, iy = _step_inputs(dev)
    _, log_a, g_a = _g_pass(dev, bt, ix, iy, lambda_f0=1000.0)
    _, log_b, g_b = _g_pass(dev, {**bt, 'f0_conv': f0_conv}, ix, iy, lambda_f0=1000.0)
    assert 'g_loss_f0' not in log_a and 'g_loss_f0' not in log_b
    print(f'\nstep: default path G_loss {float(log_a["G_loss"]):.9e} without, {float(log_b["G_loss"]):.9e} with f0_conv')
    assert torch.equal(log_a['G_loss'], log_b['G_loss'])
    assert torch.equal(g_a, g_b) and float(g_a.abs().max()) > 0


def test_step_gradient_is_the_sum_of_both_parts(dev):
    """(c) g(lam) = g0 + lam * gf with lam = |g0| / |gf| chosen so that both parts weigh the same: within 1e-3 |g(lam)|, the
    project's parity figure."""
    P = pkg()
    bt, f0_conv, ix, iy = _step_inputs(dev)
    btf = {**bt, 'f0_conv': f0_conv}
    ts, _, g0 = _g_pass(dev, btf, ix, iy)
    ts.opt_g.zero_grad()
    fake = ts._generate(btf)[0][0]
    P.losses.f0_yin_loss(fake, f0_conv).backward()
    torch.cuda.synchronize()
    gf = ts.G.arena.G[:ts.G.arena.n_live].clone()
    n0, nf = float(g0.double().norm()), float(gf.double().norm())
    assert nf > 0 and n0 > 0
    lam = n0 / nf
    _, log, gl = _g_pass(dev, btf, ix, iy, lambda_f0=lam, f0_loss='yin')
    res = float((gl.double() - g0.double() - lam * gf.double()).norm())
    print(f'\nstep: |g0| {n0:.4e}, |gf| {nf:.4e}, lambda {lam:.4e}, |g(lambda) - g0 - lambda gf| / |g(lambda)| = {res / float(gl.double().norm()):.3e}')
    assert res <= 1e-3 * float(gl.double().norm())


def test_step_with_the_f0_term_under_graph_capture(dev):
    """(d) a captured iteration with the term replays to the same G_loss and g_loss_f0 bits as the eager iteration from the same
    state (2 warm-up iterations, then the recorded one)."""
    P = pkg()
    bt, f0_conv, ix, iy = _step_inputs(dev)
    btf = {**bt, 'f0_conv': f0_conv}
    cfg = dict(lambda_f0=1000.0, f0_loss='yin')
    G, D = build_models(dev)
    ts = P.train_step.TrainStep(G, D, P.train_step.StepConfig(**cfg), dev)
    for _ in range(2):
        ts.run(btf, ix, iy)
    eager = {k: v.clone() for k, v in ts.run(btf, ix, iy).items()}
    torch.cuda.synchronize()
    G2, D2 = build_models(dev)
    ts2 = P.train_step.TrainStep(G2, D2, P.train_step.StepConfig(**cfg), dev)
    replay = ts2.capture(btf, ix, iy, warmup=2)
    log = replay()
    torch.cuda.synchronize()
    print(f'\nstep: eager G_loss {float(eager["G_loss"]):.9e} g_loss_f0 {float(eager["g_loss_f0"]):.9e}; '
          f'replay G_loss {float(log["G_loss"]):.9e} g_loss_f0 {float(log["g_loss_f0"]):.9e}')
    assert set(log) == set(eager) and float(log['g_loss_f0']) > 0
    assert torch.equal(log['g_loss_f0'], eager['g_loss_f0'])
    assert torch.equal(log['G_loss'], eager['G_loss'])
    for k in eager:                                                     # every logged loss value, not only the two the term touches
        assert torch.equal(log[k], eager[k]), k
