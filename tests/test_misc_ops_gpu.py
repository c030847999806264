"""Op-level parity of the non-convolution kernels (misc_kernels.hip, the film_k3 kernels of film_cond_bwd.hip) through the C ABI,
against references written in float64 on the CPU from the math of each op: autograd for the gradients, torch.optim.AdamW for
the optimizer. Shapes are picked to reach the branches the launch code selects: grid-stride loops with more than one trip
(the grids are capped), n % 4 != 0, pointers offset by one float (the BatchView offsets of the loss terms), row lengths
around the 64-lane wave, and the exact thresholds of the refusals. Outputs are sentinel-filled first, so an element the
kernel misses or a write outside its range shows.

Bars: element-wise ops within 1e-6 of the magnitude of the terms they combine (bit-exact where the op is a copy), reductions
rel-L2 <= 2e-5, loss scalars rel <= 1e-5."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import rel_l2
from edge_support import EINVAL, SENT, stream

pytestmark = pytest.mark.gpu
EW = 1e-6          # element-wise: |got - ref| <= EW * (magnitude of the combined terms)
TOL = 2e-5         # reductions: rel-L2 per tensor
LOSS = 1e-5        # loss scalars: rel


def _pkg():
    return importlib.import_module('td-vc-gan_amd')


def _lib():
    return _pkg()._lib


def f32(x):
    """The value a float argument has once it crosses the C ABI."""
    return float(np.float32(x))


def _padded(src, dev, lead=1, tail=3):
    """(buffer, view): `src` copied into a SENT-filled device buffer at float offset `lead` (not 16-byte aligned for lead = 1)."""
    n = src.numel()
    buf = torch.full((lead + n + tail,), SENT, dtype=torch.float32, device=dev)
    view = buf[lead:lead + n]
    view.copy_(src.reshape(-1))
    return buf, view


def _guards_intact(buf, lead, n):
    b = buf.cpu()
    return bool((b[:lead] == SENT).all() and (b[lead + n:] == SENT).all())


def _ew(got, ref, bound, what):
    """Element-wise |got - ref| <= bound (all float64 on the CPU)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {ref.numel()} elements off; first at flat {i}: got {got.reshape(-1)[i].item()!r} '
                             f'ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item() if torch.is_tensor(bound) else bound!r}')


def _loss_ok(got, ref, what):
    assert abs(got - ref) <= LOSS * abs(ref), (what, got, ref)


def _rel_scaled(got, ref, scale):
    """rel-L2 with the denominator max(||ref||, scale): for gradients that cancel to ~0 (C = 1 cosines, unit columns)."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return float((got - ref).norm() / max(float(ref.norm()), scale, 1e-30))


# ================================================================================================ optimizer
LR, B1, B2, EPS = f32(1e-4), f32(0.8), f32(0.99), f32(1e-8)


def _adamw_run(dev, n, wd, gscale, device_step, steps, max_norm=None):
    """`steps` AdamW updates by the kernel; before each one, torch.optim.AdamW(foreach=False) in float64 takes the same step
    from the kernel's previous fp32 state (p, m, v) with the same fp32 gradient, and p, m, v are compared element-wise.
    Checking every step from the kernel's own state keeps the bound tight (a free-running float64 copy drifts by the
    accumulated fp32 rounding of 30 steps) and still runs the bias corrections of steps 1..30.
    max_norm: each step first computes the clip coefficient on the device (tdvc_grad_clip_coef) and updates with
    tdvc_adamw_clipped; the reference scales its gradient by the coefficient the kernel computed."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    wd = f32(wd)
    gen = torch.Generator().manual_seed(1000 + n % 997 + (7 if device_step else 0) + int(wd > 0) * 3 + int(gscale != 1.0) * 5)
    p0 = torch.randn(n, generator=gen)
    p0 = torch.sign(p0) * (p0.abs() + 0.05)                   # away from 0: p's own rounding is the bound's scale
    mag = 10.0 ** (-6.0 * torch.rand(n, generator=gen))       # per-element gradient scale 1e-6 .. 1: eps matters where it is small
    zero = torch.arange(3, max(n, 3), 97)                      # some gradients stay exactly 0 (not element 0: n = 1 has only it)
    pb, p = _padded(p0, dev)
    mb, m = _padded(torch.zeros(n), dev)
    vb, v = _padded(torch.zeros(n), dev)
    g_d = torch.empty(n, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.full((1024 + 8,), SENT, device=dev)
    out = torch.full((4,), SENT, device=dev)
    ref_p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([ref_p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for t in range(1, steps + 1):
        g = (torch.randn(n, generator=gen) * mag).float()
        g[zero] = 0.0
        if max_norm is not None:
            g = g * 50.0                                       # norm well above max_norm: the clip is active
        g_d.copy_(g)
        p_prev, m_prev, v_prev = p.double().cpu(), m.double().cpu(), v.double().cpu()
        sp = (0, step_dev.data_ptr()) if device_step else (t, None)
        if device_step:
            L.check(lib.tdvc_inc_i32(step_dev.data_ptr(), 1, st))
        if max_norm is None:
            L.check(lib.tdvc_adamw(p.data_ptr(), g_d.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, wd, sp[0], sp[1], gscale, st))
            coef = 1.0
        else:
            L.check(lib.tdvc_grad_clip_coef(g_d.data_ptr(), n, max_norm, gscale, ws.data_ptr(), out.data_ptr(), st))
            L.check(lib.tdvc_adamw_clipped(p.data_ptr(), g_d.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, wd, sp[0], sp[1],
                                           gscale, out.data_ptr(), st))
        torch.cuda.synchronize()
        if max_norm is not None:
            coef = float(out[0])
            total = gscale * float(g.double().norm())
            assert 0.0 < coef < 1.0 and abs(coef - f32(max_norm) / (total + 1e-6)) <= LOSS * coef, (t, coef, total)
        gs = g.double() * (gscale * coef)
        with torch.no_grad():
            ref_p.copy_(p_prev)
        ref_p.grad = gs.clone()
        if t > 1:
            s = opt.state[ref_p]
            s['exp_avg'].copy_(m_prev)
            s['exp_avg_sq'].copy_(v_prev)
        opt.step()
        s = opt.state[ref_p]
        pr = ref_p.detach()
        what = f'n={n} wd={wd} gscale={gscale} dev_step={device_step} step {t}'
        _ew(m, s['exp_avg'], EW * (B1 * m_prev.abs() + (1 - B1) * gs.abs()), 'm ' + what)
        _ew(v, s['exp_avg_sq'], EW * s['exp_avg_sq'], 'v ' + what)
        decayed = p_prev * (1 - LR * wd)
        # p = decayed - update: p's own rounding (1e-6 of |p|) plus 5e-6 of the update, which carries the fp32 bias corrections
        # (1 - beta2^t in fp32 at t = 2 is off by ~1.5e-6 relative)
        _ew(p, pr, EW * decayed.abs() + 5e-6 * (decayed - pr).abs(), 'p ' + what)
    for b, nm in ((pb, 'p'), (mb, 'm'), (vb, 'v')):
        assert _guards_intact(b, 1, n), f'{nm}: write outside [0, n)'


@pytest.mark.parametrize('n', [1, 255, 257, 256 * 4096 + 3])
@pytest.mark.parametrize('wd,gscale', [(0.0, 1.0), (0.0, 0.5), (1e-2, 1.0), (1e-2, 0.5)])
@pytest.mark.parametrize('device_step', [False, True], ids=['host_step', 'dev_step'])
def test_adamw_vs_float64(n, wd, gscale, device_step, dev):
    """tdvc_adamw over 30 steps (lr 1e-4, betas (0.8, 0.99), eps 1e-8): the host step, and the device step counter advanced
    by tdvc_inc_i32 (the form the captured graph replays). n = 256 * 4096 + 3 runs the capped grid's stride loop twice."""
    _adamw_run(dev, n, wd, gscale, device_step, 30)


@pytest.mark.parametrize('device_step', [False, True], ids=['host_step', 'dev_step'])
def test_adamw_clipped_vs_float64(device_step, dev):
    """tdvc_grad_clip_coef -> tdvc_adamw_clipped, the optimizer step with clipping as the train step runs it."""
    _adamw_run(dev, 300_001, 1e-2, 0.5, device_step, 6, max_norm=0.7)


@pytest.mark.parametrize('n', [100, 300_001], ids=['n100', 'n300001_capped_parts'])
@pytest.mark.parametrize('gscale', [1.0, 0.5])
@pytest.mark.parametrize('norm', [2e-3, 40.0])
@pytest.mark.parametrize('active', [True, False], ids=['clip', 'noclip'])
def test_grad_clip_coef(n, gscale, norm, active, dev):
    """out[0] = min(1, max_norm / (gscale ||g|| + 1e-6)), out[1] = gscale ||g||. n > 1024 * 256 caps the partial-sum count at
    1024; a norm of 2e-3 makes the 1e-6 visible at the loss bar."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    gen = torch.Generator().manual_seed(n + int(norm))
    g = torch.randn(n, generator=gen)
    g = (g * (norm / float(g.norm()))).float()
    total = gscale * float(g.double().norm())
    max_norm = f32(total * (0.5 if active else 2.0))
    gb, gd = _padded(g, dev)
    ws = torch.full((1024 + 8,), SENT, device=dev)
    out = torch.full((4,), SENT, device=dev)
    L.check(lib.tdvc_grad_clip_coef(gd.data_ptr(), n, max_norm, gscale, ws.data_ptr(), out.data_ptr(), st))
    torch.cuda.synchronize()
    o = out.cpu().double()
    coef_ref = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(o[1]) - total) <= TOL * total, (float(o[1]), total)
    if active:
        assert abs(float(o[0]) - coef_ref) <= LOSS * coef_ref, (float(o[0]), coef_ref)
    else:
        assert float(o[0]) == 1.0
    assert (o[2:] == SENT).all()
    nparts = min((n + 255) // 256, 1024)
    assert (ws.cpu()[nparts:] == SENT).all(), 'clip workspace written past its partial sums'


# ================================================================================================ weight norm
# (rows, cin, K, transposed): row lengths cin * K = 1, 3, 63, 64, 65, 2624, 2816, 2816; 27 rows in all (not a multiple of 4)
WN_TENSORS = [(3, 1, 1, True), (5, 1, 3, True), (2, 21, 3, True), (7, 64, 1, False), (1, 13, 5, True), (3, 164, 16, True),
              (2, 256, 11, False), (4, 256, 11, True)]


def _wn_setup(dev):
    """A flat parameter buffer holding v and g of every tensor at odd offsets, the effective-weight arena laid out as
    arena.py does (tensor w_off rounded up to 4 floats; transposed copy at tb = w_off + r K, ts = rows K), and its row tables."""
    gen = torch.Generator().manual_seed(11)
    off, woff, ts_ = 1, 0, []
    for rows, cin, K, tr in WN_TENSORS:
        cols = cin * K
        v = torch.randn(rows, cols, generator=gen)
        g = torch.randn(rows, generator=gen) * 1.5
        g[0] = -abs(float(g[0])) - 0.1 if len(ts_) % 2 == 0 else abs(float(g[0])) + 0.1    # g < 0 in half the tensors
        ts_.append(dict(rows=rows, cols=cols, K=K, tr=tr, v=v, g=g, voff=off, goff=off + rows * cols + 1, woff=woff))
        off += rows * cols + 1 + rows + 2
        woff += (rows * cols + 3) // 4 * 4
    params = torch.full((off + 3,), SENT)
    for t in ts_:
        params[t['voff']:t['voff'] + t['rows'] * t['cols']] = t['v'].reshape(-1)
        params[t['goff']:t['goff'] + t['rows']] = t['g']
    rv, rg, rw, rl, tb, tstr, tk = [], [], [], [], [], [], []
    for t in ts_:
        for r in range(t['rows']):
            rv.append(t['voff'] + r * t['cols']); rg.append(t['goff'] + r); rw.append(t['woff'] + r * t['cols']); rl.append(t['cols'])
            tb.append(t['woff'] + r * t['K']); tstr.append(t['rows'] * t['K']); tk.append(t['K'] if t['tr'] else 0)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    tables = dict(voff=i64(rv), goff=i64(rg), woff=i64(rw), len=torch.tensor(rl, dtype=torch.int32, device=dev),
                  tbase=i64(tb), tstride=i64(tstr), k=torch.tensor(tk, dtype=torch.int32, device=dev))
    return ts_, params.to(dev), tables, len(rl), woff


def _wn_ref(t):
    v = t['v'].double().requires_grad_(True)
    g = t['g'].double().requires_grad_(True)
    w = g[:, None] * v / v.norm(dim=1, keepdim=True)
    return v, g, w


def test_weight_norm_fwd_and_transposed_copy(dev):
    """tdvc_weight_norm_fwd / _fwd_t against float64 g v / ||v||; the transposed copy checked element by element against the
    arena's layout [cin][rows][K] at w_off, nothing else of either arena written."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    ts_, params, tb, nrows, n_w = _wn_setup(dev)
    assert nrows % 4 != 0
    W = torch.full((n_w,), SENT, device=dev)
    W2 = torch.full((n_w,), SENT, device=dev)
    WT = torch.full((n_w,), SENT, device=dev)
    L.check(lib.tdvc_weight_norm_fwd(params.data_ptr(), W.data_ptr(), tb['voff'].data_ptr(), tb['goff'].data_ptr(), tb['woff'].data_ptr(),
                                     tb['len'].data_ptr(), nrows, st))
    L.check(lib.tdvc_weight_norm_fwd_t(params.data_ptr(), W2.data_ptr(), WT.data_ptr(), tb['voff'].data_ptr(), tb['goff'].data_ptr(),
                                       tb['woff'].data_ptr(), tb['len'].data_ptr(), tb['tbase'].data_ptr(), tb['tstride'].data_ptr(),
                                       tb['k'].data_ptr(), nrows, st))
    torch.cuda.synchronize()
    W, W2, WT = W.cpu(), W2.cpu(), WT.cpu()
    assert torch.equal(W, W2), '_fwd_t wrote a different effective weight than _fwd'
    covered = torch.zeros(n_w, dtype=torch.bool)
    tcovered = torch.zeros(n_w, dtype=torch.bool)
    for t in ts_:
        rows, cols, K, wo = t['rows'], t['cols'], t['K'], t['woff']
        _, _, w = _wn_ref(t)
        got = W[wo:wo + rows * cols].reshape(rows, cols)
        # w's only reduction is the row norm (<= 2816 terms): its error is the same relative error for the whole row
        _ew(got, w.detach(), 1e-5 * w.detach().abs(), f'w rows={rows} cols={cols}')
        covered[wo:wo + rows * cols] = True
        if t['tr']:
            want = got.reshape(rows, cols // K, K).permute(1, 0, 2).reshape(-1)
            assert torch.equal(WT[wo:wo + rows * cols], want), f'transposed copy rows={rows} cols={cols} K={K}'
            tcovered[wo:wo + rows * cols] = True
    assert (W[~covered] == SENT).all(), 'effective-weight arena written outside the rows'
    assert (WT[~tcovered] == SENT).all(), 'transposed arena written outside the transposed tensors'


@pytest.mark.parametrize('accumulate', [0, 1])
def test_weight_norm_bwd(accumulate, dev):
    """tdvc_weight_norm_bwd against float64 autograd of g v / ||v|| with a random upstream dW: dv and dg written (0) or added
    (1) at the parameter offsets, every other parameter-gradient element untouched."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    ts_, params, tb, nrows, n_w = _wn_setup(dev)
    gen = torch.Generator().manual_seed(12)
    dW = torch.randn(n_w, generator=gen)
    pre = torch.randn(params.numel(), generator=gen) * 0.5 if accumulate else torch.full((params.numel(),), SENT)
    grads = pre.to(dev)
    dWd = dW.to(dev)
    L.check(lib.tdvc_weight_norm_bwd(params.data_ptr(), dWd.data_ptr(), grads.data_ptr(), tb['voff'].data_ptr(), tb['goff'].data_ptr(),
                                     tb['woff'].data_ptr(), tb['len'].data_ptr(), nrows, accumulate, st))
    torch.cuda.synchronize()
    got = grads.cpu()
    touched = torch.zeros(params.numel(), dtype=torch.bool)
    for t in ts_:
        rows, cols, wo, vo, go = t['rows'], t['cols'], t['woff'], t['voff'], t['goff']
        v, g, w = _wn_ref(t)
        (w * dW[wo:wo + rows * cols].double().reshape(rows, cols)).sum().backward()
        base_v = pre[vo:vo + rows * cols].double() if accumulate else 0.0
        base_g = pre[go:go + rows].double() if accumulate else 0.0
        # one-element rows (w = g sign(v)) have dv = 0 up to rounding: the size of the terms is the scale there
        dwr = dW[wo:wo + rows * cols].double().reshape(rows, cols)
        scale = float((g.detach() / v.detach().norm(dim=1))[:, None].mul(dwr).norm())
        ev = _rel_scaled(got[vo:vo + rows * cols], base_v + v.grad.reshape(-1), scale)
        eg = rel_l2(got[go:go + rows], base_g + g.grad)
        assert ev < TOL and eg < TOL, (rows, cols, ev, eg)
        touched[vo:vo + rows * cols] = True
        touched[go:go + rows] = True
    assert torch.equal(got[~touched], pre[~touched]), 'parameter gradient written outside the rows'


# ================================================================================================ loss kernels
LOSS_N = [1, 1023, 600_001]       # 600_001 > 2048 * 256: every capped grid (256 .. 2048 blocks) strides more than once


@pytest.mark.parametrize('n', LOSS_N)
@pytest.mark.parametrize('up', [None, 0.6])
def test_mse_const(n, up, dev):
    """loss += weight mean((x - target)^2); dx = 2 weight / n (x - target) upstream (upstream NULL = 1). x is a view one float
    into its buffer."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    target, weight = f32(0.75), f32(1.7)
    xb, xd = _padded(x, dev)
    out = torch.zeros(1, device=dev)
    for _ in range(2):               # the forward adds into loss_out
        L.check(lib.tdvc_mse_const_fwd(xd.data_ptr(), n, target, weight, out.data_ptr(), st))
    upd = torch.tensor([up], device=dev) if up is not None else None
    db, dx = _padded(torch.full((n,), SENT), dev)
    L.check(lib.tdvc_mse_const_bwd(xd.data_ptr(), n, target, weight, upd.data_ptr() if up is not None else None, dx.data_ptr(), st))
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    loss = weight * ((xr - target) ** 2).mean()
    (loss * (up if up is not None else 1.0)).backward()
    _loss_ok(float(out), 2 * loss.item(), 'mse_const_fwd')
    _ew(dx, xr.grad, EW * xr.grad.abs(), 'mse_const_bwd')
    assert _guards_intact(db, 1, n)


def _l1_inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=gen)
    b = torch.randn(n, generator=gen)
    b[::5] = a[::5]                  # a == b: sign(0) = 0
    return a, b


@pytest.mark.parametrize('n', LOSS_N)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_l1_single(n, accumulate, dev):
    """tdvc_l1_fwd / tdvc_l1_bwd: loss += weight mean|a - b|; da (+)= sign(a - b) weight / n upstream, sign(0) = 0."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    a, b = _l1_inputs(n, n + 1)
    weight, up = f32(0.35), 1.9
    ab, ad = _padded(a, dev)
    bd = b.to(dev)
    out = torch.zeros(1, device=dev)
    for _ in range(2):
        L.check(lib.tdvc_l1_fwd(ad.data_ptr(), bd.data_ptr(), n, weight, out.data_ptr(), st))
    pre = torch.randn(n) if accumulate else torch.full((n,), SENT)
    dab, da = _padded(pre, dev)
    upd = torch.tensor([up], device=dev)
    L.check(lib.tdvc_l1_bwd(ad.data_ptr(), bd.data_ptr(), n, weight, upd.data_ptr(), da.data_ptr(), accumulate, st))
    torch.cuda.synchronize()
    ar = a.double().requires_grad_(True)
    loss = weight * (ar - b.double()).abs().mean()
    (loss * up).backward()
    _loss_ok(float(out), 2 * loss.item(), 'l1_fwd')
    base = pre.double() if accumulate else 0.0
    _ew(da, base + ar.grad, EW * (abs(base) + ar.grad.abs()) if accumulate else EW * ar.grad.abs(), 'l1_bwd')
    assert (da.cpu()[::5] == (pre[::5] if accumulate else 0.0)).all(), 'sign(0) must be 0'
    assert _guards_intact(dab, 1, n)


@pytest.mark.parametrize('K', [1, 63, 64, 65, 300])
@pytest.mark.parametrize('B', [1, 3])
def test_cross_entropy(K, B, dev):
    """tdvc_cross_entropy_fwd / _bwd against float64 F.cross_entropy (mean over the batch) at logits of +-80, labels 0 and K-1."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    gen = torch.Generator().manual_seed(K * 10 + B)
    z = torch.randn(B, K, generator=gen) * 3
    if K >= 3:
        z[:, 1], z[:, 2] = 80.0, -80.0
    labels = torch.tensor([K - 1, 0, min(2, K - 1)][:B], dtype=torch.int64)     # sample 2's label on the -80 logit: loss ~ 160
    weight, up = f32(0.8), 1.3
    zd, ld = z.to(dev), labels.to(dev)
    out = torch.zeros(1, device=dev)
    prob = torch.full((B, K), SENT, device=dev)
    for _ in range(2):
        L.check(lib.tdvc_cross_entropy_fwd(zd.data_ptr(), ld.data_ptr(), B, K, weight, out.data_ptr(), prob.data_ptr(), st))
    dz = torch.full((B, K), SENT, device=dev)
    upd = torch.tensor([up], device=dev)
    L.check(lib.tdvc_cross_entropy_bwd(prob.data_ptr(), ld.data_ptr(), B, K, weight, upd.data_ptr(), dz.data_ptr(), st))
    torch.cuda.synchronize()
    zr = z.double().requires_grad_(True)
    loss = weight * F.cross_entropy(zr, labels)
    (loss * up).backward()
    _loss_ok(float(out), 2 * loss.item(), f'cross_entropy K={K} B={B}')
    assert rel_l2(prob, torch.softmax(z.double(), 1)) < TOL
    if K == 1:
        assert float(dz.abs().max()) == 0.0          # one class: probability 1, gradient 0
    else:
        assert rel_l2(dz, zr.grad) < TOL


def _contrastive_ref(X, Y, ix, iy, weight):
    """InfoNCE restated: for each direction (anchor side A, positive side P, its indices) and each (b, t), logits are the cosine
    of A[b,:,t] with P[b,:,t] and with the N detached negatives A[b,:,idx[b,t,n]] of the anchor's own side; the target is index
    0; the loss is weight times the mean over the 2 B T cross-entropies."""
    def side(A, P, idx):
        B, C_, T = A.shape
        idx = idx.long()
        an = A / A.norm(dim=1, keepdim=True)
        pn = P / P.norm(dim=1, keepdim=True)
        Ad = A.detach()
        An = Ad / Ad.norm(dim=1, keepdim=True)                               # [B, C, T]
        neg = torch.gather(An.unsqueeze(2).expand(B, C_, T, T), 3,
                           idx.unsqueeze(1).expand(B, C_, T, idx.shape[2]))  # [B, C, T, N]: neg[b,:,t,n] = An[b,:,idx[b,t,n]]
        pos = (an * pn).sum(1)                                               # [B, T]
        negs = (an.unsqueeze(3) * neg).sum(1)                                # [B, T, N]
        logits = torch.cat([pos.unsqueeze(2), negs], 2)
        return (torch.logsumexp(logits, 2) - logits[:, :, 0]).sum()
    B, _, T = X.shape
    return weight * (side(X, Y, ix) + side(Y, X, iy)) / (2 * B * T)


CONTRASTIVE = [(16, 128, 50, 100), (2, 32, 9, 20), (2, 1, 40, 30), (2, 129, 40, 30), (3, 16, 30, 1), (2, 64, 40, 127),
               (2, 64, 40, 129), (2, 128, 294, 100)]
CONTRASTIVE_IDS = ['step_shape', 'T9_tsplit', 'C1', 'C129', 'N1', 'N127', 'N129', 'lds_just_under_150k']


def _lds_floats(C_, T, N):
    return C_ * T + T + 2 * (N + 1) + 2 * C_ + 8


@pytest.mark.parametrize('shape', CONTRASTIVE, ids=CONTRASTIVE_IDS)
def test_contrastive_vs_float64(shape, dev):
    """tdvc_contrastive_fwd_bwd (loss and both input gradients in one launch) against float64 autograd of the InfoNCE above,
    with the negative indices the product feeds it (losses._skip_self of draws in [0, T-1))."""
    B, C_, T, N = shape
    if shape[2] == 294:
        assert _lds_floats(C_, T, N) * 4 <= 150 * 1024 < _lds_floats(C_, T + 1, N) * 4
    L = _lib()
    lib, st = L.lib(), stream(dev)
    LS = _pkg().losses
    gen = torch.Generator().manual_seed(B * 1000 + C_ * 10 + T + N)
    X = torch.randn(B, C_, T, generator=gen)
    Y = torch.randn(B, C_, T, generator=gen)
    ix = LS._skip_self(torch.randint(0, T - 1, (B, T, N), generator=gen))
    iy = LS._skip_self(torch.randint(0, T - 1, (B, T, N), generator=gen))
    assert int(ix.min()) >= 0 and int(ix.max()) < T and int(iy.min()) >= 0 and int(iy.max()) < T
    weight = f32(0.7)
    Xd, Yd, ixd, iyd = X.to(dev), Y.to(dev), ix.to(dev), iy.to(dev)
    out = torch.zeros(1, device=dev)
    dX, dY = torch.zeros_like(Xd), torch.zeros_like(Yd)
    L.check(lib.tdvc_contrastive_fwd_bwd(Xd.data_ptr(), Yd.data_ptr(), ixd.data_ptr(), iyd.data_ptr(), B, C_, T, N, weight, out.data_ptr(),
                                         dX.data_ptr(), dY.data_ptr(), st))
    torch.cuda.synchronize()
    Xr, Yr = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    loss = _contrastive_ref(Xr, Yr, ix, iy, weight)
    loss.backward()
    _loss_ok(float(out), loss.item(), f'contrastive {shape}')
    scale = weight / (2 * B * T) * math.sqrt(B * C_ * T) / math.sqrt(C_)      # natural size of the gradient (C = 1: it cancels to 0)
    ex, ey = _rel_scaled(dX, Xr.grad, scale), _rel_scaled(dY, Yr.grad, scale)
    assert ex < TOL and ey < TOL, (ex, ey)


def test_contrastive_refuses_lds_overflow(dev):
    """One time step more than the shape above: the embedding tile no longer fits in 150 KiB -> TDVC_EUNSUPPORTED, no launch."""
    L = _lib()
    B, C_, T, N = 2, 128, 295, 100
    assert _lds_floats(C_, T, N) * 4 > 150 * 1024
    X = torch.zeros(B, C_, T, device=dev)
    idx = torch.zeros(B, T, N, dtype=torch.int32, device=dev)
    out = torch.zeros(1, device=dev)
    rc = L.lib().tdvc_contrastive_fwd_bwd(X.data_ptr(), X.data_ptr(), idx.data_ptr(), idx.data_ptr(), B, C_, T, N, 1.0, out.data_ptr(),
                                          X.data_ptr(), X.data_ptr(), stream(dev))
    assert rc == L.EUNSUPPORTED


# ================================================================================================ log-mel pieces
def _reflect_cases():
    out = []
    for T in (2, 257, 16000, 70001):                  # 70001 + 2 pad > 256 * 256: the capped grid strides more than once
        for pad in sorted({0, 1, T // 2, T - 1}):
            out.append((T, pad))
    return out


@pytest.mark.parametrize('T,pad', _reflect_cases())
def test_reflect_pad(T, pad, dev):
    """tdvc_reflect_pad_fwd (bit-exact) / _bwd (the mirrored taps folded back) against F.pad(mode='reflect') and its autograd."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, Tp = 3, T + 2 * pad
    gen = torch.Generator().manual_seed(T * 7 + pad)
    x = torch.randn(B, T, generator=gen)
    dy = torch.randn(B, Tp, generator=gen)
    xd = x.to(dev)
    yb, y = _padded(torch.full((B * Tp,), SENT), dev)
    L.check(lib.tdvc_reflect_pad_fwd(xd.data_ptr(), y.data_ptr(), B, T, pad, st))
    dyd = dy.to(dev)
    dxb, dx = _padded(torch.full((B * T,), SENT), dev)
    L.check(lib.tdvc_reflect_pad_bwd(dyd.data_ptr(), dx.data_ptr(), B, T, pad, st))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().reshape(B, Tp), F.pad(x.unsqueeze(1), (pad, pad), mode='reflect').squeeze(1))
    xr = torch.zeros(B, 1, T, dtype=torch.float64, requires_grad=True)
    F.pad(xr, (pad, pad), mode='reflect').backward(dy.double().unsqueeze(1))
    xa = torch.zeros(B, 1, T, dtype=torch.float64, requires_grad=True)
    F.pad(xa, (pad, pad), mode='reflect').backward(dy.double().abs().unsqueeze(1))
    _ew(dx, xr.grad.reshape(B * T), EW * xa.grad.reshape(B * T), f'reflect_pad_bwd T={T} pad={pad}')
    assert _guards_intact(yb, 1, B * Tp) and _guards_intact(dxb, 1, B * T)


def test_reflect_pad_refuses_pad_ge_T(dev):
    L = _lib()
    x = torch.zeros(2, 64, device=dev)
    y = torch.zeros(2, 64 * 3, device=dev)
    assert L.lib().tdvc_reflect_pad_fwd(x.data_ptr(), y.data_ptr(), 2, 64, 64, stream(dev)) == EINVAL
    assert L.lib().tdvc_reflect_pad_bwd(y.data_ptr(), x.data_ptr(), 2, 64, 64, stream(dev)) == EINVAL


@pytest.mark.parametrize('B,Fq,N', [(1, 3, 5), (2, 1028, 257)], ids=['tiny', 'nfft2048_capped_grid'])
def test_power(B, Fq, N, dev):
    """power [B][F][N] = re^2 + im^2 of spec [B][2F][N] (re rows, then im rows); dspec = 2 dpower spec."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    gen = torch.Generator().manual_seed(Fq)
    spec = torch.randn(B, 2 * Fq, N, generator=gen)
    dpw = torch.randn(B, Fq, N, generator=gen)
    sd, dpd = spec.to(dev), dpw.to(dev)
    pw = torch.full((B, Fq, N), SENT, device=dev)
    ds = torch.full((B, 2 * Fq, N), SENT, device=dev)
    L.check(lib.tdvc_power_fwd(sd.data_ptr(), pw.data_ptr(), B, Fq, N, st))
    L.check(lib.tdvc_power_bwd(sd.data_ptr(), dpd.data_ptr(), ds.data_ptr(), B, Fq, N, st))
    torch.cuda.synchronize()
    sr = spec.double().requires_grad_(True)
    p = sr[:, :Fq] ** 2 + sr[:, Fq:] ** 2
    p.backward(dpw.double())
    _ew(pw, p.detach(), EW * p.detach(), 'power_fwd')
    _ew(ds, sr.grad, EW * sr.grad.abs(), 'power_bwd')


FLOOR = f32(1e-5)


def _log_l1_ref(a, b, weight, up):
    ar = a.double().requires_grad_(True)
    loss = weight * (torch.log(torch.clamp(ar, min=FLOOR)) - torch.log(torch.clamp(b.double(), min=FLOOR))).abs().mean()
    (loss * up).backward()
    return loss.item(), ar.grad


def _log_l1_run(a, b, weight, up, dev):
    L = _lib()
    lib, st = L.lib(), stream(dev)
    n = a.numel()
    ab, ad = _padded(a, dev)
    bd = b.to(dev)
    out = torch.zeros(1, device=dev)
    for _ in range(2):
        L.check(lib.tdvc_log_l1_fwd(ad.data_ptr(), bd.data_ptr(), n, FLOOR, weight, out.data_ptr(), st))
    dab, da = _padded(torch.full((n,), SENT), dev)
    upd = torch.tensor([up], device=dev)
    L.check(lib.tdvc_log_l1_bwd(ad.data_ptr(), bd.data_ptr(), n, FLOOR, weight, upd.data_ptr(), da.data_ptr(), st))
    torch.cuda.synchronize()
    assert _guards_intact(dab, 1, n)
    return float(out), da.cpu().double()


# (a, b) around the floor: a on it with b above / below / on it, each side below it, a == b, b on it
LOG_L1_SPECIAL = [(FLOOR, 1e-3), (FLOOR, 1e-7), (FLOOR, FLOOR), (3e-6, 0.02), (0.02, 3e-6), (2e-6, 7e-6), (0.5, 0.5), (0.5, FLOOR),
                  (FLOOR, 0.5)]


def test_log_l1_bwd_floor_value(dev):
    """log(clamp(x, floor)) passes its gradient where x >= floor (torch.clamp, and the oracle that uses it): at a == floor the
    gradient of |log a - log b| is sign(...) / floor, not 0."""
    a = torch.tensor([s[0] for s in LOG_L1_SPECIAL], dtype=torch.float32)
    b = torch.tensor([s[1] for s in LOG_L1_SPECIAL], dtype=torch.float32)
    weight, up = f32(0.9), 1.4
    assert float(a[0]) == FLOOR
    loss, ref = _log_l1_ref(a, b, weight, up)
    got_loss, da = _log_l1_run(a, b, weight, up, dev)
    assert ref[0] != 0.0
    _ew(da, ref, EW * ref.abs(), 'log_l1_bwd at the floor')
    _loss_ok(got_loss, 2 * loss, 'log_l1_fwd')


@pytest.mark.parametrize('n', LOSS_N)
def test_log_l1(n, dev):
    """tdvc_log_l1_fwd / _bwd against float64 autograd of weight mean|log clamp(a) - log clamp(b)| on mel-like magnitudes
    (1e-7 .. 10) with the floor cases planted at the front."""
    gen = torch.Generator().manual_seed(n + 5)
    a = (10.0 ** (8.0 * torch.rand(n, generator=gen, dtype=torch.float64) - 7.0)).float()
    b = (10.0 ** (8.0 * torch.rand(n, generator=gen, dtype=torch.float64) - 7.0)).float()
    b[::7] = a[::7]
    k = min(n, len(LOG_L1_SPECIAL))
    a[:k] = torch.tensor([s[0] for s in LOG_L1_SPECIAL[:k]])
    b[:k] = torch.tensor([s[1] for s in LOG_L1_SPECIAL[:k]])
    # |log a - log b| either 0 or > 1e-3 after the clamp: the fp32 logs then agree with float64 on its sign
    la, lb = torch.log(a.double().clamp(min=FLOOR)), torch.log(b.double().clamp(min=FLOOR))
    close = ((la - lb).abs() < 1e-3) & ((la - lb) != 0)
    b[close] = a[close]
    weight, up = f32(0.9), 1.4
    loss, ref = _log_l1_ref(a, b, weight, up)
    got_loss, da = _log_l1_run(a, b, weight, up, dev)
    _loss_ok(got_loss, 2 * loss, 'log_l1_fwd')
    _ew(da, ref, EW * ref.abs(), 'log_l1_bwd')


@pytest.mark.parametrize('n_fft', [512, 1024, 2048])
def test_melspec_power_matches_torch_stft(n_fft, dev):
    """losses.MelSpec's power spectrogram (reflect pad, the STFT as a strided conv with the windowed DFT basis, power) against
    float64 torch.stft (periodic Hann, centre, reflect), and the mel projection against float64 fb @ power with the repo's
    filterbank (the filterbank itself is not pinned here)."""
    pkg = _pkg()
    LS, ops = pkg.losses, pkg.ops
    B, T, sr = 2, 16000, 16000
    gen = torch.Generator().manual_seed(n_fft)
    t = torch.arange(T, dtype=torch.float64) / sr
    x = torch.zeros(B, T, dtype=torch.float64)
    for i in range(B):
        for f0, amp in ((110.0 * (i + 1), 0.5), (440.0 + 30 * i, 0.2), (2300.0, 0.05)):
            x[i] += amp * torch.sin(2 * math.pi * f0 * t + float(torch.rand(1, generator=gen)) * 6.28)
    x += 0.01 * torch.randn(B, T, generator=gen, dtype=torch.float64)
    x = x.float()
    ms = LS.MelSpec(sr, n_fft, 80)
    Fq = n_fft // 2 + 1
    with torch.no_grad():
        xd = x.to(dev).unsqueeze(1)
        ms._to(xd.device)
        xp = LS._ReflectPadFn.apply(xd, n_fft // 2)
        pw = LS._PowerFn.apply(ops.conv(xp, ms.stft_spec))
        mel = ops.conv(pw, ms.mel_spec)
    torch.cuda.synchronize()
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    ref = torch.stft(x.double(), n_fft, hop_length=n_fft // 4, win_length=n_fft, window=win, center=True, pad_mode='reflect',
                     return_complex=True).abs() ** 2
    pwc = pw.cpu().double()
    assert pwc.shape[2] == ref.shape[2] == 1 + T // (n_fft // 4)
    assert rel_l2(pwc[:, :Fq], ref) < TOL, rel_l2(pwc[:, :Fq], ref)
    assert (pwc[:, Fq:] == 0).all()            # the rows padding F to a multiple of 4 carry nothing into the mel projection
    fb = torch.from_numpy(LS._mel_filterbank(Fq, 80, sr))      # [F, n_mels], float64
    mel_ref = torch.einsum('fm,bfn->bmn', fb, pwc[:, :Fq])
    assert rel_l2(mel, mel_ref) < TOL, rel_l2(mel, mel_ref)


# ================================================================================================ glue
@pytest.mark.parametrize('C_', [1, 128])
def test_l2norm(C_, dev):
    """tdvc_l2norm_fwd / _bwd against float64 F.normalize(dim=1, eps=1e-12) and its autograd; T = 300 (not a multiple of 256)
    with an all-zero column."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, T = 2, 300
    eps = f32(1e-12)
    gen = torch.Generator().manual_seed(C_)
    x = torch.randn(B, C_, T, generator=gen)
    x[0, :, 7] = 0.0
    dy = torch.randn(B, C_, T, generator=gen)
    xd, dyd = x.to(dev), dy.to(dev)
    y = torch.full((B, C_, T), SENT, device=dev)
    inv = torch.full((B, T), SENT, device=dev)
    dx = torch.full((B, C_, T), SENT, device=dev)
    L.check(lib.tdvc_l2norm_fwd(xd.data_ptr(), y.data_ptr(), inv.data_ptr(), B, C_, T, eps, st))
    L.check(lib.tdvc_l2norm_bwd(y.data_ptr(), inv.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, C_, T, st))
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    yr = F.normalize(xr, dim=1, eps=eps)
    yr.backward(dy.double())
    inv_ref = 1.0 / x.double().norm(dim=1).clamp(min=eps)
    live = torch.ones(B, T, dtype=torch.bool)
    live[0, 7] = False
    yc, dxc, ic = y.cpu().double(), dx.cpu().double(), inv.cpu().double()
    assert (yc[0, :, 7] == 0).all()
    _ew(ic[0, 7], inv_ref[0, 7], EW * inv_ref[0, 7], 'inv of the zero column')
    _ew(dxc[0, :, 7], xr.grad[0, :, 7], EW * xr.grad[0, :, 7].abs(), 'dx of the zero column: dy / eps')
    lv = live.unsqueeze(1).expand(B, C_, T)
    assert rel_l2(yc[lv], yr.detach()[lv]) < TOL
    assert rel_l2(ic[live], inv_ref[live]) < TOL
    scale = float((dy.double() * inv_ref.unsqueeze(1))[lv].norm())      # C = 1: dx cancels to ~0, the terms set the scale
    assert _rel_scaled(dxc[lv], xr.grad[lv], scale) < TOL


def test_gather_ch(dev):
    """tdvc_gather_ch_fwd: y[b][t] = x[b][label_b][t]; _bwd: dx[b][c][t] = dy[b][t] on the label's channel, 0 on the others
    (every element written). Labels 0 and C - 1."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, C_, T = 3, 5, 300
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, C_, T, generator=gen)
    dy = torch.randn(B, T, generator=gen)
    lab = torch.tensor([0, C_ - 1, 2], dtype=torch.int64)
    xd, dyd, ld = x.to(dev), dy.to(dev), lab.to(dev)
    y = torch.full((B, T), SENT, device=dev)
    dx = torch.full((B, C_, T), SENT, device=dev)
    L.check(lib.tdvc_gather_ch_fwd(xd.data_ptr(), ld.data_ptr(), y.data_ptr(), B, C_, T, st))
    L.check(lib.tdvc_gather_ch_bwd(dyd.data_ptr(), ld.data_ptr(), dx.data_ptr(), B, C_, T, st))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x[torch.arange(B), lab])
    want = torch.zeros(B, C_, T)
    want[torch.arange(B), lab] = dy
    assert torch.equal(dx.cpu(), want)


@pytest.mark.parametrize('accumulate', [0, 1])
def test_concat_cond(accumulate, dev):
    """tdvc_concat_cond: c = cat(emb repeated over T, exc) (bit-exact); _bwd: demb (+)= sum_t dc[:, :Ce], dexc = dc[:, Ce:]."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, Ce, Cx, T = 3, 128, 8, 300
    gen = torch.Generator().manual_seed(4 + accumulate)
    emb = torch.randn(B, Ce, generator=gen)
    exc = torch.randn(B, Cx, T, generator=gen)
    dc = torch.randn(B, Ce + Cx, T, generator=gen)
    pre = torch.randn(B, Ce, generator=gen) if accumulate else torch.full((B, Ce), SENT)
    ed, xd, dcd = emb.to(dev), exc.to(dev), dc.to(dev)
    c = torch.full((B, Ce + Cx, T), SENT, device=dev)
    demb = pre.to(dev)
    dexc = torch.full((B, Cx, T), SENT, device=dev)
    L.check(lib.tdvc_concat_cond(ed.data_ptr(), xd.data_ptr(), c.data_ptr(), B, Ce, Cx, T, st))
    L.check(lib.tdvc_concat_cond_bwd(dcd.data_ptr(), demb.data_ptr(), dexc.data_ptr(), B, Ce, Cx, T, accumulate, st))
    torch.cuda.synchronize()
    assert torch.equal(c.cpu(), torch.cat([emb.unsqueeze(2).expand(B, Ce, T), exc], 1))
    assert torch.equal(dexc.cpu(), dc[:, Ce:])
    ref = dc[:, :Ce].double().sum(2) + (pre.double() if accumulate else 0.0)
    assert rel_l2(demb, ref) < TOL


@pytest.mark.parametrize('T', [3, 4, 257, 16000])
def test_edge_sum3(T, dev):
    """out[b][c] = (d[..., 0], sum d[..., 1:T-1], d[..., T-1])."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, C_ = 2, 5
    d = torch.randn(B, C_, T, generator=torch.Generator().manual_seed(T))
    dd = d.to(dev)
    ob, out = _padded(torch.full((B * C_ * 3,), SENT), dev)
    L.check(lib.tdvc_edge_sum3(dd.data_ptr(), out.data_ptr(), B, C_, T, st))
    torch.cuda.synchronize()
    o = out.cpu().reshape(B, C_, 3)
    assert torch.equal(o[..., 0], d[..., 0]) and torch.equal(o[..., 2], d[..., T - 1])
    assert rel_l2(o[..., 1], d[..., 1:T - 1].double().sum(-1)) < TOL
    assert _guards_intact(ob, 1, B * C_ * 3)


def test_edge_sum3_refuses_T_below_3(dev):
    L = _lib()
    d = torch.zeros(2, 5, 3, device=dev)
    out = torch.zeros(2, 5, 3, device=dev)
    assert L.lib().tdvc_edge_sum3(d.data_ptr(), out.data_ptr(), 2, 5, 2, stream(dev)) == EINVAL


@pytest.mark.parametrize('T', [257, 20000])
def test_roll_batches(T, dev):
    """y[b] = torch.roll(x[b], shift[b], -1) for shifts 0, +-1, T-1, +-T, +-(3T+5). T = 20000 > 64 * 256: the capped grid strides."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    shifts = [0, 1, -1, T - 1, T, -T, 3 * T + 5, -(3 * T + 5)]
    B, C_ = len(shifts), 3
    x = torch.randn(B, C_, T, generator=torch.Generator().manual_seed(T))
    xd, sd = x.to(dev), torch.tensor(shifts, dtype=torch.int64, device=dev)
    y = torch.full((B, C_, T), SENT, device=dev)
    L.check(lib.tdvc_roll_batches(xd.data_ptr(), sd.data_ptr(), y.data_ptr(), B, C_, T, st))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.stack([torch.roll(x[b], s, -1) for b, s in enumerate(shifts)]))


def _strided(B, rows, T, bs, src, dev):
    """src [B][rows][T] stored with batch stride bs >= rows T in a SENT-filled buffer."""
    buf = torch.full((B * bs,), SENT, device=dev)
    if src is not None:
        buf.as_strided((B, rows, T), (bs, T, 1)).copy_(src)
    return buf


@pytest.mark.parametrize('B,H,T', [(3, 16, 333), (2, 64, 8200)], ids=['small', 'capped_grid'])
@pytest.mark.parametrize('with_g', [False, True], ids=['g_null', 'g'])
def test_gate(B, H, T, with_g, dev):
    """tdvc_gate_fwd / _bwd (acts = tanh(a) sigmoid(s) of the WaveNet stack) with every batch stride wider than contiguous;
    the gaps between samples stay untouched."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    HT = H * T
    gen = torch.Generator().manual_seed(H + T + with_g)
    xin = torch.randn(B, 2 * H, T, generator=gen) * 1.5
    g = torch.randn(B, 2 * H, T, generator=gen) if with_g else None
    dacts = torch.randn(B, H, T, generator=gen)
    xbs, gbs, abs_, dabs, dxbs = 2 * HT + 37, 2 * HT + 11, HT + 5, HT + 3, 2 * HT + 7
    xb = _strided(B, 2 * H, T, xbs, xin, dev)
    gbuf = _strided(B, 2 * H, T, gbs, g, dev) if with_g else None
    ab = _strided(B, H, T, abs_, None, dev)
    dab = _strided(B, H, T, dabs, dacts, dev)
    dxb = _strided(B, 2 * H, T, dxbs, None, dev)
    L.check(lib.tdvc_gate_fwd(xb.data_ptr(), xbs, gbuf.data_ptr() if with_g else None, gbs, ab.data_ptr(), abs_, B, H, T, st))
    L.check(lib.tdvc_gate_bwd(xb.data_ptr(), xbs, gbuf.data_ptr() if with_g else None, gbs, dab.data_ptr(), dabs, dxb.data_ptr(), dxbs,
                              B, H, T, st))
    torch.cuda.synchronize()
    z = xin.double() + (g.double() if with_g else 0.0)
    th, sg = torch.tanh(z[:, :H]), torch.sigmoid(z[:, H:])
    d = dacts.double()
    acts = ab.cpu().as_strided((B, H, T), (abs_, T, 1))
    _ew(acts, th * sg, EW * (th * sg).abs(), 'gate_fwd')
    dx = dxb.cpu().as_strided((B, 2 * H, T), (dxbs, T, 1))
    # bounds relative to the terms of 1 - tanh^2 and 1 - sigmoid (both cancel where the gate saturates)
    _ew(dx[:, :H], d * sg * (1 - th * th), EW * (d * sg).abs() * (1 + th * th), 'gate_bwd tanh half')
    _ew(dx[:, H:], d * th * sg * (1 - sg), EW * (d * th * sg).abs() * (1 + sg), 'gate_bwd sigmoid half')
    for buf, bs, used in ((ab, abs_, HT), (dxb, dxbs, 2 * HT)):
        gaps = buf.cpu().reshape(B, bs)[:, used:]
        assert (gaps == SENT).all(), 'write into the gap between samples'


@pytest.mark.parametrize('n', [3, 256 * 4096 + 5], ids=['n3', 'capped_grid'])
@pytest.mark.parametrize('with_b', [False, True], ids=['b_null', 'b'])
def test_axpby_and_fill(n, with_b, dev):
    """tdvc_axpby: y = alpha a + beta b (b NULL: alpha a); tdvc_fill: y = value; unaligned views, nothing outside written."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    gen = torch.Generator().manual_seed(n + with_b)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    alpha, beta = f32(-0.7), f32(1.3)
    _, ad = _padded(a, dev)
    _, bd = _padded(b, dev)
    yb, y = _padded(torch.full((n,), SENT), dev)
    L.check(lib.tdvc_axpby(ad.data_ptr(), bd.data_ptr() if with_b else None, y.data_ptr(), alpha, beta, n, st))
    fb, fv = _padded(torch.full((n,), SENT), dev)
    L.check(lib.tdvc_fill(fv.data_ptr(), 0.375, n, st))
    torch.cuda.synchronize()
    ref = alpha * a.double() + (beta * b.double() if with_b else 0.0)
    _ew(y, ref, EW * (abs(alpha) * a.double().abs() + (abs(beta) * b.double().abs() if with_b else 0.0)), 'axpby')
    assert (fv.cpu() == 0.375).all()
    assert _guards_intact(yb, 1, n) and _guards_intact(fb, 1, n)


# ================================================================================================ film_k3
def _k3_case(n_const, nblk, B):
    nc = n_const + 8
    gen = torch.Generator().manual_seed(n_const * 100 + nblk)
    emb_bs = n_const + 5                               # the embedding is a row view of a wider tensor
    emb_full = torch.randn(B, emb_bs, generator=gen)
    emb = emb_full[:, :n_const]
    w0 = [torch.randn(nc, nc, 3, generator=gen) / math.sqrt(nc * 3) for _ in range(nblk)]
    b0 = [torch.randn(nc, generator=gen) * 0.1 for _ in range(nblk)]
    dk3 = [torch.randn(B, nc, 3, generator=gen) for _ in range(nblk)]
    dw_pre = [torch.randn(nc, nc, 3, generator=gen) * 0.5 for _ in range(nblk)]
    db_pre = [torch.randn(nc, generator=gen) * 0.5 for _ in range(nblk)]
    return nc, emb_bs, emb_full, emb, w0, b0, dk3, dw_pre, db_pre


def _k3_ref(emb, w0, b0, dk3, nc):
    """k3 = conv1d over the length-3 constant signal emb (channels n_const.. of the input are 0), zero 'same' padding."""
    B, n_const = emb.shape
    e = emb.double().requires_grad_(True)
    x = torch.zeros(B, nc, 3, dtype=torch.float64)
    x = torch.cat([e.unsqueeze(2).expand(B, n_const, 3), x[:, n_const:]], 1)
    w, b = w0.double().requires_grad_(True), b0.double().requires_grad_(True)
    k3 = F.conv1d(x, w, b, padding=1)
    k3.backward(dk3.double())
    return k3.detach(), e.grad, w.grad, b.grad


@pytest.mark.parametrize('n_const', [1, 64, 65, 256])
@pytest.mark.parametrize('nblk', [1, 16])
@pytest.mark.parametrize('multi', [False, True], ids=['single', 'multi'])
def test_film_k3_vs_float64(n_const, nblk, multi, dev):
    """tdvc_film_k3_fwd / _bwd (per FiLM block) and tdvc_film_k3_multi_fwd / _bwd (all blocks of a stage, the embedding gradient
    summed over them) against float64 conv1d autograd. B = 7 (not a multiple of the forward's 4 samples per block); dw0 / db0
    are added into (+=), and dw0's columns of the non-constant input channels stay untouched."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B = 7
    nc, emb_bs, emb_full, emb, w0, b0, dk3, dw_pre, db_pre = _k3_case(n_const, nblk, B)
    ed = emb_full.to(dev)
    w0d, b0d, dk3d = [t.to(dev) for t in w0], [t.to(dev) for t in b0], [t.to(dev) for t in dk3]
    k3d = [torch.full((B, nc, 3), SENT, device=dev) for _ in range(nblk)]
    dwd, dbd = [t.to(dev) for t in dw_pre], [t.to(dev) for t in db_pre]
    if multi:
        P = lambda ts: (C.c_void_p * nblk)(*[t.data_ptr() for t in ts])
        demb = torch.full((B, n_const), SENT, device=dev)
        L.check(lib.tdvc_film_k3_multi_fwd(ed.data_ptr(), emb_bs, P(w0d), P(b0d), P(k3d), nblk, B, n_const, nc, st))
        L.check(lib.tdvc_film_k3_multi_bwd(P(dk3d), ed.data_ptr(), emb_bs, P(w0d), demb.data_ptr(), P(dwd), P(dbd), nblk, B, n_const, nc, st))
        dembs = [demb]
    else:
        dembs = [torch.full((B, n_const), SENT, device=dev) for _ in range(nblk)]
        for i in range(nblk):
            L.check(lib.tdvc_film_k3_fwd(ed.data_ptr(), emb_bs, w0d[i].data_ptr(), b0d[i].data_ptr(), k3d[i].data_ptr(), B, n_const, nc, st))
            L.check(lib.tdvc_film_k3_bwd(dk3d[i].data_ptr(), ed.data_ptr(), emb_bs, w0d[i].data_ptr(), dembs[i].data_ptr(), dwd[i].data_ptr(),
                                         dbd[i].data_ptr(), B, n_const, nc, st))
    torch.cuda.synchronize()
    demb_sum = torch.zeros(B, n_const, dtype=torch.float64)
    for i in range(nblk):
        k3r, der, dwr, dbr = _k3_ref(emb, w0[i], b0[i], dk3[i], nc)
        demb_sum += der
        assert rel_l2(k3d[i], k3r) < TOL, ('k3', i)
        dw = dwd[i].cpu()
        assert rel_l2(dw[:, :n_const], dw_pre[i][:, :n_const].double() + dwr[:, :n_const]) < TOL, ('dw0', i)
        assert torch.equal(dw[:, n_const:], dw_pre[i][:, n_const:]), ('dw0 written outside the constant channels', i)
        assert rel_l2(dbd[i], db_pre[i].double() + dbr) < TOL, ('db0', i)
        if not multi:
            assert rel_l2(dembs[i], der) < TOL, ('demb', i)
    if multi:
        assert rel_l2(dembs[0], demb_sum) < TOL, 'demb summed over the blocks'


def test_film_k3_refuses_n_const_above_256(dev):
    """The forward keeps a weight row of <= 256 constant channels in registers: 257 -> TDVC_EINVAL before any launch."""
    L = _lib()
    lib, st = L.lib(), stream(dev)
    B, n_const, nc = 2, 257, 265
    emb = torch.zeros(B, n_const, device=dev)
    w0 = torch.zeros(nc, nc, 3, device=dev)
    k3 = torch.zeros(B, nc, 3, device=dev)
    assert lib.tdvc_film_k3_fwd(emb.data_ptr(), n_const, w0.data_ptr(), None, k3.data_ptr(), B, n_const, nc, st) == EINVAL
    P = (C.c_void_p * 1)(w0.data_ptr())
    K = (C.c_void_p * 1)(k3.data_ptr())
    assert lib.tdvc_film_k3_multi_fwd(emb.data_ptr(), n_const, P, None, K, 1, B, n_const, nc, st) == EINVAL
