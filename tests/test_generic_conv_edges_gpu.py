"""Edge geometry of the GENERIC conv family against float64: conv_gemm_kernel<MODE,...> and its scalar twin (conv_mfma.hip),
conv_wgrad_kernel<MODE,M_REP,J> / conv_wgrad_scalar_kernel, the small-group kernels at their boundary, and the slab folds
(immediate and deferred) that end every weight-grad call.

The stride-1 lean family has test_lean_conv_edges_gpu.py (forward and input-grad; its weight-grad kernels: test_lean_wgrad_edges_gpu.py)
and test_kernel_instances_gpu.py; both edge suites drive the Edge class below. This file gives the generic family the same treatment:

  * every tile of launch_conv_gemm, pinned through tdvc_debug_force_gemm_tile, at small ragged shapes with NaN-poisoned LDS;
  * sequence lengths that are no multiple of 4, channel counts per group that are no multiple of 4 / 16, out_pad > 0,
    K % stride != 0, K < stride, grouped transposed convs, stride >= 16 with padding, stride-1 convs with Tout != Tin,
    pad == (K-1)*dil, the reflect mirror fold of the MFMA input-grad, the w_cin window and FiLM on the generic route;
  * dw / dbias are ACCUMULATED (they start at random values), the weight-grad workspace is exactly the queried size with a
    guard behind it, outputs start as SENT and may be channel slices of wider buffers whose spare channels stay SENT.

Two bars per tensor, both required: rel-L2 < 2e-5 (the project's TOL) and the element-wise forward-error bound of an fp32 dot
product in any summation order,
    |got - ref| <= (n + 8) * 2^-23 * A + 2^-22 * |ref|,
n = reduction length, A = the same float64 computation on absolute values. Where A == 0 (input-gradient positions no window
reads, output holes of a transposed conv with K < stride, dw columns outside a w_cin window) got must equal fp32(ref) exactly.
The reference is computed from the fp32-rounded inputs, so only the kernel's own arithmetic differs. Every case asserts by
trace (tdvc_debug_trace) which kernel family or instance it ran: a silent reroute cannot pass.
"""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

import test_conv_ops_gpu as OPS
from common import rel_l2, traced

pytestmark = pytest.mark.gpu
TOL = 2e-5
SENT = -7777.25      # sentinel of test_misc_ops_gpu.py: every output buffer starts filled with it
U = 2.0 ** -23
SLOPE = 0.2
EWORKSPACE, EUNSUPPORTED = -2, -4


def _mods():
    pkg = importlib.import_module('td-vc-gan_amd')
    return pkg.ops, pkg._lib, pkg.arena


# (name, cin, cout, K, stride, pad, dil, groups, reflect, transposed, out_pad, T)
GEOM = [
    # strided: forward MODE_DOWN, input-grad MODE_UP
    ('down_r5', 24, 40, 10, 5, 3, 1, 1, False, False, 0, 203),          # the last input sample is read by no window
    ('down_r3', 20, 36, 6, 3, 2, 1, 1, False, False, 0, 130),
    ('down_k3_s4', 8, 24, 3, 4, 0, 1, 1, False, False, 0, 101),         # J = 1; phase 3 of dx is exactly 0
    ('down_k7_s2', 16, 16, 7, 2, 3, 1, 1, False, False, 0, 258),        # J = 4: scalar weight-grad
    ('down_s16_c2', 2, 40, 64, 16, 8, 1, 1, False, False, 0, 1000),     # stage_rows
    ('down_k9_s2_pad6', 12, 20, 9, 2, 6, 1, 1, False, False, 0, 75),
    ('grp3', 15, 21, 11, 4, 5, 1, 3, False, False, 0, 210),             # 5 channels in and 7 out per group
    ('down_128_T64_B11', 128, 128, 4, 2, 1, 1, 1, False, False, 0, 64), # weight-grad bpb = 2, last batch group ragged
    ('down_multitile', 16, 32, 4, 2, 1, 1, 1, False, False, 0, 2210),   # five weight-grad time tiles, last one ragged
    # small-group boundary
    ('sg_g17_k5_s2', 68, 68, 5, 2, 2, 1, 17, False, False, 0, 131),
    ('sg_g16_k48_s8', 64, 64, 48, 8, 20, 1, 16, False, False, 0, 500),
    ('sg_k49_generic', 64, 64, 49, 8, 24, 1, 16, False, False, 0, 500), # one tap over the limit: the generic route
    # transposed: forward MODE_UP, input-grad MODE_DOWN
    ('up_r5', 40, 24, 10, 5, 3, 1, 1, False, True, 1, 41),
    ('up_r3', 36, 20, 6, 3, 2, 1, 1, False, True, 1, 43),
    ('up_k3_s4', 16, 8, 3, 4, 0, 1, 1, False, True, 3, 25),             # holes and the out_pad tail hold only the bias
    ('up_k7_s2', 16, 16, 7, 2, 3, 1, 1, False, True, 0, 129),
    ('up_grp3', 21, 15, 8, 4, 2, 1, 3, False, True, 0, 50),
    # stride 1 off the lean contract: MODE_DIRECT
    ('direct_valid_k5', 10, 18, 5, 1, 0, 1, 1, False, False, 0, 203),
    ('direct_pad_eq_field', 8, 8, 3, 1, 2, 1, 1, False, False, 0, 100),
    ('direct_reflect_T333', 12, 20, 7, 1, 9, 3, 1, True, False, 0, 333),
    ('direct_reflect_pad_Tm1', 6, 10, 11, 1, 25, 5, 1, True, False, 0, 26),
    ('direct_dil_notsame', 12, 12, 5, 1, 3, 4, 1, False, False, 0, 150),
    ('window_generic', 8, 24, 3, 1, 1, 1, 1, False, False, 0, 333),
]
GEOM = {c[0]: c for c in GEOM}
# pre / post: LeakyReLU before / after the conv. Both PIPE forms of the kernel (post = 1 makes the input-grad read a mask tensor)
# and the EPI_MASK input-grad (pre = 1) occur in every mode. `add`: a running sum on the forward (with out_scale = 0.5) and a
# residual gradient on the input-grad (add_scale = 0.75), never together with post (the backward mask is the stored output);
# `views`: operands are channel slices of [B, C + 3, T] buffers.
OPTS = {
    'down_r5': dict(pre=1, add=True, views=True), 'down_r3': dict(post=1), 'down_k3_s4': dict(pre=1, post=1), 'down_k7_s2': dict(),
    'down_s16_c2': dict(post=1), 'down_k9_s2_pad6': dict(pre=1), 'grp3': dict(pre=1, add=True, views=True),
    'down_128_T64_B11': dict(post=1, B=11), 'down_multitile': dict(pre=1, B=2),
    'sg_g17_k5_s2': dict(post=1), 'sg_g16_k48_s8': dict(post=1), 'sg_k49_generic': dict(post=1),
    'up_r5': dict(pre=1, add=True, views=True), 'up_r3': dict(post=1), 'up_k3_s4': dict(pre=1), 'up_k7_s2': dict(pre=1, post=1),
    'up_grp3': dict(post=1),
    'direct_valid_k5': dict(post=1), 'direct_pad_eq_field': dict(pre=1), 'direct_reflect_T333': dict(pre=1, add=True, views=True),
    'direct_reflect_pad_Tm1': dict(pre=1, post=1), 'direct_dil_notsame': dict(), 'window_generic': dict(pre=1, w_cin=14, w_cin_off=5),
    # lean-shaped, for the workspace contract and the deferred folds only
    'lean_c32_k3': dict(pre=1),
}
LEAN_GEOM = ('lean_c32_k3', 32, 32, 3, 1, 1, 1, 1, False, False, 0, 256)
WGRAD_MFMA_J = (1, 2, 3, 5, 7, 11)
GEMM_CFG = {0: (1, 4, 1, 4), 1: (2, 4, 1, 4), 2: (4, 4, 1, 4), 3: (1, 1, 1, 4), 4: (1, 4, 4, 1)}
MODE_DIRECT, MODE_DOWN, MODE_UP = 0, 1, 2


def _conv64(h, w, b, geom):
    """The float64 operation of one geometry on an already pre-activated input."""
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
    if transposed:
        return F.conv_transpose1d(h, w, b, stride=s, padding=p, output_padding=out_pad, groups=g)
    if reflect and p > 0:
        return F.conv1d(F.pad(h, (p, p), mode='reflect'), w, b, stride=s, dilation=d, groups=g)
    return F.conv1d(h, w, b, stride=s, padding=p, dilation=d, groups=g)


def _buf(B, Cc, T, dev, views, src=None, unaligned=False, fill=SENT):
    """(whole buffer, operand view): SENT-filled; with `views` the operand is the channel slice [:, :Cc] of a [B, Cc + 3, T] buffer
    (a batch stride wider than contiguous and, for odd T, planes that are not 16-byte aligned); with `unaligned` it lives one
    float into a flat buffer (contiguous rows, nothing 16-byte aligned; the float in front stays SENT). `fill`: what the buffer
    holds outside the operand (NaN behind the inputs of a `nan_spare` case)."""
    if unaligned:
        assert not views
        whole = torch.full((B * Cc * T + 1,), fill, dtype=torch.float32, device=dev)
        v = whole[1:].view(B, Cc, T)
    else:
        whole = torch.full((B, Cc + (3 if views else 0), T), fill, dtype=torch.float32, device=dev)
        v = whole[:, :Cc]
    if src is not None:
        v.copy_(src.to(dev))
    return whole, v


def _spare_intact(whole, Cc):
    if whole.dim() == 1:
        return bool(whole[0] == SENT)
    return whole.shape[1] == Cc or bool((whole[:, Cc:] == SENT).all())


def elem_check(got, ref, A, n, slack=8):
    """-> (worst err / bound over the elements with A > 0, number of elements with A == 0 that differ from fp32(ref)).
    `slack`: the roundings outside the summation the bound allows for (8; 12 with a FiLM prologue, Edge's docstring)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bound = (n + slack) * U * A + 2.0 ** -22 * ref.abs()
    zero = A == 0
    inexact = int((got[zero] != ref[zero].float()).sum())
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    if not bool(torch.isfinite(got).all()):
        ratio = float('nan')
    return ratio, inexact


class Edge:
    """One conv geometry through tdvc_conv_fwd / _dgrad / _wgrad against float64 CPU autograd (the module docstring has the rules).
    fwd() must run first: a post-LeakyReLU layer takes its backward mask from the GPU's own stored output, as the product does.

    Options beyond the geometry (the defaults are the plain case):
      with_db=False  dbias = NULL: db must stay db0 bit for bit and no bias-gradient kernel may run;
      wt=True        the slot carries the [Cin][Cout][K] weight copy the lean input-grad kernel reads;
      unaligned=True x, dy, y, dx (and add / FiLM operands) start 4 bytes into flat buffers: contiguous rows, nothing 16-byte aligned;
      film=True      (1x1 convs) the input prologue is FiLM + LeakyReLU, x' = lrelu(h * (1 + gamma) + beta), with gb = [gamma planes,
                     beta planes] as XF_FILM_LRELU's aux operand, and the input-grad runs the FiLM epilogue (dh, dgamma, dbeta).
    The FiLM bound: the GPU forms x' in fp32 from fp32 h, gamma, beta: 1 + gamma, the product and the sum are three roundings, each at
    most 2^-24 of a partial result no larger than H = |h| (1 + |gamma|) + |beta|, so |x'_gpu - x'| <= 3 * 2^-24 * H on either side of
    the kink. An element within that distance of 0 may take the other LeakyReLU branch: the branches differ by 0.8 |h2| there, at most
    0.8 * 3 * 2^-24 * H more. Together < 3 * 2^-23 * H per element, i.e. 3 more units of 2^-23 * A when A is computed from H instead of
    |x'|. So the FiLM cases take A from H and n + 12 for n + 8. The input-grad's mask is discontinuous at the kink; the seeded data is
    asserted to hold no element that close to it, so both sides take the same branch everywhere.

    Options of the forward / input-grad edge suite of the lean family (test_lean_conv_edges_gpu.py; none of them changes what the
    other options draw):
      res=True       forward y = out_scale * (conv + bias + res) + add with `res` a tensor of its own (own buffer, own batch stride);
      bias3=True     a per-sample bias [B, Cout, 3] on top: [.., 0] at t = 0, [.., 1] in the interior, [.., 2] at t = T - 1. The kernel may
                     add the interior value everywhere and correct the two ends by (end - interior), so A takes |interior| + |end| +
                     |interior| at the ends. Together with res that is four roundings more, two units of the slack;
      post=2         tanh. y is 1-Lipschitz in the conv result, so the summation bound carries over unchanged; device tanhf adds an
                     absolute term `tanh_allow` (units of 2^-24, measured by the caller on another kernel). The backward mask is
                     1 - y^2 of the GPU's own stored y (XF_MASK_TANH), as the product's;
      bias=False     no bias pointer in the slot;
      bits=True      the forward also packs sign words ([B, Cout, T / 32] int32, a view of a wider buffer when y is one): they must
                     equal pack_sign_bits(stored y) bit for bit; dgrad(x_bits=words) reads its LeakyReLU mask from such words;
      nan_spare=True everything outside the INPUT operands (spare channels of a view, the float in front of an unaligned one) is NaN
                     instead of SENT: a read past Cin, or of a column past T of the last row, lands there;
      x_src          the input values (default: seeded random), e.g. the stored output of the layer in front;
      views          True / False for every operand, or the names of the operands that are views (x, dy, y, dx, add, res, gb, dgb,
                     bits): mixed batch strides.
    A FiLM prologue with K > 1 is outside the product's use but inside the C ABI (film=True then keeps pre = 0 only)."""

    def __init__(self, geom, dev, generic=0, B=3, pre=0, post=0, add=False, views=False, w_cin=0, w_cin_off=0,
                 with_db=True, wt=False, unaligned=False, film=False, res=False, bias3=False, bias=True, bits=False,
                 nan_spare=False, x_src=None, tanh_allow=0.0):
        ops, L, arena = _mods()
        (name, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
        assert not (add and post), 'the backward mask of a post-activated layer is its stored output: no running sum on top'
        self.geom, self.dev, self.generic, self.B, self.pre, self.post, self.views = geom, dev, generic, B, pre, post, views
        self.cin, self.cout, self.T = cin, cout, T
        self.with_db, self.film, self.unaligned, self.slack = with_db, film, unaligned, 12 if film else 8
        self.has_bias, self.tanh_allow = bias, tanh_allow
        assert not film or not pre, 'FiLM stands in place of the plain LeakyReLU'
        assert post in (0, 1, 2) and not (post == 2 and (add or res))
        self.out_scale, self.add_scale = (0.5, 0.75) if add else (1.0, 1.0)
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        rnd = lambda *sh: torch.randn(*sh, generator=gen).float()      # fp32 values: the reference reads the same numbers
        vw = (lambda n: views) if isinstance(views, bool) else (lambda n: n in views)
        nanf = float('nan') if nan_spare else SENT
        wshape = (cin, cout // g, k) if transposed else (cout, (w_cin or cin) // g, k)
        self.win = slice(w_cin_off, w_cin_off + cin) if w_cin else slice(None)      # the weight's input-channel window
        self.spec = ops.ConvSpec(cin, cout, k, s, p, d, g, reflect, transposed, out_pad, w_cin, w_cin_off)
        self.tout = self.spec.tout(T)
        self.x, self.w, self.b = rnd(B, cin, T), rnd(*wshape) / (wshape[1] * k) ** 0.5, rnd(cout) * 0.1
        self.cot = rnd(B, cout, self.tout)
        self.add_y = rnd(B, cout, self.tout) if add else None
        self.add_x = rnd(B, cin, T) if add else None
        self.dw0, self.db0 = rnd(*wshape), rnd(cout)
        self.gb = rnd(B, 2 * cin, T) * 0.5 if film else None      # drawn last: the other tensors of a case do not depend on the option
        self.res = rnd(B, cout, self.tout) if res else None
        self.k3 = rnd(B, cout, 3) * 0.3 if bias3 else None
        if x_src is not None:
            assert x_src.shape == self.x.shape and x_src.dtype == torch.float32
            self.x = x_src.detach().cpu().clone()
        # n of the bound: reduction length per tensor
        self.n = dict(y=cin // g * k, dx=cout // g * k, dw=B * self.tout, db=B * self.tout)
        f = lambda t: t.to(dev).contiguous()
        self.wd, self.bd, self.dw, self.db = f(self.w), f(self.b), f(self.dw0), f(self.db0)
        self.wtd = self.wd.permute(1, 0, 2).contiguous() if wt else None      # [Cin (or w_cin)][Cout][K]
        self.spec.slot = arena.ConvSlot(self.wd.data_ptr(), self.bd.data_ptr() if bias else 0, self.dw.data_ptr(), self.db.data_ptr(), True, None,
                                        self.wtd.data_ptr() if wt else 0)
        self.x_whole, self.xv = _buf(B, cin, T, dev, vw('x'), self.x, unaligned, nanf)
        self.dy_whole, self.dyv = _buf(B, cout, self.tout, dev, vw('dy'), self.cot, unaligned, nanf)
        self.y_whole, self.yv = _buf(B, cout, self.tout, dev, vw('y'), None, unaligned)
        self.dx_whole, self.dxv = _buf(B, cin, T, dev, vw('dx'), None, unaligned)
        self.addy_v = _buf(B, cout, self.tout, dev, vw('add'), self.add_y, unaligned, nanf)[1] if add else None
        self.addx_v = _buf(B, cin, T, dev, vw('add'), self.add_x, unaligned, nanf)[1] if add else None
        self.res_v = _buf(B, cout, self.tout, dev, vw('res'), self.res, unaligned, nanf)[1] if res else None
        self.k3d = f(self.k3) if bias3 else None
        self.bits_whole = self.bits_v = None
        if bits:      # int32 words; the fill pattern is SENT's own bit pattern, so _spare_intact's comparison carries over
            assert self.tout % 32 == 0
            self.bits_whole = torch.full((B, cout + (3 if vw('bits') else 0), self.tout // 32), SENT, dtype=torch.float32, device=dev).view(torch.int32)
            self.bits_v = self.bits_whole[:, :cout]
        self.x_xf = ops._xf(L.XF_LRELU if pre else L.XF_NONE)
        if film:
            self.gbv = _buf(B, 2 * cin, T, dev, vw('gb'), self.gb, unaligned, nanf)[1]
            self.dgb_whole, self.dgbv = _buf(B, 2 * cin, T, dev, vw('dgb'), None, unaligned)
            self.x_xf = ops._xf(L.XF_FILM_LRELU, aux=self.gbv)
        self.names = {}

    def _call(self, what, fn):
        L = _mods()[1]
        L.lib().tdvc_set_force_generic(self.generic)
        tr = traced()
        try:
            with tr:
                out = fn()
        finally:
            L.lib().tdvc_set_force_generic(0)
            self.names[what] = tr.names      # also of a call that raised: what it launched before it refused
        return out

    def fwd(self):
        ops, L, _ = _mods()
        self._call('fwd', lambda: ops.conv_fwd_raw(self.spec, self.xv, self.x_xf, post=(L.POST_NONE, L.POST_LRELU, L.POST_TANH)[self.post],
                                                    res=self.res_v, add=self.addy_v, out_scale=self.out_scale, out=self.yv,
                                                    bias3=self.k3d, sign_bits=self.bits_v))
        y = self.yv.detach().cpu()
        # float64 reference, and the same computation on absolute values for the bound
        xr, wr, br = (t.double().requires_grad_(True) for t in (self.x, self.w, self.b))
        if self.film:
            gbr = self.gb.double().requires_grad_(True)
            h2 = xr * (1 + gbr[:, :self.cin]) + gbr[:, self.cin:]
            H = self.film_H()
            self.assert_off_kink()
        z = _conv64(F.leaky_relu(h2, SLOPE) if self.film else F.leaky_relu(xr, SLOPE) if self.pre else xr, wr[:, self.win],
                    br if self.has_bias else None, self.geom)
        extra = torch.zeros_like(z.detach())      # |bias3| and |res| as the kernel may add them (Edge's docstring)
        if self.k3 is not None:
            k3 = self.k3.double()
            b3 = k3[:, :, 1:2].repeat(1, 1, self.tout)
            b3[:, :, 0], b3[:, :, -1] = k3[:, :, 0], k3[:, :, 2]
            z = z + b3
            extra += k3[:, :, 1:2].abs()
            extra[:, :, 0] += k3[:, :, 0].abs() + k3[:, :, 1].abs()
            extra[:, :, -1] += k3[:, :, 2].abs() + k3[:, :, 1].abs()
        if self.res is not None:
            z = z + self.res.double()
            extra += self.res.double().abs()
        if self.post == 2:      # forward value tanh(z); the backward pass the product runs: dz = dy * (1 - y_stored^2)
            self.act = 1.0 - y.double() ** 2
            self.y_tanh = torch.tanh(z.detach())
        else:
            self.act = torch.where(y > 0, 1.0, SLOPE).double() if self.post else torch.ones_like(z)      # out_scale > 0 and no add with post
        yr = self.out_scale * z * self.act
        if self.add_y is not None:
            yr = yr + self.add_y.double()
        (yr * self.cot.double()).sum().backward()
        dy_eff = (self.cot.double() * self.out_scale * self.act).abs()
        ha = (H if self.film else F.leaky_relu(xr.detach(), SLOPE) if self.pre else xr.detach()).abs().requires_grad_(True)
        wa = self.w.double().abs().requires_grad_(True)
        za = _conv64(ha, wa[:, self.win], None, self.geom)
        (za * dy_eff).sum().backward()
        self.ref = dict(y=self.y_tanh if self.post == 2 else yr.detach(),
                        dx=xr.grad + (self.add_scale * self.add_x.double() if self.add_x is not None else 0),
                        dw=self.dw0.double() + wr.grad, db=self.db0.double() + (br.grad if self.has_bias else 0))
        self.A = dict(y=self.out_scale * (za.detach() + extra), dx=ha.grad, dw=wa.grad, db=dy_eff.sum((0, 2)))
        if self.film:      # dh = g m (1 + gamma), dgamma = g m h, dbeta = g m with g = W^T dy and the mask m <= 1
            gam = self.gb.double()[:, :self.cin].abs()
            self.ref['dgb'], self.n['dgb'] = gbr.grad, self.n['dx']
            self.A['dgb'] = torch.cat([ha.grad * self.x.double().abs(), ha.grad], 1)
            self.A['dx'] = ha.grad * (1 + gam)
        assert _spare_intact(self.y_whole, self.cout), 'forward wrote into the spare channels behind y'
        if self.bits_v is not None:
            from test_film_cond_bwd_edges_gpu import pack_sign_bits
            words = self.bits_v.cpu()
            assert torch.equal(words, pack_sign_bits(y)), f'{int((words != pack_sign_bits(y)).sum())} sign words differ from (stored y > 0)'
            assert _spare_intact(self.bits_whole.view(torch.float32), self.cout), 'forward wrote into the spare channels behind the sign words'
        return self._bars('y', self.yv)

    def film_H(self):
        gb = self.gb.double()
        return self.x.double().abs() * (1 + gb[:, :self.cin].abs()) + gb[:, self.cin:].abs()

    def assert_off_kink(self):
        """CPU only. The seeded data of a FiLM case holds no element within 3 * 2^-23 * H of the LeakyReLU kink (the other prologues
        take their masks from stored fp32 values: exact on both sides)."""
        if self.film:
            gb = self.gb.double()
            h2 = self.x.double() * (1 + gb[:, :self.cin]) + gb[:, self.cin:]
            assert bool((h2.abs() > 3 * U * self.film_H()).all()), 'an element of the seeded data sits on the LeakyReLU kink: reseed the case'

    def dy_xf(self):
        ops, L, _ = _mods()
        if self.post == 2:
            return ops._xf(L.XF_MASK_TANH, scale=self.out_scale, aux=self.yv)
        return ops._xf(L.XF_MASK_LRELU, scale=self.out_scale, aux=self.yv) if self.post else ops._xf(scale=self.out_scale)

    def dgrad(self, x_bits=None):
        """x_bits: sign words of x standing in for x_in (pre = 1 only)."""
        ops, L, _ = _mods()
        if x_bits is not None:
            assert self.pre and not self.film
            self._call('dgrad', lambda: ops.conv_dgrad_raw(self.spec, self.dyv, self.dy_xf(), self.T, L.DG_MASK_LRELU, x_in=None, x_bits=x_bits,
                                                            add=self.addx_v, add_scale=self.add_scale, out=self.dxv))
            assert _spare_intact(self.dx_whole, self.cin), 'input-grad wrote into the spare channels behind dx'
            return self._bars('dx', self.dxv)
        if self.film:
            self._call('dgrad', lambda: ops.conv_dgrad_raw(self.spec, self.dyv, self.dy_xf(), self.T, L.DG_FILM, x_in=self.xv, gb=self.gbv, dgb=self.dgbv,
                                                            add=self.addx_v, add_scale=self.add_scale, out=self.dxv))
            assert _spare_intact(self.dx_whole, self.cin) and _spare_intact(self.dgb_whole, 2 * self.cin), 'input-grad wrote outside dx / dgb'
            out = self._bars('dx', self.dxv)
            out.update(self._bars('dgb', self.dgbv))
            return out
        self._call('dgrad', lambda: ops.conv_dgrad_raw(self.spec, self.dyv, self.dy_xf(), self.T, L.DG_MASK_LRELU if self.pre else L.DG_PLAIN,
                                                        x_in=self.xv if self.pre else None, add=self.addx_v, add_scale=self.add_scale, out=self.dxv))
        assert _spare_intact(self.dx_whole, self.cin), 'input-grad wrote into the spare channels behind dx'
        return self._bars('dx', self.dxv)

    def wgrad_call(self, ws_bytes=None, with_dw=True, region=None):
        """tdvc_conv_wgrad through ctypes -> (rc, kernel names). The workspace is exactly `ws_bytes` (default: the queried size)
        inside a larger SENT-filled buffer; self.guard_ok says whether the bytes around the region are still SENT afterwards."""
        ops, L, _ = _mods()
        lib = L.lib()
        d = self.spec.desc(self.B, self.T)
        self.query = lib.tdvc_conv_wgrad_workspace(C.byref(d))
        assert self.query % 4 == 0
        nbytes = self.query if ws_bytes is None else ws_bytes
        lead = 64                                                   # floats in front of the region (keeps it 256-byte aligned)
        guard = torch.full((lead + self.query // 4 + 64,), SENT, dtype=torch.float32, device=self.dev)
        dyx = self.dy_xf()
        a = L.ConvWgradArgs(self.xv.data_ptr(), self.xv.stride(0), self.x_xf, self.dyv.data_ptr(), self.dyv.stride(0), dyx,
                            self.dw.data_ptr() if with_dw else None, self.db.data_ptr() if self.with_db else None, guard.data_ptr() + 4 * lead if nbytes else None, nbytes)
        st = torch.cuda.current_stream(self.dev).cuda_stream

        def run():
            rc = lib.tdvc_conv_wgrad(C.byref(d), C.byref(a), st)
            L.check(lib.tdvc_fold_flush(st))      # other tests of the process may have left deferral on
            return rc
        rc = self._call('wgrad', run)
        g = guard.cpu()
        self.guard_ok = bool((g[:lead] == SENT).all() and (g[lead + (nbytes + 3) // 4:] == SENT).all())
        return rc

    def wgrad(self):
        rc = self.wgrad_call()
        assert rc == 0, (rc, _mods()[1].lib().tdvc_last_error())
        assert self.guard_ok, f'weight-grad wrote outside its {self.query}-byte workspace'
        out = self._bars('dw', self.dw)
        if not self.with_db:      # dbias = NULL: the bias gradient buffer must not be touched
            assert torch.equal(self.db.cpu(), self.db0), 'dbias = NULL, but the bias gradient buffer was written'
            assert 'conv_bias_grad_kernel' not in self.names['wgrad'], sorted(self.names['wgrad'])
            return out
        out.update(self._bars('db', self.db))
        return out

    def _bars(self, key, got):
        if key == 'y' and self.post == 2:      # the summation bound of z carries over (|tanh'| <= 1), plus the absolute tanhf allowance
            g, ref = got.detach().cpu(), self.ref['y']
            bound = (self.n['y'] + self.slack) * U * self.A['y'] + 2.0 ** -22 * ref.abs() + self.tanh_allow * 2.0 ** -24
            ratio = float(((g.double() - ref).abs() / bound).max()) if bool(torch.isfinite(g).all()) else float('nan')
            return {key: dict(rel=rel_l2(got, ref), ratio=ratio, inexact=0)}
        ratio, inexact = elem_check(got, self.ref[key], self.A[key], self.n[key], self.slack)
        return {key: dict(rel=rel_l2(got, self.ref[key]), ratio=ratio, inexact=inexact)}

    def run_all(self):
        res = self.fwd()
        res.update(self.dgrad())
        res.update(self.wgrad())
        return res


def make_edge(name, dev, generic=0):
    geom = LEAN_GEOM if name == LEAN_GEOM[0] else GEOM[name]
    return Edge(geom, dev, generic, **OPTS[name])


def assert_bars(res, what):
    print(f'[edge] {what}: ' + '  '.join(f'{k}: rel {v["rel"]:.2e} err/bound {v["ratio"]:.3f}' for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not (v['rel'] < TOL and v['ratio'] <= 1.0 and v['inexact'] == 0)}
    assert not bad, (what, bad)


def _small_group_desc(geom):
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
    return not transposed and g >= 16 and cin == 4 * g and cout == 4 * g and d == 1 and not reflect and 2 <= s <= 8 and k <= 48


def expected_families(name, generic, e):
    """Kernel name prefixes the three calls of a case must have launched (mirrors the route planning of conv_api.hip)."""
    geom = e.geom
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
    if transposed:
        modes = (MODE_UP, MODE_DOWN)
    else:
        modes = (MODE_DIRECT, MODE_DIRECT) if s == 1 else (MODE_DOWN, MODE_UP)
    if generic:
        return f'conv_scalar_kernel<{modes[0]}>', f'conv_scalar_kernel<{modes[1]}>', 'conv_wgrad_scalar_kernel<'
    if _small_group_desc(geom):
        fwd, dg = f'small_group_fwd_kernel<{s}>', f'small_group_dgrad_kernel<{s}>'
    else:
        fwd, dg = f'conv_gemm_kernel<{modes[0]},', f'conv_gemm_kernel<{modes[1]},'
    J = k if s == 1 else -(-k // s)
    tout = e.tout
    if _small_group_desc(geom) and 4 * k <= 252 and 4 * (T + 2 * p + s) <= 6 * 256 and 4 * tout <= 256:
        wg = 'small_group_wgrad_kernel'
    elif not transposed and s == 1 and g == 1 and T == tout and (tout > 128 or (cin >= 32 and cout >= 32)) and \
            ((k in (1, 5) and d == 1) or (k in (3, 7, 11) and d in (1, 3, 5))):
        wg = 'conv_wgrad_'      # the stride-1 'same' weight-grad kernels (lean / tile / pipe / x6) take any sequence length
    else:
        wg = f'conv_wgrad_kernel<{MODE_DIRECT if s == 1 else MODE_DOWN},' if J in WGRAD_MFMA_J else 'conv_wgrad_scalar_kernel<'
    return fwd, dg, wg


def assert_families(e, name, generic):
    for what, prefix in zip(('fwd', 'dgrad', 'wgrad'), expected_families(name, generic, e)):
        assert any(n.startswith(prefix) for n in e.names[what]), (name, what, prefix, sorted(e.names[what]))
        if prefix == 'conv_wgrad_':
            assert not any(n.startswith(('conv_wgrad_kernel<', 'conv_wgrad_scalar_kernel<')) for n in e.names[what]), sorted(e.names[what])
    lean = [n for ns in e.names.values() for n in ns if n.startswith('conv_lean_kernel')]
    assert not lean, (name, lean)


@pytest.mark.parametrize('generic', [0, 1], ids=['mfma', 'scalar'])
@pytest.mark.parametrize('name', list(GEOM))
def test_edge_geometry(name, generic, dev):
    """Every edge geometry on the automatic route and on the scalar kernels (tdvc_set_force_generic), both bars on y, dx, dw, db."""
    e = make_edge(name, dev, generic)
    res = e.run_all()
    assert_bars(res, f'{name} {"scalar" if generic else "mfma"}')
    assert_families(e, name, generic)
    if name == 'down_k7_s2':      # J = 4 has no MFMA weight-grad instance
        assert any(n.startswith('conv_wgrad_scalar_kernel<1>') for n in e.names['wgrad']), sorted(e.names['wgrad'])
    if name == 'direct_reflect_T333' and not generic:      # the mirror fold of the MFMA kernel, not of the lean or the scalar one
        assert any(n.startswith('conv_gemm_kernel<0,') for n in e.names['dgrad']), sorted(e.names['dgrad'])
    # the positions the bound demands exact values at are really there
    if name in ('down_r5', 'down_k3_s4'):
        assert int((e.A['dx'] == 0).sum()) >= (e.B * e.cin if name == 'down_r5' else e.B * e.cin * (e.T // 4))
    if name == 'up_k3_s4':
        holes = e.A['y'] == 0
        assert int(holes.sum()) == e.B * e.cout * (e.tout - 3 * e.T)      # every sample no 3-tap window writes, the out_pad tail included
        assert torch.equal(e.yv.cpu()[holes], e.b[None, :, None].expand_as(holes)[holes]), 'holes must hold the bias bit for bit'
    if name == 'window_generic':
        outside = torch.ones(14, dtype=torch.bool); outside[5:13] = False
        assert torch.equal(e.dw.cpu()[:, outside], e.dw0[:, outside]), 'dw columns outside the w_cin window were touched'


FORCED_CASES = ['down_r5', 'down_s16_c2', 'grp3', 'up_r5', 'up_k3_s4', 'up_grp3', 'direct_valid_k5', 'direct_reflect_T333']


@pytest.mark.parametrize('name', FORCED_CASES)
@pytest.mark.parametrize('cfg', sorted(GEMM_CFG), ids=[f'tile{c}_' + 'x'.join(map(str, GEMM_CFG[c])) for c in sorted(GEMM_CFG)])
def test_forced_gemm_tile(cfg, name, dev):
    """Every tile of the generic MFMA kernel (tdvc_debug_force_gemm_tile), forward and input-grad, at shapes where rows, columns and
    reduction are ragged against it, with NaN-poisoned LDS: a tile that reads LDS words it never staged turns them into NaN."""
    L = _mods()[1]
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
    L.lib().tdvc_debug_force_gemm_tile(cfg)
    try:
        e = make_edge(name, dev, 0)
        res = e.fwd()
        res.update(e.dgrad())
    finally:
        L.lib().tdvc_debug_force_gemm_tile(-1)
    assert_bars(res, f'{name} tile{cfg}')
    fwd, dg, _ = expected_families(name, 0, e)
    inst = ','.join(map(str, GEMM_CFG[cfg])) + ','
    for what, prefix in (('fwd', fwd + inst), ('dgrad', dg + inst)):
        assert any(n.startswith(prefix) for n in e.names[what]), (what, prefix, sorted(e.names[what]))


def test_dgrad_refuses_pad_beyond_field(dev):
    """pad = 3 on a 3-tap conv: the input-grad would need a negative padding. TDVC_EUNSUPPORTED, nothing launched, dx untouched."""
    L = _mods()[1]
    e = Edge(('direct_pad_gt_field', 8, 8, 3, 1, 3, 1, 1, False, False, 0, 100), dev, pre=1)
    assert_bars(e.fwd(), 'direct_pad_gt_field forward')
    with pytest.raises(L.TdvcError, match=rf'\({EUNSUPPORTED}\)'):
        e.dgrad()
    torch.cuda.synchronize()
    assert not e.names.get('dgrad'), e.names
    assert bool((e.dxv == SENT).all())


FILM_GENERIC = [(16, 3, 1, 333, True, True), (32, 7, 3, 203, True, False)]


@pytest.mark.parametrize('cfg', FILM_GENERIC, ids=['c16k3_T333', 'c32k7d3_T203'])
def test_film_block_on_generic_route(cfg, dev):
    """The FiLM prologue (forward) and the FiLM epilogue (input-grad) of the generic kernels: T % 4 != 0 keeps the block off the lean
    and the fused kernels."""
    with traced() as tr:
        errs = OPS.film_block_errors(cfg, dev, B=2)
    assert max(errs.values()) < OPS.TOL, errs
    off_route = [n for n in tr.names if n.startswith(('conv_lean_kernel', 'film_block_fwd_kernel'))]
    assert not off_route and any(n.startswith('conv_gemm_kernel<0,') for n in tr.names), sorted(tr.names)


@pytest.mark.parametrize('name', ['down_r5', 'up_r5', 'grp3', 'sg_g16_k48_s8', 'sg_g16_k41_T250', LEAN_GEOM[0]])
def test_wgrad_workspace_contract(name, dev):
    """One byte less than tdvc_conv_wgrad_workspace() is refused with TDVC_EWORKSPACE, nothing launched, dw / dbias bit-identical.
    The small-group launcher declines instead: where the next route needs no more than what is there, its result must be right.
    dw = NULL with dbias given produces the bias gradient alone."""
    L = _mods()[1]
    if name == 'sg_g16_k41_T250':      # inside the small-group weight-grad's contract (Tout <= 64): its launcher sees the short workspace
        e = Edge(('sg_g16_k41_T250', 64, 64, 41, 4, 20, 1, 16, False, False, 0, 250), dev, post=1)
    else:
        e = make_edge(name, dev)
    e.fwd()
    rc = e.wgrad_call(ws_bytes=-1 + L.lib().tdvc_conv_wgrad_workspace(C.byref(e.spec.desc(e.B, e.T))))
    torch.cuda.synchronize()
    assert e.query > 0 and e.guard_ok
    if rc == 0:      # the small-group slabs are smaller than those of the route behind it, or that route needs none
        assert _small_group_desc(e.geom), 'only the small-group launcher may decline a short workspace'
        res = e._bars('dw', e.dw); res.update(e._bars('db', e.db))
        assert_bars(res, f'{name} fall-through')
        if name == 'sg_g16_k41_T250':      # one byte less than the small-group slabs (nsplit = 1: [G][16][K] weights + [G][4] bias partials)
            assert any(n.startswith('small_group_wgrad_kernel') for n in e.names['wgrad']), sorted(e.names['wgrad'])
            e.dw.copy_(e.dw0); e.db.copy_(e.db0)
            rc = e.wgrad_call(ws_bytes=4 * (16 * 16 * 41 + 16 * 4) - 1)
            torch.cuda.synchronize()
            assert rc == EWORKSPACE and not e.names['wgrad'] and e.guard_ok, (rc, sorted(e.names['wgrad']))
            assert torch.equal(e.dw.cpu(), e.dw0) and torch.equal(e.db.cpu(), e.db0)
    else:
        assert rc == EWORKSPACE, (rc, L.lib().tdvc_last_error())
        assert not e.names['wgrad'], sorted(e.names['wgrad'])
        assert torch.equal(e.dw.cpu(), e.dw0) and torch.equal(e.db.cpu(), e.db0)
    # dbias alone
    e.dw.copy_(e.dw0); e.db.copy_(e.db0)
    rc = e.wgrad_call(with_dw=False)
    torch.cuda.synchronize()
    assert rc == 0 and e.guard_ok, (rc, L.lib().tdvc_last_error())
    assert torch.equal(e.dw.cpu(), e.dw0), 'dw = NULL: the weight gradient buffer of the layer must not be written'
    assert_bars(e._bars('db', e.db), f'{name} dbias alone')
    assert e.names['wgrad'] == {'conv_bias_grad_kernel'}, sorted(e.names['wgrad'])


# ------------------------------------------------------------------------------------------------ deferred folds
# (name, cin, cout, K, stride, pad, dil, groups, reflect, transposed, out_pad, T), B, (w_cin, w_cin_off), has bias
FOLD_LAYERS = [
    (('mfma_r3', 20, 36, 6, 3, 2, 1, 1, False, False, 0, 130), 3, (0, 0), True),            # slabs without bias partials; bias-grad kernel
    (('lean_c32_k3', 32, 32, 3, 1, 1, 1, 1, False, False, 0, 256), 3, (0, 0), True),        # bias partials behind the weights
    (('multitile', 16, 32, 4, 2, 1, 1, 1, False, False, 0, 2210), 2, (0, 0), True),         # nslab = 10 > 8: split and re-folded
    (('win_lo', 8, 24, 3, 1, 1, 1, 1, False, False, 0, 333), 3, (16, 0), True),             # window pair: disjoint columns of one dw
    (('win_hi', 8, 24, 3, 1, 1, 1, 1, False, False, 0, 333), 3, (16, 8), False),
    (('small_group', 64, 64, 41, 4, 20, 1, 16, False, False, 0, 250), 8, (0, 0), True),     # small-group route, 4 slabs
    (('lean_reflect', 16, 16, 7, 1, 9, 3, 1, True, False, 0, 260), 3, (0, 0), True),
]
FOLD_COPIES = 4


def _fold_fixture(dev):
    """Inputs, float64 gradients and their absolute-value twins of every fold layer, computed once."""
    ops, L, arena = _mods()
    layers = []
    for geom, B, (w_cin, w_off), has_bias in FOLD_LAYERS:
        (name, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        spec = ops.ConvSpec(cin, cout, k, s, p, d, g, reflect, transposed, out_pad, w_cin, w_off)
        x, dy = torch.randn(B, cin, T, generator=gen).float(), torch.randn(B, cout, spec.tout(T), generator=gen).float()
        wshape = (cout, (w_cin or cin) // g, k)
        win = slice(w_off, w_off + cin) if w_cin else slice(None)
        grads = []
        for xx, dd in ((x.double(), dy.double()), (x.double().abs(), dy.double().abs())):
            w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
            (_conv64(xx, w[:, win], None, geom) * dd).sum().backward()
            grads.append((w.grad, dd.sum((0, 2))))
        layers.append(dict(name=name, spec=spec, B=B, T=T, x=x.to(dev), dy=dy.to(dev), wshape=wshape, cout=cout, has_bias=has_bias,
                           g=grads[0], A=grads[1], n=B * spec.tout(T)))
    return layers


def _fold_sequence(layers, bufs, dev, trace_into=None):
    """The 30 weight-grad calls. mfma_r3 twice on the same dw / dbias: the second call finds the first one's fold queued (clash on dw).
    lean_c32_k3 twice on the same dbias but a dw of its own each (clash on dbias only). Then every other (layer, copy) once, each on
    gradient buffers of its own: 26 folds behind the one still queued, so the queue fills up (24) and overflows once. One private
    workspace region per call, one flush at the end. -> how often each gradient buffer was used."""
    ops, L, _ = _mods()
    lib = L.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    calls = [(0, 0, 0), (0, 0, 0), (1, 0, 0), (1, FOLD_COPIES, 0)] + [(li, 0, 0) for li in range(2, len(layers))] + \
            [(li, c, c) for c in range(1, FOLD_COPIES) for li in range(len(layers))]      # (layer, copy of dw, copy of dbias)
    descs = [l['spec'].desc(l['B'], l['T']) for l in layers]
    need = [lib.tdvc_conv_wgrad_workspace(C.byref(d)) for d in descs]
    offs, total = [], 0
    for li, _, _ in calls:
        offs.append(total); total += (need[li] + 255) & ~255
    ws = torch.zeros(total + 256, dtype=torch.uint8, device=dev)
    uses = {}
    for (li, cw, cb), off in zip(calls, offs):
        l = layers[li]
        win_pair = l['name'] in ('win_lo', 'win_hi')
        dw = bufs['dw'][(3 if win_pair else li, cw)]      # the window pair shares one dw
        db = bufs['db'][(li, cb)] if l['has_bias'] else None
        a = L.ConvWgradArgs(l['x'].data_ptr(), l['x'].stride(0), ops._xf(), l['dy'].data_ptr(), l['dy'].stride(0), ops._xf(),
                            dw.data_ptr(), db.data_ptr() if db is not None else None, ws.data_ptr() + off if need[li] else None, need[li])
        L.check(lib.tdvc_conv_wgrad(C.byref(descs[li]), C.byref(a), st))
        uses[('dw', li, cw)] = uses.get(('dw', li, cw), 0) + 1
        if db is not None:
            uses[('db', li, cb)] = uses.get(('db', li, cb), 0) + 1
    L.check(lib.tdvc_fold_flush(st))
    torch.cuda.synchronize()
    return uses, len(calls)


def test_deferred_folds_match_immediate(dev):
    """The train step's fold path at op level: the same ~30 weight-grad calls with tdvc_fold_defer(0) and (1). Deferred, more than 24
    folds queue up (one overflow flush), two calls clash with a gradient whose fold is still queued (dw; dbias only), one fold is
    split over its slabs and re-folded, a window pair writes disjoint columns of one dw, two routes carry bias partials behind the weights. The
    folds sum in a fixed order: every dw / dbias is bit-identical between the two runs, and within both bars of float64."""
    ops, L, _ = _mods()
    lib = L.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    layers = _fold_fixture(dev)
    gen = torch.Generator().manual_seed(11)
    init = dict(dw={(li, c): torch.randn(l['wshape'], generator=gen).float() for li, l in enumerate(layers) for c in range(FOLD_COPIES + 1)},
                db={(li, c): torch.randn(l['cout'], generator=gen).float() for li, l in enumerate(layers) for c in range(FOLD_COPIES + 1)})
    L.check(lib.tdvc_fold_flush(st))
    out, names = {}, {}
    try:
        for defer in (0, 1):
            bufs = {k: {i: t.to(dev) for i, t in v.items()} for k, v in init.items()}
            lib.tdvc_fold_defer(defer)
            with traced() as tr:
                uses, ncalls = _fold_sequence(layers, bufs, dev)
            out[defer], names[defer] = bufs, tr.names
        assert ncalls == 30
        assert 'slab_reduce_multi_kernel' in names[1] and 'small_group_wgrad_kernel' in names[1], sorted(names[1])
        assert any(n.startswith('conv_wgrad_kernel<1,') for n in names[1]) and any(n.startswith('conv_wgrad_lean_kernel') for n in names[1]), sorted(names[1])
        res = {}
        for (kind, li, c), cnt in uses.items():
            l = layers[li]
            key = (3 if kind == 'dw' and l['name'] == 'win_hi' else li, c)
            a_, b_ = out[0][kind][key], out[1][kind][key]
            assert torch.equal(a_, b_), (kind, l['name'], c, float((a_ - b_).abs().max()))
            if kind == 'dw' and l['name'] in ('win_lo', 'win_hi'):      # the pair's shared dw: both windows' gradients
                g = layers[3]['g'][0] + layers[4]['g'][0]; A = layers[3]['A'][0] + layers[4]['A'][0]
            else:
                g, A = l['g'][0 if kind == 'dw' else 1] * cnt, l['A'][0 if kind == 'dw' else 1] * cnt
            ref = init[kind][key].double() + g
            ratio, inexact = elem_check(b_, ref, A, l['n'] * cnt)
            res[f'{kind}:{l["name"]}:{c}'] = dict(rel=rel_l2(b_, ref), ratio=ratio, inexact=inexact)
        worst = max(res.items(), key=lambda kv: kv[1]['ratio'])
        print(f'[edge] deferred folds: {len(res)} gradients, worst err/bound {worst[1]["ratio"]:.3f} ({worst[0]})')
        bad = {k: v for k, v in res.items() if not (v['rel'] < TOL and v['ratio'] <= 1.0 and v['inexact'] == 0)}
        assert not bad, bad
        # untouched buffers (the spare copy of the layers that were not used a fifth time) are still what they were
        for li, l in enumerate(layers):
            if li != 1:
                assert torch.equal(out[1]['dw'][(li, FOLD_COPIES)].cpu(), init['dw'][(li, FOLD_COPIES)])
        # tdvc_fold_reset after queueing: the queued fold never runs
        l = layers[1]
        lib.tdvc_fold_defer(1)
        dw, db = init['dw'][(1, 0)].to(dev), init['db'][(1, 0)].to(dev)
        d = l['spec'].desc(l['B'], l['T'])
        need = lib.tdvc_conv_wgrad_workspace(C.byref(d))
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        a = L.ConvWgradArgs(l['x'].data_ptr(), l['x'].stride(0), ops._xf(), l['dy'].data_ptr(), l['dy'].stride(0), ops._xf(),
                            dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need)
        L.check(lib.tdvc_conv_wgrad(C.byref(d), C.byref(a), st))
        lib.tdvc_fold_reset(st)
        L.check(lib.tdvc_fold_flush(st))
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu(), init['dw'][(1, 0)]) and torch.equal(db.cpu(), init['db'][(1, 0)]), 'a reset fold was still added'
    finally:
        lib.tdvc_fold_reset(st)
        lib.tdvc_fold_defer(1 if ops.FOLD_DEFER else 0)
