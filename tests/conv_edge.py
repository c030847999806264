"""The Edge class the float64 edge suites of the conv kernels drive (generic, lean, lean weight-grad, group16, small-group, split-bf16),
with the float64 operation it checks against and the helpers built on it. The rules are in the docstring of
test_generic_conv_edges_gpu.py; edge_support.py holds the bars and the guarded buffers."""
import ctypes as C

import torch
import torch.nn.functional as F

from common import rel_l2, traced
from edge_support import SENT, SLOPE, U, _buf, _spare_intact, elem_check, mods, pack_sign_bits


def _g(name, cin, cout, k, pad, dil, reflect, T):
    """Edge's geometry tuple of a stride-1 conv."""
    return (name, cin, cout, k, 1, pad, dil, 1, reflect, False, 0, T)


def _conv64(h, w, b, geom):
    """The float64 operation of one geometry on an already pre-activated input."""
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
    if transposed:
        return F.conv_transpose1d(h, w, b, stride=s, padding=p, output_padding=out_pad, groups=g)
    if reflect and p > 0:
        return F.conv1d(F.pad(h, (p, p), mode='reflect'), w, b, stride=s, dilation=d, groups=g)
    return F.conv1d(h, w, b, stride=s, padding=p, dilation=d, groups=g)


class Edge:
    """One conv geometry through tdvc_conv_fwd / _dgrad / _wgrad against float64 CPU autograd (the docstring of
    test_generic_conv_edges_gpu.py has the rules).
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
        ops, L, arena = mods()
        (name, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = geom
        assert not (add and post), 'the backward mask of a post-activated layer is its stored output: no running sum on top'
        self.geom, self.dev, self.generic, self.B, self.pre, self.post, self.views = geom, dev, generic, B, pre, post, views
        self.cin, self.cout, self.T = cin, cout, T
        self.with_db, self.film, self.unaligned, self.slack = with_db, film, unaligned, 12 if film else 8
        self.has_bias, self.tanh_allow = bias, tanh_allow
        assert not film or not pre, 'FiLM stands in place of the plain LeakyReLU'
        assert post in (0, 1, 2) and not (post == 2 and (add or res)), f'{name}: post = {post} with add = {add}, res = {res}: tanh takes neither'
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
            assert x_src.shape == self.x.shape and x_src.dtype == torch.float32, \
                f'{name}: x_src is {tuple(x_src.shape)} {x_src.dtype}, the case wants {tuple(self.x.shape)} float32'
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
            assert self.tout % 32 == 0, f'{name}: sign words need Tout % 32 == 0, Tout = {self.tout}'
            self.bits_whole = torch.full((B, cout + (3 if vw('bits') else 0), self.tout // 32), SENT, dtype=torch.float32, device=dev).view(torch.int32)
            self.bits_v = self.bits_whole[:, :cout]
        self.x_xf = ops._xf(L.XF_LRELU if pre else L.XF_NONE)
        if film:
            self.gbv = _buf(B, 2 * cin, T, dev, vw('gb'), self.gb, unaligned, nanf)[1]
            self.dgb_whole, self.dgbv = _buf(B, 2 * cin, T, dev, vw('dgb'), None, unaligned)
            self.x_xf = ops._xf(L.XF_FILM_LRELU, aux=self.gbv)
        self.names = {}

    def _call(self, what, fn):
        L = mods()[1]
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
        ops, L, _ = mods()
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
        ops, L, _ = mods()
        if self.post == 2:
            return ops._xf(L.XF_MASK_TANH, scale=self.out_scale, aux=self.yv)
        return ops._xf(L.XF_MASK_LRELU, scale=self.out_scale, aux=self.yv) if self.post else ops._xf(scale=self.out_scale)

    def dgrad(self, x_bits=None):
        """x_bits: sign words of x standing in for x_in (pre = 1 only)."""
        ops, L, _ = mods()
        if x_bits is not None:
            assert self.pre and not self.film, f'{self.geom[0]}: x_bits stand in for a plain LeakyReLU mask: pre = {self.pre}, film = {self.film}'
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
        ops, L, _ = mods()
        lib = L.lib()
        d = self.spec.desc(self.B, self.T)
        self.query = lib.tdvc_conv_wgrad_workspace(C.byref(d))
        assert self.query % 4 == 0, f'{self.geom[0]}: the workspace query {self.query} is no whole number of floats'
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
        assert rc == 0, (rc, mods()[1].lib().tdvc_last_error())
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


def plain_dgrad(e, masked):
    """tdvc_conv_dgrad with the PLAIN epilogue and dy_xf NONE / MASK_LRELU (aux = the stored forward output) -> (bars, kernel names)."""
    ops, L, _ = mods()
    (_, cin, cout, k, s, p, d, g, _, _, _, T) = e.geom
    xf = ops._xf(L.XF_MASK_LRELU, scale=e.out_scale, aux=e.yv) if masked else ops._xf(scale=e.out_scale)
    e.dxv.fill_(SENT)
    with traced() as tr:
        ops.conv_dgrad_raw(e.spec, e.dyv, xf, T, L.DG_PLAIN, out=e.dxv)
    assert _spare_intact(e.dx_whole, cin), 'input-grad wrote into the spare channels behind dx'
    dyp = e.cot.double() * e.out_scale
    if masked:
        dyp = dyp * torch.where(e.yv.detach().cpu() > 0, 1.0, SLOPE).double()
    out_pad = T - ((e.tout - 1) * s - 2 * p + k)
    ref = F.conv_transpose1d(dyp, e.w.double(), None, stride=s, padding=p, output_padding=out_pad, groups=g)
    A = F.conv_transpose1d(dyp.abs(), e.w.double().abs(), None, stride=s, padding=p, output_padding=out_pad, groups=g)
    ratio, inexact = elem_check(e.dxv, ref, A, cout // g * k)
    return {'dx_masked' if masked else 'dx': dict(rel=rel_l2(e.dxv, ref), ratio=ratio, inexact=inexact)}, tr.names


def tanh_excess(e):
    """Largest |y - tanh64(z)| beyond the propagated summation bound, in units of 2^-24 (0 where the bound already covers it)."""
    got, ref = e.yv.detach().cpu().double(), e.ref['y']
    prop = (e.n['y'] + e.slack) * U * e.A['y'] + 2.0 ** -22 * ref.abs()
    return max(0.0, float((((got - ref).abs() - prop) / 2.0 ** -24).max()))
