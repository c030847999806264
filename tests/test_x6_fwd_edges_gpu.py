"""Edge shapes of the split-bf16 FORWARD kernels against float64: conv_fwd_x6_kernel<2|4>, film_cond_fwd_x6_kernel<2|4> and
conv_x6_weight_planes_kernel (conv_fwd_x6.hip), all through the C ABI (tdvc_conv_fwd_x6, tdvc_film_cond_fwd_x6,
tdvc_conv_x6_weight_planes): the operator layer's gates (_x6_fwd_geometry, sign bits only at T >= 512, .contiguous()) hide most of
the contract.

Same rules as test_generic_conv_edges_gpu.py, with the helpers of edge_support.py: fp32-valued inputs, a float64 CPU reference on the same
numbers (the slope as float(np.float32(slope))), outputs that start as SENT and may be channel slices of wider buffers whose spare
channels stay SENT, inputs that may be channel slices of [B, C + 4, T] buffers whose spare channels are NaN (a masked-off channel
>= Cin read as a value turns the output NaN), the weight planes exactly tdvc_conv_x6_weight_planes_bytes inside a guarded buffer.
Every row asserts by trace the exact instance (<2> iff Cout % 64 != 0) and that nothing else was launched, and runs once more on
NaN-poisoned LDS.

1. Dense rows, both bars on every tensor: rel-L2 < 2e-5 and |got - ref| <= (n + 8) 2^-23 A + 2^-22 |ref|, exact where A == 0
   (n and A: FwdEdge, CondFwdEdge). Sign bits equal (stored cv0 > 0) bit for bit and differ from the reference's only where
   |cv_ref| <= its bound, element by element.
2. One product per output element: the bar on the x6 arithmetic itself, |got - ref| <= 2^-20 |ref| (test_x6_split_cpu.py has the
   derivation and asserts its figures). At dense shapes neither bar of part 1 notices a missing lo.hi product.
3. The weight-plane image, decoded with x6_split.plane_offsets.
4. Refusals: the return code, an empty trace, outputs and guards still SENT; built on buffers large enough for the refused geometry.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import rel_l2, traced
from conv_edge import Edge
from edge_support import (EINVAL, EUNSUPPORTED, SENT, U, Worst, _buf, _spare_intact, assert_bars, elem_check, mods, pack_sign_bits, poison_lds,
                          stream)
from x6_split import ONE_PRODUCT_BOUND, PLANE_GEOM, constructed, decode_planes, planes_bytes, split3

pytestmark = pytest.mark.gpu

NV = 8
GUARD16 = 0x5A5A                         # fills the int16 buffer around a plane image
BITS_SENT = 0x5A5A5A5A                   # fills a sign-word buffer before the call
SPECIALS = [0.0, -0.0, 2.0 ** -126]      # +0, -0, the smallest normal
WORST = Worst()                          # kernel -> tensor -> (err / bound, case)
_DATA = {}                               # case -> inputs and float64 references, computed once and never modified

# name, (Cin, Cout, T, B), options: slope (absent = no prologue), bias=False, views=True (x a slice of a NaN-padded buffer, y a slice of
# a SENT-padded one: both batch strides wider than contiguous). Tiles are 128 steps x (32 | 64) output channels, chunks 32 channels.
PLAIN = {c[0]: c for c in [
    # a one-channel third chunk; one <2> block; one tile, both halos outside the sequence
    ('c65_o32_T128', (65, 32, 128, 2), dict(slope=0.2)),
    # a one-channel fourth chunk; one <4> block; the second tile has 4 steps and only a left halo; no prologue
    ('c97_o64_T132', (97, 64, 132, 2), dict()),
    # three whole chunks; three <2> blocks; the second tile has 64 steps: wave half wt = 1 stores nothing
    ('c96_o96_T192', (96, 96, 192, 2), dict(slope=0.01)),
    # four whole chunks; two <4> blocks; a last tile of 124 steps; slope 1 is the identity
    ('c128_o128_T252', (128, 128, 252, 2), dict(slope=1.0)),
    # five whole chunks; five <2> blocks; the right halo of tile 0 inside, of tile 1 outside; bias = NULL
    ('c160_o160_T256_no_bias', (160, 160, 256, 2), dict(slope=0.2, bias=False)),
    # the workload's 136 (an 8-channel fifth chunk); four <4> blocks; three tiles, the last of 4 steps; every operand a view
    ('c136_o256_T260_views', (136, 256, 260, 3), dict(slope=0.2, views=True)),
    # the NaN channels 65 .. 68 sit inside the masked part of chunk 2; no prologue, no bias
    ('c65_o64_T256_views', (65, 64, 256, 3), dict(views=True, bias=False)),
    ('c97_o32_T260_views', (97, 32, 260, 2), dict(slope=0.2, views=True)),
]}
# name, (n_cond, C2, T, B), options: slope (0.2), b2=False, cv0=False (not stored), bits=True (sign words, T % 32 == 0), views=True (exc,
# gb, cv0 and the sign words all slices of wider buffers), zero_sample=True (the last sample has exc = 0 and k3 = 0).
FUSED = {c[0]: c for c in [
    # a 4-channel third chunk; one tile: k3[..., 0] and k3[..., 2] in the same tile; 4 words per channel
    ('nc68_C32_T128_bits', (68, 32, 128, 2), dict(bits=True)),
    # an 8-channel third chunk; the last tile holds one word
    ('nc72_C64_T160_bits_slope001', (72, 64, 160, 2), dict(bits=True, slope=0.01)),
    # three whole chunks; three output blocks, one of which writes cv0 and the bits; the last tile holds two words
    ('nc96_C96_T192_bits_zero_sample', (96, 96, 192, 3), dict(bits=True, zero_sample=True)),
    ('nc100_C128_T252_slope1', (100, 128, 252, 2), dict(slope=1.0)),
    ('nc136_C160_T256_bits_views', (136, 160, 256, 3), dict(bits=True, views=True)),
    # a 12-channel fifth chunk; the 4-step tile 2 holds T - 1 = 259 (k3[..., 2]), its left halo 255 and tile 1's right halo 256 take
    # k3[..., 1]; b2 = NULL. (T % 4 == 0 and tiles of 128: a halo step is never 0 or T - 1, so its bias is always the interior one.)
    ('nc140_C256_T260_no_b2', (140, 256, 260, 3), dict(b2=False)),
    # five whole chunks; k3[..., 0] and k3[..., 2] in different tiles, three samples with their own k3
    ('nc160_C32_T132', (160, 32, 132, 3), dict()),
    ('nc136_C32_T132_views', (136, 32, 132, 2), dict(views=True)),
    ('nc136_C64_T256_no_cv0_bits', (136, 64, 256, 2), dict(bits=True, cv0=False)),
    ('nc136_C64_T256_no_cv0', (136, 64, 256, 2), dict(cv0=False)),
]}
# not rows of the tables: the valid calls the refusal tests start from
PLAIN_BASE = ('plain_refusal_base', (136, 64, 160, 3), dict(slope=0.2, views=True, x_extra=32))
FUSED_BASE = ('fused_refusal_base', (136, 64, 160, 3), dict(bits=True, views=True))


def _f32(slope):
    return float(np.float32(slope))


def _lrelu64(v, slope):
    return v if slope is None else torch.where(v > 0, v, v * _f32(slope))


def _sprinkle(t, gen):
    """+0, -0 and the smallest normal at random places and along one whole row of sample 0."""
    flat = t.view(-1)
    idx = torch.randint(flat.numel(), (min(300, flat.numel() // 4),), generator=gen)
    flat[idx] = torch.tensor(SPECIALS).repeat(100)[:idx.numel()]
    t[0, 1, :] = torch.tensor(SPECIALS).repeat(t.shape[2] // 3 + 1)[:t.shape[2]]


def _nan_in(src, dev, view, extra=4):
    """An input operand: contiguous, or the slice [:, :C] of a [B, C + extra, T] buffer whose spare channels are NaN."""
    if not view:
        return src.to(dev).contiguous()
    B, Cc, T = src.shape
    whole = torch.full((B, Cc + extra, T), float('nan'), dtype=torch.float32, device=dev)
    whole[:, :Cc].copy_(src.to(dev))
    return whole[:, :Cc]


def make_planes(w_dev, Cout, Cin, dev):
    """tdvc_conv_x6_weight_planes into exactly the queried bytes of a GUARD16-filled int16 buffer -> (whole buffer, the image)."""
    L = mods()[1]
    lib = L.lib()
    nbytes = lib.tdvc_conv_x6_weight_planes_bytes(Cout, Cin, 3)
    assert nbytes == planes_bytes(Cout), (nbytes, planes_bytes(Cout))
    lead, n = 128, nbytes // 2           # 256 bytes in front: the image stays 256-byte aligned
    whole = torch.full((lead + n + 128,), GUARD16, dtype=torch.int16, device=dev)
    L.check(lib.tdvc_conv_x6_weight_planes(w_dev.data_ptr(), Cout, Cin, 3, whole.data_ptr() + 2 * lead, stream(dev)))
    g = whole.cpu()
    assert bool((g[:lead] == GUARD16).all() and (g[lead + n:] == GUARD16).all()), 'the planes kernel wrote outside the queried bytes'
    return whole, whole[lead:lead + n]


# ------------------------------------------------------------------------------------------------------------ plain forward
def plain_data(name):
    if name in _DATA:
        return _DATA[name]
    _, (Cin, Cout, T, B), o = PLAIN_BASE if name == PLAIN_BASE[0] else PLAIN[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *sh: torch.randn(*sh, generator=gen).float()
    d = dict(x=rnd(B, Cin, T), W=rnd(Cout, Cin, 3) / (3 * Cin) ** 0.5, bias=rnd(Cout) * 0.1 if o.get('bias', True) else None)
    _sprinkle(d['x'], gen)
    h = _lrelu64(d['x'].double(), o.get('slope'))
    b64 = d['bias'].double() if d['bias'] is not None else None
    d['ref'] = F.conv1d(h, d['W'].double(), b64, padding=1)
    d['A'] = F.conv1d(h.abs(), d['W'].double().abs(), b64.abs() if b64 is not None else None, padding=1)
    _DATA[name] = d
    return d


class FwdEdge:
    """One row through tdvc_conv_fwd_x6 against float64: y = bias + conv1d(x', W, padding=1), x' = LeakyReLU(x) or x.
    n = 3 Cin + 1 (the + 1 is the one rounding of x * slope), A = |bias| + conv1d(|x'|, |W|). The split-bf16 product keeps the bound
    of an fp32 dot product: three exact pieces per operand and six of the nine piece products leave at most about 2 * 2^-24 relative
    error per product, i.e. 2^-23 A in the sum, inside the slack of 8."""

    def __init__(self, name, dev, row=None, data=None):
        _, (Cin, Cout, T, B), o = row or (PLAIN_BASE if name == PLAIN_BASE[0] else PLAIN[name])
        self.name, self.dev, self.o, self.Cin, self.Cout, self.T, self.B = name, dev, o, Cin, Cout, T, B
        self.d = d = data or plain_data(name)
        self.slope, views = o.get('slope'), o.get('views', False)
        self.x = _nan_in(d['x'], dev, views, o.get('x_extra', 4))
        self.y_whole, self.y = _buf(B, Cout, T, dev, views)
        self.w = d['W'].to(dev).contiguous()
        self.bias = d['bias'].to(dev) if d['bias'] is not None else None
        self.planes_whole, self.planes = make_planes(self.w, Cout, Cin, dev)
        self.names = set()

    def kernel(self):
        return f'conv_fwd_x6_kernel<{2 if self.Cout % 64 else 4}>'

    def call(self, desc=None, args=None, planes='own'):
        """One call -> rc; `desc` / `args` replace fields of the two structs, `planes` the image pointer (the refusal tests)."""
        L = mods()[1]
        dd = dict(kind=L.CONV, B=self.B, Cin=self.Cin, Cout=self.Cout, Tin=self.T, Tout=self.T, K=3, stride=1, dilation=1, pad=1, groups=1,
                  reflect=0, w_cin=0, w_cin_off=0)
        dd.update(desc or {})
        xf = L.Xform(L.XF_NONE, 0.0, 1.0, None, 0) if self.slope is None else L.Xform(L.XF_LRELU, self.slope, 1.0, None, 0)
        aa = dict(x=self.x.data_ptr(), x_bs=self.x.stride(0), x_xf=xf, w=self.w.data_ptr(), bias=self.bias.data_ptr() if self.bias is not None else None,
                  res=None, res_bs=0, post_act=L.POST_NONE, post_slope=0.2, out_scale=1.0, add=None, add_bs=0, y=self.y.data_ptr(),
                  y_bs=self.y.stride(0), bias3=None, sign_bits=None, sign_bits_bs=0)
        aa.update(args or {})
        d_, a_ = L.ConvDesc(**dd), L.ConvFwdArgs(**aa)
        with traced() as tr:
            rc = L.lib().tdvc_conv_fwd_x6(C.byref(d_), C.byref(a_), self.planes.data_ptr() if isinstance(planes, str) else planes, stream(self.dev))
        self.names = tr.names
        return rc

    def run(self, tag=''):
        rc = self.call()
        assert rc == 0, (rc, mods()[1].lib().tdvc_last_error())
        assert self.names == {self.kernel()}, (self.name, sorted(self.names), self.kernel())
        ratio, inexact = elem_check(self.y, self.d['ref'], self.d['A'], 3 * self.Cin + 1)
        res = dict(y=dict(rel=rel_l2(self.y, self.d['ref']), ratio=ratio, inexact=inexact))
        assert_bars(res, f'{self.kernel()}: {self.name}{tag}')
        assert _spare_intact(self.y_whole, self.Cout), 'wrote into the spare channels behind y'
        WORST.note(self.kernel(), res, self.name)
        return res


@pytest.mark.parametrize('name', list(PLAIN))
def test_plain_edge(name, dev):
    """Every row of PLAIN: y within both bars, the exact instance by trace, the spare channels of a view still SENT."""
    FwdEdge(name, dev).run()


@pytest.mark.parametrize('name', list(PLAIN))
def test_plain_edge_poisoned_lds(name, dev):
    """Once more on NaN-poisoned LDS: the halo rows of a tile outside the sequence, the masked channels of a partial chunk and the
    weight rows of channels >= Cin must come from the kernel, not from what LDS held."""
    poison_lds(dev)
    e = FwdEdge(name, dev)
    e.run(' (poisoned LDS)')
    assert bool(torch.isfinite(e.y).all())


@pytest.mark.parametrize('slope', [None, 0.2], ids=['no_prologue', 'lrelu'])
def test_power_of_two_scaling(slope, dev):
    """bias = NULL: y(2^60 x) and y(2^-60 x) equal 2^+-60 y(x) bit for bit. A power-of-two scale commutes with every split, product and
    rounding of the scheme, so any absolute threshold in the kernel shows. |x| >= 0.5 and |W| >= 0.5 / sqrt(3 Cin) keep the smallest of the
    six piece products of the scaled-down run (2^-84 * 2^-6) clear of the denormal range."""
    row = ('scaling', (136, 32, 132, 2), dict(bias=False, **({} if slope is None else dict(slope=slope))))
    gen = torch.Generator().manual_seed(60)
    far = lambda *sh: (lambda r: torch.where(r < 0, r - 0.5, r + 0.5))(torch.randn(*sh, generator=gen).float())
    x, W = far(2, 136, 132), far(32, 136, 3) / 408 ** 0.5
    ys = {}
    for e2 in (0, 60, -60):
        e = FwdEdge(f'scaling 2^{e2}', dev, row=row, data=dict(x=x * 2.0 ** e2, W=W, bias=None))
        assert e.call() == 0 and e.names == {e.kernel()}
        ys[e2] = e.y.cpu()
    assert bool(torch.isfinite(ys[0]).all()) and float(ys[0].abs().min()) > 2.0 ** -40
    for e2 in (60, -60):
        want = ys[0] * 2.0 ** e2
        assert torch.equal(ys[e2], want), (e2, int((ys[e2] != want).sum()))


# ------------------------------------------------------------------------------------------------------------ fused forward
def fused_data(name):
    if name in _DATA:
        return _DATA[name]
    _, (nc, C2, T, B), o = FUSED_BASE if name == FUSED_BASE[0] else FUSED[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    rnd = lambda *sh: torch.randn(*sh, generator=gen).float()
    d = dict(exc=rnd(B, NV, T), W0=rnd(nc, nc, 3) / 24 ** 0.5, k3=rnd(B, nc, 3), W2=rnd(C2, nc, 3) / (3 * nc) ** 0.5,
             b2=rnd(C2) * 0.1 if o.get('b2', True) else None)
    _sprinkle(d['exc'], gen)
    if o.get('zero_sample'):
        d['exc'][B - 1] = 0.0
        d['k3'][B - 1] = 0.0
    d.update(cond_reference(d, o.get('slope', 0.2)))
    _DATA[name] = d
    return d


def cond_reference(d, slope):
    """float64 cv0, gb and their A of one data set (CondFwdEdge's docstring)."""
    B, nc, _ = d['k3'].shape
    T = d['exc'].shape[2]
    w0x = d['W0'][:, nc - NV:, :].double()
    kt = d['k3'].double()[:, :, 1:2].repeat(1, 1, T)      # the 3-valued bias: [..., 0] at t = 0, [..., 2] at t = T - 1
    kt[:, :, 0], kt[:, :, T - 1] = d['k3'].double()[:, :, 0], d['k3'].double()[:, :, 2]
    cv = F.conv1d(d['exc'].double(), w0x, padding=1) + kt
    A1 = F.conv1d(d['exc'].double().abs(), w0x.abs(), padding=1) + kt.abs()
    b64 = d['b2'].double() if d['b2'] is not None else None
    gb = F.conv1d(_lrelu64(cv, slope), d['W2'].double(), b64, padding=1)
    A = F.conv1d(A1, d['W2'].double().abs(), b64.abs() if b64 is not None else None, padding=1)
    return dict(ref=dict(cv0=cv, gb=gb), A=dict(cv0=A1, gb=A), n=dict(cv0=3 * NV + 1, gb=3 * nc + 3 * NV + 2))


class CondFwdEdge:
    """One row through tdvc_film_cond_fwd_x6 against float64:

        cv0[c][t] = k3[c][t == 0 | interior | t == T - 1] + sum_{ce < 8, j} W0[c][nc - 8 + ce][j] * exc[ce][t + j - 1]
        gb        = b2 + conv1d(LeakyReLU(cv0), W2, padding=1)

    cv0 is an fp32 sum of 24 products and one addition: n = 24 + 1, A1 = conv1d(|exc|, |W0x|) + |k3 value used at that t|. The second level
    computes sum w lrelu(cv^) from the GPU's own cv^: its own error is (3 nc + 1) 2^-24 sum |w| |lrelu cv^| (the + 1 is the rounding of
    cv^ * slope) and it inherits sum |w| |lrelu cv^ - lrelu cv0| <= sum |w| |cv^ - cv0| <= 25 2^-24 sum |w| A1: LeakyReLU with a slope in
    (0, 1] is 1-Lipschitz, so the first level's error passes through unamplified and an element that changes branch needs no
    special handling. Both are multiples of A = |b2| + conv1d(A1, |W2|) >= sum |w| |lrelu cv0|: n = 3 nc + 24 + 2, and the bound's 2^-23
    leaves a factor of two over the first-order term."""

    def __init__(self, name, dev, row=None, data=None, **over):
        _, (nc, C2, T, B), o = row or (FUSED_BASE if name == FUSED_BASE[0] else FUSED[name])
        o = {**o, **over}
        self.name, self.dev, self.o, self.nc, self.C2, self.T, self.B = name, dev, o, nc, C2, T, B
        self.d = d = data or fused_data(name)
        self.slope, views = o.get('slope', 0.2), o.get('views', False)
        self.exc = _nan_in(d['exc'], dev, views)
        self.gb_whole, self.gb = _buf(B, C2, T, dev, views)
        self.cv0_whole, self.cv0 = _buf(B, nc, T, dev, views) if o.get('cv0', True) else (None, None)
        self.bits_whole = self.bits = None
        if o.get('bits'):
            self.bits_whole = torch.full((B, nc + (2 if views else 0), T // 32), BITS_SENT, dtype=torch.int32, device=dev)
            self.bits = self.bits_whole[:, :nc]
        self.w0, self.k3, self.w2 = d['W0'].to(dev).contiguous(), d['k3'].to(dev).contiguous(), d['W2'].to(dev).contiguous()
        self.b2 = d['b2'].to(dev) if d['b2'] is not None else None
        self.planes_whole, self.planes = make_planes(self.w2, C2, nc, dev)
        self.names = set()

    def kernel(self):
        return f'film_cond_fwd_x6_kernel<{2 if self.C2 % 64 else 4}>'

    def call(self, args=None, planes='own', bits='own', bits_bs=None):
        L = mods()[1]
        aa = dict(B=self.B, T=self.T, n_cond=self.nc, n_var=NV, C2=self.C2, exc=self.exc.data_ptr(), exc_bs=self.exc.stride(0), w0=self.w0.data_ptr(),
                  k3=self.k3.data_ptr(), w2=None, b2=self.b2.data_ptr() if self.b2 is not None else None,
                  cv0=self.cv0.data_ptr() if self.cv0 is not None else None, cv0_bs=self.cv0.stride(0) if self.cv0 is not None else 0,
                  gb=self.gb.data_ptr(), gb_bs=self.gb.stride(0), slope=self.slope)
        aa.update(args or {})
        a_ = L.FilmCondArgs(**aa)
        if isinstance(bits, str):
            bits = self.bits.data_ptr() if self.bits is not None else None
        if bits_bs is None:
            bits_bs = self.bits.stride(0) if self.bits is not None else 0
        with traced() as tr:
            rc = L.lib().tdvc_film_cond_fwd_x6(C.byref(a_), self.planes.data_ptr() if isinstance(planes, str) else planes, bits, bits_bs, stream(self.dev))
        self.names = tr.names
        return rc

    def untouched(self):
        """No output, spare channel or sign word was written (the refusal tests)."""
        return bool((self.gb_whole == SENT).all()) and (self.cv0_whole is None or bool((self.cv0_whole == SENT).all())) and \
            (self.bits_whole is None or bool((self.bits_whole == BITS_SENT).all()))

    def run(self, tag=''):
        rc = self.call()
        assert rc == 0, (rc, mods()[1].lib().tdvc_last_error())
        assert self.names == {self.kernel()}, (self.name, sorted(self.names), self.kernel())
        d, res = self.d, {}
        for k, t in (('gb', self.gb),) + ((('cv0', self.cv0),) if self.cv0 is not None else ()):
            ratio, inexact = elem_check(t, d['ref'][k], d['A'][k], d['n'][k])
            res[k] = dict(rel=rel_l2(t, d['ref'][k]), ratio=ratio, inexact=inexact)
        assert_bars(res, f'{self.kernel()}: {self.name}{tag}')
        # cv0 and the sign words are written by output-channel block 0 alone: no SENT left inside, the spare channels intact
        assert _spare_intact(self.gb_whole, self.C2), 'wrote into the spare channels behind gb'
        if self.cv0 is not None:
            assert _spare_intact(self.cv0_whole, self.nc), 'wrote into the spare channels behind cv0'
        if self.bits is not None:
            words = self.bits.cpu()
            assert bool((self.bits_whole[:, self.nc:] == BITS_SENT).all()), 'wrote into the spare channels behind the sign words'
            cv_ref, A1 = d['ref']['cv0'], d['A']['cv0']
            got = ((words.long().unsqueeze(-1) >> torch.arange(32)) & 1).bool().reshape(self.B, self.nc, self.T)
            if self.cv0 is not None:
                assert torch.equal(words, pack_sign_bits(self.cv0.cpu())), 'sign words differ from (stored cv0 > 0)'
            flip = got != (cv_ref > 0)      # allowed only where the reference is within the bound of zero, element by element
            bound = (d['n']['cv0'] + 8) * U * A1 + 2.0 ** -22 * cv_ref.abs()
            assert bool((cv_ref.abs()[flip] <= bound[flip]).all()), (self.name, int(flip.sum()), float(cv_ref.abs()[flip].max()))
        if self.o.get('zero_sample'):      # exc = 0 and k3 = 0: cv0 is exactly +0, its bits are 0, gb is b2
            b = self.B - 1
            assert bool((self.cv0[b].view(torch.int32) == 0).all()), 'cv0 of the zero sample is not +0'
            assert bool((self.bits[b] == 0).all()), 'sign bits of the zero sample'
            assert torch.equal(self.gb[b].cpu(), d['b2'][:, None].expand(self.C2, self.T)), 'gb of the zero sample is not b2 bit for bit'
        WORST.note(self.kernel(), res, self.name)
        return res


@pytest.mark.parametrize('name', list(FUSED))
def test_fused_edge(name, dev):
    """Every row of FUSED: gb and cv0 within both bars, the sign words, the exact instance by trace."""
    CondFwdEdge(name, dev).run()


@pytest.mark.parametrize('name', list(FUSED))
def test_fused_edge_poisoned_lds(name, dev):
    """Once more on NaN-poisoned LDS: the excitation window's columns outside the sequence, the activation rows of channels >= n_cond
    and the halo rows of an edge tile must come from the kernel."""
    poison_lds(dev)
    e = CondFwdEdge(name, dev)
    e.run(' (poisoned LDS)')
    assert bool(torch.isfinite(e.gb).all())


def test_fused_optional_outputs_change_nothing(dev):
    """cv0 = NULL with and without sign bits, and bits = NULL: gb (and the words, where asked for) are the same bits as in the run that
    stored both."""
    name = 'nc136_C64_T256_no_cv0_bits'
    full = CondFwdEdge(name, dev, cv0=True)
    full.run(' (cv0 and bits stored)')
    no_cv0, neither, no_bits = CondFwdEdge(name, dev), CondFwdEdge(name, dev, bits=False), CondFwdEdge(name, dev, cv0=True, bits=False)
    for e, tag in ((no_cv0, ' (cv0 = NULL)'), (neither, ' (cv0 = NULL, bits = NULL)'), (no_bits, ' (bits = NULL)')):
        e.run(tag)
        assert torch.equal(e.gb, full.gb), tag
    assert torch.equal(no_cv0.bits, full.bits) and torch.equal(no_bits.cv0, full.cv0)


# ------------------------------------------------------------------------------------ one product per output element (part 2)
def _one_product_check(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    err, bound = (got - ref).abs(), ONE_PRODUCT_BOUND * ref.abs()
    nz = ref != 0
    worst = float((err[nz] / ref.abs()[nz]).max())
    print(f'[x6 one product] {what}: worst {worst / 2.0 ** -24:.2f} * 2^-24 over {int(nz.sum())} products (bar 16 * 2^-24)')
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), (what, worst / 2.0 ** -20, int((err > bound).sum()))
    return worst


@pytest.mark.parametrize('Cin,Cout', [(136, 32), (136, 64), (160, 32), (160, 64)])
def test_one_product_forward(Cin, Cout, dev):
    """W dense with constructed values; x has one nonzero channel at every third step (sample b at t = 1 + b mod 3, so that over the three
    samples every tile-edge halo position carries one), cycling through all Cin: every y element is exactly one product w * x."""
    T, B = 512, 3
    rng = np.random.default_rng(1000 * Cin + Cout)
    W = torch.from_numpy(constructed(rng, (Cout, Cin, 3))[0])
    vals = torch.from_numpy(constructed(rng, (B, T))[0])
    x = torch.zeros(B, Cin, T)
    for b in range(B):
        t = torch.arange((1 + b) % 3, T, 3)
        x[b, (t // 3 + 17 * b) % Cin, t] = vals[b, t]
    nz = x != 0
    assert bool(nz.any(0).any(1).all()), 'every input channel carries a product'
    assert all(bool(nz[:, :, p].any()) for p in (127, 128, 255, 256, 383, 384)), 'every tile-edge halo position carries a product'
    count = F.conv1d(nz.double(), torch.ones(1, Cin, 3, dtype=torch.float64), padding=1)
    assert float(count.max()) == 1 and float(count[:, :, 1:T - 1].min()) == 1
    ref = F.conv1d(x.double(), W.double(), padding=1)      # one nonzero term per element: exact
    row = ('one_product', (Cin, Cout, T, B), dict(bias=False))
    for tag in ('', ' (poisoned LDS)'):
        if tag:
            poison_lds(dev)
        e = FwdEdge(f'one_product_{Cin}_{Cout}', dev, row=row, data=dict(x=x, W=W, bias=None))
        assert e.call() == 0 and e.names == {e.kernel()}
        _one_product_check(e.y, ref, f'{e.kernel()} {Cin} -> {Cout}{tag}')


def _fused_one_product_weights(nc, C2, draw, rng):
    idx = np.arange(C2) + C2 * draw
    ci, tap = (idx * 37) % nc, idx % 3
    W2 = np.zeros((C2, nc, 3), dtype=np.float32)
    W2[np.arange(C2), ci, tap] = constructed(rng, (C2,))[0]
    return W2, ci, tap


@pytest.mark.parametrize('draw', [0, 1])
def test_one_product_fused(draw, dev):
    """W2 with one nonzero (ci, tap) per output channel, constructed values: gb[co][t] = W2[co][ci][tap] * lrelu(cv0[ci][t + tap - 1]) with
    the cv0 the GPU stored (the rounding of cv0 * slope fits in the margin). The two draws cover every (tap, input channel) pair."""
    nc, C2, T, B = 136, 256, 256, 2
    rng = np.random.default_rng(draw)
    W2, ci, tap = _fused_one_product_weights(nc, C2, draw, rng)
    both = set()
    for dr in (0, 1):
        _, c_, t_ = _fused_one_product_weights(nc, C2, dr, np.random.default_rng(dr))
        both |= set(zip(t_.tolist(), c_.tolist()))
    assert {(j, c // 32, c % 8) for j, c in both} == {(j, k, q) for j in range(3) for k in range(5) for q in range(8)}
    gen = torch.Generator().manual_seed(draw)
    rnd = lambda *sh: torch.randn(*sh, generator=gen).float()
    data = dict(exc=rnd(B, NV, T), W0=rnd(nc, nc, 3) / 24 ** 0.5, k3=rnd(B, nc, 3), W2=torch.from_numpy(W2), b2=None)
    data.update(cond_reference(data, 0.2))
    row = ('one_product_fused', (nc, C2, T, B), dict(b2=False))
    for tag in ('', ' (poisoned LDS)'):
        if tag:
            poison_lds(dev)
        e = CondFwdEdge(f'one_product_fused_{draw}', dev, row=row, data=data)
        assert e.call() == 0 and e.names == {e.kernel()}
        ref = F.conv1d(_lrelu64(e.cv0.cpu().double(), 0.2), data['W2'].double(), padding=1)
        _one_product_check(e.gb, ref, f'{e.kernel()} draw {draw}{tag}')
        ratio, inexact = elem_check(e.cv0, data['ref']['cv0'], data['A']['cv0'], data['n']['cv0'])
        assert ratio <= 1.0 and inexact == 0, ratio


def test_one_product_weight_grad(dev):
    """conv_wgrad_x6_kernel shares split_bf16.h: B = 1, dy with one nonzero step per output channel, x dense, dw0 = 0, so every dw
    element is one product dy[co][t_co] * x[ci][t_co + j - 1] (0 where that step is outside the sequence)."""
    Cin, Cout, T = 136, 32, 260
    rng = np.random.default_rng(260)
    x = torch.from_numpy(constructed(rng, (1, Cin, T))[0])
    t_co = torch.tensor([0, 259, 31, 32, 63, 64, 127, 128, 255, 256, 257, 258] + [8 * c + 5 for c in range(12, 32)])
    dy = torch.zeros(1, Cout, T)
    dy[0, torch.arange(Cout), t_co] = torch.from_numpy(constructed(rng, (Cout,))[0])
    xp = F.pad(x.double(), (1, 1))[0]                                       # xp[ci][t + 1] = x[ci][t]
    ref = torch.stack([dy.double()[0, torch.arange(Cout), t_co][:, None] * xp[:, t_co + j].T for j in range(3)], -1)      # [Cout][Cin][3]
    e = Edge(('x6_one_product', Cin, Cout, 3, 1, 1, 1, 1, False, False, 0, T), dev, B=1, with_db=False)
    e.xv.copy_(x.to(dev)); e.dyv.copy_(dy.to(dev)); e.dw.zero_()
    rc = e.wgrad_call()
    assert rc == 0 and e.guard_ok, (rc, mods()[1].lib().tdvc_last_error())
    assert e.names['wgrad'] == {'conv_wgrad_x6_kernel', 'slab_reduce_multi_kernel'}, sorted(e.names['wgrad'])
    assert int((ref == 0).sum()) == 2 * Cin      # tap 0 of the channel at t = 0, tap 2 of the channel at t = T - 1
    _one_product_check(e.dw, ref, 'conv_wgrad_x6_kernel 136 -> 32')


# ------------------------------------------------------------------------------------------ the weight-plane image (part 3)
@pytest.mark.parametrize('Cout,Cin', PLANE_GEOM)
def test_weight_plane_image(Cout, Cin, dev):
    """The image copied back and decoded with plane_offsets: every piece equals the numpy split of w bit for bit (so each has at most 8
    significant bits and the signs of +-0 survive), hi + mid + lo is w, channels >= Cin are zero words; make_planes asserts the byte count
    and the guard around exactly that many bytes."""
    gen = torch.Generator().manual_seed(Cout * 1000 + Cin)
    w = torch.randn(Cout, Cin, 3, generator=gen).float()
    flat = w.view(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:600]
    flat[idx] = torch.tensor([0.0, -0.0, 1.0, -1.5, 2.0 ** -10, 3.0 * 2.0 ** 40, 1.0 + 2.0 ** -8, -(1.0 + 2.0 ** -16)]).repeat(75)
    _, img = make_planes(w.to(dev), Cout, Cin, dev)
    p = decode_planes(img.cpu().numpy(), Cout)                             # [piece][Cout][tap][160]
    wt = np.ascontiguousarray(w.numpy().transpose(0, 2, 1))                # [Cout][tap][Cin]
    for k, want in enumerate(split3(wt)):
        assert np.array_equal(p[k][:, :, :Cin].view(np.uint32), want.view(np.uint32)), f'piece {k}'
    total = p[0].astype(np.float64) + p[1] + p[2]
    assert np.array_equal(total[:, :, :Cin], wt.astype(np.float64))
    assert not p[:, :, :, Cin:].view(np.uint32).any(), 'channels >= Cin are not zero'


def test_weight_planes_refuse_partial_record(dev):
    """Cout % 32 != 0: no kernel could read a partial record. TDVC_EINVAL and a buffer (large enough for the next multiple) untouched."""
    L = mods()[1]
    lib = L.lib()
    w = torch.randn(64, 136, 3, device=dev)
    buf = torch.full((planes_bytes(64) // 2,), GUARD16, dtype=torch.int16, device=dev)
    for Cout in (48, 16):
        assert lib.tdvc_conv_x6_weight_planes_bytes(Cout, 136, 3) == 0
        assert lib.tdvc_conv_x6_weight_planes(w.data_ptr(), Cout, 136, 3, buf.data_ptr(), stream(dev)) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf == GUARD16).all())


# ------------------------------------------------------------------------------------------------------- refusals (part 4)
def _xf(kind, slope, scale=1.0, aux=None):
    return mods()[1].Xform(kind, slope, scale, aux.data_ptr() if aux is not None else None, aux.stride(0) if aux is not None else 0)


KNOBS = {'knob6': (lambda lib: lib.tdvc_debug_knob(6, 1), lambda lib: lib.tdvc_debug_knob(6, 0)),
         'forced_lean_tile': (lambda lib: lib.tdvc_debug_force_tile(0), lambda lib: lib.tdvc_debug_force_tile(-1)),
         'forced_generic': (lambda lib: lib.tdvc_set_force_generic(1), lambda lib: lib.tdvc_set_force_generic(0))}
_T = lambda T: dict(Tin=T, Tout=T)
# what -> (desc fields, args fields (a callable gets the case), planes pointer offset in bytes or None for NULL, return code)
PLAIN_REFUSALS = {
    'Cin64': (dict(Cin=64), {}, 0, EUNSUPPORTED), 'Cin161': (dict(Cin=161), {}, 0, EUNSUPPORTED),
    'Cout16': (dict(Cout=16), {}, 0, EUNSUPPORTED), 'Cout48': (dict(Cout=48), {}, 0, EUNSUPPORTED),
    'T124': (_T(124), {}, 0, EUNSUPPORTED), 'T130': (_T(130), {}, 0, EUNSUPPORTED),
    'x_misaligned': ({}, lambda e: dict(x=e.x.data_ptr() + 4), 0, EUNSUPPORTED),
    'y_misaligned': ({}, lambda e: dict(y=e.y.data_ptr() + 4), 0, EUNSUPPORTED),
    'planes_misaligned': ({}, {}, 4, EUNSUPPORTED),
    'x_bs_mod4': ({}, lambda e: dict(x_bs=e.x.stride(0) + 2), 0, EUNSUPPORTED),
    'y_bs_mod4': ({}, lambda e: dict(y_bs=e.y.stride(0) + 2), 0, EUNSUPPORTED),
    'stride2': (dict(stride=2), {}, 0, EUNSUPPORTED), 'K5': (dict(K=5), {}, 0, EUNSUPPORTED), 'dilation2': (dict(dilation=2), {}, 0, EUNSUPPORTED),
    'pad0': (dict(pad=0), {}, 0, EUNSUPPORTED), 'reflect': (dict(reflect=1), {}, 0, EUNSUPPORTED), 'groups2': (dict(groups=2), {}, 0, EUNSUPPORTED),
    'w_cin': (dict(w_cin=160, w_cin_off=8), {}, 0, EUNSUPPORTED), 'transposed': (dict(kind=1), {}, 0, EUNSUPPORTED),
    # the extra operand is the (large, readable and writable) x buffer: a regression that used it stays in bounds
    'res': ({}, lambda e: dict(res=e.x.data_ptr(), res_bs=e.x.stride(0)), 0, EUNSUPPORTED),
    'add': ({}, lambda e: dict(add=e.x.data_ptr(), add_bs=e.x.stride(0)), 0, EUNSUPPORTED),
    'bias3': ({}, lambda e: dict(bias3=e.x.data_ptr()), 0, EUNSUPPORTED),
    'sign_bits': ({}, lambda e: dict(sign_bits=e.x.data_ptr(), sign_bits_bs=e.x.stride(0)), 0, EUNSUPPORTED),
    'post_lrelu': ({}, dict(post_act=1), 0, EUNSUPPORTED), 'out_scale_half': ({}, dict(out_scale=0.5), 0, EUNSUPPORTED),
    'film_prologue': ({}, lambda e: dict(x_xf=_xf(2, 0.2, 1.0, e.x)), 0, EUNSUPPORTED),
    'x_scale2': ({}, lambda e: dict(x_xf=_xf(1, 0.2, 2.0)), 0, EUNSUPPORTED),
    'slope0': ({}, lambda e: dict(x_xf=_xf(1, 0.0)), 0, EUNSUPPORTED), 'slope_neg': ({}, lambda e: dict(x_xf=_xf(1, -0.2)), 0, EUNSUPPORTED),
    'slope_1p5': ({}, lambda e: dict(x_xf=_xf(1, 1.5)), 0, EUNSUPPORTED),
    'knob6': ({}, {}, 0, EUNSUPPORTED), 'forced_lean_tile': ({}, {}, 0, EUNSUPPORTED), 'forced_generic': ({}, {}, 0, EUNSUPPORTED),
    'x_null': ({}, dict(x=None), 0, EINVAL), 'y_null': ({}, dict(y=None), 0, EINVAL), 'planes_null': ({}, {}, None, EINVAL),
}


def _planes_off(e, poff):
    return None if poff is None else e.planes.data_ptr() + poff


def _with_knob(what, fn):
    lib = mods()[1].lib()
    if what not in KNOBS:
        return fn()
    KNOBS[what][0](lib)
    try:
        return fn()
    finally:
        KNOBS[what][1](lib)


@pytest.mark.parametrize('what', list(PLAIN_REFUSALS))
def test_plain_refusals(what, dev):
    """tdvc_conv_fwd_x6 outside its contract: the return code, nothing launched, y and its spare channels still SENT. The base call is valid
    (asserted) and its x buffer has 32 spare channels, y and the planes cover every refused geometry."""
    desc, args, poff, code = PLAIN_REFUSALS[what]
    e = FwdEdge(PLAIN_BASE[0], dev)
    rc = _with_knob(what, lambda: e.call(desc, args(e) if callable(args) else args, _planes_off(e, poff)))
    torch.cuda.synchronize()
    assert rc == code, (what, rc, mods()[1].lib().tdvc_last_error())
    assert not e.names, sorted(e.names)
    assert bool((e.y_whole == SENT).all()), 'a refused call wrote y'
    if what == 'Cin64':      # the base call itself is inside the contract
        e.run(' (refusal base)')


# what -> (args fields, planes offset | None, bits: True = the case's words, return code)
FUSED_REFUSALS = {
    'n_var4': (dict(n_var=4), 0, EUNSUPPORTED),
    'nc64': (dict(n_cond=64), 0, EUNSUPPORTED), 'nc138': (dict(n_cond=138), 0, EUNSUPPORTED), 'nc164': (dict(n_cond=164), 0, EUNSUPPORTED),
    'C2_48': (dict(C2=48), 0, EUNSUPPORTED), 'T124': (dict(T=124), 0, EUNSUPPORTED), 'T130': (dict(T=130), 0, EUNSUPPORTED),
    'bits_T132': (dict(T=132), 0, EUNSUPPORTED),
    'slope0': (dict(slope=0.0), 0, EUNSUPPORTED), 'slope_1p5': (dict(slope=1.5), 0, EUNSUPPORTED),
    'exc_misaligned': (lambda e: dict(exc=e.exc.data_ptr() + 4), 0, EUNSUPPORTED),
    'gb_misaligned': (lambda e: dict(gb=e.gb.data_ptr() + 4), 0, EUNSUPPORTED),
    'cv0_misaligned': (lambda e: dict(cv0=e.cv0.data_ptr() + 4), 0, EUNSUPPORTED),
    'k3_misaligned': (lambda e: dict(k3=e.k3.data_ptr() + 4), 0, EUNSUPPORTED),
    'planes_misaligned': ({}, 4, EUNSUPPORTED),
    'exc_bs_mod4': (lambda e: dict(exc_bs=e.exc.stride(0) + 2), 0, EUNSUPPORTED),
    'gb_bs_mod4': (lambda e: dict(gb_bs=e.gb.stride(0) + 2), 0, EUNSUPPORTED),
    'cv0_bs_mod4': (lambda e: dict(cv0_bs=e.cv0.stride(0) + 2), 0, EUNSUPPORTED),
    'knob6': ({}, 0, EUNSUPPORTED), 'forced_lean_tile': ({}, 0, EUNSUPPORTED), 'forced_generic': ({}, 0, EUNSUPPORTED),
    'exc_null': (dict(exc=None), 0, EINVAL), 'w0_null': (dict(w0=None), 0, EINVAL), 'k3_null': (dict(k3=None), 0, EINVAL),
    'gb_null': (dict(gb=None), 0, EINVAL), 'planes_null': ({}, None, EINVAL),
}


@pytest.mark.parametrize('what', list(FUSED_REFUSALS))
def test_fused_refusals(what, dev):
    """tdvc_film_cond_fwd_x6 outside its contract: the return code, nothing launched, gb, cv0, the sign words and all their spare channels
    untouched. k3, W0, cv0 and the words are allocated for 168 channels, so that n_cond = 164 stays inside them."""
    args, poff, code = FUSED_REFUSALS[what]
    e = CondFwdEdge(FUSED_BASE[0], dev)
    big = 168
    e.k3 = torch.zeros(e.B, big, 3, device=dev)
    e.w0 = torch.zeros(big, big, 3, device=dev)
    e.cv0_whole = torch.full((e.B, big + 4, e.T), SENT, dtype=torch.float32, device=dev)
    e.cv0 = e.cv0_whole[:, :e.nc]
    e.bits_whole = torch.full((e.B, big + 2, e.T // 32), BITS_SENT, dtype=torch.int32, device=dev)
    e.bits = e.bits_whole[:, :e.nc]
    rc = _with_knob(what, lambda: e.call(args(e) if callable(args) else args, _planes_off(e, poff)))
    torch.cuda.synchronize()
    assert rc == code, (what, rc, mods()[1].lib().tdvc_last_error())
    assert not e.names, sorted(e.names)
    assert e.untouched(), 'a refused call wrote an output'
    if what == 'n_var4':      # the base call itself is inside the contract
        CondFwdEdge(FUSED_BASE[0], dev).run(' (refusal base)')


def test_zz_worst_error_by_kernel():
    """Prints the worst err / bound per kernel and tensor over the cases that ran in this session (asserted case by case)."""
    WORST.report()
