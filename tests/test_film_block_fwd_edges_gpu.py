"""The C ABI of tdvc_film_block_fwd (film_block.hip, film_block_fwd_kernel<FILM>: dilated conv + FiLM + 1x1 conv + residual + MRF sum in
one launch, 16 channels) through ctypes, against float64. test_fused_film_block_forward_is_bit_identical compares the kernel with the
two-launch path through ops.FilmBlockFn (contiguous operands, K in {3, 7, 11}); this file checks the contract itself.

Rules (those of test_generic_conv_edges_gpu.py; the rows, their data and the float64 reference are in film_block_ref.py):

  * Inputs hold fp32 values; the references are float64 on the same numbers.
  * h = float64 reflect-padded dilated conv of lrelu(x), plus b1; bars with n = 16 K, A = conv(|lrelu(x)|, |w1|), slack 8.
  * out is computed in float64 from the GPU's OWN stored h (fp32 values), gamma / beta, w2, b2, x and acc, so only the second stage's
    arithmetic is judged: out = scale * (w2 . lrelu(h (1 + gamma) + beta) + b2 + x) + acc. The kink assertion uses that h: no element of
    h2 = h (1 + gamma) + beta within 3 * 2^-23 * H of 0, H = |h| (1 + |gamma|) + |beta| (test_lean_edges_cpu.py screens the rows
    with the float64 h rounded to fp32). Without FiLM the mask is the sign of the stored h: exact on both sides.
  * Bars for out: n = 16, A = scale * (sum |w2| H' + |b2| + |x|) + |acc| with H' = H, or |h| without FiLM. Slack: the prologue and the
    product are those of the posconv (12 with FiLM, 8 without: Edge's docstring); behind them the kernel adds the residual, scales and
    adds acc, one rounding each of a partial result no larger than A, i.e. 3 * 2^-24 * A = 1.5 units: slack 13.5 / 9.5.
        rel-L2 < 2e-5   and   |got - ref| <= (n + slack) * 2^-23 * A + 2^-22 * |ref|
  * x, h, gb, add and y may be [:, :C] views of [B, C + 3, T] buffers (batch strides wider than contiguous). The spares are NaN behind
    the inputs and SENT behind the outputs; every buffer, view or not, has a 64-float guard behind its last row (NaN / SENT alike), so
    a write at columns >= T of the last row, or a read there, shows.
  * Every accepted row asserts by trace film_block_fwd_kernel<true|false> and nothing else, runs a second time on NaN-poisoned LDS,
    and must be bit-identical, h and out, to the two tdvc_conv_fwd calls FilmBlockFn's fallback makes on the same buffers.
  * Every refusal asserts the return code, an empty trace, and that every output and guard is still SENT.

RESULTS (first run on an MI355X, err / bound, the bar is 1.0): film_block_fwd_kernel<true> h 0.068 (k1_d7_T512_nohalo), out 0.056
(k4_d2_T512_even); film_block_fwd_kernel<false> below that. Every accepted row is bit-identical to the two-launch path, every refusal
returns its code with nothing launched. No defect was found.
"""
import ctypes as C

import pytest
import torch

from common import rel_l2, traced
from edge_support import EINVAL, EUNSUPPORTED, SENT, SLOPE, U, Worst, assert_bars, elem_check, lib, mods, poison_lds, stream
from film_block_ref import ROWS, block_data, conv_h64, out64

pytestmark = pytest.mark.gpu
GUARD = 64
NAN = float('nan')
WORST = Worst()      # kernel -> tensor -> (err / bound, row)


def gbuf(B, Cc, T, dev, views, fill, src=None, lead=0, bs=None):
    """(flat buffer, operand): [B, Cc (+ 3 with views), T] filled with `fill` with a GUARD of the same fill behind the last row; `lead`
    floats in front (an operand that is not 16-byte aligned), `bs` a batch stride of its own."""
    rows = Cc + (3 if views else 0)
    bs = bs or rows * T
    flat = torch.full((lead + (B - 1) * bs + rows * T + GUARD,), fill, dtype=torch.float32, device=dev)
    v = flat[lead:].as_strided((B, Cc, T), (bs, T, 1))
    if src is not None:
        v.copy_(src.to(dev))
    return flat, v


def untouched(flat, v):
    """Everything of an output buffer outside the operand still holds SENT."""
    mask = torch.ones_like(flat, dtype=torch.bool)
    off = v.storage_offset() - flat.storage_offset()
    B, Cc, T = v.shape
    idx = (off + torch.arange(B, device=flat.device)[:, None] * v.stride(0) + torch.arange(Cc * T, device=flat.device)[None, :]).reshape(-1)
    mask[idx] = False
    return bool((flat[mask] == SENT).all())


class Block:
    """One call of tdvc_film_block_fwd on guarded buffers."""

    def __init__(self, name, K, d, T, dev, B=3, C_=16, views=False, x_lead=0, x_bs=None, **opts):
        self.name, self.K, self.d, self.T, self.B, self.C, self.dev = name, K, d, T, B, C_, dev
        self.data = D = block_data(name, K, d, T, B, C_, **opts)
        f = lambda t: t.to(dev).contiguous() if t is not None else None
        vw = (lambda n: views) if isinstance(views, bool) else (lambda n: n in views)      # True / False, or the names of the views
        self.w1, self.b1, self.w2, self.b2 = f(D['w1']), f(D['b1']), f(D['w2']), f(D['b2'])
        self.x_flat, self.x = gbuf(B, C_, T, dev, vw('x'), NAN, D['x'], lead=x_lead, bs=x_bs)
        self.gb = gbuf(B, 2 * C_, T, dev, vw('gb'), NAN, D['gb'])[1] if D['gb'] is not None else None
        self.acc = gbuf(B, C_, T, dev, vw('acc'), NAN, D['acc'])[1] if D['acc'] is not None else None
        self.h_flat, self.h = gbuf(B, C_, T, dev, vw('h'), SENT)
        self.y_flat, self.y = gbuf(B, C_, T, dev, vw('y'), SENT)
        self.names = set()

    def args(self, **over):
        L = mods()[1]
        pb = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
        v = dict(B=self.B, C=self.C, T=self.T, K=self.K, d=self.d, w1=self.w1.data_ptr())
        v.update(over)
        return L.FilmBlockArgs(v['B'], v['C'], v['T'], v['K'], v['d'], *pb(self.x), v['w1'], self.b1.data_ptr() if self.b1 is not None else None,
                               *pb(self.h), *pb(self.gb), self.w2.data_ptr(), self.b2.data_ptr() if self.b2 is not None else None, *pb(self.acc),
                               self.data['scale'], SLOPE, *pb(self.y))

    def call(self, **over):
        a = self.args(**over)
        with traced() as tr:
            rc = lib().tdvc_film_block_fwd(C.byref(a), stream(self.dev))
        self.names = tr.names
        return rc

    def outputs_untouched(self):
        return bool((self.h_flat == SENT).all()) and bool((self.y_flat == SENT).all())

    def bars(self):
        D = self.data
        h_ref, h_A = conv_h64(D['x'], D['w1'], D['b1'], self.K, self.d)
        h_gpu = self.h.detach().cpu()
        out_ref, out_A, h2, H = out64(h_gpu, D['x'], D['gb'], D['w2'], D['b2'], D['acc'], D['eff_scale'])
        if D['gb'] is not None:
            assert bool((h2.abs() > 3 * U * H).all()), 'an element of h2 sits on the LeakyReLU kink: reseed (rename) the row'
        film = D['gb'] is not None
        res = {}
        for key, got, ref, A, n, slack in (('h', self.h, h_ref, h_A, 16 * self.K, 8), ('out', self.y, out_ref, out_A, 16, 13.5 if film else 9.5)):
            ratio, inexact = elem_check(got, ref, A, n, slack)
            res[key] = dict(rel=rel_l2(got, ref), ratio=ratio, inexact=inexact)
        return res

    def two_launch(self):
        """h and out of the two tdvc_conv_fwd calls FilmBlockFn's fallback makes, on the same input buffers."""
        ops, L, arena = mods()
        cs = ops.ConvSpec(16, 16, self.K, 1, (self.K - 1) * self.d // 2, self.d, 1, True)
        cs.slot = arena.ConvSlot(self.w1.data_ptr(), self.b1.data_ptr() if self.b1 is not None else 0, 0, 0, False, None, 0)
        ps = ops.ConvSpec(16, 16, 1)
        ps.slot = arena.ConvSlot(self.w2.data_ptr(), self.b2.data_ptr() if self.b2 is not None else 0, 0, 0, False, None, 0)
        h = ops.conv_fwd_raw(cs, self.x, ops._xf(L.XF_LRELU))
        xf2 = ops._xf(L.XF_FILM_LRELU, aux=self.gb) if self.gb is not None else ops._xf(L.XF_LRELU)
        out = ops.conv_fwd_raw(ps, h, xf2, res=self.x, add=self.acc, out_scale=self.data['scale'])
        return h, out


@pytest.mark.parametrize('name', list(ROWS))
def test_film_block_row(name, dev):
    """Every accepted row: rc 0, the instance by trace and nothing else, both bars on h and out, nothing written outside the two
    operands, bit-identical to the two-launch fallback; once more on NaN-poisoned LDS."""
    K, d, T, opts = ROWS[name]
    for poison in (False, True):
        blk = Block(name, K, d, T, dev, **opts)
        if poison:
            poison_lds(dev)
        rc = blk.call()
        assert rc == 0, (rc, lib().tdvc_last_error())
        kern = 'film_block_fwd_kernel<true>' if opts.get('film') else 'film_block_fwd_kernel<false>'
        assert blk.names == {kern}, sorted(blk.names)
        assert untouched(blk.h_flat, blk.h) and untouched(blk.y_flat, blk.y), 'the kernel wrote outside h / out'
        res = blk.bars()
        assert_bars(res, name + (' (poisoned LDS)' if poison else ''))
        WORST.note(kern, res, name)
        with traced() as tr:
            h2, out2 = blk.two_launch()
        assert not any(n.startswith('film_block_fwd_kernel') for n in tr.names), sorted(tr.names)
        assert torch.equal(blk.h, h2), ('h differs from the two-launch path', float((blk.h - h2).abs().max()))
        assert torch.equal(blk.y, out2), ('out differs from the two-launch path', float((blk.y - out2).abs().max()))


# name: (K, d, T, Block options, overrides of the call, expected return code)
REFUSALS = {r[0]: r[1:] for r in [
    ('T508', 3, 1, 508, {}, {}, EUNSUPPORTED),
    ('T514', 3, 1, 514, {}, {}, EUNSUPPORTED),
    ('k4_d1_odd_field', 4, 1, 512, {}, {}, EUNSUPPORTED),
    ('k16', 16, 2, 512, {}, {}, EUNSUPPORTED),
    ('k15_d5_span', 15, 5, 512, {}, {}, EUNSUPPORTED),
    ('k3_d33_span', 3, 33, 512, {}, {}, EUNSUPPORTED),
    ('c32', 3, 1, 512, dict(C_=32), {}, EUNSUPPORTED),
    ('x_4_bytes_in', 3, 1, 512, dict(x_lead=1), {}, EUNSUPPORTED),
    ('x_bs_mod4', 3, 1, 512, dict(x_bs=16 * 512 + 2), {}, EUNSUPPORTED),
    ('pinned_lean_tile', 3, 1, 512, {}, dict(force_tile=0), EUNSUPPORTED),
    ('null_w1', 3, 1, 512, {}, dict(w1=None), EINVAL),
    ('b0', 3, 1, 512, {}, dict(B=0), EINVAL),
]}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_film_block_refusal(name, dev):
    """Outside the contract: the return code, nothing launched, every output and guard still SENT. The buffers are sized for the refused
    geometry (32 channels where C = 32 is asked for), so a launch that slipped through would stay inside them."""
    K, d, T, bopts, over, want = REFUSALS[name]
    blk = Block(name, K, d, T, dev, **bopts)
    if blk.C != 16:      # w2 for the refused channel count
        blk.w2 = torch.randn(blk.C, blk.C, device=dev)
    over = dict(over)
    tile = over.pop('force_tile', None)
    if tile is not None:
        lib().tdvc_debug_force_tile(tile)
    try:
        rc = blk.call(**over)
    finally:
        lib().tdvc_debug_force_tile(-1)
    torch.cuda.synchronize()
    assert rc == want, (name, rc, lib().tdvc_last_error())
    assert not blk.names, sorted(blk.names)
    assert blk.outputs_untouched(), 'a refused call wrote to h / out or their guards'


def test_zz_worst_error_film_block():
    """Prints the worst err / bound per kernel and tensor over the rows that ran in this session (asserted row by row)."""
    WORST.report()
    assert all(r <= 1.0 for r in WORST.ratios())
