"""Edge shapes of the FiLM conditioning BACKWARD against float64: film_cond_bwd_kernel<BITS> (film_cond_fused_bwd.hip, the fused
backward behind cond_var.2's output gradient) and film_cond0_bwd_kernel (film_cond_bwd.hip, cond_var.0 alone), each with the
dk3_fold_kernel and the slab fold that close the call. Both entry points are driven through the C ABI (tdvc_film_cond_bwd,
tdvc_film_cond0_bwd): ops.FilmCondFn's gates (sign bits only at T >= 512, contiguous operands, n_cond = 136) hide most of the contract.

Same rules as test_generic_conv_edges_gpu.py, with the helpers of edge_support.py: fp32-valued inputs, a float64 CPU reference on the same
numbers, dw0 ACCUMULATED onto random values, dexc and dk3 starting as SENT, the workspace exactly the queried bytes inside a
SENT-guarded buffer, operands that may be channel slices of wider buffers, and both bars on every tensor:
    rel-L2 < 2e-5   and   |got - ref| <= (n + 8) * 2^-23 * A + 2^-22 * |ref|
(n and A: CondEdge's docstring). dw0 columns 0 .. n_cond - 9 (the embedding window, A = 0) must still hold dw0_start bit for bit.
Every case asserts by trace the exact kernel, dk3_fold_kernel iff a workspace was given, slab_reduce_multi_kernel iff dw0 was given,
and nothing else.

The table is CASES of film_cond_cases.py; test_cond_plan_cpu.py checks the plan figures quoted in it (chunks per block, blocks, straddling) on the CPU.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from common import rel_l2, traced
from edge_support import (EINVAL, EUNSUPPORTED, EWORKSPACE, SENT, Worst, _buf, _spare_intact, assert_bars, elem_check, mods, pack_sign_bits,
                          poison_lds)
from film_cond_cases import BITS_ROWS, CASES, COND0, FUSED, NV, REFUSAL_BASE, ROWS

pytestmark = pytest.mark.gpu

FOLD, SLAB = 'dk3_fold_kernel', 'slab_reduce_multi_kernel'
WORST = Worst()                          # kernel -> tensor -> (err / bound, case)
_DATA = {}                               # (case, which) -> inputs and float64 references, computed once and never modified


def _row(name):
    return REFUSAL_BASE if name == REFUSAL_BASE[0] else CASES[name]


def _convT(x, w):
    return F.conv_transpose1d(x, w, padding=1)


def _consume(d, exc, w0x, T):
    """dexc, dW0x [nc][8][3] and dk3 of a d_cv0 tensor (float64; the same call on absolute values gives A)."""
    dexc = _convT(d, w0x)
    ep = F.pad(exc, (1, 1))
    dw = torch.stack([torch.einsum('bct,bet->ce', d, ep[:, :, j:j + T]) for j in range(3)], -1)      # exc[t + j - 1], zero outside [0, T)
    dk3 = torch.stack([d[:, :, 0], d[:, :, 1:T - 1].sum(-1), d[:, :, T - 1]], -1)
    return dexc, dw, dk3


def case_data(name, which):
    """Inputs (fp32, CPU) and float64 references of one (row, entry point)."""
    if (name, which) in _DATA:
        return _DATA[(name, which)]
    _, (nc, C2, T, B), o = _row(name)
    slope = o.get('slope', 0.2)
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *sh: torch.randn(*sh, generator=gen).float()
    d = dict(dgb=rnd(B, C2, T), W2=rnd(C2, nc, 3) / (3 * nc) ** 0.5, W0=rnd(nc, nc, 3) / (3 * nc) ** 0.5, exc=rnd(B, NV, T),
             cv0=rnd(B, nc, T), dcv=rnd(B, nc, T), dw0_start=rnd(nc, nc, 3), slope=slope)
    flat = d['cv0'].view(-1)
    idx = torch.randint(flat.numel(), (min(300, flat.numel() // 2),), generator=gen)
    flat[idx] = torch.tensor([0.0, -0.0, 2.0 ** -149]).repeat(100)[:idx.numel()]      # +0, -0 (mask = slope), the smallest denormal (mask = 1)
    w0x = d['W0'][:, nc - NV:, :].double()
    if which == FUSED:
        m = torch.where(d['cv0'] > 0, 1.0, slope).double()
        dcv = m * _convT(d['dgb'].double(), d['W2'].double())
        A1 = m * _convT(d['dgb'].double().abs(), d['W2'].double().abs())
    else:
        dcv, A1 = d['dcv'].double(), d['dcv'].double().abs()
    dexc, dw, dk3 = _consume(dcv, d['exc'].double(), w0x, T)
    a_dexc, a_dw, a_dk3 = _consume(A1, d['exc'].double().abs(), w0x.abs(), T)
    grad, A_dw = torch.zeros(nc, nc, 3, dtype=torch.float64), torch.zeros(nc, nc, 3, dtype=torch.float64)
    grad[:, nc - NV:], A_dw[:, nc - NV:] = dw, a_dw
    n1 = 3 * C2 if which == FUSED else 0
    d.update(grad=grad, ref=dict(dexc=dexc, dw0=d['dw0_start'].double() + grad, dk3=dk3), A=dict(dexc=a_dexc, dw0=A_dw, dk3=a_dk3),
             n=dict(dexc=3 * nc + n1, dw0=B * T + n1, dk3=T + n1))
    _DATA[(name, which)] = d
    return d


def _sliced(B, Cc, T, dev, src=None, extra=4, dtype=torch.float32):
    """(whole [B, Cc + extra, T] buffer, its channel slice [:, :Cc]): SENT-filled (zero words for integers) around the operand."""
    whole = torch.full((B, Cc + extra, T), SENT if dtype == torch.float32 else 0, dtype=dtype, device=dev)
    v = whole[:, :Cc]
    if src is not None:
        v.copy_(src.to(dev))
    return whole, v


class CondEdge:
    """One (row, entry point) through tdvc_film_cond_bwd / tdvc_film_cond0_bwd against float64, with m = where(cv0 > 0, 1, slope):

        d_cv0 = m * conv_transpose1d(dgb, W2, padding=1)                          (fused; cond0: d_cv0 = dcv, an input)
        dexc  = conv_transpose1d(d_cv0, W0[:, nc-8:, :], padding=1)
        dW0[:, nc-8:, j] = dw0_start + sum_{b,t} d_cv0[b,c,t] * exc[b,ce,t+j-1]   (zero outside [0, T))
        dk3[b,c,:] = d_cv0[b,c,0], sum_{0<t<T-1} d_cv0[b,c,t], d_cv0[b,c,T-1]

    A is the same computation on absolute values, with m <= 1 kept as it is. The bound: cond0 sums fp32 products of its inputs, n = 3 nc
    for dexc, B T for dW0, T for dk3 (the indicator rows multiply by exactly 1 or 0). The fused kernel forms d_cv0 in fp32 first: a sum of
    3 C2 products and one multiplication by m, so |d^ - d_cv0| <= (3 C2 + 1) 2^-24 A1 to first order, A1 = m conv_transpose1d(|dgb|, |W2|).
    The second sum then computes sum w d^ with its own error n2 2^-24 sum |w| |d^| and inherits sum |w| |d^ - d_cv0|; both are multiples of
    A = sum |w| A1 >= sum |w| |d_cv0|, together (n2 + 3 C2 + 1) 2^-24 A. So the fused n is n2 + 3 C2 per tensor, and the bound's 2^-23 leaves
    a factor of two over the first-order term; the three-tap LDS sum of dexc (two more additions), the sum of the block slabs and of the
    dk3 slots (as many additions more as a sample or the batch has blocks, each at 2^-24 of a partial sum bounded by A) sit inside that
    factor and the slack of 8. Where A = 0 (dW0 columns of the embedding window) the buffer must still hold dw0_start bit for bit."""

    def __init__(self, name, which, dev, mask=None, cv0_unaligned=False):
        _, (nc, C2, T, B), o = _row(name)
        self.name, self.which, self.dev, self.o = name, which, dev, o
        self.nc, self.C2, self.T, self.B = nc, C2, T, B
        self.mask = mask or o.get('mask', 'fp32')
        self.d = d = case_data(name, which)
        views = o.get('views', False)
        buf = (lambda Cc, src=None: _sliced(B, Cc, T, dev, src)) if views else (lambda Cc, src=None: _buf(B, Cc, T, dev, False, src))
        self.src_whole, self.src = buf(C2, d['dgb']) if which == FUSED else buf(nc, d['dcv'])
        self.exc = buf(NV, d['exc'])[1]
        self.dexc_whole, self.dexc = buf(NV)
        self.cv0 = self.bits = None
        if which == FUSED:
            self.wt2 = d['W2'].permute(1, 0, 2).contiguous().to(dev)
            if self.mask == 'bits':
                words = pack_sign_bits(d['cv0'])
                self.bits = _sliced(B, nc, T // 32, dev, words, 2, torch.int32)[1] if o.get('bits_views') else words.to(dev)
            elif cv0_unaligned:
                self.cv0_whole, self.cv0 = _buf(B, nc, T, dev, False, d['cv0'], unaligned=True)
            else:
                self.cv0_whole, self.cv0 = buf(nc, d['cv0'])
        self.w0 = d['W0'].to(dev)
        self.dw0 = d['dw0_start'].to(dev)
        self.dk3 = torch.full((B, nc, 3), SENT, dtype=torch.float32, device=dev)
        self.with_dexc, self.with_dw, self.with_ws = o.get('dexc', True), o.get('dw', True), o.get('ws', True)
        self.names, self.calls = set(), 0

    def args(self, ws_ptr, ws_bytes, **over):
        """The argument struct of the case; `over` replaces fields (the refusal tests)."""
        L = mods()[1]
        f = dict(B=self.B, T=self.T, n_cond=self.nc, n_var=NV, exc=self.exc.data_ptr(), exc_bs=self.exc.stride(0), w0=self.w0.data_ptr(),
                 dexc=self.dexc.data_ptr() if self.with_dexc else None, dexc_bs=self.dexc.stride(0), dk3=self.dk3.data_ptr(),
                 dw0=self.dw0.data_ptr() if self.with_dw else None, workspace=ws_ptr, workspace_bytes=ws_bytes)
        if self.which == FUSED:
            f.update(C2=self.C2, dgb=self.src.data_ptr(), dgb_bs=self.src.stride(0), wt2=self.wt2.data_ptr(), slope=self.d['slope'],
                     cv0_sign_bits=self.bits.data_ptr() if self.bits is not None else None,
                     cv0_sign_bits_bs=self.bits.stride(0) if self.bits is not None else 0,
                     cv0=self.cv0.data_ptr() if self.cv0 is not None else None, cv0_bs=self.cv0.stride(0) if self.cv0 is not None else 0)
        else:
            f.update(dcv=self.src.data_ptr(), dcv_bs=self.src.stride(0))
        f.update(over)
        return (L.FilmCondBwdArgs if self.which == FUSED else L.FilmCond0BwdArgs)(**f)

    def call(self, ws_short=0, with_ws=None, **over):
        """One call -> rc. The workspace is exactly the queried size (less `ws_short` bytes) inside a larger SENT-filled buffer;
        self.guard_ok says whether the bytes around the region are still SENT afterwards."""
        L = mods()[1]
        lib = L.lib()
        q = lib.tdvc_film_cond_bwd_workspace if self.which == FUSED else lib.tdvc_film_cond0_bwd_workspace
        self.query = q(self.B, self.T, self.nc, NV)
        assert self.query > 0 and self.query % 4 == 0
        nbytes = self.query - ws_short
        lead = 64                                                   # floats in front of the region (keeps it 256-byte aligned)
        guard = torch.full((lead + self.query // 4 + 64,), SENT, dtype=torch.float32, device=self.dev)
        use_ws = self.with_ws if with_ws is None else with_ws
        a = self.args(guard.data_ptr() + 4 * lead if use_ws else None, nbytes if use_ws else 0, **over)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        fn = lib.tdvc_film_cond_bwd if self.which == FUSED else lib.tdvc_film_cond0_bwd
        with traced() as tr:
            rc = fn(C.byref(a), st)
            L.check(lib.tdvc_fold_flush(st))      # other tests of the process may have left deferral on
        self.names = tr.names
        g = guard.cpu()
        self.guard_ok = bool((g[:lead] == SENT).all() and (g[lead + (nbytes if use_ws else 0) // 4:] == SENT).all())
        self.calls += rc == 0
        return rc

    def kernel(self):
        if self.which == COND0:
            return 'film_cond0_bwd_kernel'
        return 'film_cond_bwd_kernel<true>' if self.bits is not None else 'film_cond_bwd_kernel<false>'

    def bars(self):
        """Both bars of every tensor the call produced (dw0 after self.calls accumulating calls); what it must not touch is asserted here."""
        d, res = self.d, {}
        got = dict(dk3=self.dk3)
        if self.with_dexc:
            got['dexc'] = self.dexc
        else:
            assert bool((self.dexc == SENT).all()), 'dexc = NULL, but the buffer was written'
        if self.with_dw:
            got['dw0'] = self.dw0
        else:
            assert torch.equal(self.dw0.cpu(), d['dw0_start']), 'dw0 = NULL, but the weight gradient buffer was written'
        for k, t in got.items():
            ref, A, n = d['ref'][k], d['A'][k], d['n'][k]
            if k == 'dw0' and self.calls != 1:
                ref, A, n = d['dw0_start'].double() + self.calls * d['grad'], self.calls * A, self.calls * n
            ratio, inexact = elem_check(t, ref, A, n)
            res[k] = dict(rel=rel_l2(t, ref), ratio=ratio, inexact=inexact)
        assert _spare_intact(self.dexc_whole, NV), 'wrote into the spare channels behind dexc'
        assert _spare_intact(self.src_whole, self.src.shape[1]), 'an input buffer was written'
        return res

    def run(self, tag=''):
        rc = self.call()
        assert rc == 0, (rc, mods()[1].lib().tdvc_last_error())
        assert self.guard_ok, f'wrote outside the {self.query}-byte workspace'
        want = {self.kernel()} | ({FOLD} if self.with_ws else set()) | ({SLAB} if self.with_dw else set())
        assert self.names == want, (self.name, self.which, sorted(self.names), sorted(want))
        res = self.bars()
        assert_bars(res, f'{self.kernel()}: {self.name}{tag}')
        if self.with_dw:      # the embedding window really is part of the checked tensor
            assert int((self.d['A']['dw0'] == 0).sum()) == self.nc * (self.nc - NV) * 3
        WORST.note(self.kernel(), res, self.name)
        return res


def _ids(rows):
    return [f'{n}-{w}' for n, w in rows]


@pytest.mark.parametrize('name,which', ROWS, ids=_ids(ROWS))
def test_cond_bwd_edge(name, which, dev):
    """Every row of the table on both entry points: dexc, dk3, dW0 within both bars, the exact kernels by trace."""
    e = CondEdge(name, which, dev)
    e.run()
    if name == 'views' and which == FUSED:      # once more with cv0 one float into a flat buffer: no alignment is required of it
        e = CondEdge(name, which, dev, cv0_unaligned=True)
        e.run(' (cv0 4 bytes off alignment)')
        assert _spare_intact(e.cv0_whole, e.nc)


@pytest.mark.parametrize('name,which', ROWS, ids=_ids(ROWS))
def test_cond_bwd_edge_poisoned_lds(name, which, dev):
    """Every row once more on NaN-poisoned LDS: the zero rows >= n_cond of the staged W2^T chunk, of the W0 window and of the sign-word
    table, the pad columns of the staging tiles and the sign words past the last one must come from the kernel, not from what LDS held."""
    poison_lds(dev)
    e = CondEdge(name, which, dev)
    e.run(' (poisoned LDS)')
    assert all(bool(torch.isfinite(t).all()) for t in (e.dk3, e.dw0) + ((e.dexc,) if e.with_dexc else ()))


@pytest.mark.parametrize('name', BITS_ROWS)
def test_sign_bits_equal_fp32_mask(name, dev):
    """film_cond_bwd_kernel<true> against <false> on the same data: only the mask source differs, so dexc, dk3 and dW0 (summed in a fixed
    order through the workspace) are the same bits."""
    a, b = CondEdge(name, FUSED, dev), CondEdge(name, FUSED, dev, mask='fp32')
    a.run(); b.run(' (fp32 mask)')
    assert a.kernel() == 'film_cond_bwd_kernel<true>' and b.kernel() == 'film_cond_bwd_kernel<false>'
    for k in ('dexc', 'dk3', 'dw0'):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y), (name, k, int((x != y).sum()), float((x - y).abs().max()))


@pytest.mark.parametrize('which', [FUSED, COND0])
def test_dw0_accumulates_across_calls(which, dev):
    """Two calls onto the same dw0: dw0_start + 2 * grad within the bound of the doubled sum; dexc and dk3 are overwritten, not
    accumulated: the same bits after the second call."""
    e = CondEdge('seam_T64', which, dev)
    e.run()
    dexc1, dk31 = e.dexc_whole.clone(), e.dk3.clone()
    e.run(' (second call onto the same dw0)')
    assert e.calls == 2
    assert torch.equal(e.dexc_whole, dexc1) and torch.equal(e.dk3, dk31)


def _src(e, suffix=''):
    return ('dgb' if e.which == FUSED else 'dcv') + suffix


# what, entry points, changed argument fields (callables get the case; 'no_ws' / 'short_ws' change the workspace), return code
REFUSALS = [
    ('T6', 'both', dict(T=6), EUNSUPPORTED),
    ('T2', 'both', dict(T=2), EUNSUPPORTED),
    ('n_var4', 'both', dict(n_var=4), EUNSUPPORTED),
    ('nc138', 'both', dict(n_cond=138), EUNSUPPORTED),
    ('nc148', 'both', dict(n_cond=148), EUNSUPPORTED),
    ('nc8', 'both', dict(n_cond=8), EUNSUPPORTED),
    ('src_misaligned', 'both', lambda e: {_src(e): e.src.data_ptr() + 4}, EUNSUPPORTED),
    ('exc_misaligned', 'both', lambda e: dict(exc=e.exc.data_ptr() + 4), EUNSUPPORTED),
    ('dexc_misaligned', 'both', lambda e: dict(dexc=e.dexc.data_ptr() + 4), EUNSUPPORTED),
    ('src_bs_mod4', 'both', lambda e: {_src(e, '_bs'): e.src.stride(0) + 2}, EUNSUPPORTED),
    ('exc_bs_mod4', 'both', lambda e: dict(exc_bs=e.exc.stride(0) + 2), EUNSUPPORTED),
    ('dexc_bs_mod4', 'both', lambda e: dict(dexc_bs=e.dexc.stride(0) + 2), EUNSUPPORTED),
    ('dw0_without_workspace', 'both', 'no_ws', EWORKSPACE),
    ('workspace_4_bytes_short', 'both', 'short_ws', EWORKSPACE),
    ('C2_16', FUSED, dict(C2=16), EUNSUPPORTED),
    ('C2_48', FUSED, dict(C2=48), EUNSUPPORTED),
    ('bits_T36', FUSED, dict(T=36), EUNSUPPORTED),
    ('no_mask_source', FUSED, dict(cv0=None, cv0_sign_bits=None), EINVAL),
]


def _refusal(what, which, dev):
    _, _, change, code = next(r for r in REFUSALS if r[0] == what)
    e = CondEdge(REFUSAL_BASE[0], which, dev, mask='bits' if what == 'bits_T36' else None)
    over = change(e) if callable(change) else change if isinstance(change, dict) else {}
    rc = e.call(with_ws=change != 'no_ws', ws_short=4 if change == 'short_ws' else 0, **over)
    torch.cuda.synchronize()
    assert rc == code, (what, which, rc, mods()[1].lib().tdvc_last_error())
    assert not e.names, sorted(e.names)
    assert e.guard_ok and bool((e.dexc_whole == SENT).all()) and bool((e.dk3 == SENT).all()), 'a refused call wrote an output'
    assert torch.equal(e.dw0.cpu(), e.d['dw0_start']), 'a refused call wrote dw0'


@pytest.mark.parametrize('what', [r[0] for r in REFUSALS])
def test_fused_refusals(what, dev):
    """tdvc_film_cond_bwd outside its contract: the return code, nothing launched, dexc / dk3 / the workspace guard still SENT, dw0 untouched."""
    _refusal(what, FUSED, dev)


@pytest.mark.parametrize('what', [r[0] for r in REFUSALS if r[1] == 'both'])
def test_cond0_refusals(what, dev):
    """The same for tdvc_film_cond0_bwd."""
    _refusal(what, COND0, dev)


def test_zz_worst_error_by_kernel():
    """Prints the worst err / bound per kernel and tensor over the cases that ran in this session (asserted case by case)."""
    WORST.report()
