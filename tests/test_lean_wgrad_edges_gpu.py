"""Edge geometry of the stride-1 'same' WEIGHT-GRAD family against float64: conv_wgrad_lean_kernel<1,1,J,D> (narrow layers),
conv_wgrad_tile_kernel<M,C,J,D,SCAL> in its two staging modes, conv_wgrad_pipe_kernel<M,C,J,D,XFILM> and the split-bf16
conv_wgrad_x6_kernel, each with the slab fold (bias partials behind the weights) that ends the call.

Same rules as test_generic_conv_edges_gpu.py; this file drives the Edge class of conv_edge.py: fp32-valued inputs, float64 autograd on the same numbers,
dw / db ACCUMULATED onto random values, the workspace exactly tdvc_conv_wgrad_workspace() bytes inside a SENT-guarded buffer, the
mask of a post-LeakyReLU layer taken from the GPU's own stored output, and both bars on every tensor:
    rel-L2 < 2e-5   and   |got - ref| <= (n + 8) * 2^-23 * A + 2^-22 * |ref|,   n = B * Tout for dw and db,
with equality where A == 0 (dw columns outside a w_cin window still hold dw0). The split-bf16 kernel keeps the bound: three exact
bf16 pieces per operand and six of the nine piece products leave at most about 2 * 2^-24 relative error per product, i.e. at most
2^-23 * A in the sum, inside the slack of 8; the accumulation is fp32 MFMA. The FiLM cases take A from H = |h| (1 + |gamma|) + |beta|
and n + 12 (derivation: Edge's docstring).

What the shapes are for: small launches give every block exactly one chunk. The table below holds the smallest shapes at which a
block walks several chunks (tpb >= 2; the pipe kernel's double buffer over odd and even walk lengths and its weightless repeat
commit), crosses from one sample into the next, ends in a 4- or 8-column chunk, stages reflect halos that overlap, runs the
element-wise fallback of the tile kernel (FiLM on rows that are not 16-byte aligned), takes the contiguous-run staging at T = 1,
sits at both ends of the split-bf16 kernel's Cin window, and gets dbias = NULL. Every case asserts by trace the exact weight-grad
instance, that the slab fold ran, and that the generic weight-grad kernels did not; forward and input-grad come for free with their
own bars and their route (conv_lean_kernel or conv_gemm_kernel<0,...>, by the rule of conv_api.hip).

The table is CASES of wgrad_cases.py; test_wgrad_plan_cpu.py checks the plan figures quoted there (slabs, chunks per block, straddling) on the CPU.
"""
import pytest
import torch

from conv_edge import Edge
from edge_support import Worst, assert_bars, poison_lds
from wgrad_cases import CASES, NARROW, expected_route

pytestmark = pytest.mark.gpu

NO_DB_RERUN = ['pipe_72x40_k3', 'x6_144_32_T64', 'tile_mask_64_k5_T260', 'tile_d5_k5_T63']      # run once more with dbias = NULL
WIDE = [n for n, c in CASES.items() if c[2] != NARROW]                 # row tile 32 or 64: once more on poisoned LDS
WORST = Worst()                                                        # kernel class -> tensor -> (err / bound, case)


def make_case(name, dev, **override):
    geom, opts, _, _ = CASES[name]
    return Edge(geom, dev, **{**dict(wt=True), **opts, **override})


def run_case(name, dev, tag='', **override):
    """fwd, dgrad, wgrad of one case: both bars on every tensor, the routes of all three calls by trace, untouched dw columns."""
    geom, opts, kclass, inst = CASES[name]
    e = make_case(name, dev, **override)
    res = e.run_all()
    assert_bars(res, f'{kclass}: {name}{tag}')
    for what in ('fwd', 'dgrad'):
        prefix = expected_route(e, what)
        assert any(n.startswith(prefix) for n in e.names[what]), (name, what, prefix, sorted(e.names[what]))
    wg = e.names['wgrad']
    assert inst in wg, (name, inst, sorted(wg))
    assert not any(n.startswith(('conv_wgrad_kernel<', 'conv_wgrad_scalar_kernel<')) for n in wg), sorted(wg)
    assert 'slab_reduce_multi_kernel' in wg, sorted(wg)
    assert wg - {inst, 'slab_reduce_multi_kernel'} == set(), (name, sorted(wg))      # nothing else: no second route, no bias-grad kernel
    if e.spec.w_cin:
        outside = torch.ones(e.spec.w_cin, dtype=torch.bool)
        outside[e.win] = False
        assert bool(outside.any()) and torch.equal(e.dw.cpu()[:, outside], e.dw0[:, outside]), 'dw columns outside the w_cin window were touched'
    WORST.note(kclass, res, name)
    return e, res


@pytest.mark.parametrize('name', list(CASES))
def test_wgrad_edge(name, dev):
    """Every case of the table: y, dx, dw, db (dgb with FiLM) within both bars, the exact weight-grad instance by trace."""
    run_case(name, dev)


@pytest.mark.parametrize('name', NO_DB_RERUN)
def test_wgrad_edge_without_dbias(name, dev):
    """dbias = NULL on the pipe, the split-bf16 and both staging modes of the tile kernel (the table has it on the narrow and the FiLM
    pipe instance): db stays db0 bit for bit, no bias-gradient kernel runs, dw passes both bars, the workspace guard holds."""
    e, res = run_case(name, dev, tag=' (dbias = NULL)', with_db=False)
    assert 'db' not in res and torch.equal(e.db.cpu(), e.db0)


@pytest.mark.parametrize('name', WIDE)
def test_wgrad_edge_poisoned_lds(name, dev):
    """The kernels with a 32- or 64-row tile once more on NaN-poisoned LDS: a fragment read of a word that was never staged (partial
    row and column tiles, the tail of a short last chunk, the second stage of the double buffer) turns into NaN."""
    poison_lds(dev)
    run_case(name, dev, tag=' (poisoned LDS)')


def test_zz_worst_error_by_kernel():
    """Prints the worst err / bound per kernel class and tensor over the cases that ran in this session (asserted case by case)."""
    WORST.report()
