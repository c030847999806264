"""Edge geometry of the stride-1 'same' WEIGHT-GRAD family against float64: conv_wgrad_lean_kernel<1,1,J,D> (narrow layers),
conv_wgrad_tile_kernel<M,C,J,D,SCAL> in its two staging modes, conv_wgrad_pipe_kernel<M,C,J,D,XFILM> and the split-bf16
conv_wgrad_x6_kernel, each with the slab fold (bias partials behind the weights) that ends the call.

Same rules as test_generic_conv_edges_gpu.py, whose Edge this file drives: fp32-valued inputs, float64 autograd on the same numbers,
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

test_wgrad_plan_cpu.py imports CASES and checks the plan figures quoted here (slabs, chunks per block, straddling) on the CPU.
"""
import pytest
import torch

from test_generic_conv_edges_gpu import Edge, _mods, assert_bars

pytestmark = pytest.mark.gpu

NARROW, PIPE, PIPE_FILM, X6, TILE1, TILE2 = 'narrow', 'pipe', 'pipe-FiLM', 'x6', 'tile SCAL=1', 'tile SCAL=2'


def _g(name, cin, cout, k, pad, dil, reflect, T):
    """Edge's geometry tuple of a stride-1 conv."""
    return (name, cin, cout, k, 1, pad, dil, 1, reflect, False, 0, T)


# name: (geometry, Edge options, kernel class, weight-grad instance in the trace's spelling)
CASES = {c[0][0]: c for c in [
    # ---- narrow: conv_wgrad_lean_kernel<1,1,J,D>, 256-step chunks, slabs = B * groups per sample
    # odd T: scalar staging; the last chunk has 45 columns; MASK_LRELU stream on dy
    (_g('nar_d0_k15_T301', 1, 16, 15, 7, 1, True, 301), dict(post=1), NARROW, 'conv_wgrad_lean_kernel<1,1,15,1>'),
    # one chunk holds both mirror folds; the x window runs 150 columns past T
    (_g('nar_c16_k11_d5_T132', 16, 16, 11, 25, 5, True, 132), dict(pre=1), NARROW, 'conv_wgrad_lean_kernel<1,1,11,5>'),
    # chunk 0 on the padding path, chunks 1-3 on the vector path, chunk 4 has 4 columns; 10 slabs
    (_g('nar_c16_k7_d3_T1028', 16, 16, 7, 9, 3, True, 1028), dict(pre=1, B=2), NARROW, 'conv_wgrad_lean_kernel<1,1,7,3>'),
    # batch stride wider than contiguous, still aligned
    (_g('nar_c8_k5_T500_views', 8, 8, 5, 2, 1, False, 500), dict(pre=1, add=True, views=True), NARROW, 'conv_wgrad_lean_kernel<1,1,5,1>'),
    (_g('nar_c16_k3_unaligned', 16, 16, 3, 1, 1, False, 260), dict(unaligned=True), NARROW, 'conv_wgrad_lean_kernel<1,1,3,1>'),
    # 2070 blocks -> tpb = 2: 10 chunks in 5 groups per sample, 115 slabs, the last chunk has 4 columns; dw columns 0..127 stay dw0
    (_g('nar_var_window_tpb2', 8, 136, 3, 1, 1, False, 2308), dict(B=23, w_cin=136, w_cin_off=128, with_db=False), NARROW,
     'conv_wgrad_lean_kernel<1,1,3,1>'),
    # tpb = 2 WITH a bias gradient (the partial sums of a block's two chunks add up), 9 chunks per sample: the last group of each
    # sample is the 4-column chunk alone; 130 slabs
    (_g('nar_tpb2_odd_chunks', 8, 136, 3, 1, 1, False, 2052), dict(B=26, pre=1), NARROW, 'conv_wgrad_lean_kernel<1,1,3,1>'),
    # ---- pipe: conv_wgrad_pipe_kernel<M,C,J,D,XFILM>, aligned rows, dy plain
    # second row tile has 8 rows, 40 of 64 columns, last chunk 4 wide; 15 slabs
    (_g('pipe_72x40_k3', 40, 72, 3, 1, 1, False, 260), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<2,2,3,1,false>'),
    # 24 rows keep it off the split-bf16 kernel; 136 = 4 1/4 column tiles; 27 slabs
    (_g('pipe_24x136_k3', 136, 24, 3, 1, 1, False, 520), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<1,1,3,1,false>'),
    # 75 chunks, tpb = 2, 38 slabs, 15 chunks per sample: block 7 crosses samples 0 / 1, the last block has one chunk, reflect halos
    (_g('pipe_straddle_k7_d3', 128, 128, 7, 9, 3, True, 900), dict(pre=1, B=5), PIPE, 'conv_wgrad_pipe_kernel<2,1,7,3,false>'),
    # 132 chunks, tpb = 3, 44 slabs, 44 chunks per sample (44 % 3 != 0: straddles); odd walk length of the double buffer
    (_g('pipe_deep_k3_d3', 128, 256, 3, 3, 3, True, 2756), dict(), PIPE, 'conv_wgrad_pipe_kernel<2,2,3,3,false>'),
    # the widest span; the last chunk has 8 columns
    (_g('pipe_k11_d5_64', 64, 64, 11, 25, 5, True, 200), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<1,1,11,5,false>'),
    # T <= 128 admitted as "wide"
    (_g('pipe_pw_96x100', 100, 96, 1, 0, 1, False, 68), dict(), PIPE, 'conv_wgrad_pipe_kernel<2,2,1,1,false>'),
    # beta planes start at channel 40 (no tile multiple), partial tiles both ways
    (_g('pipe_film_40', 40, 40, 1, 0, 1, False, 260), dict(film=True), PIPE_FILM, 'conv_wgrad_pipe_kernel<2,2,1,1,true>'),
    (_g('pipe_film_32', 32, 32, 1, 0, 1, False, 128), dict(film=True, B=2, with_db=False), PIPE_FILM, 'conv_wgrad_pipe_kernel<1,1,1,1,true>'),
    # ---- split-bf16: conv_wgrad_x6_kernel, 3 taps, 65 .. 144 input channels, T % 4 == 0, T >= 64
    # lower Cin end; 8 row blocks -> 99 chunks, tpb = 2, 50 slabs, 33 chunks per sample (straddles), the last chunk has 4 columns
    (_g('x6_65_256_T1028', 65, 256, 3, 1, 1, False, 1028), dict(pre=1), X6, 'conv_wgrad_x6_kernel'),
    # upper Cin end, minimum T
    (_g('x6_144_32_T64', 144, 32, 3, 1, 1, False, 64), dict(pre=1, B=5), X6, 'conv_wgrad_x6_kernel'),
    (_g('x6_136_64_T68_views', 136, 64, 3, 1, 1, False, 68), dict(views=True), X6, 'conv_wgrad_x6_kernel'),
    # T % 4 != 0: must NOT be the split-bf16 kernel
    (_g('x6_miss_T66', 136, 32, 3, 1, 1, False, 66), dict(pre=1), TILE1, 'conv_wgrad_tile_kernel<1,1,3,1,1>'),
    # ---- tile: conv_wgrad_tile_kernel<M,C,J,D,SCAL>
    # contiguous-run staging with a MASK_LRELU stream
    (_g('tile_d5_k5_T63', 128, 128, 5, 2, 1, False, 63), dict(post=1), TILE2, 'conv_wgrad_tile_kernel<2,1,5,1,2>'),
    # a batch stride % 4 != 0 breaks the contract of the contiguous-run staging
    (_g('tile_d5_k5_T63_views', 128, 128, 5, 2, 1, False, 63), dict(post=1, views=True), TILE1, 'conv_wgrad_tile_kernel<2,1,5,1,1>'),
    # aligned, but the dy mask keeps it off the pipe kernel; 5 chunks
    (_g('tile_mask_64_k5_T260', 64, 64, 5, 2, 1, False, 260), dict(post=1), TILE1, 'conv_wgrad_tile_kernel<2,1,5,1,1>'),
    (_g('tile_unaligned_48_k3', 48, 48, 3, 1, 1, False, 260), dict(unaligned=True, pre=1), TILE1, 'conv_wgrad_tile_kernel<2,2,3,1,1>'),
    # chunk mode 0, the element-wise fallback: FiLM prologue on rows that are not 16-byte aligned
    (_g('tile_film_64_T50', 64, 64, 1, 0, 1, False, 50), dict(film=True), TILE1, 'conv_wgrad_tile_kernel<2,2,1,1,1>'),
    # the two mirrors overlap
    (_g('tile_reflect_k11_d5_T30', 64, 64, 11, 25, 5, True, 30), dict(pre=1), TILE1, 'conv_wgrad_tile_kernel<2,1,11,5,1>'),
    # N = 1
    (_g('tile_pw_32x64_T1', 32, 64, 1, 0, 1, False, 1), dict(B=5), TILE2, 'conv_wgrad_tile_kernel<2,1,1,1,2>'),
    (_g('tile_pw_40x64_T1', 40, 64, 1, 0, 1, False, 1), dict(B=5), TILE1, 'conv_wgrad_tile_kernel<2,2,1,1,1>'),
    # the k3 fallback route of film_cond; dw columns 128..135 stay dw0
    (_g('tile_k3_T3_window', 128, 136, 3, 1, 1, False, 3), dict(B=4, w_cin=136, w_cin_off=0), TILE1, 'conv_wgrad_tile_kernel<2,2,3,1,1>'),
]}
NO_DB_RERUN = ['pipe_72x40_k3', 'x6_144_32_T64', 'tile_mask_64_k5_T260', 'tile_d5_k5_T63']      # run once more with dbias = NULL
WIDE = [n for n, c in CASES.items() if c[2] != NARROW]                 # row tile 32 or 64: once more on poisoned LDS
WORST = {}                                                             # kernel class -> tensor -> (err / bound, case)


def expected_route(e, what):
    """Kernel name prefix of a case's forward ('fwd') or input-grad ('dgrad'), by the rule of conv_api.hip: the lean kernel takes
    channel counts that are multiples of 4 (Cin forward, Cout backward, with the slot's transposed weight copy) at T <= 80 or at
    T % 4 == 0 with 16-byte aligned operands; it has no instance for a mask prologue together with a mask epilogue. The operator
    layer sends a plain 3-tap forward with 65 .. 160 input channels, Cout % 32 == 0 and T >= 128 to the split-bf16 forward."""
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = e.geom
    aligned = T % 4 == 0 and not e.unaligned
    if what == 'fwd' and k == 3 and d == 1 and p == 1 and not e.spec.w_cin and 64 < cin <= 160 and cout % 32 == 0 and T >= 128 and aligned \
            and not e.post and e.add_y is None and not e.film:
        return 'conv_fwd_x6_kernel<'
    ch = cin if what == 'fwd' else cout
    lean = ch % 4 == 0 and (T <= 80 or aligned)
    if what == 'dgrad' and e.post and e.pre:
        lean = False
    return 'conv_lean_kernel' if lean else 'conv_gemm_kernel<0,'


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
    for k, v in res.items():
        if v['ratio'] >= WORST.setdefault(kclass, {}).get(k, (-1.0, ''))[0]:
            WORST[kclass][k] = (v['ratio'], name)
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
    L = _mods()[1]
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
    run_case(name, dev, tag=' (poisoned LDS)')


def test_zz_worst_error_by_kernel():
    """Prints the worst err / bound per kernel class and tensor over the cases that ran in this session (asserted case by case)."""
    for kclass, per in WORST.items():
        print(f'[edge] worst {kclass}: ' + '  '.join(f'{k} {r:.3f} ({n})' for k, (r, n) in sorted(per.items())))
