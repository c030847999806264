"""Edge geometry of the GENERIC conv family against float64: conv_gemm_kernel<MODE,...> and its scalar twin (conv_mfma.hip),
conv_wgrad_kernel<MODE,M_REP,J> / conv_wgrad_scalar_kernel, the small-group kernels at their boundary, and the slab folds
(immediate and deferred) that end every weight-grad call.

The stride-1 lean family has test_lean_conv_edges_gpu.py (forward and input-grad; its weight-grad kernels: test_lean_wgrad_edges_gpu.py)
and test_kernel_instances_gpu.py; the edge suites drive the Edge class of conv_edge.py, with the bars and buffers of edge_support.py. This file gives the generic family the same treatment:

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

import pytest
import torch

from common import rel_l2, traced
from conv_edge import Edge, _conv64
from conv_ops_cases import film_block_errors
from edge_support import EUNSUPPORTED, EWORKSPACE, SENT, TOL, assert_bars, elem_check, mods, poison_lds, stream
from small_group_cases import WGRAD_MFMA_J, small_group_desc

pytestmark = pytest.mark.gpu

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
GEMM_CFG = {0: (1, 4, 1, 4), 1: (2, 4, 1, 4), 2: (4, 4, 1, 4), 3: (1, 1, 1, 4), 4: (1, 4, 4, 1)}
MODE_DIRECT, MODE_DOWN, MODE_UP = 0, 1, 2


def make_edge(name, dev, generic=0):
    geom = LEAN_GEOM if name == LEAN_GEOM[0] else GEOM[name]
    return Edge(geom, dev, generic, **OPTS[name])


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
    if small_group_desc(geom):
        fwd, dg = f'small_group_fwd_kernel<{s}>', f'small_group_dgrad_kernel<{s}>'
    else:
        fwd, dg = f'conv_gemm_kernel<{modes[0]},', f'conv_gemm_kernel<{modes[1]},'
    J = k if s == 1 else -(-k // s)
    tout = e.tout
    if small_group_desc(geom) and 4 * k <= 252 and 4 * (T + 2 * p + s) <= 6 * 256 and 4 * tout <= 256:
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
    L = mods()[1]
    poison_lds(dev)
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
    L = mods()[1]
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
        errs = film_block_errors(cfg, dev, B=2)
    assert max(errs.values()) < TOL, errs
    off_route = [n for n in tr.names if n.startswith(('conv_lean_kernel', 'film_block_fwd_kernel'))]
    assert not off_route and any(n.startswith('conv_gemm_kernel<0,') for n in tr.names), sorted(tr.names)


@pytest.mark.parametrize('name', ['down_r5', 'up_r5', 'grp3', 'sg_g16_k48_s8', 'sg_g16_k41_T250', LEAN_GEOM[0]])
def test_wgrad_workspace_contract(name, dev):
    """One byte less than tdvc_conv_wgrad_workspace() is refused with TDVC_EWORKSPACE, nothing launched, dw / dbias bit-identical.
    The small-group launcher declines instead: where the next route needs no more than what is there, its result must be right.
    dw = NULL with dbias given produces the bias gradient alone."""
    L = mods()[1]
    if name == 'sg_g16_k41_T250':      # inside the small-group weight-grad's contract (Tout <= 64): its launcher sees the short workspace
        e = Edge(('sg_g16_k41_T250', 64, 64, 41, 4, 20, 1, 16, False, False, 0, 250), dev, post=1)
    else:
        e = make_edge(name, dev)
    e.fwd()
    rc = e.wgrad_call(ws_bytes=-1 + L.lib().tdvc_conv_wgrad_workspace(C.byref(e.spec.desc(e.B, e.T))))
    torch.cuda.synchronize()
    assert e.query > 0 and e.guard_ok
    if rc == 0:      # the small-group slabs are smaller than those of the route behind it, or that route needs none
        assert small_group_desc(e.geom), 'only the small-group launcher may decline a short workspace'
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
    ops, L, arena = mods()
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
    ops, L, _ = mods()
    lib = L.lib()
    st = stream(dev)
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
    ops, L, _ = mods()
    lib = L.lib()
    st = stream(dev)
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
