"""Edge geometry of the MFMA kernels for grouped stride-4 convs with 4 input and 16 output channels per group
(group16_fwd_kernel / group16_dgrad_kernel, conv_small_group.hip: discriminator layers 1-3) against float64, through the Edge
class of conv_edge.py (rules: test_generic_conv_edges_gpu.py): both bars on every tensor (rel-L2 < 2e-5 and the element-wise summation bound), the
kernel names of every call, NaN-poisoned LDS before every case.

Every case runs the forward, the input-grad twice (dy_xf NONE and MASK_LRELU, both with the PLAIN epilogue the route takes) and the
weight-grad, which stays on its present route. The input-grad goes straight through conv_dgrad_raw (plain_dgrad of conv_edge.py), because Edge.dgrad() ties the
dy transform to the case's `post` option: its float64 reference is the transposed conv of dy' = dy * out_scale (* lrelu'(aux)),
with aux = the stored forward output, whatever activation the case has.

Both kernels walk their reduction in the generic MFMA kernel's order (taps outside, four reduced channels per MFMA), so the route
changes no bit of a result: test_group16_bits_of_generic_route compares y and dx with the small-group off switch set and cleared.

The shapes that must NOT take the new route (pad % 4 != 0, K > 44, stride 2, a running sum on either pass, the small-group off
switch) assert the generic conv_gemm_kernel by name, and right results.
"""
import pytest
import torch

from common import traced
from conv_edge import Edge, plain_dgrad
from edge_support import assert_bars, mods, poison_lds

pytestmark = pytest.mark.gpu

# Mirror of the grid rule (conv_small_group.hip: g16_tpr): 256 CUs x 14 resident one-wave blocks; a wave walks
# ceil(tiles of the launch / 3584) consecutive 64-column tiles, evened out over the runs of a row.
G16_WAVES = 256 * 14


def tiles_per_run(B, G, ntile):
    tpr = min(max(-(-B * G * ntile // G16_WAVES), 1), ntile)
    nruns = -(-ntile // tpr)
    return -(-ntile // nruns)


# 2 samples x 16 groups need 113 tiles before a wave walks two of them; 113 is odd, so the last run of a row is one tile, and the last
# tile holds 8 of its 64 columns (forward: Tout = 7176) or 13 (input-grad: M = 7181)
WALK_T = 28704


def geom(name, cin, cout, K, s, pad, groups, T):
    return (name, cin, cout, K, s, pad, 1, groups, False, False, 0, T)


# name -> (geometry, Edge options, out_scale)
CASES = {
    'one_tile': (geom('one_tile', 16, 64, 41, 4, 20, 4, 256), dict(B=3, post=1), 1.0),                  # Tout = 64
    'one_over': (geom('one_over', 16, 64, 41, 4, 20, 4, 260), dict(B=3, post=1), 1.0),                  # Tout = 65: one step into the next tile
    'unaligned': (geom('unaligned', 16, 64, 41, 4, 20, 4, 250), dict(B=3, post=1), 1.0),                # Tout = 63, Tin % 4 = 2: scalar y, float2 dx
    'odd_T': (geom('odd_T', 16, 64, 41, 4, 20, 4, 253), dict(B=3, post=1), 1.0),                        # Tin odd: scalar dx stores
    'walk': (geom('walk', 64, 256, 41, 4, 20, 16, WALK_T), dict(B=2, pre=1), 1.0),
    'k44': (geom('k44', 16, 64, 44, 4, 20, 4, 256), dict(B=3, post=1), 1.0),                            # no zero taps
    'k9': (geom('k9', 16, 64, 9, 4, 4, 4, 256), dict(B=3, post=1), 1.0),                                # J = 3
    'views': (geom('views', 16, 64, 41, 4, 20, 4, 264), dict(B=3, views=True, bias=False, with_db=False), 0.5),      # Tout = 66: float2 y with a scalar tail
    'g5': (geom('g5', 20, 80, 41, 4, 20, 5, 256), dict(B=3, post=1), 1.0),
}
OFF_ROUTE = ('conv_gemm_kernel', 'weight_repack_kernel', 'conv_scalar_kernel', 'small_group_')


def make_case(name, dev):
    g, opts, out_scale = CASES[name]
    e = Edge(g, dev, **opts)
    e.out_scale = out_scale      # Edge ties out_scale to `add`; the forward call, its reference and dy_xf all read the attribute
    return e


def assert_route(names, kernel, what):
    assert any(n.startswith(kernel) for n in names), (what, kernel, sorted(names))
    assert not any(n.startswith(OFF_ROUTE) for n in names), (what, sorted(names))


@pytest.mark.parametrize('name', list(CASES))
def test_group16_edge(name, dev):
    """Forward and input-grad on the new kernels (by name; no generic kernel, no weight repack), weight-grad on its present route."""
    poison_lds(dev)
    e = make_case(name, dev)
    (_, cin, cout, k, s, p, d, g, _, _, _, T) = e.geom
    if name == 'walk':      # the shape really makes a wave walk two tiles, and the last walk of a row is partial, in both kernels
        for ncol in (e.tout, (T - 1 + p) // 4 + 1):
            ntile = -(-ncol // 64)
            tpr = tiles_per_run(e.B, g, ntile)
            assert tpr >= 2 and ntile % tpr != 0, (ncol, ntile, tpr)
    res = e.fwd()
    assert_route(e.names['fwd'], 'group16_fwd_kernel', f'{name} fwd')
    for masked in (False, True):
        r, names = plain_dgrad(e, masked)
        res.update(r)
        assert_route(names, 'group16_dgrad_kernel', f'{name} dgrad masked={masked}')
    res.update(e.wgrad())
    assert not any(n.startswith('group16_') for n in e.names['wgrad']), sorted(e.names['wgrad'])
    assert_bars(res, f'group16 {name}')


# off the route by descriptor or by operands: the generic MFMA kernel, forward MODE_DOWN (1) and input-grad MODE_UP (2)
DECLINE = {
    'pad18': (geom('pad18', 16, 64, 41, 4, 18, 4, 256), dict(B=3, post=1)),
    'k45': (geom('k45', 16, 64, 45, 4, 20, 4, 256), dict(B=3, post=1)),
    'stride2': (geom('stride2', 16, 64, 41, 2, 20, 4, 256), dict(B=3, post=1)),
    'add': (geom('add', 16, 64, 41, 4, 20, 4, 256), dict(B=3, add=True)),      # a running sum on the forward and on the input-grad
    'knob_off': (geom('knob_off', 16, 64, 41, 4, 20, 4, 256), dict(B=3, post=1)),
}


@pytest.mark.parametrize('name', list(DECLINE))
def test_group16_declines_to_generic(name, dev):
    L = mods()[1]
    poison_lds(dev)
    g, opts = DECLINE[name]
    e = Edge(g, dev, **opts)
    if name == 'knob_off':
        L.lib().tdvc_debug_knob(2, 1)
    try:
        res = e.fwd()
        res.update(e.dgrad())
    finally:
        L.lib().tdvc_debug_knob(2, 0)
    assert_bars(res, f'group16 decline {name}')
    for what, prefix in (('fwd', 'conv_gemm_kernel<1,'), ('dgrad', 'conv_gemm_kernel<2,')):
        assert any(n.startswith(prefix) for n in e.names[what]), (name, what, sorted(e.names[what]))
        assert not any(n.startswith('group16_') for n in e.names[what]), (name, what, sorted(e.names[what]))


@pytest.mark.parametrize('name', ['one_over', 'unaligned', 'k9', 'views', 'walk'])
def test_group16_bits_of_generic_route(name, dev):
    """y and dx (dy_xf NONE and MASK_LRELU) are bit-identical with the route on and off (tdvc_debug_knob(2, 1): conv_gemm_kernel)."""
    ops, L, _ = mods()
    poison_lds(dev)
    e = make_case(name, dev)
    T = e.geom[-1]
    post = (L.POST_NONE, L.POST_LRELU)[e.post]
    out = {}
    try:
        for off in (0, 1):
            L.lib().tdvc_debug_knob(2, off)
            with traced() as tr:
                y = ops.conv_fwd_raw(e.spec, e.xv, e.x_xf, post=post, out_scale=e.out_scale).clone()
                dx = [ops.conv_dgrad_raw(e.spec, e.dyv, xf, T, L.DG_PLAIN).clone()
                      for xf in (ops._xf(scale=e.out_scale), ops._xf(L.XF_MASK_LRELU, scale=e.out_scale, aux=y))]
            assert any(n.startswith('conv_gemm_kernel' if off else 'group16_') for n in tr.names), (off, sorted(tr.names))
            assert not any(n.startswith('group16_' if off else 'conv_gemm_kernel') for n in tr.names), (off, sorted(tr.names))
            out[off] = [y] + dx
    finally:
        L.lib().tdvc_debug_knob(2, 0)
    for what, a, b in zip(('y', 'dx', 'dx masked'), out[0], out[1]):
        assert torch.equal(a, b), (name, what, int((a != b).sum()), float((a - b).abs().max()))
