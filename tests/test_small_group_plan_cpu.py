"""The case table of test_small_group_conv_edges_gpu.py (the 4 -> 4-channels-per-group kernels of conv_small_group.hip) and the host
side of what those cases rely on. tdvc_conv_wgrad_workspace() is host code: no GPU needed.

  * the workspace query covers the small-group weight-grad's slabs, nsplit * ([G][16][K] weights + [G][4] bias partials) floats with
    nsplit = 4 from B = 8 on, and is exactly that where the route behind it accumulates into dw directly (no MFMA instance for
    J = ceil(K / s));
  * the weight-grad kernel each case asserts by trace is the one a Python mirror of launch_small_group_wgrad's contract names, and
    the geometric figures the table quotes beside each case (Tout, the padded row XW, the input-grad's column count M) are what the
    geometry gives: a case that was edited off its edge fails here, not silently on the GPU.
"""
import ctypes as C
import importlib

import pytest

SG_WGRAD, MFMA_WGRAD, SCALAR_WGRAD = 'small_group_wgrad_kernel', 'conv_wgrad_kernel<1,', 'conv_wgrad_scalar_kernel<'
WGRAD_MFMA_J = (1, 2, 3, 5, 7, 11)      # the generic MFMA weight-grad's instances (conv_mfma.hip: wgrad_mfma_supported)


def geom(name, K, s, pad, T, G=16):
    """(name, cin, cout, K, stride, pad, dil, groups, reflect, transposed, out_pad, T) of a 4 -> 4-channels-per-group conv."""
    return (name, 4 * G, 4 * G, K, s, pad, 1, G, False, False, 0, T)


# name -> (geometry, Edge options, out_scale, weight-grad kernel asserted by trace, (Tout, XW, M) the case is there for)
# XW = T + 2 pad + s: the weight-grad's padded input row (limit 384); M = (T - 1 + pad) / s + 1: columns of the input-grad.
CASES = {
    # Tout = 64: one full forward tile, two input-grad tiles, the weight-grad at its 4 * Tout == 256 limit
    'tile64': (geom('tile64', 41, 4, 20, 256), dict(post=1), 1.0, SG_WGRAD, (64, 300, 69)),
    # Tout = 65: one column in the second tile; the weight-grad declines
    'tile65': (geom('tile65', 41, 4, 20, 260), dict(post=1), 1.0, MFMA_WGRAD, (65, 304, 70)),
    # u0 = 4 m - 18: scalar dx stores; the lane with u0 = -2 writes only t = 0, 1
    'pad18': (geom('pad18', 41, 4, 18, 256), dict(post=1), 1.0, SG_WGRAD, (63, 296, 69)),
    'odd_T': (geom('odd_T', 41, 4, 20, 253), dict(post=1), 1.0, SG_WGRAD, (64, 297, 69)),
    # wider batch strides, planes that are not 16-byte aligned, no bias, dbias = NULL, a dy scale
    'views': (geom('views', 41, 4, 20, 250), dict(views=True, bias=False, with_db=False), 0.5, SG_WGRAD, (63, 294, 68)),
    # 16 K == 768 (forward registers) and 16 J s == 768 (input-grad registers), J = 24
    's2_k48': (geom('s2_k48', 48, 2, 23, 129), dict(post=1), 1.0, SG_WGRAD, (64, 177, 76)),
    # J = 24 with the last tap (k = 47) past K
    's2_k47': (geom('s2_k47', 47, 2, 23, 128), dict(post=1), 1.0, SG_WGRAD, (64, 176, 76)),
    # XW = 384: all six staging roles of the weight-grad full; the forward stages its window (552 positions) in two passes
    's8_xw384': (geom('s8_xw384', 48, 8, 20, 336), dict(post=1), 1.0, SG_WGRAD, (42, 384, 45)),
    # XW = 385: the weight-grad declines; J = 6 has no MFMA instance
    's8_xw385': (geom('s8_xw385', 48, 8, 20, 337), dict(post=1), 1.0, SCALAR_WGRAD, (42, 385, 45)),
    # K < s, J = 1, pad 0: phase 3 of dx is exactly 0
    'k3_s4': (geom('k3_s4', 3, 4, 0, 101), dict(pre=1, post=1), 1.0, SG_WGRAD, (25, 105, 26)),
    'k5_s8': (geom('k5_s8', 5, 8, 2, 64), dict(post=1), 1.0, SG_WGRAD, (8, 76, 9)),
    # Tout = 1: the input is shorter than the kernel
    'T2': (geom('T2', 41, 4, 20, 2), dict(post=1), 1.0, SG_WGRAD, (1, 46, 6)),
    # the last block of forward and input-grad: three live waves, one dead
    'g19': (geom('g19', 41, 4, 20, 250, G=19), dict(post=1), 1.0, SG_WGRAD, (63, 294, 68)),
    # act_in in the forward and the weight-grad
    'pre': (geom('pre', 41, 4, 20, 250), dict(pre=1), 1.0, SG_WGRAD, (63, 294, 68)),
    # POST_TANH in the forward; XF_MASK_TANH keeps input-grad and weight-grad off the route (J = 3: the MFMA weight-grad)
    'tanh': (geom('tanh', 9, 4, 4, 256), dict(post=2), 1.0, MFMA_WGRAD, (64, 268, 65)),
    # strides without a forward / input-grad instance: those launchers decline, the weight-grad takes the stride at run time
    's3': (geom('s3', 7, 3, 3, 100), dict(post=1), 1.0, SG_WGRAD, (34, 109, 35)),
    's5': (geom('s5', 10, 5, 3, 150), dict(post=1), 1.0, SG_WGRAD, (30, 161, 31)),
    's7': (geom('s7', 16, 7, 5, 200), dict(post=1), 1.0, SG_WGRAD, (28, 217, 30)),
}
SPLIT_B = (7, 8, 10, 11)      # the weight-grad's sample split (nsplit = 4 from B = 8 on) runs at the tile64 geometry


def tout_of(g):
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    return (T + 2 * p - (k - 1) - 1) // s + 1


def small_group_desc(g):
    """small_group_ok() of conv_api.hip without its off switches."""
    (_, cin, cout, k, s, p, d, G, reflect, transposed, _, T) = g
    return not transposed and G >= 16 and cin == 4 * G and cout == 4 * G and d == 1 and not reflect and 2 <= s <= 8 and k <= 48


def wgrad_contract(g):
    """launch_small_group_wgrad: a thread per (ci, k) with four idle ones for the bias, six staging roles of 256 for the padded
    rows of the four input channels, one role for the four dy rows."""
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    return 4 * k <= 252 and 4 * (T + 2 * p + s) <= 6 * 256 and 4 * tout_of(g) <= 256


def expected_families(name):
    """Kernel name prefixes of (forward, input-grad with the PLAIN epilogue and dy_xf NONE / MASK_LRELU, weight-grad)."""
    g, opts, _, wg, _ = CASES[name]
    s = g[4]
    if s in (2, 4, 8):
        return f'small_group_fwd_kernel<{s}>', f'small_group_dgrad_kernel<{s}>', wg
    return 'conv_gemm_kernel<1,', 'conv_gemm_kernel<2,', wg      # MODE_DOWN forward, MODE_UP input-grad


def sg_slab_bytes(g, B):
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    return (4 if B >= 8 else 1) * (G * 16 * k + 4 * G) * 4


@pytest.mark.parametrize('name', list(CASES))
def test_case_sits_on_its_edge(name):
    g, opts, out_scale, wg, (tout, xw, m) = CASES[name]
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    assert small_group_desc(g), name
    assert (tout_of(g), T + 2 * p + s, (T - 1 + p) // s + 1) == (tout, xw, m), name
    J = -(-k // s)
    on_route = wgrad_contract(g) and opts.get('post', 0) != 2      # a tanh mask is no operand of the small-group kernels
    want = SG_WGRAD if on_route else (MFMA_WGRAD if J in WGRAD_MFMA_J else SCALAR_WGRAD)
    assert wg == want, (name, wg, want, J)
    # the register and LDS limits of the forward / input-grad launchers: every stride with an instance stays inside them
    if s in (2, 4, 8):
        cs = (64 + J + 1 + 15) // 16 * 16
        assert 16 * k <= 768 and 16 * J * s <= 768 and 4 * (4 * s * cs + 16 * k) * 4 <= 64 * 1024, name


def test_the_limit_cases_are_at_their_limits():
    K = lambda n: CASES[n][0][3]
    S = lambda n: CASES[n][0][4]
    assert 16 * K('s2_k48') == 768 and 16 * -(-K('s2_k48') // 2) * 2 == 768
    assert -(-K('s2_k47') // 2) * 2 == K('s2_k47') + 1                       # the last tap of the last step is past K
    assert CASES['s8_xw384'][4][1] == 384 and CASES['s8_xw385'][4][1] == 385 and 63 * 8 + 48 > 5 * 64
    assert 4 * CASES['tile64'][4][0] == 256 and CASES['tile65'][4][0] == 65
    assert K('k3_s4') < S('k3_s4') and K('k5_s8') < S('k5_s8')
    assert CASES['pad18'][0][5] % 4 == 2 and CASES['T2'][0][11] < K('T2')
    assert CASES['g19'][0][7] % 4 == 3


@pytest.mark.parametrize('B', [3, 7, 8, 10])
@pytest.mark.parametrize('name', list(CASES))
def test_workspace_query_covers_the_small_group_slabs(name, B):
    pkg = importlib.import_module('td-vc-gan_amd')
    g = CASES[name][0]
    (_, cin, cout, k, s, p, d, G, reflect, transposed, out_pad, T) = g
    spec = pkg.ops.ConvSpec(cin, cout, k, s, p, d, G, reflect, transposed, out_pad)
    assert spec.tout(T) == tout_of(g)
    query = pkg._lib.lib().tdvc_conv_wgrad_workspace(C.byref(spec.desc(B, T)))
    need = sg_slab_bytes(g, B)
    assert query >= need, (name, B, query, need)
    if -(-k // s) not in WGRAD_MFMA_J:      # the scalar weight-grad behind it needs no workspace
        assert query == need, (name, B, query, need)
