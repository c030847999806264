"""The host side of what the cases of test_small_group_conv_edges_gpu.py (small_group_cases.py: the 4 -> 4-channels-per-group kernels
of conv_small_group.hip) rely on. tdvc_conv_wgrad_workspace() is host code: no GPU needed.

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

from small_group_cases import CASES, MFMA_WGRAD, SCALAR_WGRAD, SG_WGRAD, WGRAD_MFMA_J, small_group_desc


def tout_of(g):
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    return (T + 2 * p - (k - 1) - 1) // s + 1


def wgrad_contract(g):
    """launch_small_group_wgrad: a thread per (ci, k) with four idle ones for the bias, six staging roles of 256 for the padded
    rows of the four input channels, one role for the four dy rows."""
    (_, cin, cout, k, s, p, d, G, _, _, _, T) = g
    return 4 * k <= 252 and 4 * (T + 2 * p + s) <= 6 * 256 and 4 * tout_of(g) <= 256


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
