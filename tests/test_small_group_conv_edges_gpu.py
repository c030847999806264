"""Edge geometry of the vector-ALU kernels for grouped strided convs with 4 input and 4 output channels per group
(small_group_fwd_kernel<S>, small_group_dgrad_kernel<S>, small_group_wgrad_kernel, conv_small_group.hip: discriminator layer 4)
against float64, through the Edge class of conv_edge.py (rules: test_generic_conv_edges_gpu.py): both bars on every tensor (rel-L2 < 2e-5 and the
element-wise summation bound with exact zeros where A == 0), NaN-poisoned LDS before every case, outputs that start as SENT, the
weight-grad workspace exactly as large as the query says with a guard around it, and the kernel of every call asserted by name.

The case table, with the edge each row sits on, is CASES of small_group_cases.py (test_small_group_plan_cpu.py runs host-side checks of
the same table without a GPU). Every case runs the forward, the input-grad twice (dy_xf NONE and MASK_LRELU with the PLAIN epilogue: the
only forms the route takes; plain_dgrad of conv_edge.py) and the weight-grad. What the rows reach that nothing else does:

  * Tout = 64 / 65 (tile boundary of the forward, 4 * Tout == 256 limit of the weight-grad and the first shape past it);
  * pad % 4 != 0 (scalar dx stores, a lane that straddles t = 0), odd Tin, channel-slice views with unaligned planes;
  * the register limits 16 K == 768 and 16 J s == 768, a last step whose last tap is past K, K < stride;
  * XW == 384 (all six staging roles of the weight-grad) and 385 (declined), a forward window staged in two passes;
  * Tout == 1, a last block with a dead wave, act_in on forward and weight-grad, dbias == NULL, no bias, a dy scale, tanh;
  * strides 3, 5, 7: forward and input-grad launchers decline to the generic MFMA kernel, the weight-grad stays;
  * the weight-grad's sample split at B = 7 (one block per group), 8, 10, 11 (four; the prefetch guard b + nsplit < B);
  * the off switch (tdvc_debug_knob(2, 1)): all three calls on the generic kernels.

tanh. The term device tanhf adds to the y bar is measured as the lean suite measures it: on ANOTHER kernel, the scalar generic
route on the same case (tanh_excess of conv_edge.py). TANH_EXCESS_MEASURED is that figure in units of 2^-24; the bar
allows twice that (test_tanh_allowance_measured_on_scalar_route repeats the measurement and prints it).

RESULTS (first run on an MI355X; every figure is err / bound, the bar is 1.0)
  case        y      dx     dx masked  dw     db      (kernels as asserted)
  tile64      0.010  0.012  0.014      0.003  0.002
  tile65      0.011  0.011  0.013      0.003  0.001   weight-grad conv_wgrad_kernel<1,..>
  pad18       0.010  0.011  0.014      0.004  0.002
  odd_T       0.012  0.013  0.013      0.003  0.003
  views       0.011  0.012  0.013      0.003  -       db untouched bit for bit
  s2_k48      0.008  0.008  0.011      0.004  0.004
  s2_k47      0.008  0.010  0.011      0.003  0.002
  s8_xw384    0.008  0.012  0.013      0.005  0.003
  s8_xw385    0.007  0.010  0.011      0.004  0.001   weight-grad conv_wgrad_scalar_kernel<1>
  k3_s4       0.073  0.048  0.060      0.009  0.004   phase 3 of dx exactly 0
  k5_s8       0.037  0.042  0.042      0.028  0.022
  T2          0.006  0.006  0.005      0.149  0.180   (n = B * Tout = 3 on dw and db)
  g19         0.011  0.011  0.012      0.004  0.002
  pre         0.015  0.010  0.012      0.003  0.002   MASK epilogue on conv_gemm_kernel<2,..>: dx 0.013
  tanh        0.019  0.039  0.038      0.002  0.001   tanh mask on conv_gemm_kernel<2,..>: dx 0.041; weight-grad conv_wgrad_kernel<1,..>
  s3          0.040  0.038  0.044      0.009  0.004   forward / input-grad conv_gemm_kernel<1,..> / <2,..>
  s5          0.029  0.029  0.028      0.007  0.006   "
  s7          0.024  0.020  0.021      0.008  0.004   "
  sample split, tile64 at B = 7 / 8 / 10 / 10 without dbias / 11: dw 0.001 each, db below 0.001.
  off switch, tile64 on the generic kernels: y 0.011, dx 0.012, dx masked 0.014, dw 0.003, db 0.001.
  tanh: the measured excess on the scalar route is 0.000 x 2^-24 (the summation bound already covers device tanhf there), so the
  allowance is 0 and the tanh case passes the plain bars. rel-L2 stayed below 2.5e-7 on every tensor of every case.
  No defect was found in the three small-group kernels or their launchers.
"""
import pytest

from conv_edge import Edge, plain_dgrad, tanh_excess
from edge_support import assert_bars, lib, poison_lds
from small_group_cases import CASES, MFMA_WGRAD, SG_WGRAD, SPLIT_B, small_group_families

pytestmark = pytest.mark.gpu

TANH_EXCESS_MEASURED = 0.0      # units of 2^-24, scalar generic route on the `tanh` case (RESULTS in the docstring)
TANH_ALLOW = 2 * TANH_EXCESS_MEASURED
SG = 'small_group_'


def make_case(name, dev, generic=0, **over):
    g, opts, out_scale, _, _ = CASES[name]
    opts = {**opts, **over}
    if opts.get('post') == 2:
        opts['tanh_allow'] = TANH_ALLOW
    e = Edge(g, dev, generic, **opts)
    e.out_scale = out_scale      # Edge ties out_scale to `add`; the forward call, its reference and dy_xf all read the attribute
    return e


def has(names, prefix):
    return any(n.startswith(prefix) for n in names)


def assert_family(names, prefix, what):
    """The call ran `prefix`; a small-group kernel only where that is what `prefix` names."""
    assert has(names, prefix), (what, prefix, sorted(names))
    stray = [n for n in names if n.startswith(SG) and not n.startswith(prefix)]
    assert not stray, (what, prefix, stray)


def run_case(e, name, fams):
    """forward and input-grad (dy_xf NONE, MASK_LRELU) -> bars; the kernel family of each call asserted. The caller runs the
    weight-grad (and the input-grad forms that leave the route) after it."""
    fwd, dg, _ = fams
    res = e.fwd()
    assert_family(e.names['fwd'], fwd, f'{name} fwd')
    for masked in (False, True):
        r, names = plain_dgrad(e, masked)
        res.update(r)
        assert_family(names, dg, f'{name} dgrad masked={masked}')
    return res


@pytest.mark.parametrize('name', list(CASES))
def test_small_group_edge(name, dev):
    poison_lds(dev)
    e = make_case(name, dev)
    fwd, dg, wg = small_group_families(name)
    res = run_case(e, name, (fwd, dg, wg))
    if name == 'k3_s4':      # no tap reaches phase 3 of an input position: exact zeros, written (dx started as SENT)
        assert bool((e.dxv[:, :, 3::4] == 0).all()) and bool((e.dxv[:, :, 0::4] != 0).any())
    if name == 'pre':        # the MASK epilogue is outside the route: the generic MFMA kernel
        r = e.dgrad()
        res['dx_mask_epilogue'] = r['dx']
        assert_family(e.names['dgrad'], 'conv_gemm_kernel<2,', 'pre dgrad MASK epilogue')
    if name == 'tanh':       # dy_xf = XF_MASK_TANH (aux = the stored forward output): off the route, input-grad and weight-grad
        r = e.dgrad()
        res['dx_tanh_mask'] = r['dx']
        assert_family(e.names['dgrad'], 'conv_gemm_kernel<2,', 'tanh dgrad')
    res.update(e.wgrad())
    assert_family(e.names['wgrad'], wg, f'{name} wgrad')
    if wg == SG_WGRAD:
        assert 'slab_reduce_multi_kernel' in e.names['wgrad'], sorted(e.names['wgrad'])
    if name == 'views':
        assert 'db' not in res      # dbias = NULL: Edge.wgrad asserted db bit for bit and that no bias-gradient kernel ran
    assert_bars(res, f'small-group {name}')


@pytest.mark.parametrize('B,with_db', [(7, True), (8, True), (10, True), (10, False), (11, True)],
                         ids=['B7', 'B8', 'B10', 'B10_no_db', 'B11'])
def test_wgrad_sample_split(B, with_db, dev):
    """tile64 at the batch sizes around the split: B = 7 one block per group walks all samples; from 8 on four blocks take every
    fourth sample, 2 + 2 + 2 + 2 (B = 8), 3 + 3 + 2 + 2 (10) and 3 + 3 + 3 + 2 (11) of them: the last prefetch of each is guarded by
    b + nsplit < B. Edge's bound scales with B (n = B * Tout)."""
    assert B in SPLIT_B
    poison_lds(dev)
    e = make_case('tile64', dev, B=B, with_db=with_db)
    res = e.fwd()
    assert_family(e.names['fwd'], 'small_group_fwd_kernel<4>', f'B={B} fwd')
    res.update(e.wgrad())
    assert e.query >= (4 if B >= 8 else 1) * (16 * 16 * 41 + 16 * 4) * 4, e.query      # nsplit slabs of [G][16][K] + [G][4]
    assert_family(e.names['wgrad'], SG_WGRAD, f'B={B} wgrad')
    assert 'slab_reduce_multi_kernel' in e.names['wgrad'], sorted(e.names['wgrad'])
    assert ('db' in res) == with_db
    assert_bars(res, f'small-group split B={B}{"" if with_db else " no db"}')


def test_small_group_off_switch(dev):
    """tdvc_debug_knob(2, 1): the same geometry on the generic kernels, same bars."""
    poison_lds(dev)
    e = make_case('tile64', dev)
    lib().tdvc_debug_knob(2, 1)
    try:
        res = run_case(e, 'tile64 off', ('conv_gemm_kernel<1,', 'conv_gemm_kernel<2,', MFMA_WGRAD))
        res.update(e.wgrad())
    finally:
        lib().tdvc_debug_knob(2, 0)
    assert_family(e.names['wgrad'], MFMA_WGRAD, 'tile64 off wgrad')
    assert_bars(res, 'small-group tile64, route switched off')


def test_tanh_allowance_measured_on_scalar_route(dev):
    """The measurement behind TANH_EXCESS_MEASURED, repeated: the `tanh` case on the scalar generic route, which must itself pass
    the y bar with the allowance (twice the recorded figure)."""
    poison_lds(dev)
    e = make_case('tanh', dev, generic=1)
    res = e.fwd()
    assert_family(e.names['fwd'], 'conv_scalar_kernel<1>', 'tanh scalar fwd')
    x = tanh_excess(e)
    print(f'[edge] tanh excess on the scalar route: {x:.3f} x 2^-24 (recorded {TANH_EXCESS_MEASURED}, allowed {TANH_ALLOW})')
    assert_bars(res, 'small-group tanh, scalar route')
