"""Edge geometry of conv_lean_kernel<M_REP,N_REP,WM,WN,XFK,EPI[,FOLD]> (conv_lean.hip), FORWARD and INPUT-GRAD, against float64:
every stride-1 trunk conv, posconv, conditioning conv and discriminator layer 5 of the step runs one of its instances.

The rules are those of test_generic_conv_edges_gpu.py; this file drives the Edge class of conv_edge.py on the tables of lean_cases.py:

  * Inputs hold fp32 values; the reference is float64 CPU autograd on the same numbers.
  * The mask of a post-activated layer (LeakyReLU, tanh) comes from the GPU's own stored output. The seeded data of a FiLM case is
    asserted (on the CPU: Edge.assert_off_kink, also run by test_lean_edges_cpu.py) to hold no element within 3 * 2^-23 * H of the
    FiLM/LeakyReLU kink; otherwise the case is reseeded (renamed).
  * Two bars on every tensor, n = reduction length (Cin * K forward, Cout * K backward):
        rel-L2 < 2e-5   and   |got - ref| <= (n + slack) * 2^-23 * A + 2^-22 * |ref|,
    A = the same computation on absolute values, slack = 8, or 12 with a FiLM prologue (derivation: Edge's docstring); where A == 0
    the result must be exact. bias3 and res enter A as Edge's docstring says.
  * Outputs start as SENT. With `views` every operand is the [:, :C] slice of a [B, C + 3, T] buffer: the spare channels of the
    outputs (y, dx, dgb, the sign words) must still be SENT afterwards, and the spare channels of the INPUTS are NaN (as in the
    split-bf16 suite), so that a read past Cin, or past T in the last row of a sample, poisons the result.
  * Every call asserts by trace the exact instance, conv_lean_kernel<m,n,wm,wn,xfk,epi> with `,true>` appended for FOLD and the tile
    figures of lean_cases.LEAN_CFG, and that nothing else was launched; a reroute asserts conv_gemm_kernel<0, and no
    lean instance. expected_instance() mirrors the host gate (conv_api.hip: lean_shape_ok / lean_fill; launch_conv_lean).
  * Every accepted row runs a second time with tdvc_debug_poison_lds(0xFFFFFFFF) in front of EACH of its calls.
  * The worst err / bound per instance and tensor is collected; test_zz_worst_error_by_instance prints it.

The case table holds the smallest shapes that reach the edge named beside each row; every row runs at every forced tile 0..7
(tdvc_debug_force_tile), except the 256-column tiles at T <= 80, which launch_conv_lean never selects.

tanh (head_16_1_tanh_T132). The term device tanhf adds to the y bar cannot be derived here, so it is measured, on ANOTHER kernel:
the scalar generic route (tdvc_set_force_generic) on the same case. TANH_EXCESS_MEASURED is the largest |y - tanh64(z)| beyond
the propagated summation bound, in units of 2^-24; the bar allows twice that (test_tanh_allowance_measured_on_generic_route
repeats the measurement and prints it).

RESULTS (first run on an MI355X; every figure is err / bound, the bar is 1.0)
  * worst per (prologue, epilogue) pair over all eight tiles: ACT/FWD y 0.087 (one_step_4x20_pw_T132), FILM/FWD y 0.038, ACT/MASK dx
    0.021, ACT/FILM dx 0.038 dgb 0.040 (film_pw_24_T260_views), ACT/PLAIN dx 0.042, MASK_LRELU/PLAIN dx 0.009; folded instances
    y 0.031, dx 0.027; the generic MFMA kernel on the reroutes y 0.042, dx 0.082. The tiles differ in the third decimal only. No
    defect was found in conv_lean_kernel or its host gate.
  * tanh: the measured excess on the scalar generic route is 0.000 x 2^-24 (the summation bound already covers device tanhf there), so
    the allowance is 0 and head_16_1_tanh_T132 passes the plain bars on every tile.
  * the two FiLM-with-K=3 rows run on the lean kernel both ways (FILM_K3_ROUTE) and pass.
  * fold_16x32_k3_T32 folds its forward only: its input-grad has 16 output rows and launch_conv_lean folds from 32 rows on.
"""
import pytest
import torch

from conv_edge import Edge, tanh_excess
from edge_support import SENT, Worst, assert_bars, forced_tile, lib, poison_lds
from lean_cases import (CASES, EPI_FILM, EPI_FWD, EPI_MASK, EPI_PLAIN, FILM_K3, FOLD_ROWS, GENERIC, LEAN_CFG, LXF_ACT, LXF_FILM, REROUTES,
                        TANH_ALLOW, TANH_EXCESS_MEASURED, TILES, WINDOW, WINDOW_NEXT, expected_instance, lean_call, lean_chunk, lean_footprint,
                        lean_name, skipped)

pytestmark = pytest.mark.gpu

REPACK = 'weight_repack_kernel<0>'      # the generic MFMA kernel's per-launch weight helper
TILE_IDS = [f'tile{c}_' + 'x'.join(map(str, LEAN_CFG[c])) for c in TILES]
WORST = Worst()      # instance -> tensor -> (err / bound, case)


def make(row, dev, **override):
    geom, opts = row[0], row[1]
    return Edge(geom, dev, **{**dict(wt=True, nan_spare=True), **opts, **override})


def assert_only(e, what, want):
    """Exactly one kernel was launched by the call: the instance `want`, or (want == GENERIC) one generic MFMA instance, which may
    bring its weight repack helper along."""
    names = e.names[what]
    if want == GENERIC:
        names = names - {REPACK}
        assert len(names) == 1 and all(n.startswith(GENERIC) for n in names), (e.geom[0], what, sorted(e.names[what]))
    else:
        assert names == {want}, (e.geom[0], what, want, sorted(names))


def record(e, res, what_keys):
    for what, keys in what_keys.items():
        inst = next(iter(sorted(e.names[what] - {REPACK})))
        inst = 'generic ' + GENERIC[:-1] + '...>' if inst.startswith(GENERIC) else inst
        WORST.note(inst, {k: res[k] for k in keys if k in res}, e.geom[0])


def fwd_dgrad(e, dev, poison, cfg=-1, **dgrad_kw):
    def run():
        if poison:
            poison_lds(dev)
        res = e.fwd()
        if poison:
            poison_lds(dev)
        res.update(e.dgrad(**dgrad_kw))
        return res
    return forced_tile(cfg, run)


def run_row(row, dev, cfg, poison, want=None):
    e = make(row, dev)
    res = fwd_dgrad(e, dev, poison, cfg)
    assert_bars(res, f'{e.geom[0]} tile {cfg}' + (' (poisoned LDS)' if poison else ''))
    for what in ('fwd', 'dgrad'):
        assert_only(e, what, want[what] if want else expected_instance(row[0], row[1], what, cfg))
    record(e, res, dict(fwd=('y',), dgrad=('dx', 'dgb')))
    return e


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('cfg', TILES, ids=TILE_IDS)
def test_lean_edge(cfg, name, dev):
    """Every row of the table at every forced tile: y and dx (dgb with FiLM) within both bars, spare channels intact, the exact
    instance of each call by trace and nothing else launched; then the same once more on NaN-poisoned LDS."""
    row = CASES[name]
    if skipped(row[0], cfg):
        pytest.skip('256-column tiles are never selected for T <= 80 (launch_conv_lean)')
    for poison in (False, True):
        run_row(row, dev, cfg, poison)


@pytest.mark.parametrize('cfg', TILES, ids=TILE_IDS)
def test_lean_window_bias3_sign_bits(cfg, dev):
    """window8_of136_bias3_bits_T288: the forward reads the weight columns [128, 136) of a 136-channel layer, adds the 3-valued bias
    (t = 0, interior, t = T - 1) and packs sign words that must equal pack_sign_bits(stored y) bit for bit (Edge.fwd), y and the words
    being views. Its DG_PLAIN input-grad writes 8 rows from the `wt` rows behind w_cin_off. A second conv (136 -> 32) then takes the
    stored y as its input: its DG_MASK_LRELU input-grad with x_bits = those words must be bit-identical to the run with x_in on the
    same tile. Tiles 3 and 7 (one sub-tile per wave) must move to tile 0 whenever words are given."""
    eff = 0 if cfg in (3, 7) else cfg
    for poison in (False, True):
        e1 = make(WINDOW, dev)
        res = fwd_dgrad(e1, dev, poison, cfg)
        assert_bars(res, f'{e1.geom[0]} tile {cfg}' + (' (poisoned LDS)' if poison else ''))
        assert_only(e1, 'fwd', lean_name(eff, LXF_ACT, EPI_FWD))
        assert_only(e1, 'dgrad', lean_name(cfg, LXF_ACT, EPI_PLAIN))
        record(e1, res, dict(fwd=('y',), dgrad=('dx',)))
        e2 = make(WINDOW_NEXT, dev, x_src=e1.yv)
        e2.fwd()      # the references; the forward itself belongs to another suite (split-bf16 route)
        runs = {}
        for tag, tile, kw in (('x_in', cfg, {}), ('x_in at the words\' tile', eff, {}), ('x_bits', cfg, dict(x_bits=e1.bits_v))):
            e2.dxv.fill_(SENT)
            if poison:
                poison_lds(dev)
            r = forced_tile(tile, lambda: e2.dgrad(**kw))
            assert_bars(r, f'{e2.geom[0]} tile {cfg} {tag}')
            assert_only(e2, 'dgrad', lean_name(eff if kw else tile, LXF_ACT, EPI_MASK))
            record(e2, r, dict(dgrad=('dx',)))
            runs[tag] = e2.dxv.clone()
        assert torch.equal(runs['x_bits'], runs["x_in at the words' tile"]), 'dx from the sign words differs from dx from x_in'
        assert float(runs['x_bits'].abs().max()) > 0


def test_tanh_allowance_measured_on_generic_route(dev):
    """The measurement behind TANH_EXCESS_MEASURED, repeated: head_16_1_tanh_T132 on the scalar generic route. The generic route must
    itself pass the y bar with the allowance (twice the recorded figure)."""
    e = make(CASES['head_16_1_tanh_T132'], dev, generic=1)
    res = e.fwd()
    assert not any(n.startswith('conv_lean_kernel') for n in e.names['fwd']), sorted(e.names['fwd'])
    x = tanh_excess(e)
    print(f'[edge] tanh excess on the generic route: {x:.3f} x 2^-24 (recorded {TANH_EXCESS_MEASURED}, allowed {TANH_ALLOW}); kernels {sorted(e.names["fwd"])}')
    assert_bars(res, 'head_16_1_tanh_T132 generic route')


# the routes observed on an MI355X: both rows stay on the lean kernel, forward and backward (Cin * K = 48 takes the 16 x 256 override;
# the mirror fold of the reflect row's input-grad keeps it on the automatic 16 x 64 tile)
FILM_K3_ROUTE = {'film_k3_zero_T132': dict(fwd=lean_name(0, LXF_FILM, EPI_FWD), dgrad=lean_name(0, LXF_ACT, EPI_FILM)),
                 'film_k3_reflect_T132': dict(fwd=lean_name(0, LXF_FILM, EPI_FWD), dgrad=lean_name(3, LXF_ACT, EPI_FILM))}


@pytest.mark.parametrize('name', list(FILM_K3))
def test_film_prologue_with_three_taps(name, dev):
    """A FiLM prologue on a 3-tap conv, zero- and reflect-padded: no layer of the product does this, the C ABI admits it. Both bars on
    y, dx and dgb on the route the call takes (one kernel per call; FILM_K3_ROUTE holds what was observed); the padding
    applies to the ACTIVATED input (zero padding: lrelu(film(0)) must not leak beta into the halo)."""
    row = FILM_K3[name]
    for poison in (False, True):
        e = make(row, dev)
        res = fwd_dgrad(e, dev, poison)
        print(f'[edge] {name}: routes ' + '  '.join(f'{w}: {sorted(e.names[w])}' for w in ('fwd', 'dgrad')))
        assert_bars(res, name + (' (poisoned LDS)' if poison else ''))
        for what in ('fwd', 'dgrad'):
            assert e.names[what] == {FILM_K3_ROUTE[name][what]}, (what, sorted(e.names[what]))
        record(e, res, dict(fwd=('y',), dgrad=('dx', 'dgb')))


@pytest.mark.parametrize('name', list(FOLD_ROWS))
def test_lean_fold(name, dev):
    """Folded short sequences with automatic tiles: the `,true>` instance on forward and input-grad where the launcher folds (ragged
    batches: B % fold != 0; views; a chunk that must divide Cin), and the plain instance where it must not (Cin % 16 != 0, fewer than
    32 rows, a mask tensor whose batch stride differs from dy's). Both bars either way, also on poisoned LDS."""
    geom, opts, ffold, bfold = FOLD_ROWS[name]
    for poison in (False, True):
        e = make((geom, opts), dev)
        res = fwd_dgrad(e, dev, poison)
        assert_bars(res, name + (' (poisoned LDS)' if poison else ''))
        for what, fold in (('fwd', ffold), ('dgrad', bfold)):
            _, _, _, _, _, xfk, epi = lean_call(geom, opts, what)
            names = e.names[what]
            if fold:
                assert names == {lean_name(6, xfk, epi, True)}, (what, sorted(names))
            else:
                assert len(names) == 1 and all(n.startswith('conv_lean_kernel<') and n.endswith(f',{xfk},{epi}>') for n in names), (what, sorted(names))
        record(e, res, dict(fwd=('y',), dgrad=('dx',)))


def test_lean_fold_chunk_divides_cin():
    """CPU arithmetic: 48 channels at K = 5 fold into chunks of 24 (32 would leave a partial chunk running into the next sample)."""
    assert lean_chunk(48, 5, 1, 2, 0, 6, LXF_ACT, fold_T=16) == 24
    assert lean_chunk(48, 5, 1, 2, 0, 6, LXF_ACT) == 32


LDS_CAPS = [('chunk4', 4), ('chunk12', 12), ('below4', 0)]


@pytest.mark.parametrize('tag,chunk', LDS_CAPS, ids=[t for t, _ in LDS_CAPS])
def test_lean_chunk_size_by_lds_cap(tag, chunk, dev):
    """reflect_k11_d5_T276 on tile 1 with tdvc_debug_lds_cap set, per call, to the footprint of a 4-channel chunk (eight chunks of 4),
    of a 12-channel chunk (12 + 12 + 8), and to 4 bytes below the 4-channel footprint, where the launcher declines and the trace
    must show the generic route. Same bars; the cap is restored to 0 whatever happens."""
    row = CASES['reflect_k11_d5_T276']
    for poison in (False, True):
        e = make(row, dev)
        res = {}
        try:
            for what, call in (('fwd', e.fwd), ('dgrad', e.dgrad)):
                red, k, d, pad, mirror, xfk, epi = lean_call(row[0], row[1], what)
                cap = lean_footprint(chunk or 4, k, d, pad, mirror, 1)[0] - (0 if chunk else 4)
                assert lean_chunk(red, k, d, pad, mirror, 1, xfk, cap) == chunk
                lib().tdvc_debug_lds_cap(cap)
                if poison:
                    poison_lds(dev)
                res.update(forced_tile(1, call))
                assert_only(e, what, lean_name(1, xfk, epi) if chunk else GENERIC)
        finally:
            lib().tdvc_debug_lds_cap(0)
        assert_bars(res, f'reflect_k11_d5_T276 tile 1 {tag}' + (' (poisoned LDS)' if poison else ''))
        record(e, res, dict(fwd=('y',), dgrad=('dx',)))


@pytest.mark.parametrize('name', list(REROUTES))
def test_lean_reroute(name, dev):
    """Lean-shaped calls one step outside the gate (Cin % 4 != 0 forward, Cout % 4 != 0 backward, no transposed weight copy, T = 84
    with operands that are not 16-byte aligned, T = 82): the generic MFMA kernel, alone, with results inside both bars."""
    geom, opts, generic_calls = REROUTES[name]
    e = make((geom, opts), dev)
    res = fwd_dgrad(e, dev, False)
    assert_bars(res, name)
    for what in ('fwd', 'dgrad'):
        want = expected_instance(geom, opts, what, 0)
        assert (want == GENERIC) == (what in generic_calls), (name, what, want)
        if want == GENERIC:
            assert_only(e, what, GENERIC)
        else:
            assert len(e.names[what]) == 1 and all(n.startswith('conv_lean_kernel<') for n in e.names[what]), sorted(e.names[what])
    record(e, res, dict(fwd=('y',), dgrad=('dx',)))


def test_zz_worst_error_by_instance():
    """Prints the worst err / bound per instance and tensor over the cases that ran in this session (asserted case by case)."""
    WORST.report()
    assert all(r <= 1.0 for r in WORST.ratios())
