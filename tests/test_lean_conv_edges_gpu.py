"""Edge geometry of conv_lean_kernel<M_REP,N_REP,WM,WN,XFK,EPI[,FOLD]> (conv_lean.hip), FORWARD and INPUT-GRAD, against float64:
every stride-1 trunk conv, posconv, conditioning conv and discriminator layer 5 of the step runs one of its instances.

The rules are those of test_generic_conv_edges_gpu.py, whose Edge this file drives:

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
    figures of test_kernel_instances_gpu.LEAN_CFG, and that nothing else was launched; a reroute asserts conv_gemm_kernel<0, and no
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

from test_generic_conv_edges_gpu import Edge, SENT, U, _mods, assert_bars
from test_kernel_instances_gpu import LEAN_CFG, LXF_ACT, LXF_FILM, LXF_MASK_LRELU, EPI_FWD, EPI_MASK, EPI_FILM, EPI_PLAIN
from test_lean_wgrad_edges_gpu import _g

pytestmark = pytest.mark.gpu

GENERIC = 'conv_gemm_kernel<0,'
REPACK = 'weight_repack_kernel<0>'      # the generic MFMA kernel's per-launch weight helper
TANH_EXCESS_MEASURED = 0.0      # units of 2^-24, scalar generic route on head_16_1_tanh_T132 (RESULTS in the docstring)
TANH_ALLOW = 2 * TANH_EXCESS_MEASURED
TILES = sorted(LEAN_CFG)
TILE_IDS = [f'tile{c}_' + 'x'.join(map(str, LEAN_CFG[c])) for c in TILES]

# name: (geometry (name, Cin, Cout, K, 1, pad, dil, 1, reflect, False, 0, T), Edge options); B = 3 unless said otherwise
CASES = {c[0][0]: c for c in [
    # Cout ragged against every row tile; one 20-channel chunk forward, 32 + 8 backward; a 4-column last tile
    (_g('rows40_c20_k3_T260_views', 20, 40, 3, 1, 1, False, 260), dict(pre=1, add=True, views=True)),
    # nothing ragged: T is exactly one 256-column tile or four 64-column tiles, the right halo lies wholly outside;
    # MASK_LRELU prologue with PLAIN epilogue
    (_g('exact_64_k5_T256_post', 64, 64, 5, 2, 1, False, 256), dict(post=1)),
    # the right mirror zone [250, 274] straddles the 256 boundary, the last tile is shorter than the pad
    (_g('reflect_k11_d5_T276', 32, 32, 11, 25, 5, True, 276), dict(pre=1, add=True, views=True)),
    # both mirrors overlap inside one tile
    (_g('reflect_pad_Tm3_T28', 16, 16, 11, 25, 5, True, 28), dict(pre=1)),
    # T % 4 != 0: tail masking, rows not 16-byte aligned, scalar epilogue
    (_g('odd_T50_k7_d3_views', 24, 24, 7, 9, 3, True, 50), dict(pre=1, views=True)),
    # vec == 0 at a T % 4 == 0 shape
    (_g('unaligned_T64', 16, 24, 3, 1, 1, False, 64), dict(pre=1, add=True, unaligned=True)),
    # the posconv exactly as FilmBlockFn calls it: FILM/FWD and ACT/FILM with every FiLM stride non-contiguous
    (_g('film_pw_24_T260_views', 24, 24, 1, 0, 1, False, 260), dict(film=True, res=True, add=True, views=True)),
    # FiLM prologue and epilogue on the scalar path
    (_g('film_pw_32_T50', 32, 32, 1, 0, 1, False, 50), dict(film=True)),
    # one output row; the input-grad (tanh mask) has no lean instance and must take the generic route
    (_g('head_16_1_tanh_T132', 16, 1, 7, 3, 1, True, 132), dict(pre=1, post=2, tanh_allow=TANH_ALLOW)),
    # chunks of more than 32 channels on the 16-row tiles (56 + 56 + 56 + 56 + 32 at 64 columns: test_lean_edges_cpu.py)
    (_g('deep_256x16_k3_T64', 256, 16, 3, 1, 1, False, 64), dict(B=2)),
    # nsteps == 1 forward (the pipelined loop is skipped); 4 output rows backward
    (_g('one_step_4x20_pw_T132', 4, 20, 1, 0, 1, False, 132), dict()),
    (_g('no_bias_48_k3_T132', 48, 48, 3, 1, 1, False, 132), dict(bias=False, pre=1)),
]}
# Cin 8 as the window [128, 136) of a 136-channel weight, bias3, sign words, views; Cin * K = 24 takes the 16 x 256 override when
# nothing is pinned; one word in the last 256-column tile. Its sign words feed the LeakyReLU mask of a second conv's input-grad.
WINDOW = (_g('window8_of136_bias3_bits_T288', 8, 136, 3, 1, 1, False, 288), dict(w_cin=136, w_cin_off=128, bias3=True, bits=True, views=True))
WINDOW_NEXT = (_g('window_next_136x32_T288', 136, 32, 3, 1, 1, False, 288), dict(pre=1, views=True))
# Contract rows beyond the product's use: a FiLM prologue with K = 3 (forward and input-grad only)
FILM_K3 = {c[0][0]: c for c in [
    (_g('film_k3_zero_T132', 16, 16, 3, 1, 1, False, 132), dict(film=True, views=True)),
    (_g('film_k3_reflect_T132', 16, 16, 3, 1, 1, True, 132), dict(film=True, views=True)),
]}
# FOLD: T = 16 / 32 put 4 / 2 samples into one 64-column tile; automatic tiles. (geometry, options, folded forward, folded backward)
FOLD_ROWS = {c[0][0]: c for c in [
    (_g('fold_32x48_k5_T16_B7_post_views', 32, 48, 5, 2, 1, False, 16), dict(B=7, post=1, views=True), True, True),
    (_g('fold_16x32_k3_T32', 16, 32, 3, 1, 1, False, 32), dict(B=3), True, False),      # backward: 16 output rows < 32
    # the chunk must divide 48; add on both passes: each sample of a folded tile reads its own rows of the running sum
    (_g('fold_48x64_k5_T16_B9_add', 48, 64, 5, 2, 1, False, 16), dict(B=9, add=True), True, True),
    # the misses run unfolded
    (_g('fold_miss_cin24_T16', 24, 32, 3, 1, 1, False, 16), dict(B=7), False, False),    # Cin % 16 != 0 forward, 24 rows backward
    (_g('fold_miss_cout16_T16', 32, 16, 3, 1, 1, False, 16), dict(B=7), False, True),    # 16 rows forward; the backward still folds
    # dy a view while the mask tensor (the stored y) is contiguous: aux_bs != x_bs on the input-grad
    (_g('fold_miss_aux_bs_T16', 32, 48, 5, 2, 1, False, 16), dict(B=7, post=1, views=('dy',)), True, False),
]}
# Reroutes: (geometry, options, which calls must end on the generic MFMA kernel)
REROUTES = {c[0][0]: c for c in [
    (_g('reroute_cin18_fwd', 18, 24, 3, 1, 1, False, 132), dict(pre=1), ('fwd',)),
    (_g('reroute_cout18_bwd', 24, 18, 3, 1, 1, False, 132), dict(pre=1), ('dgrad',)),
    (_g('reroute_no_wt', 16, 24, 3, 1, 1, False, 132), dict(pre=1, wt=False), ('dgrad',)),
    (_g('reroute_T84_unaligned', 16, 24, 3, 1, 1, False, 84), dict(pre=1, unaligned=True), ('fwd', 'dgrad')),
    (_g('reroute_T82', 16, 24, 3, 1, 1, False, 82), dict(pre=1), ('fwd', 'dgrad')),
]}
WORST = {}      # instance -> tensor -> (err / bound, case)


# ------------------------------------------------------------------------------------------------ host mirror (CPU)
def tile_rows_cols(cfg):
    m, n, wm, wn = LEAN_CFG[cfg]
    return 16 * m * wm, 16 * n * wn


def _walk_geometry(rows, nvec):
    rp = min(256 // nvec if nvec <= 256 else 0, rows)
    return rp, (-(-rows // rp) if rp else 1 << 20)


def lean_footprint(cc, K, d, pad, mirror, cfg, fold_T=0):
    """LDS bytes and (input passes, weight passes) of a `cc`-channel chunk: the formula of launch_conv_lean. `pad` is the padding as
    the kernel sees it (the input-grad's is (K - 1) * d - pad), `mirror` the reflect pad of an input-grad, fold_T the sequence length
    of a folded launch. Hand figures, reflect_k11_d5_T276 (K = 11, d = 5, pad 25) on tile 1 (32 x 256):
      forward (mirror 0): lo = -28, hi = 25, span = 312, row stride 336;
        4 channels: 2 passes of 3 rows + 2 passes of 23 weight rows of 46    = (2016 + 2116) * 4 = 16528 bytes
        8 channels: 3 x 3 rows + 3 x 11 rows of 90                          = (3024 + 2970) * 4 = 23976
        12 channels: 4 x 3 rows + 5 x 7 rows of 134                         = (4032 + 4690) * 4 = 34888
        16 channels: 7 weight passes > the 6 the 32-row tiles prefetch: refused, so the chunk is 12 under the built-in 52 KiB
      input-grad (pad 25, mirror 25): lo = -52, hi = 50, span = 360, row stride 368;
        4 channels: 2 x 2 rows + 2116 = (1472 + 2116) * 4 = 14352;   12 channels: 6 x 2 rows + 4690 = (4416 + 4690) * 4 = 36424."""
    MT, NT = tile_rows_cols(cfg)
    lo = -((pad + mirror + 3) // 4 * 4)
    hi = (K - 1) * d - pad + mirror
    span = (NT + hi - lo + 3) // 4 * 4
    if fold_T:
        span = (64 // fold_T) * ((fold_T + hi - lo + 3) // 4 * 4)
    XS = (span + 15) // 32 * 32 + 16
    xrp, xnp = _walk_geometry(cc, span // 4)
    wrp, wnp = _walk_geometry(MT, K * cc // 4)
    return (xnp * xrp * XS + wnp * wrp * (K * cc + 2)) * 4, xnp, wnp


def lean_chunk(cin, K, d, pad, mirror, cfg, xfk, lds_cap=0, fold_T=0):
    """Channels per chunk launch_conv_lean picks (0: none fits, the launcher declines and the generic route takes the call)."""
    MT, NT = tile_rows_cols(cfg)
    xvp = 4 if (MT >= 144 or NT <= 64) else (12 if MT >= 32 else 6)
    wvp = 10 if MT >= 48 else (6 if MT >= 32 else 4)
    cap = lds_cap if lds_cap > 0 else (40 if cfg == 4 else 52) * 1024
    best = 0
    for cc in range(4, min(64 if (MT == 16 and cin >= 256) else 32, (cin + 3) // 4 * 4) + 1, 4):
        lds, xnp, wnp = lean_footprint(cc, K, d, pad, mirror, cfg, fold_T)
        if lds > cap or wnp > wvp or (xfk == LXF_ACT and xnp > xvp):
            continue
        if fold_T and cin % cc:
            continue
        best = cc
    return best


def lean_name(cfg, xfk, epi, fold=False):
    m, n, wm, wn = LEAN_CFG[cfg]
    return f'conv_lean_kernel<{m},{n},{wm},{wn},{xfk},{epi}' + (',true>' if fold else '>')


def lean_call(geom, opts, what):
    """(channels reduced, K, d, pad as the kernel sees it, mirror, xfk, epi) of a call, or None where the host gate keeps it off the
    lean kernel whatever the tile."""
    (_, cin, cout, k, _s, pad, d, _g_, reflect, _t, _o, T) = geom
    pre, post, film = opts.get('pre', 0), opts.get('post', 0), opts.get('film', False)
    aligned = T % 4 == 0 and not opts.get('unaligned', False)
    if not (T <= 80 or aligned):
        return None
    if what == 'fwd':
        return None if cin % 4 else (cin, k, d, pad, 0, LXF_FILM if film else LXF_ACT, EPI_FWD)
    if cout % 4 or not opts.get('wt', True) or post == 2 or (post == 1 and (pre or film)):
        return None
    return (cout, k, d, (k - 1) * d - pad, pad if reflect else 0, LXF_MASK_LRELU if post == 1 else LXF_ACT,
            EPI_FILM if film else (EPI_MASK if pre else EPI_PLAIN))


def expected_instance(geom, opts, what, cfg, bits=False, lds_cap=0):
    """The instance a call at forced tile `cfg` must launch (GENERIC for a reroute). Sign words move the tiles with one 16-column
    sub-tile per wave (3, 7) to tile 0."""
    c = lean_call(geom, opts, what)
    if c is None:
        return GENERIC
    if bits and cfg in (3, 7):
        cfg = 0
    red, k, d, pad, mirror, xfk, epi = c
    return lean_name(cfg, xfk, epi) if lean_chunk(red, k, d, pad, mirror, cfg, xfk, lds_cap) else GENERIC


def skipped(geom, cfg):
    return geom[-1] <= 80 and tile_rows_cols(cfg)[1] == 256


def expected_instances():
    """Every lean instance the tables of this file assert by trace (CPU; test_lean_edges_cpu.py checks the set for completeness)."""
    names = set()
    for geom, opts in CASES.values():
        names |= {expected_instance(geom, opts, w, c) for w in ('fwd', 'dgrad') for c in TILES if not skipped(geom, c)}
    for c in TILES:
        names |= {expected_instance(*WINDOW, 'fwd', c, bits=True), expected_instance(*WINDOW, 'dgrad', c),
                  expected_instance(*WINDOW_NEXT, 'dgrad', c), expected_instance(*WINDOW_NEXT, 'dgrad', c, bits=True)}
    for geom, opts, ffold, bfold in FOLD_ROWS.values():
        for what, fold in (('fwd', ffold), ('dgrad', bfold)):
            _, _, _, _, _, xfk, epi = lean_call(geom, opts, what)
            if fold:
                names.add(lean_name(6, xfk, epi, True))
    names.discard(GENERIC)
    return names


# ------------------------------------------------------------------------------------------------ running
def _lib():
    return _mods()[1].lib()


def _poison(dev):
    L = _mods()[1]
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))


def _forced(cfg, fn):
    lib = _lib()
    lib.tdvc_debug_force_tile(cfg)
    try:
        return fn()
    finally:
        lib.tdvc_debug_force_tile(-1)


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
        for k in keys:
            if k in res and res[k]['ratio'] >= WORST.setdefault(inst, {}).get(k, (-1.0, ''))[0]:
                WORST[inst][k] = (res[k]['ratio'], e.geom[0])


def fwd_dgrad(e, dev, poison, cfg=-1, **dgrad_kw):
    def run():
        if poison:
            _poison(dev)
        res = e.fwd()
        if poison:
            _poison(dev)
        res.update(e.dgrad(**dgrad_kw))
        return res
    return _forced(cfg, run)


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
                _poison(dev)
            r = _forced(tile, lambda: e2.dgrad(**kw))
            assert_bars(r, f'{e2.geom[0]} tile {cfg} {tag}')
            assert_only(e2, 'dgrad', lean_name(eff if kw else tile, LXF_ACT, EPI_MASK))
            record(e2, r, dict(dgrad=('dx',)))
            runs[tag] = e2.dxv.clone()
        assert torch.equal(runs['x_bits'], runs["x_in at the words' tile"]), 'dx from the sign words differs from dx from x_in'
        assert float(runs['x_bits'].abs().max()) > 0


def tanh_excess(e):
    """Largest |y - tanh64(z)| beyond the propagated summation bound, in units of 2^-24 (0 where the bound already covers it)."""
    got, ref = e.yv.detach().cpu().double(), e.ref['y']
    prop = (e.n['y'] + e.slack) * U * e.A['y'] + 2.0 ** -22 * ref.abs()
    return max(0.0, float((((got - ref).abs() - prop) / 2.0 ** -24).max()))


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
    lib = _lib()
    for poison in (False, True):
        e = make(row, dev)
        res = {}
        try:
            for what, call in (('fwd', e.fwd), ('dgrad', e.dgrad)):
                red, k, d, pad, mirror, xfk, epi = lean_call(row[0], row[1], what)
                cap = lean_footprint(chunk or 4, k, d, pad, mirror, 1)[0] - (0 if chunk else 4)
                assert lean_chunk(red, k, d, pad, mirror, 1, xfk, cap) == chunk
                lib.tdvc_debug_lds_cap(cap)
                if poison:
                    _poison(dev)
                res.update(_forced(1, call))
                assert_only(e, what, lean_name(1, xfk, epi) if chunk else GENERIC)
        finally:
            lib.tdvc_debug_lds_cap(0)
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
    for inst, per in sorted(WORST.items()):
        print(f'[edge] worst {inst}: ' + '  '.join(f'{k} {r:.3f} ({n})' for k, (r, n) in sorted(per.items())))
    assert all(r <= 1.0 for per in WORST.values() for r, _ in per.values())
