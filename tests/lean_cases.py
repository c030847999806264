"""The lean conv kernel's tile table, a CPU mirror of its host gate (conv_api.hip: lean_shape_ok / lean_fill; launch_conv_lean) and
the case tables of test_lean_conv_edges_gpu.py. No GPU: test_lean_edges_cpu.py checks the tables for completeness and the mirror
against hand figures, test_kernel_instances_gpu.py names its instances with the same tile table."""
from conv_edge import _g

LEAN_CFG = {0: (1, 4, 1, 4), 1: (2, 4, 1, 4), 2: (4, 4, 1, 4), 3: (1, 1, 1, 4), 4: (1, 4, 4, 1), 5: (3, 4, 1, 4), 6: (1, 2, 2, 2), 7: (9, 1, 1, 4)}
LXF_ACT, LXF_FILM, LXF_MASK_LRELU = 0, 1, 2
EPI_FWD, EPI_MASK, EPI_FILM, EPI_PLAIN = 0, 1, 2, 3

GENERIC = 'conv_gemm_kernel<0,'
TANH_EXCESS_MEASURED = 0.0      # units of 2^-24, scalar generic route on head_16_1_tanh_T132 (RESULTS in test_lean_conv_edges_gpu.py's docstring)
TANH_ALLOW = 2 * TANH_EXCESS_MEASURED
TILES = sorted(LEAN_CFG)

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
