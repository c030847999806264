"""The batched epilogue of conv_lean_kernel (conv_lean.hip: lean_epi_rows, `epilogue`): FORWARD and INPUT-GRAD against float64, and bit for
bit against the one-float4-at-a-time epilogue the same instances keep behind tdvc_debug_knob(9, 1).

The batched epilogue issues the operand loads of a whole batch (a row of the wave's sub-tiles, or several) in front of the arithmetic
and the stores, and tests no bound per float4: a lane past Cout, past T or past the last sample of a folded group carries an
out-of-range buffer offset (its loads return zero, its stores are dropped), an absent operand an empty descriptor. It moves no bit:
every element goes through the same expressions in the same order. So each case, at each tile that takes it, checks

  * both float64 bars of the lean edge suite (edge_support.assert_bars; the rules are in test_lean_conv_edges_gpu.py's docstring);
    the buffers are SENT-filled with spare channels behind every operand, so a store that should have been dropped shows,
  * the instance of each call by trace: the name the tile table of lean_cases.py gives, unchanged by the epilogue,
  * torch.equal between knob 9 off (batched) and on (one float4 at a time) on y, dx and, with a FiLM epilogue, dgb, and on the sign
    words where the forward writes them,
  * and all of it once more with NaN bit patterns in the LDS of every CU in front of every call.

Rows (Edge options; each gives one forward and one input-grad, so one row covers a pair of each pass), B = 2:

  plain        ACT/FWD with bias                          ACT/PLAIN
  bias3_res    ACT/FWD with bias3 and res                 ACT/MASK, fp32 mask
  mask_add     ACT/FWD with add (out_scale 0.5)           ACT/MASK, fp32 mask, with add
  post         ACT/FWD, post LeakyReLU                    MASK_LRELU/PLAIN
  tanh         ACT/FWD, post tanh                         (no lean input-grad: not run)
  film_res     FILM/FWD with res (K = 1)                  ACT/FILM
  film_add     FILM/FWD with add                          ACT/FILM with add
  bits         ACT/FWD writing sign words                 ACT/MASK, 1-bit mask (the sign words of x)
  bits_add     ACT/FWD writing sign words, with add       ACT/MASK, 1-bit mask, with add

Shapes, the smallest at which the epilogue can go wrong: channels ragged against the row tile on both passes (Cin = Cout = 20 on the
16-row tiles, 40 on 32 rows, 72 on 48 and 64 rows, 136 on 144 rows) and a last time tile with columns past T (T = 68 on the 64-column
tiles, 260 on the 256-column ones; 96 / 288 where sign words are read or written: T % 32 == 0); T = 50 on the 64-column tiles for the
scalar path (rows not 16-byte aligned); and folded rows at T = 16 with B = 5, a partial last group (automatic tile: forcing one
disables the fold). test_epilogue_rows_reach_the_lean_kernel checks on the CPU, with the launcher's mirror, that every (tile, row)
runs on the lean kernel and that every shape has lanes out of range."""
import contextlib

import pytest
import torch

from conv_edge import Edge, _g
from edge_support import assert_bars, forced_tile, lib, pack_sign_bits, poison_lds
from lean_cases import GENERIC, LEAN_CFG, TANH_ALLOW, TILES, expected_instance, lean_call, lean_name, tile_rows_cols

TILE_IDS = {c: f'tile{c}_' + 'x'.join(map(str, LEAN_CFG[c])) for c in TILES}
ROWS = {
    'plain': dict(),
    'bias3_res': dict(pre=1, bias3=True, res=True),
    'mask_add': dict(pre=1, add=True),
    'post': dict(post=1),
    'tanh': dict(pre=1, post=2, tanh_allow=TANH_ALLOW),
    'film_res': dict(film=True, res=True),
    'film_add': dict(film=True, add=True),
    'bits': dict(pre=1, bits=True),
    'bits_add': dict(pre=1, bits=True, add=True),
}
BITS_TILES = tuple(c for c in TILES if c not in (3, 7))      # tiles 3 and 7 hand a call with sign words to tile 0
FOLD = {r[0][0]: r for r in [
    (_g('epi_fold_c48_T16_B5_post', 48, 32, 5, 2, 1, False, 16), dict(B=5, post=1)),
    (_g('epi_fold_c32_T16_B5_bias3_res_add', 32, 32, 3, 1, 1, False, 16), dict(B=5, bias3=True, res=True, add=True)),
]}


def ragged_channels(cfg):
    return {16: 20, 32: 40, 48: 72, 64: 72, 144: 136}[tile_rows_cols(cfg)[0]]


def row_case(cfg, row, scalar=False):
    """(geometry, options) of a row at a tile."""
    opts = ROWS[row]
    cols = tile_rows_cols(cfg)[1]
    T = 50 if scalar else ((96 if cols == 64 else 288) if opts.get('bits') else (68 if cols == 64 else 260))
    c, k = ragged_channels(cfg), (1 if opts.get('film') else 3)
    return _g(f'epi_{row}_c{c}_k{k}_T{T}', c, c, k, (k - 1) // 2, 1, False, T), {**dict(B=2), **opts}


def passes(row):
    return ('fwd',) if ROWS[row].get('post') == 2 else ('fwd', 'dgrad')


FORCED = [(c, r, False) for c in TILES for r in ROWS if not ROWS[r].get('bits') or c in BITS_TILES] + \
         [(c, r, True) for c in TILES if tile_rows_cols(c)[1] == 64 for r in ROWS if not ROWS[r].get('bits')]
FORCED_IDS = [f'{TILE_IDS[c]}-{r}' + ('-T50' if s else '') for c, r, s in FORCED]


def test_epilogue_rows_reach_the_lean_kernel():
    """CPU. Every (tile, row) of the table runs on the lean kernel both ways (the tanh row forward only), with the pair the docstring
    names; every shape leaves lanes of the last row tile past the channels and lanes of the last time tile past T; the scalar rows
    have T % 4 != 0; the folded rows fold (whole chunks, 64 / T samples per tile) and their last group is partial."""
    pairs = set()
    for cfg, row, scalar in FORCED:
        geom, opts = row_case(cfg, row, scalar)
        MT, NT = tile_rows_cols(cfg)
        for what in passes(row):
            name = expected_instance(geom, opts, what, cfg, bits=bool(opts.get('bits')))
            assert name != GENERIC and name.startswith(lean_name(cfg, 0, 0)[:-4]), (cfg, row, what, name)
            pairs.add(lean_call(geom, opts, what)[-2:])
        assert geom[1] % MT and geom[2] % MT and geom[-1] % NT, (cfg, row, geom)      # rows past the channels both ways, columns past T
        assert (geom[-1] % 4 != 0) == scalar and (not opts.get('bits') or geom[-1] % 32 == 0)
    assert pairs == {(0, 0), (1, 0), (0, 1), (0, 2), (0, 3), (2, 3)}, sorted(pairs)
    for geom, opts in FOLD.values():
        for what in ('fwd', 'dgrad'):
            red, k, d, pad, mirror, xfk, epi = lean_call(geom, opts, what)
            rows = geom[2] if what == 'fwd' else geom[1]
            assert rows >= 32 and red % 16 == 0 and geom[-1] == 16 and opts['B'] % 4, (geom[0], what)


@contextlib.contextmanager
def one_at_a_time(on):
    """tdvc_debug_knob(9, 1): the lean kernel runs the epilogue that handles one float4 at a time."""
    lib().tdvc_debug_knob(9, int(on))
    try:
        yield
    finally:
        lib().tdvc_debug_knob(9, 0)


def run(case, dev, cfg, knob, poison, whats):
    """The forward and (if asked) the input-grad of a fresh Edge -> Edge."""
    geom, opts = case
    e = Edge(geom, dev, **{**dict(wt=True, nan_spare=True), **opts})
    kw = dict(x_bits=pack_sign_bits(e.x).to(dev)) if opts.get('bits') else {}

    def calls():
        if poison:
            poison_lds(dev)
        res = e.fwd()
        if 'dgrad' in whats:
            if poison:
                poison_lds(dev)
            res.update(e.dgrad(**kw))
        return res
    with one_at_a_time(knob):
        res = forced_tile(cfg, calls)
    assert_bars(res, f'{geom[0]} tile {cfg} ' + ('one float4 at a time' if knob else 'batched') + (' (poisoned LDS)' if poison else ''))
    return e


def assert_same_bits(new, old, whats, what):
    keys = ('yv',) + (('dxv',) + (('dgbv',) if new.film else ()) if 'dgrad' in whats else ()) + (('bits_v',) if new.bits_v is not None else ())
    for key in keys:
        a, b = getattr(new, key), getattr(old, key)
        assert torch.equal(a, b), f'{what}: {key[:-1]} differs between the batched and the one-at-a-time epilogue in {int((a != b).sum())} elements'
        assert float(a.float().abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('cfg,row,scalar', FORCED, ids=FORCED_IDS)
def test_batched_epilogue_equals_one_at_a_time(cfg, row, scalar, dev):
    case = row_case(cfg, row, scalar)
    whats = passes(row)
    for poison in (False, True):
        new = run(case, dev, cfg, 0, poison, whats)
        old = run(case, dev, cfg, 1, poison, whats)
        for e in (new, old):
            for what in whats:
                want = expected_instance(case[0], case[1], what, cfg, bits=bool(case[1].get('bits')))
                assert e.names[what] == {want}, (case[0][0], what, want, sorted(e.names[what]))
        assert_same_bits(new, old, whats, f'{case[0][0]} tile {cfg}' + (' (poisoned LDS)' if poison else ''))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(FOLD))
def test_batched_epilogue_on_folded_short_sequences(name, dev):
    case = FOLD[name]
    for poison in (False, True):
        new = run(case, dev, -1, 0, poison, ('fwd', 'dgrad'))
        old = run(case, dev, -1, 1, poison, ('fwd', 'dgrad'))
        for e in (new, old):
            for what in ('fwd', 'dgrad'):
                _, _, _, _, _, xfk, epi = lean_call(case[0], case[1], what)
                assert e.names[what] == {lean_name(6, xfk, epi, True)}, (name, what, sorted(e.names[what]))
        assert_same_bits(new, old, ('fwd', 'dgrad'), name + (' (poisoned LDS)' if poison else ''))
