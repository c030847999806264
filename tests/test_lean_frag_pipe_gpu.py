"""The fragment ring of conv_lean_kernel's MFMA loop (conv_lean.hip: lean_ring_depth, ring_run) on the two tiles that have it, 16 x 64
(tile 3, <1,1,1,4>) and 32 x 64 (tile 6, <1,2,2,2>): FORWARD and INPUT-GRAD against float64, and bit for bit against the one-step-ahead
loop the same instances keep behind tdvc_debug_knob(8, 1).

The loop walks one tap at a time and issues the LDS reads of a step DEPTH (<= 8) steps ahead of its MFMAs. It moves no bit: every accumulator receives the same
MFMAs with the same operands in the same order as in the one-step-ahead loop. So each case, at each of the two tiles, checks

  * both float64 bars of the lean edge suite (edge_support.assert_bars; the rules are in test_lean_conv_edges_gpu.py's docstring),
  * the instance of each call by trace: the name the tile table of lean_cases.py gives, unchanged by the ring,
  * torch.equal between knob 8 off (ring) and on (one-step-ahead loop) on y, dx and, with a FiLM epilogue, dgb,
  * and all of it once more with NaN bit patterns in the LDS of every CU in front of every call: a read for a step past the chunk's
    last, or from a slot that was never filled, turns the result into NaN or breaks the equality.

What can go wrong in a ring is decided by the number of steps of a chunk (K * channels / 4) against DEPTH, and by where the read
cursor wraps from the last channel group of a tap to the next tap. The rows are the smallest shapes that reach each of these, B = 2,
one or two 64-column tiles (test_ring_tables_reach_every_step_count checks the step counts on the CPU with the launcher's mirror):

  STEPS       K = 1, Cin = 4 .. 72, Cout = 32, T = 64: 1 .. 18 steps per wave; a chunk holds at most 32 channels here, so the rows are
              chunks of 1 .. 8 steps, and from 36 channels on full chunks of 8 followed by a last chunk of 1 .. 8 (1, 2, 3: shorter
              than any DEPTH). The input-grads reduce over Cout = 32 with the flipped tap walk.
  CHUNKS      the step counts 9 .. 18 within ONE chunk, which K = 1 cannot give: K = 3 (9, 12, 15, 18), 5 (10), 7 (14), 11 (11), 13 (13),
              17 (17), and 16 as 64 channels of a 256-channel layer (16-row tile only: the 32-row tile takes 32 channels).
  WRAP        the cursor wraps every step (4 channels: one channel group per tap; K = 3 and K = 11 with dilation 5, zero padding,
              T = 64 and T = 132) and in the middle of a round (12 channels, K = 3).
  PAIRS       the other (prologue, epilogue) pairs at 5 and 9 steps: ACT/MASK (pre, add), MASK_LRELU/PLAIN (post), and FILM/FWD with
              ACT/FILM at 24 channels.
  REFLECT     the reflect fold of the 16-row sub-tiles (the same ring per tap, for each side): K = 11, d = 5, pad 25, 4 / 8 / 28 / 36 channels; T = 52
              (both mirrors in one tile), T = 50 (scalar epilogue) and T = 132 (the mirrors in different tiles).
  FOLD        folded short sequences keep their per-sub-tile column offsets: T = 16 with B = 5 (a partial last group) and T = 32 with
              B = 3, K = 5, 16 and 48 input channels; automatic tiles (forcing one disables the fold), the `,true>` name asserted.
"""
import contextlib

import pytest
import torch

from conv_edge import Edge, _g
from edge_support import assert_bars, forced_tile, lib, poison_lds
from lean_cases import GENERIC, LEAN_CFG, expected_instance, lean_call, lean_chunk, lean_name

RING_TILES = (3, 6)
TILE_IDS = [f'tile{c}_' + 'x'.join(map(str, LEAN_CFG[c])) for c in RING_TILES]
B2 = dict(B=2)

STEPS = [(_g(f'ring_steps{c // 4}_pw_T64', c, 32, 1, 0, 1, False, 64), B2) for c in range(4, 73, 4)]
CHUNKS = [(_g(f'ring_chunk{k * c // 4}_k{k}_c{c}_T64', c, c, k, (k - 1) // 2, 1, False, 64), B2)
          for k, c in ((3, 16), (3, 20), (3, 24), (5, 8), (7, 8), (13, 4), (17, 4))] + \
         [(_g('ring_chunk16_pw_256x32_T64', 256, 32, 1, 0, 1, False, 64), B2)]
WRAP = [(_g(f'ring_wrap_c{c}_k{k}_d{d}_T{T}', c, c, k, (k - 1) * d // 2, d, False, T), B2)
        for c, k, d, Ts in ((4, 3, 1, (64, 132)), (4, 11, 5, (64, 132)), (12, 3, 1, (64,))) for T in Ts]
PAIRS = [(_g('ring_mask_add_pw_c20_T64', 20, 20, 1, 0, 1, False, 64), dict(B=2, pre=1, add=True)),
         (_g('ring_mask_add_k3_c12_T64', 12, 12, 3, 1, 1, False, 64), dict(B=2, pre=1, add=True)),
         (_g('ring_post_pw_c20_T64', 20, 20, 1, 0, 1, False, 64), dict(B=2, post=1)),
         (_g('ring_post_k3_c12_T64', 12, 12, 3, 1, 1, False, 64), dict(B=2, post=1)),
         (_g('ring_film_pw_c24_T64', 24, 24, 1, 0, 1, False, 64), dict(B=2, film=True))]
REFLECT = [(_g(f'ring_reflect_c{c}_T{T}', c, c, 11, 25, 5, True, T), dict(B=2, pre=1)) for c in (4, 8, 28, 36) for T in (52, 50, 132)]
FORCED = {r[0][0]: r for r in STEPS + CHUNKS + WRAP + PAIRS + REFLECT}
# (geometry, options, folded forward, folded input-grad): the input-grad of a 16-channel layer has 16 output rows, below the fold's 32
FOLD = {r[0][0]: r for r in [
    (_g('ring_fold_c16_T16_B5', 16, 32, 5, 2, 1, False, 16), dict(B=5), True, False),
    (_g('ring_fold_c48_T16_B5_post', 48, 32, 5, 2, 1, False, 16), dict(B=5, post=1), True, True),
    (_g('ring_fold_c16_T32_B3', 16, 32, 5, 2, 1, False, 32), dict(B=3), True, False),
    (_g('ring_fold_c48_T32_B3_post', 48, 32, 5, 2, 1, False, 32), dict(B=3, post=1), True, True),
]}


def chunk_steps(geom, opts, what, cfg, fold_T=0):
    """Steps of each chunk of a call at tile `cfg`, by the launcher's mirror (None: the call does not run on the lean kernel there)."""
    c = lean_call(geom, opts, what)
    if c is None:
        return None
    red, k, d, pad, mirror, xfk, _ = c
    cc = lean_chunk(red, k, d, pad, mirror, cfg, xfk, fold_T=fold_T)
    if not cc:
        return None
    return [k * min(cc, red - c0) // 4 for c0 in range(0, red, cc)]


def test_ring_tables_reach_every_step_count():
    """CPU. Every forced row runs on the lean kernel at both tiles, both ways. Over the table, a wave runs every step count 1 .. 18 per
    call; ONE chunk has every step count 1 .. 18 on the 16-row tile and all but 16 on the 32-row tile (odd K: 16 steps are 64 channels
    at K = 1, which only the 16-row tiles take); some call ends on a chunk of fewer than 4 steps behind a full one; the cursor wraps
    every step (4 channels at K > 1) in some row. The folded rows fold where the table says (whole chunks of 20 and 30 steps)."""
    for cfg in RING_TILES:
        per_chunk, per_call, short_last = set(), set(), False
        for geom, opts in FORCED.values():
            for what in ('fwd', 'dgrad'):
                assert expected_instance(geom, opts, what, cfg) != GENERIC, (geom[0], what, cfg)
                st = chunk_steps(geom, opts, what, cfg)
                per_chunk |= set(st)
                per_call.add(sum(st))
                short_last |= len(st) > 1 and st[-1] < 4
        want = set(range(1, 19)) - ({16} if cfg == 6 else set())
        assert want <= per_chunk, (cfg, sorted(want - per_chunk))
        assert set(range(1, 19)) <= per_call, (cfg, sorted(set(range(1, 19)) - per_call))
        assert short_last
    assert chunk_steps(*STEPS[8], 'fwd', 3) == [8, 1] and chunk_steps(*STEPS[17], 'fwd', 6) == [8, 8, 2]
    assert chunk_steps(*FORCED['ring_chunk16_pw_256x32_T64'], 'fwd', 3) == [16] * 4
    assert chunk_steps(*FORCED['ring_wrap_c4_k11_d5_T64'], 'fwd', 3) == [11]
    for geom, opts, ffold, bfold in FOLD.values():
        assert chunk_steps(geom, opts, 'fwd', 6, fold_T=geom[-1]) == ([20] if geom[1] == 16 else [30, 30])
        assert ffold and bfold == (geom[1] >= 32)


@contextlib.contextmanager
def one_ahead(on):
    """tdvc_debug_knob(8, 1): the ring tiles run the one-step-ahead loop (and the plain reflect-fold loop)."""
    lib().tdvc_debug_knob(8, int(on))
    try:
        yield
    finally:
        lib().tdvc_debug_knob(8, 0)


def run(row, dev, cfg, knob, poison):
    """One forward and one input-grad of a fresh Edge -> (Edge, bars)."""
    e = Edge(row[0], dev, **{**dict(wt=True, nan_spare=True), **row[1]})

    def calls():
        if poison:
            poison_lds(dev)
        res = e.fwd()
        if poison:
            poison_lds(dev)
        res.update(e.dgrad())
        return res
    with one_ahead(knob):
        res = forced_tile(cfg, calls)
    assert_bars(res, f'{e.geom[0]} tile {cfg} ' + ('one-step-ahead loop' if knob else 'ring') + (' (poisoned LDS)' if poison else ''))
    return e, res


def assert_same_bits(ring, ahead, what):
    for key in ('yv', 'dxv') + (('dgbv',) if ring.film else ()):
        a, b = getattr(ring, key), getattr(ahead, key)
        assert torch.equal(a, b), f'{what}: {key[:-1]} differs between the ring and the one-step-ahead loop in {int((a != b).sum())} elements'
        assert float(a.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(FORCED))
@pytest.mark.parametrize('cfg', RING_TILES, ids=TILE_IDS)
def test_ring_equals_one_step_ahead_loop(cfg, name, dev):
    row = FORCED[name]
    for poison in (False, True):
        ring, _ = run(row, dev, cfg, 0, poison)
        ahead, _ = run(row, dev, cfg, 1, poison)
        for e in (ring, ahead):
            for what in ('fwd', 'dgrad'):
                assert e.names[what] == {expected_instance(row[0], row[1], what, cfg)}, (name, what, sorted(e.names[what]))
        assert_same_bits(ring, ahead, f'{name} tile {cfg}' + (' (poisoned LDS)' if poison else ''))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(FOLD))
def test_ring_on_folded_short_sequences(name, dev):
    geom, opts, ffold, bfold = FOLD[name]
    for poison in (False, True):
        ring, _ = run((geom, opts), dev, -1, 0, poison)
        ahead, _ = run((geom, opts), dev, -1, 1, poison)
        for e in (ring, ahead):
            for what, fold in (('fwd', ffold), ('dgrad', bfold)):
                _, _, _, _, _, xfk, epi = lean_call(geom, opts, what)
                if fold:
                    assert e.names[what] == {lean_name(6, xfk, epi, True)}, (name, what, sorted(e.names[what]))
                else:
                    assert len(e.names[what]) == 1 and all(n.startswith('conv_lean_kernel<') and n.endswith(f',{xfk},{epi}>') for n in e.names[what]), \
                        (name, what, sorted(e.names[what]))
        assert_same_bits(ring, ahead, name + (' (poisoned LDS)' if poison else ''))
