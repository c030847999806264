"""The workspace queries of the FiLM conditioning backward against a Python mirror of film_cond_plan (film_cond_bwd.hip), for every row
of test_film_cond_bwd_edges_gpu.py. tdvc_film_cond_bwd_workspace() / tdvc_film_cond0_bwd_workspace() are host code: no GPU needed.

The GPU rows that exist for a block walking several chunks, crossing from one sample into the next or covering three samples depend on
plan figures (chunks per block, blocks, chunks per sample). A plan change that silently turns them back into one-chunk blocks fails here."""
import importlib

import pytest

from film_cond_cases import CASES, COND0, FUSED, NV

CHUNK = {FUSED: 60, COND0: 64}


def cond_plan(B, T, chunk):
    """-> (chunks per sample, chunks per block, blocks): at most 512 blocks (one resident wave, 2 per CU) walk the B * ntile chunks."""
    ntile = -(-T // chunk)
    nchunks = B * ntile
    nb = min(nchunks, 512)
    tpb = -(-nchunks // nb)
    return ntile, tpb, -(-nchunks // tpb)


def _query(which):
    lib = importlib.import_module('td-vc-gan_amd')._lib.lib()
    return lib.tdvc_film_cond_bwd_workspace if which == FUSED else lib.tdvc_film_cond0_bwd_workspace


@pytest.mark.parametrize('which', [FUSED, COND0])
@pytest.mark.parametrize('name', list(CASES))
def test_workspace_query_matches_the_plan(name, which):
    """One [24][nc] slab per block, and one [3][nc] dk3 slot per (block, sample) pair: a block's samples start where the previous
    block's end, so nblocks + B slots are enough."""
    _, (nc, C2, T, B), _ = CASES[name]
    ntile, tpb, nblocks = cond_plan(B, T, CHUNK[which])
    assert _query(which)(B, T, nc, NV) == (nblocks * 24 + (nblocks + B) * 3) * nc * 4, (name, which, ntile, tpb, nblocks)
    for n_var in (4, 7, 9, 16):
        assert _query(which)(B, T, nc, n_var) == 0


# row: {entry point: (chunks per sample, chunks per block, blocks, chunks of the last block)}
WALKS = {
    'walk_tpb2_straddle_bits': {FUSED: (3, 2, 300, 2), COND0: (3, 2, 300, 2)},
    'walk_tpb3_three_samples': {FUSED: (1, 3, 344, 1), COND0: (1, 3, 344, 1)},
    'walk_tpb3_fp32': {FUSED: (2, 3, 347, 2), COND0: (1, 2, 260, 2)},
}
CROSSES = {('walk_tpb2_straddle_bits', FUSED), ('walk_tpb2_straddle_bits', COND0), ('walk_tpb3_fp32', FUSED)}


@pytest.mark.parametrize('which', [FUSED, COND0])
@pytest.mark.parametrize('name', list(WALKS))
def test_walk_rows_still_walk_and_straddle(name, which):
    _, (nc, C2, T, B), _ = CASES[name]
    ntile, tpb, nblocks = cond_plan(B, T, CHUNK[which])
    last = B * ntile - (nblocks - 1) * tpb
    assert (ntile, tpb, nblocks, last) == WALKS[name][which], (name, which, ntile, tpb, nblocks, last)
    assert tpb >= 2
    if (name, which) in CROSSES:      # a block range that does not divide the sample: some block crosses into the next sample mid-sample
        assert ntile % tpb != 0
    if name == 'walk_tpb3_three_samples':      # one chunk per sample: every full block covers three samples, slots 4k .. 4k + 2 of 4k + 3
        assert ntile == 1 and tpb == 3
    if (name, which) == ('walk_tpb3_fp32', COND0):      # blocks of two whole samples
        assert ntile == 1 and B % tpb == 0


def test_small_rows_are_one_chunk_blocks():
    """Everything but the walk rows has fewer than 512 chunks: tpb = 1, one block per chunk."""
    for name, (_, (nc, C2, T, B), _) in CASES.items():
        for which in (FUSED, COND0):
            ntile, tpb, nblocks = cond_plan(B, T, CHUNK[which])
            assert (tpb == 1 and nblocks == B * ntile) == (name not in WALKS), (name, which)
