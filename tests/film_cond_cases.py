"""The case table of test_film_cond_bwd_edges_gpu.py (the FiLM conditioning backward kernels). No GPU: test_cond_plan_cpu.py checks the
plan figures quoted beside the rows (chunks per block, blocks, straddling)."""

NV = 8                                   # excitation channels: the last 8 input channels of cond_var.0
FUSED, COND0 = 'fused', 'cond0'

# name, (nc, C2, T, B), options. Every row runs on the fused kernel (chunks of 60 steps + a 2-column halo either side) and on
# cond0 (chunks of 64) unless `only` says otherwise. Options: mask = 'bits' (fused: sign words, cv0 = NULL) | 'fp32';
# views: dgb, exc, dexc, cv0 / dcv are channel slices [:, :C] of [B, C + 4, T] buffers; bits_views: the sign words are a slice of
# [B, nc + 2, T / 32]; dexc / dw / ws = False: that pointer is NULL; slope: LeakyReLU slope of the mask (0.2).
CASES = {c[0]: c for c in [
    # minimum of every dimension; the dk3 deltas at t = 0 and t = T - 1 in one k-step; one 12-row channel tile, eight empty ones
    ('min_T4', (12, 32, 4, 3), dict()),
    # exactly one channel tile; exactly one fused chunk (column 61 = T - 1); cond0: 60 of 64 columns
    ('one_tile_nc16', (16, 32, 60, 2), dict()),
    # nw = 1: words 1, 2 of every 3-word window are out of range
    ('bits_T32', (136, 32, 32, 5), dict(mask='bits')),
    # fused chunk 1 (n0 = 60) wants words 1 .. 3 of 3; cond0: the second chunk is 32 wide
    ('bits_T96_past_last_word', (136, 64, 96, 3), dict(mask='bits')),
    # fused: the second chunk has 4 columns and holds the T - 1 delta; cond0: exactly one chunk
    ('seam_T64', (100, 32, 64, 3), dict()),
    # cond0: the second chunk has 4 columns
    ('seam_T68', (72, 32, 68, 2), dict()),
    # fused chunk 1 ends on T - 1: the generic indicator path of stage (b)
    ('T120_not_interior', (136, 32, 120, 2), dict()),
    # fused chunk 1 is interior (constant-indicator fast path), chunk 2 has 4 columns
    ('T124_interior', (136, 32, 124, 2), dict()),
    # full 144 rows, no zero tile; an interior chunk on the bits path; the last fused chunk is 8 wide; cond0: two exact chunks
    ('bits_T128', (144, 32, 128, 2), dict(mask='bits')),
    # six reduction steps of the software-pipelined d_cv0 product
    ('ncc6', (136, 96, 64, 2), dict()),
    # ten steps; 140 = 8 3/4 channel tiles
    ('ncc10_nc140', (140, 160, 64, 2), dict(mask='bits')),
    # every batch stride wider than contiguous; the spare channels of dexc stay SENT; fused: cv0 once more 4 bytes off alignment
    ('views', (136, 64, 132, 3), dict(views=True)),
    # cv0_sign_bits_bs
    ('bits_views', (136, 32, 64, 3), dict(mask='bits', bits_views=True)),
    # stage (a) and its barrier skipped; dk3 and dW0 unchanged against the reference
    ('no_dexc', (136, 32, 124, 2), dict(dexc=False)),
    # slots at offset 0 of the workspace; no slab fold, the dw0 buffer bit-identical
    ('no_dw_ws', (136, 32, 124, 3), dict(dw=False)),
    # atomics into the zeroed dk3
    ('no_dw_no_ws', (136, 32, 124, 3), dict(dw=False, ws=False)),
    # a hard-coded 0.2
    ('slope_001', (136, 32, 64, 2), dict(slope=0.01, only=FUSED)),
    # both plans: 3 chunks per sample, 600 chunks, tpb = 2, 300 blocks: every other block crosses a sample; dk3 from two slots per sample
    ('walk_tpb2_straddle_bits', (136, 32, 160, 200), dict(mask='bits')),
    # 1 chunk per sample, tpb = 3, 344 blocks, the last with one chunk: a block covers three samples and flushes dk3 every chunk;
    # slot 4k + 3 is never written and must never be read
    ('walk_tpb3_three_samples', (136, 32, 32, 1030), dict(mask='bits')),
    # fused: 2 chunks per sample, 1040 chunks, tpb = 3, 347 blocks, the last with two; cond0: tpb = 2, 260 blocks of two whole samples
    ('walk_tpb3_fp32', (136, 64, 64, 520), dict()),
]}
# not a row of the table: the valid call the refusal tests start from (views: every operand sits inside a wider buffer; T % 32 == 0)
REFUSAL_BASE = ('refusal_base', (136, 64, 64, 3), dict(views=True))
ROWS = [(n, w) for n, c in CASES.items() for w in (FUSED, COND0) if c[2].get('only', w) == w]
BITS_ROWS = [n for n, c in CASES.items() if c[2].get('mask') == 'bits']
