"""The case table of test_lean_wgrad_edges_gpu.py (the stride-1 'same' weight-grad kernels) and the route mirror of its forward and
input-grad calls. No GPU: test_wgrad_plan_cpu.py checks the plan figures quoted beside the cases (slabs, chunks per block, straddling)."""
from conv_edge import _g

NARROW, PIPE, PIPE_FILM, X6, TILE1, TILE2 = 'narrow', 'pipe', 'pipe-FiLM', 'x6', 'tile SCAL=1', 'tile SCAL=2'

# name: (geometry, Edge options, kernel class, weight-grad instance in the trace's spelling)
CASES = {c[0][0]: c for c in [
    # ---- narrow: conv_wgrad_lean_kernel<1,1,J,D>, 256-step chunks, slabs = B * groups per sample
    # odd T: scalar staging; the last chunk has 45 columns; MASK_LRELU stream on dy
    (_g('nar_d0_k15_T301', 1, 16, 15, 7, 1, True, 301), dict(post=1), NARROW, 'conv_wgrad_lean_kernel<1,1,15,1>'),
    # one chunk holds both mirror folds; the x window runs 150 columns past T
    (_g('nar_c16_k11_d5_T132', 16, 16, 11, 25, 5, True, 132), dict(pre=1), NARROW, 'conv_wgrad_lean_kernel<1,1,11,5>'),
    # chunk 0 on the padding path, chunks 1-3 on the vector path, chunk 4 has 4 columns; 10 slabs
    (_g('nar_c16_k7_d3_T1028', 16, 16, 7, 9, 3, True, 1028), dict(pre=1, B=2), NARROW, 'conv_wgrad_lean_kernel<1,1,7,3>'),
    # batch stride wider than contiguous, still aligned
    (_g('nar_c8_k5_T500_views', 8, 8, 5, 2, 1, False, 500), dict(pre=1, add=True, views=True), NARROW, 'conv_wgrad_lean_kernel<1,1,5,1>'),
    (_g('nar_c16_k3_unaligned', 16, 16, 3, 1, 1, False, 260), dict(unaligned=True), NARROW, 'conv_wgrad_lean_kernel<1,1,3,1>'),
    # 2070 blocks -> tpb = 2: 10 chunks in 5 groups per sample, 115 slabs, the last chunk has 4 columns; dw columns 0..127 stay dw0
    (_g('nar_var_window_tpb2', 8, 136, 3, 1, 1, False, 2308), dict(B=23, w_cin=136, w_cin_off=128, with_db=False), NARROW,
     'conv_wgrad_lean_kernel<1,1,3,1>'),
    # tpb = 2 WITH a bias gradient (the partial sums of a block's two chunks add up), 9 chunks per sample: the last group of each
    # sample is the 4-column chunk alone; 130 slabs
    (_g('nar_tpb2_odd_chunks', 8, 136, 3, 1, 1, False, 2052), dict(B=26, pre=1), NARROW, 'conv_wgrad_lean_kernel<1,1,3,1>'),
    # ---- pipe: conv_wgrad_pipe_kernel<M,C,J,D,XFILM>, aligned rows, dy plain
    # second row tile has 8 rows, 40 of 64 columns, last chunk 4 wide; 15 slabs
    (_g('pipe_72x40_k3', 40, 72, 3, 1, 1, False, 260), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<2,2,3,1,false>'),
    # 24 rows keep it off the split-bf16 kernel; 136 = 4 1/4 column tiles; 27 slabs
    (_g('pipe_24x136_k3', 136, 24, 3, 1, 1, False, 520), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<1,1,3,1,false>'),
    # 75 chunks, tpb = 2, 38 slabs, 15 chunks per sample: block 7 crosses samples 0 / 1, the last block has one chunk, reflect halos
    (_g('pipe_straddle_k7_d3', 128, 128, 7, 9, 3, True, 900), dict(pre=1, B=5), PIPE, 'conv_wgrad_pipe_kernel<2,1,7,3,false>'),
    # 132 chunks, tpb = 3, 44 slabs, 44 chunks per sample (44 % 3 != 0: straddles); odd walk length of the double buffer
    (_g('pipe_deep_k3_d3', 128, 256, 3, 3, 3, True, 2756), dict(), PIPE, 'conv_wgrad_pipe_kernel<2,2,3,3,false>'),
    # the widest span; the last chunk has 8 columns
    (_g('pipe_k11_d5_64', 64, 64, 11, 25, 5, True, 200), dict(pre=1), PIPE, 'conv_wgrad_pipe_kernel<1,1,11,5,false>'),
    # T <= 128 admitted as "wide"
    (_g('pipe_pw_96x100', 100, 96, 1, 0, 1, False, 68), dict(), PIPE, 'conv_wgrad_pipe_kernel<2,2,1,1,false>'),
    # beta planes start at channel 40 (no tile multiple), partial tiles both ways
    (_g('pipe_film_40', 40, 40, 1, 0, 1, False, 260), dict(film=True), PIPE_FILM, 'conv_wgrad_pipe_kernel<2,2,1,1,true>'),
    (_g('pipe_film_32', 32, 32, 1, 0, 1, False, 128), dict(film=True, B=2, with_db=False), PIPE_FILM, 'conv_wgrad_pipe_kernel<1,1,1,1,true>'),
    # ---- split-bf16: conv_wgrad_x6_kernel, 3 taps, 65 .. 144 input channels, T % 4 == 0, T >= 64
    # lower Cin end; 8 row blocks -> 99 chunks, tpb = 2, 50 slabs, 33 chunks per sample (straddles), the last chunk has 4 columns
    (_g('x6_65_256_T1028', 65, 256, 3, 1, 1, False, 1028), dict(pre=1), X6, 'conv_wgrad_x6_kernel'),
    # upper Cin end, minimum T
    (_g('x6_144_32_T64', 144, 32, 3, 1, 1, False, 64), dict(pre=1, B=5), X6, 'conv_wgrad_x6_kernel'),
    (_g('x6_136_64_T68_views', 136, 64, 3, 1, 1, False, 68), dict(views=True), X6, 'conv_wgrad_x6_kernel'),
    # T % 4 != 0: must NOT be the split-bf16 kernel
    (_g('x6_miss_T66', 136, 32, 3, 1, 1, False, 66), dict(pre=1), TILE1, 'conv_wgrad_tile_kernel<1,1,3,1,1>'),
    # ---- tile: conv_wgrad_tile_kernel<M,C,J,D,SCAL>
    # contiguous-run staging with a MASK_LRELU stream
    (_g('tile_d5_k5_T63', 128, 128, 5, 2, 1, False, 63), dict(post=1), TILE2, 'conv_wgrad_tile_kernel<2,1,5,1,2>'),
    # a batch stride % 4 != 0 breaks the contract of the contiguous-run staging
    (_g('tile_d5_k5_T63_views', 128, 128, 5, 2, 1, False, 63), dict(post=1, views=True), TILE1, 'conv_wgrad_tile_kernel<2,1,5,1,1>'),
    # aligned, but the dy mask keeps it off the pipe kernel; 5 chunks
    (_g('tile_mask_64_k5_T260', 64, 64, 5, 2, 1, False, 260), dict(post=1), TILE1, 'conv_wgrad_tile_kernel<2,1,5,1,1>'),
    (_g('tile_unaligned_48_k3', 48, 48, 3, 1, 1, False, 260), dict(unaligned=True, pre=1), TILE1, 'conv_wgrad_tile_kernel<2,2,3,1,1>'),
    # chunk mode 0, the element-wise fallback: FiLM prologue on rows that are not 16-byte aligned
    (_g('tile_film_64_T50', 64, 64, 1, 0, 1, False, 50), dict(film=True), TILE1, 'conv_wgrad_tile_kernel<2,2,1,1,1>'),
    # the two mirrors overlap
    (_g('tile_reflect_k11_d5_T30', 64, 64, 11, 25, 5, True, 30), dict(pre=1), TILE1, 'conv_wgrad_tile_kernel<2,1,11,5,1>'),
    # N = 1
    (_g('tile_pw_32x64_T1', 32, 64, 1, 0, 1, False, 1), dict(B=5), TILE2, 'conv_wgrad_tile_kernel<2,1,1,1,2>'),
    (_g('tile_pw_40x64_T1', 40, 64, 1, 0, 1, False, 1), dict(B=5), TILE1, 'conv_wgrad_tile_kernel<2,2,1,1,1>'),
    # the k3 fallback route of film_cond; dw columns 128..135 stay dw0
    (_g('tile_k3_T3_window', 128, 136, 3, 1, 1, False, 3), dict(B=4, w_cin=136, w_cin_off=0), TILE1, 'conv_wgrad_tile_kernel<2,2,3,1,1>'),
]}


def expected_route(e, what):
    """Kernel name prefix of a case's forward ('fwd') or input-grad ('dgrad'), by the rule of conv_api.hip: the lean kernel takes
    channel counts that are multiples of 4 (Cin forward, Cout backward, with the slot's transposed weight copy) at T <= 80 or at
    T % 4 == 0 with 16-byte aligned operands; it has no instance for a mask prologue together with a mask epilogue. The operator
    layer sends a plain 3-tap forward with 65 .. 160 input channels, Cout % 32 == 0 and T >= 128 to the split-bf16 forward."""
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T) = e.geom
    aligned = T % 4 == 0 and not e.unaligned
    if what == 'fwd' and k == 3 and d == 1 and p == 1 and not e.spec.w_cin and 64 < cin <= 160 and cout % 32 == 0 and T >= 128 and aligned \
            and not e.post and e.add_y is None and not e.film:
        return 'conv_fwd_x6_kernel<'
    ch = cin if what == 'fwd' else cout
    lean = ch % 4 == 0 and (T <= 80 or aligned)
    if what == 'dgrad' and e.post and e.pre:
        lean = False
    return 'conv_lean_kernel' if lean else 'conv_gemm_kernel<0,'
