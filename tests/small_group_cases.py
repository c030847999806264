"""The case table of test_small_group_conv_edges_gpu.py (the 4 -> 4-channels-per-group kernels of conv_small_group.hip) and the kernel
families its cases assert by trace. No GPU: test_small_group_plan_cpu.py checks that every case sits on the edge named beside it."""

SG_WGRAD, MFMA_WGRAD, SCALAR_WGRAD = 'small_group_wgrad_kernel', 'conv_wgrad_kernel<1,', 'conv_wgrad_scalar_kernel<'
WGRAD_MFMA_J = (1, 2, 3, 5, 7, 11)      # the generic MFMA weight-grad's instances (conv_mfma.hip: wgrad_mfma_supported)


def geom(name, K, s, pad, T, G=16):
    """(name, cin, cout, K, stride, pad, dil, groups, reflect, transposed, out_pad, T) of a 4 -> 4-channels-per-group conv."""
    return (name, 4 * G, 4 * G, K, s, pad, 1, G, False, False, 0, T)


# name -> (geometry, Edge options, out_scale, weight-grad kernel asserted by trace, (Tout, XW, M) the case is there for)
# XW = T + 2 pad + s: the weight-grad's padded input row (limit 384); M = (T - 1 + pad) / s + 1: columns of the input-grad.
CASES = {
    # Tout = 64: one full forward tile, two input-grad tiles, the weight-grad at its 4 * Tout == 256 limit
    'tile64': (geom('tile64', 41, 4, 20, 256), dict(post=1), 1.0, SG_WGRAD, (64, 300, 69)),
    # Tout = 65: one column in the second tile; the weight-grad declines
    'tile65': (geom('tile65', 41, 4, 20, 260), dict(post=1), 1.0, MFMA_WGRAD, (65, 304, 70)),
    # u0 = 4 m - 18: scalar dx stores; the lane with u0 = -2 writes only t = 0, 1
    'pad18': (geom('pad18', 41, 4, 18, 256), dict(post=1), 1.0, SG_WGRAD, (63, 296, 69)),
    'odd_T': (geom('odd_T', 41, 4, 20, 253), dict(post=1), 1.0, SG_WGRAD, (64, 297, 69)),
    # wider batch strides, planes that are not 16-byte aligned, no bias, dbias = NULL, a dy scale
    'views': (geom('views', 41, 4, 20, 250), dict(views=True, bias=False, with_db=False), 0.5, SG_WGRAD, (63, 294, 68)),
    # 16 K == 768 (forward registers) and 16 J s == 768 (input-grad registers), J = 24
    's2_k48': (geom('s2_k48', 48, 2, 23, 129), dict(post=1), 1.0, SG_WGRAD, (64, 177, 76)),
    # J = 24 with the last tap (k = 47) past K
    's2_k47': (geom('s2_k47', 47, 2, 23, 128), dict(post=1), 1.0, SG_WGRAD, (64, 176, 76)),
    # XW = 384: all six staging roles of the weight-grad full; the forward stages its window (552 positions) in two passes
    's8_xw384': (geom('s8_xw384', 48, 8, 20, 336), dict(post=1), 1.0, SG_WGRAD, (42, 384, 45)),
    # XW = 385: the weight-grad declines; J = 6 has no MFMA instance
    's8_xw385': (geom('s8_xw385', 48, 8, 20, 337), dict(post=1), 1.0, SCALAR_WGRAD, (42, 385, 45)),
    # K < s, J = 1, pad 0: phase 3 of dx is exactly 0
    'k3_s4': (geom('k3_s4', 3, 4, 0, 101), dict(pre=1, post=1), 1.0, SG_WGRAD, (25, 105, 26)),
    'k5_s8': (geom('k5_s8', 5, 8, 2, 64), dict(post=1), 1.0, SG_WGRAD, (8, 76, 9)),
    # Tout = 1: the input is shorter than the kernel
    'T2': (geom('T2', 41, 4, 20, 2), dict(post=1), 1.0, SG_WGRAD, (1, 46, 6)),
    # the last block of forward and input-grad: three live waves, one dead
    'g19': (geom('g19', 41, 4, 20, 250, G=19), dict(post=1), 1.0, SG_WGRAD, (63, 294, 68)),
    # act_in in the forward and the weight-grad
    'pre': (geom('pre', 41, 4, 20, 250), dict(pre=1), 1.0, SG_WGRAD, (63, 294, 68)),
    # POST_TANH in the forward; XF_MASK_TANH keeps input-grad and weight-grad off the route (J = 3: the MFMA weight-grad)
    'tanh': (geom('tanh', 9, 4, 4, 256), dict(post=2), 1.0, MFMA_WGRAD, (64, 268, 65)),
    # strides without a forward / input-grad instance: those launchers decline, the weight-grad takes the stride at run time
    's3': (geom('s3', 7, 3, 3, 100), dict(post=1), 1.0, SG_WGRAD, (34, 109, 35)),
    's5': (geom('s5', 10, 5, 3, 150), dict(post=1), 1.0, SG_WGRAD, (30, 161, 31)),
    's7': (geom('s7', 16, 7, 5, 200), dict(post=1), 1.0, SG_WGRAD, (28, 217, 30)),
}
SPLIT_B = (7, 8, 10, 11)      # the weight-grad's sample split (nsplit = 4 from B = 8 on) runs at the tile64 geometry


def small_group_desc(g):
    """small_group_ok() of conv_api.hip without its off switches."""
    (_, cin, cout, k, s, p, d, G, reflect, transposed, _, T) = g
    return not transposed and G >= 16 and cin == 4 * G and cout == 4 * G and d == 1 and not reflect and 2 <= s <= 8 and k <= 48


def small_group_families(name):
    """Kernel name prefixes of (forward, input-grad with the PLAIN epilogue and dy_xf NONE / MASK_LRELU, weight-grad)."""
    g, opts, _, wg, _ = CASES[name]
    s = g[4]
    if s in (2, 4, 8):
        return f'small_group_fwd_kernel<{s}>', f'small_group_dgrad_kernel<{s}>', wg
    return 'conv_gemm_kernel<1,', 'conv_gemm_kernel<2,', wg      # MODE_DOWN forward, MODE_UP input-grad
