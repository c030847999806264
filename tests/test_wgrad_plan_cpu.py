"""The weight-grad workspace query against a Python mirror of its grid plans (wgrad_lean_plan in conv_wgrad_lean.hip, wgrad_x6_plan in
conv_wgrad_x6.hip), for every case of test_lean_wgrad_edges_gpu.py. tdvc_conv_wgrad_workspace() is host code: no GPU needed.

The GPU cases that exist for a block walking several chunks, or crossing from one sample into the next, depend on plan figures
(chunks per block, slabs, chunks per sample). A plan change that silently turns them back into one-chunk blocks fails here."""
import ctypes as C
import importlib

import pytest

from wgrad_cases import CASES, NARROW, X6


def prefers_ct32(cin):
    return ((cin + 31) // 32 * 32) * 10 < ((cin + 63) // 64 * 64) * 9


def lean_plan(R, cin, N, K, B):
    """-> (chunks per sample, chunks per block, slabs). The narrow kernel groups the chunks of each sample on their own (a block never
    leaves its sample); the wide kernels group the B * chunks-per-sample (sample, chunk) pairs in one run."""
    narrow = R <= 16 or cin <= 16
    ntc = 256 if narrow else 64
    mt = 16 if narrow else (32 if (R <= 32 or K >= 11) else 64)
    ctw = 16 if narrow else (64 if (K <= 3 and not prefers_ct32(cin)) else 32)
    ntiles = -(-N // ntc)
    tiles = -(-R // mt) * -(-cin // ctw)
    if narrow:
        t = max(1, min(B * ntiles * tiles // 1024, ntiles))
        return ntiles, t, B * -(-ntiles // t)
    groups = 1 if tiles >= 512 else 512 // tiles
    t = max(1, min(-(-B * ntiles // groups), B * ntiles))
    return ntiles, t, -(-B * ntiles // t)


def x6_ok(R, cin, T, K, dil, pad, reflect, w_cin):
    return K == 3 and dil == 1 and pad == 1 and not reflect and not w_cin and 64 < cin <= 144 and R >= 32 and R % 32 == 0 and T >= 64 and T % 4 == 0


def x6_plan(R, T, B):
    ntiles = -(-T // 32)
    nchunks = B * ntiles
    grp = max(1, min(768 // (R // 32), nchunks))
    tpb = -(-nchunks // grp)
    return ntiles, tpb, -(-nchunks // tpb)


def plans(name):
    """-> {route: (chunks per sample, chunks per block, slabs)} of the routes the case's descriptor admits."""
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T), opts, kclass, _ = CASES[name]
    B = opts.get('B', 3)
    out = {'lean': lean_plan(cout, cin, T, k, B)}
    if x6_ok(cout, cin, T, k, d, p, reflect, opts.get('w_cin', 0)):
        out['x6'] = x6_plan(cout, T, B)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_workspace_query_matches_the_plan(name):
    pkg = importlib.import_module('td-vc-gan_amd')
    (_, cin, cout, k, s, p, d, g, reflect, transposed, out_pad, T), opts, kclass, _ = CASES[name]
    spec = pkg.ops.ConvSpec(cin, cout, k, s, p, d, g, reflect, transposed, out_pad, opts.get('w_cin', 0), opts.get('w_cin_off', 0))
    assert spec.tout(T) == T
    query = pkg._lib.lib().tdvc_conv_wgrad_workspace(C.byref(spec.desc(opts.get('B', 3), T)))
    routes = plans(name)
    assert ('x6' in routes) == (kclass == X6), (name, sorted(routes))
    wsize = cout * cin * k
    assert query == max(nslab for _, _, nslab in routes.values()) * (wsize + cout) * 4, (name, query, routes)


# case: (route it takes, chunks per block, slabs)
STRADDLE = {'nar_var_window_tpb2': ('lean', 2, 115), 'nar_tpb2_odd_chunks': ('lean', 2, 130), 'pipe_straddle_k7_d3': ('lean', 2, 38),
            'pipe_deep_k3_d3': ('lean', 3, 44), 'x6_65_256_T1028': ('x6', 2, 50)}


@pytest.mark.parametrize('name', list(STRADDLE))
def test_multi_chunk_cases_still_walk_and_straddle(name):
    route, tpb, nslab = STRADDLE[name]
    per_sample, got_tpb, got_nslab = plans(name)[route]
    assert (got_tpb, got_nslab) == (tpb, nslab), (name, per_sample, got_tpb, got_nslab)
    if CASES[name][2] == NARROW:      # groups per sample; 10 chunks make 5 full groups, 9 chunks leave the last group one chunk
        assert nslab == CASES[name][1]['B'] * -(-per_sample // tpb)
        assert per_sample == (9 if name == 'nar_tpb2_odd_chunks' else 10)
    else:                             # a block range that does not divide the sample: some block crosses into the next sample
        assert per_sample % tpb != 0, (name, per_sample, tpb)
