"""CPU-side checks of the two edge suites test_lean_conv_edges_gpu.py and test_film_block_fwd_edges_gpu.py (their tables and mirrors:
lean_cases.py, film_block_ref.py): what their GPU cases rely on but a GPU run would not tell apart from a kernel defect.

  * every seeded case passes its kink assertion (a case that does not would fail on the GPU for a reason of the data);
  * the film-block float64 reference equals a naive loop nest at (K, d, T) = (3, 2, 12), C = 16;
  * the instances the case tables assert by trace are together all that lean_launch2 and lean_launch_fold can launch at the shapes
    of this suite;
  * the chunk-footprint mirror of launch_conv_lean reproduces the hand figures of its docstring.
"""
import pytest
import torch

import film_block_ref as FB
import lean_cases as LE
from conv_edge import Edge
from edge_support import SLOPE, U
from lean_cases import LEAN_CFG

CPU = torch.device('cpu')
SEEDED = {**{n: c[:2] for n, c in LE.CASES.items()}, LE.WINDOW[0][0]: LE.WINDOW, **{n: c[:2] for n, c in LE.FILM_K3.items()},
          **{n: c[:2] for n, c in LE.FOLD_ROWS.items()}, **{n: c[:2] for n, c in LE.REROUTES.items()}}


@pytest.mark.parametrize('name', list(SEEDED))
def test_seeded_lean_case_is_off_the_kink(name):
    geom, opts = SEEDED[name]
    e = Edge(geom, CPU, **{**dict(wt=True, nan_spare=True), **opts})
    e.assert_off_kink()
    assert e.film == bool(opts.get('film'))


@pytest.mark.parametrize('name', list(FB.ROWS))
def test_seeded_film_block_row_is_off_the_kink(name):
    """The GPU test makes the decisive assertion, on the h the kernel stored. Here the same assertion runs on the float64 h rounded to
    fp32, the closest stand-in the CPU has: a row that fails this screen would almost surely fail there for a reason of its data."""
    K, d, T, opts = FB.ROWS[name]
    D = FB.block_data(name, K, d, T, **opts)
    h, _ = FB.conv_h64(D['x'], D['w1'], D['b1'], K, d)
    _, _, h2, H = FB.out64(h.float(), D['x'], D['gb'], D['w2'], D['b2'], D['acc'], D['eff_scale'])
    if D['gb'] is not None:
        assert bool((h2.abs() > 3 * U * H).all()), 'an element of h2 sits on the LeakyReLU kink: reseed (rename) the row'


def test_film_block_reference_equals_naive_loops():
    K, d, T, B = 3, 2, 12, 2
    D = FB.block_data('naive', K, d, T, B=B, film=True, acc=True)
    h, _ = FB.conv_h64(D['x'], D['w1'], D['b1'], K, d)
    out, _, _, _ = FB.out64(h, D['x'], D['gb'], D['w2'], D['b2'], D['acc'], D['eff_scale'])
    x, w1, b1, w2, b2, gb, acc = (D[k].double() for k in ('x', 'w1', 'b1', 'w2', 'b2', 'gb', 'acc'))
    lr = lambda v: v if v > 0 else SLOPE * v
    pad = (K - 1) * d // 2
    refl = lambda q: -q if q < 0 else (2 * (T - 1) - q if q >= T else q)
    hn, on = torch.zeros(B, 16, T, dtype=torch.float64), torch.zeros(B, 16, T, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            for co in range(16):
                s = float(b1[co])
                for ci in range(16):
                    for k in range(K):
                        s += float(w1[co, ci, k]) * lr(float(x[b, ci, refl(t - pad + k * d)]))
                hn[b, co, t] = s
            a2 = [lr(float(hn[b, c, t]) * (1 + float(gb[b, c, t])) + float(gb[b, 16 + c, t])) for c in range(16)]
            for co in range(16):
                s = float(b2[co]) + sum(float(w2[co, c]) * a2[c] for c in range(16)) + float(x[b, co, t])
                on[b, co, t] = D['eff_scale'] * s + float(acc[b, co, t])
    assert float((h - hn).abs().max()) < 1e-12 and float((out - on).abs().max()) < 1e-12


def test_case_tables_name_every_lean_instance():
    """lean_launch2: 8 tiles x 6 (prologue, epilogue) pairs; lean_launch_fold: 3 pairs on the 32 x 64 tile. The folded 64 x 64 tile needs
    ceil(Cout / 64) * ceil(B / fold) >= 1024 blocks (launch_conv_lean), i.e. Cout * B >= 2^18 at T = 16: no shape of this suite, and no
    launch of the train step, comes near it, so its three instances stay outside the tables; that is said here, not passed over."""
    pairs = [(LE.LXF_ACT, LE.EPI_FWD), (LE.LXF_FILM, LE.EPI_FWD), (LE.LXF_ACT, LE.EPI_MASK), (LE.LXF_ACT, LE.EPI_FILM),
             (LE.LXF_ACT, LE.EPI_PLAIN), (LE.LXF_MASK_LRELU, LE.EPI_PLAIN)]
    fold_pairs = [(LE.LXF_ACT, LE.EPI_FWD), (LE.LXF_ACT, LE.EPI_PLAIN), (LE.LXF_MASK_LRELU, LE.EPI_PLAIN)]
    want = {LE.lean_name(c, x, e) for c in LEAN_CFG for x, e in pairs} | {LE.lean_name(6, x, e, True) for x, e in fold_pairs}
    assert len(want) == 51
    got = LE.expected_instances()
    assert want - got == set(), sorted(want - got)
    assert got - want == set(), sorted(got - want)      # nothing is expected that the launcher has no instance for


def test_chunk_footprint_figures():
    fp = LE.lean_footprint
    assert [fp(c, 11, 5, 25, 0, 1)[0] for c in (4, 8, 12)] == [16528, 23976, 34888]
    assert fp(16, 11, 5, 25, 0, 1)[2] == 7      # weight passes: one more than the 32-row tiles prefetch
    assert [fp(c, 11, 5, 25, 25, 1)[0] for c in (4, 12)] == [14352, 36424]
    assert LE.lean_chunk(32, 11, 5, 25, 0, 1, LE.LXF_ACT) == 12
    assert LE.lean_chunk(32, 11, 5, 25, 0, 1, LE.LXF_ACT, 16528) == 4
    assert LE.lean_chunk(32, 11, 5, 25, 0, 1, LE.LXF_ACT, 34888) == 12
    assert LE.lean_chunk(32, 11, 5, 25, 0, 1, LE.LXF_ACT, 16524) == 0
    # deep_256x16_k3_T64: the 16-row tiles may take up to 64 channels; at 64 columns 56 is what the 4 input passes hold (4 x 14 rows)
    assert LE.lean_chunk(256, 3, 1, 1, 0, 3, LE.LXF_ACT) == 56 and LE.lean_footprint(64, 3, 1, 1, 0, 3)[1] == 5
    assert LE.lean_chunk(256, 3, 1, 1, 0, 0, LE.LXF_ACT) == 16      # ... and 16 on the 16 x 256 tile (6 input passes of 3 rows)
    assert LE.lean_chunk(256, 3, 1, 1, 0, 6, LE.LXF_ACT) == 32
