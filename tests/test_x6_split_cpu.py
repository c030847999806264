"""The figures the one-product bar of test_x6_fwd_edges_gpu.py rests on, from the split-bf16 x6 scheme of csrc/split_bf16.h as x6_split.py
restates it in numpy. No GPU: the split is three truncations and two exact subtractions, a piece product is exact in fp32 (8 x 8 significant
bits), and with ONE nonzero product per output element the matrix pipe's accumulation is six fp32 additions in the committed order.

Operands of the one-product rows are s * 2^e * (h 2^16 + m 2^8 + l) * 2^-23 with h, m, l in [128, 255]: every piece is exactly
h, m or l (scaled) and none is small, so every one of the six products weighs at least 2^-18 of the whole and leaving any one of
them out is far outside
    |got - w x| <= 2^-20 |w x|,
while the full scheme stays below 8.1 * 2^-24: the three dropped products are below (2^-23 + 2^-32) |w x| and six additions round
by at most 6 * 2^-24. Both figures are asserted here, on 2e5 pairs.

Also here: the index function of the weight-plane image (tdvc_conv_x6_weight_planes; x6_split.plane_offsets, which the GPU file decodes
the planes with) is checked, and the byte count of that image against the host library.
"""
import importlib

import numpy as np
import pytest

from x6_split import F32, ONE_PRODUCT_BOUND, PLANE_GEOM, U32, constructed, plane_offsets, planes_bytes, split3, x6_mt

# (weight piece, activation piece) in the order x6_mfma issues them: smallest products first. 0 = hi, 1 = mid, 2 = lo
ORDER = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]
PRODUCT_NAMES = ['lo.hi', 'hi.lo', 'mid.mid', 'mid.hi', 'hi.mid', 'hi.hi']


def x6_product(w, x, omit=None):
    """The six piece products of one (w, x) pair summed in fp32 in the committed order, from c = 0; `omit`: index into ORDER left out."""
    pw, px = split3(w), split3(x)
    c = np.zeros(np.shape(w), dtype=F32)
    for k, (i, j) in enumerate(ORDER):
        if k != omit:
            c = (c + pw[i] * px[j]).astype(F32)      # the product has 16 significant bits: exact in fp32
    return c


N_PAIRS = 200_000


@pytest.fixture(scope='module')
def pairs():
    rng = np.random.default_rng(20240611)
    return constructed(rng, (N_PAIRS,)), constructed(rng, (N_PAIRS,))


def test_constructed_pieces_are_h_m_l(pairs):
    """The split of a constructed value gives back exactly h, m and l: none of the three pieces is small or empty."""
    for v, h, m, l, e, s in pairs:
        ph, pm, pl = (p.astype(np.float64) for p in split3(v))
        unit = s * 2.0 ** (e - 23.0)
        assert np.array_equal(ph, unit * h * 65536.0) and np.array_equal(pm, unit * m * 256.0) and np.array_equal(pl, unit * l)
        assert np.array_equal(ph + pm + pl, v.astype(np.float64))


def test_split_is_exact_on_any_fp32():
    """hi + mid + lo == x bit for bit on random fp32 values, +-0, the smallest normal and short mantissas; 8 significant bits per piece."""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(100_000).astype(F32), (rng.standard_normal(1000) * 1e-30).astype(F32),
                        np.array([0.0, -0.0, 2.0 ** -126, 1.0, -1.5, 3.0 * 2.0 ** 40], dtype=F32)])
    h, m, l = split3(x)
    assert np.array_equal((h.astype(np.float64) + m + l).astype(F32).view(U32) | (x.view(U32) & U32(0x80000000)), x.view(U32))
    for p in (h, m, l):
        assert not np.any(p.view(U32) & U32(0xffff))


def test_one_product_figures(pairs):
    """The full scheme's worst relative error is below 8.1 * 2^-24 (so 2^-20 leaves a factor of two); without any one of the six
    products every pair is at least 2^-18 off, four times the bar."""
    (w, *_), (x, *_) = pairs
    ref = w.astype(np.float64) * x.astype(np.float64)      # 48 significant bits: exact
    rel = lambda got: np.abs(got.astype(np.float64) - ref) / np.abs(ref)
    full = rel(x6_product(w, x))
    print(f'[x6 split] full scheme: worst {full.max() / 2.0 ** -24:.2f} * 2^-24 over {N_PAIRS} pairs')
    assert full.max() < 8.1 * 2.0 ** -24 < ONE_PRODUCT_BOUND / 1.9
    for k, name in enumerate(PRODUCT_NAMES):
        r = rel(x6_product(w, x, omit=k))
        print(f'[x6 split] without {name}: least {r.min() / 2.0 ** -20:.2f} * 2^-20')
        assert r.min() >= 2.0 ** -18 > 3.9 * ONE_PRODUCT_BOUND


@pytest.mark.parametrize('Cout,Cin', PLANE_GEOM + [(256, 136)])
def test_plane_image_layout_and_bytes(Cout, Cin):
    """The index function addresses every element of the image exactly once, a block's chunk is one linear run of MT / 32 records, and
    the host library reports the same byte count."""
    off = plane_offsets(Cout)
    n = planes_bytes(Cout) // 2
    assert np.array_equal(np.sort(off.ravel()), np.arange(n))
    mt = x6_mt(Cout)
    run = off[:, mt:2 * mt, :, 32:64] if Cout > mt else off[:, :mt, :, 32:64]      # block 1 (or the only one), chunk 1
    first = ((1 if Cout > mt else 0) * 5 + 1) * (mt // 32) * (3 * 32 * 3 * 32)
    assert run.min() == first and run.max() == first + (mt // 32) * (3 * 32 * 3 * 32) - 1
    lib = importlib.import_module('td-vc-gan_amd')._lib.lib()
    assert lib.tdvc_conv_x6_weight_planes_bytes(Cout, Cin, 3) == planes_bytes(Cout)


@pytest.mark.parametrize('Cout,Cin,K', [(48, 136, 3), (16, 136, 3), (33, 136, 3), (0, 136, 3), (64, 0, 3), (64, 161, 3), (64, 136, 5)])
def test_plane_bytes_refuses(Cout, Cin, K):
    """No image exists for Cout % 32 != 0 (no kernel could read it), Cin outside 1 .. 160 or K != 3: the byte count is 0."""
    lib = importlib.import_module('td-vc-gan_amd')._lib.lib()
    assert lib.tdvc_conv_x6_weight_planes_bytes(Cout, Cin, K) == 0
