"""The rows of test_film_block_fwd_edges_gpu.py (tdvc_film_block_fwd: dilated conv + FiLM + 1x1 conv + residual + MRF sum, 16
channels), their seeded inputs and the float64 reference of both stages. No GPU: test_lean_edges_cpu.py screens the rows for the
LeakyReLU kink and checks the reference against a naive loop nest."""
import torch
import torch.nn.functional as F

from edge_support import SLOPE

# name: (K, d, T, options); B = 3, C = 16
ROWS = {r[0]: r[1:] for r in [
    ('k3_d1_T512_film_acc_views', 3, 1, 512, dict(film=True, acc=True, views=True)),      # the minimum T, everything strided
    ('k11_d5_T516_nofilm', 11, 5, 516, dict(film=False, acc=True)),      # the third tile has 4 columns, its whole left halo lies in tile 1
    ('k7_d3_T764_film', 7, 3, 764, dict(film=True, acc=False, views=True)),      # a 252-column last tile
    ('k15_d2_T520_nobias_scale0', 15, 2, 520, dict(film=True, acc=True, b1=False, b2=False, scale=0.0)),      # wnp == FB_WVP; scale 0 means 1
    ('k13_d5_T640_span80', 13, 5, 640, dict(film=True, acc=False)),      # span / 4 == 80 == FB_XSP
    ('k3_d31_T512_span80', 3, 31, 512, dict(film=False, acc=False, views=True)),      # the same limit by dilation
    # even K with pad 3; acc and out are views while x, h and gb are contiguous: five batch strides of two kinds
    ('k4_d2_T512_even', 4, 2, 512, dict(film=True, acc=True, views=('acc', 'y'))),
    ('k1_d7_T512_nohalo', 1, 7, 512, dict(film=True, acc=False, views=True)),      # no halo
]}


def lrelu(t):
    return F.leaky_relu(t, SLOPE)


def conv_h64(x, w1, b1, K, d):
    """float64 h: reflect-padded dilated conv of lrelu(x) plus b1, and the same on absolute values (without the bias)."""
    pad = (K - 1) * d // 2
    assert 2 * pad == (K - 1) * d, f'K = {K}, d = {d}: the field (K - 1) d is odd, no symmetric padding'
    padr = (lambda t: F.pad(t, (pad, pad), mode='reflect')) if pad else (lambda t: t)
    h = F.conv1d(padr(lrelu(x.double())), w1.double(), b1.double() if b1 is not None else None, dilation=d)
    return h, F.conv1d(padr(lrelu(x.double()).abs()), w1.double().abs(), None, dilation=d)


def out64(h, x, gb, w2, b2, acc, scale):
    """float64 out from a given h (fp32 values of the GPU, or float64), and A of its bound; also (h2, H) for the kink assertion."""
    h = h.double()
    if gb is not None:
        ga, be = gb.double()[:, :16], gb.double()[:, 16:]
        h2, H = h * (1 + ga) + be, h.abs() * (1 + ga.abs()) + be.abs()
    else:
        h2, H = h, h.abs()
    w = w2.double().view(16, 16, 1)
    z = F.conv1d(lrelu(h2), w, b2.double() if b2 is not None else None) + x.double()
    A = F.conv1d(H, w.abs(), b2.double().abs() if b2 is not None else None) + x.double().abs()
    out, A = scale * z, scale * A
    if acc is not None:
        out, A = out + acc.double(), A + acc.double().abs()
    return out, A, h2, H


def block_data(name, K, d, T, B=3, C_=16, film=True, acc=True, b1=True, b2=True, scale=1.0 / 3, **_):
    """The fp32-valued inputs of a row (CPU), seeded by its name."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *sh: torch.randn(*sh, generator=gen).float()
    return dict(x=rnd(B, C_, T), w1=rnd(C_, C_, K) / (C_ * K) ** 0.5, b1=rnd(C_) * 0.1 if b1 else None, w2=rnd(C_, C_) / C_ ** 0.5,
                b2=rnd(C_) * 0.1 if b2 else None, gb=rnd(B, 2 * C_, T) * 0.5 if film else None, acc=rnd(B, C_, T) if acc else None,
                scale=scale, eff_scale=scale if scale != 0.0 else 1.0)
