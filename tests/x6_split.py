"""The split-bf16 x6 scheme of csrc/split_bf16.h restated in numpy: the three-piece split, the operands of the one-product rows and
the index function of the weight-plane image (tdvc_conv_x6_weight_planes). test_x6_split_cpu.py derives and asserts the figures the
one-product bar rests on; test_x6_fwd_edges_gpu.py builds its rows and decodes the planes with what is here."""
import numpy as np

F32, U32 = np.float32, np.uint32
X6_CP = 160                              # padded input-channel count of the plane image: 5 chunks of 32
ONE_PRODUCT_BOUND = 2.0 ** -20
PLANE_GEOM = [(32, 65), (64, 136), (96, 100), (128, 72), (160, 160)]


def split3(x):
    """x6_split: x = hi + mid + lo exactly, each piece the upper 16 bits of its fp32 word (a bf16 value)."""
    x = np.ascontiguousarray(x, dtype=F32)
    top = lambda v: (v.view(U32) & U32(0xffff0000)).view(F32)
    h = top(x)
    r1 = (x - h).astype(F32)
    m = top(r1)
    r2 = (r1 - m).astype(F32)
    return h, m, top(r2)                 # lo's lower half is zero by construction; the pack drops it


def constructed(rng, shape):
    """-> (fp32 values s 2^e (h 2^16 + m 2^8 + l) 2^-23, h, m, l, e, s) with h, m, l in [128, 255], e in [-20, 20]."""
    h, m, l = (rng.integers(128, 256, size=shape) for _ in range(3))
    e = rng.integers(-20, 21, size=shape)
    s = rng.choice(np.array([-1.0, 1.0]), size=shape)
    v = s * (h * 65536.0 + m * 256.0 + l) * 2.0 ** (e - 23.0)
    assert np.array_equal(v.astype(F32).astype(np.float64), v), 'a constructed value does not fit fp32 exactly'
    return v.astype(F32), h, m, l, e, s


def x6_mt(Cout):
    return 64 if Cout % 64 == 0 else 32


def planes_bytes(Cout):
    """Bytes of the plane image: three pieces x Cout x 3 taps x 160 padded channels, bf16."""
    return 3 * Cout * 3 * X6_CP * 2


def plane_offsets(Cout):
    """Element offset of (piece, co, tap, ci) in the image [Cout / MT][5 chunks][MT / 32][piece][32 co][tap][32 ci] -> int64
    array [3][Cout][3][160]. MT = 64 iff Cout % 64 == 0: the 32-channel chunk of one block's MT output channels is one linear run."""
    assert Cout % 32 == 0, f'no plane image for Cout = {Cout}'
    cbn = x6_mt(Cout) // 32
    pc, co, j, ci = np.ix_(np.arange(3), np.arange(Cout), np.arange(3), np.arange(X6_CP))
    blk, cb, co32 = co // (32 * cbn), (co // 32) % cbn, co % 32
    rec = (blk * 5 + ci // 32) * cbn + cb
    return (((rec * 3 + pc) * 32 + co32) * 3 + j) * 32 + ci % 32


def decode_planes(words, Cout):
    """uint16 image -> fp32 pieces [3][Cout][3][160]."""
    words = np.ascontiguousarray(words).view(np.uint16)
    assert words.size == planes_bytes(Cout) // 2, (words.size, planes_bytes(Cout) // 2)
    return (words[plane_offsets(Cout)].astype(U32) << U32(16)).view(F32)
