"""The slab fold behind every weight-grad (slab_reduce_multi_kernel, conv_mfma.hip) on its own, through tdvc_debug_slab_fold.

  dst[map(i)] += slab[0][i] + ... + slab[nslab-1][i]

Every case runs the production kernel (float4 groups, the loads of up to 8 slabs in flight) and the one-load-per-slab reference
loop it replaced on equal inputs and requires
  * equal bits of the two results, gaps and guards included: the production kernel keeps the reference's order of additions
    per element (slab s0 .. s1-1 inside a y-block, then the y-blocks' partials in order);
  * the result within the fp32 bound of a sum of nslab + 1 terms against float64 (elem_check of edge_support:
    (terms + 8) * 2^-23 * sum|terms| + 2^-22 |ref|) and rel-L2 < 2e-5;
  * the sentinel in the columns between mapped rows and in the guards around dw / dbias.

Cases: n % 4 != 0 (scalar tail behind the float4 groups), slab rows that are not 16-byte aligned (stride % 4 != 0, slab pointer
4 bytes off: scalar groups), a w_cin row mapping with rows of 4k floats (one 16-byte read-modify-write per group) and of 7 (per
element), an unaligned dw, bias partials behind the weights with n_w % 4 == 0 and != 0 (a group straddles the boundary), nslab
1 / 8 / 9 / 41 (no split; one full batch of loads; batch + remainder and a 2-way split; 5- or 6-way split), several blocks, and
one fold longer than the grid (8192 blocks x 1024 elements) so that a thread walks on to a second group."""
import pytest
import torch

from common import rel_l2, traced
from edge_support import SENT, elem_check

pytestmark = pytest.mark.gpu
GUARD = 8
KERNEL = 'slab_reduce_multi_kernel'

# name: (rows, rowlen, dst_row_stride, nbias, stride_pad, slab_off, dw_off)   n_w = rows * rowlen, n = n_w + nbias,
# stride = n + stride_pad floats, slabs / dw start slab_off / dw_off floats behind a 16-byte boundary
LAYOUTS = {
    'flat_n1027': (1, 1027, 1027, 0, 1, 0, 0),
    'flat_n1027_stride_odd': (1, 1027, 1027, 0, 0, 0, 0),
    'flat_n5000_bias24': (1, 5000, 5000, 24, 0, 0, 0),
    'flat_n4098_bias5_slab_off': (1, 4098, 4098, 5, 1, 1, 0),
    'flat_n2048_dw_off': (1, 2048, 2048, 16, 0, 0, 1),
    'rows24x12_into20_bias24': (24, 12, 20, 24, 0, 0, 0),
    'rows24x12_into18': (24, 12, 18, 0, 0, 0, 0),
    'rows33x7_into11_bias33': (33, 7, 11, 33, 0, 0, 0),
    'rows16x16_bias16': (16, 16, 16, 16, 0, 0, 0),
}
NSLAB = (1, 8, 9, 41)


def _run(L, st, slabs, nslab, stride, n, dw, rowlen, drs, n_w, db, ref):
    L.check(L.lib().tdvc_debug_slab_fold(slabs.data_ptr(), nslab, stride, n, dw.data_ptr(), rowlen, drs, n_w,
                                         db.data_ptr() if db is not None else None, ref, st))


def _case(pkg, dev, layout, nslab, seed):
    rows, rowlen, drs, nbias, pad, slab_off, dw_off = layout
    L = pkg._lib
    st = torch.cuda.current_stream(dev).cuda_stream
    n_w = rows * rowlen
    n, stride = n_w + nbias, n_w + nbias + pad
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(nslab, stride, generator=g)
    dw0 = torch.randn(rows, rowlen, generator=g)
    db0 = torch.randn(nbias, generator=g)
    ref64 = src[:, :n].double().sum(0)
    A = src[:, :n].double().abs().sum(0)
    ref_w, A_w = dw0.double() + ref64[:n_w].view(rows, rowlen), dw0.double().abs() + A[:n_w].view(rows, rowlen)
    ref_b, A_b = db0.double() + ref64[n_w:], db0.double().abs() + A[n_w:]

    out = []
    for ref in (0, 1):
        sbuf = torch.full((slab_off + nslab * stride + GUARD,), SENT, device=dev)
        slabs = sbuf[slab_off:slab_off + nslab * stride]
        slabs.copy_(src.view(-1))
        wbuf = torch.full((GUARD + dw_off + rows * drs + GUARD,), SENT, device=dev)
        assert sbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
        dw = wbuf[GUARD + dw_off:GUARD + dw_off + rows * drs]
        dw.view(rows, drs)[:, :rowlen] = dw0.to(dev)
        bbuf = torch.full((GUARD + nbias + GUARD,), SENT, device=dev)
        db = bbuf[GUARD:GUARD + nbias] if nbias else None
        if nbias:
            db.copy_(db0)
        if ref:
            _run(L, st, slabs, nslab, stride, n, dw, rowlen, drs, n_w if nbias else -1, db, 1)
            torch.cuda.synchronize()
        else:
            with traced() as tr:
                _run(L, st, slabs, nslab, stride, n, dw, rowlen, drs, n_w if nbias else -1, db, 0)
            assert KERNEL in tr.names, sorted(tr.names)
        assert bool((sbuf[:slab_off] == SENT).all()) and bool((sbuf[slab_off + nslab * stride:] == SENT).all())
        out.append((wbuf.cpu(), bbuf.cpu()))
    (w_new, b_new), (w_ref, b_ref) = out
    assert torch.equal(w_new, w_ref), 'dw differs from the reference loop in bits'
    assert torch.equal(b_new, b_ref), 'dbias differs from the reference loop in bits'
    lo = GUARD + dw_off
    assert bool((w_new[:lo] == SENT).all()) and bool((w_new[lo + rows * drs:] == SENT).all())
    got_w = w_new[lo:lo + rows * drs].view(rows, drs)
    assert bool((got_w[:, rowlen:] == SENT).all()), 'columns between the mapped rows were written'
    ratio, inexact = elem_check(got_w[:, :rowlen].contiguous(), ref_w, A_w, nslab + 1)
    print(f'dw: rel-L2 {rel_l2(got_w[:, :rowlen], ref_w):.3g}, err / bound {ratio:.3g}')
    assert rel_l2(got_w[:, :rowlen], ref_w) < 2e-5 and ratio <= 1.0 and inexact == 0
    assert bool((b_new[:GUARD] == SENT).all()) and bool((b_new[GUARD + nbias:] == SENT).all())
    if nbias:
        got_b = b_new[GUARD:GUARD + nbias]
        ratio, inexact = elem_check(got_b, ref_b, A_b, nslab + 1)
        print(f'dbias: rel-L2 {rel_l2(got_b, ref_b):.3g}, err / bound {ratio:.3g}')
        assert rel_l2(got_b, ref_b) < 2e-5 and ratio <= 1.0 and inexact == 0


@pytest.mark.parametrize('nslab', NSLAB)
@pytest.mark.parametrize('name', list(LAYOUTS))
def test_fold_matches_reference_loop_and_float64(name, nslab, pkg, dev):
    _case(pkg, dev, LAYOUTS[name], nslab, seed=1000 + 7 * nslab + len(name))


def test_fold_longer_than_the_grid(pkg, dev):
    """n > 8192 blocks x 256 groups x 4: threads of the first blocks take a second group; n % 4 = 1 and bias partials behind."""
    _case(pkg, dev, (1, 8192 * 1024 + 1029, 8192 * 1024 + 1029, 12, 3, 0, 0), 2, seed=5)


def test_fold_rejects_bad_arguments(pkg, dev):
    L = pkg._lib
    st = torch.cuda.current_stream(dev).cuda_stream
    s = torch.zeros(64, device=dev); w = torch.full((16,), SENT, device=dev)
    for args in ((s.data_ptr(), 0, 16, 16, w.data_ptr(), 16, 16, -1, None, 0, st),      # no slab
                 (s.data_ptr(), 2, 8, 16, w.data_ptr(), 16, 16, -1, None, 0, st),       # stride < n
                 (s.data_ptr(), 2, 16, 16, w.data_ptr(), 8, 4, -1, None, 0, st),        # destination rows shorter than the compact ones
                 (s.data_ptr(), 2, 16, 16, w.data_ptr(), 12, 12, 12, None, 0, st)):     # bias partials without dbias
        assert L.lib().tdvc_debug_slab_fold(*args) != 0
    torch.cuda.synchronize()
    assert bool((w == SENT).all())
