"""GPU parity of the conv C-ABI (tdvc_conv_fwd / dgrad / wgrad) against torch CPU float64 autograd,
for every conv shape class on the path, on both the MFMA and the scalar kernels."""
import pytest
import torch

from common import rel_l2, traced
from conv_ops_cases import CASES, TOL, conv_case_errors, film_block_errors, film_cond_errors
from edge_support import mods, poison_lds, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('generic', [0, 1], ids=['mfma', 'scalar'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_conv_fwd_bwd(case, generic, dev):
    errs = conv_case_errors(case, dev, generic)
    assert max(errs.values()) < TOL, errs


POISON_CASES = ['grp_64_64_k41_s4_g16', 'grp_16_64_k41_s4', 'dil_c16_k11_d5', 'dil_c64_k3_d5', 'cond2_136_32', 'd5_256_256_k5_lrelu',
                'down_64_128_s8', 'up_128_64_s8', 'fir_dw8_k33_s2', 'k7_256_128_T50']


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in POISON_CASES], ids=[c[0] for c in CASES if c[0] in POISON_CASES])
def test_conv_with_poisoned_lds(case, dev):
    """Every kernel family with the LDS of all CUs pre-filled with NaN bit patterns (tdvc_debug_poison_lds): a kernel that
    reads LDS words it never staged -- masked by a zero WEIGHT only -- turns them into NaN (0 * NaN) instead of passing on
    whatever finite values the previous kernel happened to leave (small_group_fwd_kernel, taps past K)."""
    poison_lds(dev)
    errs = conv_case_errors(case, dev, 0)
    assert all(e == e for e in errs.values()) and max(errs.values()) < TOL, errs


@pytest.mark.parametrize('cfg', [(16, 3, 1, 900, True, True), (32, 7, 3, 400, True, False), (64, 11, 5, 260, False, True),
                                 (128, 3, 1, 100, True, True), (256, 11, 5, 50, False, False)],
                         ids=['c16k3', 'c32k7d3', 'c64k11d5_enc', 'c128k3', 'c256k11d5_enc'])
def test_film_block(cfg, dev):
    """Fused FiLM residual block (model/generator.py:96-111) incl. MRF running-mean epilogue."""
    errs = film_block_errors(cfg, dev)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize('cfg', [(16, 2048, 2), (64, 600, 3), (128, 260, 2), (32, 64, 2), (32, 260, 120), (32, 96, 1100)],
                         ids=['C16_T2048', 'C64_T600', 'C128_T260', 'C32_T64', 'C32_T260_B120_split', 'C32_T96_B1100_3samples'])
@pytest.mark.parametrize('fused_bwd', [True, False], ids=['bwd1launch', 'bwd2launch'])
@pytest.mark.parametrize('fused_fwd', [False, True], ids=['fwd2launch', 'fwd1launch'])
def test_film_conditioning_fused(cfg, fused_fwd, fused_bwd, dev):
    """tdvc_film_cond_fwd / tdvc_film_cond_bwd / tdvc_film_cond0_bwd (FiLM conditioning path of model/generator.py:86-92,103 in
    the split formulation) against float64 autograd of the dense reference formulation
        gb = cond_var.2(LeakyReLU(cond_var.0(cat([emb.repeat(T), exc])))).
    Ragged cases on purpose: T = 600 / 260 / 64 are not multiples of the fused backward's 60-step chunk or of 32 (fp32 mask
    source), T = 2048 runs the sign-bit mask with a partial last chunk. The last two have more than 512 (sample, chunk) pairs
    in both backward plans (64-step and 60-step chunks), so a block walks several chunks and dk3 is folded from per-(block,
    sample) slots: at T = 260, B = 120 (5 chunks per sample, 2 per block) a sample's chunks are split across two blocks; at
    T = 96, B = 1100 (2 chunks per sample, 5 per block) one block covers three samples."""
    ops = mods()[0]
    old = ops.FUSED_COND_FWD, ops.FUSED_COND_BWD
    ops.FUSED_COND_FWD, ops.FUSED_COND_BWD = fused_fwd, fused_bwd
    try:
        with traced() as tr:
            errs = film_cond_errors(cfg, dev)
    finally:
        ops.FUSED_COND_FWD, ops.FUSED_COND_BWD = old
    assert max(errs.values()) < TOL, errs
    assert any(n.startswith('film_cond_bwd_kernel') for n in tr.names) == fused_bwd, sorted(tr.names)


def test_fanout_sum(dev):
    """ops.fanout: n aliases forward, ONE n-ary sum backward (tdvc_sum_n), incl. the > 16-source chaining and a consumer that
    sends no gradient."""
    ops, L, _ = mods()
    for n, shape in ((3, (2, 16, 520)), (9, (3, 8, 333)), (36, (4, 128))):
        x = torch.randn(*shape, device=dev, requires_grad=True)
        ws = [torch.randn(*shape, device=dev) for _ in range(n)]
        outs = ops.fanout(x, n)
        assert all(o.data_ptr() == x.data_ptr() for o in outs)
        sum((o * w).sum() for o, w in list(zip(outs, ws))[1:]).backward()      # consumer 0 unused: its gradient is None
        ref = torch.stack([w.double() for w in ws[1:]]).sum(0)
        assert rel_l2(x.grad, ref) < 1e-6
    with torch.no_grad():
        y = torch.randn(2, 3, device=dev)
        assert all(o is y for o in ops.fanout(y, 4))


def test_l1_multi(dev):
    """tdvc_l1_multi_fwd / _bwd (all feature-matching terms in one launch) against torch: ragged sizes incl. an unaligned
    pair, a pair longer than one chunk, zero-fill entries, more pairs than one launch holds."""
    import ctypes as C
    _, L, _ = mods()
    lib = L.lib()
    st = stream(dev)
    rs = torch.Generator().manual_seed(5)
    sizes = [40000, 7, 16384, 16385, 1023] + [300 + 3 * i for i in range(70)]
    big = torch.randn(sum(sizes) + 8, generator=rs).to(dev)
    a, b, off = [], [], 1                                  # offset 1 float: the first pairs are NOT 16-byte aligned
    for n in sizes:
        a.append(big[off:off + n]); off += n
    b = [torch.randn(n, generator=rs).to(dev) for n in sizes]
    da = [torch.full((n,), 7.0, device=dev) for n in sizes]
    zero = torch.full((5000,), 3.0, device=dev)
    w = [0.5 + 0.01 * i for i in range(len(sizes))]
    ents = [L.L1Pair(x.data_ptr(), y.data_ptr(), d.data_ptr(), x.numel(), wi) for x, y, d, wi in zip(a, b, da, w)]
    ents.insert(3, L.L1Pair(None, None, zero.data_ptr(), zero.numel(), 0.0))
    pairs = (L.L1Pair * len(ents))(*ents)
    out = torch.zeros(1, device=dev)
    up = torch.tensor([1.7], device=dev)
    L.check(lib.tdvc_l1_multi_fwd(pairs, len(ents), out.data_ptr(), st))
    L.check(lib.tdvc_l1_multi_bwd(pairs, len(ents), up.data_ptr(), st))
    torch.cuda.synchronize()
    ref = sum(wi * (x.double() - y.double()).abs().mean() for x, y, wi in zip(a, b, w))
    assert abs(float(out) - float(ref)) < 1e-5 * float(ref)
    for x, y, d, wi in zip(a, b, da, w):
        assert torch.allclose(d, torch.sign(x - y) * (wi * 1.7 / x.numel()), rtol=1e-6, atol=0)
    assert float(zero.abs().max()) == 0.0


def test_film_k3_multi_matches_single(dev):
    """ops.film_k3_multi (all FiLM blocks of a stage in one launch each way) against the per-block FilmK3Fn: outputs, weight /
    bias gradients per block, and the embedding gradient summed over the blocks."""
    ops, L, arena = mods()
    torch.manual_seed(3)
    B, n_const, nc, nblk = 5, 128, 136, 9
    ws = [(torch.randn(nc, nc, 3, device=dev) / (nc * 3) ** 0.5) for _ in range(nblk)]
    bs = [torch.randn(nc, device=dev) * 0.1 for _ in range(nblk)]
    cots = [torch.randn(B, nc, 3, device=dev) for _ in range(nblk)]
    emb = torch.randn(B, n_const, device=dev)

    def run(multi):
        dws, dbs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs]
        specs = []
        for w, b, dw, db in zip(ws, bs, dws, dbs):
            sp = ops.ConvSpec(n_const, nc, 3, 1, 1, 1, 1, False, w_cin=nc, w_cin_off=0)
            sp.slot = arena.ConvSlot(w.data_ptr(), b.data_ptr(), dw.data_ptr(), db.data_ptr(), True, None, 0)
            specs.append(sp)
        e = emb.clone().requires_grad_(True)
        k3s = ops.film_k3_multi(e, specs) if multi else [ops.film_k3(e, sp) for sp in specs]
        sum((k * c).sum() for k, c in zip(k3s, cots)).backward()
        torch.cuda.synchronize()
        return [k.detach() for k in k3s], e.grad, dws, dbs
    k_m, de_m, dw_m, db_m = run(True)
    k_s, de_s, dw_s, db_s = run(False)
    for a, b_ in zip(k_m, k_s):
        assert torch.equal(a, b_)
    assert rel_l2(de_m, de_s) < 1e-6
    for a, b_ in zip(dw_m + db_m, dw_s + db_s):
        assert torch.equal(a, b_)
    # and the forward against plain torch: cond_var.0 on the constant embedding channels as a length-3 signal
    x3 = emb[:, :, None].expand(B, n_const, 3).double().cpu()
    ref = torch.nn.functional.conv1d(x3, ws[0][:, :n_const].double().cpu(), bs[0].double().cpu(), padding=1)
    assert rel_l2(k_m[0], ref) < 1e-6


@pytest.mark.parametrize('cfg', [(3, 1, 1040, True, True), (7, 3, 16000, True, False), (11, 5, 2052, False, True), (3, 5, 516, True, False)],
                         ids=['k3d1_T1040', 'k7d3_T16000', 'k11d5_T2052_nofilm', 'k3d5_T516'])
def test_fused_film_block_forward_is_bit_identical(cfg, dev):
    """tdvc_film_block_fwd (dilated conv + FiLM + 1x1 conv + residual in one launch, 16 channels) against the two-launch path:
    h and out must be bit-identical (same arithmetic in the same order), over ragged time tiles, with / without FiLM and MRF sum."""
    ops, L, arena = mods()
    k, d, T, film, with_acc = cfg
    torch.manual_seed(k * 100 + d)
    B, Cc = 3, 16
    w1 = (torch.randn(Cc, Cc, k) / (Cc * k) ** 0.5).to(dev); b1 = (torch.randn(Cc) * 0.1).to(dev)
    w2 = (torch.randn(Cc, Cc, 1) / Cc ** 0.5).to(dev); b2 = (torch.randn(Cc) * 0.1).to(dev)
    cs = ops.ConvSpec(Cc, Cc, k, 1, (k - 1) * d // 2, d, 1, True)
    cs.slot = arena.ConvSlot(w1.data_ptr(), b1.data_ptr(), 0, 0, False, None, 0)
    ps = ops.ConvSpec(Cc, Cc, 1)
    ps.slot = arena.ConvSlot(w2.data_ptr(), b2.data_ptr(), 0, 0, False, None, 0)
    x0 = torch.randn(B, Cc, T, device=dev)
    gb0 = torch.randn(B, 2 * Cc, T, device=dev) * 0.5 if film else None
    acc = torch.randn(B, Cc, T, device=dev) if with_acc else None
    cot = torch.randn(B, Cc, T, device=dev)
    outs = {}
    for fused in (True, False):
        old = ops.FUSED_FILM_BLOCK
        ops.FUSED_FILM_BLOCK = fused
        x = x0.clone().requires_grad_(True)
        gb = gb0.clone().requires_grad_(True) if film else None
        try:
            with traced() as tr:
                y = ops.FilmBlockFn.apply(x, gb, acc, None, cs, ps, 1.0 / 3)
                y.backward(cot)      # reads the stored h: a wrong h shows up in both gradients
        finally:
            ops.FUSED_FILM_BLOCK = old
        assert any(n.startswith('film_block_fwd_kernel') for n in tr.names) == fused, sorted(tr.names)
        outs[fused] = (y.detach().clone(), x.grad.clone(), gb.grad.clone() if film else None)
    for a_, b_ in zip(outs[True], outs[False]):
        if a_ is not None:
            assert torch.equal(a_, b_), float((a_ - b_).abs().max())
