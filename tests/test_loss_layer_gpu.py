"""The view-based loss layer of td-vc-gan_amd/losses.py -- lsgan_loss, lsgan_split, multiscale_feat_loss, multiscale_spec_loss,
cross_entropy_loss with MseViewsFn, L1ViewsFn, _fill_gaps, _group, MelSpec and _LogL1Fn underneath -- against the float64
references of tests/loss_ref.py on the same seeded fp32 values. The kernels themselves are covered through the C ABI
(test_misc_ops_gpu.py, test_conv_ops_gpu.py::test_l1_multi); here it is the host code that turns BatchViews into pointer offsets
and writes ONE full-size gradient per batched tensor: ranges at a non-zero offset, unaligned view pointers (odd per-sample sizes),
several views of one tensor, the gaps no view covers, more backward entries than one launch holds, gradients accumulated across
calls, and the per-site device state of loss_accumulate.

Bars: loss scalars rel <= 1e-5 (LOSS of test_misc_ops_gpu.py); gradients of the MSE and L1 terms |got - ref| <= 1e-6 * |ref|
(its EW bar; for the L1 terms the sign is exact and the magnitude is w / n * upstream), so rows outside every view are exactly 0.
Spectral gradient: rel-L2 <= 4 x the rel-L2 error of stock torch's fp32 CPU evaluation of the same chain against float64.

Allocator poison: the gradients are torch.empty_like buffers, and a missed gap passes whenever the caching allocator hands back
memory that happens to hold zeros. Before each backward the test makes sure the allocator caches room for every gradient, then
allocates every free block of its small pool whole, fills it with NaN and frees it again; a hook on every leaf records the
address of the gradient buffer the backward produced, and the test FAILS if that buffer does not lie inside the poisoned memory.

Measured on an MI355X, worst error / bar per group:
    lsgan_loss               loss 0.008   grad 0.160        lsgan_split            loss 0.008   (grads inside the bar)
    multiscale_feat_loss     loss 0.004   grad 0.075        waveform L1            loss 0.003
    accumulation across calls loss 0.003                    cross_entropy_loss     loss 0.011   grad 0.004
    lsgan_loss at 3e3 (1 / 3 / 16 blocks)  loss 0.008 / 0.004 / 0.010
    multiscale_spec_loss     loss 0.010;  gradient rel-L2 5.04e-06 (first resolution) and 2.58e-06 (all resolutions) against
        2.08e-06 and 1.16e-06 of stock torch's fp32 conv chain: error / bar 0.607 and 0.555. Against four times the error of stock
        fp32 with torch.stft in place of the STFT conv (1.15e-06, 7.24e-07) the ratios would be 1.098 and 0.892: a direct fp32 DFT sum
        of 512 terms is less accurate than an fp32 FFT.
Defects found: (1) loss_accumulate's fixed-point sum wrapped around when many blocks each stayed below its 2^20 limit but their sum
times 2^40 passed 2^63 (16 blocks at a mean of 9e6) -- it now also requires |partial| * blocks < 2^22; (2) overlapping or empty
ranges were silently wrong / NaN -- now refused. Skipping the trailing gap in L1ViewsFn.backward or in _fill_gaps makes
test_feat_loss_vs_float64 / test_lsgan_loss_vs_float64 fail (tried, with the poison in place)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from common import pkg, rel_l2

pytestmark = pytest.mark.gpu
EW, LOSS, TOL = 1e-6, 1e-5, 2e-5
UP = float(np.float32(0.6))            # upstream factor: the loss is multiplied by fp32 0.6 before backward
NAN = float('nan')


def _LS():
    return pkg().losses


def _leaf(t, dev):
    return t.to(dev).requires_grad_(True)


def _ref_leaf(t):
    return t.detach().double().cpu().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ allocator poison
class Poison:
    """NaN into the memory the next backward's torch.empty_like calls receive, and the proof that they received it."""

    def __init__(self, leaves, dev):
        self.leaves, self.seen = leaves, {}
        self.hooks = [x.register_hook(lambda g, i=i: self.seen.__setitem__(i, (g.data_ptr(), g.numel()))) for i, x in enumerate(leaves)]
        need = sum((x.numel() * 4 + 511) // 512 * 512 for x in leaves)
        room = [torch.empty(1 << 18, dtype=torch.float32, device=dev) for _ in range(need // (1 << 20) + 2)]      # cached room for every gradient
        del room
        held, before, cur = [], None, torch.cuda.current_stream(dev).cuda_stream
        for _ in range(16):
            free = []      # every free block of the caching allocator's small pool (requests up to 1 MiB: all the gradients here)
            for seg in torch.cuda.memory_snapshot():
                if seg['device'] == (dev.index or 0) and seg['segment_type'] == 'small' and seg.get('stream', cur) == cur:
                    free += [b['size'] for b in seg['blocks'] if b['state'] == 'inactive']
            free.sort()
            if not free or free == before:      # what a request on this stream cannot get (another stream's blocks) the backward cannot get either
                break
            before = free
            # a request for exactly a free block's size is served by a block of that size, whole (a block above 1 MiB in pieces, over
            # the rounds of this loop): all of them end up allocated and NaN
            held += [torch.full((min(size, 1 << 20) // 4,), NAN, dtype=torch.float32, device=dev) for size in sorted(free, reverse=True)]
        self.ranges = sorted((b.data_ptr(), b.data_ptr() + 4 * b.numel()) for b in held)
        assert sum(b - a for a, b in self.ranges) >= need
        del held

    def _inside(self, ptr, numel):
        lo, hi = ptr, ptr + 4 * numel
        for a, b in self.ranges:               # adjacent poisoned blocks count as one range
            if a <= lo < b:
                lo = b
        return lo >= hi

    def check(self):
        for h in self.hooks:
            h.remove()
        leaves, self.leaves = self.leaves, None
        for i, x in enumerate(leaves):
            assert i in self.seen, f'leaf {i} received no gradient'
            ptr, numel = self.seen[i]
            assert numel == x.numel()
            assert self._inside(ptr, numel), (f'the gradient buffer of leaf {i} ({numel} floats at {ptr:#x}) does not lie in the '
                                              f'{len(self.ranges)} NaN-poisoned blocks: the gap check would be vacuous')


def _scalar_ok(got, ref, what):
    got, ref = float(got), float(ref)
    print(f'[loss layer] {what}: loss rel err / bar {abs(got - ref) / (LOSS * abs(ref)):.3f}')
    assert abs(got - ref) <= LOSS * abs(ref), (what, got, ref)


def _grad_ok(got, ref, what):
    """|got - ref| <= EW |ref| element-wise: where the reference is exactly 0 (rows outside every view, a == b) so is the device."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, bound = (got - ref).abs(), EW * ref.abs()
    ok = err <= bound                                     # NaN compares false
    if not bool(ok.all()):
        i = int(torch.nonzero(~ok.reshape(-1))[0])
        raise AssertionError(f'{what}: {int((~ok).sum())} of {ref.numel()} elements off; first at flat {i}: got {got.reshape(-1)[i].item()!r} '
                             f'ref {ref.reshape(-1)[i].item()!r}')
    nz = ref != 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


# ------------------------------------------------------------------------------------------------ 1. lsgan_loss
LSGAN_T = (1, 7, 64, 257, 1023)        # 7 and 257: an odd per-sample size, so the view pointers are not 16-byte aligned


def _thirds(B):
    return {'first': (0, B), 'middle': (B, 2 * B), 'last': (2 * B, 3 * B), 'none': None}


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('which', ['first', 'middle', 'last', 'none'])
def test_lsgan_loss_vs_float64(B, which, dev):
    """Five outputs [3B, 1, T_i]; the T = 7 output goes in as BatchView(t, off=1, n=3B-1) so that rng composes with a non-zero offset
    (with rng = the last third that view would be one row short: there its tensor has 3B + 1 rows and the view n = 3B)."""
    LS = _LS()
    rng = _thirds(B)[which]
    gen = torch.Generator().manual_seed(100 * B + len(which))
    rows = [3 * B + (1 if (T == 7 and which == 'last') else 0) for T in LSGAN_T]
    xs = [torch.randn(r, 1, T, generator=gen) for r, T in zip(rows, LSGAN_T)]
    leaves = [_leaf(x, dev) for x in xs]
    outs = [LS.BatchView(x, off=1, n=x.shape[0] - 1) if T == 7 else x for x, T in zip(leaves, LSGAN_T)]
    loss = LS.lsgan_loss(outs, 1.0, rng=rng)
    p = Poison(leaves, dev)
    (loss * UP).backward()
    torch.cuda.synchronize()
    p.check()
    refs = [_ref_leaf(x) for x in xs]
    ranges = []
    for x, T in zip(xs, LSGAN_T):
        off, n = (1, x.shape[0] - 1) if T == 7 else (0, x.shape[0])
        lo, hi = (0, n) if rng is None else rng
        ranges.append((off + lo, off + hi))
    ref = R.lsgan(refs, ranges, 1.0)
    (ref * UP).backward()
    _scalar_ok(loss, ref, f'lsgan_loss B={B} rng={which}')
    worst = max(_grad_ok(x.grad, r.grad, f'lsgan_loss B={B} rng={which} T={T}') for x, r, T in zip(leaves, refs, LSGAN_T))
    print(f'[loss layer] lsgan_loss B={B} rng={which}: grad worst err/bar {worst:.3f}')


@pytest.mark.parametrize('T', [7, 64])
def test_lsgan_loss_two_disjoint_views_of_one_tensor(T, dev):
    """Rows [0, B) and [2B, 3B) of ONE tensor as two views in one call (plus a second tensor): one gradient, the middle rows 0."""
    LS = _LS()
    B = 2
    gen = torch.Generator().manual_seed(T)
    xs = [torch.randn(3 * B, 1, T, generator=gen), torch.randn(3 * B, 1, 33, generator=gen)]
    leaves = [_leaf(x, dev) for x in xs]
    outs = [LS.BatchView(leaves[0], 2 * B, B), leaves[1], LS.BatchView(leaves[0], 0, B)]
    loss = LS.lsgan_loss(outs, 0.0)
    p = Poison(leaves, dev)
    (loss * UP).backward()
    torch.cuda.synchronize()
    p.check()
    refs = [_ref_leaf(x) for x in xs]
    ref = R.lsgan([refs[0], refs[1], refs[0]], [(2 * B, 3 * B), None, (0, B)], 0.0)
    (ref * UP).backward()
    _scalar_ok(loss, ref, f'lsgan_loss two views T={T}')
    for x, r in zip(leaves, refs):
        _grad_ok(x.grad, r.grad, f'lsgan_loss two views T={T}')
    assert bool((leaves[0].grad[B:2 * B] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. lsgan_split
@pytest.mark.parametrize('rows,B', [(2, 1), (6, 3), (5, 2)])
def test_lsgan_split_vs_float64(rows, B, dev):
    """Both scalars and both halves of the gradient; then backward through l_real alone: the other output's grad is None and
    the fake half must be exactly 0, not NaN."""
    LS = _LS()
    gen = torch.Generator().manual_seed(10 * rows + B)
    xs = [torch.randn(rows, 1, T, generator=gen) for T in LSGAN_T]
    for only_real in (False, True):
        leaves = [_leaf(x, dev) for x in xs]
        l_real, l_fake = LS.lsgan_split(leaves, B)
        p = Poison(leaves, dev)
        (l_real * UP if only_real else l_real * UP + l_fake * 1.25).backward()
        torch.cuda.synchronize()
        p.check()
        refs = [_ref_leaf(x) for x in xs]
        r_real, r_fake = R.lsgan_split(refs, B)
        (r_real * UP if only_real else r_real * UP + r_fake * 1.25).backward()
        what = f'lsgan_split rows={rows} B={B} only_real={only_real}'
        _scalar_ok(l_real, r_real, what + ' real')
        _scalar_ok(l_fake, r_fake, what + ' fake')
        for x, r, T in zip(leaves, refs, LSGAN_T):
            _grad_ok(x.grad, r.grad, f'{what} T={T}')
            if only_real:
                assert bool((x.grad[B:] == 0).all()) and bool((x.grad[:B] != 0).any())


# ------------------------------------------------------------------------------------------------ 3. multiscale_feat_loss
FEAT_C = (1, 4, 16)
FEAT_T = (5, 9, 33, 64, 131, 596)      # + the pass index: ragged, 5 .. 600; C = 1 with an odd T gives unaligned view pointers
SAME_STORAGE = (2, 3)                  # (pass, map) whose reference rows are rows [0, B) of the sig tensor itself


def _feat_case(B, seed, dev):
    """The product's structure at toy size: 5 passes x 6 maps [3B, C, T]. sig = rows [B, 2B) of each map (through rng), ref = rows
    [2B, 3B) of a separate tensor as a BatchView (roff != off); every fifth element of a ref row equals the sig row."""
    gen = torch.Generator().manual_seed(seed)
    sig, ref = [], []
    for p_ in range(5):
        sig.append([]); ref.append([])
        for m_ in range(6):
            C_, T = FEAT_C[(p_ + m_) % 3], FEAT_T[m_] + p_
            a = torch.randn(3 * B, C_, T, generator=gen)
            b = torch.randn(3 * B, C_, T, generator=gen)
            b[2 * B:, :, ::5] = a[B:2 * B, :, ::5]
            if (p_, m_) == SAME_STORAGE:
                a[:B, :, ::5] = a[B:2 * B, :, ::5]
            sig[-1].append(a); ref[-1].append(b)
    return sig, ref


def _feat_run(B, sig, ref, dev):
    LS = _LS()
    leaves = [[_leaf(a, dev) for a in fl] for fl in sig]
    refs_d = [[b.to(dev) for b in fl] for fl in ref]
    views = [[LS.BatchView(leaves[p_][m_], 0, B) if (p_, m_) == SAME_STORAGE else LS.BatchView(refs_d[p_][m_], 2 * B, B) for m_ in range(6)]
             for p_ in range(5)]
    loss = LS.multiscale_feat_loss(leaves, views, rng=(B, 2 * B))
    flat = [x for fl in leaves for x in fl]
    p = Poison(flat, dev)
    (loss * UP).backward()
    torch.cuda.synchronize()
    p.check()
    return loss, flat


def _feat_ref(B, sig, ref):
    a64 = [[_ref_leaf(a) for a in fl] for fl in sig]
    pairs = []
    for p_ in range(5):
        for m_ in range(6):
            a = a64[p_][m_]
            pairs.append((a, B, 2 * B, a, 0, B) if (p_, m_) == SAME_STORAGE else (a, B, 2 * B, ref[p_][m_].double(), 2 * B, 3 * B))
    loss = R.feat_l1(pairs)
    (loss * UP).backward()
    return loss, [x for fl in a64 for x in fl]


@pytest.mark.parametrize('B', [2, 3])
def test_feat_loss_vs_float64(B, dev, monkeypatch):
    """5 x 6 maps with rng = (B, 2B) in the middle of the batch: per map a zero-fill entry, the term and another zero-fill entry,
    90 entries for a launch that holds 64 (L1M_MAX), so the backward has to split. The map with C = 16, T = 596 has a range
    above 16384 elements (two chunks). One pair reads sig and ref from the same storage: the gradient goes to the sig rows only."""
    L = pkg()._lib
    lib = L.lib()
    calls = []
    orig = lib.tdvc_l1_multi_bwd
    monkeypatch.setattr(lib, 'tdvc_l1_multi_bwd', lambda pairs, n, up, st: (calls.append(n), orig(pairs, n, up, st))[1])
    sig, ref = _feat_case(B, 40 + B, dev)
    assert max(B * a[0].numel() for fl in sig for a in fl) > 16384
    loss, flat = _feat_run(B, sig, ref, dev)
    assert calls == [90], calls
    r_loss, r_flat = _feat_ref(B, sig, ref)
    _scalar_ok(loss, r_loss, f'multiscale_feat_loss B={B}')
    worst = 0.0
    for k, (x, r) in enumerate(zip(flat, r_flat)):
        worst = max(worst, _grad_ok(x.grad, r.grad, f'multiscale_feat_loss B={B} pass {k // 6} map {k % 6}'))
        g = x.grad
        assert bool((g[:B] == 0).all()) and bool((g[2 * B:] == 0).all())        # the rows the term does not read, the same-storage ref rows too
        assert bool((g[B:2 * B, :, ::5] == 0).all()) and bool((g[B:2 * B, :, 1::5] != 0).all())     # a == b: exactly 0
    print(f'[loss layer] multiscale_feat_loss B={B}: grad worst err/bar {worst:.3f}')


def test_feat_loss_refuses_mismatches_and_runs_waveform_form(dev):
    """The shape-mismatch and batch-mismatch RuntimeErrors, and the single-map waveform form [[rec]], [[real]] at T = 8960."""
    LS = _LS()
    a = torch.randn(4, 3, 10, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        LS.multiscale_feat_loss([[a]], [[torch.randn(4, 3, 11, device=dev)]])
    with pytest.raises(RuntimeError, match='batch mismatch'):
        LS.multiscale_feat_loss([[a]], [[torch.randn(5, 3, 10, device=dev)]])
    with pytest.raises(RuntimeError, match='batch mismatch'):
        LS.multiscale_feat_loss([[a]], [[torch.randn(4, 3, 10, device=dev)]], rng=(1, 3))
    gen = torch.Generator().manual_seed(8960)
    rec, real = torch.randn(2, 1, 8960, generator=gen), torch.randn(2, 1, 8960, generator=gen)
    real[:, :, ::5] = rec[:, :, ::5]
    x = _leaf(rec, dev)
    loss = LS.multiscale_feat_loss([[x]], [[real.to(dev)]])
    p = Poison([x], dev)
    (loss * UP).backward()
    torch.cuda.synchronize()
    p.check()
    r = _ref_leaf(rec)
    r_loss = R.feat_l1([(r, 0, 2, real.double(), 0, 2)])
    (r_loss * UP).backward()
    _scalar_ok(loss, r_loss, 'waveform L1')
    _grad_ok(x.grad, r.grad, 'waveform L1')


# ------------------------------------------------------------------------------------------------ 4. accumulation across calls
def test_gradients_accumulate_across_loss_calls(dev):
    """Two feature-loss calls and two LSGAN calls read different row ranges of the same batched maps / outputs, as the train step
    does with adv_rng, idt_rng and rec_rng; one backward through their weighted sum. Each call writes a full-size gradient with
    zeros outside its range and autograd adds them: the sum equals the float64 one on every row. (The buffers autograd hands to
    the leaf are the sums, so their addresses are not checked here; the NaN blocks are still laid out before the backward.)"""
    LS = _LS()
    B = 2
    gen = torch.Generator().manual_seed(44)
    shapes = [(1, 7), (4, 33), (16, 64), (1, 257)]
    maps = [torch.randn(3 * B, C_, T, generator=gen) for C_, T in shapes]
    refs_a = [torch.randn(B, C_, T, generator=gen) for C_, T in shapes]
    refs_b = [torch.randn(2 * B, C_, T, generator=gen) for C_, T in shapes]
    outs = [torch.randn(3 * B, 1, T, generator=gen) for T in (7, 64, 257)]
    lm, lo = [_leaf(t, dev) for t in maps], [_leaf(t, dev) for t in outs]
    w = [float(np.float32(v)) for v in (0.7, 1.1, 0.9, 1.3)]
    l1 = LS.multiscale_feat_loss([lm], [[t.to(dev) for t in refs_a]], rng=(B, 2 * B))
    l2 = LS.multiscale_feat_loss([lm], [[LS.BatchView(t.to(dev), B, B) for t in refs_b]], rng=(2 * B, 3 * B))
    l3 = LS.lsgan_loss(lo, 1.0, rng=(0, B))
    l4 = LS.lsgan_loss(lo, 0.0, rng=(B, 3 * B))
    p = Poison(lm + lo, dev)
    (w[0] * l1 + w[1] * l2 + w[2] * l3 + w[3] * l4).backward()
    torch.cuda.synchronize()
    for h in p.hooks:
        h.remove()
    rm, ro = [_ref_leaf(t) for t in maps], [_ref_leaf(t) for t in outs]
    r1 = R.feat_l1([(a, B, 2 * B, b.double(), 0, B) for a, b in zip(rm, refs_a)])
    r2 = R.feat_l1([(a, 2 * B, 3 * B, b.double(), B, 2 * B) for a, b in zip(rm, refs_b)])
    r3 = R.lsgan(ro, [(0, B)] * 3, 1.0)
    r4 = R.lsgan(ro, [(B, 3 * B)] * 3, 0.0)
    (w[0] * r1 + w[1] * r2 + w[2] * r3 + w[3] * r4).backward()
    for got, ref, nm in ((l1, r1, 'feat 1'), (l2, r2, 'feat 2'), (l3, r3, 'lsgan 1'), (l4, r4, 'lsgan 2')):
        _scalar_ok(got, ref, 'accumulate ' + nm)
    for x, r in zip(lm + lo, rm + ro):
        _grad_ok(x.grad, r.grad, 'accumulated gradient')
    for x in lm:
        assert bool((x.grad[:B] == 0).all())              # no call reads the first third of the maps


# ------------------------------------------------------------------------------------------------ 5. multiscale_spec_loss
def _spec_refs(ffts):
    sig, ref = R.spec_inputs()
    s64 = _ref_leaf(sig)
    l64, t64 = R.log_mel_l1(s64, ref.double(), ffts, separated=True)
    l64.backward()
    s32 = sig.clone().requires_grad_(True)
    R.log_mel_l1_conv(s32, ref, ffts).backward()
    f32 = sig.clone().requires_grad_(True)
    R.log_mel_l1(f32, ref, ffts).backward()
    return sig, ref, l64, t64, s64.grad, rel_l2(s32.grad, s64.grad), rel_l2(f32.grad, s64.grad)


@pytest.mark.parametrize('all_res', [False, True], ids=['first_resolution', 'all_resolutions'])
def test_spec_loss_full_chain_vs_float64(all_res, dev):
    """Reflect pad, STFT conv, power, mel projection, log-L1, forward and backward, B = 2, T = 2304, fft_sizes [512, 1024, 2048]
    (only the first contributes unless all_resolutions), with return_separated. The float64 reference is torch.stft-based
    (loss_ref.log_mel_l1); the bar's fp32 evaluation is stock torch running the same chain of operations, the STFT as a strided
    conv1d with the fp32 DFT basis included (loss_ref.log_mel_l1_conv). An fp32 FFT is a different, more accurate algorithm than a
    direct fp32 DFT sum: its error is printed beside the bar, not asserted."""
    LS = _LS()
    ffts = list(R.SPEC_FFTS) if all_res else list(R.SPEC_FFTS)[:1]
    sig, ref, l64, t64, g64, err32, err32_fft = _spec_refs(ffts)
    x = _leaf(sig, dev)
    total, parts = LS.multiscale_spec_loss(x, ref.to(dev), list(R.SPEC_FFTS), return_separated=True, all_resolutions=all_res)
    assert len(parts) == len(ffts)
    plain = LS.multiscale_spec_loss(x, ref.to(dev), list(R.SPEC_FFTS), all_resolutions=all_res)
    assert torch.equal(plain, total)
    total.backward()
    torch.cuda.synchronize()
    _scalar_ok(total, l64, f'multiscale_spec_loss all_resolutions={all_res}')
    for n, got, want in zip(ffts, parts, t64):
        _scalar_ok(got, want, f'multiscale_spec_loss term n_fft={n}')
    err, bar = rel_l2(x.grad, g64), 4.0 * err32
    print(f'[loss layer] multiscale_spec_loss all_resolutions={all_res}: grad rel-L2 {err:.3e}, stock fp32 CPU {err32:.3e}, err / bar {err / bar:.3f}'
          f'  (stock fp32 CPU with torch.stft in place of the STFT conv {err32_fft:.3e}: err / 4x {err / (4.0 * err32_fft):.3f})')
    assert bool(torch.isfinite(x.grad).all())
    assert err <= bar, (err, bar)


def test_spec_loss_bins_below_the_floor_have_zero_gradient(dev):
    """Row 1's 512 exact zeros: the 80 mel bins of n_fft = 512's frame 9 are exactly 0 on the device as well, on both sides, and the
    log-L1 gradient there is exactly 0 (below the floor the clamp passes nothing)."""
    LS = _LS()
    sig, ref = R.spec_inputs()
    t = LS.get_melspec_transform(16000, 512, 80)
    with torch.no_grad():
        mref = t(ref.to(dev))
    mel = t(_leaf(sig, dev))
    mel.retain_grad()
    LS._LogL1Fn.apply(mel, mref, 1e-5).backward()
    torch.cuda.synchronize()
    assert bool((mel[1, :, 9] == 0).all()) and bool((mref[1, :, 9] == 0).all())
    assert bool((mel.grad[1, :, 9] == 0).all())
    assert int((mel.grad == 0).sum()) == 80 and bool(torch.isfinite(mel.grad).all())
    m64 = R.mel_power(sig.double(), 512)
    assert rel_l2(mel, m64) < TOL, rel_l2(mel, m64)


# ------------------------------------------------------------------------------------------------ 6. loss_accumulate state
def _ordinary_lsgan(dev):
    """A multi-block call (n = 3000: 12 blocks) with an ordinary value, twice: right, and the same bits."""
    LS = _LS()
    x = torch.randn(3, 1, 1000, generator=torch.Generator().manual_seed(9))
    xd = x.to(dev)
    got = [LS.lsgan_loss([xd], 1.0) for _ in range(2)]
    torch.cuda.synchronize()
    _scalar_ok(got[0], R.lsgan([x.double()], [None], 1.0), 'ordinary call after a fallback call')
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize('rows,T', [(1, 256), (3, 256), (4, 1024)], ids=['one_block', 'three_blocks', 'sixteen_blocks_below_2p20_each'])
def test_loss_accumulate_large_values_leave_clean_state(rows, T, dev):
    """Inputs near 3e3: a mean of 9e6. With 1 or 3 blocks every block's partial is >= 2^20 and goes through the float fallback; with
    16 blocks each partial (5.6e5) is below 2^20 but their sum times 2^40 does not fit 64 bits -- the fixed-point path must not be
    taken there either (it wrapped around before this case existed). Afterwards the per-site state is clean."""
    LS = _LS()
    x = 3000.0 + torch.randn(rows, 1, T, generator=torch.Generator().manual_seed(rows))
    got = LS.lsgan_loss([x.to(dev)], 0.0)
    torch.cuda.synchronize()
    _scalar_ok(got, R.lsgan([x.double()], [None], 0.0), f'lsgan_loss at 3e3, {rows * T // 256} blocks')
    _ordinary_lsgan(dev)


def test_loss_accumulate_nan_leaves_clean_state(dev):
    LS = _LS()
    x = torch.randn(3, 1, 1000, generator=torch.Generator().manual_seed(5))
    x[1, 0, 500] = NAN
    got = LS.lsgan_loss([x.to(dev)], 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got).all())
    _ordinary_lsgan(dev)


@pytest.mark.parametrize('B', [1, 3])
def test_cross_entropy_loss_autograd(B, dev):
    """cross_entropy_loss through autograd at K = 16: value, and the gradient with an upstream factor."""
    LS = _LS()
    gen = torch.Generator().manual_seed(16 + B)
    z = torch.randn(B, 16, generator=gen) * 3
    labels = torch.tensor([15, 0, 7][:B], dtype=torch.int64)
    zd = _leaf(z, dev)
    loss = LS.cross_entropy_loss(zd, labels.to(dev))
    p = Poison([zd], dev)
    (loss * UP).backward()
    torch.cuda.synchronize()
    p.check()
    zr = _ref_leaf(z)
    ref = F.cross_entropy(zr, labels)
    (ref * UP).backward()
    _scalar_ok(loss, ref, f'cross_entropy_loss B={B}')
    err = rel_l2(zd.grad, zr.grad)
    print(f'[loss layer] cross_entropy_loss B={B}: grad rel-L2 / bar {err / TOL:.3f}')
    assert err < TOL, err


# ------------------------------------------------------------------------------------------------ 7. overlap and empty ranges
def test_overlapping_and_empty_ranges_are_refused_before_any_launch(dev, monkeypatch):
    """Two views of one tensor whose rows overlap would keep the gradient of whichever entry was launched last (the kernels write,
    they do not add); an empty range divides by 0. Both raise ValueError naming the function, and nothing is launched."""
    LS = _LS()
    lib = pkg()._lib.lib()
    launched = []
    for name in ('tdvc_mse_const_fwd', 'tdvc_l1_multi_fwd'):
        orig = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _o=orig, _n=name: (launched.append(_n), _o(*a))[1])
    BV = LS.BatchView
    t = torch.randn(6, 1, 7, device=dev, requires_grad=True)
    u = torch.randn(6, 1, 7, device=dev)
    with pytest.raises(ValueError, match='lsgan_loss.*overlap'):
        LS.lsgan_loss([BV(t, 0, 3), BV(t, 2, 2)], 1.0)
    with pytest.raises(ValueError, match='lsgan_loss.*empty'):
        LS.lsgan_loss([t], 1.0, rng=(2, 2))
    with pytest.raises(ValueError, match='lsgan_loss.*empty'):
        LS.lsgan_loss([torch.zeros(3, 1, 0, device=dev)], 1.0)
    with pytest.raises(ValueError, match='lsgan_split.*overlap'):
        LS.lsgan_split([BV(t, 0, 4), BV(t, 3, 3)], 2)
    for B in (0, 6):
        with pytest.raises(ValueError, match='lsgan_split.*empty'):
            LS.lsgan_split([t], B)
    with pytest.raises(ValueError, match='multiscale_feat_loss.*overlap'):
        LS.multiscale_feat_loss([[BV(t, 0, 3), BV(t, 2, 3)]], [[BV(u, 0, 3), BV(u, 3, 3)]])
    with pytest.raises(ValueError, match='multiscale_feat_loss.*empty'):
        LS.multiscale_feat_loss([[t]], [[BV(u, 0, 0)]], rng=(3, 3))
    assert launched == []
    LS.lsgan_loss([BV(t, 0, 3), BV(t, 3, 3)], 1.0)        # ranges that touch do not overlap
    LS.multiscale_feat_loss([[BV(t, 0, 3), BV(t, 3, 3)]], [[BV(u, 3, 3), BV(u, 3, 3)]])      # overlapping REFERENCE rows carry no gradient
    torch.cuda.synchronize()
    assert launched == ['tdvc_mse_const_fwd'] * 2 + ['tdvc_l1_multi_fwd']
