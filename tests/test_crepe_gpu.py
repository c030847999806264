"""GPU: the CREPE pitch tracker on the device (td-vc-gan_amd/crepe.py, csrc/pitch_crepe.hip) against the float64 restatement
tests/crepe_ref.py, which tests/test_crepe_cpu.py pins. torchcrepe is not available: nothing here is a parity test against it.

1. crepe_frames element by element: |got - ref| <= 4 * 2^-24 * max|reference frames of the row| (one rounding x 4, the project's bar
   for float64-inside kernels); rows of 63, 64, 1023, 1024, 1025 and 2047 samples, a constant row (every frame inside the row exactly 0,
   the frames that straddle the zero padding not) and an all-zero row (exactly 0) in one padded buffer that is a strided view with NaN
   spares and NaN past each length; hop 64 and 160; the frame counts; a row alone has the bits of the row in the batch.
2. tdvc_crepe_conv alone through the C ABI against float64: each of `tiny`'s six layers, 128 -> 128 at 64 positions (`full`'s layer 3)
   and 1 -> 1024 for layer 1; N = 1, 2, 15, 16, 17, 33 frames (a workgroup takes 256 / Lc frames: 1, 2, 4, 8, 16 and 32 for Lc = 256
   .. 8, so these N leave the last workgroup of every geometry partly empty, fill it exactly and start another one); the output
   buffer prefilled with NaN, LDS poisoned first; negative BatchNorm scales, and in float64 at least one pooled pair changes its winner
   if the pool runs before the affine (asserted). Bar per case: 4 x the max-abs error of stock torch's fp32 CPU evaluation against
   float64.
3. tdvc_crepe_head: 256 and 2048 features, N = 1 and 17, the bar built the same way; the channel-major flatten of the same input
   differs from the reference by more than 100 x the bar (asserted), so an implementation with the wrong order cannot pass.
4. crepe_decode on synthetic activations: bumps whose centre moves; centres at both range edges (the +-4 window cut by 0, by 360 and
   by the mask); centres below minidx and at or above maxidx (the masked maximum wins); exact ties (lowest index); peaks on both
   sides of 0.21 by 1e-3. argmax bins and voicing equal the restatement's on every frame, Hz within 4 * 2^-24 relative,
   weighted_argmax within 64 * 2^-24 relative. viterbi: on a lattice of small dyadic rationals the path equals the restatement's on
   every frame; on real-valued bumps with an octave-jump distractor a frame may be left out only where the float64 margin between the
   best and the second-best path is below F * 2^-21 * M (Viterbi decoder; M bounds the renormalised scores: max|lattice| +
   log 144), at most 2 % of the frames; the seeds were chosen on the CPU so that the restatement leaves out none (asserted).
5. End to end: Crepe('tiny').activations on rows of 64, 1024, 2047 and 8000 samples in one buffer with lengths, bar 4 x the fp32 CPU
   chain's error against the float64 chain; the reference activations differ between neighbouring frames by more than 100 x the bar
   (asserted: a kernel that mixes up frames fails); each row alone bit-identical to the row in the batch; two runs bit-identical; graph
   replay equals eager; filtered_pitch with each decoder (shapes as the reference's, pitch equal to crepe_decode of its own activations
   bit for bit); Crepe('full') on one row of 1024 samples; convert_audio(f0_tracker=crepe) equals convert on the track computed by
   hand, and convert_audio() without the tracker is bit-identical to the parent commit's path (track_f0 called explicitly).
6. Refusals, each before any launch.
Every test prints error / bar (run with -s).
Measured on an MI355X (error / bar, worst per launch): crepe_frames 0.12-0.21 (the constant row 0.02-0.14, the all-zero row 0);
tdvc_crepe_conv 0.13 (1 -> 128), 0.14 (128 -> 16), 0.05-0.10 (layers 3-6), 0.12 (128 -> 128), 0.08 (1 -> 1024) over all six N;
tdvc_crepe_head 0.02-0.06, the channel-major flatten 6e5-1.6e6 bars away; crepe_decode argmax 0.19 and weighted_argmax 0.013 on both
ranges, bins and voicing equal on all 47 frames; viterbi: no frame off the float64 path on either lattice (smallest margins 1.0e-1
and 8.0e-4 against bounds of 2.0e-4 and 3.0e-4, none left out; the per-frame argmax jumps to the distractor on 9 of 60 frames);
Crepe('tiny').activations 0.12-0.13 (max|a - a64| 3.5e-8, bar 2.7e-7), Crepe('full') 0.12.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import crepe_ref as R
from common import build_models, pkg
from edge_support import EINVAL, EUNSUPPORTED, poison_lds

pytestmark = pytest.mark.gpu
NAN = float('nan')
U24 = 2.0 ** -24


def K():
    return pkg().crepe


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ----------------------------------------------------------------------------------------------------------------- 1. frames
FRAME_ROWS = (63, 64, 1023, 1024, 1025, 2047, 2047, 1500)      # the last two: the constant row and the all-zero row


@functools.lru_cache(maxsize=None)
def frames_case():
    T = 2047
    x = np.full((len(FRAME_ROWS), T), np.nan, dtype=np.float32)
    for b, n in enumerate(FRAME_ROWS[:6]):
        x[b, :n] = R.tones(n, seed=b)
    x[6, :FRAME_ROWS[6]] = 0.3
    x[7, :FRAME_ROWS[7]] = 0.0
    refs = {hop: [R.frames(x[b, :n], hop).numpy() for b, n in enumerate(FRAME_ROWS)] for hop in (64, 160)}
    x.setflags(write=False)
    return x, refs


@pytest.mark.parametrize('hop', [64, 160])
def test_frames_against_float64(dev, hop):
    x, refs = frames_case()
    B, T = x.shape
    whole = torch.full((2 * B, T + 5), NAN, device=dev)
    whole[::2, :T] = torch.from_numpy(np.array(x)).to(dev)
    view = whole[::2, :T]
    assert view.stride() == (2 * (T + 5), 1)
    lengths = torch.tensor(FRAME_ROWS, dtype=torch.int32, device=dev)
    poison_lds(dev)
    got_t = K().crepe_frames(view[:, None], hop=hop, lengths=lengths)
    Fm = 1 + T // hop
    assert got_t.shape == (B, Fm, 1024) and got_t.dtype == torch.float32 and bool(torch.isfinite(got_t).all())
    got = got_t.double().cpu().numpy()
    for b, n in enumerate(FRAME_ROWS):
        ref = refs[hop][b]
        nf = 1 + n // hop
        assert ref.shape == (nf, 1024)
        assert (got[b, nf:] == 0).all(), f'row {b}: frames past the row\'s own count'
        bar = 4 * U24 * float(np.abs(ref).max())
        err = float(np.abs(got[b, :nf] - ref).max())
        print(f'crepe_frames hop {hop} n={n} row {b}: {nf} frames, max|got - ref| {err:.3e}, error / bar {err / bar if bar else 0.0:.3f}')
        assert err <= bar, (b, n, err, bar)
    n = FRAME_ROWS[6]                                                           # the constant row
    inside = [f for f in range(1 + n // hop) if f * hop - 512 >= 0 and f * hop + 512 <= n]
    straddle = [f for f in range(1 + n // hop) if f not in inside]
    assert inside and straddle and (got[6, inside] == 0).all() and all((got[6, f] != 0).any() for f in straddle)
    assert (got[7] == 0).all()                                                  # the all-zero row
    alone = K().crepe_frames(torch.from_numpy(np.array(x[4, :FRAME_ROWS[4]])).to(dev), hop=hop)      # no lengths, one row [T]
    assert alone.shape == (1, 1 + FRAME_ROWS[4] // hop, 1024) and torch.equal(alone[0], got_t[4, :alone.shape[1]])
    assert torch.equal(K().crepe_frames(view, hop=hop, lengths=lengths), got_t)


# ------------------------------------------------------------------------------------------------------------------- 2. conv
CONV_N = (1, 2, 15, 16, 17, 33)
#            layer (its geometry), Cin, Cout, Lin
CONV_CASES = {'tiny1': (1, 1, 128, 1024), 'tiny2': (2, 128, 16, 128), 'tiny3': (3, 16, 16, 64), 'tiny4': (4, 16, 16, 32), 'tiny5': (5, 16, 32, 16),
              'tiny6': (6, 32, 64, 8), 'full3': (3, 128, 128, 64), 'full1': (1, 1, 1024, 1024)}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """Seeded weights in crepe_ref's recipe under the keys of `layer`, the input, y64 / y32 for max(CONV_N) frames (frames are
    independent: the first N frames are the reference of a call with N), the bar, the folded scale / shift."""
    layer, Cin, Cout, Lin = CONV_CASES[name]
    g = torch.Generator().manual_seed(sorted(CONV_CASES).index(name) + 40)
    k = R.KERNELS[layer - 1]
    p = f'conv{layer}'
    gamma = 0.5 + torch.rand(Cout, generator=g)
    gamma[1::3] = -gamma[1::3]
    sd = {p + '.weight': (2 * torch.rand(Cout, Cin, k, 1, generator=g) - 1) * math.sqrt(3.0 / (Cin * k)),
          p + '.bias': (2 * torch.rand(Cout, generator=g) - 1) / math.sqrt(Cin * k),
          p + '_BN.weight': gamma, p + '_BN.bias': 0.1 * torch.randn(Cout, generator=g),
          p + '_BN.running_mean': 0.2 * torch.rand(Cout, generator=g), p + '_BN.running_var': 0.5 + torch.rand(Cout, generator=g)}
    x = torch.randn(max(CONV_N), Cin, Lin, generator=g)
    y64 = R.layer(sd, layer, x[..., None], torch.float64)[..., 0]
    y32 = R.layer(sd, layer, x[..., None], torch.float32)[..., 0]
    wrong = R.layer(sd, layer, x[..., None], torch.float64, pool_first=True)[..., 0]
    flipped = int((wrong != y64).sum())
    bar = 4 * float((y32.double() - y64).abs().max())
    scale = sd[p + '_BN.weight'].double() / torch.sqrt(sd[p + '_BN.running_var'].double() + R.BN_EPS)
    shift = sd[p + '_BN.bias'].double() - sd[p + '_BN.running_mean'].double() * scale
    return dict(sd=sd, x=x, y64=y64, bar=bar, flipped=flipped, scale=scale.float(), shift=shift.float(), layer=layer)


def conv_call(dev, x, w, bias, scale, shift, y, N, Cin, Cout, Lin, Kk, stride):
    L = pkg()._lib
    a = L.CrepeConvArgs()
    a.N, a.Cin, a.Cout, a.Lin, a.K, a.stride = N, Cin, Cout, Lin, Kk, stride
    ptr = lambda t: None if t is None else t.data_ptr()
    a.x, a.w, a.bias, a.scale, a.shift, a.y = ptr(x), ptr(w), ptr(bias), ptr(scale), ptr(shift), ptr(y)
    rc = L.lib().tdvc_crepe_conv(C.byref(a), stream(dev))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('name', sorted(CONV_CASES))
def test_conv_against_float64(dev, name):
    c = conv_case(name)
    layer, Cin, Cout, Lin = CONV_CASES[name]
    assert c['flipped'] > 0 and bool((c['scale'] < 0).any())                    # the pool before the affine would change a winner
    p = f'conv{layer}'
    w = c['sd'][p + '.weight'].to(dev).contiguous()
    bias, scale, shift = c['sd'][p + '.bias'].to(dev), c['scale'].to(dev), c['shift'].to(dev)
    Nmax, Lout = max(CONV_N), c['y64'].shape[2]
    worst = 0.0
    for N in CONV_N:
        xd = c['x'][:N].to(dev).contiguous()
        y = torch.full((Nmax, Cout, Lout), NAN, device=dev)
        poison_lds(dev)
        rc = conv_call(dev, xd, w, bias, scale, shift, y, N, Cin, Cout, Lin, R.KERNELS[layer - 1], R.STRIDES[layer - 1])
        assert rc == 0, pkg()._lib.lib().tdvc_last_error()
        got = y.double().cpu()
        assert torch.isnan(got[N:]).all(), f'N={N}: frames past N were written'
        assert torch.isfinite(got[:N]).all(), f'N={N}'
        worst = max(worst, float((got[:N] - c['y64'][:N]).abs().max()))
    print(f'crepe_conv {name} {Cin}->{Cout} on {Lin}: {c["flipped"]} pooled outputs depend on the order of pool and affine; '
          f'max|y - y64| {worst:.3e}, bar {c["bar"]:.3e}, error / bar {worst / c["bar"]:.3f}')
    assert worst <= c['bar']


# ------------------------------------------------------------------------------------------------------------------- 3. head
@pytest.mark.parametrize('C6,N', [(64, 1), (64, 17), (512, 1), (512, 17)])
def test_head_against_float64(dev, C6, N):
    g = torch.Generator().manual_seed(C6 + N)
    sd = {'classifier.weight': (2 * torch.rand(360, 4 * C6, generator=g) - 1) * math.sqrt(3.0 / (4 * C6)),
          'classifier.bias': (2 * torch.rand(360, generator=g) - 1) / math.sqrt(4 * C6)}
    x = torch.randn(N, C6, 4, generator=g)
    y64 = R.head(sd, x[..., None])
    y32 = R.head(sd, x[..., None], torch.float32)
    bar = 4 * float((y32.double() - y64).abs().max())
    wrong = float((R.head(sd, x[..., None], channel_major=True) - y64).abs().max())
    assert bar > 0 and wrong > 100 * bar
    poison_lds(dev)
    got = K().crepe_head(x.to(dev), sd['classifier.weight'].to(dev), sd['classifier.bias'].to(dev))
    assert got.shape == (N, 360) and got.dtype == torch.float32
    err = float((got.double().cpu() - y64).abs().max())
    print(f'crepe_head {4 * C6} features N={N}: max|y - y64| {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}; the channel-major '
          f'flatten is {wrong / bar:.0f} bars away')
    assert err <= bar
    if N == 17:                                                                 # the [B, 360, F] layout of Crepe.activations: n = b F + f
        rows = K().crepe_head(x[:16].to(dev), sd['classifier.weight'].to(dev), sd['classifier.bias'].to(dev), frames_per_row=8)
        assert rows.shape == (2, 360, 8) and torch.equal(rows.permute(0, 2, 1).reshape(16, 360), got[:16])


# ----------------------------------------------------------------------------------------------------------------- 4. decode
WIDE = (32.0, 2006.0)      # bins [0, 360): the window is cut by 0 and by 360 themselves


@functools.lru_cache(maxsize=None)
def decode_case():
    """fp32 activations [2, 360, F]: row 0 for the reference's range [39, 248), row 1 the same construction for the whole axis."""
    rows = []
    for lo, hi in ((39, 248), (0, 360)):
        cols = []
        for k in range(24):                                                     # a centre that moves, fractional: no symmetry
            cols.append(R.bump(lo + 20 + 6.37 * k, 0.55 + 0.015 * k))
        for c in (lo, lo + 1, lo + 2, lo + 3, lo + 4, lo + 5, hi - 1, hi - 2, hi - 3, hi - 4, hi - 5, hi - 6):      # the window cut at both edges
            cols.append(R.bump(c + 0.3, 0.8))
        if lo > 0:                                                              # centres in the mask: the masked maximum must win
            cols += [np.maximum(R.bump(lo - 19, 0.9), R.bump(120.4, 0.5)), np.maximum(R.bump(hi + 30, 0.9), R.bump(150.2, 0.4)),
                     R.bump(lo - 2, 0.9), R.bump(hi + 1, 0.9), R.bump(hi, 0.95)]
        else:                                                                   # as many columns for the whole axis: bumps at both ends again
            cols += [R.bump(c, 0.6) for c in (0.0, 2.5, 180.49, 357.5, 359.0)]
        tie = R.bump(100.0, 0.3)
        tie[[110, 150, 200]] = 0.75                                             # exact ties: the lowest index
        plateau = np.full(360, 0.5)
        cols += [tie, plateau]
        for peak in (0.2085, 0.2115, 0.2, 0.22):                                  # both sides of the threshold
            cols.append(R.bump(130.0, peak, floor=0.01))
        rows.append(np.stack(cols, 1))
    a = np.stack(rows).astype(np.float32)
    a.setflags(write=False)
    return a


def test_decode_argmax_and_weighted(dev):
    a = decode_case()
    ad = torch.from_numpy(np.array(a)).to(dev)
    for row, (fmin, fmax) in enumerate(((50.0, 550.0), WIDE)):
        assert K().bin_range(fmin, fmax) == ((39, 248), (0, 360))[row]
        peaks = a[row, :, -4:].max(0).astype(np.float64)
        assert (np.abs(peaks - 0.21) >= 1e-3).all() and (peaks < 0.21).any() and (peaks > 0.21).any()
        for decoder, tol in (('argmax', 4 * U24), ('weighted_argmax', 64 * U24)):
            want = R.decode(a[row].astype(np.float64), fmin, fmax, decoder)
            open_ = R.decode(a[row].astype(np.float64), fmin, fmax, decoder, threshold=0.0)
            pitch, per = K().crepe_decode(ad[row:row + 1], fmin, fmax, decoder)
            all_p, _ = K().crepe_decode(ad[row:row + 1], fmin, fmax, decoder, threshold=0.0)
            assert pitch.shape == per.shape == (1, a.shape[2]) and pitch.dtype == torch.float32
            pitch, per, all_p = pitch[0].double().cpu().numpy(), per[0].double().cpu().numpy(), all_p[0].double().cpu().numpy()
            assert np.array_equal(per, want['periodicity'])                     # the fp32 activation at the chosen bin, exactly
            assert np.array_equal(pitch != 0, want['voiced']) and want['voiced'].any() and not want['voiced'].all()
            rel = np.abs(all_p - open_['pitch']) / open_['pitch']               # threshold 0: the bin of every frame shows in its pitch
            relv = np.abs(pitch - want['pitch'])[want['voiced']] / want['pitch'][want['voiced']]
            print(f'crepe_decode {decoder} bins [{fmin}, {fmax}) Hz: {a.shape[2]} frames, worst relative Hz error {rel.max():.3e}, '
                  f'error / bar {max(rel.max(), relv.max()) / tol:.3f}')
            assert rel.max() <= tol and relv.max() <= tol                       # a bin is 1.2 % wide: within the bar means the same bin
            if decoder == 'argmax':
                got_bins = np.rint((1200.0 * np.log2(all_p / 10.0) - R.CENTS0) / 20.0).astype(np.int64)
                assert np.array_equal(got_bins, open_['bins'])
    tie = a.shape[2] - 6
    assert R.decode(a[0].astype(np.float64))['bins'][tie] == 110 and R.decode(a[0].astype(np.float64))['bins'][tie + 1] == 39
    lengths = torch.tensor([5], dtype=torch.int32, device=dev)                  # frame counts: frames at and past them give 0, 0
    p5, q5 = K().crepe_decode(ad[:1], lengths=lengths)
    full_p, full_q = K().crepe_decode(ad[:1])
    assert torch.equal(p5[:, :5], full_p[:, :5]) and torch.equal(q5[:, :5], full_q[:, :5]) and not bool(p5[:, 5:].any()) and not bool(q5[:, 5:].any())
    view = torch.full((1, 360, a.shape[2] + 3), NAN, device=dev)                # a view with dense frames stays a view
    view[:, :, :a.shape[2]] = ad[:1]
    pv, qv = K().crepe_decode(view[:, :, :a.shape[2]])
    assert torch.equal(pv, full_p) and torch.equal(qv, full_q)


def got_path(dev, act32, fmin=50.0, fmax=550.0):
    """The device's Viterbi path as bins, read from the pitch at threshold 0."""
    p, per = K().crepe_decode(torch.from_numpy(act32[None]).to(dev), fmin, fmax, 'viterbi', threshold=0.0)
    b = np.rint((1200.0 * np.log2(p[0].double().cpu().numpy() / 10.0) - R.CENTS0) / 20.0).astype(np.int64)
    assert np.array_equal(per[0].cpu().numpy(), act32[b, np.arange(act32.shape[1])])
    return b


def viterbi_bound(act32, lo, hi):
    Fn = act32.shape[1]
    return Fn * 2.0 ** -21 * (float(np.abs(R.log_observations(act32, lo, hi)).max()) + math.log(144.0))


@functools.lru_cache(maxsize=None)
def dyadic_case(seed=3):
    """Activations that are multiples of 1/64: a ridge that wanders by up to 3 bins per frame over random dyadic clutter."""
    rng = np.random.default_rng(seed)
    Fn = 40
    a = rng.integers(0, 17, size=(360, Fn)) / 64.0
    c = 120
    for f in range(Fn):
        c = int(np.clip(c + rng.integers(-3, 4), 45, 240))
        a[c, f] = 60 / 64.0
        a[c - 1, f], a[c + 1, f] = 40 / 64.0, 36 / 64.0
    return a.astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_case(seed=5):
    """Real-valued bumps: a slow glide, and on every seventh frame a stronger distractor an octave (60 bins) above."""
    rng = np.random.default_rng(seed)
    Fn = 60
    cols = []
    for f in range(Fn):
        col = R.bump(100.0 + 0.9 * f + rng.uniform(-0.5, 0.5), rng.uniform(0.5, 0.7)) + rng.uniform(0.0, 0.02, 360)
        if f % 7 == 3:
            col = np.maximum(col, R.bump(160.0 + 0.9 * f, 0.9))
        cols.append(col)
    return np.stack(cols, 1).astype(np.float32)


def test_decode_viterbi(dev):
    lo, hi = 39, 248
    a = dyadic_case()
    assert np.array_equal(a * 64, np.rint(a * 64))
    want, margin = R.viterbi(a.astype(np.float64), lo, hi)
    bound = viterbi_bound(a, lo, hi)
    assert margin.min() > bound                                                 # the condition on the inputs
    got = got_path(dev, a)
    print(f'crepe viterbi, dyadic lattice: {a.shape[1]} frames, smallest float64 margin {margin.min():.3e} (bound {bound:.3e}), '
          f'frames off the float64 path {int((got != want).sum())}')
    assert np.array_equal(got, want)
    r = real_case()
    want, margin = R.viterbi(r.astype(np.float64), lo, hi)
    bound = viterbi_bound(r, lo, hi)
    excused = margin < bound
    assert not excused.any()                                                    # the seed was chosen so that the restatement leaves out none
    per_frame = R.decode(r.astype(np.float64), decoder='argmax', threshold=0.0)['bins']
    assert int((np.abs(per_frame - want) > 30).sum()) >= 5                      # the per-frame decision does jump to the distractor
    got = got_path(dev, r)
    off = (got != want) & ~excused
    print(f'crepe viterbi, real bumps: {r.shape[1]} frames, smallest float64 margin {margin.min():.3e} (bound {bound:.3e}), left out '
          f'{int(excused.sum())}, frames off the float64 path {int(off.sum())}; the per-frame argmax jumps on {int((np.abs(per_frame - want) > 30).sum())}')
    assert excused.mean() <= 0.02 and not off.any()
    assert np.abs(np.diff(got)).max() <= 11
    lat = K().crepe_lattice(torch.from_numpy(r[None]).to(dev))                  # the lattice launch against float64
    ref = R.log_observations(r.astype(np.float64), lo, hi)
    assert lat.shape == (1, r.shape[1], hi - lo)
    err = float(np.abs(lat[0].double().cpu().numpy() - ref).max())
    assert err <= 4 * U24 * float(np.abs(ref).max())


# ------------------------------------------------------------------------------------------------------------- 5. end to end
E2E_ROWS = (64, 1024, 2047, 8000)


@functools.lru_cache(maxsize=None)
def e2e_case():
    T = max(E2E_ROWS)
    x = np.full((len(E2E_ROWS), T), np.nan, dtype=np.float32)
    for b, n in enumerate(E2E_ROWS):
        x[b, :n] = R.tones(n, seed=20 + b)
    sd = R.state_dict(11, 'tiny')
    a64 = [R.activations(sd, x[b, :n]).numpy() for b, n in enumerate(E2E_ROWS)]
    a32 = [R.activations(sd, x[b, :n], dtype=torch.float32).double().numpy() for b, n in enumerate(E2E_ROWS)]
    bar = 4 * max(float(np.abs(p - q).max()) for p, q in zip(a32, a64))
    x.setflags(write=False)
    return x, sd, a64, bar


@functools.lru_cache(maxsize=None)
def tiny_model():
    return K().load_crepe(e2e_case()[1], 'tiny', device='cuda')


def test_activations_end_to_end(dev):
    x, sd, a64, bar = e2e_case()
    m = tiny_model()
    B, T = x.shape
    for b, n in enumerate(E2E_ROWS):                                            # neighbouring frames differ: mixed-up frames would show
        if a64[b].shape[1] > 1:
            assert float(np.abs(np.diff(a64[b], axis=1)).max(0).min()) > 100 * bar, b
    whole = torch.full((B, T + 3), NAN, device=dev)
    whole[:, :T] = torch.from_numpy(np.array(x)).to(dev)
    xd = whole[:, :T]
    lengths = torch.tensor(E2E_ROWS, dtype=torch.int32, device=dev)
    poison_lds(dev)
    act = m.activations(xd[:, None], lengths=lengths)
    Fm = 1 + T // 64
    assert act.shape == (B, 360, Fm) and act.dtype == torch.float32 and bool(torch.isfinite(act).all())
    got = act.double().cpu().numpy()
    for b, n in enumerate(E2E_ROWS):
        nf = 1 + n // 64
        err = float(np.abs(got[b, :, :nf] - a64[b]).max())
        print(f'Crepe(tiny).activations n={n}: {nf} frames, max|a - a64| {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}')
        assert err <= bar, (b, n, err, bar)
        alone = m.activations(xd[b, :n])
        assert alone.shape == (1, 360, nf) and torch.equal(alone[0], act[b, :, :nf]), f'row {b} alone differs from the row in the batch'
    assert torch.equal(m.activations(xd[:, None], lengths=lengths), act)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.activations(xd, lengths=lengths)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m.activations(xd, lengths=lengths)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, act)


def test_filtered_pitch_with_each_decoder(dev):
    m = tiny_model()
    x = torch.from_numpy(np.array(e2e_case()[0][3])).to(dev)[None, None]         # [1, 1, 8000], a full row
    Fm = 1 + x.shape[-1] // 64
    for decoder in ('argmax', 'weighted_argmax', 'viterbi'):
        pitch, act = m.filtered_pitch(x, decoder)
        assert pitch.shape == (1, 1, Fm) and act.shape == (1, 360, Fm) and pitch.dtype == torch.float32
        again, _ = K().crepe_decode(act, 50.0, 550.0, decoder, 0.21)
        assert torch.equal(pitch[:, 0], again)
        flat, _ = m.filtered_pitch(x[:, 0], decoder)
        assert flat.shape == (1, Fm) and torch.equal(flat, pitch[:, 0])
        assert bool(((pitch == 0) | ((pitch > 49.0) & (pitch < 560.0))).all()) and bool((pitch > 0).any())


def test_full_capacity_on_one_row(dev):
    sd = R.state_dict(12, 'full')
    x = R.tones(1024, seed=31)
    a64 = R.activations(sd, x).numpy()
    a32 = R.activations(sd, x, dtype=torch.float32).double().numpy()
    bar = 4 * float(np.abs(a32 - a64).max())
    m = K().load_crepe(sd, 'full', device=dev)
    act = m.activations(torch.from_numpy(x).to(dev))
    assert act.shape == (1, 360, 17)
    err = float(np.abs(act[0].double().cpu().numpy() - a64).max())
    print(f'Crepe(full).activations n=1024: 17 frames, max|a - a64| {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}')
    assert err <= bar


def test_convert_audio_with_and_without_the_tracker(dev):
    P = pkg()
    G, _ = build_models(dev)
    m = tiny_model()
    T = 8320
    rng = np.random.default_rng(12)
    x = torch.from_numpy(R.tones(T, seed=41, amp=0.3))[None, None].to(dev)
    tgt = torch.from_numpy(R.tones(4800, seed=42, amp=0.3))[None, None].to(dev)
    c_tgt = torch.zeros(1, 16, device=dev); c_tgt[0, 3] = 1.0
    noise = (torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev),
             torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev))
    phi0 = torch.tensor([0.5], device=dev)
    f0_src, f0_tgt = m.filtered_pitch(x, 'viterbi')[0], m.filtered_pitch(tgt, 'viterbi')[0]
    assert f0_src.shape == (1, 1, T // 64 + 1)
    y = P.infer.convert_audio(G, x, c_tgt, f0_ratio=1.25, noise=noise, start_phase=phi0, f0_tracker=m)
    y_ref = P.infer.convert(G, x, c_tgt, f0_src * 1.25, noise=noise, start_phase=phi0)
    assert y.shape == (1, 1, T) and bool(torch.isfinite(y).all()) and torch.equal(y, y_ref)
    y2 = P.infer.convert_audio(G, x, c_tgt, noise=noise, start_phase=phi0, f0_tracker=m, target_signal=tgt)
    assert torch.equal(y2, P.infer.convert(G, x, c_tgt, P.infer.shift_f0(f0_src, f0_tgt), noise=noise, start_phase=phi0))
    plain = P.infer.convert_audio(G, x, c_tgt, f0_ratio=1.25, noise=noise, start_phase=phi0)      # no tracker: the parent commit's path
    assert torch.equal(plain, P.infer.convert(G, x, c_tgt, P.track_f0(x) * 1.25, noise=noise, start_phase=phi0))
    with pytest.raises(ValueError):
        P.infer.convert_audio(G, x, c_tgt, f0_tracker=m, decoder='viterbi')
    with pytest.raises(ValueError):
        P.infer.convert_audio(G, x, c_tgt, target_signal=tgt)


# -------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_before_any_launch(dev):
    L = pkg()._lib
    lib = L.lib()
    x = torch.zeros(2, 2048, device=dev)
    m = tiny_model()
    for fn in (lambda: K().crepe_frames(x, sample_rate=44100), lambda: m.activations(x, sample_rate=22050), lambda: K().crepe_frames(x, hop=0),
               lambda: m.activations(x, hop=-64), lambda: K().crepe_frames(x[:, :0]), lambda: K().crepe_frames(x, lengths=torch.ones(3, device=dev)),
               lambda: m.activations(x, lengths=torch.ones(2, 1, device=dev)), lambda: K().crepe_decode(torch.zeros(1, 360, 4, device=dev), 550.0, 50.0),
               lambda: K().crepe_decode(torch.zeros(1, 360, 4, device=dev), 8000.0, 9000.0), lambda: K().crepe_decode(torch.zeros(1, 360, 4, device=dev), decoder='median'),
               lambda: K().crepe_decode(torch.zeros(1, 359, 4, device=dev)), lambda: K().crepe_decode(torch.zeros(2, 360, 4, device=dev), lengths=torch.ones(3, device=dev)),
               lambda: K().crepe_decode(torch.zeros(1, 360, 4, device=dev), decoder='viterbi', lengths=torch.ones(1, device=dev)),
               lambda: K().Crepe('medium'), lambda: m.filtered_pitch(x, 'median')):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: K().crepe_frames(x.cpu()), lambda: m.activations(x.cpu()), lambda: K().crepe_decode(torch.zeros(1, 360, 4)),
               lambda: K().crepe_frames(x, lengths=torch.ones(2, dtype=torch.int32))):
        with pytest.raises(RuntimeError):
            fn()
    # the C ABI: the output stays untouched
    y = torch.full((4, 32, 64), -7.0, device=dev)
    xin, w, v = torch.zeros(4, 24, 128, device=dev), torch.zeros(32 * 24 * 64, device=dev), torch.zeros(32, device=dev)
    cases = [(dict(Cin=24), EUNSUPPORTED), (dict(Cout=24), EUNSUPPORTED), (dict(Lin=100), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED),
             (dict(stride=2), EUNSUPPORTED), (dict(Cin=16, K=512, stride=4, Lin=1024), EUNSUPPORTED), (dict(N=-1), EINVAL), (dict(null='w'), EINVAL),
             (dict(null='scale'), EINVAL), (dict(null='y'), EINVAL)]
    for kw, want in cases:
        g = dict(N=4, Cin=16, Cout=32, Lin=128, K=64, stride=1)
        g.update({k: val for k, val in kw.items() if k != 'null'})
        ops = dict(x=xin, w=w, bias=v, scale=v, shift=v, y=y)
        if 'null' in kw:
            ops[kw['null']] = None
        rc = conv_call(dev, ops['x'], ops['w'], ops['bias'], ops['scale'], ops['shift'], ops['y'], g['N'], g['Cin'], g['Cout'], g['Lin'], g['K'], g['stride'])
        assert rc == want and lib.tdvc_last_error(), (kw, rc)
        assert bool((y == -7.0).all()), kw
    with pytest.raises(ValueError):                                             # through the wrapper: channel counts that are not multiples of 16
        K().crepe_conv(xin, torch.zeros(32, 24, 64, device=dev), v, v, v)
    with pytest.raises(ValueError):
        K().crepe_head(torch.zeros(2, 24, 4, device=dev), torch.zeros(360, 96, device=dev), torch.zeros(360, device=dev))
    out = torch.full((2, 5), -7.0, device=dev)
    st = stream(dev)
    act = torch.zeros(2, 360, 5, device=dev)
    dec = lambda lo, hi, mode, bins=None, a_cs=5: lib.tdvc_crepe_decode(act.data_ptr(), 1800, a_cs, 2, 5, 360, lo, hi, mode, 0.21, None, bins,
                                                                        out.data_ptr(), out.data_ptr(), None, st)
    assert dec(40, 40, 0) == EUNSUPPORTED and dec(-1, 10, 0) == EUNSUPPORTED and dec(0, 361, 0) == EUNSUPPORTED
    assert dec(39, 248, 3) == EINVAL and dec(39, 248, 2) == EINVAL and dec(39, 248, 0, a_cs=4) == EINVAL
    assert dec(39, 248, 1, bins=torch.zeros(2, 5, dtype=torch.int32, device=dev).data_ptr()) == EINVAL
    fr = lambda T, hop, F: lib.tdvc_crepe_frames(x.data_ptr(), 2048, None, T, 2, hop, F, out.data_ptr(), st)
    assert fr(2048, 0, 33) == EUNSUPPORTED and fr(0, 64, 1) == EUNSUPPORTED and fr(2048, 64, 32) == EINVAL
    assert lib.tdvc_crepe_head(act.data_ptr(), 10, 16, 4, act.data_ptr(), act.data_ptr(), 360, 3, out.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
