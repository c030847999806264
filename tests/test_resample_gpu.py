"""GPU: tdvc_resample / tdvc_segment (csrc/audio_resample.hip) through resample.resample / load_segments against the float64
restatement tests/resample_ref.py (the per-sample loop with the float time register, eq_rms, the segment steps).

Bound (per row, every element): |y - truth| <= 4 * 2^-24 * max|truth_row|, the bar of tests/peq_ref.py. resample's output is the
float64 sum rounded once to fp32 (<= 2^-25 of the element, a quarter of the bound at the row maximum); load_segments rounds twice
(the resampled row to fp32, then the scaled sample), half of the bound. The exact integer phase against the float time register and
another float64 summation order are below 1e-12 of the row maximum. Inputs: a few harmonics plus noise at about -30 dB, seeded.
"""
import functools

import numpy as np
import pytest
import torch

import resample_ref as RR
from common import pkg

pytestmark = pytest.mark.gpu

TO = 256      # asserted against the library below


def assert_within_bound(y, ref, what):
    """y: device or numpy fp32 [B, N]; ref float64 [B, N]. Prints the worst error in units of the bound, then asserts."""
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else y
    assert y.dtype == np.float32 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    assert np.isfinite(y).all(), what
    bd = RR.bound(ref)
    err = np.abs(y.astype(np.float64) - ref)
    worst = float((err / np.where(bd > 0, bd, 1.0)).max()) if err.size else 0.0
    print(f'[resample] {what}: worst |y - truth| / bound = {worst:.3f}')
    assert (err <= bd).all(), (what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def case(name):
    """(x fp32 [B, T] padded, lengths, sr_orig, sr_new, filter, truth float64 [B, max n_out], n_out): computed once per session"""
    sr_new, filt, fill, T = 16000, 'kaiser_best', 0.0, None
    if name == 'down3':
        sr, lengths, seed = 48000, (6000, 4097, 385), 1
    elif name == 'down_frac':
        sr, lengths, seed = 44100, (5000, 1323), 2
    elif name == 'l320':
        sr, lengths, seed = 22050, (4000,), 3
    elif name == 'up_3_2':
        sr, sr_new, lengths, seed = 16000, 24000, (3000, 64), 4
    elif name == 'up_2_1':
        sr, sr_new, lengths, seed = 8000, 16000, (3000, 64), 5
    elif name == 'tiny':
        sr, lengths, seed = 48000, (1, 2, 3, 50), 6
    elif name == 'tile_l1':      # L = 1
        sr, seed = 48000, 7
        lengths = tuple(RR.length_for(n, sr, sr_new) for n in (TO - 1, TO, TO + 1, 2 * TO + 1))
    elif name == 'tile_l2':      # L = 2: the per-lane weights kernel (24 kHz -> 16 kHz; upsampling cannot give every n_out)
        sr, seed = 24000, 8
        lengths = tuple(RR.length_for(n, sr, sr_new) for n in (TO - 1, TO, TO + 1, 2 * TO + 1))
    elif name == 'odd':          # rows of a wider buffer, 1e3 past each row's length
        sr, lengths, seed, fill, T = 44100, (2001, 1500, 777), 9, 1e3, 2001
    elif name == 'kaiser_fast':
        sr, lengths, seed, filt = 48000, (1500, 700), 10, 'kaiser_fast'
    elif name == 'kaiser_fast_up':
        sr, sr_new, lengths, seed, filt = 16000, 24000, (900, 333), 11, 'kaiser_fast'
    else:
        raise KeyError(name)
    x = RR.padded(np.random.default_rng(seed), lengths, sr, fill=fill, T=T)
    truth, n_out = RR.resample_rows(x, lengths, sr, sr_new, filt)
    return x, lengths, sr, sr_new, filt, truth, n_out


def run_case(dev, name, x_dev=None):
    R = pkg().resample
    x, lengths, sr, sr_new, filt, truth, n_out = case(name)
    xd = torch.from_numpy(x).to(dev) if x_dev is None else x_dev
    y, n = R.resample(xd, sr, sr_new, lengths=lengths, filter=filt)
    assert n.host == n_out and n.dev.dtype == torch.int32 and n.dev.cpu().tolist() == n_out
    assert y.shape == truth.shape and y.dtype == torch.float32
    assert_within_bound(y, truth, name)
    for b, k in enumerate(n_out):
        assert not bool(y[b, k:].any()), (name, b)                      # exact zeros past the row's end
    return y, truth, n_out


def test_tile_constant_matches_the_library():
    P = pkg()
    assert P._lib.lib().tdvc_resample_tile() == P._lib.RESAMPLE_TO == P.resample.TO == TO


@pytest.mark.parametrize('name', ['down3', 'down_frac', 'l320', 'up_3_2', 'up_2_1', 'tile_l1', 'tile_l2'])
def test_resample_vs_float64(dev, name):
    _, truth, n_out = run_case(dev, name)
    if name.startswith('tile'):
        assert n_out == [TO - 1, TO, TO + 1, 2 * TO + 1]
    if name == 'down_frac':
        assert pkg().resample.resample_bank(44100, 16000).L == 160 and min(n_out) > 2 * 160      # every phase wraps several times


def test_tiny_rows(dev):
    y, _, n_out = run_case(dev, 'tiny')
    assert n_out == [0, 0, 1, 16]
    assert not bool(y[:2].any()) and bool(torch.isfinite(y).all())
    R = pkg().resample
    x = torch.from_numpy(case('tiny')[0]).to(dev)
    y0, n0 = R.resample(x[:2], 48000, 16000, lengths=[1, 2])             # nothing to compute at all
    assert y0.shape == (2, 0) and n0.host == [0, 0]


def test_odd_strided_rows_do_not_leak_their_padding(dev):
    x, lengths, *_ = case('odd')
    pitch = 2003                                                         # not a multiple of 4
    wide = torch.full((len(lengths), pitch), 1e3, device=dev)
    wide[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    xv = wide[:, :x.shape[1]]
    assert xv.stride(0) == pitch and not xv.is_contiguous()
    assert all(float(xv[b, n:].min()) == 1e3 for b, n in enumerate(lengths) if n < x.shape[1])
    y, truth, _ = run_case(dev, 'odd', x_dev=xv)
    assert float(y.abs().max()) < 1.0                                    # a leaked sentinel would be ~1e3 * a filter weight


@pytest.mark.parametrize('name', ['kaiser_fast', 'kaiser_fast_up'])
def test_kaiser_fast_by_name_and_as_a_table(dev, name):
    R = pkg().resample
    y, _, _ = run_case(dev, name)
    x, lengths, sr, sr_new, *_ = case(name)
    table, precision = RR.sinc_window('kaiser_fast')
    y2, _ = R.resample(torch.from_numpy(x).to(dev), sr, sr_new, lengths=lengths, filter=(table.copy(), precision))
    assert torch.equal(y, y2)
    yb, _ = R.resample(torch.from_numpy(x).to(dev), sr, sr_new, lengths=lengths)
    assert yb.shape == y.shape and not torch.equal(y, yb)                # and it is not the default filter


def test_layouts_repeats_and_guards(dev):
    P = pkg()
    R = P.resample
    x, lengths, sr, sr_new, *_ = case('down3')
    xd = torch.from_numpy(x).to(dev)
    y, n = R.resample(xd, sr, sr_new, lengths=lengths)
    y2, _ = R.resample(xd, sr, sr_new, lengths=lengths)
    assert torch.equal(y, y2)                                            # bit-identical
    y3, _ = R.resample(xd[:, None], sr, sr_new, lengths=lengths)
    assert y3.shape == (3, 1, y.shape[1]) and torch.equal(y3[:, 0], y)
    y1, n1 = P.resample(xd[1, :lengths[1]], sr, sr_new)                  # [T], default lengths, the package-level name
    assert y1.shape == (n.host[1],) and torch.equal(y1, y[1, :n.host[1]])
    same, ns = R.resample(xd, 16000, 16000, lengths=lengths)
    assert same is xd and ns.host == list(lengths)                       # equal rates: the input itself
    with pytest.raises(ValueError):
        R.resample(xd, 16000, 44101)                                     # 44101 phases: a bank over 8 MiB
    with pytest.raises(P._lib.TdvcError):
        R.resample(torch.from_numpy(x), sr, sr_new)                      # no CPU fallback
    with pytest.raises(ValueError):
        R.resample(xd, sr, sr_new, lengths=[1, 2, x.shape[1] + 1])


def test_c_abi_refuses_a_bank_over_8_mib(dev):
    """The library's own check, before any launch: TDVC_EUNSUPPORTED for L * W * 8 bytes > 8 MiB."""
    L = pkg()._lib
    t = torch.zeros(16, device=dev)
    i = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.lib().tdvc_resample(t.data_ptr(), 16, i.data_ptr(), i.data_ptr(), 1, 16, 4, t.data_ptr(), 44101, 1, 44101, 16000, 130, 65, t.data_ptr(), 16,
                               t.data_ptr(), 64, None)
    assert rc == L.EUNSUPPORTED and b'8 MiB' in L.lib().tdvc_last_error()


def test_resample_under_graph_capture(dev):
    """Once the bank and the lengths are cached the call uploads nothing and can be captured; a replay follows its input."""
    R = pkg().resample
    x, lengths, sr, sr_new, *_ = case('down_frac')
    xd = torch.from_numpy(x).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        R.resample(xd, sr, sr_new, lengths=lengths)                      # warm-up: library load, bank and lengths upload, allocator
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, _ = R.resample(xd, sr, sr_new, lengths=lengths)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(y, R.resample(xd, sr, sr_new, lengths=lengths)[0])
    xd.mul_(-0.5)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(y, R.resample(xd, sr, sr_new, lengths=lengths)[0])


# ---- load_segments

MS = 5120


@functools.lru_cache(maxsize=None)
def seg_case():
    """48 kHz -> 16 kHz rows around max_segment = 5120: two longer rows, one whose crop ends on its last sample, one of exactly
    5120, a shorter one and a silent one; the resampled float64 rows and the draws."""
    sr = 48000
    n_out = (6000, 5800, 5500, MS, 2000, 5300)
    lengths = tuple(RR.length_for(n, sr, 16000) for n in n_out)
    rng = np.random.default_rng(21)
    x = RR.padded(rng, lengths, sr)
    x[5] = 0.0                                                           # silent, and longer than max_segment
    res, n = RR.resample_rows(x, lengths, sr, 16000)
    assert n == list(n_out)
    start = np.array([0, n_out[1] - MS - 1, n_out[2] - MS, 7, 3, 11], np.int32)      # rows 3, 4 are not cropped: their start is ignored
    aug_gain = rng.uniform(0.3, 1.0, 6).astype(np.float32)
    aug_sign = np.array([1, -1, 1, -1, -1, 1], np.float32)
    noise = rng.standard_normal((6, RR.segment_size(MS))).astype(np.float32)
    return dict(x=x, lengths=lengths, sr=sr, res=res, n_out=n, start=start, aug_gain=aug_gain, aug_sign=aug_sign, noise=noise)


def seg_truth(c, data_augment, augment_noise, rows=None, db=-30):
    rows = range(len(c['n_out'])) if rows is None else rows
    return np.stack([RR.segment(c['res'][b, :c['n_out'][b]], db, data_augment, c['aug_gain'][b], c['aug_sign'][b], int(c['start'][b]), MS,
                                c['noise'][b], augment_noise) for b in rows])


@pytest.mark.parametrize('data_augment,augment_noise', [(True, None), (True, 0.003), (False, None)])
def test_load_segments_vs_float64(dev, data_augment, augment_noise):
    P = pkg()
    c = seg_case()
    to = lambda a: torch.from_numpy(a).to(dev)
    out, info = P.load_segments(to(c['x']), c['lengths'], c['sr'], max_segment=MS, data_augment=data_augment, augment_noise=augment_noise,
                                aug_gain=to(c['aug_gain']), aug_sign=to(c['aug_sign']), start=to(c['start']), noise=to(c['noise']))
    S = out.shape[2]
    assert out.shape == (6, 1, S) and out.dtype == torch.float32 and S % 320 == 0 and S >= 5120 and S == RR.segment_size(MS)
    assert info['n_out'] == c['n_out']
    ref = seg_truth(c, data_augment, augment_noise)
    assert_within_bound(out[:, 0], ref, f'load_segments augment={data_augment} noise={augment_noise}')
    if augment_noise is None:
        assert not bool(out[5].any())                                    # the silent row: zeros, no NaN
        assert not bool(out[4, 0, c['n_out'][4]:].any())                 # zero padding behind a short row
    target = 10 ** (-30 / 20)
    gain = info['gain'].cpu().numpy()
    for b in range(5):                                                   # full-row RMS before augmentation
        r = np.sqrt((c['res'][b, :c['n_out'][b]] ** 2).mean())
        assert abs(gain[b] * r - target) <= 1e-6 * target, (b, gain[b] * r)
    assert gain[5] == 0.0
    if not data_augment and augment_noise is None:
        for b in (3, 4):                                                 # uncropped rows carry their whole row: measure it on the output
            r = float(np.sqrt((out[b, 0, :c['n_out'][b]].double().cpu().numpy() ** 2).mean()))
            assert abs(r - target) <= 1e-6 * target, (b, r)


def test_load_segments_equal_rate_and_options(dev):
    """sr_orig == sample_rate: no resampling, the RMS from the row itself, one rounding. Also normalization_db=None and another level."""
    P = pkg()
    c = seg_case()
    to = lambda a: torch.from_numpy(a).to(dev)
    rows = [0, 1, 4]
    lengths = [6000, 5800, 2000]
    x = c['x'][rows][:, :6000].copy()
    x[2, 2000:] = 1e3                                                    # padding of the collated batch: not the row's signal
    fake = dict(c, res=x.astype(np.float64), n_out=lengths, start=c['start'][rows], aug_gain=c['aug_gain'][rows],
                aug_sign=c['aug_sign'][rows], noise=c['noise'][rows])
    kw = dict(max_segment=MS, aug_gain=to(fake['aug_gain']), aug_sign=to(fake['aug_sign']), start=to(fake['start']), noise=to(fake['noise']))
    out, info = P.load_segments(to(x), lengths, 16000, **kw)
    assert info['n_out'] == lengths
    assert_within_bound(out[:, 0], seg_truth(fake, True, None), 'load_segments equal rate')
    out, _ = P.load_segments(to(x), lengths, 16000, normalization_db=-20, augment_noise=0.01, **kw)
    assert_within_bound(out[:, 0], seg_truth(fake, True, 0.01, db=-20), 'load_segments equal rate, -20 dB, noise')
    out, info = P.load_segments(to(x), lengths, 16000, normalization_db=None, **kw)
    assert_within_bound(out[:, 0], seg_truth(fake, True, None, db=None), 'load_segments equal rate, no normalisation')
    assert bool((info['gain'] == 1).all())


def test_load_segments_default_draws(dev):
    """Seeded default draws: deterministic, every drawn crop holds a non-zero sample, gains in [0.3, 1], both signs, and
    device_batch takes the result."""
    P = pkg()
    R = P.resample
    sr, B = 48000, 8
    n_in = 3 * 9000
    rng = np.random.default_rng(33)
    x = np.zeros((B, n_in), np.float32)
    for b in range(B):                                                   # one short burst per row between long silences
        at = 3 * int(rng.integers(200, 8500))
        x[b, at:at + 900] = RR.make_signal(rng, 900, sr)
    xd = torch.from_numpy(x).to(dev)
    lengths = [n_in] * B
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    out, info = P.load_segments(xd, lengths, sr, max_segment=MS, augment_noise=0.001, generator=gen(5))
    out2, info2 = P.load_segments(xd, lengths, sr, max_segment=MS, augment_noise=0.001, generator=gen(5))
    assert torch.equal(out, out2) and torch.equal(info['start'], info2['start'])
    out3, info3 = P.load_segments(xd, lengths, sr, max_segment=MS, augment_noise=0.001, generator=gen(6))
    assert not torch.equal(out, out3)
    y, n = R.resample(xd, sr, 16000, lengths=lengths)
    start = info['start'].cpu().tolist()
    for b in range(B):
        assert 0 <= start[b] < n.host[b] - MS and bool(y[b, start[b]:start[b] + MS].any()), (b, start[b])
    g = info['aug_gain'].cpu().numpy()
    assert g.min() >= 0.3 and g.max() <= 1.0 and set(info['aug_sign'].cpu().tolist()) <= {-1.0, 1.0}
    replay, _ = P.load_segments(xd, lengths, sr, max_segment=MS, augment_noise=0.001, aug_gain=info['aug_gain'], aug_sign=info['aug_sign'],
                                start=info['start'], noise=info['noise'])
    assert torch.equal(out, replay)                                      # info replays the run
    clean, _ = P.load_segments(xd, lengths, sr, max_segment=MS, generator=gen(5))
    bt = P.device_batch(clean, torch.arange(B, device=dev) % 16, 16, generator=gen(1))
    assert bt['signal_real'].shape == (B, 1, RR.segment_size(MS)) and bt['signal_corrupted'].shape == bt['signal_real'].shape
    assert all(bool(torch.isfinite(v).all()) for v in bt.values() if v.is_floating_point())
