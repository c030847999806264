"""GPU: WORLD's DIO and StoneMask on the device (td-vc-gan_amd/pitch.py dio / stonemask / world_f0, mcd(f0_method='dio');
csrc/pitch_dio.hip) through the package and through the raw C ABI, against the float64 restatement tests/dio_ref.py, which
tests/test_dio_cpu.py pins to independent facts and shows to be stable in its discrete decisions on exactly these waveforms.
pyworld is not available: nothing here is a parity test against WORLD.

Bars: the device evaluates in float64 and rounds once, so every voiced f0 is within 4 * 2^-24 relative of the restatement (the
project's factor 4 on one fp32 rounding) and zeros are exact: the voiced sets are identical, no frame excluded. Candidates and
scores are float64 and within 1e-9 relative, with identical zeros.

1. dio on a B = 3 batch of glides with two unvoiced gaps (lengths 4000, 8000, 16040: no multiple of the hop or of the 1024-sample
   tile) in a padded, strided buffer with NaN at and past every length and spare output columns that keep their sentinel; the
   same through the package, on one dense row without lengths and on a [T] input.
2. Degenerate rows: zeros, len = 0, F <= vrm, 1500 samples, the 100 -> 200 Hz step, the last frame on the final sample, a length one
   short of a tile edge and one past it, for the 1024-sample tiles of the filters and the 1022-sample tiles of the events.
3. A second parameter set: fs 24000, hop 120, floor 71, ceil 800, 4 channels per octave (14 bands).
4. stonemask: a constructed track over every N from 256 to 4096, the special values, windows clamped at both row ends, tracks 30 %
   and 5 % off, a strided f0 view, in place.
5. world_f0 end to end: voiced sets identical, values within the bar except where the device's fp32 DIO value is one ulp from the
   restatement's AND the restatement itself moves by more than the bar when given the device's value; at most 1 % of the voiced frames.
6. mcd(f0_method='dio') equals mcd with world_f0's tracks entry for entry; the default equals f0_method='yin' bit for bit; the
   call is captured into a graph and replays to the same bits; an unknown method raises.
7. Two calls of each operator are bit-identical.
Measured on an MI355X (printed by the tests, run with -s), worst error over its bar:
    case                        f0      candidates   scores
    batch of three glides       0.225   1.2e-02      0.16
    one dense row               0.194   2.6e-03      0.04
    degenerate rows             0.207   2.4e-02      0.41
    fs 24000, 14 bands          0.216   2.0e-02      0.09
    stonemask, all tracks       0.235
    world_f0 end to end         0.233 / 0.202 / 0.221 on 247 / 114 / 50 voiced frames, no frame excepted
0.25 of the f0 bar is 2^-24: the one rounding to fp32 and nothing else. The scores are the ill-conditioned output (a standard
deviation of four nearly equal values divided by their mean) and still sit under half of the 1e-9 bar.
"""
import numpy as np
import pytest
import torch

import dio_ref as R
from common import pkg, traced

pytestmark = pytest.mark.gpu
NAN = float('nan')
BAR = 4 * 2.0 ** -24
BAR64 = 1e-9
BATCH = ('glide4000', 'glide8000', 'glide16040')
DIO_KERNELS = {'dio_tables_kernel', 'dio_mean_kernel', 'dio_lowcut_kernel', 'dio_band_kernel<0>', 'dio_band_kernel<1>',
               'dio_candidate_kernel', 'dio_fix_kernel'}


def padded(dev, names, lead=8, tail=24):
    """The rows of a wider buffer: signal view [B, Tmax] with NaN before, behind and at and past every length; lengths int32 [B]."""
    rows = [R.waveform(n) for n in names]
    T = max(max(len(r) for r in rows), 1)
    buf = np.full((len(rows), lead + T + tail), np.nan, np.float32)
    for b, r in enumerate(rows):
        buf[b, lead:lead + len(r)] = r
    t = torch.from_numpy(buf).to(dev)
    return t[:, lead:lead + T], torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)


def check_f0(got, want, what):
    """got: device fp32 row(s) [F]; want: float64 [F_b]. Voiced set identical, zeros exact (past F_b too), values within BAR."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    assert (got[len(want):] == 0).all(), what
    got = got[:len(want)]
    assert np.array_equal(got > 0, want > 0), (what, np.nonzero((got > 0) != (want > 0))[0][:8])
    assert (got[want == 0] == 0).all(), what
    v = want > 0
    ratio = np.abs(got - want)[v] / (BAR * want[v]) if v.any() else np.zeros(1)
    assert (ratio <= 1).all(), (what, float(ratio.max()))
    return float(ratio.max())


def check_f64(got, want, what):
    """Float64 candidates or scores [nb, F] against [nb, F_b]: identical zeros, BAR64 relative elsewhere."""
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float64 and np.isfinite(got).all(), what
    fb = want.shape[1]
    assert (got[:, fb:] == (0.0 if 'cand' in what else R.BIG / R.EPS)).all(), what
    got = got[:, :fb]
    assert np.array_equal(got == 0, want == 0), what
    nz = want != 0
    ratio = np.abs(got - want)[nz] / (BAR64 * np.abs(want[nz])) if nz.any() else np.zeros(1)
    assert (ratio <= 1).all(), (what, float(ratio.max()))
    return float(ratio.max())


def check_rows(names, f0, cand, score, what):
    worst = [0.0, 0.0, 0.0]
    for b, n in enumerate(names):
        r = R.dio_of(n)
        worst[0] = max(worst[0], check_f0(f0[b], r['f0'], f'{what} f0 {n}'))
        worst[1] = max(worst[1], check_f64(cand[b], r['cand'], f'{what} cand {n}'))
        worst[2] = max(worst[2], check_f64(score[b], r['score'], f'{what} score {n}'))
    print(f'\n{what}: worst f0 error over 4 * 2^-24 relative {worst[0]:.3f}; worst candidate and score error over 1e-9 relative '
          f'{worst[1]:.2e} and {worst[2]:.2e}')
    return worst


def raw_dio(dev, x, lengths, f0, cand, score, fs=R.FS, hop=R.HOP, floor=50.0, ceil=500.0, cpo=2.0, allowed=0.1):
    lib = pkg()._lib.lib()
    B, T = x.shape
    F = T // hop + 1
    n = lib.tdvc_dio_workspace(B, T, F, hop, fs, floor, ceil, cpo)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib.tdvc_dio(x.data_ptr(), x.stride(0), x.stride(1), None if lengths is None else lengths.data_ptr(), T, B, F, hop, fs, floor, ceil,
                      cpo, allowed, f0.data_ptr(), f0.stride(0), cand.data_ptr(), score.data_ptr(), ws.data_ptr(), n,
                      torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------ dio
def test_dio_batch_in_a_padded_strided_buffer(dev):
    P = pkg()
    x, lengths = padded(dev, BATCH)
    B, T = x.shape
    F, nb, spare = T // R.HOP + 1, 7, 5
    assert not x.is_contiguous() and bool(torch.isnan(x).any())
    f0 = torch.full((B, F + spare), -7.0, dtype=torch.float32, device=dev)
    cand = torch.full((B, nb, F), -7.0, dtype=torch.float64, device=dev)
    score = torch.full((B, nb, F), -7.0, dtype=torch.float64, device=dev)
    with traced() as tr:
        assert raw_dio(dev, x, lengths, f0, cand, score) == 0
    assert tr.names == DIO_KERNELS, tr.names
    assert bool((f0[:, F:] == -7.0).all())                                     # spare columns keep their sentinel
    check_rows(BATCH, f0[:, :F], cand, score, 'batch, raw ABI')
    g0, gc, gs = P.dio(x, lengths=lengths, return_candidates=True)
    assert g0.shape == (B, F) and gc.shape == gs.shape == (B, nb, F) and g0.dtype == torch.float32
    assert bits_equal(g0, f0[:, :F]) and bits_equal(gc, cand) and bits_equal(gs, score)
    assert bits_equal(P.dio(x, lengths=lengths), g0)                           # a second call, without the candidates
    assert bits_equal(P.dio(x[:, None], lengths=lengths), g0[:, None])         # [B, 1, T]


def test_dio_dense_row_without_lengths_and_a_1d_input(dev):
    P = pkg()
    x = torch.from_numpy(R.waveform('glide8000').copy()).to(dev)
    g0, gc, gs = P.dio(x[None], return_candidates=True)
    check_rows(('glide8000',), g0, gc, gs, 'one dense row')
    h0, hc, hs = P.dio(x, return_candidates=True)
    assert h0.shape == (101,) and hc.shape == (7, 101)
    assert bits_equal(h0, g0[0]) and bits_equal(hc, gc[0]) and bits_equal(hs, gs[0])


DEGENERATE = ('zeros', 'short', 'row1500', 'step', 'lastframe', 'tile-1', 'tile+1', 'ev-1', 'ev+1')


def test_dio_degenerate_rows(dev):
    P = pkg()
    x, lengths = padded(dev, DEGENERATE)
    f0, cand, score = P.dio(x, lengths=lengths, return_candidates=True)
    check_rows(DEGENERATE, f0, cand, score, 'degenerate rows')
    assert bool((f0[:3] == 0).all()) and bool((f0[3] > 0).any())
    assert len(R.waveform('lastframe')) % R.HOP == 1 and len(R.waveform('tile-1')) == 4095 and len(R.waveform('tile+1')) == 4097
    assert len(R.waveform('ev-1')) == 4 * 1022 - 1 and len(R.waveform('ev+1')) == 4 * 1022 + 1
    # len = 0: nothing is read, everything is zero
    z = torch.full((2, 4000), NAN, device=dev)
    z[1] = torch.from_numpy(R.waveform('glide4000').copy()).to(dev)
    f0, cand, score = P.dio(z, lengths=torch.tensor([0, 4000], device=dev), return_candidates=True)
    assert bool((f0[0] == 0).all()) and bool((cand[0] == 0).all()) and bool((score[0] == R.BIG / R.EPS).all())
    check_f0(f0[1], R.dio_of('glide4000')['f0'], 'beside an empty row')
    assert P.dio(torch.zeros(2, 0, device=dev)).shape == (2, 1) and P.dio(torch.zeros(0, 400, device=dev)).shape == (0, 6)


def test_dio_second_parameter_set(dev):
    P = pkg()
    x = torch.from_numpy(R.waveform('glide24').copy()).to(dev)[None]
    p = R.P2
    with traced() as tr:
        f0, cand, score = P.dio(x, p['fs'], p['hop'], p['f0_floor'], p['f0_ceil'], p['cpo'], return_candidates=True)
    assert tr.names == DIO_KERNELS and cand.shape == (1, 14, 51)
    check_rows(('glide24',), f0, cand, score, 'fs 24000, hop 120, 71..800 Hz, 4 per octave')
    assert int((f0 > 0).sum()) >= 40
    with pytest.raises(ValueError, match='dio'):
        P.dio(x, 16000, 80, 50.0, 500.0, 5.0)                                  # 17 bands: TDVC_EUNSUPPORTED as ValueError
    with pytest.raises(ValueError, match='lengths'):
        P.dio(x, lengths=torch.tensor([1, 2], device=dev))
    with pytest.raises(ValueError, match='dio'):
        P.dio(torch.zeros(2, 2, 64, device=dev))
    with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
        P.dio(torch.zeros(2, 640))


# ------------------------------------------------------------------------------------------------------------ stonemask
def sm_check(got, want, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    assert np.array_equal(got > 0, want > 0) and (got[want == 0] == 0).all(), what
    v = want > 0
    ratio = np.abs(got - want)[v] / (BAR * want[v])
    assert (ratio <= 1).all(), (what, float(ratio.max()), np.nonzero(ratio > 1)[0][:8])
    return float(ratio.max())


def test_stonemask_every_fft_size_special_values_and_clamped_windows(dev):
    """f = 500, 250, 120, 60, 41 Hz give N = 256, 512, 1024, 2048, 4096 (half = 49 .. 586); the first and last frames of the row have
    windows clamped at its ends (at 41 Hz every frame within 586 samples of one). Measured worst error 0.235 of the bar."""
    P = pkg()
    name = 'glide8000'
    x = torch.from_numpy(R.waveform(name).copy()).to(dev)
    F = 101
    rng = np.random.default_rng(4)
    track = rng.choice(np.array([500.0, 250.0, 120.0, 60.0, 41.0], np.float32), F)
    track[:5] = [500.0, 250.0, 120.0, 60.0, 41.0]
    track[-5:] = [41.0, 60.0, 120.0, 250.0, 500.0]
    track[10:18] = [0.0, 40.0, R.FS / 12 + 1, NAN, np.inf, -100.0, 40.001, 1333.0]
    sizes = {2 ** (2 + int(np.log2(2 * int(1.5 * R.FS / f + 1) + 1))) for f in (500.0, 250.0, 120.0, 60.0, 41.0)}
    assert sizes == {256, 512, 1024, 2048, 4096}
    want = R.stonemask(R.waveform(name), track.astype(np.float64))
    assert (want[10:16] == 0).all() and (want[16:18] > 0).all()
    with traced() as tr:
        got = P.stonemask(x, torch.from_numpy(track).to(dev))
    assert tr.names == {'stonemask_kernel'} and got.shape == (F,) and got.dtype == torch.float32
    worst = sm_check(got, want, 'constructed track')
    # the true track of the glide, 30 % and 5 % off, through a strided view and a padded row with lengths
    base = R.world_of(name)[1]
    wide = torch.full((3, 2 * F), -3.0, device=dev)
    for b, m in enumerate((1.3, 1.05, 0.7)):
        wide[b, ::2] = torch.from_numpy((base * m).astype(np.float32)).to(dev)
    xp, lengths = padded(dev, (name, name, name))
    got3 = P.stonemask(xp, wide[:, ::2], lengths=lengths)
    for b, m in enumerate((1.3, 1.05, 0.7)):
        t32 = (base * m).astype(np.float32).astype(np.float64)
        want_b = R.stonemask(R.waveform(name), t32)
        worst = max(worst, sm_check(got3[b], want_b, f'track x {m}'))
        if m != 1.05:
            assert ((want_b == t32) | (np.abs(want_b - t32) <= 0.2 * t32)).all()
    print(f'\nstonemask: worst error over 4 * 2^-24 relative {worst:.3f}')
    assert bits_equal(P.stonemask(xp, wide[:, ::2], lengths=lengths), got3)
    # in place through the raw ABI: f0_out may be f0_in
    lib = P._lib.lib()
    buf = torch.from_numpy(track).to(dev).clone()
    assert lib.tdvc_stonemask(x.data_ptr(), 8000, 1, None, 8000, buf.data_ptr(), F, 1, 1, F, R.HOP, R.FS, buf.data_ptr(), F,
                              torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    assert bits_equal(buf, got)
    with pytest.raises(ValueError, match='stonemask'):
        P.stonemask(xp, wide[:2, ::2])
    assert P.stonemask(x, torch.zeros(0, device=dev)).shape == (0,)


# ------------------------------------------------------------------------------------------------------------ world_f0, mcd
WORLD_BATCHES = (('glide4000', 'glide8000', 'glide16040'), ('lastframe', 'tile-1', 'tile+1'))


@pytest.mark.parametrize('names', WORLD_BATCHES + (('glide24',),))
def test_world_f0_end_to_end(dev, names):
    """Measured on an MI355X: no frame excepted (module docstring)."""
    P = pkg()
    x, lengths = padded(dev, names)
    p = R.params(names[0])
    kw = dict(f0_floor=R.P2['f0_floor'], f0_ceil=R.P2['f0_ceil'], channels_in_octave=R.P2['cpo']) if names[0] == 'glide24' else {}
    got = P.world_f0(x, p['fs'], p['hop'], lengths=lengths, **kw)
    d_dev = P.dio(x, p['fs'], p['hop'], lengths=lengths, **kw).cpu().numpy()
    assert bits_equal(P.world_f0(x, p['fs'], p['hop'], lengths=lengths, **kw), got)
    voiced = excepted = 0
    worst = 0.0
    for b, n in enumerate(names):
        want, d_ref = R.world_of(n)
        g = got[b].cpu().numpy().astype(np.float64)
        assert (g[len(want):] == 0).all()
        g = g[:len(want)]
        assert np.array_equal(g > 0, want > 0), n
        v = want > 0
        ratio = np.zeros(len(want))
        ratio[v] = np.abs(g - want)[v] / (BAR * want[v])
        over = np.nonzero(ratio > 1)[0]
        if len(over):                                                          # only where the fp32 DIO values differ and the reference moves too
            dd = d_dev[b, :len(want)].astype(np.float64)
            moved = R.stonemask(R.waveform(n), dd, p['fs'], p['hop'])
            for i in over:
                assert dd[i] != d_ref[i] and abs(dd[i] - d_ref[i]) <= 2.0 ** -23 * d_ref[i] * 1.0000001, (n, i)
                assert abs(moved[i] - want[i]) > BAR * want[i] and abs(g[i] - moved[i]) <= BAR * moved[i], (n, i)
        voiced += int(v.sum()); excepted += len(over)
        worst = max(worst, float(ratio[ratio <= 1].max()))
    print(f'\nworld_f0 {names}: {voiced} voiced frames, {excepted} excepted, worst error over 4 * 2^-24 relative {worst:.3f}')
    assert voiced > 0 and excepted <= 0.01 * voiced


def mcd_pair(dev):
    a, b = R.waveform('glide8000'), R.waveform('glide16040')[4000:12000]
    s = R.waveform('step')
    test = torch.from_numpy(np.stack([a, s])).to(dev)[:, None]
    ref = torch.from_numpy(np.stack([b, a])).to(dev)[:, None]
    return test, ref, torch.tensor([8000, 7000], device=dev), torch.tensor([7500, 8000], device=dev)


def test_mcd_with_dio_is_mcd_with_world_f0_tracks(dev):
    P = pkg()
    test, ref, tl, rl = mcd_pair(dev)
    kw = dict(envelope='cheaptrick', align='fastdtw')
    auto = P.mcd(test, ref, tl, rl, f0_method='dio', **kw)
    ft, fr = P.world_f0(test[:, 0], lengths=tl), P.world_f0(ref[:, 0], lengths=rl)
    given = P.mcd(test, ref, tl, rl, f0_test=ft, f0_ref=fr, **kw)
    assert set(auto) == set(given) and all(bits_equal(auto[k], given[k]) for k in auto)
    assert bool((auto['n_test'] > 10).all()) and bool((auto['mcd'] > 0).all()) and bool(torch.isfinite(auto['f0_ratio']).all())
    print('\nmcd(f0_method=dio, cheaptrick, fastdtw):', {k: [round(float(x), 4) for x in v] for k, v in auto.items()})
    plain, yin = P.mcd(test, ref, tl, rl), P.mcd(test, ref, tl, rl, f0_method='yin')
    assert all(bits_equal(plain[k], yin[k]) for k in plain)
    assert not bits_equal(P.mcd(test, ref, tl, rl, f0_method='dio')['mcd'], plain['mcd'])
    with pytest.raises(ValueError, match='f0_method'):
        P.mcd(test, ref, f0_method='harvest')


def test_mcd_with_dio_under_graph_capture(dev):
    P = pkg()
    test, ref, tl, rl = mcd_pair(dev)
    call = lambda: P.mcd(test, ref, tl, rl, f0_method='dio', envelope='cheaptrick', align='fastdtw')
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call()                                                                 # warm-up
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = call()
    graph.replay()
    torch.cuda.synchronize(dev)
    eager = call()
    assert all(bits_equal(r[k], eager[k]) for k in r) and float(r['mcd'][0]) > 0
    first = {k: v.clone() for k, v in r.items()}
    graph.replay()
    torch.cuda.synchronize(dev)
    assert all(bits_equal(r[k], first[k]) for k in r)


def test_two_calls_are_bit_identical(dev):
    P = pkg()
    x, lengths = padded(dev, BATCH)
    a, b = P.dio(x, lengths=lengths, return_candidates=True), P.dio(x, lengths=lengths, return_candidates=True)
    assert all(bits_equal(u, v) for u, v in zip(a, b))
    assert bits_equal(P.stonemask(x, a[0], lengths=lengths), P.stonemask(x, a[0], lengths=lengths))
    assert bits_equal(P.world_f0(x, lengths=lengths), P.world_f0(x, lengths=lengths))
    assert bits_equal(P.world_f0(x, lengths=lengths), P.stonemask(x, a[0], lengths=lengths))
