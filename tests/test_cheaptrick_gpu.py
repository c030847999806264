"""GPU: WORLD's CheapTrick spectral envelope on the device (td-vc-gan_amd/evaluate.py cheaptrick, mel_cepstrum / mcd with
envelope='cheaptrick'; csrc/eval_cheaptrick.hip) through the package and through the raw C ABI, against the float64 restatement
tests/cheaptrick_ref.py, which tests/test_cheaptrick_cpu.py pins to independent statements. pyworld is not available: nothing here
is a parity test against WORLD.

1. Element by element at n_fft 512, 1024 and 2048 on cheaptrick_ref.case: |env - env64| <= 4 * 2^-24 * env64 (one fp32 rounding of a
   float64 evaluation, the project's factor 4) and |mc - mc64| <= 4 * 2^-24 * max |mc64 of that frame| (the bar of test_mcd_gpu.py).
   The inputs hold the F0 values 0, NaN, negative, inf, just below and just above 3 fs/(N - 3) (the window nearly fills N), fs/4 and
   just above it, 55, 140, 480 (1.5 fs/f = 50 exactly), 384 (62.5: the tie), 500; frames on the first and on the last sample and
   three past the row end; a row cut short by `lengths` with NaN in the spare samples. env only, mc only and both give the same
   bits, as do strided views and a second call. The float64 reference itself is within 2^-24 / 4 of a long double evaluation on
   these inputs (test_cheaptrick_cpu.py), which is what makes the bar meaningful.
   Measured on an MI355X (printed by the tests, run with -s), worst error over its bar:
       n_fft   env     mc
       512     0.249   0.226
       1024    0.248   0.239
       2048    0.250   0.231
   0.25 of the bar is 2^-24: the one rounding to fp32 and nothing else.
2. The fused mc against sp2mc(cheaptrick(...)): both within the bar of float64.
3. The recovery property on the device output, with the bars of the CPU test. Measured: log env peak-to-peak 8.606e-04 at 100 Hz and
   3.345e-04 at 250 Hz, 7.9e-03 / 9.1e-03 across the frame positions: the reference's figures.
4. mcd(envelope='cheaptrick') with given F0 tracks against cheaptrick_ref -> freqt -> dtw_ref: equal path length, and
   |cost - C*| <= (N + M - 1) e with e the error of one local distance: both frames within d = 4 * 2^-24 * max |mc64| per element give
   2 sqrt(D) d, plus the fp32 evaluation of the distance, (D + 2) 2^-24 relative (test_mcd_gpu.py). Measured: C* 9.115044 and
   9.711447, |cost - C*| 8.2e-08 and 2.0e-07, bounds 1.0e-03 and 1.1e-03, paths of 50 and 51 cells. The default envelope returns the
   bits of a call without the keyword; the whole call is captured into a graph.
5. Refusals with the documented code before any launch; B * F == 0 is a no-op.
"""
import functools

import numpy as np
import pytest
import torch

import cheaptrick_ref as R
import dtw_ref as DR
from common import pkg, traced

pytestmark = pytest.mark.gpu
NAN = float('nan')
EINVAL, EUNSUPPORTED = -1, -4
ORDER, ALPHA = 24, 0.42
BAR = 4 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def mc_ref(n_fft):
    mc = R.mc_from_c(R.case_ref(n_fft)[1], ORDER, ALPHA)
    mc.setflags(write=False)
    return mc


def device_case(dev, n_fft):
    """The case on the device: signal [2, 1, T] with NaN at and past lengths[b], f0 [2, F], lengths int32 [2]."""
    k = R.case(n_fft)
    x = k['x'].copy()
    for b, n in enumerate(k['lengths']):
        x[b, n:] = np.nan
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return t(x)[:, None], t(k['f0']), t(k['lengths'])


def raw(dev, sig, f0, lengths, *, n_fft, env, mc, G, order=ORDER, B=None, F=None, T=None, hop=R.HOP, fs=R.FS, q1=-0.15, floor=R.FLOOR,
        s_strides=None, f_strides=None, nulls=()):
    """tdvc_cheaptrick through ctypes; returns the status code."""
    lib = pkg()._lib.lib()
    t = dict(sig=sig, f0=f0, lengths=lengths, env=env, mc=mc, G=G)
    ptr = lambda name: None if (name in nulls or t[name] is None) else t[name].data_ptr()
    s_bs, s_ts = (sig.stride(0), sig.stride(-1)) if s_strides is None else s_strides
    f_bs, f_fs = f0.stride() if f_strides is None else f_strides
    rc = lib.tdvc_cheaptrick(ptr('sig'), s_bs, s_ts, ptr('lengths'), sig.shape[-1] if T is None else T, ptr('f0'), f_bs, f_fs,
                             f0.shape[0] if B is None else B, f0.shape[1] if F is None else F, hop, fs, n_fft, q1, floor, ptr('G'), order,
                             ptr('env'), ptr('mc'), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


def check_env(env, want):
    got = env.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / (BAR * want)
    assert (ratio <= 1).all(), (float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max())


def check_mc(mc, want):
    got = mc.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / (BAR * np.abs(want).max(-1, keepdims=True))
    assert (ratio <= 1).all(), (float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize('n_fft', (512, 1024, 2048))
def test_env_and_mc_equal_float64_to_one_rounding(dev, n_fft):
    E = pkg().evaluate
    sig, f0, lengths = device_case(dev, n_fft)
    env64, _ = R.case_ref(n_fft)
    with traced() as tr:
        env = E.cheaptrick(sig, f0, n_fft=n_fft, lengths=lengths)
    assert tr.names == {f'cheaptrick_kernel<{n_fft}>'}, tr.names
    assert env.shape == (2, R.F_CASE, n_fft // 2 + 1) and env.dtype == torch.float32
    mc, nfr = E.mel_cepstrum(sig, n_fft=n_fft, hop=R.HOP, order=ORDER, alpha=ALPHA, lengths=lengths, envelope='cheaptrick', f0=f0)
    assert mc.shape == (2, R.F_CASE, ORDER + 1) and mc.dtype == torch.float32
    assert nfr.tolist() == [min(1 + int(n) // R.HOP, R.F_CASE) for n in R.case(n_fft)['lengths']] and nfr.dtype == torch.int32
    r_env, r_mc = check_env(env, env64), check_mc(mc, mc_ref(n_fft))
    print(f'\ncheaptrick n_fft {n_fft}: worst |env - env64| / (4 * 2^-24 env64) {r_env:.3f}, worst mc error over its bar {r_mc:.3f}')
    # env only, mc only and both: the same bits; a second call: the same bits
    G = torch.tensor(E.cheaptrick_mc_matrix(n_fft, ORDER, ALPHA), device=dev)
    env2, mc2 = torch.full_like(env, -7.0), torch.full_like(mc, -7.0)
    assert raw(dev, sig, f0, lengths, n_fft=n_fft, env=env2, mc=mc2, G=G) == 0
    assert torch.equal(env2, env) and torch.equal(mc2, mc)
    assert torch.equal(E.cheaptrick(sig, f0, n_fft=n_fft, lengths=lengths), env)
    # the frames past the row end see one repeated sample: nothing is left after the mean removal, the floor decides
    flat = np.float32(R.FLOOR + R.EPS)
    assert np.allclose(env[0, [31, 33]].cpu().numpy(), flat, rtol=1e-6, atol=0)      # (frame 32 has the longest window: it reaches back into the row)


def test_strided_signal_and_f0_views(dev):
    E = pkg().evaluate
    n_fft = 1024
    sig, f0, lengths = device_case(dev, n_fft)
    B, _, T = sig.shape
    want = E.cheaptrick(sig, f0, n_fft=n_fft, lengths=lengths)
    ws = torch.full((2 * B, 1, 3 * T + 5), NAN, device=dev)
    ws[::2, :, 2:2 + 3 * T:3] = sig
    wf = torch.full((B, 2 * R.F_CASE + 1, 2), NAN, device=dev)
    wf[:, 1::2, 1] = f0
    vs, vf = ws[::2, :, 2:2 + 3 * T:3], wf[:, 1::2, 1]
    assert vs.stride() == (2 * (3 * T + 5), 3 * T + 5, 3) and vf.stride() == (2 * (2 * R.F_CASE + 1), 4)
    assert torch.equal(E.cheaptrick(vs, vf, n_fft=n_fft, lengths=lengths), want)
    mc = E.mel_cepstrum(sig, n_fft=n_fft, envelope='cheaptrick', f0=f0, lengths=lengths)[0]
    assert torch.equal(E.mel_cepstrum(vs, n_fft=n_fft, envelope='cheaptrick', f0=vf, lengths=lengths)[0], mc)
    # without lengths the whole row counts: the reference on the untruncated rows
    full = torch.from_numpy(R.case(n_fft)['x'].copy()).to(dev)[:, None]
    check_env(E.cheaptrick(full, f0, n_fft=n_fft), R.case_ref(n_fft, False)[0])


def test_fused_mc_and_sp2mc_of_the_envelope_both_within_the_bar(dev):
    E = pkg().evaluate
    n_fft = 1024
    sig, f0, lengths = device_case(dev, n_fft)
    fused = E.mel_cepstrum(sig, n_fft=n_fft, order=ORDER, alpha=ALPHA, envelope='cheaptrick', f0=f0, lengths=lengths)[0]
    two = E.sp2mc(E.cheaptrick(sig, f0, n_fft=n_fft, lengths=lengths), ORDER, ALPHA, floor=1e-30)
    a, b = check_mc(fused, mc_ref(n_fft)), check_mc(two, mc_ref(n_fft))
    print(f'\nmc error over its bar: fused {a:.3f}, sp2mc of the fp32 envelope {b:.3f}')


def test_f0_from_yin_when_none_is_given(dev):
    P = pkg()
    n_fft = 1024
    sig = torch.from_numpy(R.case(n_fft)['x'].copy()).to(dev)[:, None]
    f0 = P.yin_f0(sig[:, 0], R.FS, pitch_min=50, pitch_max=500, frame_stride=R.HOP / R.FS)
    mc = P.mel_cepstrum(sig, n_fft=n_fft, envelope='cheaptrick')
    assert mc.shape == (2, f0.shape[1], 25) and int((f0 > 0).sum()) > 20
    assert torch.equal(mc, P.mel_cepstrum(sig, n_fft=n_fft, envelope='cheaptrick', f0=f0))


# ------------------------------------------------------------------------------------------------------------ recovery
@pytest.mark.parametrize('f0', R.RECOVERY_F0)
def test_recovery_of_a_flat_harmonic_spectrum_on_the_device(dev, f0):
    E = pkg().evaluate
    k = R.recovery_case(f0)
    F = int(k['frames'][-1]) + 1
    sig = torch.from_numpy(k['x'].astype(np.float32)).to(dev)[None, None]
    env = E.cheaptrick(sig, torch.full((1, F), f0, device=dev), sample_rate=k['fs'], n_fft=k['n_fft'], hop=k['hop'])
    le = np.log(env[0, k['frames']].cpu().numpy().astype(np.float64)[:, k['band']])
    flat, across = np.ptp(le, axis=1).max(), np.ptp(le, axis=0).max()
    print(f'\nrecovery on the device f0 {f0}: log env peak-to-peak {flat:.3e}, across positions {across:.2e}')
    assert flat <= 4 * R.RECOVERY_FLATNESS[f0] and across < 0.06


# ------------------------------------------------------------------------------------------------------------ mcd
@functools.lru_cache(maxsize=None)
def mcd_case():
    """Two pairs of short voiced signals with given F0 tracks (a few unvoiced frames in each) and the float64 pipeline's results."""
    rng = np.random.default_rng(21)
    T, n_fft = 4000, 1024
    F = T // R.HOP
    pitch = ((130.0, 170.0), (220.0, 105.0))
    x = np.stack([[R.voiced(rng, T, p) for p in pair] for pair in pitch]).astype(np.float32)      # [pair, side, T]
    f0 = np.stack([[np.full(F, p, np.float32) for p in pair] for pair in pitch])
    f0[0, 0, :3] = 0.0
    f0[0, 1, 20:24] = 0.0
    f0[1, 0, -5:] = 0.0
    want = []
    for b in range(2):
        mcs = []
        for side in range(2):
            _, c = R.cheaptrick(x[b, side], f0[b, side], R.FS, n_fft, R.HOP)
            mcs.append(R.mc_from_c(c, ORDER, ALPHA)[f0[b, side] > 0])
        w = DR.dtw(mcs[0], mcs[1], 'l2')
        d = DR.distance(mcs[0], mcs[1], 'l2')
        delta = BAR * max(np.abs(mcs[0]).max(), np.abs(mcs[1]).max())
        e_cell = 2 * np.sqrt(ORDER + 1) * delta
        e_cell += (ORDER + 3) * 2.0 ** -24 * (d.max() + e_cell)
        want.append(dict(cost=w['cost'], length=w['length'], n=(len(mcs[0]), len(mcs[1])), bound=(len(mcs[0]) + len(mcs[1]) - 1) * e_cell))
    return x, f0, want


def test_mcd_with_the_cheaptrick_envelope_against_the_float64_pipeline(dev):
    P = pkg()
    x, f0, want = mcd_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    test, ref, ft, fr = t(x[:, 0])[:, None], t(x[:, 1])[:, None], t(f0[:, 0]), t(f0[:, 1])
    with traced() as tr:
        r = P.mcd(test, ref, f0_test=ft, f0_ref=fr, envelope='cheaptrick')
    assert 'cheaptrick_kernel<1024>' in tr.names
    for b, w in enumerate(want):
        cost = float(r['mcd'][b] * r['path_len'][b])
        print(f'\nmcd pair {b}: C* {w["cost"]:.6f}, |cost - C*| {abs(cost - w["cost"]):.3e}, bound {w["bound"]:.3e}, path {int(r["path_len"][b])}')
        assert (int(r['n_test'][b]), int(r['n_ref'][b])) == w['n']
        assert int(r['path_len'][b]) == w['length']
        assert abs(cost - w['cost']) <= w['bound']
    # the default envelope: the bits of a call without the keyword
    plain, kw = P.mcd(test, ref, f0_test=ft, f0_ref=fr), P.mcd(test, ref, f0_test=ft, f0_ref=fr, envelope='stft')
    assert all(torch.equal(plain[k].nan_to_num(-1.0), kw[k].nan_to_num(-1.0)) for k in plain)
    assert not torch.equal(plain['mcd'], r['mcd'])
    # the F0 track from YIN serves the envelope and the voicing
    auto = P.mcd(test, ref, envelope='cheaptrick')
    assert all(v.shape == (2,) and v.dtype == torch.float64 for v in auto.values()) and bool((auto['n_test'] > 10).all())


def test_mcd_with_the_cheaptrick_envelope_under_graph_capture(dev):
    P = pkg()
    x, _, _ = mcd_case()
    test, ref = torch.from_numpy(x[:1, 0].copy()).to(dev)[:, None], torch.from_numpy(x[:1, 1].copy()).to(dev)[:, None]
    tl = torch.tensor([x.shape[-1]], device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        P.mcd(test, ref, tl, tl, envelope='cheaptrick')                           # warm-up
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = P.mcd(test, ref, tl, tl, envelope='cheaptrick')
    graph.replay()
    torch.cuda.synchronize(dev)
    eager = P.mcd(test, ref, tl, tl, envelope='cheaptrick')
    assert all(torch.equal(r[k], eager[k]) for k in r) and float(r['mcd'][0]) > 0
    ref.copy_(test)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert float(r['mcd'][0]) == 0.0


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch(dev):
    E = pkg().evaluate
    lib = pkg()._lib.lib()
    n_fft = 512
    sig, f0, lengths = device_case(dev, n_fft)
    G = torch.tensor(E.cheaptrick_mc_matrix(n_fft, ORDER, ALPHA), device=dev)
    env = torch.full((2, R.F_CASE, n_fft // 2 + 1), -7.0, device=dev)
    mc = torch.full((2, R.F_CASE, ORDER + 1), -7.0, device=dev)
    base = dict(n_fft=n_fft, env=env, mc=mc, G=G)
    s_bs, f_bs = sig.stride(0), f0.stride(0)
    cases = [
        (dict(n_fft=256), EUNSUPPORTED), (dict(n_fft=1000), EUNSUPPORTED), (dict(n_fft=4096), EUNSUPPORTED), (dict(n_fft=0), EUNSUPPORTED),
        (dict(nulls=('env', 'mc')), EINVAL), (dict(nulls=('G',)), EINVAL), (dict(order=n_fft // 2 + 1), EINVAL), (dict(order=-1), EINVAL),
        (dict(floor=0.0), EINVAL), (dict(floor=-1e-16), EINVAL), (dict(floor=NAN), EINVAL), (dict(floor=float('inf')), EINVAL),
        (dict(hop=0), EINVAL), (dict(hop=-80), EINVAL), (dict(fs=0), EINVAL), (dict(fs=-16000), EINVAL), (dict(q1=NAN), EINVAL),
        (dict(fs=1999), EINVAL),                                                  # 500 Hz above fs/4
        (dict(fs=85000), EINVAL),                                                 # 500 Hz under 3 fs/(N - 3) = 501 Hz
        (dict(s_strides=(-1, 1)), EINVAL), (dict(s_strides=(s_bs, -1)), EINVAL), (dict(f_strides=(-1, 1)), EINVAL), (dict(f_strides=(f_bs, -1)), EINVAL),
        (dict(B=-1), EINVAL), (dict(F=-1), EINVAL), (dict(T=-1), EINVAL), (dict(nulls=('sig',)), EINVAL), (dict(nulls=('f0',)), EINVAL),
    ]
    with traced() as tr:
        for kw, want in cases:
            rc = raw(dev, sig, f0, lengths, **{**base, **kw})
            assert rc == want, (kw, rc, want)
            assert lib.tdvc_last_error() and bool((env == -7).all()) and bool((mc == -7).all()), kw
        assert raw(dev, sig, f0, lengths, **{**base, 'B': 0}) == 0 and raw(dev, sig, f0, lengths, **{**base, 'F': 0}) == 0      # no-ops
        assert raw(dev, sig, f0, lengths, **{**base, 'B': 0, 'nulls': ('sig', 'f0')}) == 0
        assert bool((env == -7).all()) and bool((mc == -7).all())
    assert tr.names == set()
    assert raw(dev, sig, f0, lengths, **{**base, 'fs': 2000}) == 0                # 500 Hz = fs/4 is inside
    assert raw(dev, sig, f0, lengths, n_fft=n_fft, env=env, mc=None, G=None) == 0      # env alone needs no matrix
    assert raw(dev, sig, f0, lengths, **{**base, 'order': 0, 'nulls': ('env',)}) == 0
    check_env(env, R.case_ref(n_fft)[0])                                           # and the same buffers do work


def test_python_refusals(dev):
    P = pkg()
    E = P.evaluate
    sig, f0 = torch.zeros(2, 1, 4000, device=dev), torch.zeros(2, 50, device=dev)
    with pytest.raises(RuntimeError):
        E.cheaptrick(sig.cpu(), f0.cpu())                                         # there is no CPU fallback
    with pytest.raises(ValueError):
        E.cheaptrick(sig, f0, n_fft=256)
    with pytest.raises(ValueError):
        E.cheaptrick(sig[:, 0], f0)
    with pytest.raises(ValueError):
        E.cheaptrick(sig, f0[:1])
    with pytest.raises(ValueError):
        E.cheaptrick(sig, f0, lengths=torch.tensor([4000], device=dev))
    with pytest.raises(RuntimeError):
        E.cheaptrick(sig, f0, floor=0.0)                                          # TDVC_EINVAL from the library
    with pytest.raises(ValueError):
        E.mel_cepstrum(sig, envelope='world')
    with pytest.raises(ValueError):
        P.mcd(sig, sig, envelope='world')
    assert P.cheaptrick is E.cheaptrick and P.cheaptrick_mc_matrix is E.cheaptrick_mc_matrix
    assert np.allclose(E.cheaptrick(sig, f0).cpu().numpy(), np.float32(R.FLOOR + R.EPS), rtol=1e-6, atol=0)      # digital silence: the floor
