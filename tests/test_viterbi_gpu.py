"""GPU: tdvc_viterbi_path (csrc/pitch_viterbi.hip) through pitch.viterbi_path / yin_f0 / track_f0 / infer.convert_audio and through
the raw C ABI, against the dense float64 decoder of tests/viterbi_ref.py.

1. Exact lattices: x, prior, logw and jump are multiples of 1/8 below 64 in magnitude and scale is 1 or 2, so every fp32 operation
   of the kernel is exact and its path must equal the float64 path on EVERY frame, ties included (the coarse lattices are full
   of ties). The shapes cover every kernel instance: 4, 2 and 1 lanes per state (n <= 256, <= 512, above), the band table in LDS
   and in the workspace (n233w200, n1023), bands clipped at both ends, W = 1, F = 1, 2 and 4096.
2. Real lattices: the device's own fp32 CMDF; the device path and the float64-optimal path of that same fp32 lattice, both scored
   in float64, may differ by at most F * 2^-21 * M, M = 100 max(cmdf) + octave_cost log2(lag_max / lag_min) + jump_cost: every
   renormalised score is bounded by M and each frame rounds a few times on each of the two paths.
3. The decoded track of yin_f0 / track_f0 / convert_audio.  4. Refusals, before any launch.

Measured on an MI355X (printed by the tests, run with -s): every exact lattice identical to the float64 path; on the real lattices
    case      B x F x n        float64 score gap   bound       frames off the float64-optimal path
    speech    2 x 63 x 233     0                   6.210e-03   0 of 126
    odd       3 x 26 x 279     0                   2.578e-03   0 of 78
    default   2 x 63 x 799     0                   8.066e-03   0 of 126
    long      1 x 1120 x 233   0                   1.207e-01   0 of 1120
    hard      1 x 500 x 233    0                   6.198e-02   0 of 500
and on the hard case the per-frame tracker makes 16 errors above 100 cents over 389 voiced frames, the decoded track none.
"""
import functools
import math

import numpy as np
import pytest
import torch

import viterbi_ref as VR
import yin_ref as YR
from common import build_models, pkg

pytestmark = pytest.mark.gpu
SR, THR = 16000, 0.1
OCTAVE_COST, JUMP_COST = 1.0, 16.0
INF = math.inf


# ------------------------------------------------------------------------------------------------------------ exact lattices
def eighths(rng, shape, lo, hi):
    """Multiples of 1/8 in [lo, hi]."""
    return (rng.integers(int(lo * 8), int(hi * 8) + 1, size=shape) / 8.0).astype(np.float32)


#        name          n     W    F   jump  scale prior  coarse
EXACT = {
    'n3':        (3,    3,   7,   3.5,   1.0, True,  False),
    'n63':       (63,   9,   9,   20.0,  2.0, True,  False),
    'n64':       (64,   17,  9,   12.5,  1.0, True,  True),
    'n65':       (65,   33,  9,   40.0,  2.0, True,  False),
    'n233':      (233,  64,  9,   16.0,  1.0, True,  False),
    'n233w128':  (233,  128, 5,   24.0,  1.0, True,  False),      # 123 KB of table in LDS: past the 64 KB a block gets by default
    'n233w200':  (233,  200, 5,   16.0,  2.0, True,  True),       # 4 lanes per state, table in the workspace
    'n257':      (257,  40,  9,   30.0,  1.0, True,  True),       # 2 lanes per state
    'n600':      (600,  16,  6,   25.0,  2.0, True,  False),      # 1 lane per state, table in LDS
    'n1023':     (1023, 248, 5,   16.0,  1.0, True,  False),      # the YIN kernel's own limit, table in the workspace
    'w1':        (65,   1,   8,   INF,   1.0, True,  False),      # self transitions only
    'w1_floor':  (65,   1,   8,   6.25,  2.0, True,  True),
    'F1':        (65,   9,   1,   10.0,  1.0, True,  True),
    'F2':        (65,   9,   2,   10.0,  2.0, True,  True),
    'F4096':     (65,   9,   4096, 10.0, 2.0, True,  False),      # 4095 frames of the floor shortcut, which holds only under the renormalisation
    'jump_inf':  (129,  11,  9,   INF,   1.0, True,  True),
    'no_prior':  (129,  11,  9,   8.0,   2.0, False, True),
    'w_eq_n':    (40,   40,  6,   5.0,   1.0, True,  True),       # the band is the whole state axis: lo = 0 everywhere
}
B_EXACT = 3


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """dict(x [B, F, n], prior, logw, lo, jump, scale, want [B, F]): built once, the float64 path included."""
    n, W, F, jump, scale, has_prior, coarse = EXACT[name]
    rng = np.random.default_rng(sorted(EXACT).index(name) + 100)
    lim = 1.0 if coarse else 63.0
    x = eighths(rng, (B_EXACT, F, n), 32.0 if name == 'F4096' else -lim, lim)
    prior = eighths(rng, n, -lim, lim) if has_prior else None
    centre = np.arange(n) + rng.integers(-2, 3, size=n)
    lo = np.clip(centre - W // 2, 0, n - W).astype(np.int32)      # clipped at both ends of the state axis
    logw = eighths(rng, (n, W), -lim, 0.0 if not coarse else 0.5)
    logw[rng.random((n, W)) < 0.15] = -np.inf                      # unused slots
    if not np.isfinite(jump):
        self_k = np.clip(np.arange(n) - lo, 0, W - 1)              # one finite predecessor per state: no state is cut off
        logw[np.arange(n), self_k] = np.where(np.isfinite(logw[np.arange(n), self_k]), logw[np.arange(n), self_k], 0.0)
    want = VR.decode(x, logw, lo, scale, prior, jump)
    return dict(x=x, prior=prior, logw=logw, lo=lo, jump=jump, scale=scale, want=want)


def device_path(c, dev, x=None):
    Pt = pkg().pitch
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    p = Pt.viterbi_path(t(c['x']) if x is None else x, t(c['logw']), t(c['lo']), scale=c['scale'], prior=t(c['prior']), jump=c['jump'])
    torch.cuda.synchronize()
    return p


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_lattice_equals_float64_path(dev, name):
    c = exact_case(name)
    got = device_path(c, dev)
    assert got.dtype == torch.int64 and got.shape == c['want'].shape
    diff = int((got.cpu().numpy() != c['want']).sum())
    assert diff == 0, (name, diff, c['want'].size)
    assert torch.equal(device_path(c, dev), got)                   # two calls, the same bits


def test_all_equal_lattice_is_all_zeros(dev):
    Pt = pkg().pitch
    n, W, F = 233, 64, 17
    lo = torch.from_numpy(np.clip(np.arange(n) - W // 2, 0, n - W).astype(np.int32)).to(dev)
    for jump in (4.0, INF):
        p = Pt.viterbi_path(torch.full((B_EXACT, F, n), 1.5, device=dev), torch.zeros(n, W, device=dev), lo, jump=jump)
        assert p.shape == (B_EXACT, F) and not bool(p.any())


def test_strided_lattice_view_with_nan_in_the_spare_elements(dev):
    c = exact_case('n233')
    B, F, n = c['x'].shape
    wide = torch.full((B, F + 2, n + 5), float('nan'), device=dev)
    wide[:, 1:1 + F, 3:3 + n] = torch.from_numpy(c['x']).to(dev)
    view = wide[:, 1:1 + F, 3:3 + n]
    assert view.stride() == ((F + 2) * (n + 5), n + 5, 1) and not view.is_contiguous()
    assert np.array_equal(device_path(c, dev, x=view).cpu().numpy(), c['want'])
    assert np.array_equal(device_path(c, dev, x=view[1]).cpu().numpy(), c['want'][1])      # [F, n]
    lead = device_path(c, dev, x=torch.from_numpy(c['x']).to(dev)[:, None].expand(B, 2, F, n))
    assert lead.shape == (B, 2, F) and np.array_equal(lead[:, 1].cpu().numpy(), c['want'])


def raw_call(dev, c, path, path_bs, *, B=None, F=None, n=None, W=None, jump=None, ws='query', nulls=(), x_fs=None):
    """tdvc_viterbi_path through ctypes on device copies of case c; returns the status code."""
    L = pkg()._lib
    lib = L.lib()
    xb, xf, xn = c['x'].shape
    B, F, n = xb if B is None else B, xf if F is None else F, xn if n is None else n
    W = c['logw'].shape[1] if W is None else W
    t = {k: (None if c[k] is None else torch.from_numpy(c[k]).to(dev)) for k in ('x', 'prior', 'logw', 'lo')}
    ptr = lambda k: None if (k in nulls or t[k] is None) else t[k].data_ptr()
    if ws == 'query':
        nbytes = lib.tdvc_viterbi_workspace(max(B, 1), max(F, 1), max(min(n, 1024), 1))
        ws = (torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes)
    buf, nbytes = ws
    rc = lib.tdvc_viterbi_path(ptr('x'), F * n, n if x_fs is None else x_fs, float(c['scale']), ptr('prior'), ptr('logw'), ptr('lo'), W,
                               float(c['jump'] if jump is None else jump), B, F, n, None if 'path' in nulls else path.data_ptr(), path_bs,
                               None if buf is None else buf.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_strided_path_and_poisoned_lds(dev):
    """Path rows F + 7 apart through the C ABI, the elements between them untouched; the same call after every CU's LDS has been
    filled with NaN bit patterns: a read of LDS the kernel has not written would change the path."""
    L = pkg()._lib
    for name in ('n233', 'n65'):
        c = exact_case(name)
        B, F, n = c['x'].shape
        path = torch.full((B, F + 7), -7, dtype=torch.int32, device=dev)
        assert raw_call(dev, c, path, F + 7) == 0
        assert np.array_equal(path[:, :F].cpu().numpy(), c['want']) and bool((path[:, F:] == -7).all())
        L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream))
        again = torch.full((B, F + 7), -7, dtype=torch.int32, device=dev)
        assert raw_call(dev, c, again, F + 7) == 0
        assert torch.equal(again, path)


# ------------------------------------------------------------------------------------------------------------ real lattices
REAL = ('speech', 'odd', 'default', 'long', 'hard')


def real_signal(name):
    """(x fp32 [B, T], tau_min, tau_max, stride, pitch_min, pitch_max)"""
    if name == 'hard':
        return torch.from_numpy(VR.hard_case()[0])[None], int(SR / 500), int(SR / 60), VR.HARD_HOP, 60, 500
    t = YR.long_truth() if name == 'long' else YR.truth(name)
    s = t['meta']
    return t['x'], s['tau_min'], s['tau_max'], s['stride'], s['pitch_min'], s['pitch_max']


@functools.lru_cache(maxsize=None)
def real_case(name):
    """The device's CMDF, hard track and decoded path of one signal, and the float64-optimal path of that fp32 lattice under the
    device's own fp32 table and prior: computed once per session and left unchanged."""
    Pt = pkg().pitch
    x, tau_min, tau_max, stride, pmin, pmax = real_signal(name)
    hard, c = Pt.yin_f0(x.cuda(), SR, pmin, pmax, stride / SR, THR, return_cmdf=True)
    n = c.shape[-1]
    logw, lo = Pt.viterbi_transition(tau_min, tau_max)
    prior = torch.from_numpy(VR.octave_prior(tau_min, n, OCTAVE_COST).astype(np.float32))
    path = Pt.viterbi_path(c, logw, lo, scale=-YR.THETA, prior=prior.cuda(), jump=JUMP_COST)
    torch.cuda.synchronize()
    lw, l, pr, c64 = logw.cpu().numpy(), lo.cpu().numpy(), prior.numpy(), c.cpu().numpy().astype(np.float64)
    t = VR.dense_transition(lw, l, JUMP_COST, n)
    best = VR.decode(c64, lw, l, -YR.THETA, pr, JUMP_COST, t)
    sc = lambda p, b: VR.score(p, c64[b], lw, l, -YR.THETA, pr, JUMP_COST, t)
    gaps = [sc(best[b], b) - sc(path[b].cpu().numpy(), b) for b in range(c64.shape[0])]
    return dict(hard=hard.cpu(), cmdf=c.cpu(), path=path.cpu(), best=best, gaps=gaps, tau_min=tau_min, tau_max=tau_max, stride=stride,
                pmin=pmin, pmax=pmax, x=x)


@pytest.mark.parametrize('name', REAL)
def test_real_lattice_score_gap(dev, name):
    r = real_case(name)
    B, F, n = r['cmdf'].shape
    M = YR.THETA * float(r['cmdf'].max()) + OCTAVE_COST * math.log2((r['tau_max'] - 1) / (r['tau_min'] + 1)) + JUMP_COST
    bound = F * 2.0 ** -21 * M
    differ = int((r['path'].numpy() != r['best']).sum())
    print(f'\nviterbi {name}: B {B} F {F} n {n}: float64 score gap max {max(np.abs(r["gaps"])):.3e} (bound {bound:.3e}), '
          f'frames that differ from the float64-optimal path {differ} of {B * F}')
    assert r['path'].shape == (B, F) and int(r['path'].min()) >= 0 and int(r['path'].max()) < n
    assert max(np.abs(r['gaps'])) <= bound, (name, r['gaps'], bound)


def test_table_on_the_device_is_the_formula_rounded_once(dev):
    Pt = pkg().pitch
    for tau_min, tau_max in ((32, 266), (0, 800)):
        logw, lo = Pt.viterbi_transition(tau_min, tau_max)
        assert logw.dtype == torch.float32 and lo.dtype == torch.int32 and logw.is_cuda and lo.is_cuda
        assert Pt.viterbi_transition(tau_min, tau_max)[0] is logw              # cached per arguments and device
        ref_logw, ref_lo = VR.transition(tau_min, tau_max)
        assert np.array_equal(lo.cpu().numpy(), ref_lo)
        got, fin = logw.cpu().numpy().astype(np.float64), np.isfinite(ref_logw)
        assert np.array_equal(np.isneginf(got), ~fin)
        assert np.all(np.abs(got[fin] - ref_logw[fin]) <= 2.0 ** -24 * np.abs(ref_logw[fin]) + 2.0 ** -149)


# ------------------------------------------------------------------------------------------------------------ the decoded track
@pytest.mark.parametrize('name', ['speech', 'long', 'hard'])
def test_track_f0_viterbi(dev, name):
    P = pkg()
    r = real_case(name)
    x = r['x'][:, None].to(dev)
    B, T = x.shape[0], x.shape[-1]
    kw = dict(hop=r['stride'], sample_rate=SR, pitch_min=r['pmin'], pitch_max=r['pmax'], threshold=THR)
    plain = P.track_f0(x, **kw)
    f0 = P.track_f0(x, decoder='viterbi', **kw)
    assert f0.shape == plain.shape == (B, 1, T // r['stride'] + 1) and f0.dtype == torch.float32
    assert torch.equal(f0 == 0, plain == 0) and bool((f0 > 0).any())
    nf = r['path'].shape[-1]
    idx = torch.arange(T // r['stride'] + 1).clamp_(max=nf - 1)
    hard, path = r['hard'].to(dev), r['path'].to(dev)
    want = torch.where(hard != 0, SR / (path + (r['tau_min'] + 1)).float(), torch.zeros_like(hard))[:, idx.to(dev)]
    assert torch.equal(f0[:, 0], want)
    assert torch.equal(P.track_f0(x, decoder=None, **kw), plain) and torch.equal(P.track_f0(x, **kw), plain)
    y, c = P.yin_f0(x[:, 0], SR, r['pmin'], r['pmax'], r['stride'] / SR, THR, decoder='viterbi', return_cmdf=True)
    assert torch.equal(y, want[:, :nf]) and torch.equal(c.cpu(), r['cmdf'])
    if name == 'hard':
        true_f = torch.from_numpy(VR.hard_case()[1])[None, :f0.shape[-1]]
        v = (plain[:, 0] > 0).cpu()
        cents = lambda f: (1200 * torch.log2(f.cpu().double() / true_f)).abs()
        hard_err, dec_err = int((cents(plain[:, 0])[v] > 100).sum()), int((cents(f0[:, 0])[v] > 100).sum())
        print(f'\nhard case on the device: errors > 100 cents over {int(v.sum())} voiced frames: per-frame YIN {hard_err}, decoded {dec_err}')
        assert hard_err >= 10 and dec_err == 0


def test_silence_decodes_to_zeros(dev):
    P = pkg()
    x = YR.truth('silence')['x'][:, None].to(dev)
    f0 = P.track_f0(x, decoder='viterbi')
    assert f0.shape == (1, 1, x.shape[-1] // 64 + 1) and not bool(f0.any())


def test_convert_audio_with_the_viterbi_decoder(dev):
    P = pkg()
    G, _ = build_models(dev)
    T = 8320
    rng = np.random.default_rng(12)
    x = torch.from_numpy(YR.make_signal(rng, T))[None, None].to(dev)
    c_tgt = torch.zeros(1, 16, device=dev); c_tgt[0, 3] = 1.0
    noise = (torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev),
             torch.from_numpy(rng.standard_normal((1, 1, T)).astype(np.float32)).to(dev))
    phi0 = torch.tensor([0.5], device=dev)
    y = P.infer.convert_audio(G, x, c_tgt, noise=noise, start_phase=phi0, decoder='viterbi')
    y_ref = P.infer.convert(G, x, c_tgt, P.track_f0(x, decoder='viterbi'), noise=noise, start_phase=phi0)
    torch.cuda.synchronize()
    assert y.shape == (1, 1, T) and bool(torch.isfinite(y).all()) and torch.equal(y, y_ref)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch(dev):
    L = pkg()._lib
    lib = L.lib()
    c = exact_case('n65')
    B, F, n = c['x'].shape
    W = c['logw'].shape[1]
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
    path = torch.full((B, F), -7, dtype=torch.int32, device=dev)
    nbytes = lib.tdvc_viterbi_workspace(B, F, n)
    assert nbytes >= B * F * n * 2
    wsbuf = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    ws = (wsbuf, nbytes)
    cases = [
        (dict(n=0), EINVAL), (dict(n=-3), EINVAL), (dict(F=0), EINVAL), (dict(F=-1), EINVAL), (dict(W=0), EINVAL), (dict(W=-2), EINVAL),
        (dict(B=-1), EINVAL), (dict(W=n + 1), EINVAL),                           # a band wider than the state axis leaves [0, n)
        (dict(jump=-0.5), EINVAL), (dict(jump=float('nan')), EINVAL), (dict(x_fs=n - 1), EINVAL),
        (dict(nulls=('x',)), EINVAL), (dict(nulls=('logw',)), EINVAL), (dict(nulls=('lo',)), EINVAL), (dict(nulls=('path',)), EINVAL),
        (dict(n=1025, W=W), EUNSUPPORTED), (dict(n=1024, W=257), EUNSUPPORTED),
        (dict(ws=(None, nbytes)), EWORKSPACE), (dict(ws=(wsbuf, nbytes - 1)), EWORKSPACE), (dict(ws=(wsbuf, 0)), EWORKSPACE),
    ]
    for kw, want in cases:
        kw = {'ws': ws, **kw}
        rc = raw_call(dev, c, path, F, **kw)
        assert rc == want, (kw.keys(), rc, want)
        assert lib.tdvc_last_error()
        assert bool((path == -7).all()) and bool((wsbuf == 0x5A).all()), kw.keys()
    assert raw_call(dev, c, path, F, B=0, ws=ws) == 0                            # a no-op
    assert bool((path == -7).all()) and bool((wsbuf == 0x5A).all())
    assert lib.tdvc_viterbi_workspace(B, F, 1025) == 0 and lib.tdvc_viterbi_workspace(B, 0, n) == 0
    assert raw_call(dev, c, path, F, ws=ws) == 0 and np.array_equal(path.cpu().numpy(), c['want'])      # and the same buffers do work


def test_python_refusals(dev):
    P = pkg()
    Pt = P.pitch
    x = torch.zeros(1, 1, 4096, device=dev)
    with pytest.raises(ValueError):
        P.track_f0(x, decoder='viterbi', soft=True)
    with pytest.raises(ValueError):
        P.yin_f0(x[0], SR, 60, 500, 64 / SR, decoder='viterbi', soft=True)
    with pytest.raises(ValueError):
        P.track_f0(x, decoder='median')
    with pytest.raises(ValueError):
        P.yin_f0(x[0], SR, decoder='argmax')
    c = exact_case('n65')
    t = lambda a: torch.from_numpy(a).to(dev)
    bad = c['lo'].copy(); bad[-1] = c['x'].shape[-1] - c['logw'].shape[1] + 1      # the last band leaves [0, n)
    with pytest.raises(ValueError):
        Pt.viterbi_path(t(c['x']), t(c['logw']), t(bad))
    bad[-1] = c['lo'][-1]; bad[0] = -1
    with pytest.raises(ValueError):
        Pt.viterbi_path(t(c['x']), t(c['logw']), t(bad))
    with pytest.raises(ValueError):
        Pt.viterbi_path(t(c['x']), t(c['logw'])[:-1], t(c['lo']))
    with pytest.raises(RuntimeError):
        Pt.viterbi_path(torch.from_numpy(c['x']), t(c['logw']), t(c['lo']))      # a CPU lattice: there is no fallback
