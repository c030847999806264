"""GPU: tdvc_peq_sos / tdvc_sos_filter (csrc/audio_eq.hip) through corrupt.peq_sos / sos_filter / random_eq / corrupt_audio /
device_batch against the float64 restatement tests/peq_ref.py, which tests/golden/peq.npz pins to the reference's own random_eq.

Bound (per row, every element): |y - truth| <= 4 * 2^-24 * max|truth_row|. The kernel's output is the float64 result rounded once to
fp32 (<= 2^-25 of the element, i.e. a quarter of the bound at the row maximum); the factor 4 is margin for another float64 operation
order. The same cascade run with fp32 coefficients and state misses this bound by 50x or more on every speech-like case
(asserted below, so the bound cannot be too loose to tell). peq_sos: 1e-12 relative, per coefficient.
"""
import os

import numpy as np
import pytest
import torch

import peq_ref as PR
from common import ROOT, build_models, pkg

pytestmark = pytest.mark.gpu


def dev_inputs(name, dev):
    t = PR.truth(name)
    return t, torch.from_numpy(t['x']).to(dev), torch.from_numpy(t['sos']).to(dev)


def assert_within_bound(y, ref, what):
    """y: device or numpy fp32 [B, T]; ref float64 [B, T]. Prints the worst error in units of the bound, then asserts."""
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else y
    assert y.dtype == np.float32 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    assert np.isfinite(y).all(), what
    bd = PR.bound(ref)
    err = np.abs(y.astype(np.float64) - ref)
    worst = float((err / np.where(bd > 0, bd, 1.0)).max())
    print(f'[peq] {what}: worst |y - truth| / bound = {worst:.3f}')
    assert (err <= bd).all(), (what, worst)
    return worst


def rms(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))


def assert_rms_matched(y, x, rms_unscaled, what):
    """rms(y) == rms(x) to 1e-6 relative. The reference's gain is rms(x) / (rms(y0) + 1e-8) with y0 the unscaled output, so by its own
    formula rms(y) = rms(x) * r / (r + 1e-8), r = rms(y0): at the project's -30 dB signal level a cut EQ leaves r ~ 5e-3 and the 1e-8
    alone moves the ratio by 2e-6 (the float64 truth misses a plain 1e-6 comparison there too). The comparison therefore takes that
    known factor into account, at the same 1e-6, on every case; where the 1e-8 is itself below a quarter of the tolerance
    (1e-8 / r <= 2.5e-7) the plain rms(y) == rms(x) is asserted as well."""
    want = rms(x) * rms_unscaled / (rms_unscaled + 1e-8)
    assert abs(rms(y) - want) <= 1e-6 * want, (what, rms(y), want)
    if 1e-8 / rms_unscaled <= 2.5e-7:
        assert abs(rms(y) - rms(x)) <= 1e-6 * rms(x), (what, rms(y), rms(x))


@pytest.mark.parametrize('match', [False, True])
@pytest.mark.parametrize('name', PR.CASES)
def test_sos_filter_vs_float64(dev, name, match):
    C = pkg().corrupt
    t, x, sos = dev_inputs(name, dev)
    ref = t['y_rms'] if match else t['y']
    if name == 'odd':      # rows of a wider buffer: x_bs = ODD_PITCH != T, and the neighbouring floats must not leak in
        wide = torch.full((PR.ODD_B, PR.ODD_PITCH), 1e3, device=dev)
        wide[:, :PR.ODD_T] = x
        x = wide[:, :PR.ODD_T]
        assert x.stride(0) == PR.ODD_PITCH and not x.is_contiguous()
    y = C.sos_filter(x, sos, match_rms=match)
    assert y.shape == x.shape and y.dtype == torch.float32
    assert_within_bound(y, ref, f'{name} match_rms={match}')
    if name == 'silence':
        assert not bool(y.any())                                        # exact zeros, no NaN from 0 / (0 + 1e-8)
    if match and name != 'silence':
        for b in range(len(ref)):
            assert_rms_matched(y[b].cpu().numpy(), t['x'][b], rms(t['y'][b]), (name, b))
    if name in PR.SPEECH_LIKE:
        ratio = (np.abs(PR.fp32_run(name) - t['y']) / PR.bound(t['y'])).max(-1)
        assert float(ratio.min()) >= 50, (name, ratio)                  # an fp32 cascade would not pass this bound


@pytest.mark.parametrize('name', ['speech', 'mixed_rows', 'odd', 'step'])
def test_peq_sos_vs_float64(dev, name):
    C = pkg().corrupt
    t = PR.truth(name)
    sos = C.peq_sos(torch.from_numpy(t['G']).to(dev), torch.from_numpy(t['Q']).to(dev))
    assert sos.dtype == torch.float64 and tuple(sos.shape) == t['sos'].shape
    got = sos.cpu().numpy()
    rel = np.abs(got - t['sos']) / np.abs(t['sos'])
    print(f'[peq] peq_sos {name}: worst relative coefficient error {rel.max():.3e}')
    assert float(rel.max()) <= 1e-12 and np.all(got[..., 3] == 1.0)


def test_peq_sos_other_band_counts_and_guards(dev):
    """n = 2 (two shelves) and n = 5 with caller-given centres, one of them below the reference's 2 Hz floor."""
    C = pkg().corrupt
    rng = np.random.default_rng(11)
    for n, fc in ((2, np.array([100.0, 5000.0])), (5, np.array([0.5, 300.0, 1000.0, 3000.0, 7000.0]))):
        G = rng.uniform(-12, 12, (3, n)).astype(np.float32)
        Q = rng.uniform(2, 5, (3, n)).astype(np.float32)
        ref = PR.peq_sos(G.astype(np.float64), Q.astype(np.float64), fc=fc)
        got = C.peq_sos(torch.from_numpy(G).to(dev), torch.from_numpy(Q).to(dev), fc=fc).cpu().numpy()
        assert float((np.abs(got - ref) / np.abs(ref)).max()) <= 1e-12, n
    with pytest.raises(ValueError):
        C.peq_sos(torch.zeros(2, 1, device=dev), torch.ones(2, 1, device=dev), fc=[100.0])


@pytest.mark.parametrize('n', [1, 3])
def test_sos_filter_arbitrary_sections(dev, n):
    """Stable sections that are no EQ bands, S = 1 and S = 3: the section count is not hard-wired to 10."""
    C = pkg().corrupt
    _, g = PR.fixture()
    x0 = g['speech_signal'][:1]
    sec = g['sections_sos'][:n]
    ref = PR.sosfilt(sec, x0[0])[None]
    y = C.sos_filter(torch.from_numpy(x0).to(dev), torch.from_numpy(sec)[None].to(dev))
    assert_within_bound(y, ref, f'sections S={n}')
    y1 = C.sos_filter(torch.from_numpy(x0[0]).to(dev), torch.from_numpy(sec).to(dev))      # [T] with a [S, 6] cascade
    assert y1.shape == (x0.shape[1],) and torch.equal(y1, y[0])


def test_sixteen_sections_run_and_seventeen_raise(dev):
    C = pkg().corrupt
    _, g = PR.fixture()
    x0 = g['speech_signal'][:1, :600]
    sec = np.concatenate([g['sections_sos']] * 6)[:17]
    ref = PR.sosfilt(sec[:16], x0[0])[None]
    y = C.sos_filter(torch.from_numpy(x0).to(dev), torch.from_numpy(sec[:16])[None].to(dev))
    assert_within_bound(y, ref, 'S=16')
    with pytest.raises(ValueError):
        C.sos_filter(torch.from_numpy(x0).to(dev), torch.from_numpy(sec)[None].to(dev))
    with pytest.raises(ValueError):
        C.sos_filter(torch.from_numpy(x0).to(dev), torch.zeros(1, 0, 6, dtype=torch.float64, device=dev))


def test_random_eq_with_the_reference_draws_matches_the_reference(dev):
    """random_eq / corrupt_audio fed the reference's float64 draws against what the reference's random_eq (+ eq_rms_signals) returned
    for them: the stored output is the truth here, not the restatement."""
    P = pkg()
    _, g = PR.fixture()
    x = torch.from_numpy(g['speech_signal']).to(dev)
    G, z = torch.from_numpy(g['speech_G']).to(dev), torch.from_numpy(g['speech_z']).to(dev)
    assert_within_bound(P.corrupt.random_eq(x, gains_db=G, z=z, match_rms=False), g['speech_y'], 'random_eq vs reference')
    y = P.corrupt_audio(x[:, None], gains_db=G, z=z)
    assert y.shape == (2, 1, 4000)
    assert_within_bound(y[:, 0], g['speech_y_rms'], 'corrupt_audio vs reference')
    assert torch.equal(y, P.corrupt.random_eq(x[:, None], gains_db=G, z=z, match_rms=True))


def test_layouts_and_repeat_runs_are_bit_identical(dev):
    C = pkg().corrupt
    t, x, sos = dev_inputs('speech', dev)
    for match in (False, True):
        y = C.sos_filter(x, sos, match_rms=match)
        assert torch.equal(y, C.sos_filter(x, sos, match_rms=match))
        assert torch.equal(y, C.sos_filter(x[:, None], sos, match_rms=match)[:, 0])
        assert torch.equal(y[1], C.sos_filter(x[1], sos[1:], match_rms=match))
        wide = torch.zeros(2, 2, 4000, device=dev)
        wide[:, 1] = x
        assert torch.equal(y, C.sos_filter(wide[:, 1], sos, match_rms=match))          # row stride 8000
        sparse = torch.zeros(2, 8000, device=dev)
        sparse[:, ::2] = x
        assert torch.equal(y, C.sos_filter(sparse[:, ::2], sos, match_rms=match))        # last axis not dense: copied
    assert C.sos_filter(x[:0], sos[:0]).shape == (0, 4000)
    assert C.sos_filter(x[:, :0], sos).shape == (2, 0)


def test_random_eq_draws(dev):
    """Without draws: reproducible under a seeded generator, different under another seed, and over 64 rows the gains stay in
    [-12, 12] dB and z in [0, 1] (read back by drawing from an identically seeded generator in the same order)."""
    C = pkg().corrupt
    x = torch.from_numpy(PR.truth('speech')['x'][:1, :1000]).to(dev).expand(64, 1000)
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    y = C.random_eq(x, generator=gen(7))
    assert torch.equal(y, C.random_eq(x, generator=gen(7)))
    assert not torch.equal(y, C.random_eq(x, generator=gen(8)))
    g7 = gen(7)
    G = (torch.rand(64, 10, device=dev, generator=g7) * 2.0 - 1.0) * 12.0
    z = torch.rand(64, 10, device=dev, generator=g7)
    assert float(G.min()) >= -12 and float(G.max()) <= 12 and float(z.min()) >= 0 and float(z.max()) <= 1
    assert float(G.max() - G.min()) > 20 and float(z.max() - z.min()) > 0.9              # and they fill those ranges
    assert torch.equal(y, C.random_eq(x, gains_db=G, z=z))
    y0 = C.random_eq(x, gains_db=G, z=z, match_rms=False).cpu().numpy()
    for b in range(64):                                                                  # RMS-matched, every row
        assert_rms_matched(y[b].cpu().numpy(), x[0].cpu().numpy(), rms(y0[b]), b)
    assert len({bytes(r.cpu().numpy().tobytes()) for r in y[:8]}) == 8                   # per-row coefficients


def test_random_eq_under_graph_capture(dev):
    """random_eq with static inputs captured into one graph; a replay after rewriting the input equals the eager result."""
    C = pkg().corrupt
    t = PR.truth('speech')
    x = torch.from_numpy(t['x']).to(dev)
    G = torch.from_numpy(t['G']).to(dev)
    z = torch.rand(2, 10, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        C.random_eq(x, gains_db=G, z=z)                                                  # warm-up: library load, fc upload, allocator
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = C.random_eq(x, gains_db=G, z=z)
    graph.replay()
    torch.cuda.synchronize(dev)
    first = y.clone()
    assert torch.equal(first, C.random_eq(x, gains_db=G, z=z))
    x.copy_(x.flip(0) * 0.5)
    G.copy_(-G)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert not torch.equal(y, first)
    assert torch.equal(y, C.random_eq(x, gains_db=G, z=z))


def test_device_batch_feeds_a_train_step(dev):
    """device_batch on a 4 x 8960 speech-like batch: keys, shapes and dtypes of synth.make_batch (plus f0_conv), signal_corrupted
    against the float64 truth for the supplied draws, and one conv_enc-stage1 iteration on it with every logged loss finite."""
    P = pkg()
    B, T, num_spk = 4, 8960, 16
    rng = np.random.default_rng(31)
    x = np.stack([PR.make_signal(rng, T, PR.SR) for _ in range(B)])
    G = rng.uniform(-12, 12, (B, 10)).astype(np.float32)
    z = rng.uniform(0, 1, (B, 10)).astype(np.float32)
    labels = torch.tensor([3, 0, 7, 12])
    perm = torch.tensor([2, 0, 3, 1])
    bt = P.device_batch(torch.from_numpy(x)[:, None].to(dev), labels.to(dev), num_spk, gains_db=torch.from_numpy(G).to(dev),
                        z=torch.from_numpy(z).to(dev), perm=perm.to(dev), generator=torch.Generator(device=dev).manual_seed(1))
    like = P.synth.make_batch(B, T, seed=1, num_spk=num_spk)
    assert set(bt) == set(like) | {'f0_conv'}
    for k, v in like.items():
        assert bt[k].shape == v.shape and bt[k].dtype == v.dtype and bt[k].is_cuda, (k, bt[k].shape, bt[k].dtype)
    assert bt['f0_conv'].shape == (B, 1, T // 64 + 1) and bt['f0_conv'].dtype == torch.float32
    assert torch.equal(bt['perm'].cpu(), perm) and torch.equal(bt['label_tgt'].cpu(), labels[perm])
    assert torch.equal(bt['c_src'].argmax(1).cpu(), labels) and torch.equal(bt['c_tgt'].argmax(1).cpu(), labels[perm])
    assert torch.equal(bt['signal_real'][:, 0].cpu(), torch.from_numpy(x))
    Q = PR.q_of_z(z.astype(np.float64)).astype(np.float32)                # as random_eq hands it to tdvc_peq_sos
    ref = PR.match_rms(PR.sosfilt_rows(PR.peq_sos(G.astype(np.float64), Q.astype(np.float64)), x), x)
    assert_within_bound(bt['signal_corrupted'][:, 0], ref, 'device_batch signal_corrupted')
    voiced = bt['f0_conv'] > 0
    assert 0.15 <= float(voiced.float().mean()) <= 0.95
    for k in ('c_f0_src', 'c_f0_conv'):
        assert bool(torch.isfinite(bt[k]).all()) and 0.01 < float(bt[k].std()) < 0.2, k
    same = P.device_batch(bt['signal_real'], labels.to(dev), num_spk, conversion=False)
    assert torch.equal(same['label_tgt'], same['label_src']) and torch.equal(same['perm'].cpu(), torch.arange(B))

    hp = P.hparams.HParam(os.path.join(ROOT, 'config', 'conv_enc-stage1.yaml'))
    cfg = P.train_step.StepConfig.from_hparams(hp.train, f0_loss='yin')
    Gm, Dm = build_models(dev)
    log = P.train_step.TrainStep(Gm, Dm, cfg, dev).run(bt)
    torch.cuda.synchronize()
    assert log and all(np.isfinite(float(v)) for v in log.values()), {k: float(v) for k, v in log.items()}
