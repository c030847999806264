"""CPU: the host side of the ECAPA-TDNN speaker-recognition metric (td-vc-gan_amd/ecapa.py) and the float64 restatement the GPU tests
measure against (tests/ecapa_ref.py). speechbrain and torchaudio are not available: nothing here is a parity test against them.

1. The symbols are declared, bound and built; eval_ecapa.hip is in SRCS; the "unchecked" sentence is in the header and the docstring.
2. The filterbank: mel(700 (10^(1000/2595) - 1)) = 1000, centres monotone, every filter symmetric about its centre with half-width
   equal to the LEFT spacing (a table built with the right spacing, or area-normalised, fails), the package's vectorised table
   equals the band-by-band one.
3. The state-dict keys and shapes equal the listed ones for the default configuration and for a small one; loading is strict both
   ways.
4. load_ecapa takes the two fixtures: 99 labels, ind2lab[0] == 'p293', weight (100, 192).
5. running_mean_norm against the literal loop (first row zero); speaker_classify against the numpy lines of the script.
6. The restatement's row-alone property in float64: a row inside a padded batch equals the row evaluated alone.
7. The float64 front end is within 2^-24 / 4 (of the row's largest magnitude) of a long double evaluation on inputs the GPU test
   uses: the bar of 4 * 2^-24 there is meaningful.
8. Every wrapper refuses CPU tensors; the constructor refuses what the kernels do not take.
"""
import os
import re

import numpy as np
import pytest
import torch

import ecapa_ref as R
from common import GOLDEN, ROOT, pkg

NAMES = ['tdvc_fbank', 'tdvc_fbank_workspace', 'tdvc_tdnn_fwd', 'tdvc_se_block', 'tdvc_asp_pool', 'tdvc_asp_pool_workspace', 'tdvc_ecapa_head']


def E():
    return pkg().ecapa


def test_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = pkg()._lib.lib()
    for n in NAMES:
        assert n in pkg()._lib.SIGNATURES and re.search(r'\b%s\(' % n, header) and hasattr(lib, n), n
    mk = open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\beval_ecapa\.hip\b', mk, re.M)
    words = 'parity with an installed speechbrain is unchecked'
    assert words in E().__doc__ and words in header.lower()
    # refusals are decided on the host: the workspace queries answer 0 for what the calls refuse
    assert lib.tdvc_fbank_workspace(1, 639, 80) == 0 and lib.tdvc_fbank_workspace(1, 640, 136) == 0 and lib.tdvc_fbank_workspace(1, 640, 72) == 0
    assert lib.tdvc_fbank_workspace(2, 800, 80) == 2 * 80 * 6 * 8 + 256
    assert lib.tdvc_asp_pool_workspace(1, 384, 32, 4) == 0 and lib.tdvc_asp_pool_workspace(1, 380, 32, 5) == 0
    assert lib.tdvc_asp_pool_workspace(1, 384, 32, 5) == 3072 + 256 + 768 + 7680
    for name in ('EcapaTdnn', 'load_ecapa', 'fbank', 'fbank_matrix', 'speaker_classify', 'running_mean_norm'):
        assert getattr(pkg(), name) is getattr(E(), name)


def test_filterbank_is_speechbrains():
    assert abs(R.hz_to_mel(700.0 * (10.0 ** (1000.0 / 2595.0) - 1.0)) - 1000.0) < 1e-9
    assert abs(float(E().hz_to_mel(700.0 * (10.0 ** (1000.0 / 2595.0) - 1.0))) - 1000.0) < 1e-9
    hz = R.mel_points(80)
    assert hz.shape == (82,) and hz[0] == 0.0 and abs(hz[-1] - 8000.0) < 1e-9 and (np.diff(hz) > 0).all()
    fb = R.filterbank(80)
    assert fb.shape == (80, 201) and (fb >= 0).all() and fb.max() <= 1.0
    f = np.linspace(0.0, 8000.0, 201)
    for i in range(80):
        f_c, left, right = hz[i + 1], hz[i + 1] - hz[i], hz[i + 2] - hz[i + 1]
        want = np.maximum(0.0, 1.0 - np.abs(f - f_c) / left)                # symmetric, half-width = the LEFT spacing, peak 1
        assert np.abs(fb[i] - want).max() < 1e-12, i
        above = (f > f_c + left) & (f < f_c + right)                        # where a right-spaced triangle would still be positive
        assert (fb[i][above] == 0).all()
    assert any(((f > hz[i + 1] + hz[i + 1] - hz[i]) & (f < hz[i + 2])).any() for i in range(80))       # the distinction is sampled
    assert fb.sum(1).max() > 2.0                                            # not area-normalised: wide bands sum to many bins
    got = E().fbank_matrix(80)
    assert got.shape == fb.shape and np.abs(got - fb).max() <= 1e-12 and not got.flags.writeable
    assert E().fbank_matrix(80) is got
    assert np.abs(E().fbank_matrix(16) - R.filterbank(16)).max() <= 1e-12


@pytest.mark.parametrize('cfg', [R.FULL, R.SMALL], ids=['default', 'small'])
def test_state_dict_keys_and_shapes(cfg):
    want = R.expected_shapes(**cfg)
    with torch.device('meta'):
        enc = E().EcapaTdnn(**cfg) if cfg is not R.FULL else E().EcapaTdnn()
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    assert len(want) == 7 + 3 * (7 * 9 + 4) + 7 + 7 + 2 + 5 + 2
    if cfg is R.FULL:
        assert want['blocks.0.conv.conv.weight'] == (1024, 80, 5) and want['blocks.2.res2net_block.blocks.6.conv.conv.weight'] == (128, 128, 3)
        assert want['asp.tdnn.conv.conv.weight'] == (128, 9216, 1) and want['asp_bn.norm.running_var'] == (6144,) and want['fc.conv.weight'] == (192, 6144, 1)
    else:
        enc = E().EcapaTdnn(**cfg)
        sd = R.state_dict(1, cfg)
        enc.load_state_dict(sd, strict=True)                                # strict one way ...
        assert all(torch.equal(enc.state_dict()[k], sd[k]) for k in sd)
        with pytest.raises(RuntimeError):
            enc.load_state_dict({k: v for k, v in sd.items() if k != 'fc.conv.bias'}, strict=True)
        with pytest.raises(RuntimeError):
            enc.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
        x = torch.randn(80, 9, dtype=torch.float64)                         # ... and the other: the restatement runs on the module's own dict
        assert R.embed_row(R.cast(enc.state_dict(), torch.float64), x).shape == (48,)


def test_constructor_refuses_what_the_kernels_do_not_take():
    X = E().EcapaTdnn
    for bad in (dict(channels=[64, 64, 64, 64, 192]), dict(channels=[136, 136, 136, 136, 408]), dict(input_size=72), dict(se_channels=8),
                dict(attention_channels=100), dict(lin_neurons=50), dict(kernel_sizes=[7, 3, 3, 3, 1]), dict(dilations=[1, 2, 3, 5, 1]),
                dict(channels=[128, 128, 128, 128, 256]), dict(res2net_scale=4)):
        with pytest.raises(ValueError, match='EcapaTdnn'):
            X(**{**R.SMALL, **bad})


def test_load_ecapa_takes_the_fixtures(tmp_path):
    out = E().load_ecapa(None, os.path.join(GOLDEN, 'ecapa_classifier.npz'), os.path.join(GOLDEN, 'ecapa_labels_vctk.txt'))
    assert out['model'] is None and tuple(out['weight'].shape) == (100, 192) and out['weight'].dtype == torch.float32
    assert len(out['lab2ind']) == 99 and out['ind2lab'][0] == 'p293' and out['lab2ind']['p244'] == 98
    assert 'starting_index' not in out['lab2ind']
    assert torch.isfinite(out['weight']).all() and float(out['weight'].abs().max()) > 0
    sd = R.state_dict(2)
    torch.save(sd, tmp_path / 'embedding_model.ckpt')
    torch.save({'weight': torch.ones(3, 48)}, tmp_path / 'classifier.ckpt')
    got = E().load_ecapa(str(tmp_path / 'embedding_model.ckpt'), str(tmp_path / 'classifier.ckpt'), **R.SMALL)
    assert all(torch.equal(got['model'].state_dict()[k], sd[k]) for k in sd) and not got['model'].training
    assert tuple(got['weight'].shape) == (3, 48)
    torch.save(dict(sd, extra=torch.zeros(1)), tmp_path / 'bad.ckpt')
    with pytest.raises(RuntimeError):
        E().load_ecapa(str(tmp_path / 'bad.ckpt'), **R.SMALL)
    with pytest.raises(ValueError, match='load_ecapa'):
        E().load_ecapa(None, str(tmp_path / 'embedding_model.ckpt'))


def test_running_mean_norm_is_the_literal_loop():
    emb = np.random.RandomState(0).randn(9, 192)
    got = E().running_mean_norm(torch.from_numpy(emb)).double().numpy()
    want = R.running_mean_loop(emb)
    assert (got[0] == 0).all() and np.abs(got - want).max() <= 64 * 2.0 ** -24
    assert not np.allclose(E().running_mean_norm(torch.from_numpy(emb[::-1].copy())).numpy()[::-1], got)      # it depends on the order


def test_speaker_classify_against_the_script_lines():
    r = np.random.RandomState(1)
    weight = np.load(os.path.join(GOLDEN, 'ecapa_classifier.npz'))['weight'].astype(np.float64)
    target = r.randint(0, 100, 12)
    emb = weight[target] + 0.05 * r.randn(12, 192) * np.abs(weight).max()
    prob, pred, tp = R.classify_numpy(emb, weight, target)
    gp, gpred, gtp = E().speaker_classify(torch.from_numpy(emb).float(), torch.from_numpy(weight).float(), torch.from_numpy(target))
    assert gp.shape == (12, 100) and gpred.dtype == torch.int64
    assert np.abs(gp.numpy() - prob).max() <= 64 * 2.0 ** -24 and np.abs(gtp.numpy() - tp).max() <= 64 * 2.0 ** -24
    assert np.array_equal(gpred.numpy(), pred) and np.array_equal(pred, target)
    assert abs(float(gp.sum(1).max()) - 1.0) < 1e-5 and E().speaker_classify(torch.from_numpy(emb).float(), torch.from_numpy(weight).float())[2] is None


def test_restatement_evaluates_a_row_as_if_alone():
    sd = R.cast(R.state_dict(3), torch.float64)
    ns = (5, 33, 47)
    g = torch.Generator().manual_seed(0)
    feats = torch.full((3, 80, 47), float('nan'), dtype=torch.float64)
    for b, n in enumerate(ns):
        feats[b, :, :n] = torch.randn(80, n, generator=g, dtype=torch.float64)
    batch = R.embed_batch(sd, feats, ns)
    assert torch.isfinite(batch).all()
    for b, n in enumerate(ns):
        assert torch.equal(batch[b], R.embed_row(sd, feats[b, :, :n].clone()))


@pytest.mark.parametrize('n,kind', [(640, 'tones'), (799, 'tones'), (25439, 'tones'), (8000, 'burst')])
def test_float64_front_end_is_good_to_well_under_the_fp32_bar(n, kind):
    x = R.tones(n, seed=n) if kind == 'tones' else R.burst(n, seed=n)
    f64 = R.fbank(x)
    fld = R.fbank(x, dtype=np.longdouble)
    assert f64.shape == (80, 1 + n // 160)
    err = float(np.abs(f64 - fld).max()) / float(np.abs(fld).max())
    print(f'float64 fbank against long double, n={n} {kind}: {err:.3e} of the row maximum (bar 2^-24 / 4 = {2.0 ** -26:.3e})')
    assert err <= 2.0 ** -26
    assert np.abs(f64.mean(axis=1)).max() < 1e-9


def test_no_cpu_fallback():
    P, ec = pkg(), E()
    enc = ec.EcapaTdnn(**R.SMALL)
    x = torch.zeros(2, 1, 8000)
    a, w = torch.zeros(1, 16, 8), torch.zeros(16, 16, 3)
    v = torch.zeros(16)
    for fn in (lambda: ec.fbank(x), lambda: enc.embed(x), lambda: enc.features(x), lambda: enc(x), lambda: enc.embed_features(torch.zeros(1, 80, 8)),
               lambda: ec.tdnn_fwd(a, w, v), lambda: ec.se_block(a, a, torch.zeros(16, 16), v, torch.zeros(16, 16), v),
               lambda: ec.asp_pool(a, torch.zeros(16, 48), v, v, v, torch.zeros(16, 16), v), lambda: ec.ecapa_head(torch.zeros(1, 32), torch.zeros(32),
                                                                                                                   torch.zeros(32), torch.zeros(16, 32), v)):
        with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
            fn()
