"""CPU: the host side of the WavLM feature extractor (td-vc-gan_amd/wavlm.py) and the float64 restatement the GPU tests measure against
(tests/wavlm_ref.py), pinned to the reference's own output by tests/golden/wavlm_small.npz (tools/make_golden_wavlm.py).

1. The symbols are declared, bound and built; ssl_wavlm.hip is in SRCS; the "unchecked" sentence is in the header, the docstring and
   the README.
2. The state-dict keys and shapes, on the meta device for the Large defaults and on the small configuration, equal the fixture's key
   set; loading is strict both ways; relative_attention_bias appears in layer 0 only.
3. wavlm_ref against the fixture: the final output, both output_layer results and ret_conv within 1e-12 of their largest magnitude
   (float64 against float64, another summation order); the host bucket table equal to the reference's at all 4095 offsets.
4. The frame-count formula for L = 400, 401, 719, 720, 8160, 32160.
5. Every refusal and NotImplementedError path; the wrappers refuse CPU tensors.
6. The folded positional-convolution weight and the permuted convolution weights against their definitions.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import wavlm_ref as R
from common import GOLDEN, ROOT, pkg
from edge_support import EINVAL, EUNSUPPORTED

NAMES = ['tdvc_wavlm_gemm', 'tdvc_wavlm_frames', 'tdvc_wavlm_conv0', 'tdvc_wavlm_layernorm', 'tdvc_wavlm_posconv', 'tdvc_wavlm_attention']
WORDS = 'parity with a real wavlm-large.pt is unchecked'


def W():
    return pkg().wavlm


def fixture():
    z = np.load(os.path.join(GOLDEN, 'wavlm_small.npz'))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return z, json.loads(str(z['cfg'])), sd


def test_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = pkg()._lib.lib()
    for n in NAMES:
        assert n in pkg()._lib.SIGNATURES and re.search(r'\b%s\(' % n, header) and hasattr(lib, n), n
    mk = open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bssl_wavlm\.hip\b', mk, re.M)
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert WORDS in W().__doc__.lower().replace('*', '') and WORDS in header.lower() and WORDS in ' '.join(readme.lower().replace('*', '').split())
    for name in ('WavLM', 'WavLMConfig', 'load_wavlm'):
        assert getattr(pkg(), name) is getattr(W(), name)


def test_state_dict_keys_and_shapes_large_on_meta():
    want = R.expected_shapes(R.LARGE)
    with torch.device('meta'):
        m = W().WavLM()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want and len(got) == 1 + 21 + 2 + 2 + 3 + 2 + 24 * 19 + 1
    assert got['encoder.pos_conv.0.weight_v'] == (1024, 64, 128) and got['encoder.pos_conv.0.weight_g'] == (1, 1, 128)
    assert got['feature_extractor.conv_layers.0.0.weight'] == (512, 1, 10) and got['encoder.layers.23.fc1.weight'] == (4096, 1024)
    assert [k for k in got if 'relative_attention_bias' in k] == ['encoder.layers.0.self_attn.relative_attention_bias.weight']
    assert got['encoder.layers.0.self_attn.relative_attention_bias.weight'] == (320, 16) and got['mask_emb'] == (1024,)
    assert not any('packed' in k or 'pos.' in k for k in got)


def test_state_dict_small_equals_the_fixture_and_loads_strictly():
    z, cfg, sd = fixture()
    m = W().WavLM(W().WavLMConfig(cfg))
    mine = m.state_dict()
    assert set(mine) == set(sd) and all(tuple(mine[k].shape) == tuple(sd[k].shape) for k in sd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.expected_shapes(R.SMALL)
    assert [k for k in sd if 'relative_attention_bias' in k] == ['encoder.layers.0.self_attn.relative_attention_bias.weight']
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    for drop in ('mask_emb', 'encoder.pos_conv.0.weight_g', 'encoder.layers.1.self_attn.grep_a'):
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != drop}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{'encoder.layers.1.self_attn.relative_attention_bias.weight': torch.zeros(320, 4)}), strict=True)
    assert not m.training and m.num_frames(8160) == 25 and m.min_samples() == 400


def test_load_wavlm_takes_the_reference_checkpoint_layout(tmp_path):
    z, cfg, sd = fixture()
    torch.save({'cfg': cfg, 'model': sd}, tmp_path / 'wavlm.pt')
    m = W().load_wavlm(str(tmp_path / 'wavlm.pt'))
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd) and m.cfg.encoder_embed_dim == 64 and not m.training
    torch.save({'cfg': cfg, 'model': dict(sd, extra=torch.zeros(1))}, tmp_path / 'bad.pt')
    with pytest.raises(RuntimeError):
        W().load_wavlm(str(tmp_path / 'bad.pt'))
    torch.save(sd, tmp_path / 'bare.pt')
    with pytest.raises(ValueError, match='load_wavlm'):
        W().load_wavlm(str(tmp_path / 'bare.pt'))


def test_restatement_against_the_reference_fixture():
    z, cfg, sd = fixture()
    assert all(cfg[k] == v for k, v in R.full_cfg(R.SMALL).items())
    sdd, x = R.cast(sd, torch.float64), torch.from_numpy(z['input']).double()
    assert tuple(x.shape) == (2, 8160) and 0.02 < float(x.std()) < 0.045      # -30 dB
    trace = {}
    for name, kw in (('out', dict(trace=trace)), ('layer1', dict(output_layer=1)), ('layer2', dict(output_layer=2)), ('conv', dict(ret_conv=True))):
        got, want = R.extract(sdd, R.SMALL, x, **kw), torch.from_numpy(z[name])
        assert want.dtype == torch.float64 and tuple(want.shape) == (2, 25, 64)
        err = float((got - want).abs().max() / want.abs().max())
        print(f'wavlm_ref against the reference, {name}: {err:.3e} of the largest magnitude {float(want.abs().max()):.3f}')
        assert err <= 1e-12, (name, err)
    assert not np.array_equal(z['layer2'], z['out']) and not np.array_equal(z['layer1'], z['layer2'])
    assert {'conv0', 'conv6', 'norm', 'proj', 'pos', 'l0', 'l1'} <= set(trace) and set(trace['l0']) == {'h', 'qkv', 'gate', 'att', 'x1', 'h2', 'f1', 'x2'}
    gate = trace['l0']['gate']
    assert float(gate.max() - gate.min()) > 0.2 and float((gate - 1.75).abs().min()) > 1e-6      # not the init value 0.5 (0.5 - 1) + 2 = 1.75


def test_bucket_table_equals_the_reference_at_all_offsets():
    z, _, _ = fixture()
    rel = torch.arange(-2047, 2048)
    want = torch.from_numpy(z['buckets'])
    assert want.shape == (4095,) and int(want.min()) == 0 and int(want.max()) == 319
    assert torch.equal(W().relative_buckets(rel, 320, 800), want) and torch.equal(R.buckets(rel, 320, 800), want)
    assert want[2047 - 79] == 79 and want[2047 - 80] == 80 and want[2047 + 1] == 161 and want[0] == 159 and want[-1] == 319
    assert int((want == 159).sum()) > 1000                                    # the clamp is reached long before 2047


@pytest.mark.parametrize('n,want', [(399, 0), (400, 1), (401, 1), (719, 1), (720, 2), (8160, 25), (32160, 100), (320160, 1000)])
def test_frame_count_formula(n, want):
    layers = W().conv_layers(W().WavLMConfig())
    assert layers == [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
    assert W().frame_count(n, layers) == want == R.frames(n, R.LARGE)
    ks = (C.c_int32 * 7)(*[k for _, k, _ in layers])
    ss = (C.c_int32 * 7)(*[s for _, _, s in layers])
    assert pkg()._lib.lib().tdvc_wavlm_frames(n, 7, ks, ss) == want
    x = torch.zeros(1, 1, n)
    for _, k, s in layers:                                                   # torch's own Conv1d arithmetic
        if x.shape[2] < k:
            x = x[:, :, :0]
            break
        x = torch.nn.functional.conv1d(x, torch.zeros(1, 1, k), stride=s)
    assert x.shape[2] == want


def test_configurations_outside_the_definition_are_named():
    X, Cf = W().WavLM, W().WavLMConfig
    small = R.full_cfg(R.SMALL)
    for bad, word in ((dict(extractor_mode='default'), 'extractor_mode'), (dict(layer_norm_first=False), 'layer_norm_first'),
                      (dict(gru_rel_pos=False), 'gru_rel_pos'), (dict(relative_position_embedding=False), 'relative_position_embedding'),
                      (dict(conv_bias=True), 'conv_bias'), (dict(activation_fn='relu'), 'activation_fn'), (dict(encoder_attention_heads=8), 'head width'),
                      (dict(conv_pos=15), 'conv_pos'), (dict(conv_pos_groups=8), 'conv_pos'), (dict(encoder_embed_dim=72), 'multiples of 16'),
                      (dict(conv_feature_layers='[(64,10,5)]'), 'post_extract_proj'), (dict(conv_feature_layers='[(24,10,5)]'), 'multiples of 16')):
        with pytest.raises(NotImplementedError, match=word):
            X(Cf(dict(small, **bad)))
    with pytest.raises(ValueError, match='conv_feature_layers'):
        X(Cf(dict(small, conv_feature_layers='__import__("os")')))
    m = X(Cf(small))
    x = torch.zeros(1, 8160)
    for kw, word in ((dict(mask=True), 'mask=True'), (dict(padding_mask=torch.zeros(1, 8160, dtype=torch.bool)), 'padding_mask'),
                     (dict(ret_layer_results=True), 'ret_layer_results'), (dict(output_layer=3), 'output_layer=3'), (dict(output_layer=0), 'output_layer=0')):
        with pytest.raises(NotImplementedError, match=word):
            m.extract_features(x, **kw)


def test_no_cpu_fallback():
    P, w = pkg(), W()
    m = w.WavLM(w.WavLMConfig(R.full_cfg(R.SMALL)))
    a, v = torch.zeros(1, 4, 16), torch.zeros(16)
    for fn in (lambda: m.extract_features(torch.zeros(1, 8160)), lambda: m(torch.zeros(1, 8160)), lambda: w.wavlm_gemm(a, torch.zeros(16, 16), v),
               lambda: w.wavlm_conv0(torch.zeros(1, 400), torch.zeros(10, 16), v, v, 5), lambda: w.wavlm_layernorm(a, v, v),
               lambda: w.wavlm_posconv(torch.zeros(1, 5, 16), torch.zeros(16, 2, 16), v, 2, 1),
               lambda: w.wavlm_attention(torch.zeros(1, 4, 48), 1, torch.zeros(1, 1, 4), torch.zeros(1, 7))):
        with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
            fn()


def test_c_abi_refusals_need_no_device():
    """Every refusal is decided on the host before any launch: the calls below return their status without a GPU."""
    L = pkg()._lib
    lib = L.lib()
    buf = (C.c_float * 72)()
    p = (C.addressof(buf) + 15) & ~15                                       # 16-byte aligned, 64 floats behind it

    def gemm(**kw):
        a = L.WavlmGemmArgs()
        a.B, a.T, a.N, a.K, a.groups = 1, 4, 16, 16, 1
        a.x, a.x_bs, a.x_ts, a.w, a.y, a.y_bs, a.y_ts = p, 64, 16, p, p, 64, 16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.tdvc_wavlm_gemm(C.byref(a), None)
    assert gemm(B=0) == 0 and gemm(T=0) == 0
    assert gemm(N=24) == EUNSUPPORTED and gemm(K=24) == EUNSUPPORTED and gemm(seg_len=8) == EUNSUPPORTED and gemm(B=70000) == EUNSUPPORTED
    assert gemm(epilogue=2) == EINVAL and gemm(x_ts=18) == EINVAL and gemm(y_ts=8) == EINVAL and gemm(x=p + 4) == EINVAL and gemm(y=None) == EINVAL
    assert gemm(K=48, seg_len=32) == EINVAL and gemm(T=-1) == EINVAL
    assert gemm(res=p, r_bs=64, r_ts=32) == EINVAL                          # a residual that is y, with other strides
    assert b'residual' in lib.tdvc_last_error()
    conv0 = lambda B=1, Ln=400, K=10, s=5, Cc=16, y_ts=16: lib.tdvc_wavlm_conv0(p, 400, B, Ln, p, K, s, Cc, p, p, p, 64, y_ts, None)
    assert conv0(B=0) == 0 and conv0(Ln=9) == EUNSUPPORTED and conv0(Cc=24) == EUNSUPPORTED and conv0(Cc=1040) == EUNSUPPORTED
    assert conv0(K=65) == EUNSUPPORTED and conv0(s=0) == EINVAL and conv0(y_ts=8) == EINVAL
    ln = lambda B=1, T=4, Cc=16, gelu=0, Hh=0, x_ts=16: lib.tdvc_wavlm_layernorm(p, 64, x_ts, B, T, Cc, p, p, gelu, p, 64, 16, Hh, p, p, p, p, None)
    assert ln(B=0) == 0 and ln(Cc=1040) == EUNSUPPORTED and ln(Cc=20) == EUNSUPPORTED and ln(gelu=2) == EINVAL and ln(x_ts=8) == EINVAL
    assert ln(Hh=3) == EINVAL and ln(Hh=1, gelu=1) == EINVAL
    pos = lambda B=1, T=2, Cc=16, K=2, G=1, bs=48: lib.tdvc_wavlm_posconv(p, bs, B, T, Cc, K, G, p, p, p, 32, 16, None)
    assert pos(B=0) == 0 and pos(K=3) == EUNSUPPORTED and pos(G=2) == EUNSUPPORTED and pos(bs=32) == EINVAL
    att = lambda B=1, T=4, Hh=1, d=16, ts=48, q=p: lib.tdvc_wavlm_attention(q, p, p, 192, ts, B, T, Hh, d, p, p, p, 64, 16, None)
    assert att(B=0) == 0 and att(d=8) == EUNSUPPORTED and att(d=128) == EUNSUPPORTED and att(T=4097) == EUNSUPPORTED
    assert att(ts=8) == EINVAL and att(ts=50) == EINVAL and att(q=p + 4) == EINVAL and att(q=None) == EINVAL


def test_folded_and_permuted_weights_against_their_definitions():
    z, cfg, sd = fixture()
    w = W()
    g, v = sd['encoder.pos_conv.0.weight_g'], sd['encoder.pos_conv.0.weight_v']
    folded = w.fold_pos_conv(g, v)
    assert tuple(folded.shape) == (64, 16, 16) and folded.dtype == torch.float32          # [C][K][C / G]
    want = torch._weight_norm(v.double(), g.double(), 2)                     # torch's own fold (what nn.utils.weight_norm calls), [C, C / G, K]
    assert float((folded.permute(0, 2, 1).double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())
    for tap in range(16):                                                    # one norm per tap, over dims 0 and 1
        col = folded[:, tap, :].double()
        assert abs(float(col.pow(2).sum().sqrt()) - abs(float(g[0, 0, tap]))) < 1e-6
    assert torch.equal(folded, R.fold_pos(R.cast(sd, torch.float64)).permute(0, 2, 1).float())
    cw = sd['feature_extractor.conv_layers.1.0.weight']                       # [32, 32, 3]
    perm = w.permute_conv(cw)
    assert tuple(perm.shape) == (32, 96)
    x = torch.randn(1, 7, 32, dtype=torch.float64)                            # token-major
    want = torch.nn.functional.conv1d(x.transpose(1, 2), cw.double(), stride=2)[0].t()          # [3, 32]
    rows = torch.stack([x[0, 2 * t:2 * t + 3].reshape(-1) for t in range(3)])
    assert float((rows @ perm.double().t() - want).abs().max()) < 1e-12
