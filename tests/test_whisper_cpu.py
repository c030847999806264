"""CPU: the host side of the Whisper ASR metric (td-vc-gan_amd/whisper.py) and the float64 restatement the GPU tests measure against
(tests/whisper_ref.py), pinned to HF transformers' own output by tests/golden/whisper_small.npz, whisper_small_audio.npz and
whisper_heads.npz (tools/make_golden_whisper.py; transformers is not needed here).

1. whisper_ref against the fixtures: the filter table, the encoder, the teacher-forced logits (1e-12 of the largest magnitude: float64
   against float64 in another summation order), the greedy ids, n_tokens and margins; the features within 2.5e-7 (HF's numpy path
   stores the spectrum as complex64 and rounds the log10 values to float32: half an ulp of 16 and of 8, plus 2^-23 / ln 10, over 4).
2. The fixture's own conditions: every margin >= 1e-3, one row stops at eos before the cap, one reaches it.
3. The symbols are declared, bound and built; asr_whisper.hip is in SRCS; the "unchecked" sentence is in the header and the docstrings.
4. The state-dict keys and shapes equal the fixture's; loading is strict both ways; proj_out.weight is accepted only when tied.
5. Every refusal through the C ABI with dummy pointers (nothing is launched); CPU tensors are refused; P + max_new_tokens beyond
   max_target_positions is refused on the host.
6. asr_wer / asr_cer on hand-computed cases and asr_report's aggregation on a two-speaker toy.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import whisper_ref as R
from common import GOLDEN, ROOT, pkg
from edge_support import EINVAL, EUNSUPPORTED

NAMES = ['tdvc_whisper_log_mel_workspace', 'tdvc_whisper_log_mel', 'tdvc_whisper_attention', 'tdvc_whisper_embed', 'tdvc_whisper_linear_step',
         'tdvc_whisper_attn_step', 'tdvc_whisper_workspace', 'tdvc_whisper_logits', 'tdvc_whisper_pick']
WORDS = 'parity with a real whisper-medium checkpoint is unchecked'


def W():
    return pkg().whisper


def fixtures():
    return tuple(np.load(os.path.join(GOLDEN, n)) for n in ('whisper_small.npz', 'whisper_small_audio.npz', 'whisper_heads.npz'))


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_restatement_against_the_fixture():
    z, a, hz = fixtures()
    cfg, sd = R.load(z)
    assert z['enc'].dtype == z['logits'].dtype == np.float64 and z['enc'].shape == (3, 100, 64) and z['logits'].shape == (3, 32, 203)
    assert rel(R.mel_filters(80), z['mel_filters']) <= 1e-12 and rel(W().whisper_mel_filters(80), z['mel_filters']) <= 1e-12
    feats = torch.from_numpy(a['features'].astype(np.float64))
    lm = R.log_mel(a['input'], a['lengths'], n_samples=a['input'].shape[1])
    ferr = float(np.abs(lm - a['features']).max())
    enc = R.encode(sd, cfg, feats)
    logits = R.step_logits(sd, cfg, torch.from_numpy(z['enc']), z['ids'])
    print(f'whisper_ref against HF: features {ferr:.3e} (absolute), enc {rel(enc, z["enc"]):.3e}, logits {rel(logits, z["logits"]):.3e}')
    assert a['features'].dtype == np.float32 and ferr <= 2.5e-7
    assert rel(enc, z['enc']) <= 1e-12 and rel(logits, z['logits']) <= 1e-12
    ids, n_tokens, margins = R.greedy(sd, cfg, torch.from_numpy(z['enc']), z['prompt'], 28, z['suppress'], z['begin_suppress'], int(z['eos']), int(z['pad']))
    assert np.array_equal(ids, z['ids']) and np.array_equal(n_tokens, z['n_tokens'])
    assert np.array_equal(np.isnan(margins), np.isnan(z['margins'])) and float(np.nanmax(np.abs(margins - z['margins']))) <= 1e-12 * np.abs(z['logits']).max()
    for tag in ('w16/', 'w64/'):
        c, s = R.load(hz, tag)
        assert c['d_model'] // c['encoder_attention_heads'] == int(tag[1:3])
        assert rel(R.encode(s, c, feats[1:2])[0], hz[tag + 'enc']) <= 1e-12
        assert rel(R.step_logits(s, c, torch.from_numpy(hz[tag + 'enc'])[None], hz[tag + 'ids'])[0], hz[tag + 'logits']) <= 1e-12


def test_fixture_meets_its_own_conditions():
    z, a, _ = fixtures()
    P, total = len(z['prompt']), z['ids'].shape[1]
    assert float(np.nanmin(z['margins'])) >= 1e-3
    assert (z['n_tokens'] < total).any() and (z['n_tokens'] == total).any()
    for b in range(3):
        n = int(z['n_tokens'][b])
        assert list(z['ids'][b, :P]) == list(z['prompt']) and (n == total or (z['ids'][b, n - 1] == z['eos'] and (z['ids'][b, n:] == z['pad']).all()))
        assert not set(z['ids'][b, P:n].tolist()) & set(z['suppress'].tolist()) and z['ids'][b, P] not in z['begin_suppress']
        assert len(set(z['ids'][b, P:n].tolist())) >= 3                      # not one repeated token
    assert list(a['lengths']) == [20000, 32000, 27000] and all((a['input'][b, a['lengths'][b]:] == 0).all() for b in range(3))
    assert all(z[k].dtype == np.float16 for k in z.files if k.startswith('sd/'))


def test_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'tdvc.h')).read()
    lib = pkg()._lib.lib()
    for n in NAMES:
        assert n in pkg()._lib.SIGNATURES and re.search(r'\b%s\(' % n, header) and hasattr(lib, n), n
    mk = open(os.path.join(ROOT, 'td-vc-gan_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\basr_whisper\.hip\b', mk, re.M) and re.search(r'^HDRS\s*:=.*\battn_tile\.h\b', mk, re.M)
    flat = lambda s: ' '.join(s.lower().replace('*', '').split())
    assert WORDS in flat(W().__doc__) and WORDS in flat(W().Whisper.__doc__) and WORDS in flat(header.replace(' *', ' '))
    for name in ('Whisper', 'WhisperConfig', 'load_whisper', 'whisper_log_mel', 'asr_wer', 'asr_cer', 'asr_report'):
        assert getattr(pkg(), name) is getattr(W(), name)


def test_state_dict_equals_hf_and_loads_strictly(tmp_path):
    z, _, hz = fixtures()
    cfg, sd = R.load(z)
    sd = {k: v.float() for k, v in sd.items()}
    assert 'proj_out.weight' in sd and {k: tuple(v.shape) for k, v in sd.items()} == R.expected_shapes(cfg, proj_out=True)
    m = W().Whisper(W().WhisperConfig(cfg))
    mine = m.state_dict()
    assert set(mine) == set(sd) - {'proj_out.weight'} and all(tuple(mine[k].shape) == tuple(sd[k].shape) for k in mine)
    assert {k: tuple(v.shape) for k, v in mine.items()} == R.expected_shapes(cfg)
    assert not any('k_proj.bias' in k for k in mine)
    m.load_state_dict(sd, strict=True)                                        # with the tied proj_out.weight
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in mine) and not m.training
    bare = {k: v for k, v in sd.items() if k != 'proj_out.weight'}
    m.load_state_dict(bare, strict=True)
    with pytest.raises(RuntimeError, match='tied'):
        m.load_state_dict(dict(sd, **{'proj_out.weight': sd['proj_out.weight'] + 1}), strict=True)
    for drop in ('model.encoder.embed_positions.weight', 'model.decoder.layers.1.encoder_attn.k_proj.weight', 'model.decoder.layer_norm.bias'):
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in bare.items() if k != drop}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(bare, **{'model.decoder.layers.0.self_attn.k_proj.bias': torch.zeros(64)}), strict=True)
    torch.save(sd, tmp_path / 'w.pt')
    m2 = W().load_whisper(str(tmp_path / 'w.pt'), cfg)
    assert all(torch.equal(m2.state_dict()[k], sd[k]) for k in mine) and m2.cfg.d_model == 64
    with pytest.raises(ValueError, match='load_whisper'):
        W().load_whisper({'cfg': 1}, cfg)
    with torch.device('meta'):
        big = W().Whisper()
    got = {k: tuple(v.shape) for k, v in big.state_dict().items()}
    assert got == R.expected_shapes(W().MEDIUM) and got['model.decoder.embed_tokens.weight'] == (51865, 1024) and got['model.encoder.embed_positions.weight'] == (1500, 1024)


def test_configurations_outside_the_definition_are_named():
    X = W().Whisper
    z, _, _ = fixtures()
    cfg, _ = R.load(z)
    for bad, word in ((dict(d_model=1280, encoder_attention_heads=20, decoder_attention_heads=20), 'whisper-large'), (dict(scale_embedding=True), 'scale_embedding'),
                      (dict(activation_function='relu'), 'activation_function'), (dict(decoder_attention_heads=8), 'head width'), (dict(d_model=72), 'multiple of 16'),
                      (dict(max_source_positions=5000), '4096')):
        with pytest.raises(NotImplementedError, match=word):
            X(dict(cfg, **bad))


def test_step_counter_contract_and_no_cpu_fallback():
    z, _, _ = fixtures()
    cfg, _ = R.load(z)
    w, P = W(), pkg()
    m = w.Whisper(cfg)
    feats = torch.zeros(1, 80, 200)
    with pytest.raises(ValueError, match='max_target_positions'):
        m.generate(feats, [196, 197, 198, 199], 29)                          # 4 + 29 > 32, refused before anything touches a device
    with pytest.raises(ValueError, match='max_target_positions'):
        m.step_logits(torch.zeros(1, 100, 64), np.zeros((1, 33), dtype=np.int32))
    with pytest.raises(ValueError, match='vocabulary'):
        m.generate(feats, [196, 203], 2)
    with pytest.raises(ValueError, match='empty prompt'):
        m.generate(feats, [], 2)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    v, x = torch.zeros(16), torch.zeros(1, 16)
    for fn in (lambda: m.generate(feats, [196], 2), lambda: m.encode(feats), lambda: m.step_logits(torch.zeros(1, 100, 64), [[1, 2]]),
               lambda: m.transcribe(torch.zeros(1, 100), None, [196], 2), lambda: w.whisper_log_mel(torch.zeros(1, 100), chunk_length=2),
               lambda: w.whisper_attention(torch.zeros(1, 4, 48), 1), lambda: w.whisper_embed(i32(1, 4), i32(1), torch.zeros(8, 16), torch.zeros(4, 16)),
               lambda: w.whisper_linear_step(x, torch.zeros(16, 16), v), lambda: w.whisper_attn_step(x, torch.zeros(1, 4, 16), torch.zeros(1, 4, 16), 1),
               lambda: w.whisper_logits(x, v, v, torch.zeros(8, 16), i32(1), 1, torch.zeros(256, dtype=torch.uint8)),
               lambda: w.whisper_pick(torch.zeros(256, dtype=torch.uint8), 8, i32(1, 4), 1, 0, 0, i32(1), i32(1), i32(1), i32(1))):
        with pytest.raises(P._lib.TdvcError, match='no CPU fallback'):
            fn()


def test_c_abi_refusals_need_no_device():
    """Every refusal is decided on the host before any launch: the calls below return their status without a GPU."""
    L = pkg()._lib
    lib = L.lib()
    buf = (C.c_float * 1100)()
    p = (C.addressof(buf) + 15) & ~15

    def lin(**kw):
        a = L.WhisperLinearArgs()
        a.B, a.N, a.K, a.x, a.x_bs, a.w, a.y, a.y_bs = 1, 16, 16, p, 16, p + 64, p + 2048, 16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.tdvc_whisper_linear_step(C.byref(a), None)
    assert lin(B=0) == 0 and lin(B=17) == EUNSUPPORTED and lin(N=24) == EUNSUPPORTED and lin(K=24) == EUNSUPPORTED
    assert lin(gamma=p, beta=p, K=1040, x_bs=1040) == EUNSUPPORTED and lin(gamma=p) == EINVAL and lin(epilogue=2) == EINVAL
    assert lin(x_bs=18) == EINVAL and lin(x_bs=8) == EINVAL and lin(y_bs=8) == EINVAL and lin(x=p + 4) == EINVAL and lin(w=None) == EINVAL and lin(B=-1) == EINVAL
    assert lin(y=p) == EINVAL and b'y must not be x' in lib.tdvc_last_error()
    assert lin(res=p, r_bs=8) == EINVAL
    cache = dict(N=48, cache_lo=16, cache_len=4, pos=p, k_cache=p, v_cache=p, c_bs=64)
    assert lin(**dict(cache, B=0)) == 0 and lin(**dict(cache, pos=None)) == EINVAL and lin(**dict(cache, v_cache=None)) == EINVAL
    assert lin(**dict(cache, c_bs=32)) == EINVAL and lin(**dict(cache, cache_lo=24)) == EINVAL and lin(**dict(cache, cache_lo=48)) == EINVAL
    assert lin(**dict(cache, res=p, r_bs=48)) == EINVAL
    mel = lambda B=1, Ln=400, ns=32000, nm=80, wb=1 << 30, x=p: lib.tdvc_whisper_log_mel(x, Ln, None, B, Ln, ns, p, nm, p, 0, 200, 1, p, wb, None)
    assert mel(B=0) == 0 and mel(ns=32001) == EUNSUPPORTED and mel(ns=320) == EUNSUPPORTED and mel(nm=129) == EUNSUPPORTED and mel(nm=0) == EUNSUPPORTED
    assert mel(wb=1000) == EINVAL and b'workspace' in lib.tdvc_last_error() and mel(x=None) == EINVAL and mel(Ln=-1) == EINVAL
    assert lib.tdvc_whisper_log_mel_workspace(2, 32000, 80) >= 2 * 200 * 80 * 8 + 2 * 25 * 8
    att = lambda B=1, T=4, Hh=1, d=16, ts=48, q=p: lib.tdvc_whisper_attention(q, p, p, 192, ts, B, T, Hh, d, p, 64, 16, None)
    assert att(B=0) == 0 and att(d=8) == EUNSUPPORTED and att(d=128) == EUNSUPPORTED and att(T=4097) == EUNSUPPORTED
    assert att(ts=8) == EINVAL and att(ts=50) == EINVAL and att(q=p + 4) == EINVAL and att(q=None) == EINVAL
    emb = lambda B=1, d=16, mp=4, ld=4, pos=p: lib.tdvc_whisper_embed(p, ld, pos, mp, p, p, B, d, 8, p, 16, None)
    assert emb(B=0) == 0 and emb(B=17) == EUNSUPPORTED and emb(d=1040) == EUNSUPPORTED and emb(d=24) == EUNSUPPORTED and emb(ld=2) == EINVAL and emb(pos=None) == EINVAL
    ast = lambda B=1, Hh=1, d=16, ln=4, ts=16, bs=64, q=p: lib.tdvc_whisper_attn_step(q, 16, p, p, bs, ts, None, ln, B, Hh, d, p, 16, None)
    assert ast(B=0) == 0 and ast(B=17) == EUNSUPPORTED and ast(d=48) == EUNSUPPORTED and ast(ln=4097, bs=4097 * 16) == EUNSUPPORTED
    assert ast(ln=0) == EINVAL and ast(ts=18) == EINVAL and ast(ts=8) == EINVAL and ast(bs=48) == EINVAL and ast(q=p + 4) == EINVAL and ast(q=None) == EINVAL
    off = (C.c_int64 * 4)()
    need = lib.tdvc_whisper_workspace(1024, 24, 51865, 1, 1500, 448, off)
    assert off[3] == (3242 + 2) // 3 and off[1] == 2 * 24 * 448 * 1024 * 4 and off[2] - off[1] == 2 * 24 * 1500 * 1024 * 4 == 294912000      # 295 MB per utterance
    assert need == off[2] + ((16 * off[3] * 8 + 255) & ~255) and lib.tdvc_whisper_workspace(0, 1, 1, 1, 1, 1, None) == 0
    nb = 16 * 13 * 8                                                         # vocab 203: 13 column tiles, one per workgroup
    lg = lambda B=1, d=16, V=203, np_=1, pb=nb, x=p, pos=p, x_bs=16: lib.tdvc_whisper_logits(x, x_bs, p, p, p, B, d, V, None, pos, np_, None, 0, p, pb, None)
    assert lg(B=0) == 0 and lg(B=17) == EUNSUPPORTED and lg(d=1040, x_bs=1040) == EUNSUPPORTED and lg(d=24, x_bs=24) == EUNSUPPORTED
    assert lg(pb=nb - 1) == EINVAL and b'workspace' in lib.tdvc_last_error() and lg(np_=0) == EINVAL and lg(pos=None) == EINVAL and lg(x_bs=8) == EINVAL
    pk = lambda B=1, V=203, ld=8, np_=2, tot=8, eos=3, pad=4, pb=nb, pos=p: lib.tdvc_whisper_pick(p, pb, V, B, p, ld, np_, tot, eos, pad, pos, p, p, p, None)
    assert pk(B=0) == 0 and pk(B=17) == EUNSUPPORTED and pk(ld=4) == EINVAL and pk(tot=1) == EINVAL and pk(eos=203) == EINVAL and pk(pad=-1) == EINVAL
    assert pk(pb=nb - 1) == EINVAL and pk(pos=None) == EINVAL


def test_wer_and_cer_on_hand_computed_cases():
    w = W()
    assert w.asr_wer(['a b c'], ['a b c']) == 0.0 and w.asr_cer(['abc'], ['abc']) == 0.0
    assert w.asr_wer([''], ['a b c']) == 1.0 and w.asr_cer([''], ['abc']) == 1.0          # an empty hypothesis: three deletions of three
    assert w.asr_wer(['a x b c y'], ['a b c']) == pytest.approx(2 / 3)                      # pure insertion
    assert w.asr_wer(['a c'], ['a b c']) == pytest.approx(1 / 3)                            # pure deletion
    assert w.asr_wer(['a d c'], ['a b c']) == pytest.approx(1 / 3)                          # substitution
    assert w.asr_cer(['a c'], ['abc']) == pytest.approx(1 / 3) and w.asr_cer(['ab  c'], ['ab c']) == pytest.approx(1 / 4)          # spaces are characters
    # the corpus total is not the mean of the per-sentence rates: (1 + 0) / (1 + 4) = 0.2, the mean is 0.5
    assert w.asr_wer(['x', 'a b c d'], ['y', 'a b c d']) == pytest.approx(0.2)
    assert w.asr_wer(['x', 'a b c d'], ['y', 'a b c d']) == pytest.approx(R.wer(['x', 'a b c d'], ['y', 'a b c d']))
    assert w.asr_cer(['kitten', 'flaw'], ['sitting', 'lawn']) == pytest.approx((3 + 2) / 11) == pytest.approx(R.cer(['kitten', 'flaw'], ['sitting', 'lawn']))
    with pytest.raises(ValueError):
        w.asr_wer(['a'], [''])
    with pytest.raises(ValueError):
        w.asr_wer(['a'], ['a', 'b'])


def test_report_aggregates_like_the_reference_script():
    w = W()
    conv = {'s1': {'s1': ['a b', 'c d e'], 's2': ['a x', 'c d']}, 's2': {'s1': ['f g'], 's2': ['f']}}
    orig = {'s1': ['a b', 'c d e'], 's2': ['f g']}
    refs = {'s1': ['a b', 'c d f'], 's2': ['f g h h']}
    r = w.asr_report(conv, orig, refs)
    assert r['wer_pair']['s1']['s1'] == 0.0 and r['wer_pair']['s1']['s2'] == pytest.approx(2 / 5) and r['wer_pair']['s2']['s1'] == 0.0
    assert r['wer_pair']['s2']['s2'] == pytest.approx(1 / 2)
    assert r['wer'] == pytest.approx((0 + 2 + 0 + 1) / (5 + 5 + 2 + 2))                     # a conversion is scored against the ORIGINAL's transcript
    assert r['orig_wer_single'] == {'s1': pytest.approx(1 / 5), 's2': pytest.approx(2 / 4)} and r['orig_wer'] == pytest.approx(3 / 9)
    assert r['cer_pair']['s1']['s2'] == pytest.approx((1 + 2) / 8) and r['orig_cer'] == pytest.approx((1 + 4) / (3 + 5 + 7))
    assert set(r) == {'wer_pair', 'cer_pair', 'wer', 'cer', 'orig_wer_single', 'orig_cer_single', 'orig_wer', 'orig_cer'}
