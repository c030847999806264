"""GPU: the Whisper ASR metric on the device (td-vc-gan_amd/whisper.py, csrc/asr_whisper.hip) against the float64 restatement
tests/whisper_ref.py, which tests/test_whisper_cpu.py pins to HF transformers' own output (tests/golden/whisper_small.npz).

Bars. An fp32 launch or network output: 4 x the largest error of stock torch's fp32 CPU evaluation of the same quantity against
float64, computed in the test (the bar of the LSTM, ECAPA and WavLM tests). A kernel that is float64 inside and rounds once (log_mel):
4 x 2^-24 x the row's largest magnitude. Token ids: equal, and the device's own teacher-forced logit error is asserted to be below half
the smallest top-2 margin of the fixture, so that equality is decided and not luck. Operands are strided views into NaN-filled
buffers where the kernel takes strides; the spare elements must still be NaN afterwards. Every test prints error / bar (run with -s).
Measured on an MI355X, worst error / bar: log_mel 0.20; attention 0.33; linear_step 0.59 (0.15 at 16 x 1024 x 1024 and at K = 4096, cache epilogue
0.32); attn_step 0.27; logits 0.25 (203) and 0.44 (51865); encode 0.14 and step_logits 0.27 on the fixture, 0.29 / 0.34 at head widths 16 and 64;
teacher-forced logit error 1.6e-5 against the smallest top-2 margin 1.4e-2.
"""
import functools
import os

import numpy as np
import pytest
import torch

import whisper_ref as R
from common import GOLDEN, pkg

pytestmark = pytest.mark.gpu
NAN = float('nan')
DEV = 'cuda:0'


def W():
    return pkg().whisper


def rnd(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def check32(got, fn, what, *args):
    """fn(*args) evaluated by stock torch on the CPU in float64 (the reference) and in float32 (its error is a quarter of the bar)."""
    ref = fn(*[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
    f32 = fn(*args)
    assert f32.dtype == torch.float32 and ref.dtype == torch.float64
    bar = 4.0 * float((f32.double() - ref).abs().max())
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    err = float((got - ref).abs().max())
    print(f'{what}: error {err:.3e} / bar {bar:.3e} = {err / max(bar, 1e-300):.3f}')
    assert err <= bar, (what, err, bar)
    return err / max(bar, 1e-300)


@functools.lru_cache(None)
def fixtures():
    return tuple(np.load(os.path.join(GOLDEN, n)) for n in ('whisper_small.npz', 'whisper_small_audio.npz', 'whisper_heads.npz'))


@functools.lru_cache(None)
def small():
    z, a, hz = fixtures()
    cfg, sd = R.load(z)
    m = W().Whisper(cfg)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m.to(DEV), cfg, sd


def gen_kw(z):
    return dict(suppress=z['suppress'].tolist(), begin_suppress=z['begin_suppress'].tolist(), eos=int(z['eos']), pad=int(z['pad']))


# ---------------------------------------------------------------------------------------------------------------- log_mel
def assert_mel(got, ref, what):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    bar = 4 * 2.0 ** -24 * np.abs(ref).max(axis=(1, 2), keepdims=True)
    ratio = float((np.abs(got - ref) / bar).max())
    print(f'{what}: error / bar {ratio:.3f}')
    assert ratio <= 1.0, (what, ratio)


def test_log_mel_fixture_rows_with_lengths_in_a_strided_view():
    _, a, _ = fixtures()
    x = torch.from_numpy(a['input'].astype(np.float32))
    whole = torch.full((3, 32000 + 48), NAN, device=DEV)
    view = whole[:, 16:32016]
    view.copy_(x)
    for b, n in enumerate(a['lengths']):
        view[b, int(n):] = NAN                                                # never read: a NaN would spread over the row through the maximum
    lengths = torch.tensor(a['lengths'], device=DEV)
    got = W().whisper_log_mel(view, lengths, chunk_length=2)
    assert tuple(got.shape) == (3, 80, 200)
    assert_mel(got, R.log_mel(a['input'], a['lengths'], n_samples=32000), 'log_mel, fixture rows with lengths')
    hf = np.abs(got.double().cpu().numpy() - a['features']).max()
    print(f'log_mel against HF numpy features (float32 inside): {hf:.3e}')
    assert hf <= 2.5e-7 + 2.0 ** -24 * 2                                      # the definition's distance from HF plus the store's rounding
    again = W().whisper_log_mel(view, lengths, chunk_length=2)
    assert torch.equal(got, again)
    alone = W().whisper_log_mel(view[2:3], lengths[2:3], chunk_length=2)
    assert torch.equal(alone[0], got[2])
    tm = torch.full((3, 202, 96), NAN, device=DEV)                            # the encoder's token-major interior
    W().whisper_log_mel(view, lengths, chunk_length=2, out=tm[:, 1:201, :80].transpose(1, 2))
    assert torch.equal(tm[:, 1:201, :80].transpose(1, 2), got) and int(torch.isnan(tm).sum()) == tm.numel() - got.numel()


def test_log_mel_zeros_truncation_and_short_rows():
    w = W()
    z = w.whisper_log_mel(torch.zeros(1, 5000, device=DEV), chunk_length=2)
    assert bool((z == -1.5).all())                                            # everything at the floor: (log10(1e-10) + 4) / 4
    x = rnd(5, 2, 40000, scale=0.1)
    got = w.whisper_log_mel(x.to(DEV), chunk_length=2)                        # longer than n_samples: truncated
    assert_mel(got, R.log_mel(x.numpy(), None, n_samples=32000), 'log_mel, rows longer than the chunk')
    assert torch.equal(got, w.whisper_log_mel(x[:, :32000].to(DEV), chunk_length=2))
    short = w.whisper_log_mel(x[:, :1000].to(DEV), torch.tensor([1000, 0], device=DEV), chunk_length=2)
    assert_mel(short, R.log_mel(x[:, :1000].numpy(), [1000, 0], n_samples=32000), 'log_mel, a short row and an empty one')
    assert bool((short[1] == -1.5).all())


def test_log_mel_thirty_seconds():
    t = torch.arange(480000, dtype=torch.float64) / 16000.0
    x = (0.2 * torch.sin(2 * np.pi * (150.0 * t + 40.0 * t * t)) + 0.01 * torch.randn(480000, generator=torch.Generator().manual_seed(9), dtype=torch.float64)).float()[None]
    got = W().whisper_log_mel(x.to(DEV), torch.tensor([400000], device=DEV))
    assert tuple(got.shape) == (1, 80, 3000)
    assert_mel(got, R.log_mel(x.numpy(), [400000], n_samples=480000), 'log_mel, 30 s (3000 frames)')


# -------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize('d', [16, 32, 64])
@pytest.mark.parametrize('T', [1, 63, 64, 65, 100])
def test_attention(T, d):
    heads, B = 2, 3
    Cc = heads * d
    qkv = rnd(T * 100 + d, B, T, 3 * Cc)
    qkv[..., :Cc] *= 2.0 * d ** -0.5                                         # scores of a few units: the running maximum moves between tiles
    if T > 70:
        qkv[:, 70, Cc:2 * Cc] = 3.0 * qkv[:, 3, :Cc]                          # key 70 leads query 3 by far: the maximum jumps in the second tile
    whole = torch.full((B, T + 2, 3 * Cc + 16), NAN, device=DEV)
    view = whole[:, 1:T + 1, :3 * Cc]
    view.copy_(qkv)
    ow = torch.full((B, T + 2, Cc + 16), NAN, device=DEV)
    out = W().whisper_attention(view, heads, out=ow[:, 1:T + 1, :Cc])
    assert int(torch.isnan(ow).sum()) == ow.numel() - out.numel()
    check32(out, lambda t: R.attend(t[..., :Cc], t[..., Cc:2 * Cc], t[..., 2 * Cc:], heads), f'attention T={T} d={d}', qkv)
    alone = W().whisper_attention(qkv[1:2].to(DEV), heads)
    assert torch.equal(alone[0], out[1]) and torch.equal(W().whisper_attention(view, heads), out)


# ------------------------------------------------------------------------------------------------------------ linear_step
def lin_ref(x, w, bias, gamma, beta, gelu, res, scale):
    if gamma is not None:
        mu = x.mean(-1, keepdim=True)
        x = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * gamma + beta
    y = x @ w.t()
    if bias is not None:
        y = y + bias
    if scale is not None:
        y = torch.cat([y[:, :scale[0]], y[:, scale[0]:scale[1]] * scale[2], y[:, scale[1]:]], 1)
    if gelu:
        y = R.gelu(y)
    return y if res is None else y + res


MODES = ('plain', 'gelu', 'residual', 'norm', 'norm_gelu', 'nobias', 'scale')


@pytest.mark.parametrize('N,K', [(64, 64), (256, 64), (64, 256), (48, 80), (32, 1040)])
@pytest.mark.parametrize('B', [1, 3, 16])
def test_linear_step(B, N, K):
    w_ = W()
    worst = 0.0
    for mi, mode in enumerate(MODES):
        seed = 1000 * B + N + K + mi
        x, w, b = rnd(seed, B, K), rnd(seed + 1, N, K, scale=K ** -0.5), rnd(seed + 2, N)
        gamma, beta = (1.0 + 0.3 * rnd(seed + 3, K), 0.3 * rnd(seed + 4, K)) if mode.startswith('norm') else (None, None)
        if gamma is not None and K > 1024:
            with pytest.raises(ValueError, match='1024'):
                w_.whisper_linear_step(x.to(DEV), w.to(DEV), b.to(DEV), norm=(gamma.to(DEV), beta.to(DEV)))
            continue
        res = rnd(seed + 5, B, N) if mode == 'residual' else None
        bias = None if mode == 'nobias' else b
        scale = (16, 32, 0.25) if mode == 'scale' else None
        xw = torch.full((B + 2, K + 16), NAN, device=DEV)
        xv = xw[1:B + 1, :K]
        xv.copy_(x)
        ow = torch.full((B + 2, N + 16), NAN, device=DEV)
        ov = ow[1:B + 1, :N]
        if res is not None:
            ov.copy_(res)                                                     # the residual is the output buffer, as in the step
        out = w_.whisper_linear_step(xv, w.to(DEV), None if bias is None else bias.to(DEV), norm=None if gamma is None else (gamma.to(DEV), beta.to(DEV)),
                                     epilogue=w_.EPI_GELU if 'gelu' in mode else w_.EPI_NONE, residual=ov if res is not None else None, out=ov, scale=scale)
        assert int(torch.isnan(ow).sum()) == ow.numel() - out.numel() and int(torch.isnan(xw).sum()) == xw.numel() - xv.numel()
        worst = max(worst, check32(out, lambda *a: lin_ref(*a, 'gelu' in mode, None if res is None else a[0].new_tensor(res.numpy()), scale),
                                   f'linear_step B={B} N={N} K={K} {mode}', x, w, bias, gamma, beta))
        r = B // 2                                                            # a row alone gets the bits it gets in the batch
        alone = w_.whisper_linear_step(x[r:r + 1].to(DEV), w.to(DEV), None if bias is None else bias.to(DEV),
                                       norm=None if gamma is None else (gamma.to(DEV), beta.to(DEV)), epilogue=w_.EPI_GELU if 'gelu' in mode else w_.EPI_NONE,
                                       residual=None if res is None else res[r:r + 1].to(DEV), scale=scale)
        assert torch.equal(alone[0], out[r]), mode
    print(f'linear_step B={B} N={N} K={K}: worst error / bar {worst:.3f}')


def test_linear_step_whisper_medium_shapes():
    w_ = W()
    x, w, b, g, be = rnd(1, 16, 1024), rnd(2, 1024, 1024, scale=1 / 32), rnd(3, 1024), 1.0 + 0.3 * rnd(4, 1024), 0.3 * rnd(5, 1024)
    out = w_.whisper_linear_step(x.to(DEV), w.to(DEV), b.to(DEV), norm=(g.to(DEV), be.to(DEV)))
    check32(out, lambda *a: lin_ref(*a, False, None, None), 'linear_step 16 x 1024 x 1024 with the LayerNorm prologue', x, w, b, g, be)
    x4, w4 = rnd(6, 16, 4096), rnd(7, 64, 4096, scale=1 / 64)                  # fc2's reduction: four chunks of the input rows
    out = w_.whisper_linear_step(x4.to(DEV), w4.to(DEV), b[:64].to(DEV), epilogue=w_.EPI_GELU)
    check32(out, lambda *a: lin_ref(*a, None, None, True, None, None), 'linear_step 16 x 64 x 4096 + GELU', x4, w4, b[:64])
    assert torch.equal(out, w_.whisper_linear_step(x4.to(DEV), w4.to(DEV), b[:64].to(DEV), epilogue=w_.EPI_GELU))


@pytest.mark.parametrize('p', [0, 5, 11])
def test_linear_step_cache_epilogue(p):
    w_ = W()
    B, d, Lc = 3, 32, 12
    x, w, b = rnd(p, B, d), rnd(p + 1, 3 * d, d, scale=d ** -0.5), rnd(p + 2, 3 * d)
    g, be = 1.0 + 0.3 * rnd(p + 3, d), 0.3 * rnd(p + 4, d)
    cache = torch.full((2, B, Lc, d), NAN, device=DEV)
    pos = torch.tensor([p], dtype=torch.int32, device=DEV)
    q = w_.whisper_linear_step(x.to(DEV), w.to(DEV), b.to(DEV), norm=(g.to(DEV), be.to(DEV)), scale=(0, d, d ** -0.5), cache=(cache[0], cache[1], pos, d))
    assert tuple(q.shape) == (B, d) and int(pos) == p
    got = torch.cat([q, cache[0, :, p], cache[1, :, p]], 1)
    check32(got, lambda *a: lin_ref(*a, False, None, (0, d, d ** -0.5)), f'linear_step cache epilogue at p={p}', x, w, b, g, be)
    assert int(torch.isnan(cache).sum()) == cache.numel() - 2 * B * d          # every other position untouched


# -------------------------------------------------------------------------------------------------------------- attn_step
@pytest.mark.parametrize('d', [16, 32, 64])
@pytest.mark.parametrize('ln,cross', [(1, False), (2, False), (63, False), (64, False), (65, False), (100, True), (1500, True)])
def test_attn_step(ln, cross, d):
    w_ = W()
    heads, B = 2, 3
    Cc = heads * d
    q, k, v = rnd(ln + d, B, Cc, scale=2.0 * d ** -0.5), rnd(ln + d + 1, B, ln, Cc), rnd(ln + d + 2, B, ln, Cc)
    k[:, ln // 2] = 2.0 * q / (2.0 * d ** -0.5)                              # one key leads: the waves' maxima differ
    cap = ln if cross else 80
    kv = torch.full((B, cap, 2 * Cc + 16), NAN, device=DEV)                   # k | v side by side, NaN behind len and beside
    kv[:, :ln, :Cc], kv[:, :ln, Cc:2 * Cc] = k.to(DEV), v.to(DEV)
    pos = None if cross else torch.tensor([ln - 1], dtype=torch.int32, device=DEV)
    ow = torch.full((B + 1, Cc + 16), NAN, device=DEV)
    out = w_.whisper_attn_step(q.to(DEV), kv[:, :, :Cc], kv[:, :, Cc:2 * Cc], heads, pos=pos, out=ow[:B, :Cc])
    assert int(torch.isnan(ow).sum()) == ow.numel() - out.numel()
    check32(out, lambda a, b_, c: R.attend(a[:, None], b_, c, heads)[:, 0], f'attn_step len={ln} d={d} {"cross" if cross else "self"}', q, k, v)
    alone = w_.whisper_attn_step(q[1:2].to(DEV), kv[1:2, :, :Cc], kv[1:2, :, Cc:2 * Cc], heads, pos=pos)
    assert torch.equal(alone[0], out[1])


# ----------------------------------------------------------------------------------------------------------- logits, pick
def read_partials(partials, nwg, B):
    pm = partials[:64 * nwg].view(torch.float32).view(16, nwg)[:B].cpu()
    pa = partials[64 * nwg:128 * nwg].view(torch.int32).view(16, nwg)[:B].cpu()
    return pm, pa


def best_of(pm, pa):
    out = []
    for b in range(pm.shape[0]):
        top = pm[b].max()
        out.append(int(pa[b][pm[b] == top].min()))
    return out


@pytest.mark.parametrize('V', [203, 51865])
def test_logits_partials_suppression_and_ties(V):
    w_ = W()
    B, d, P = 3, 64, 4
    nwg = w_.partial_count(V)
    assert nwg == (13 if V == 203 else 1081)
    x, E, g, be = rnd(V, B, d), rnd(V + 1, V, d, scale=d ** -0.5), 1.0 + 0.3 * rnd(V + 2, d), 0.3 * rnd(V + 3, d)
    partials = torch.zeros(16 * nwg * 8, dtype=torch.uint8, device=DEV)
    pos = torch.tensor([7], dtype=torch.int32, device=DEV)
    logits = torch.full((B, V + 5), NAN, device=DEV)
    w_.whisper_logits(x.to(DEV), g.to(DEV), be.to(DEV), E.to(DEV), pos, P, partials, logits=logits[:, :V])
    assert int(torch.isnan(logits).sum()) == 5 * B
    check32(logits[:, :V], lambda a, e, gg, bb: lin_ref(a, e, None, gg, bb, False, None, None), f'logits V={V}', x, E, g, be)
    dev_logits = logits[:, :V].cpu()
    assert best_of(*read_partials(partials, nwg, B)) == dev_logits.argmax(1).tolist()
    # suppression: the three leaders of every row (bit 0), and the next one only at the first generated step (bit 1)
    order = dev_logits.argsort(1, descending=True)
    mask = torch.zeros(V, dtype=torch.uint8)
    mask[order[:, :3].reshape(-1)] |= 1
    mask[order[:, 3]] |= 2
    allowed = lambda bits: [int(next(t for t in order[b].tolist() if not int(mask[t]) & bits)) for b in range(B)]
    w_.whisper_logits(x.to(DEV), g.to(DEV), be.to(DEV), E.to(DEV), pos, P, partials, mask=mask.to(DEV))      # logits = NULL
    assert best_of(*read_partials(partials, nwg, B)) == allowed(1)
    pos.fill_(P - 1)
    w_.whisper_logits(x.to(DEV), g.to(DEV), be.to(DEV), E.to(DEV), pos, P, partials, mask=mask.to(DEV))
    assert best_of(*read_partials(partials, nwg, B)) == allowed(3) != allowed(1)
    # exact ties: identical embedding rows give identical logits; inside one workgroup and across workgroups the lowest index wins
    lead = 4.0 * E[dev_logits.argmax(1)[0]]
    far = V - 3
    for toks in ((far, 37, 41), (far, 41)):
        E2 = E.clone()
        E2[list(toks)] = lead
        w_.whisper_logits(x[:1].to(DEV), g.to(DEV), be.to(DEV), E2.to(DEV), pos, P, partials, logits=logits[:1, :V])
        row = logits[0, :V].cpu()
        assert float(row[toks[0]]) == float(row[toks[1]]) == float(row.max())
        pm, pa = read_partials(partials, nwg, 1)
        assert best_of(pm, pa) == [min(toks)] and int((pm[0] == pm[0].max()).sum()) >= 2      # the tie spans two partials


def test_pick_forced_prompt_eos_pad_and_counter():
    w_ = W()
    V, B, P, total, eos, pad = 203, 2, 2, 6, 200, 201
    nwg = w_.partial_count(V)
    partials = torch.zeros(16 * nwg * 8, dtype=torch.uint8, device=DEV)
    pm = partials[:64 * nwg].view(torch.float32).view(16, nwg)
    pa = partials[64 * nwg:128 * nwg].view(torch.int32).view(16, nwg)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    ids = torch.full((B, total + 2), -1, dtype=torch.int32, device=DEV)[:, :total]
    ids[:, :P] = i32(196, 197)
    pos, n_tokens, finished, all_done = i32(0), i32(P, P), i32(0, 0), i32(0)

    def step(row0, row1):
        pm.fill_(-1.0)
        for b, (tok, wg) in enumerate((row0, row1)):
            pm[b, wg], pa[b, wg] = 3.0, tok
            pm[b, (wg + 5) % nwg], pa[b, (wg + 5) % nwg] = 3.0, tok + 7       # an equal maximum with a higher index in another partial
        w_.whisper_pick(partials, V, ids, P, eos, pad, pos, n_tokens, finished, all_done)
    step((9, 1), (10, 2))                                                     # p = 0: the next token is the prompt's
    assert ids.tolist() == [[196, 197, -1, -1, -1, -1]] * 2 and int(pos) == 1 and n_tokens.tolist() == [2, 2]
    step((9, 1), (10, 12))                                                    # p = 1: the first generated token
    assert ids[:, 2].tolist() == [9, 10] and int(pos) == 2 and n_tokens.tolist() == [3, 3] and int(all_done) == 0
    step((eos, 3), (11, 0))                                                   # row 0 ends
    assert ids[:, 3].tolist() == [eos, 11] and finished.tolist() == [1, 0] and n_tokens.tolist() == [4, 4] and int(all_done) == 0
    step((50, 3), (eos, 4))                                                   # row 0 emits pad whatever its argmax; row 1 ends
    assert ids[:, 4].tolist() == [pad, eos] and n_tokens.tolist() == [4, 5] and int(all_done) == 1 and int(pos) == 4
    step((50, 3), (51, 4))
    assert ids[:, 5].tolist() == [pad, pad] and int(pos) == 5 and n_tokens.tolist() == [4, 5]
    step((50, 3), (51, 4))                                                    # no slot left: nothing moves
    assert int(pos) == 5 and ids.tolist() == [[196, 197, 9, eos, pad, pad], [196, 197, 10, 11, eos, pad]]
    assert ids._base.tolist()[0][total:] == [-1, -1]


# -------------------------------------------------------------------------------------------------------------- end to end
def test_encode_and_step_logits_against_the_fixture():
    z, a, hz = fixtures()
    m, cfg, sd = small()
    feats = torch.from_numpy(a['features'])
    enc = m.encode(feats.to(DEV))
    check32(enc, lambda f: R.encode(R_cast(sd, f.dtype), cfg, f), 'encode (fixture)', feats)
    assert float((enc.double().cpu() - torch.from_numpy(z['enc'])).abs().max()) < 1e-3
    assert torch.equal(m.encode(feats[1:2].to(DEV))[0], enc[1]) and torch.equal(m.encode(feats.to(DEV)), enc)
    ench = torch.from_numpy(z['enc']).float()
    ids = torch.from_numpy(z['ids'])
    logits = m.step_logits(ench.to(DEV), ids)
    check32(logits, lambda e: R.step_logits(R_cast(sd, e.dtype), cfg, e, ids), 'step_logits (fixture)', ench)
    err = float((logits.double().cpu() - torch.from_numpy(z['logits'])).abs().max())
    margin = float(np.nanmin(z['margins']))
    print(f'teacher-forced logit error {err:.3e} against the smallest top-2 margin {margin:.3e}')
    assert err < 0.5 * margin
    for tag in ('w16/', 'w64/'):
        c, s = R.load(hz, tag)
        mh = W().Whisper(c)
        mh.load_state_dict({k: v.float() for k, v in s.items()}, strict=True)
        mh = mh.to(DEV)
        e = mh.encode(feats[1:2].to(DEV))
        check32(e, lambda f: R.encode(R_cast(s, f.dtype), c, f), f'encode, head width {tag[1:3]}', feats[1:2])
        eh, hid = torch.from_numpy(hz[tag + 'enc']).float()[None], torch.from_numpy(hz[tag + 'ids'])
        check32(mh.step_logits(eh.to(DEV), hid), lambda t: R.step_logits(R_cast(s, t.dtype), c, t, hid), f'step_logits, head width {tag[1:3]}', eh)


def R_cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def test_generate_equals_the_fixture_in_every_mode():
    z, a, _ = fixtures()
    m, cfg, sd = small()
    feats = torch.from_numpy(a['features']).to(DEV)
    prompt, kw = z['prompt'].tolist(), gen_kw(z)
    want, want_n = torch.from_numpy(z['ids']), torch.from_numpy(z['n_tokens'])
    ids, n = m.generate(feats, prompt, 28, **kw)                              # graph=True
    assert ids.dtype == n.dtype == torch.int32 and torch.equal(ids.cpu(), want) and torch.equal(n.cpu(), want_n)      # every step of every row
    eager = m.generate(feats, prompt, 28, graph=False, **kw)
    assert torch.equal(eager[0], ids) and torch.equal(eager[1], n)
    again = m.generate(feats, prompt, 28, **kw)
    assert torch.equal(again[0], ids) and torch.equal(again[1], n)
    for b in range(3):                                                        # a row alone gets the ids it gets in the batch
        one = m.generate(feats[b:b + 1], prompt, 28, **kw)
        assert torch.equal(one[0][0], ids[b]) and int(one[1][0]) == int(n[b])
    chk = m.generate(feats, prompt, 28, check_every=4, **kw)
    assert torch.equal(chk[0], ids) and torch.equal(chk[1], n)
    early = m.generate(feats[:1], prompt, 28, check_every=4, **kw)             # the row that ends at its eos: the loop stops early
    assert torch.equal(early[0][0], ids[0]) and int(early[1][0]) == int(n[0]) < 32
    enc = m.encode(feats)
    tids = torch.from_numpy(z['ids'])
    lg, le = m.step_logits(enc, tids, graph=True), m.step_logits(enc, tids, graph=False)
    assert torch.equal(lg, le) and torch.equal(m.step_logits(enc, tids, graph=True), lg)          # the same bits, replayed or launched, call after call
    x = torch.from_numpy(a['input'].astype(np.float32)).to(DEV)
    tr = m.transcribe(x, torch.tensor(a['lengths'], device=DEV), prompt, 28, **kw)
    assert torch.equal(tr[0], ids) and torch.equal(tr[1], n)

    class Tok:
        def decode(self, toks, skip_special_tokens=True):
            return ' '.join(str(t) for t in toks)
    texts = m.transcribe(x, torch.tensor(a['lengths'], device=DEV), prompt, 28, tokenizer=Tok(), **kw)[2]
    assert texts == [' '.join(str(t) for t in z['ids'][b, 4:int(z['n_tokens'][b])] if t != int(z['eos'])) for b in range(3)]


def test_generate_splits_batches_above_sixteen_rows():
    z, a, _ = fixtures()
    m, cfg, sd = small()
    enc = torch.from_numpy(z['enc']).float().to(DEV)
    big = enc[[0, 1, 2] * 6]                                                  # 18 rows: 16 + 2
    ids, n = m.generate(None, z['prompt'].tolist(), 28, encoder_output=big, **gen_kw(z))
    want = torch.from_numpy(z['ids'])[[0, 1, 2] * 6]
    assert tuple(ids.shape) == (18, 32) and torch.equal(ids.cpu(), want)


def test_refusals_through_python():
    w_ = W()
    m, cfg, sd = small()
    z = lambda *s: torch.zeros(*s, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='16 rows'):
        w_.whisper_linear_step(z(17, 16), z(16, 16))
    with pytest.raises(ValueError, match='multiples of 16'):
        w_.whisper_linear_step(z(1, 24), z(16, 24))
    with pytest.raises(ValueError, match='head width'):
        w_.whisper_attn_step(z(1, 48), z(1, 4, 48), z(1, 4, 48), 1)
    with pytest.raises(ValueError, match='4096'):
        w_.whisper_attn_step(z(1, 16), z(1, 4097, 16), z(1, 4097, 16), 1)
    with pytest.raises(ValueError, match='head width'):
        w_.whisper_attention(z(1, 4, 24), 1)
    with pytest.raises(ValueError, match='4096'):
        w_.whisper_attention(z(1, 4097, 48), 1)
    with pytest.raises(ValueError, match='mel bands'):
        w_.whisper_log_mel(z(1, 400), chunk_length=1, n_mels=129)
    with pytest.raises(ValueError, match='16 rows'):
        w_.whisper_embed(i32(17, 4), i32(1), z(8, 16), z(4, 16))
    with pytest.raises(ValueError, match='max_target_positions'):
        m.generate(z(1, 80, 200), [196], 32)
    with pytest.raises(ValueError, match='features must be'):
        m.encode(z(1, 80, 300))
    with pytest.raises(ValueError, match='chunk'):
        m.transcribe(z(1, 400), None, [196], 2, chunk_length=30)
    assert tuple(m.generate(z(0, 80, 200), [196], 3)[0].shape) == (0, 4) and tuple(m.encode(z(0, 80, 200)).shape) == (0, 100, 64)
