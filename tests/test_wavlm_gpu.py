"""GPU: the WavLM feature extractor on the device (td-vc-gan_amd/wavlm.py, csrc/ssl_wavlm.hip) against the float64 restatement
tests/wavlm_ref.py, which tests/test_wavlm_cpu.py pins to the reference's own output (tests/golden/wavlm_small.npz).

Bars. (a) A pure fp32 chain (gemm, posconv, attention): the project's element-wise bar of edge_support.elem_check,
|got - ref| <= (n + slack) 2^-23 A + 2^-22 |ref| with A the sum of the absolute values of the terms of that element and n the length of
its reduction; an erf-GELU behind the sum is 1.13-Lipschitz and costs a few roundings of its own (A x 1.13, slack 16), a residual adds
its magnitude to A. For the attention A_t = sum_s p_s |v_s| and the bound also carries twice the absolute error E_t an fp32 score can
have, because the exponential turns an absolute error of its argument into a relative error of p (numerator and denominator):
E_t = max_s (d + 4) 2^-23 (sum_c |q_c k_c| + |gate bias|) + 2^-23 (|score_s| + |max score|). (b) A kernel that is float64 inside and
rounds once (conv0, layernorm, the gates): 4 x 2^-24 x the largest magnitude of the row (the fbank bar). (c) Network-level outputs:
4 x the error of stock torch's fp32 CPU evaluation of the same weights (wavlm_ref in float32) against float64, computed here: the
bar of the LSTM and ECAPA tests.
Every operand is a strided view into a NaN-filled buffer (spare tokens in front and behind, spare channels beside); after the call
the spare elements must still be NaN and the output finite. Every test prints error / bar (run with -s).
Measured on an MI355X, worst error / bar: gemm 0.09 (each epilogue, both tile heights), as a strided convolution 0.02, into the padded
interior 0.04; conv0 0.22-0.25; layernorm 0.19-0.25, gates 0.18-0.22; posconv 0.001-0.003; attention 0.003-0.013 (0.000 where one key leads by
80 and where gate x bias reaches +-400: the score-error term dominates those bars), 1.6e-6 at scale 1.06 for 1100 tokens; extract_features on
the fixture 0.28 (final), 0.20 / 0.20 (output_layer 1, 2), 0.20 (ret_conv); two heads of width 64: 0.17; SSLEncoder.features: 0.16.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wavlm_ref as R
from common import GOLDEN, pkg
from edge_support import U, elem_check, poison_lds

pytestmark = pytest.mark.gpu
NAN = float('nan')


def W():
    return pkg().wavlm


def guarded(B, T, Cc, dev, src=None):
    """(whole, view): view [B, T, Cc] inside a NaN-filled [B, T + 2, Cc + 16] buffer (token stride Cc + 16, one spare token on each side)."""
    whole = torch.full((B, T + 2, Cc + 16), NAN, dtype=torch.float32, device=dev)
    view = whole[:, 1:T + 1, :Cc]
    if src is not None:
        view.copy_(src.to(dev))
    return whole, view


def spare_intact(whole, view):
    return int(torch.isnan(whole).sum()) == whole.numel() - view.numel() and bool(torch.isfinite(view).all())


def assert_close_elementwise(got, ref, A, n, what, slack=8):
    ratio, inexact = elem_check(got, ref, A, n, slack)
    print(f'{what}: error / bar {ratio:.3f}')
    assert ratio <= 1.0 and inexact == 0, (what, ratio, inexact)
    return ratio


def assert_rows_close(got, ref, what):
    """float64 inside, one rounding: 4 x 2^-24 x the row's largest magnitude."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    bar = 4 * 2.0 ** -24 * ref.abs().amax(-1, keepdim=True)
    err = (got - ref).abs()
    assert bool((err[(bar == 0).expand_as(err)] == 0).all()), what
    ratio = float((err / bar.clamp_min(1e-300)).max())
    print(f'{what}: error / bar {ratio:.3f}')
    assert ratio <= 1.0, (what, ratio)
    return ratio


def rnd(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


# ------------------------------------------------------------------------------------------------------------------- gemm
def gemm_case(dev, mode, B, K, T, N):
    w_ = W()
    seed = K + 7 * T + N
    x, w, b = rnd(seed, B, T, K), rnd(seed + 1, N, K, scale=K ** -0.5), rnd(seed + 2, N)
    res = rnd(seed + 3, B, T, N) if mode.startswith('residual') else None
    xw, xv = guarded(B, T, K, dev, x)
    ow, ov = guarded(B, T, N, dev)
    kw = {}
    if mode == 'gelu':
        kw['epilogue'] = w_.EPI_GELU
    if mode == 'scale':
        kw['scale'] = (16, 32, 0.25)
    if mode == 'residual':
        rw, rv = guarded(B, T, N, dev, res)
        kw['residual'] = rv
    if mode == 'residual_is_out':
        ov.copy_(res.to(dev))
        kw['residual'] = ov
    out = w_.wavlm_gemm(xv, w.to(dev), b.to(dev), out=ov, **kw)
    assert out.data_ptr() == ov.data_ptr() and spare_intact(ow, ov), (K, T, N)
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() + b.double()
    A = xd.abs() @ wd.abs().t() + b.double().abs()
    slack = 8
    if mode == 'scale':
        mul = torch.ones(N, dtype=torch.float64)
        mul[16:32] = 0.25
        ref, A = ref * mul, A * mul
    if mode == 'gelu':
        ref, A, slack = R.gelu(ref), 1.13 * A, 16
    if res is not None:
        ref, A = ref + res.double(), A + res.double().abs()
    return assert_close_elementwise(ov, ref, A, K, f'gemm {mode} B={B} K={K} T={T} N={N}', slack)


@pytest.mark.parametrize('mode', ['none', 'gelu', 'residual', 'residual_is_out', 'scale'])
def test_gemm_against_float64(dev, mode):
    poison_lds(dev)
    cases = [(2, K, T, N) for K in (16, 64, 4096) for T in (1, 63, 64, 65, 130) for N in (16, 48, 64, 80)
             if K != 4096 or (T, N) in ((1, 16), (65, 80), (130, 48))]
    cases += [(16, 16, 65, 1024), (64, 64, 130, 208)]                         # 512 workgroups and more: the 64-token tile (32 below)
    worst = max(gemm_case(dev, mode, *case) for case in cases)
    print(f'gemm {mode}: worst error / bar {worst:.3f}')


@pytest.mark.parametrize('k,cin,to', [(3, 16, 1), (3, 16, 64), (3, 16, 65), (2, 24, 1), (2, 24, 130)])
def test_gemm_as_strided_convolution(dev, k, cin, to):
    """K = k Cin = 48: a stride-2 Conv1d over token-major input whose last window ends on the last token; NaN follows that token."""
    w_ = W()
    stride, N, B = 2, 32, 2
    T = stride * (to - 1) + k
    x, cw = rnd(to + k, B, T, cin), rnd(to + k + 1, N, cin, k, scale=(k * cin) ** -0.5)
    flat = torch.full((B, T * cin + 32), NAN, device=dev)
    flat[:, :T * cin] = x.reshape(B, -1).to(dev)
    xv = flat[:, :T * cin].unflatten(1, (T, cin))
    assert xv.stride() == (T * cin + 32, cin, 1)
    ow, ov = guarded(B, to, N, dev)
    poison_lds(dev)
    w_.wavlm_gemm(xv, w_.permute_conv(cw).to(dev), None, kernel=k, stride=stride, out=ov)
    assert spare_intact(ow, ov)
    ref = F.conv1d(x.double().transpose(1, 2), cw.double(), stride=stride).transpose(1, 2)
    A = F.conv1d(x.double().abs().transpose(1, 2), cw.double().abs(), stride=stride).transpose(1, 2)
    assert_close_elementwise(ov, ref, A, k * cin, f'gemm as conv k={k} Cin={cin} T\'={to}')


def test_gemm_writes_into_a_padded_buffer_and_b0_is_a_noop(dev):
    w_ = W()
    B, T, K, N, pad = 2, 65, 32, 64, 8
    x, w, b = rnd(1, B, T, K), rnd(2, N, K, scale=K ** -0.5), rnd(3, N)
    xp = torch.zeros(B, T + 2 * pad - 1, N, device=dev)
    inner = xp[:, pad:pad + T]
    w_.wavlm_gemm(x.to(dev), w.to(dev), b.to(dev), out=inner)
    assert bool((xp[:, :pad] == 0).all()) and bool((xp[:, pad + T:] == 0).all())          # the border stays untouched
    ref = x.double() @ w.double().t() + b.double()
    assert_close_elementwise(inner, ref, x.double().abs() @ w.double().abs().t() + b.double().abs(), K, 'gemm into the padded interior')
    out = torch.full((0, T, N), NAN, device=dev)
    assert w_.wavlm_gemm(torch.zeros(0, T, K, device=dev), w.to(dev), b.to(dev), out=out).shape == (0, T, N)
    with pytest.raises(pkg()._lib.TdvcError, match='residual'):                               # a residual that is `out` with other strides
        buf = torch.zeros(B, 2 * T, N, device=dev)
        w_.wavlm_gemm(x.to(dev), w.to(dev), b.to(dev), out=buf[:, :T], residual=buf[:, :T].as_strided((B, T, N), (2 * T * N, 2 * N, 1)))
    with pytest.raises(ValueError, match='multiples of 16'):
        w_.wavlm_gemm(torch.zeros(1, 4, 24, device=dev), torch.zeros(16, 24, device=dev))


# ------------------------------------------------------------------------------------------------------------------ conv0
@pytest.mark.parametrize('n,cc', [(400, 32), (404, 32), (405, 32), (405, 512), (8160, 32)])
def test_conv0_against_float64(dev, n, cc):
    w_ = W()
    B, k, s = 3, 10, 5
    x = rnd(n, B, n, scale=10.0 ** -1.5)
    x[2] = 0.0                                                               # variance 0: the output is gelu(beta)
    cw, g, b = rnd(n + 1, cc, 1, k, scale=0.45), 1.0 + rnd(n + 2, cc, scale=0.3), rnd(n + 3, cc, scale=0.3)
    T = (n - k) // s + 1
    flat = torch.full((2 * B, n + 3), NAN, device=dev)
    flat[::2, :n] = x.to(dev)
    ow, ov = guarded(B, T, cc, dev)
    w_.wavlm_conv0(flat[::2, :n], cw[:, 0, :].t().contiguous().to(dev), g.to(dev), b.to(dev), s, out=ov)
    assert spare_intact(ow, ov)
    raw = F.conv1d(x.double()[:, None], cw.double(), stride=s).transpose(1, 2)
    ref = R.gelu(R.layer_norm(raw, g.double(), b.double()))
    assert ref.shape == (B, T, cc)
    assert_rows_close(ov, ref, f'conv0 L={n} C={cc}')
    assert float((ov[2].double().cpu() - R.gelu(b.double())[None]).abs().max()) <= 2.0 ** -24 * float(b.abs().max())


# -------------------------------------------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize('cc', [32, 64, 512, 1024])
@pytest.mark.parametrize('gelu', [False, True])
def test_layernorm_against_float64(dev, cc, gelu):
    w_ = W()
    B, T = 2, 37
    x = rnd(cc, B, T, cc, scale=3.0) + 5.0
    x[0, 3] = 2.5                                                            # constant rows: variance 0, the output is beta
    x[1, 36] = 0.0
    g, b = 1.0 + rnd(cc + 1, cc, scale=0.3), rnd(cc + 2, cc, scale=0.3)
    xw, xv = guarded(B, T, cc, dev, x)
    ow, ov = guarded(B, T, cc, dev)
    w_.wavlm_layernorm(xv, g.to(dev), b.to(dev), gelu=gelu, out=ov)
    assert spare_intact(ow, ov)
    ref = R.layer_norm(x.double(), g.double(), b.double())
    ref = R.gelu(ref) if gelu else ref
    assert_rows_close(ov, ref, f'layernorm C={cc} gelu={gelu}')
    w_.wavlm_layernorm(xv, g.to(dev), b.to(dev), gelu=gelu, out=xv)          # in place: the same bits
    assert torch.equal(xv, ov) and spare_intact(xw, xv)


@pytest.mark.parametrize('cc,heads', [(64, 4), (128, 2), (512, 16)])
def test_layernorm_gates_against_the_restatement(dev, cc, heads):
    w_ = W()
    B, T, d = 2, 33, cc // heads
    x = rnd(cc, B, T, cc, scale=2.0)
    g, b = 1.0 + rnd(cc + 1, cc, scale=0.3), rnd(cc + 2, cc, scale=0.3)
    gw, gb = rnd(cc + 3, 8, d, scale=d ** -0.5), rnd(cc + 4, 8, scale=0.3)
    gw[:, 0] *= 6.0
    gw[0:2] *= 25.0                                                          # |u0 + .. + u3| reaches 40 and beyond: a saturated sigmoid
    ga = rnd(cc + 5, heads) + 0.2
    ga[0] = -1.5                                                             # grep_a negative
    h, gate = w_.wavlm_layernorm(x.to(dev), g.to(dev), b.to(dev), grep=(gw.to(dev), gb.to(dev), ga.to(dev)))
    assert_rows_close(h, R.layer_norm(x.double(), g.double(), b.double()), f'layernorm with gates C={cc}')
    hd = h.double().cpu()                                                    # the gates are computed from the stored row
    u = hd.reshape(B, T, heads, d) @ gw.double().t() + gb.double()
    assert float(u[..., :4].sum(-1).abs().max()) > 40.0 and float(u[..., :4].sum(-1).abs().min()) < 1.0
    ref = R.gates(hd, gw.double(), gb.double(), ga.double().reshape(1, heads, 1, 1), heads)
    assert gate.shape == (B, heads, T) and float(ref.min()) < 1.0 and float(ref.max()) > 1.9
    assert_rows_close(gate, ref, f'gates C={cc} H={heads}')


# ---------------------------------------------------------------------------------------------------------------- posconv
@pytest.mark.parametrize('T,cc,k,groups', [(1, 64, 16, 4), (2, 64, 16, 4), (15, 64, 16, 4), (16, 64, 16, 4), (17, 64, 16, 4), (130, 64, 16, 4),
                                           (5, 256, 128, 16)])
def test_posconv_against_float64(dev, T, cc, k, groups):
    w_ = W()
    B = 2
    x = rnd(T + k, B, T, cc)
    wg, wv, bias = 1.0 + rnd(T + 1, 1, 1, k, scale=0.3), rnd(T + 2, cc, cc // groups, k, scale=(k * cc // groups) ** -0.5), rnd(T + 3, cc, scale=0.3)
    folded = w_.fold_pos_conv(wg, wv)                                        # fp32 [C][K][C / G]: the operand the launch gets
    xp = torch.zeros(B, T + k - 1, cc, device=dev)
    xp[:, k // 2:k // 2 + T] = x.to(dev)
    before = xp.clone()
    ow, ov = guarded(B, T, cc, dev)
    poison_lds(dev)
    w_.wavlm_posconv(xp, folded.to(dev), bias.to(dev), k, groups, out=ov)
    assert spare_intact(ow, ov) and torch.equal(xp, before)
    wd = folded.double().permute(0, 2, 1)
    conv = lambda a, w, b: F.conv1d(a.transpose(1, 2), w, b, padding=k // 2, groups=groups)[:, :, :T].transpose(1, 2)
    ref = x.double() + R.gelu(conv(x.double(), wd, bias.double()))
    A = 1.13 * conv(x.double().abs(), wd.abs(), bias.double().abs()) + x.double().abs()
    assert_close_elementwise(ov, ref, A, k * cc // groups, f'posconv T\'={T} C={cc} k={k} groups={groups}', slack=16)


# -------------------------------------------------------------------------------------------------------------- attention
def attention_case(dev, d, T, kind, heads=2, B=2):
    w_ = W()
    cc = heads * d
    seed = 1000 * d + T
    q, k, v = rnd(seed, B, T, heads, d, scale=d ** -0.25), rnd(seed + 1, B, T, heads, d, scale=d ** -0.25), rnd(seed + 2, B, T, heads, d)
    gate, table = 1.75 + rnd(seed + 3, B, heads, T, scale=0.2), rnd(seed + 4, heads, 2 * T - 1)
    if kind == 'dominant':                                                   # key t + 3 leads by about 80, key t - 5 by about 40: the running
        q, k, table = q * 0.3, k * 0.3, table * 0.3                          # maximum rises twice, for t near 64 in different key tiles
        table[:, T - 1 + 3] += 80.0 / 1.75
        table[:, T - 1 - 5] += 40.0 / 1.75
    elif kind == 'equal':
        q = torch.zeros_like(q)
        table = torch.zeros_like(table)
    elif kind == 'big_bias':
        table = table * 30.0
        gate[:, 0] = -gate[:, 0]
    qkv = torch.cat([q.reshape(B, T, cc), k.reshape(B, T, cc), v.reshape(B, T, cc)], -1)
    qw, qv = guarded(B, T, 3 * cc, dev, qkv)
    ow, ov = guarded(B, T, cc, dev)
    poison_lds(dev)
    w_.wavlm_attention(qv, heads, gate.to(dev), table.contiguous().to(dev), out=ov)
    assert spare_intact(ow, ov)
    qd, kd, vd, gd, td = q.double(), k.double(), v.double(), gate.double(), table.double()
    rel = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1
    bias = gd[..., None] * td[:, rel][None]                                  # [B, H, t, s]
    dot = torch.einsum('bthd,bshd->bhts', qd, kd)
    scores = dot + bias
    p = torch.softmax(scores, -1)
    ref = torch.einsum('bhts,bshd->bthd', p, vd).reshape(B, T, cc)
    A = torch.einsum('bhts,bshd->bthd', p, vd.abs()).reshape(B, T, cc)
    absdot = torch.einsum('bthd,bshd->bhts', qd.abs(), kd.abs())
    E = ((d + 4) * U * (absdot + bias.abs()) + U * (scores.abs() + scores.abs().amax(-1, keepdim=True))).amax(-1)      # [B, H, t]
    extra = (2.0 * E).permute(0, 2, 1)[..., None].expand(B, T, heads, d).reshape(B, T, cc) / U
    got = ov.detach().double().cpu()
    bound = (T + 8 + extra) * U * A + 2.0 ** -22 * ref.abs()
    ratio = float(((got - ref).abs() / bound).max())
    print(f'attention {kind} d={d} T\'={T}: error / bar {ratio:.3f}; score spread {float((scores.amax(-1) - scores.amin(-1)).max()):.1f}')
    assert ratio <= 1.0, (kind, d, T, ratio)
    return scores, ref


@pytest.mark.parametrize('d', [16, 32, 64])
@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 257])
def test_attention_against_float64(dev, d, T):
    attention_case(dev, d, T, 'plain')


@pytest.mark.parametrize('kind', ['dominant', 'equal', 'big_bias'])
def test_attention_extreme_scores(dev, kind):
    for d, T in ((16, 65), (64, 257)):
        scores, ref = attention_case(dev, d, T, kind)
        top2 = scores.topk(min(2, T), -1).values
        if kind == 'dominant':
            lead = scores.amax(-1) - scores.median(-1).values
            assert float(lead.min()) > 25.0 and float(lead.median()) > 60.0     # the last three queries have the 40-leader only
        if kind == 'equal':
            assert float((top2[..., 0] - top2[..., -1]).abs().max()) == 0.0
        if kind == 'big_bias':
            assert float(scores.max()) > 100.0 and float(scores.min()) < -100.0


def test_attention_long_row_passes_the_exact_range_and_the_clamp(dev):
    """T' = 1100: |s - t| passes 80 (the exact buckets) and 800 (the clamp at bucket 159 / 319); the table is the model's own."""
    w_ = W()
    T, heads, d = 1100, 1, 16
    m = w_.WavLM(w_.WavLMConfig(R.full_cfg(R.SMALL)))
    sd = R.state_dict(5, R.SMALL)
    m.load_state_dict(sd)
    m.to(dev)
    table = m.bias_table(T, dev)[:1].contiguous()
    want = R.bias_table(R.cast(sd, torch.float64), R.SMALL, T)[:1]
    assert torch.equal(table.cpu().double(), want)
    idx = R.buckets(torch.arange(-(T - 1), T), 320, 800)
    assert int(idx.min()) == 0 and int(idx.max()) == 319 and int((idx == 159).sum()) > 200 and int((idx == 319).sum()) > 200
    q, k, v = rnd(1, 1, T, heads, d, scale=0.5), rnd(2, 1, T, heads, d, scale=0.5), rnd(3, 1, T, heads, d)
    gate = 1.75 + rnd(4, 1, heads, T, scale=0.2)
    qkv = torch.cat([q.reshape(1, T, d), k.reshape(1, T, d), v.reshape(1, T, d)], -1).to(dev)
    out = w_.wavlm_attention(qkv, heads, gate.to(dev), table)
    ref = R.attention(q.double(), k.double(), v.double(), gate.double(), want)
    scale = float(ref.abs().max())
    err = float((out.double().cpu() - ref).abs().max())
    print(f'attention T\'=1100: max error {err:.3e} at scale {scale:.3f}')
    assert err <= (T + 64) * U * scale                                       # every |v| <= a few: the coarse form of the element-wise bar
    with pytest.raises(ValueError, match='4096'):
        w_.wavlm_attention(torch.zeros(1, 4097, 48, device=dev), 1, torch.zeros(1, 1, 4097, device=dev), torch.zeros(1, 8193, device=dev))


# -------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, 'wavlm_small.npz'))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    x = torch.from_numpy(z['input'])
    sd32 = R.cast(sd, torch.float32)
    want = {name: torch.from_numpy(z[name]) for name in ('out', 'layer1', 'layer2', 'conv')}
    kws = dict(out={}, layer1=dict(output_layer=1), layer2=dict(output_layer=2), conv=dict(ret_conv=True))
    bars = {name: 4.0 * float((R.extract(sd32, R.SMALL, x, **kws[name]).double() - want[name]).abs().max()) for name in want}
    return json.loads(str(z['cfg'])), sd, x, want, kws, bars


def small_model(dev):
    cfg, sd, x, want, kws, bars = fixture()
    m = W().WavLM(W().WavLMConfig(cfg))
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def test_extract_features_against_the_reference_fixture(dev):
    cfg, sd, x, want, kws, bars = fixture()
    m = small_model(dev)
    xd = x.to(dev)
    for name in ('out', 'layer1', 'layer2', 'conv'):
        got, none = m.extract_features(xd, **kws[name])
        assert none is None and got.shape == (2, 25, 64) and got.dtype == torch.float32
        err = float((got.double().cpu() - want[name]).abs().max())
        print(f'extract_features {name}: max error {err:.3e}, bar {bars[name]:.3e} (4 x the fp32 CPU chain), error / bar {err / bars[name]:.3f}, '
              f'scale {float(want[name].abs().max()):.2f}')
        assert err <= bars[name], (name, err, bars[name])
    assert torch.equal(m(xd), m.extract_features(xd)[0])


def test_extract_features_row_alone_repeat_and_graph(dev):
    cfg, sd, x, want, kws, bars = fixture()
    m = small_model(dev)
    xd = torch.cat([x, R.wave(1, 8160, seed=9)]).to(dev)
    full = m.extract_features(xd)[0]
    for b in range(3):
        assert torch.equal(m.extract_features(xd[b:b + 1])[0][0], full[b]), b          # a row alone: the same bits as in the batch
    assert torch.equal(m.extract_features(xd)[0], full)                          # two calls: the same bits
    assert torch.equal(m.extract_features(xd[:, None].expand(3, 2, 8160)[:, 1])[0], full)  # a strided view of the same rows
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    static = xd.clone()
    with torch.cuda.stream(stream):
        m.extract_features(static)
    torch.cuda.current_stream(dev).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = m.extract_features(static)[0]
    static.copy_(xd.flip(0))
    graph.replay()
    assert torch.equal(captured, full.flip(0))
    static.copy_(xd)
    graph.replay()
    assert torch.equal(captured, full)
    assert m.extract_features(torch.zeros(0, 8160, device=dev))[0].shape == (0, 25, 64)
    with pytest.raises(ValueError, match='no frame'):
        m.extract_features(torch.zeros(1, 399, device=dev))


def network_case(dev, cfg, seed, x):
    sd = R.state_dict(seed, cfg)
    m = W().WavLM(W().WavLMConfig(R.full_cfg(cfg)))
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    ref = R.extract(R.cast(sd, torch.float64), cfg, x.double())
    bar = 4.0 * float((R.extract(sd, cfg, x).double() - ref).abs().max())
    return m, ref, bar


def test_extract_features_two_heads_of_width_64(dev):
    x = R.wave(2, 4000, seed=3)
    m, ref, bar = network_case(dev, R.WIDE, 11, x)
    got = m.extract_features(x.to(dev))[0]
    err = float((got.double().cpu() - ref).abs().max())
    print(f'extract_features C=128 d=64: max error {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}, scale {float(ref.abs().max()):.2f}')
    assert got.shape == (2, 12, 128) and err <= bar


def test_ssl_encoder_features_runs_the_extractor(dev):
    """SSLEncoder hard-codes 1024 features: one layer of width 1024 with 16 heads behind 16-channel convolutions."""
    x = R.wave(2, 8000, seed=4)
    m, _, _ = network_case(dev, R.SSL, 12, x[:, :400])
    sd = R.state_dict(12, R.SSL)
    enc = pkg().ssl_encoder.SSLEncoder(num_layers=2, cmodel=m)
    assert enc.cmodel is m and not m.training
    padded = F.pad(x, (160, 0))
    ref = R.extract(R.cast(sd, torch.float64), R.SSL, padded.double()).transpose(1, 2)
    bar = 4.0 * float((R.extract(sd, R.SSL, padded).double().transpose(1, 2) - ref).abs().max())
    got = enc.features(x[:, None].to(dev))
    err = float((got.double().cpu() - ref).abs().max())
    print(f'SSLEncoder.features: max error {err:.3e}, bar {bar:.3e}, error / bar {err / bar:.3f}, scale {float(ref.abs().max()):.2f}')
    assert got.shape == (2, 1024, 25) and got.is_contiguous() and err <= bar


def test_convert_audio_runs_waveform_to_waveform(dev):
    """Generator(encoder_model='wavlm', cmodel=WavLM(...)) needs no change: infer.convert_audio runs with nothing injected from outside,
    and the content features it converts from are the extractor's."""
    from common import build_ssl_models
    x = R.wave(1, 8960, seed=6, db=-12.0)
    m, _, _ = network_case(dev, R.SSL, 12, x[:, :400])
    G, _, _ = build_ssl_models(dev, extractor=m)
    assert G.encoder.cmodel is m
    c_tgt = torch.zeros(1, 16, device=dev)
    c_tgt[0, 3] = 1.0
    y = pkg().infer.convert_audio(G, x[:, None].to(dev), c_tgt)
    assert y.shape == (1, 1, 8960) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    feats = G.encoder.features(x[:, None].to(dev))
    assert torch.equal(feats, m.extract_features(F.pad(x, (160, 0)).to(dev))[0].transpose(1, 2))
