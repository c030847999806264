"""GPU: the ECAPA-TDNN speaker-recognition metric on the device (td-vc-gan_amd/ecapa.py, csrc/eval_ecapa.hip) against the float64
restatement tests/ecapa_ref.py, which tests/test_ecapa_cpu.py pins. speechbrain and torchaudio are not available: nothing here is a
parity test against them.

1. fbank against float64 element by element: |got - ref| <= 4 * 2^-24 * max|row of ref| (one rounding x 4, the project's bar for
   float64-inside kernels); rows of 640, 799, 800, 25439 and 71680 samples, a loud burst followed by digital silence (the 1e-10 clamp
   and the M - 80 floor both active, asserted) and an all-zero row (exactly 0) in one padded buffer that is a strided view with NaN
   spares; the frame counts are returned.
2. tdvc_tdnn_fwd alone through the C ABI against float64 F.conv1d on the reflect-padded row cut to its own length: (80->128, k5, d1),
   (16->16, k3, d 2|3|4) with the added second input and channel-slice input and output inside 128-channel buffers whose other
   channels are NaN and stay NaN, (128->128, k1), (48->32, k1: the k1 kernel reduces over chunks of 32 channels, the second one
   half empty), (384->384, k1) with each epilogue and the per-row bias. Rows of 5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
   129 frames (the kernel's time tile is 64) mixed in one batch, NaN past each row's end, LDS poisoned first. The bar of each case
   is 4 x the max-abs error of stock torch's fp32 CPU evaluation of the same case against float64.
3. tdvc_se_block, tdvc_asp_pool, tdvc_ecapa_head each against float64, the bar built the same way per row (max-abs over the row's
   output vector); 5, 33 and 130 frames; a constant channel, so that the 1e-12 clamp is active (asserted).
4. embed end to end: the small network (C = 128) on rows of 640, 8000, 31520 and 71680 samples in one buffer, and the shipped widths
   (1024 / 3072) on two rows of 8000 samples; bar 4 x the fp32 CPU chain's error on the float64 features; each row alone is
   bit-identical to the same row in the batch; two runs are bit-identical; graph replay equals eager.
5. speaker_classify on the device: pred equals the float64 prediction on every row, every row's float64 top-two gap exceeds 1e-3
   (asserted), target_prob within 64 * 2^-24.
6. Refusals, each before any launch.
Every test prints error / bar (run with -s). Measured on an MI355X: fbank 0.12-0.18 (the all-zero row 0); tdnn_fwd 0.13 (80->128 k5),
0.25-0.32 (16->16 k3 with the second input, sliced), 0.11 (128->128), 0.26 (48->32), 0.05-0.07 (384->384 with each epilogue and the
row bias);
se_block 0.18-0.24; asp_pool 0.08-0.11; ecapa_head 0.03-0.04; embed 0.05-0.12 (C = 128) and 0.03 (shipped widths); target
probabilities within 4.0e-9 of float64 (bar 3.8e-6), the smallest float64 top-two gap 1.29e-3.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ecapa_ref as R
from common import pkg
from edge_support import EINVAL, EUNSUPPORTED, EWORKSPACE, poison_lds

pytestmark = pytest.mark.gpu
NAN = float('nan')
FRAMES = (5, 6, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def E():
    return pkg().ecapa


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------------------------------ 1. fbank
@functools.lru_cache(maxsize=None)
def fbank_case():
    ns = (640, 799, 800, 25439, 71680, 8000, 8000)
    T = 71999
    x = np.full((len(ns), T), np.nan, dtype=np.float32)
    for b, n in enumerate(ns[:5]):
        x[b, :n] = R.tones(n, seed=b)
    x[5, :8000] = R.burst(8000, seed=5)
    x[6, :8000] = 0.0
    refs = [R.fbank(x[b, :n]) for b, n in enumerate(ns)]
    x.setflags(write=False)
    return ns, x, refs


def test_fbank_against_float64(dev):
    ns, x, refs = fbank_case()
    B, T = x.shape
    whole = torch.full((2 * B, T + 5), NAN, device=dev)
    whole[::2, :T] = torch.from_numpy(np.array(x)).to(dev)
    view = whole[::2, :T]
    assert view.stride() == (2 * (T + 5), 1)
    lengths = torch.tensor(ns, dtype=torch.int32, device=dev)
    poison_lds(dev)
    feats, frames = E().fbank(view[:, None], lengths=lengths, return_frames=True)
    Fm = 1 + T // 160
    assert feats.shape == (B, 80, Fm) and feats.dtype == torch.float32 and frames.dtype == torch.int32
    assert frames.tolist() == [1 + n // 160 for n in ns]
    assert torch.isfinite(feats).all()
    got = feats.double().cpu().numpy()
    db, mel = R.log_mel(x[5, :8000])
    assert (mel < 1e-10).any() and (db < db.max() - 80.0).any()             # the burst row: clamp and floor both active
    for b, n in enumerate(ns):
        nf = 1 + n // 160
        assert (got[b, :, nf:] == 0).all()                                  # frames past the row's own count
        bar = 4 * 2.0 ** -24 * float(np.abs(refs[b]).max())
        err = float(np.abs(got[b, :, :nf] - refs[b]).max())
        print(f'fbank n={n} row {b}: max|got - ref| {err:.3e}, error / bar {err / bar if bar else 0.0:.3f}')
        assert err <= bar, (b, n, err, bar)
    assert (got[6] == 0).all()                                              # the all-zero row: exactly 0
    alone = E().fbank(torch.from_numpy(np.array(x[3, :ns[3]])).to(dev))     # no lengths, one row [T]: the same bits
    assert torch.equal(alone[0], feats[3, :, :alone.shape[2]])
    again = E().fbank(view, lengths=lengths)
    assert torch.equal(again, feats)


# ------------------------------------------------------------------------------------------------------------------- 2. TDNN
def tdnn_call(dev, Cin, Cout, K, d, epi, x, w, bias, y, frames, x2=None, row_bias=None, scale=None, shift=None):
    L = pkg()._lib
    a = L.TdnnArgs()
    a.B, a.Cin, a.Cout, a.F, a.K, a.dilation, a.epilogue = x.shape[0], Cin, Cout, x.shape[2], K, d, epi
    a.x, a.x_bs, a.x_cs = x.data_ptr(), x.stride(0), x.stride(1)
    if x2 is not None:
        a.x2, a.x2_bs, a.x2_cs = x2.data_ptr(), x2.stride(0), x2.stride(1)
    a.w, a.w_rs = w.data_ptr(), 0
    a.bias = bias.data_ptr()
    for name, t in (('row_bias', row_bias), ('scale', scale), ('shift', shift)):
        if t is not None:
            setattr(a, name, t.data_ptr())
    a.y, a.y_bs, a.y_cs = y.data_ptr(), y.stride(0), y.stride(1)
    a.frames = frames.data_ptr()
    return L.lib().tdvc_tdnn_fwd(C.byref(a), stream(dev))


def tdnn_ref(dtype, x, x2, w, bias, rb, scale, shift, epi, d, frames):
    """-> list of [Cout, n] per row: the row cut to its own length, reflect-padded, F.conv1d."""
    out = []
    pad = (w.shape[2] - 1) * d // 2
    for b, n in enumerate(frames):
        xi = x[b, :, :n].to(dtype)
        if x2 is not None:
            xi = xi + x2[b, :, :n].to(dtype)
        xi = xi[None]
        if pad:
            xi = F.pad(xi, (pad, pad), mode='reflect')
        y = F.conv1d(xi, w.to(dtype), bias.to(dtype), dilation=d)[0]
        if rb is not None:
            y = y + rb[b].to(dtype)[:, None]
        if epi:
            y = torch.relu(y) * scale.to(dtype)[:, None] + shift.to(dtype)[:, None]
        if epi == 2:
            y = torch.tanh(y)
        out.append(y)
    return out


def tdnn_case(dev, Cin, Cout, K, d, epi, second=False, sliced=False, rowbias=False, seed=0):
    g = torch.Generator().manual_seed(1000 * Cin + 10 * K + d + seed)
    B, Fm = len(FRAMES), max(FRAMES) + 2
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, x2 = rnd(B, Cin, Fm), (rnd(B, Cin, Fm) if second else None)
    w = (2 * torch.rand(Cout, Cin, K, generator=g) - 1) / float(Cin * K) ** 0.5
    bias, rb = 0.1 * rnd(Cout), (0.5 * rnd(B, Cout) if rowbias else None)
    scale, shift = (0.5 + torch.rand(Cout, generator=g), rnd(Cout) * 0.3) if epi else (None, None)
    y64 = tdnn_ref(torch.float64, x, x2, w, bias, rb, scale, shift, epi, d, FRAMES)
    y32 = tdnn_ref(torch.float32, x, x2, w, bias, rb, scale, shift, epi, d, FRAMES)
    bar = 4 * max(float((a.double() - b).abs().max()) for a, b in zip(y32, y64))
    for b, n in enumerate(FRAMES):                                          # NaN past each row's end
        x[b, :, n:] = NAN
        if second:
            x2[b, :, n:] = NAN
    wide = 128 if sliced else None
    if sliced:                                                              # x in channels 32..48 of one buffer, x2 in 16..32 and y in 48..64 of another
        bx, by = torch.full((B, wide, Fm), NAN), torch.full((B, wide, Fm), NAN)
        bx[:, 32:48], by[:, 16:32] = x, x2
        bx, by = bx.to(dev), by.to(dev)
        xd, x2d, yd = bx[:, 32:48], by[:, 16:32], by[:, 48:64]
        before = by.clone()
    else:
        xd, x2d = x.to(dev), (x2.to(dev) if second else None)
        by = torch.full((B, Cout, Fm), NAN, device=dev)
        yd, before = by, None
    dv = lambda t: None if t is None else t.to(dev).contiguous()
    wd, bd, rbd, sd_, shd = dv(w), dv(bias), dv(rb), dv(scale), dv(shift)
    frames = torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    poison_lds(dev)
    rc = tdnn_call(dev, Cin, Cout, K, d, epi, xd, wd, bd, yd, frames, x2=x2d, row_bias=rbd, scale=sd_, shift=shd)
    assert rc == 0, pkg()._lib.lib().tdvc_last_error()
    torch.cuda.synchronize()
    got = yd.double().cpu()
    worst = 0.0
    for b, n in enumerate(FRAMES):
        assert torch.isnan(got[b, :, n:]).all(), f'row {b}: frames past {n} were written'
        assert torch.isfinite(got[b, :, :n]).all(), f'row {b}'
        worst = max(worst, float((got[b, :, :n] - y64[b]).abs().max()))
    if sliced:
        after = by.cpu()
        keep = torch.ones(wide, dtype=torch.bool)
        keep[48:64] = False
        assert torch.equal(torch.isnan(after[:, keep]), torch.isnan(before.cpu()[:, keep]))
        assert torch.equal(after[:, 16:32].nan_to_num(7.0), before.cpu()[:, 16:32].nan_to_num(7.0))
        assert torch.isnan(bx.cpu()[:, :32]).all() and torch.isnan(bx.cpu()[:, 48:]).all()
    print(f'tdnn {Cin}->{Cout} k{K} d{d} epilogue {epi}{" +x2 sliced" if sliced else ""}{" +row bias" if rowbias else ""}: '
          f'max|y - y64| {worst:.3e}, bar {bar:.3e}, error / bar {worst / bar:.3f}')
    assert worst <= bar


@pytest.mark.parametrize('Cin,Cout,K,d,epi,second,sliced,rowbias', [
    (80, 128, 5, 1, 1, False, False, False),
    (16, 16, 3, 2, 1, True, True, False), (16, 16, 3, 3, 1, True, True, False), (16, 16, 3, 4, 1, True, True, False),
    (128, 128, 1, 1, 0, False, False, False), (48, 32, 1, 1, 1, False, False, False),      # 48: a partly filled 32-channel chunk
    (384, 384, 1, 1, 0, False, False, True), (384, 384, 1, 1, 1, False, False, True), (384, 384, 1, 1, 2, False, False, True)])
def test_tdnn_against_float64(dev, Cin, Cout, K, d, epi, second, sliced, rowbias):
    tdnn_case(dev, Cin, Cout, K, d, epi, second, sliced, rowbias)


# --------------------------------------------------------------------------------------------------- 3. SE, pooling and head
SMALL_FRAMES = (5, 33, 130)


def row_check(what, got, r64, r32):
    worst = 0.0
    for b in range(len(r64)):
        err, bar = float((got[b].double().cpu() - r64[b]).abs().max()), 4 * float((r32[b].double() - r64[b]).abs().max())
        print(f'{what} row {b}: max|got - ref| {err:.3e}, fp32 CPU {bar / 4:.3e}, error / bar {err / bar:.3f}')
        assert torch.isfinite(got[b]).all() and err <= bar, (what, b, err, bar)
        worst = max(worst, err / bar)
    return worst


def padded(rows, Fm, dev):
    """rows: list of [C, n] -> [B, C, Fm] on the device with NaN past each row's end."""
    buf = torch.full((len(rows), rows[0].shape[0], Fm), NAN)
    for b, r in enumerate(rows):
        buf[b, :, :r.shape[1]] = r
    return buf.to(dev)


def test_se_block_against_float64(dev):
    sd = R.state_dict(11)
    key = 'blocks.2.se_block'
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(128, n, generator=g) for n in SMALL_FRAMES]
    rs = [torch.randn(128, n, generator=g) for n in SMALL_FRAMES]
    r64 = [R.se(R.cast(sd, torch.float64), key, x[None].double(), r[None].double())[0] for x, r in zip(xs, rs)]
    r32 = [R.se(sd, key, x[None], r[None])[0] for x, r in zip(xs, rs)]
    frames = torch.tensor(SMALL_FRAMES, dtype=torch.int32, device=dev)
    wide = torch.full((3, 256, 131), NAN, device=dev)                       # the output is a channel slice
    out = wide[:, 64:192]
    p = {k: sd[f'{key}.{k}'].to(dev) for k in ('conv1.conv.weight', 'conv1.conv.bias', 'conv2.conv.weight', 'conv2.conv.bias')}
    E().se_block(padded(xs, 131, dev), padded(rs, 131, dev), p['conv1.conv.weight'], p['conv1.conv.bias'], p['conv2.conv.weight'],
                 p['conv2.conv.bias'], frames=frames, out=out)
    got = [out[b, :, :n] for b, n in enumerate(SMALL_FRAMES)]
    row_check('se_block', got, r64, r32)
    assert torch.isnan(wide[:, :64]).all() and torch.isnan(wide[:, 192:]).all()
    assert all(torch.isnan(out[b, :, n:]).all() for b, n in enumerate(SMALL_FRAMES))


def test_asp_pool_against_float64(dev):
    sd = R.state_dict(12)
    sd64 = R.cast(sd, torch.float64)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(384, n, generator=g) for n in SMALL_FRAMES]
    for x in xs:
        x[7] = 0.3125                                                       # a channel that is dead after ReLU: constant after the BatchNorm
    r64 = [R.asp(sd64, x[None].double())[0] for x in xs]
    r32 = [R.asp(sd, x[None])[0] for x in xs]
    assert all(float(r[384 + 7]) == 1e-12 ** 0.5 for r in r64)              # the clamp is active
    E_ = E()
    scale, shift = E_.fold_bn(bn_module(sd, 'asp.tdnn.norm', 32))
    frames = torch.tensor(SMALL_FRAMES, dtype=torch.int32, device=dev)
    poison_lds(dev)
    got = E_.asp_pool(padded(xs, 131, dev), sd['asp.tdnn.conv.conv.weight'].to(dev), sd['asp.tdnn.conv.conv.bias'].to(dev), scale.to(dev),
                      shift.to(dev), sd['asp.conv.conv.weight'].to(dev), sd['asp.conv.conv.bias'].to(dev), frames=frames)
    assert got.shape == (3, 768)
    row_check('asp_pool', got, r64, r32)


def bn_module(sd, key, c):
    m = torch.nn.BatchNorm1d(c, eps=1e-5)
    m.load_state_dict({k: sd[f'{key}.norm.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')})
    return m.eval()


def test_ecapa_head_against_float64(dev):
    sd = R.state_dict(13)
    g = torch.Generator().manual_seed(5)
    pooled = torch.randn(3, 768, generator=g)
    r64 = R.head(R.cast(sd, torch.float64), pooled.double())
    r32 = R.head(sd, pooled)
    scale, shift = E().fold_bn(bn_module(sd, 'asp_bn', 768))
    got = E().ecapa_head(pooled.to(dev), scale.to(dev), shift.to(dev), sd['fc.conv.weight'].to(dev), sd['fc.conv.bias'].to(dev))
    assert got.shape == (3, 48)
    row_check('ecapa_head', got, r64, r32)


# ------------------------------------------------------------------------------------------------------------------ 4. embed
@functools.lru_cache(maxsize=None)
def embed_case(which):
    cfg, ns = (R.SMALL, (640, 8000, 31520, 71680)) if which == 'small' else (R.FULL, (8000, 8000))
    T = max(ns) + 319
    x = np.full((len(ns), T), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = R.tones(n, seed=40 + b)
    sd = R.state_dict(21, cfg)
    sd64 = R.cast(sd, torch.float64)
    e64, e32 = [], []
    for b, n in enumerate(ns):
        f64 = torch.from_numpy(R.fbank(x[b, :n]))
        e64.append(R.embed_row(sd64, f64))
        e32.append(R.embed_row(sd, f64.float()))
    x.setflags(write=False)
    return cfg, ns, x, sd, e64, e32


@pytest.mark.parametrize('which', ['small', 'full'])
def test_embed_end_to_end(dev, which):
    cfg, ns, x, sd, e64, e32 = embed_case(which)
    enc = E().EcapaTdnn(**cfg)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    xd = torch.from_numpy(np.array(x)).to(dev)[:, None]
    lengths = torch.tensor(ns, dtype=torch.int32, device=dev)
    poison_lds(dev)
    emb = enc.embed(xd, lengths=lengths)
    assert emb.shape == (len(ns), cfg['lin_neurons']) and emb.dtype == torch.float32
    row_check(f'embed {which}', emb, e64, e32)
    assert torch.equal(enc.embed(xd, lengths=lengths), emb)                 # bit-identical from call to call
    for b, n in enumerate(ns):                                              # a row alone: the same bits as inside the batch
        assert torch.equal(enc.embed(xd[b, :, :n])[0], emb[b]), f'row {b} alone differs from the row in the batch'
    if which == 'small':
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc.embed(xd, lengths=lengths)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = enc.embed(xd, lengths=lengths)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, emb)


# ------------------------------------------------------------------------------------------------------------- 5. classifier
def test_speaker_classify_on_the_device(dev):
    cfg, ns, x, sd, e64, _ = embed_case('small')
    e64 = torch.stack(e64).numpy()
    r = np.random.RandomState(9)
    # the rows' embeddings share most of their direction (cosines up to 0.995), and cosine logits leave a softmax over 16 speakers
    # flat: the rows' own classifier rows are the embeddings without their common direction, which is what tells them apart, and
    # the random others are orthogonal to every test embedding (logit 0)
    u = e64.mean(axis=0) / np.linalg.norm(e64.mean(axis=0))
    q, _ = np.linalg.qr(e64.T)
    weight = r.randn(16, 48)
    weight = weight - (weight @ q) @ q.T
    target = np.array([3, 0, 11, 7])
    weight[target] = (e64 - np.outer(e64 @ u, u)) * r.uniform(0.5, 2.0, (4, 1))
    prob, pred, tp = R.classify_numpy(e64, weight, target)
    top2 = np.sort(prob, axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 1e-3).all() and np.array_equal(pred, target)       # every row, none excluded
    enc = E().EcapaTdnn(**cfg)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    emb = enc.embed(torch.from_numpy(np.array(x)).to(dev), lengths=torch.tensor(ns, dtype=torch.int32, device=dev))
    gp, gpred, gtp = E().speaker_classify(emb, torch.from_numpy(weight).float().to(dev), torch.from_numpy(target).to(dev))
    assert gp.is_cuda and gp.shape == (4, 16)
    assert np.array_equal(gpred.cpu().numpy(), pred)
    err = float(np.abs(gtp.double().cpu().numpy() - tp).max())
    print(f'speaker_classify: target probabilities {tp}, max error {err:.3e} (bar {64 * 2.0 ** -24:.3e})')
    assert err <= 64 * 2.0 ** -24


# -------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    ec, L = E(), pkg()._lib
    lib = L.lib()
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError, match='fbank.*640'):
        ec.fbank(z(2, 639))
    with pytest.raises(ValueError, match='fbank.*n_mels'):
        ec.fbank(z(1, 800), n_mels=136)
    with pytest.raises(ValueError, match='tdnn_fwd.*multiples of 16'):
        ec.tdnn_fwd(z(1, 24, 8), z(16, 24, 3), z(16))
    with pytest.raises(ValueError, match='tdnn_fwd.*multiples of 16'):
        ec.tdnn_fwd(z(1, 16, 8), z(24, 16, 3), z(24))
    with pytest.raises(ValueError, match='tdnn_fwd.*1, 3 or 5'):
        ec.tdnn_fwd(z(1, 16, 8), z(16, 16, 7), z(16))
    with pytest.raises(ValueError, match='tdnn_fwd.*dilation'):
        ec.tdnn_fwd(z(1, 16, 8), z(16, 16, 3), z(16), dilation=5)
    with pytest.raises(ValueError, match='tdnn_fwd.*5 frames'):
        ec.tdnn_fwd(z(1, 16, 4), z(16, 16, 3), z(16))
    with pytest.raises(ValueError, match='EcapaTdnn.*128'):
        ec.EcapaTdnn(**{**R.SMALL, 'channels': [144, 144, 144, 144, 432]})
    with pytest.raises(L.TdvcError, match='no CPU fallback'):
        ec.fbank(torch.zeros(1, 800))
    # workspaces, through the C ABI: null and one byte short; the outputs keep their sentinel (nothing was launched)
    x, tab = z(1, 800), ec._tables(dev, 80)
    feats, frames = torch.full((1, 80, 6), -7.0, device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    need = lib.tdvc_fbank_workspace(1, 800, 80)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for wptr, wbytes in ((None, need), (ws.data_ptr(), need - 1)):
        rc = lib.tdvc_fbank(x.data_ptr(), 800, None, 800, 1, 80, tab.data_ptr(), feats.data_ptr(), 480, 6, 6, frames.data_ptr(), wptr, wbytes, stream(dev))
        assert rc == EWORKSPACE and b'fbank' in lib.tdvc_last_error()
    assert lib.tdvc_fbank(x.data_ptr(), 800, None, 800, 1, 80, tab.data_ptr(), feats.data_ptr(), 480, 6, 7, frames.data_ptr(), ws.data_ptr(), need,
                          stream(dev)) == EINVAL
    act, pooled = z(1, 32, 8), torch.full((1, 64), -7.0, device=dev)
    v32, v16 = z(32), z(16)
    need = lib.tdvc_asp_pool_workspace(1, 32, 16, 8)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    w_t, w_c = z(16, 96), z(32, 16)
    for wptr, wbytes in ((None, need), (ws.data_ptr(), need - 1)):
        rc = lib.tdvc_asp_pool(act.data_ptr(), 256, 8, 1, 32, 8, None, 16, w_t.data_ptr(), v16.data_ptr(), v16.data_ptr(), v16.data_ptr(), w_c.data_ptr(),
                               v32.data_ptr(), pooled.data_ptr(), wptr, wbytes, stream(dev))
        assert rc == EWORKSPACE and b'asp_pool' in lib.tdvc_last_error()
    assert lib.tdvc_asp_pool(act.data_ptr(), 256, 8, 1, 24, 8, None, 16, w_t.data_ptr(), v16.data_ptr(), v16.data_ptr(), v16.data_ptr(), w_c.data_ptr(),
                             v32.data_ptr(), pooled.data_ptr(), ws.data_ptr(), need, stream(dev)) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (feats == -7.0).all() and (frames == -7).all() and (pooled == -7.0).all()
