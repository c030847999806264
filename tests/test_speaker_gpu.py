"""GPU: the speaker-similarity evaluation on the device (td-vc-gan_amd/speaker.py, csrc/eval_speaker.hip) against the float64
restatement tests/speaker_ref.py, which tests/test_speaker_cpu.py pins. Resemblyzer and librosa are not available: nothing here is
a parity test against them.

1. The recurrence alone (lstm_fwd) against torch.nn.LSTM in float64 on the CPU, max-abs over h. The bar of each case is 4 x the
   max-abs error of stock torch's fp32 CPU evaluation of the same module on the same inputs against float64: derived from the
   reference, computed per case, with the project's factor 4 for another summation order. Seeded weights in nn.LSTM's default
   initialisation, and the same times 4 so that the gates saturate. Windows 1, 5, 32, 33, 65 (a tile edge, several tiles), steps
   1, 2, 160, 1 and 3 layers, input size 40 and 256; overlapping windows of one frame array, windows from different rows, a
   strided frame array with NaN in every frame no window covers, a row with zero windows, poisoned LDS.
2. voice_mel against the float64 mel element by element: |mel - mel64| <= 4 * 2^-24 * mel64 (one rounding, x 4), n = 1000, 25440,
   31519, 31520, 71680 in one padded buffer with NaN past n, both pad modes, normalize on a quiet and a loud row, an expanded row
   and an every-other-row view.
3. embed_utterance end to end: rows of 20000, 31520 and 71680 samples in one padded buffer against the float64 chain, the bar built
   the same way from the fp32 CPU chain on the float64 mel; counts 1, 2, 5; two runs bit-identical; graph replay equals eager.
4. Refusals surface as ValueError with the operator's name.
5. speaker_similarity on device tensors equals the CPU result.
Measured on an MI355X (error over bar, printed with -s): recurrence 0.10-0.29 over all cases (0.25 at one step, 0.13-0.16 with
saturated gates), mel 0.237-0.249 (0.25 is the one rounding to fp32), embed_utterance 0.09-0.31 on the utterance and 0.06-0.29 on
the window embeddings. An earlier build with 32-row tiles and one summation chain over all of K measured 1.29 at one step.
"""
import functools

import numpy as np
import pytest
import torch

import speaker_ref as R
from common import pkg

pytestmark = pytest.mark.gpu
BAR = 4 * 2.0 ** -24
NAN = float('nan')


def S():
    return pkg().speaker


def layer_weights(sd, dev):
    n = sum(k.startswith('lstm.weight_hh') for k in sd)
    return [tuple(sd[f'lstm.{name}_l{k}'].to(dev) for name in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')) for k in range(n)]


@functools.lru_cache(maxsize=None)
def rec_case(nwin, T, layers, I, scale):
    """(sd, windows fp32 [nwin, T, I], h64, bar per window count): windows are independent, so the first P of them are a case of P."""
    sd = R.state_dict(seed=100 + layers + I, scale=scale, input_size=I, layers=layers)
    g = torch.Generator().manual_seed(T * 1000 + I)
    win = torch.randn(nwin, T, I, generator=g)
    h64 = R.hidden(R.net(sd, torch.float64), win)
    h32 = R.hidden(R.net(sd, torch.float32), win).double()
    return sd, win, h64, (h32 - h64).abs()


def check_h(what, got, h64, err32):
    bar = 4 * float(err32.max())
    err = float((got.double().cpu() - h64).abs().max())
    print(f'{what}: max|h - h64| {err:.3e}, fp32 CPU {float(err32.max()):.3e}, error / bar {err / bar:.3f}')
    assert torch.isfinite(got).all()
    assert err <= bar, (what, err, bar)


def own_rows(P, dev):
    s = torch.zeros(P, 2, dtype=torch.int32, device=dev)
    s[:, 0] = torch.arange(P, dtype=torch.int32)
    return s


@pytest.mark.parametrize('P,nwin,T,layers,I,scale', [
    (1, 65, 160, 3, 40, 1.0), (5, 65, 160, 3, 40, 1.0), (32, 65, 160, 3, 40, 1.0), (33, 65, 160, 3, 40, 1.0), (65, 65, 160, 3, 40, 1.0),
    (33, 33, 160, 3, 40, 4.0), (33, 33, 1, 3, 40, 1.0), (33, 33, 2, 3, 40, 1.0), (5, 5, 160, 1, 256, 1.0), (33, 33, 2, 3, 256, 4.0)])
def test_recurrence_against_float64(dev, P, nwin, T, layers, I, scale):
    sd, win, h64, err32 = rec_case(nwin, T, layers, I, scale)
    pkg()._lib.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream)
    got = S().lstm_fwd(win[:P].to(dev), own_rows(P, dev), layer_weights(sd, dev), T_steps=T)
    assert got.shape == (P, 256)
    check_h(f'P={P} T={T} layers={layers} I={I} scale={scale}', got, h64[:P], err32[:P])


def test_recurrence_window_lists(dev):
    """Overlapping windows of one frame array; windows from different rows; a strided array with NaN wherever no window reads; a
    row without windows."""
    sd = R.state_dict(seed=7, scale=1.0)
    w = layer_weights(sd, dev)
    m64, m32 = R.net(sd, torch.float64), R.net(sd, torch.float32)
    g = torch.Generator().manual_seed(5)

    def ref(frames, slots):
        win = torch.stack([frames[r, s:s + 160] for r, s in slots])
        h64 = R.hidden(m64, win)
        return h64, (R.hidden(m32, win).double() - h64).abs()

    fr = torch.randn(1, 314, 40, generator=g)
    slots = [(0, 0), (0, 77), (0, 154)]
    got = S().lstm_fwd(fr.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev), w)
    check_h('overlapping windows', got, *ref(fr, slots))

    fr = torch.randn(3, 200, 40, generator=g)
    slots = [(2, 5), (0, 40), (1, 0), (2, 40), (0, 0)]
    got = S().lstm_fwd(fr.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev), w)
    check_h('windows from different rows', got, *ref(fr, slots))

    buf = torch.full((4, 250, 64), NAN)                                     # rows 0 and 2 are the array: every other row, 40 of 64 columns
    fr = torch.randn(2, 250, 40, generator=g)
    slots = [(0, 3), (1, 90), (0, 10)]
    cover = torch.zeros(2, 250, dtype=torch.bool)
    for r, s in slots:
        cover[r, s:s + 160] = True
    fr[~cover] = NAN
    buf[::2, :, :40] = fr
    view = buf.to(dev)[::2, :, :40]
    assert view.stride() == (2 * 250 * 64, 64, 1)
    got = S().lstm_fwd(view, torch.tensor(slots, dtype=torch.int32, device=dev), w)
    check_h('strided frames, NaN where no window reads', got, *ref(fr, slots))

    fr = torch.randn(2, 237, 40, generator=g)
    fr[1] = NAN                                                             # the row without windows is never read
    slots = [(0, 0), (0, 77), (1, 0), (1, 77)]
    counts = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    got = S().lstm_fwd(fr.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev), w, counts=counts, P_max=2)
    check_h('a row of zero windows', got[:2], *ref(fr, slots[:2]))
    assert (got[2:] == 0).all()                                             # unused slots are zeroed


@functools.lru_cache(maxsize=None)
def mel_case():
    ns = (1000, 25440, 31519, 31520, 71680)
    T = 72001
    x = np.full((len(ns), T), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = R.tones(n, seed=b)
    x.setflags(write=False)
    return ns, x


@functools.lru_cache(maxsize=None)
def mel_ref(b, pad_mode, normalize=False):
    ns, x = mel_case()
    m = R.mel(x[b, :ns[b]], pad_mode, normalize)
    m.setflags(write=False)
    return m


def check_mel(what, got, want):
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all()
    F = want.shape[0]
    assert (got[F:] == 0).all()                                             # frames past the row's own padded length
    live = want > 0
    assert np.array_equal(got[:F] == 0, ~live)
    err = float((np.abs(got[:F] - want)[live] / want[live]).max())
    print(f'{what}: worst relative error {err:.3e}, error / bar {err / BAR:.3f}')
    assert err <= BAR, (what, err)


@pytest.mark.parametrize('pad_mode', ['reflect', 'constant'])
def test_mel_against_float64(dev, pad_mode):
    ns, x = mel_case()
    xd = torch.from_numpy(np.array(x)).to(dev)
    lengths = torch.tensor(ns, dtype=torch.int32, device=dev)
    pkg()._lib.lib().tdvc_debug_poison_lds(0xFFFFFFFF, torch.cuda.current_stream(dev).cuda_stream)
    mel = S().voice_mel(xd[:, None], lengths=lengths, pad_mode=pad_mode)
    assert mel.shape == (len(ns), 1 + S().window_count(x.shape[1])[1] // 160, 40) and mel.dtype == torch.float32
    for b, n in enumerate(ns):
        check_mel(f'{pad_mode} n={n}', mel[b], mel_ref(b, pad_mode))
    if pad_mode == 'reflect':                                               # an every-other-row view and an expanded row: the same bits
        wide = torch.full((2 * len(ns), x.shape[1]), NAN, device=dev)
        wide[::2] = xd
        assert torch.equal(S().voice_mel(wide[::2], lengths=lengths), mel)
        again = S().voice_mel(xd[4:5].expand(3, -1), lengths=lengths[4:5].expand(3))
        assert all(torch.equal(again[i], mel[4]) for i in range(3))
        full = S().voice_mel(xd[4, :71680])                                 # no lengths, one row [T]
        check_mel('n = T = 71680', full[0], mel_ref(4, 'reflect'))


def test_mel_normalize(dev):
    n = 31520
    quiet, loud = R.tones(n, seed=11, amp=0.003), R.tones(n, seed=12, amp=0.1)
    assert R.gain_of(quiet) > 5 and R.gain_of(loud) == 1.0
    x = torch.full((2, n + 480), NAN)
    x[0, :n], x[1, :n] = torch.from_numpy(quiet), torch.from_numpy(loud)
    lengths = torch.tensor([n, n], dtype=torch.int32, device=dev)
    mel = S().voice_mel(x.to(dev), lengths=lengths, normalize=True)
    check_mel('normalize, quiet row', mel[0], R.mel(quiet, normalize=True))
    check_mel('normalize, loud row', mel[1], R.mel(loud, normalize=True))
    plain = S().voice_mel(x.to(dev), lengths=lengths)
    assert torch.equal(plain[1], mel[1]) and not torch.equal(plain[0], mel[0])


@functools.lru_cache(maxsize=None)
def utterance_case(scale):
    ns = (20000, 31520, 71680)
    T = 71999
    x = np.full((3, T), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = R.tones(n, seed=20 + b)
    sd = R.state_dict(seed=3, scale=scale)
    m64, m32 = R.net(sd, torch.float64), R.net(sd, torch.float32)
    out = []
    for b, n in enumerate(ns):
        mel = R.mel(x[b, :n])
        u64, p64 = R.embed_utterance(m64, mel, n)
        u32, p32 = R.embed_utterance(m32, mel, n)
        out.append((u64, p64, float((u32.double() - u64).abs().max()), float((p32.double() - p64).abs().max())))
    return ns, x, sd, out


@pytest.mark.parametrize('scale', [1.0, 4.0])
def test_embed_utterance_end_to_end(dev, scale):
    ns, x, sd, ref = utterance_case(scale)
    enc = pkg().VoiceEncoder()
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    xd = torch.from_numpy(np.array(x)).to(dev)[:, None]
    lengths = torch.tensor(ns, dtype=torch.int32, device=dev)
    utt, part, counts = enc.embed_utterance(xd, lengths=lengths, return_partials=True)
    assert utt.shape == (3, 256) and part.shape == (3, 5, 256) and counts.tolist() == [1, 2, 5]
    assert torch.isfinite(utt).all()
    for b in range(3):
        u64, p64, eu, ep = ref[b]
        c = p64.shape[0]
        du = float((utt[b].double().cpu() - u64).abs().max())
        dp = float((part[b, :c].double().cpu() - p64).abs().max())
        print(f'scale {scale} n={ns[b]}: utterance {du:.3e} (fp32 CPU {eu:.3e}, error / bar {du / (4 * eu):.3f}), '
              f'windows {dp:.3e} (fp32 CPU {ep:.3e}, error / bar {dp / (4 * ep):.3f})')
        assert du <= 4 * eu and dp <= 4 * ep
        assert (part[b, c:] == 0).all()
    again = enc.embed_utterance(xd, lengths=lengths)
    assert torch.equal(again, utt)                                          # bit-identical from call to call
    one = enc(torch.from_numpy(R.mel(x[2, :ns[2]])[:160].astype(np.float32))[None].to(dev))      # forward: the first window of row 2
    assert float((one[0].double().cpu() - ref[2][1][0]).abs().max()) <= 4 * ref[2][3]
    if scale == 1.0:
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            enc.embed_utterance(xd, lengths=lengths)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = enc.embed_utterance(xd, lengths=lengths)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, utt)


def test_refusals(dev):
    sp = S()
    sd = R.state_dict(seed=1)
    w = layer_weights(sd, dev)
    fr = torch.zeros(1, 200, 40, device=dev)
    slots = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    bad = [tuple(t if i else t[:, :39] for i, t in enumerate(w[0]))] + w[1:]
    with pytest.raises(ValueError, match='lstm_fwd'):
        sp.lstm_fwd(fr, slots, bad)
    with pytest.raises(ValueError, match='lstm_fwd.*160 steps'):
        sp.lstm_fwd(fr, slots, w, T_steps=161)
    w257 = layer_weights(R.state_dict(seed=1, input_size=257, layers=1), dev)
    with pytest.raises(ValueError, match='lstm_fwd.*256'):
        sp.lstm_fwd(torch.zeros(1, 200, 257, device=dev), slots, w257)
    with pytest.raises(ValueError, match='lstm_fwd.*layers'):
        sp.lstm_fwd(fr, slots, w + w[1:2])
    with pytest.raises(ValueError, match='voice_mel'):
        sp.voice_mel(torch.zeros(1, 200, device=dev))
    assert sp.voice_mel(torch.zeros(1, 200, device=dev), pad_mode='constant').shape == (1, 161, 40)
    with pytest.raises(ValueError, match='voice_mel'):
        sp.voice_mel(torch.zeros(1, 400, device=dev), pad_mode='edge')
    with pytest.raises(ValueError, match='VoiceEncoder.forward'):
        pkg().VoiceEncoder().to(dev)(torch.zeros(1, 159, 40, device=dev))


def test_speaker_similarity_on_the_device(dev):
    te, tt, re_, rs = (torch.from_numpy(a) for a in R.similarity_case())
    cpu = pkg().speaker_similarity(te, tt, re_, rs, 16)
    got = pkg().speaker_similarity(te.to(dev), tt.to(dev), re_.to(dev), rs.to(dev), 16)
    assert got['cos'].is_cuda and torch.equal(got['pred'].cpu(), cpu['pred'])
    assert float((got['cos'].cpu() - cpu['cos']).abs().max()) <= 64 * 2.0 ** -24
    assert float((got['centroids'].cpu() - cpu['centroids']).abs().max()) <= 8 * 2.0 ** -24
    assert abs(float(got['accuracy']) - float(cpu['accuracy'])) < 1e-6
