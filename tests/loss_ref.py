"""Float64 references of the view-based loss layer (td-vc-gan_amd/losses.py) on plain tensor slices, with torch autograd for the
gradients, and the seeded inputs of the spectral-loss test (tests/test_loss_layer_gpu.py; their conditions are asserted without
a GPU by tests/test_loss_layer_cpu.py). Every function computes in the dtype of its inputs: float64 for the reference, float32
for the stock-torch evaluation that sets the bar of the spectral gradient."""
import importlib

import torch

FLOOR = 1e-5
SPEC_B, SPEC_T, SPEC_FFTS = 2, 2304, (512, 1024, 2048)      # 2304 = 2048 + 256: short, and longer than n_fft = 2048's reflect pad
SPEC_ZEROS = (896, 1408)                                     # row 1 is exactly 0 here: frame 9 of n_fft = 512 sees nothing else
SPEC_SEED = 6                                                # of seeds 0..11, 6 and 9 meet the conditions test_loss_layer_cpu.py asserts


def lsgan(outs, ranges, target):
    """sum_i mean((o_i[lo_i:hi_i] - target)^2); ranges[i] = (lo, hi) rows of outs[i] (None: all of them)."""
    tot = 0
    for o, r in zip(outs, ranges):
        lo, hi = (0, o.shape[0]) if r is None else r
        tot = tot + ((o[lo:hi] - target) ** 2).mean()
    return tot


def lsgan_split(outs, B):
    """(sum_i mean((o_i[:B] - 1)^2), sum_i mean(o_i[B:]^2))."""
    return sum(((o[:B] - 1.0) ** 2).mean() for o in outs), sum((o[B:] ** 2).mean() for o in outs)


def feat_l1(pairs):
    """sum mean|a[lo:hi] - b[rlo:rhi]| over pairs (a, lo, hi, b, rlo, rhi); b carries no gradient."""
    tot = 0
    for a, lo, hi, b, rlo, rhi in pairs:
        tot = tot + (a[lo:hi] - b[rlo:rhi].detach()).abs().mean()
    return tot


def mel_power(x, n_fft, n_mels=80, sr=16000):
    """x [B, 1, T] -> mel power [B, n_mels, 1 + T // hop]: torch.stft (periodic Hann, centre, reflect pad, hop n_fft / 4), power 2,
    and the float64 filterbank of losses._mel_filterbank cast to x's dtype."""
    LS = importlib.import_module('td-vc-gan_amd.losses')
    win = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    spec = torch.stft(x[:, 0], n_fft, hop_length=n_fft // 4, win_length=n_fft, window=win, center=True, pad_mode='reflect',
                      return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    fb = torch.from_numpy(LS._mel_filterbank(n_fft // 2 + 1, n_mels, sr)).to(x.dtype)
    return torch.einsum('fm,bfn->bmn', fb, power)


def log_mel_l1(signal, ref, n_ffts, separated=False):
    """sum over n_ffts of mean|log clamp(mel(signal), 1e-5) - log clamp(mel(ref), 1e-5)|; ref carries no gradient."""
    terms = [(mel_power(signal, n).clamp(min=FLOOR).log() - mel_power(ref.detach(), n).clamp(min=FLOOR).log()).abs().mean()
             for n in n_ffts]
    return (sum(terms), terms) if separated else sum(terms)


def log_mel_l1_conv(signal, ref, n_ffts):
    """The same term evaluated by stock torch through the chain of operations the product runs: F.pad(mode='reflect'), the STFT as
    a strided F.conv1d with MelSpec's windowed DFT basis, power, the mel projection as a 1x1 F.conv1d with MelSpec's filterbank,
    log-L1. In float32 this is the evaluation whose error against float64 sets the bar of the spectral gradient."""
    import torch.nn.functional as F
    LS = importlib.import_module('td-vc-gan_amd.losses')
    tot = 0
    for n in n_ffts:
        ms = LS.MelSpec(16000, n, 80)
        basis, fb = ms.basis.to(signal.dtype), ms.fb.to(signal.dtype)

        def mel(x):
            spec = F.conv1d(F.pad(x, (n // 2, n // 2), mode='reflect'), basis, stride=n // 4)
            h = spec.shape[1] // 2
            return F.conv1d(spec[:, :h] ** 2 + spec[:, h:] ** 2, fb)
        tot = tot + (mel(signal).clamp(min=FLOOR).log() - mel(ref.detach()).clamp(min=FLOOR).log()).abs().mean()
    return tot


def spec_inputs(seed=SPEC_SEED):
    """(signal, ref) fp32 [2, 1, 2304]: a few partials plus noise each, different on the two sides; row 1 of both is exactly 0 on
    SPEC_ZEROS, so the mel bins of n_fft = 512's frame 9 are exactly 0, below the floor, on both sides."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(SPEC_T, dtype=torch.float64) / 16000.0
    out = []
    for side in range(2):
        x = 0.05 * torch.randn(SPEC_B, SPEC_T, generator=gen, dtype=torch.float64)
        for b in range(SPEC_B):
            for f in (150.0 + 70.0 * b + 15.0 * side, 900.0 + 130.0 * side, 3100.0 - 200.0 * b):
                amp = 0.1 + 0.3 * float(torch.rand(1, generator=gen))
                x[b] += amp * torch.sin(2 * torch.pi * f * t + 6.28 * float(torch.rand(1, generator=gen)))
        x[1, SPEC_ZEROS[0]:SPEC_ZEROS[1]] = 0.0
        out.append(x.float().unsqueeze(1))
    return out[0], out[1]


def spec_conditions(signal, ref, n_ffts=SPEC_FFTS):
    """-> (smallest non-zero mel bin of either side, smallest |log a - log b| among the bins above the floor on both sides,
    number of bins that are exactly 0 on both sides), on the float64 reference."""
    lo, gap, zeros = float('inf'), float('inf'), 0
    for n in n_ffts:
        a, b = mel_power(signal.double(), n), mel_power(ref.double(), n)
        for m in (a, b):
            lo = min(lo, float(m[m != 0].min()))
        assert bool(((a == 0) == (b == 0)).all())
        zeros += int((a == 0).sum())
        live = (a > FLOOR) & (b > FLOOR)
        gap = min(gap, float((a[live].log() - b[live].log()).abs().min()))
    return lo, gap, zeros
