"""Float64 reference of the sine + noise excitation (tdvc_f0_to_excitation, csrc/misc_kernels.hip) and the cases that
tests/test_excitation_gpu.py runs; tests/test_loss_layer_cpu.py pins both without a GPU.

The definition is the kernel's header comment and synth.excitation_from_f0: drop the last frame, omega = 2 pi f0 / sr per frame,
nearest-upsampled by `step`, replaced by the align_corners=False linear value where both neighbouring frames are > 0, cumulative
phase, 0.1 sin(phase + phi0) + 0.003 n_v on voiced samples and (0.1 / 3) n_u where omega == 0. Unlike the numpy restatement in
synth.py nothing is rounded to fp32, and the draws are arguments."""
import numpy as np

# (n_frames, step) -> T = (n_frames - 1) * step. The kernel gives each of its 256 threads per = ceil(T / 256) consecutive samples.
SHAPES = [(2, 1), (2, 64), (5, 64), (6, 64), (86, 3), (87, 3), (141, 64), (1121, 64)]
SHAPE_IDS = ['T1', 'T64_below_256', 'T256', 'T320_per2_empty_tail', 'T255_odd_step', 'T258_odd_step', 'T8960_product', 'T71680_longest']
PATTERNS_A = ('constant', 'unvoiced', 'alternating')
PATTERNS_B = ('runs_1_2', 'first_unvoiced', 'last_voiced')
MIXED = ('alternating', 'runs_1_2', 'first_unvoiced', 'last_voiced')       # voiced AND unvoiced frames once there are >= 4 frames
_CYCLES = {'runs_1_2': (1, 0, 1, 1, 0, 0), 'first_unvoiced': (0, 1, 1, 1, 0, 1), 'last_voiced': (1, 1, 0, 1, 0, 0)}


def excitation(f0, noise_v, noise_u, start_phase, step, sr=16000, linear=True):
    """f0 [B, 1, n_frames] in Hz (0 = unvoiced; the last frame is dropped and never read), noise_v / noise_u [B, 1, T] standard-normal
    draws, start_phase in radians -> (exc, unvoiced, A), all [B, 1, T] with T = (n_frames - 1) * step: the float64 excitation,
    the mask of the samples with omega == 0, and the magnitude of the terms of each sample (0.1 + 0.003 |n_v| voiced,
    |(0.1 / 3) n_u| unvoiced). Each branch takes only its own draw: the other one may hold NaN there."""
    f0 = np.asarray(f0, np.float64)[:, :, :-1]
    n = f0.shape[2]
    T = n * int(step)
    w = 2.0 * np.pi * f0 / sr
    up = np.repeat(w, step, axis=-1)
    if linear:
        src = np.clip((np.arange(T) + 0.5) / step - 0.5, 0.0, None)
        i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        lam = src - i0
        w0, w1 = w[..., i0], w[..., i1]
        up = np.where((w0 > 0) & (w1 > 0), w0 * (1.0 - lam) + w1 * lam, up)
    phase = np.cumsum(up, axis=-1) + float(start_phase)
    unv = up == 0
    nv = np.where(unv, 0.0, np.asarray(noise_v, np.float64))
    nu = np.where(unv, np.asarray(noise_u, np.float64), 0.0)
    exc = np.where(unv, nu * (0.1 / 3.0), 0.1 * np.sin(phase) + nv * 0.003)
    A = np.where(unv, np.abs(nu * (0.1 / 3.0)), 0.1 + 0.003 * np.abs(nv))
    return exc, unv, A


def voiced_frames(pattern, n):
    """The voiced (1) / unvoiced (0) flag of each of the n kept frames of an F0 pattern."""
    i = np.arange(n)
    if pattern == 'constant':
        return np.ones(n, np.int64)
    if pattern == 'unvoiced':
        return np.zeros(n, np.int64)
    if pattern == 'alternating':                 # single voiced and unvoiced frames in turn, the first one voiced
        return (i % 2 == 0).astype(np.int64)
    cyc = np.array(_CYCLES[pattern])
    if pattern == 'last_voiced':                 # the cycle counted from the last kept frame, which is voiced
        return cyc[(n - 1 - i) % len(cyc)]
    return cyc[i % len(cyc)]                     # runs_1_2: V U VV UU ...;  first_unvoiced: U VVV U V ...


def voiced_runs(v):
    """Lengths of the maximal runs of voiced frames."""
    runs, k = [], 0
    for x in list(v) + [0]:
        if x:
            k += 1
        elif k:
            runs.append(k)
            k = 0
    return runs


def make_case(n_frames, step, patterns, seed=0):
    """One call of the GPU test: B = len(patterns) rows with a different F0 pattern each. Voiced frames carry a seeded F0 that
    differs from frame to frame (440 .. 500 Hz on the longest row so that the phase passes 10^4 rad, 90 .. 300 Hz otherwise); the
    dropped last frame is NaN in every row. Returns fp32 arrays f0 [B, 1, n_frames], noise_v, noise_u [B, 1, T] and the row
    patterns; noise_v is NaN wherever the reference says unvoiced and noise_u wherever it says voiced."""
    n = n_frames - 1
    T = n * step
    rs = np.random.RandomState(1000 * n_frames + 10 * step + seed)
    lo, hi = (440.0, 500.0) if n_frames > 1000 else (90.0, 300.0)
    f0 = np.zeros((len(patterns), 1, n_frames), np.float32)
    for b, p in enumerate(patterns):
        f0[b, 0, :n] = np.where(voiced_frames(p, n) > 0, rs.uniform(lo, hi, size=n), 0.0)
    f0[:, :, n] = np.nan
    nv = rs.randn(len(patterns), 1, T).astype(np.float32)
    nu = rs.randn(len(patterns), 1, T).astype(np.float32)
    unv = np.repeat(f0[:, :, :n] == 0, step, axis=-1)
    nv[unv] = np.nan
    nu[~unv] = np.nan
    return dict(f0=f0, noise_v=nv, noise_u=nu, step=step, patterns=tuple(patterns), T=T)
