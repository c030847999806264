"""F0 extraction on the device: the reference's YIN pitch tracker (util/yin.py, `estimate` and its `soft` variant; the calls
train.py:238, :548 and :634 keep commented out) as one HIP launch per call (csrc/pitch_yin.hip, tdvc_yin_f0).

`yin_f0` has `estimate`'s signature and return value; `track_f0` gives the [B, 1, T/hop + 1] layout that `infer.convert`,
`infer.shift_f0` and `TrainStep` take. The difference function is summed directly in fp32 instead of through the reference's FFT
autocorrelation: same quantity, without the cancellation at its minimum.
"""
import torch

from . import _lib as L


def _yin(x, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf):
    """x [..., T] (device tensor, last axis dense) -> f0 [..., n_frames] (, cmdf [..., n_frames, tau_max - 1 - tau_min])."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise L.TdvcError('yin_f0: the HIP path needs a CUDA/ROCm tensor (there is no CPU fallback)')
    if x.dim() < 1:
        raise ValueError('yin_f0: signal must be [T], [B, T] or [..., T]')
    x = x.float()
    lead, T = x.shape[:-1], x.shape[-1]
    x2 = x.reshape(-1, T) if x.dim() != 2 else x          # a view wherever the leading axes share one stride
    if T > 1 and x2.stride(-1) != 1:
        x2 = x2.contiguous()
    B = x2.shape[0]
    x_bs = x2.stride(0) if B > 1 else T
    if x_bs < 0:
        x2, x_bs = x2.contiguous(), T
    lib = L.lib()
    nf = lib.tdvc_yin_num_frames(T, tau_max, stride)
    n = tau_max - 1 - tau_min
    f0 = torch.empty(B, max(nf, 0), dtype=torch.float32, device=x.device)
    cmdf = torch.empty(B, max(nf, 0), max(n, 0), dtype=torch.float32, device=x.device) if return_cmdf else None
    L.check(lib.tdvc_yin_f0(x2.data_ptr(), x_bs, B, T, tau_min, tau_max, stride, float(threshold), int(bool(soft)), float(sample_rate),
                            f0.data_ptr(), cmdf.data_ptr() if return_cmdf else None, torch.cuda.current_stream(x.device).cuda_stream))
    f0 = f0.reshape(*lead, nf)
    return (f0, cmdf.reshape(*lead, nf, n)) if return_cmdf else f0


def yin_f0(signal, sample_rate, pitch_min=20, pitch_max=20000, frame_stride=0.01, threshold=0.1, soft=False, return_cmdf=False):
    """YIN pitch of a signal [T], [B, T] or [..., T] -> [..., n_frames] in Hz, 0 = non-periodic frame (reference: util/yin.py:24-85,
    same arguments). Frames of 2*sample_rate/pitch_min samples every frame_stride seconds; n_frames = (max(T, L) - 1) // stride + 1.
    return_cmdf=True also returns the cumulative-mean-normalised difference [..., n_frames, tau_max - 1 - tau_min]."""
    tau_min = int(sample_rate / pitch_max)
    tau_max = int(sample_rate / pitch_min)
    stride = int(frame_stride * sample_rate)
    return _yin(signal, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf)


def track_f0(signal, hop=64, sample_rate=16000, pitch_min=60, pitch_max=500, threshold=0.1):
    """signal [B, 1, T] -> F0 track [B, 1, T // hop + 1] in Hz, 0 = unvoiced: the frame count of the reference's CREPE front end
    (pad=True), which is what `infer.convert`, `infer.shift_f0` and `TrainStep` take. YIN yields T // hop frames for an utterance
    of whole hops, so the last frame is repeated once; `f0_to_excitation` drops that frame, as the reference does."""
    if signal.dim() != 3 or signal.shape[1] != 1:
        raise ValueError('track_f0: signal must be [B, 1, T]')
    T = signal.shape[-1]
    f0 = _yin(signal[:, 0], sample_rate, int(sample_rate / pitch_max), int(sample_rate / pitch_min), int(hop), threshold, False, False)
    idx = torch.arange(T // int(hop) + 1, device=f0.device).clamp_(max=f0.shape[-1] - 1)
    return f0.index_select(-1, idx).unsqueeze(1)
