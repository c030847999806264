"""F0 extraction on the device: the reference's YIN pitch tracker (util/yin.py, `estimate` and its `soft` variant; the calls
train.py:238, :548 and :634 keep commented out) as one HIP launch per call (csrc/pitch_yin.hip, tdvc_yin_f0).

`yin_f0` has `estimate`'s signature and return value; `track_f0` gives the [B, 1, T/hop + 1] layout that `infer.convert`,
`infer.shift_f0` and `TrainStep` take. The difference function is summed directly in fp32 instead of through the reference's FFT
autocorrelation: same quantity, without the cancellation at its minimum.

The soft variant is differentiable: with `soft=True`, an input that requires grad and grad mode on, the F0 track carries a
`grad_fn` whose backward is tdvc_yin_soft_bwd (csrc/pitch_yin_bwd.hip: per-frame gradient, then a gather; no atomics). The hard
search is piecewise constant and the CMDF of `return_cmdf=True` is a diagnostic output: neither is differentiable.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L


class _YinSoftFn(torch.autograd.Function):
    """Soft YIN on x2 [B, T] (rows x_bs apart, last axis dense). The forward is the plain tdvc_yin_f0 call (same bits as without
    autograd); the backward recomputes the forward's intermediates on the device from x2, which is all it keeps."""

    @staticmethod
    def forward(ctx, x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, return_cmdf):
        f0, cmdf = _launch(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, True, return_cmdf)
        ctx.save_for_backward(x2)
        ctx.args = (x_bs, sample_rate, tau_min, tau_max, stride, threshold)
        if not return_cmdf:
            return f0
        ctx.mark_non_differentiable(cmdf)
        return f0, cmdf

    @staticmethod
    @once_differentiable                    # the backward is a raw library call: a second derivative raises instead of returning a graph-less tensor
    def backward(ctx, gy, *_):
        (x2,) = ctx.saved_tensors
        x_bs, sample_rate, tau_min, tau_max, stride, threshold = ctx.args
        B, T = x2.shape
        gy = gy.contiguous().float()
        lib = L.lib()
        nbytes = lib.tdvc_yin_soft_bwd_workspace(B, T, tau_max, stride)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)      # caching allocator: graph-safe
        dx = torch.empty(B, T, dtype=torch.float32, device=x2.device)      # the kernel writes every element
        L.check(lib.tdvc_yin_soft_bwd(x2.data_ptr(), x_bs, B, T, tau_min, tau_max, stride, float(threshold), float(sample_rate),
                                      gy.data_ptr(), dx.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(x2.device).cuda_stream))
        return (dx,) + (None,) * 7


def _launch(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf):
    """x2 [B, T] -> (f0 [B, n_frames], cmdf [B, n_frames, n] or None): one tdvc_yin_f0 call."""
    B, T = x2.shape
    lib = L.lib()
    nf = lib.tdvc_yin_num_frames(T, tau_max, stride)
    n = tau_max - 1 - tau_min
    f0 = torch.empty(B, max(nf, 0), dtype=torch.float32, device=x2.device)
    cmdf = torch.empty(B, max(nf, 0), max(n, 0), dtype=torch.float32, device=x2.device) if return_cmdf else None
    L.check(lib.tdvc_yin_f0(x2.data_ptr(), x_bs, B, T, tau_min, tau_max, stride, float(threshold), int(bool(soft)), float(sample_rate),
                            f0.data_ptr(), cmdf.data_ptr() if return_cmdf else None, torch.cuda.current_stream(x2.device).cuda_stream))
    return f0, cmdf


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
    if soft and x2.requires_grad and torch.is_grad_enabled():
        # differentiable path: the layout steps above are torch ops, so the gradient returns in the input's shape
        out = _YinSoftFn.apply(x2, x_bs, sample_rate, tau_min, tau_max, stride, threshold, bool(return_cmdf))
        f0, cmdf = out if return_cmdf else (out, None)
    else:
        f0, cmdf = _launch(x2.detach(), x_bs, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf)
    nf, n = f0.shape[-1], tau_max - 1 - tau_min
    f0 = f0.reshape(*lead, nf)
    return (f0, cmdf.reshape(*lead, nf, n)) if return_cmdf else f0


def yin_f0(signal, sample_rate, pitch_min=20, pitch_max=20000, frame_stride=0.01, threshold=0.1, soft=False, return_cmdf=False):
    """YIN pitch of a signal [T], [B, T] or [..., T] -> [..., n_frames] in Hz, 0 = non-periodic frame (reference: util/yin.py:24-85,
    same arguments). Frames of 2*sample_rate/pitch_min samples every frame_stride seconds; n_frames = (max(T, L) - 1) // stride + 1.
    return_cmdf=True also returns the cumulative-mean-normalised difference [..., n_frames, tau_max - 1 - tau_min].
    soft=True on a signal that requires grad gives a differentiable track (the gradient has the signal's shape); the hard track
    and the CMDF carry no grad_fn."""
    tau_min = int(sample_rate / pitch_max)
    tau_max = int(sample_rate / pitch_min)
    stride = int(frame_stride * sample_rate)
    return _yin(signal, sample_rate, tau_min, tau_max, stride, threshold, soft, return_cmdf)


def track_f0(signal, hop=64, sample_rate=16000, pitch_min=60, pitch_max=500, threshold=0.1, soft=False):
    """signal [B, 1, T] -> F0 track [B, 1, T // hop + 1] in Hz, 0 = unvoiced: the frame count of the reference's CREPE front end
    (pad=True), which is what `infer.convert`, `infer.shift_f0` and `TrainStep` take. YIN yields T // hop frames for an utterance
    of whole hops, so the last frame is repeated once; `f0_to_excitation` drops that frame, as the reference does.
    soft=True selects the softmax-weighted period, differentiable with respect to a signal that requires grad."""
    if signal.dim() != 3 or signal.shape[1] != 1:
        raise ValueError('track_f0: signal must be [B, 1, T]')
    T = signal.shape[-1]
    f0 = _yin(signal[:, 0], sample_rate, int(sample_rate / pitch_max), int(sample_rate / pitch_min), int(hop), threshold, soft, False)
    idx = torch.arange(T // int(hop) + 1, device=f0.device).clamp_(max=f0.shape[-1] - 1)
    return f0.index_select(-1, idx).unsqueeze(1)
