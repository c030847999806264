"""What every operator wrapper (pitch, corrupt, resample, evaluate, util) does on the host before its launch, defined once: the
device check, strided [B, T] / [B, N, D] views with the strides the C ABI takes, per-row lengths and parameter vectors as the kernels
read them, scratch, optional pointers, the current stream, host tables uploaded once per device (the DFT table prefix of the two mel
front ends among them), and TDVC_EUNSUPPORTED as ValueError. Nothing here synchronises with the host. Torch tensors
have no negative strides (as_strided refuses them, flip copies), so the layout helpers do not look for them."""
import numpy as np
import torch

from . import _lib as L

_host_tables, _device_tables = {}, {}


def need_device(who, *tensors):
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.TdvcError(f'{who}: the HIP path needs CUDA/ROCm tensors (there is no CPU fallback)')


def dev_key(device):
    """Hashable identity of anything torch.device() accepts; 'cuda' without an index is the current device."""
    device = torch.device(device)
    return (device.type, torch.cuda.current_device() if device.index is None and device.type == 'cuda' else device.index)


def stream(t):
    """The current stream of a tensor's device, as the void* the C ABI takes."""
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def scratch(nbytes, device):
    """Workspace from the caching allocator (graph-safe); at least one byte, so that data_ptr() is valid."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def check(who, rc):
    """_lib.check, with TDVC_EUNSUPPORTED (an argument the kernels do not take) as the caller's ValueError."""
    if rc == L.EUNSUPPORTED:
        raise ValueError(f'{who}: {L.lib().tdvc_last_error().decode()}')
    L.check(rc)


def rows2(who, signal, any_lead=False, keep_grad=False):
    """signal [T], [B, T] or [B, 1, T] ([..., T] with any_lead) -> (x2 [B, T] fp32 with a dense last axis, row stride in elements,
    leading shape). A view wherever the leading axes share one stride; only a signal whose last axis is not dense is copied. A
    single row reports T as its stride. keep_grad leaves the signal attached: every step here is a torch op, so a gradient
    with respect to x2 returns in the signal's shape."""
    if not (signal.dim() >= 1 if any_lead else signal.dim() in (1, 2) or (signal.dim() == 3 and signal.shape[1] == 1)):
        raise ValueError(f'{who}: signal must be [T], [B, T] or {"[..., T]" if any_lead else "[B, 1, T]"}')
    x = (signal if keep_grad else signal.detach()).float()
    lead, T = x.shape[:-1], x.shape[-1]
    x2 = x if x.dim() == 2 else x.reshape(lead.numel(), T)
    if T > 1 and x2.stride(1) != 1:
        x2 = x2.contiguous()
    return x2, (x2.stride(0) if x2.shape[0] > 1 else T), tuple(lead)


def frames3(who, t):
    """t [N, D] or [..., N, D] -> (t3 [B, N, D] fp32 detached, batch stride, frame stride), in elements. A view unless the last
    axis is not dense or the frame stride is below D (expanded or overlapping frames), which are copied. A single pair reports
    N * D, a single frame D."""
    if t.dim() < 2:
        raise ValueError(f'{who}: needs [N, D] or [..., N, D], got {tuple(t.shape)}')
    t = t.detach().float()
    N, D = t.shape[-2:]
    t3 = t if t.dim() == 3 else t.reshape(t.shape[:-2].numel(), N, D)
    if (D > 1 and t3.stride(2) != 1) or (N > 1 and t3.stride(1) < D):
        t3 = t3.contiguous()
    return t3, (t3.stride(0) if t3.shape[0] > 1 else N * D), (t3.stride(1) if N > 1 else D)


def device_lengths(who, lengths, B, device, move=False, any_shape=False):
    """lengths (None, a sequence or a tensor) -> None or int32 contiguous [B] on `device`. A sequence is uploaded; a tensor must be
    on a device already (TdvcError) unless `move` takes it there. The shape must be (B,) unless `any_shape` takes any B elements."""
    if lengths is None:
        return None
    if not torch.is_tensor(lengths):
        lengths = torch.as_tensor(lengths, device=device)
    elif move:
        lengths = lengths.to(device)
    else:
        need_device(who, lengths)
    if lengths.numel() != B if any_shape else lengths.shape != (B,):
        raise ValueError(f'{who}: lengths must be [{B}]' + (' or any shape of that many elements' if any_shape else ''))
    return lengths.reshape(-1).to(torch.int32).contiguous()


def vec(who, t, n, name='a vector'):
    """A parameter of n elements in any shape -> flat fp32 contiguous device tensor [n], detached."""
    need_device(who, t)
    if t.numel() != n:
        raise ValueError(f'{who}: {name} has {t.numel()} elements, expected {n}')
    return t.detach().float().contiguous().reshape(-1)


def dft_tables(n_fft, window):
    """float64 [cos | sin | window] of 2 pi i / n_fft, n_fft values each: the table of csrc/dft400.h up to the caller's filterbank.
    window: (a, b) for a - b cos (Hann 0.5, 0.5; Hamming 0.54, 0.46), or the n_fft values themselves."""
    ang = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    window = window[0] - window[1] * np.cos(ang) if len(window) == 2 else np.asarray(window, dtype=np.float64).reshape(n_fft)
    return np.concatenate([np.cos(ang), np.sin(ang), window])


def host_table(key, build):
    """build() once per key; a build that raises leaves nothing behind."""
    if key not in _host_tables:
        _host_tables[key] = build()
    return _host_tables[key]


def device_table(device, key, build, upload=lambda h, device: torch.tensor(h, device=device)):
    """host_table(key, build) on `device`, uploaded once per key and device: a repeated call copies nothing from the host and can
    be captured into a graph. `upload(host value, device)` defaults to one tensor of the host array's dtype."""
    k = (key, dev_key(device))
    if k not in _device_tables:
        _device_tables[k] = upload(host_table(key, build), device)
    return _device_tables[k]
