"""Float64 restatement of the backward of the CREPE tracker with respect to its signal, as include/tdvc.h defines it (tdvc_crepe_conv_train,
tdvc_crepe_conv_bwd, tdvc_crepe_head_bwd, tdvc_crepe_frames_bwd), in stock torch ops on top of tests/crepe_ref.py. Two parts:

  codes(sd, frames)   the pooling decision of every output of the six blocks and its two margins: |v_even - v_odd| (how far the pair is
                      from changing its winner) and |z_winner| (how far the winner's ReLU is from switching)
  backward(...)       the manual backward FOR GIVEN DECISIONS: with the decisions fixed the network is a linear map from the head's
                      gradient to the frames' gradient, so an implementation is compared as that linear map, with no exclusions.
                      Parametrised by dtype: the same formulae in fp32 on the CPU give the error bar.

tests/test_crepe_grad_cpu.py pins `backward` under its own codes to torch.autograd through crepe_ref."""
import torch
import torch.nn.functional as F

import crepe_ref as R

LIN = (1024, 128, 64, 32, 16, 8)      # input positions of the six blocks


def fold(sd, i, dtype=torch.float64):
    """(scale, shift) of block i: evaluated in float64 and rounded once, as crepe.fold_bn does."""
    p = f'conv{i}_BN'
    scale = sd[p + '.weight'].double() / torch.sqrt(sd[p + '.running_var'].double() + R.BN_EPS)
    shift = sd[p + '.bias'].double() - sd[p + '.running_mean'].double() * scale
    return scale.to(dtype), shift.to(dtype)


def layer_codes(sd, i, x, dtype=torch.float64):
    """Block i on x [N, Cin, L] -> dict(y [N, Cout, Lc / 2], code uint8, margin_v, margin_z, dead): code 0 the winner's z <= 0, 1 the even
    position wins (also on a tie) and is on, 2 the odd one; dead: both z of the pair <= 0 (code 0 whatever the winner)."""
    c = lambda k: sd[k].to(dtype)
    p = f'conv{i}'
    xp = F.pad(x.to(dtype)[..., None], (0, 0) + R.PADS[i - 1])
    z = F.conv2d(xp, c(p + '.weight'), c(p + '.bias'), stride=(R.STRIDES[i - 1], 1))[..., 0]
    scale, shift = fold(sd, i, dtype)
    v = F.relu(z) * scale[None, :, None] + shift[None, :, None]
    ze, zo, ve, vo = z[..., 0::2], z[..., 1::2], v[..., 0::2], v[..., 1::2]
    odd = vo > ve
    zw = torch.where(odd, zo, ze)
    code = torch.where(zw <= 0, 0, torch.where(odd, 2, 1)).to(torch.uint8)
    return dict(y=torch.where(odd, vo, ve), code=code, margin_v=(ve - vo).abs(), margin_z=zw.abs(), dead=(ze <= 0) & (zo <= 0), z=z, v=v)


def codes(sd, frames, dtype=torch.float64):
    """Normalised frames [N, 1024] -> (list of the six layer_codes dicts, activations [N, 360])."""
    x = frames.to(dtype)[:, None, :]
    out = []
    for i in range(1, 7):
        d = layer_codes(sd, i, x, dtype)
        out.append(d)
        x = d['y']
    return out, R.head(sd, x[..., None], dtype)


def unpool(dy, code, scale):
    """dz [N, Cout, Lc]: dy scale at the position the code names, 0 elsewhere."""
    g = dy * scale[None, :, None]
    dz = torch.zeros(dy.shape[0], dy.shape[1], 2 * dy.shape[2], dtype=dy.dtype)
    dz[..., 0::2] = torch.where(code == 1, g, torch.zeros_like(g))
    dz[..., 1::2] = torch.where(code == 2, g, torch.zeros_like(g))
    return dz


def block_backward(sd, i, dy, code, dtype=torch.float64, scale=None):
    """dy [N, Cout, Lc / 2], code -> dx [N, Cin, Lin]: unpool, mask, scale, the conv's input gradient (the transposed conv, cropped by
    the padding)."""
    scale = fold(sd, i, dtype)[0] if scale is None else scale.to(dtype)
    dz = unpool(dy.to(dtype), code, scale)
    full = F.conv_transpose2d(dz[..., None], sd[f'conv{i}.weight'].to(dtype), stride=(R.STRIDES[i - 1], 1))[..., 0]
    lo = R.PADS[i - 1][0]
    return full[..., lo:lo + LIN[i - 1]]


def head_backward(sd, act, target, gL, dtype=torch.float64, dact=None):
    """act, target [N, 360] (frame-major) -> dx6 [N, C6, 4]: dlogit = gL 2 (act - target) / numel act (1 - act) (or dact act (1 - act)),
    times the classifier weight, back through the position-major flatten."""
    a = act.to(dtype)
    up = dact.to(dtype) if dact is not None else gL * 2.0 * (a - target.to(dtype)) / a.numel()
    dflat = (up * a * (1 - a)) @ sd['classifier.weight'].to(dtype)
    return dflat.reshape(a.shape[0], 4, -1).permute(0, 2, 1)


def backward(sd, code_list, act, target, gL, dtype=torch.float64):
    """The gradient of gL * mean((act - target)^2) with respect to the normalised frames [N, 1024], for the given decisions (six code
    arrays); act, target [N, 360]."""
    dx = head_backward(sd, act, target, gL, dtype)
    for i in range(6, 0, -1):
        dx = block_backward(sd, i, dx, code_list[i - 1], dtype)
    return dx[:, 0]


def frames_backward(x, g, hop=64, dtype=torch.float64):
    """One row x [n] and the gradient g [F, 1024] of its normalised frames -> d x [n]: per frame dxf = (g - mean(g) - y sum(g y) / 1023) /
    den for std > 1e-10, (g - mean(g)) / den otherwise, then the overlap-add over the frames that cover a sample; the padding receives
    nothing."""
    x = torch.as_tensor(x).to(dtype)
    n = x.shape[0]
    Fn = 1 + n // hop
    xp = F.pad(x, (R.WINDOW // 2, R.WINDOW // 2))
    fr = torch.stack([xp[f * hop:f * hop + R.WINDOW] for f in range(Fn)])
    mean = fr.mean(1, keepdim=True)
    std = (fr - mean).std(1, keepdim=True)
    den = torch.clamp(std, min=1e-10)
    y = (fr - mean) / den
    g = g.to(dtype)
    gc = g - g.mean(1, keepdim=True)
    dxf = torch.where(std > 1e-10, gc - y * (g * y).sum(1, keepdim=True) / (R.WINDOW - 1), gc) / den
    out = torch.zeros(n + R.WINDOW, dtype=dtype)
    for f in range(Fn):
        out[f * hop:f * hop + R.WINDOW] += dxf[f]
    return out[R.WINDOW // 2:R.WINDOW // 2 + n]


def roll_batches(input, shifts, dim):
    """util.roll_batches of the reference, restated literally (util/__init__.py:91-102)."""
    repeat = [d if i != dim else 1 for i, d in enumerate(input.shape)]
    view = [1 if i != dim else -1 for i in range(input.ndim)]
    idx = torch.arange(input.shape[dim], device=input.device).view(view).repeat(repeat)
    view = [1 if i != 0 else -1 for i in range(input.ndim)]
    idx = (idx - shifts.view(view)) % input.shape[dim]
    return torch.gather(input, dim, idx)


def conversion_target(f0_src, act_src, perm, get_shift):
    """train.py:245-252, restated literally; get_shift is util.crepe.get_shift's stand-in (bin(target) - bin(source))."""
    f0_tgt = f0_src[perm]
    mu_tgt = torch.sum((f0_tgt > 0) * torch.log(f0_tgt + 1e-6), -1, keepdim=True) / (torch.sum(f0_tgt > 0, -1, keepdim=True) + 1e-6)
    mu_src = torch.sum((f0_src > 0) * torch.log(f0_src + 1e-6), -1, keepdim=True) / (torch.sum(f0_src > 0, -1, keepdim=True) + 1e-6)
    f0_conv_tgt = torch.zeros(f0_src.shape)
    f0_conv_tgt[f0_src > 0] = torch.exp(torch.log(f0_src + 1e-6) + mu_tgt - mu_src)[f0_src > 0]
    return f0_conv_tgt, roll_batches(act_src, get_shift(torch.exp(mu_src), torch.exp(mu_tgt)), 1)


def undecided(d, tau_v, tau_z):
    """The pooled outputs of a layer_codes dict whose decision an fp32 evaluation may take differently: a margin below its tau, unless
    both z of the pair are <= 0 (code 0 either way)."""
    return ((d['margin_v'] < tau_v) | (d['margin_z'] < tau_z)) & ~d['dead']


def taus(d64, d32):
    """4 x the largest difference between the fp32 and the float64 evaluation, for v and for z."""
    return 4 * float((d32['v'].double() - d64['v']).abs().max()), 4 * float((d32['z'].double() - d64['z']).abs().max())
