"""Times the backward of the CREPE tracker (tdvc_crepe_head_bwd, the six tdvc_crepe_conv_bwd, tdvc_crepe_frames_bwd) and the whole
activation-MSE lambda_f0 term (losses.f0_crepe_loss, forward + backward) on the GPU, beside the forward launches of the same run and
beside the same term built from stock torch fp32 ops with autograd on the same device.

    python tools/bench_crepe_bwd.py [--iters 50] [--warmup 5] [--rounds 5] [--torch-iters 5] [--out profiles/crepe_bwd_bench.txt]

Shapes: `tiny` at 16 x 16000 (a training batch) and 1 x 71680 (the longest inference segment), hop 64, seeded weights in the recipe of
tests/crepe_ref.py. Device time from events around `iters` back-to-back calls after a warm-up, the variants alternating in rounds so
that drift hits all of them; the median round is reported, with the spread. One JSON line per shape: microseconds for each conv
layer's forward (tdvc_crepe_conv), training-mode forward (tdvc_crepe_conv_train) and backward launch with their ratio, for the head
and frames backward, for forward + backward of f0_crepe_loss, for the stock-torch term, and the term's share of a 52 ms train step.
"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdvc_amd as P  # noqa: E402
from _timing import measure, parse_args, report  # noqa: E402

STEP_MS = 52.0


def seeded_state_dict(model, seed=7):
    """The recipe of tests/crepe_ref.state_dict: activations away from saturation, gamma negative on every third channel."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        u = lambda: torch.rand(v.shape, generator=g)
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.tensor(0, dtype=torch.int64)
        elif k.endswith('running_var'):
            sd[k] = 0.5 + u()
        elif k.endswith('running_mean'):
            sd[k] = 0.2 * u()
        elif k.endswith('_BN.weight'):
            sd[k] = 0.5 + u()
            sd[k][1::3] = -sd[k][1::3]
        elif k.endswith('_BN.bias'):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith('.weight'):
            sd[k] = (2 * u() - 1) * math.sqrt(3.0 / v[0].numel())
        else:
            sd[k] = (2 * u() - 1) / math.sqrt(sd[k[:-4] + 'weight'][0].numel())
    return sd


def tone(B, T, sr=16000, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)
    f = 175.0 + 75.0 * torch.sin(2 * math.pi * t[None] / sr * torch.rand(B, 1, generator=g, dtype=torch.float64) + 6.28 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    ph = 2 * math.pi * f.cumsum(-1) / sr
    x = sum(torch.sin(h * ph) / h for h in range(1, 5)) + 0.01 * torch.randn(B, T, generator=g, dtype=torch.float64)
    return (0.03 * x).float()


def torch_term(m, x, target):
    """The same term in stock torch ops (fp32, autograd): framing, normalisation, six blocks, head, MSE."""
    B, T = x.shape
    fr = F.pad(x, (512, 512)).unfold(1, 1024, 64)[:, :1 + T // 64]
    fr = fr - fr.mean(-1, keepdim=True)
    fr = fr / torch.clamp(fr.std(-1, keepdim=True), min=1e-10)
    h = fr.reshape(-1, 1, 1024, 1)
    for i in range(1, 7):
        conv, bn = getattr(m, f'conv{i}'), getattr(m, f'conv{i}_BN')
        h = F.pad(h, (0, 0, 254, 254) if i == 1 else (0, 0, 31, 32))
        h = F.relu(F.conv2d(h, conv.weight, conv.bias, stride=conv.stride))
        h = F.batch_norm(h, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        h = F.max_pool2d(h, (2, 1), (2, 1))
    act = torch.sigmoid(F.linear(h.permute(0, 2, 1, 3).reshape(h.shape[0], -1), m.classifier.weight, m.classifier.bias))
    act = act.reshape(B, -1, 360).transpose(1, 2)
    return F.mse_loss(act, target)


def main():
    a = parse_args('bench_crepe_bwd', iters=50, warmup=5, rounds=5, torch_iters=5, out=os.path.join(ROOT, 'profiles', 'crepe_bwd_bench.txt'))
    dev = torch.device('cuda:0')
    K = P.crepe
    m = K.Crepe('tiny')
    m.load_state_dict(seeded_state_dict(m))
    m = m.to(dev)
    for p_ in m.parameters():
        p_.requires_grad = False
    lines = []
    for name, B, T in (('tiny 16x16000', 16, 16000), ('tiny 1x71680', 1, 71680)):
        x = tone(B, T).to(dev)
        act, codes = m._forward_train(x, 64)
        target = K.roll_bins(act, torch.full((B,), 5, device=dev))
        Fn = act.shape[2]
        N = B * Fn
        fold, packed = m._fold(dev), m._pack(dev)
        # the inputs of every launch, kept from one forward / backward
        xin = [K.crepe_frames(x, 64).view(N, 1, 1024)]
        for i in range(1, 7):
            conv = getattr(m, f'conv{i}')
            xin.append(K.crepe_conv(xin[-1], conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0]))
        gl = torch.ones(1, device=dev)
        dys = [None] * 7
        dys[6] = K.crepe_head_bwd(act, m.classifier.weight, 64, 4, target=target, gL=gl)
        for i in range(6, 0, -1):
            conv = getattr(m, f'conv{i}')
            dys[i - 1] = K.crepe_conv_bwd(dys[i], codes[i - 1], fold[i - 1][0], packed[i - 1], conv.in_channels, xin[i - 1].shape[2], conv.kernel_size[0], conv.stride[0])
        variants = {}
        for i in range(1, 7):
            conv = getattr(m, f'conv{i}')
            yb, db = torch.empty_like(xin[i]), torch.empty_like(xin[i - 1])
            variants[f'conv{i}_fwd'] = (lambda i=i, conv=conv, yb=yb: K.crepe_conv(xin[i - 1], conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0], out=yb), a.iters)
            variants[f'conv{i}_train'] = (lambda i=i, conv=conv, yb=yb: K.crepe_conv(xin[i - 1], conv.weight, conv.bias, *fold[i - 1], stride=conv.stride[0], out=yb, train=True), a.iters)
            variants[f'conv{i}_bwd'] = (lambda i=i, conv=conv, db=db: K.crepe_conv_bwd(dys[i], codes[i - 1], fold[i - 1][0], packed[i - 1], conv.in_channels, xin[i - 1].shape[2],
                                                                                      conv.kernel_size[0], conv.stride[0], out=db), a.iters)
        variants['head_fwd'] = (lambda: K.crepe_head(xin[6], m.classifier.weight, m.classifier.bias, frames_per_row=Fn), a.iters)
        variants['head_bwd'] = (lambda: K.crepe_head_bwd(act, m.classifier.weight, 64, 4, target=target, gL=gl), a.iters)
        variants['frames_fwd'] = (lambda: K.crepe_frames(x, 64), a.iters)
        variants['frames_bwd'] = (lambda: K.crepe_frames_bwd(x, dys[0], 64), a.iters)
        variants['mse'] = (lambda: K.crepe_act_mse(act, target), a.iters)
        variants['forward'] = (lambda: m.activations(x), a.iters)
        xr = x[:, None].clone().requires_grad_()

        def term():
            xr.grad = None
            P.losses.f0_crepe_loss(xr, target, m).backward()
        variants['term'] = (term, a.iters)
        xt = x.clone().requires_grad_()
        torch_err = None

        def torch_fb():
            xt.grad = None
            torch_term(m, xt, target).backward()
        try:
            torch_fb()
            torch.cuda.synchronize()
            agree = float((xt.grad - xr.grad[:, 0]).abs().max() / xt.grad.abs().max()) if xr.grad is not None else None
            variants['torch_term'] = (torch_fb, a.torch_iters)
        except Exception as e:      # the stock route is a yardstick only: report why it did not run
            torch_err, agree = repr(e)[:200], None
        med, mm = measure(variants, a.warmup, a.rounds, once=('torch_term',))
        term()
        torch.cuda.synchronize()
        if 'torch_term' in med:
            agree = float((xt.grad - xr.grad[:, 0]).abs().max() / xt.grad.abs().max())
        # the stock fp32 route takes its own pooling decisions, so the two gradients are compared through a float64 run of the stock
        # ops (one call, on the smaller shape only): each gradient's distance from it, relative to its largest element
        vs64 = None
        if 'torch_term' in med and N <= 2000:
            try:
                m64 = K.Crepe('tiny')
                m64.load_state_dict(m.state_dict())
                m64 = m64.to(dev).double()
                x64 = x.double().requires_grad_()
                torch_term(m64, x64, target.double()).backward()
                top = float(x64.grad.abs().max())
                vs64 = {'hip': float((xr.grad[:, 0].double() - x64.grad).abs().max()) / top, 'torch_fp32': float((xt.grad.double() - x64.grad).abs().max()) / top}
            except Exception as e:
                vs64 = repr(e)[:200]
        out = {'shape': name, 'frames': N, **report(med, mm, 2),
               'bwd_over_fwd': {f'conv{i}': round(med[f'conv{i}_bwd'] / med[f'conv{i}_fwd'], 2) for i in range(1, 7)},
               'backward_launches_us': round(med['head_bwd'] + sum(med[f'conv{i}_bwd'] for i in range(1, 7)) + med['frames_bwd'], 2),
               'term_share_of_52ms_step': round(med['term'] / (STEP_MS * 1e3), 4)}
        if 'torch_term' in med:
            out.update({'torch_over_term': round(med['torch_term'] / med['term'], 2), 'torch_grad_rel_diff': agree, 'grad_rel_diff_to_float64': vs64})
        else:
            out['torch_term_error'] = torch_err
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
