"""GPU: run-to-run reproducibility of the gradient reductions, and the FiLM conditioning backward's optional workspace.

The train step sums its gradient partials in a fixed order (conv bias gradient per channel over the batch, slab folds in
slab order and y order, dk3 through per-block slots), so two runs from the same state give the same parameter bits. The
loss scalars are still summed across blocks with atomics and are compared with a tolerance only.
"""
import ctypes as C
import importlib

import pytest
import torch

from common import build_models, rel_l2, to_dev

pytestmark = pytest.mark.gpu


def _lib():
    return importlib.import_module('td-vc-gan_amd')._lib


def _cond_bwd_inputs(dev, B=2, T=1024, nc=136, nv=8, C2=32):
    g = torch.Generator(device='cpu').manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    return dict(B=B, T=T, nc=nc, nv=nv, C2=C2, dgb=r(B, C2, T), wt2=r(nc, C2, 3) / (nc * 3) ** 0.5, cv0=r(B, nc, T),
                exc=r(B, nv, T), w0=r(nc, nc, 3) / (nc * 3) ** 0.5, dcv=r(B, nc, T))


def _run_cond_bwd(which, x, ws):
    """dk3 and dexc of tdvc_film_cond_bwd (fused) or tdvc_film_cond0_bwd with no weight gradient (dw0 = NULL)."""
    L = _lib()
    B, T, nc, nv, C2 = x['B'], x['T'], x['nc'], x['nv'], x['C2']
    dexc = torch.full_like(x['exc'], float('nan'))
    dk3 = torch.full((B, nc, 3), float('nan'), device=x['exc'].device)
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    st = torch.cuda.current_stream().cuda_stream
    if which == 'fused':
        a = L.FilmCondBwdArgs(B, T, nc, nv, C2, x['dgb'].data_ptr(), x['dgb'].stride(0), x['wt2'].data_ptr(), None, 0,
                              x['cv0'].data_ptr(), x['cv0'].stride(0), x['exc'].data_ptr(), x['exc'].stride(0), x['w0'].data_ptr(),
                              dexc.data_ptr(), dexc.stride(0), dk3.data_ptr(), None, wsp, wsn, 0.2)
        L.check(L.lib().tdvc_film_cond_bwd(C.byref(a), st))
    else:
        a = L.FilmCond0BwdArgs(B, T, nc, nv, x['dcv'].data_ptr(), x['dcv'].stride(0), x['exc'].data_ptr(), x['exc'].stride(0),
                               x['w0'].data_ptr(), dexc.data_ptr(), dexc.stride(0), dk3.data_ptr(), None, wsp, wsn)
        L.check(L.lib().tdvc_film_cond0_bwd(C.byref(a), st))
    torch.cuda.synchronize()
    return dk3, dexc


@pytest.mark.parametrize('which', ['fused', 'cond0'])
def test_film_cond_bwd_workspace_optional_without_dw0(which, dev):
    """Without dw0 the workspace is optional (include/tdvc.h): absent, dk3 is accumulated with atomics; given, dk3 goes
    through the fixed-order fold and repeats bit for bit. Both agree to fp32 rounding."""
    x = _cond_bwd_inputs(dev)
    q = _lib().lib().tdvc_film_cond_bwd_workspace if which == 'fused' else _lib().lib().tdvc_film_cond0_bwd_workspace
    ws = torch.empty(q(x['B'], x['T'], x['nc'], x['nv']), dtype=torch.uint8, device=dev)
    dk3_a, dexc_a = _run_cond_bwd(which, x, None)
    dk3_w1, dexc_w1 = _run_cond_bwd(which, x, ws)
    dk3_w2, _ = _run_cond_bwd(which, x, ws)
    assert torch.isfinite(dk3_a).all() and torch.isfinite(dk3_w1).all()
    assert torch.equal(dk3_w1, dk3_w2)
    assert torch.equal(dexc_a, dexc_w1)
    assert rel_l2(dk3_a, dk3_w1) < 1e-6


def test_train_step_parameters_reproducible(pkg, dev):
    """Two runs of the captured D+G step (bench.py's timed path) from the same seeded models and batch end with the same
    parameter bits; their losses agree to rounding."""
    B, T = 2, 8960
    cfg = pkg.train_step.StepConfig()
    bt = to_dev(pkg.synth.make_batch(B, T, seed=11), dev)
    ix = pkg.synth.contrastive_indices(B, T // 320, cfg.n_neg, 1).to(dev)
    iy = pkg.synth.contrastive_indices(B, T // 320, cfg.n_neg, 2).to(dev)
    runs = []
    for _ in range(2):
        G, D = build_models(dev)
        ts = pkg.train_step.TrainStep(G, D, cfg, dev)
        step = ts.capture(bt, ix, iy, warmup=2)
        for _ in range(3):
            log = step()
        torch.cuda.synchronize()
        runs.append((G.arena.P.clone(), D.arena.P.clone(), {k: float(v) for k, v in log.items()}))
        del step, ts, G, D
    (g1, d1, l1), (g2, d2, l2) = runs
    assert torch.equal(g1, g2), f'G parameters differ: max |diff| {float((g1 - g2).abs().max()):.3g}'
    assert torch.equal(d1, d2), f'D parameters differ: max |diff| {float((d1 - d2).abs().max()):.3g}'
    for k, v in l1.items():
        assert abs(v - l2[k]) <= 1e-6 * (abs(v) + 1e-6), (k, v, l2[k])
