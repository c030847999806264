"""What the float64 edge suites share beside the cases themselves: the bars, the sentinel, the guarded buffers, the library
lookups, the LDS poison and the worst-error bookkeeping. conv_edge.py holds the Edge class that most of them drive."""
import importlib

import torch

TOL = 2e-5
SENT = -7777.25      # sentinel of test_misc_ops_gpu.py: every output buffer starts filled with it
U = 2.0 ** -23
SLOPE = 0.2
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4      # TDVC_EINVAL, TDVC_EWORKSPACE, TDVC_EUNSUPPORTED of include/tdvc.h


def mods():
    pkg = importlib.import_module('td-vc-gan_amd')
    return pkg.ops, pkg._lib, pkg.arena


def lib():
    return mods()[1].lib()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def poison_lds(dev):
    """NaN bit patterns into the LDS of every CU: a kernel that reads words it never staged turns them into NaN."""
    L = mods()[1]
    L.check(L.lib().tdvc_debug_poison_lds(0xFFFFFFFF, stream(dev)))


def forced_tile(cfg, fn):
    """fn() with the lean kernel pinned to tile `cfg` (tdvc_debug_force_tile; -1 leaves the choice to the launcher)."""
    lib().tdvc_debug_force_tile(cfg)
    try:
        return fn()
    finally:
        lib().tdvc_debug_force_tile(-1)


def _buf(B, Cc, T, dev, views, src=None, unaligned=False, fill=SENT):
    """(whole buffer, operand view): SENT-filled; with `views` the operand is the channel slice [:, :Cc] of a [B, Cc + 3, T] buffer
    (a batch stride wider than contiguous and, for odd T, planes that are not 16-byte aligned); with `unaligned` it lives one
    float into a flat buffer (contiguous rows, nothing 16-byte aligned; the float in front stays SENT). `fill`: what the buffer
    holds outside the operand (NaN behind the inputs of a `nan_spare` case)."""
    if unaligned:
        assert not views, 'an unaligned operand lives in a flat buffer: it cannot be a channel slice as well'
        whole = torch.full((B * Cc * T + 1,), fill, dtype=torch.float32, device=dev)
        v = whole[1:].view(B, Cc, T)
    else:
        whole = torch.full((B, Cc + (3 if views else 0), T), fill, dtype=torch.float32, device=dev)
        v = whole[:, :Cc]
    if src is not None:
        v.copy_(src.to(dev))
    return whole, v


def _spare_intact(whole, Cc):
    if whole.dim() == 1:
        return bool(whole[0] == SENT)
    return whole.shape[1] == Cc or bool((whole[:, Cc:] == SENT).all())


def elem_check(got, ref, A, n, slack=8):
    """-> (worst err / bound over the elements with A > 0, number of elements with A == 0 that differ from fp32(ref)).
    `slack`: the roundings outside the summation the bound allows for (8; 12 with a FiLM prologue, Edge's docstring)."""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bound = (n + slack) * U * A + 2.0 ** -22 * ref.abs()
    zero = A == 0
    inexact = int((got[zero] != ref[zero].float()).sum())
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    if not bool(torch.isfinite(got).all()):
        ratio = float('nan')
    return ratio, inexact


def assert_bars(res, what):
    print(f'[edge] {what}: ' + '  '.join(f'{k}: rel {v["rel"]:.2e} err/bound {v["ratio"]:.3f}' for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not (v['rel'] < TOL and v['ratio'] <= 1.0 and v['inexact'] == 0)}
    assert not bad, (what, bad)


def pack_sign_bits(cv0):
    """[B][nc][T] -> int32 words [B][nc][T / 32], bit t % 32 of word t / 32 set where cv0 > 0 (test_sign_bit_masks' expression)."""
    B, nc, T = cv0.shape
    w = ((cv0 > 0).reshape(B, nc, T // 32, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


class Worst:
    """kernel -> tensor -> (worst err / bound, case) over the cases a suite ran in this session."""

    def __init__(self):
        self.table = {}

    def note(self, kernel, res, case):
        for k, v in res.items():
            if v['ratio'] >= self.table.setdefault(kernel, {}).get(k, (-1.0, ''))[0]:
                self.table[kernel][k] = (v['ratio'], case)

    def report(self):
        for kernel, per in sorted(self.table.items()):
            print(f'[edge] worst {kernel}: ' + '  '.join(f'{k} {r:.3f} ({n})' for k, (r, n) in sorted(per.items())))

    def ratios(self):
        return [r for per in self.table.values() for r, _ in per.values()]
