"""Traffic and time of the weight-grad slab folds of one training iteration (diagnostic tool).

Runs the bench configuration eagerly with tdvc_debug_fold_log on: every flush of deferred folds is one row with the bytes its
FoldDesc list moves (slabs read once, partials of split folds written and re-read, the gradient read and written) and the
time of its launches between two events. Prints the rows and the achieved GB/s of the whole pass.

  python tools/fold_traffic.py [--ref] [--batch 16] [--seconds 1.0] [--config conv_enc-stage1] [--passes 3]
Set TDVC_HIP_LIB to measure another build of the library that exports the log."""
import argparse, ctypes as C, importlib, os, sys, warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--config', default='conv_enc-stage1')
    ap.add_argument('--ref', action='store_true', help='run every fold on the one-load-per-slab reference kernel and its grid plan')
    ap.add_argument('--passes', type=int, default=3, help='logged iterations; the last one is printed row by row')
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module('td-vc-gan_amd')
    from common import build_models, to_dev
    lib = pkg._lib.lib()
    dev = torch.device('cuda:0'); torch.cuda.set_device(dev)
    hp = pkg.hparams.HParam(os.path.join(ROOT, 'config', f'{args.config}.yaml'))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cfg = pkg.train_step.StepConfig.from_hparams(hp.train)
    G, D = build_models(dev)
    ts = pkg.train_step.TrainStep(G, D, cfg, dev)
    B, T = args.batch, int(round(16000 * args.seconds))
    bt = to_dev(pkg.synth.make_batch(B, T, seed=1234, conversion=not cfg.no_conv), dev)
    ix = pkg.synth.contrastive_indices(B, T // 320, cfg.n_neg, 17).to(dev)
    iy = pkg.synth.contrastive_indices(B, T // 320, cfg.n_neg, 917).to(dev)
    for _ in range(2):
        ts.run(bt, ix, iy)
    torch.cuda.synchronize()
    totals = []
    rows = None
    for _ in range(args.passes):
        lib.tdvc_debug_fold_log(2 if args.ref else 1)
        ts.run(bt, ix, iy)
        torch.cuda.synchronize()
        lib.tdvc_debug_fold_log(0)
        n = lib.tdvc_debug_fold_log_read(None, 0)
        buf = (C.c_double * (5 * n))()
        lib.tdvc_debug_fold_log_read(buf, n)
        rows = [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]
        totals.append((sum(r[3] for r in rows), sum(r[4] for r in rows)))
    print(f'{args.config} B={B} T={T} kernel={"reference" if args.ref else "production"}: {len(rows)} flushes per iteration')
    print('flush folds launches blocks        MB       us     GB/s')
    for i, (folds, launches, blocks, nbytes, us) in enumerate(rows):
        print(f'{i:5d} {int(folds):5d} {int(launches):8d} {int(blocks):6d} {nbytes / 1e6:9.2f} {us:8.1f} {nbytes / us / 1e3 if us else 0:8.0f}')
    for nbytes, us in totals:
        print(f'pass total: {nbytes / 1e6:9.2f} MB in {us:8.1f} us = {nbytes / us / 1e3:6.0f} GB/s')


if __name__ == '__main__':
    main()
