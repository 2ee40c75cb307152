"""Times the pretraining validation's LinearSVC fit at the ModelNet40 probe's size on synthetic features.

    python tools/bench_linsvc.py host [--dims 384 1024]     svm_probe.evaluate_svm on the host: sklearn's LinearSVC()
    python tools/bench_linsvc.py hip  [--dims 384 1024]     linsvc_ops.fit_predict on the device, warm, median of --runs

Features: point_dae_amd.synthetic.class_features (class means + unit noise, column scales, a constant offset), 9 843 train
and 2 468 test rows, 40 classes.  One JSON line per width.  The hip mode also counts the C entry calls of one fit (every
one is a kernel launch or, for a split-K product, two) and reports the Newton steps and Hessian products.
The numbers are for synthetic features: features of a trained encoder may condition the problem differently.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('host', 'hip'))
    ap.add_argument('--dims', type=int, nargs='+', default=[384, 1024])
    ap.add_argument('--n', type=int, default=9843)
    ap.add_argument('--m', type=int, default=2468)
    ap.add_argument('--classes', type=int, default=40)
    ap.add_argument('--sep', type=float, default=0.3)
    ap.add_argument('--runs', type=int, default=5)
    args = ap.parse_args()
    from point_dae_amd.synthetic import class_features
    from point_dae_amd.svm_probe import evaluate_svm
    for D in args.dims:
        xtr, ytr, xte, yte = class_features(args.n, args.m, D, args.classes, sep=args.sep, seed=5)
        row = dict(mode=args.mode, n=args.n, m=args.m, D=D, K=args.classes, sep=args.sep)
        if args.mode == 'host':
            t0 = time.perf_counter()
            acc = evaluate_svm(xtr, ytr, xte, yte)
            row.update(seconds=time.perf_counter() - t0, acc=acc)
        else:
            import torch
            from point_dae_amd import _lib, linsvc_ops
            dtr, dte = torch.from_numpy(xtr).cuda(), torch.from_numpy(xte).cuda()
            calls = []
            _lib.CALL_HOOK = lambda name, a: calls.append(name)
            pred, _, status = linsvc_ops.fit_predict(dtr, ytr, dte)             # (also the warm-up)
            _lib.CALL_HOOK = None
            times = []
            for _ in range(args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pred, _, status = linsvc_ops.fit_predict(dtr, ytr, dte)         # ends in a device-to-host copy
                times.append(time.perf_counter() - t0)
            newton = int(status['newton_iters'].max())
            row.update(seconds=float(np.median(times)), seconds_min=min(times), seconds_max=max(times),
                       acc=float(np.mean(pred == yte)), newton_steps=newton, hv_products=int(status['hv_products']),
                       entry_calls=len(calls), gemm_calls=sum(c == 'pdae_rows_gemm' for c in calls),
                       calls_per_newton_step=len(calls) / max(newton, 1),
                       max_ratio_over_threshold=float((status['grad_ratio'] / status['threshold']).max()))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
