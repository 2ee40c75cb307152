"""Times the linear-SVM evaluation protocol (--svm_classification) at ModelNet40's shape and prints ONE JSON line.

Features are synthetic and ModelNet40-shaped: 9 840 x 1024 train, 2 468 test, 40 Gaussian classes (unit variance around
random means of scale --scale) with ModelNet40's training class sizes.  Each step is a child process under its own time
limit; the first one that fails ends the run (nothing more is started on the GPU after a fault or a time-out).

  extract   DGCNN_feat eval forward incl. the protocol's FPS + gather, B = 32, N = 1024 of 8192-point clouds: ms per batch
            and per cloud, HIP events around --steps batches after --warmup
  hip       on the device features: the two Gram GEMMs, the solver launch for the six Cs (with the maximum and median
            iterations per pair), the predict launch -- HIP events around each -- and svm_ops.fit_predict_ovo as a whole
            (host clock around a synchronised call, uploads of the layout and the status read-back included)
  sklearn   PDAE_SVM=sklearn's path on the same features: six SVC(C=c, kernel='linear') fits and scores on the host
            (libsvm is single-threaded; the box's thread settings are reported beside the time)

    python tools/bench_svm.py [--steps-list extract,hip,sklearn] [--scale 0.1] [--limit 900]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ModelNet40's training split by class (9 843 clouds); the train loader's drop_last leaves 9 840 rows of features
MODELNET40_TRAIN = (626, 106, 515, 173, 572, 335, 64, 197, 889, 167, 79, 138, 200, 109, 200, 149, 171, 155, 145, 124, 149,
                    284, 465, 200, 88, 231, 240, 104, 115, 128, 680, 124, 90, 392, 163, 344, 267, 475, 87, 103)
N_TRAIN, N_TEST, DIM = 9840, 2468, 1024


def features(scale, seed=0):
    """-> Xtr (9840, 1024) fp32, ytr, Xte (2468, 1024), yte: shuffled Gaussian classes with ModelNet40's class sizes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sizes = np.array(MODELNET40_TRAIN)
    K = len(sizes)
    means = rng.standard_normal((K, DIM)) * scale
    ytr = rng.permutation(np.repeat(np.arange(K), sizes))[:N_TRAIN]
    yte = rng.choice(K, N_TEST, p=sizes / sizes.sum())
    Xtr = (means[ytr] + rng.standard_normal((N_TRAIN, DIM))).astype(np.float32)
    Xte = (means[yte] + rng.standard_normal((N_TEST, DIM))).astype(np.float32)
    return Xtr, ytr, Xte, yte


def _events_ms(fn, n=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def step_extract(a):
    import torch
    from point_dae_amd import builder
    from point_dae_amd.config import cfg_from_yaml_file
    from point_dae_amd.graph_step import use_created_stream
    from point_dae_amd.runner_finetune import resample
    from point_dae_amd.synthetic import labelled_clouds
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    use_created_stream(dev)
    config = cfg_from_yaml_file(os.path.join(ROOT, 'cfgs', 'finetune_modelnet_svm_dgcnn.yaml'))
    torch.manual_seed(0)
    model = builder.model_builder(config.model).to(dev).eval()
    B, N = 32, config.npoints
    x, _ = labelled_clouds(B, 8192, seed=0, classes=3)
    pts = torch.from_numpy(x).to(dev)

    def batch():
        with torch.no_grad():
            return model(resample(pts, N, point_all=N))
    for _ in range(a.warmup):
        batch()
    ms = _events_ms(batch, a.steps)
    return dict(batch=B, npoints=N, stored_points=8192, ms_per_batch=round(ms, 3), ms_per_cloud=round(ms / B, 4),
                protocol_clouds=N_TRAIN + N_TEST, protocol_extract_s=round(ms / B * (N_TRAIN + N_TEST) / 1e3, 2))


def step_hip(a):
    import ctypes
    import numpy as np
    import torch
    from point_dae_amd import _lib, svm_ops
    from point_dae_amd.graph_step import use_created_stream
    from point_dae_amd.rows import rows_gemm
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    use_created_stream(dev)
    Xtr, ytr, Xte, yte = features(a.scale)
    X, Xt = torch.from_numpy(Xtr).to(dev), torch.from_numpy(Xte).to(dev)
    Cs = svm_ops.SVM_CS
    classes, order, class_ptr = svm_ops.class_layout(ytr)
    n, m, K, nC = N_TRAIN, N_TEST, len(classes), len(Cs)
    P = K * (K - 1) // 2
    out = dict(n=n, m=m, dim=DIM, classes=K, pairs=P, Cs=list(Cs), largest_pair=int(np.sort(np.diff(class_ptr))[-2:].sum()))
    rows_gemm(X[:256], X[:256])                                    # warm-up: code objects, the GEMM plan
    torch.cuda.synchronize()
    hold = {}
    out['gram_train_ms'] = round(_events_ms(lambda: hold.update(G=rows_gemm(X, X))), 3)
    out['gram_test_ms'] = round(_events_ms(lambda: hold.update(Gte=rows_gemm(Xt, X))), 3)
    out['gram_tflops'] = round(2.0 * (n + m) * n * DIM / ((out['gram_train_ms'] + out['gram_test_ms']) * 1e-3) / 1e12, 1)
    G, Gte = hold['G'], hold['Gte']
    cptr = (ctypes.c_int * (K + 1))(*class_ptr.tolist())
    cs = (ctypes.c_double * nC)(*[float(c) for c in Cs])
    order_d = torch.from_numpy(order).to(dev)
    coef = torch.empty((nC, K - 1, n), device=dev, dtype=torch.float64)
    rho, gap = (torch.empty((nC, P), device=dev, dtype=torch.float64) for _ in range(2))
    st = torch.empty((nC, P, 2), device=dev, dtype=torch.int32)
    dec = torch.empty((nC, m, P), device=dev, dtype=torch.float64)
    pred = torch.empty((nC, m), device=dev, dtype=torch.int32)

    def train():
        _lib.call('pdae_svm_ovo_train', X, n, G.shape[1], K, nC, _lib.ptr(G), _lib.ptr(order_d), cptr, cs, 1e-3,
                  svm_ops.MAX_ITER, _lib.ptr(coef), _lib.ptr(rho), _lib.ptr(st), _lib.ptr(gap))

    def predict():
        _lib.call('pdae_svm_ovo_predict', X, m, n, Gte.shape[1], K, nC, _lib.ptr(Gte), _lib.ptr(order_d), cptr,
                  _lib.ptr(coef), _lib.ptr(rho), _lib.ptr(dec), _lib.ptr(pred))
    out['solver_ms'] = [round(_events_ms(train), 2) for _ in range(a.reps)]
    it = st[..., 0].cpu().numpy()
    out['iterations'] = {str(c): dict(max=int(it[i].max()), median=float(np.median(it[i]))) for i, c in enumerate(Cs)}
    out['iterations_total'] = int(it.sum())
    out['capped'] = int(st[..., 1].sum().item())
    out['predict_ms'] = [round(_events_ms(predict), 2) for _ in range(a.reps)]
    del G, Gte, hold
    whole = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels, _, _ = svm_ops.fit_predict_ovo(X, ytr, Xt, Cs)
        torch.cuda.synchronize()
        whole.append(round(time.perf_counter() - t0, 3))
    out['fit_predict_s'] = whole
    out['accuracy'] = [round(float(np.mean(labels[i] == yte)), 4) for i in range(nC)]
    out['device'] = torch.cuda.get_device_name(dev)
    return out


def step_sklearn(a):
    from point_dae_amd import svm_ops
    from point_dae_amd.svm_probe import svc_accuracies
    Xtr, ytr, Xte, yte = features(a.scale)
    t0 = time.perf_counter()
    accs = svc_accuracies(Xtr, ytr, Xte, yte, svm_ops.SVM_CS)
    return dict(six_fits_and_scores_s=round(time.perf_counter() - t0, 2), accuracy=[round(v, 4) for v in accs],
                cpus_given=os.environ.get('OMP_NUM_THREADS'), note='libsvm fits on one core')


STEPS = {'extract': step_extract, 'hip': step_hip, 'sklearn': step_sklearn}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--steps-list', default='extract,hip,sklearn')
    p.add_argument('--only', choices=sorted(STEPS), default=None, help='(child) run this one step in this process')
    p.add_argument('--scale', type=float, default=0.1, help='scale of the class means (unit-variance classes)')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--reps', type=int, default=2)
    p.add_argument('--limit', type=int, default=900, help='seconds each step may take')
    a = p.parse_args(argv)
    if a.only:
        print('BENCH_SVM_STEP ' + json.dumps(STEPS[a.only](a)))
        return 0
    out = dict(workload='svm_classification', scale=a.scale)
    for name in a.steps_list.split(','):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--only', name, '--scale',
               str(a.scale), '--steps', str(a.steps), '--warmup', str(a.warmup), '--reps', str(a.reps)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('BENCH_SVM_STEP ')]
        if r.returncode != 0 or not lines:
            out[name] = dict(failed=True, returncode=r.returncode, stderr=r.stderr[-800:])
            print(json.dumps(out))
            return 1                                     # nothing more is started after a failed step
        out[name] = json.loads(lines[-1][len('BENCH_SVM_STEP '):])
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
