"""The pretraining validation's classifier on the gfx950 kernels of csrc/linsvc.hip.

The reference (tools/runner_pretrain.py:25-48) fits sklearn.svm.LinearSVC() -- liblinear's one-vs-rest machines with the
squared hinge loss and a regularised intercept -- on one feature per labelled training cloud and scores it on the test
clouds.  With a_i = [x_i, 1] and y_ik = +1 where label_i == classes[k], else -1, class k's machine minimises

    f_k(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_ik a_i.w)^2,        w = [coef_k, intercept_k]

which is strongly convex: one optimum, whichever solver.  Here every class is solved at once by a truncated Newton method
in the primal:

    pred, W, status = fit_predict(train_feats, train_labels, test_feats)

A Newton step takes the gradient G = W - 2 C A^T (Y o R o act) (R = 1 - Y o A W, act = R > 0), solves H s = -g per column
by conjugate gradients (H = I + 2 C A^T diag(act) A, until |r| <= 0.01 |g|), and moves by the first step of 1, 1/2, 1/4, ...
that passes Armijo's test.  The four products A W, A P, A S and A^T V are row GEMMs (rows.rows_gemm: the operands are
zero-padded to multiples of 32, which the exact-split bf16 kernels need, and the intercept's column of ones sits in that
padding); everything between them is csrc/linsvc.hip, one launch for all classes.  A class is finished by liblinear's rule,
|g_k(w)| <= tol min(pos_k, neg_k) / n |g_k(0)|, and then stops moving while the others go on.  The host reads one small
block of flags per Newton step and per round of CG_ROUND conjugate-gradient steps, never per step.

What differs from liblinear: the step (liblinear's primal solver is a trust-region / preconditioned Newton method; this is
a line-search Newton method with plain conjugate gradients; both stop by the same rule at the same optimum), and the
products are fp32 while liblinear's are fp64, so the optimum is met to fp32 rounding: below roughly 1e-6 |g(0)| a line
search no longer finds a decrease and the class is reported as stalled.

Two classes: sklearn fits ONE machine, for classes[1], and predicts it where the decision is positive; so does this
(W has one column, the status arrays one entry).

PDAE_LINSVC=sklearn (the default) is the reference's own LinearSVC call on the host (svm_probe.evaluate_svm),
PDAE_LINSVC=hip these kernels; accuracy() dispatches.
"""
import os

import numpy as np
import torch

from . import _lib
from .rows import pad2d, rows_gemm, rows_gemm_few_rows

MAX_NEWTON = 100
CG_ROUND = 8                       # conjugate-gradient steps between two reads of the flags
CG_XI = 0.01                       # conjugate gradients end at |r| <= CG_XI |g| (0.1 took three times the Newton steps)
ARMIJO_ETA = 1e-2                  # liblinear's line-search constant
ROW_BLOCK = 64                     # csrc/linsvc.hip LS_ROWS
SC, FL = _lib.CONST['PDAE_LINSVC_SC'], _lib.CONST['PDAE_LINSVC_FL']
SC_F, SC_GNORM, SC_GNORM0, SC_EPS, SC_RR, SC_GS, SC_T, SC_T0 = range(8)
FL_DONE, FL_NEWTON, FL_CG_ACTIVE, FL_CAPPED, FL_STALLED, FL_HV, FL_CG_ITERS, FL_LS_FAILS = range(8)


def backend():
    """'hip' or 'sklearn', from PDAE_LINSVC.  The default is sklearn: tests/test_gpu_probe.py pins validate()'s accuracy
    to the reference's host fit to 1e-12, and two solvers stopped at tol = 1e-4 may differ on a test row whose two best
    decision values are closer than that."""
    name = os.environ.get('PDAE_LINSVC', 'sklearn')
    if name not in ('hip', 'sklearn'):
        raise ValueError('PDAE_LINSVC=%r: hip or sklearn' % name)
    return name


def label_layout(labels):
    """labels (n,) -> (classes, index): the distinct labels ascending (np.unique, as sklearn's classes_) and every
    sample's class index (int32)."""
    classes, inverse = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    return classes, inverse.reshape(-1).astype(np.int32)


def columns(K):
    """(ncol, col0): the machines solved for K classes are those of the classes col0 .. col0 + ncol - 1 -- all of them,
    or the second class alone when there are two (sklearn's binary case)."""
    return (1, 1) if K == 2 else (K, 0)


def targets(index, K):
    """index (n,) -> Y (n, ncol) of +-1: column k is +1 on the samples of class col0 + k (the kernels' layout)."""
    ncol, col0 = columns(K)
    return np.where(np.asarray(index).reshape(-1, 1) == np.arange(col0, col0 + ncol)[None, :], 1.0, -1.0)


def stopping_eps(index, K, tol=1e-4):
    """liblinear's primal stopping factor per machine (ncol,): tol * max(min(pos, neg), 1) / n; a machine is finished
    when |g(w)| <= that * |g(0)|."""
    Y = targets(index, K)
    pos = (Y > 0).sum(0)
    return tol * np.maximum(np.minimum(pos, Y.shape[0] - pos), 1) / Y.shape[0]


def _require_feats(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('linsvc_ops: %s must be a tensor on the GPU (PDAE_LINSVC=sklearn is the host path)' % name)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError('linsvc_ops: %s must be a 2-D fp32 tensor' % name)
    return t.detach().contiguous()


def _with_ones(x, D):
    """x (r, D) -> (r32, Dp) with zero rows / columns up to multiples of 32 and ones in column D of the r real rows."""
    r = x.shape[0]
    a = pad2d(x, (-r) % 32, (-(D + 1)) % 32 + 1)
    _lib.call('pdae_linsvc_ones', a, r, a.shape[1], D, _lib.ptr(a))
    return a


def fit_predict(train_feats, train_labels, test_feats, C=1.0, tol=1e-4, max_newton=MAX_NEWTON, check=True):
    """LinearSVC(C=C, tol=tol).fit(train).predict(test) on the kernels.

    train_feats (n, D), test_feats (m, D): fp32 on the device; train_labels (n,): host array or tensor.
    -> pred (m,) numpy, the predicted labels; W (D + 1, K) fp32 on the device, [coef_k, intercept_k] per column (one column,
    the machine of classes[1], when K == 2); status: dict of classes (K,), newton_iters, grad_ratio = |g| / |g(0)|,
    threshold (the stopping factor), capped, stalled, f (one entry per column each) and hv_products (the batched Hessian
    products issued).
    Raises, naming the class, when a class took max_newton steps without meeting its threshold, or stalled above it at the
    products' rounding floor; check=False returns such a fit as it is, flagged in the status."""
    X, Xt = _require_feats(train_feats, 'train_feats'), _require_feats(test_feats, 'test_feats')
    if X.shape[1] != Xt.shape[1]:
        raise ValueError('linsvc_ops: train and test features differ in width')
    if isinstance(train_labels, torch.Tensor):
        train_labels = train_labels.detach().cpu().numpy()
    classes, index = label_layout(train_labels)
    (n, D), m, K = X.shape, Xt.shape[0], len(classes)
    if index.shape[0] != n:
        raise ValueError('linsvc_ops: %d labels for %d feature rows' % (index.shape[0], n))
    if not C > 0 or not tol > 0 or max_newton < 1:
        raise ValueError('linsvc_ops: C > 0, tol > 0 and max_newton >= 1 required')
    # a layout the kernels refuse (one class, more than PDAE_LINSVC_MAX_CLASSES = 64, empty input) raises here, before anything is launched
    handle = _lib.lib()
    _lib._check(handle, 'pdae_linsvc_supported', handle.pdae_linsvc_supported(n, m, D, K))
    ncol, col0 = columns(K)
    ld, D1, dev = ncol + (-ncol) % 4, D + 1, X.device
    A = _with_ones(X, D)                                 # (rows, Dp)
    At = A.t().contiguous()                              # (Dp, rows): the left operand of A^T V
    rows, Dp = A.shape
    nb, nb_ls = -(-rows // ROW_BLOCK), -(-n // ROW_BLOCK)
    eps = stopping_eps(index, K, tol)
    sc_h = np.zeros((ncol, SC))
    sc_h[:, SC_EPS], sc_h[:, SC_T0] = eps, 1.0
    sc = torch.from_numpy(sc_h).to(dev)
    fl = torch.zeros((ncol, FL), device=dev, dtype=torch.int32)
    labels = torch.from_numpy(index).to(dev)
    W, G, S, R, P = (torch.zeros((Dp, ld), device=dev) for _ in range(5))
    V = torch.empty((rows, ld), device=dev)
    part = torch.empty((nb, ld), device=dev, dtype=torch.float64)
    part_ls = torch.empty((nb_ls, ld, 8), device=dev, dtype=torch.float64)
    cg_max = max(D1, 5)                                  # liblinear's cap on the conjugate-gradient steps of a Newton step
    ptr = _lib.ptr
    hv = 0
    for _newton in range(max_newton + 1):
        Z = rows_gemm(A, W, True)                        # (rows, ld) margins
        _lib.call('pdae_linsvc_residual', X, 0, n, rows, ld, ncol, col0, ptr(Z), None, ptr(labels), ptr(fl), ptr(V), ptr(part))
        T = rows_gemm_few_rows(At, V, True, None, 0)     # (Dp, ld)
        _lib.call('pdae_linsvc_newton_begin', X, D1, ld, ncol, nb, float(C), int(max_newton), ptr(W), ptr(T), ptr(part),
                  ptr(G), ptr(S), ptr(R), ptr(P), ptr(sc), ptr(fl))
        fl_h = fl.cpu().numpy()
        if fl_h[:, FL_DONE].all():
            break
        while fl_h[:, FL_CG_ACTIVE].any():
            for _ in range(CG_ROUND):
                AP = rows_gemm(A, P, True)
                _lib.call('pdae_linsvc_residual', X, 1, n, rows, ld, ncol, col0, ptr(Z), ptr(AP), ptr(labels), ptr(fl), ptr(V),
                          None)
                T = rows_gemm_few_rows(At, V, True, None, 0)
                _lib.call('pdae_linsvc_cg_update', X, D1, ld, ncol, float(C), CG_XI, cg_max, ptr(T), ptr(S), ptr(R), ptr(P),
                          ptr(sc), ptr(fl))
            hv += CG_ROUND
            fl_h = fl.cpu().numpy()
        AS = rows_gemm(A, S, True)
        _lib.call('pdae_linsvc_linesearch', X, n, ld, ncol, col0, ptr(Z), ptr(AS), ptr(labels), ptr(sc), ptr(fl), ptr(part_ls))
        _lib.call('pdae_linsvc_step', X, D1, ld, ncol, nb_ls, float(C), ARMIJO_ETA, ptr(W), ptr(S), ptr(G), ptr(part_ls),
                  ptr(sc), ptr(fl))
    assert fl_h[:, FL_DONE].all()                        # (the max_newton + 1-th newton_begin caps whatever is left)
    Zt = rows_gemm(_with_ones(Xt, D), W, True)
    pred = torch.empty((m,), device=dev, dtype=torch.int32)
    _lib.call('pdae_linsvc_predict', X, m, ld, ncol, ptr(Zt), ptr(pred))
    sc_h = sc.cpu().numpy()
    g0 = sc_h[:, SC_GNORM0]
    status = dict(classes=classes, newton_iters=fl_h[:, FL_NEWTON].copy(), hv_products=hv,
                  grad_ratio=np.where(g0 > 0, sc_h[:, SC_GNORM] / np.where(g0 > 0, g0, 1.0), 0.0), threshold=eps,
                  capped=fl_h[:, FL_CAPPED] != 0, stalled=fl_h[:, FL_STALLED] != 0, f=sc_h[:, SC_F].copy())
    if check:
        for key, what in (('capped', 'took max_newton = %d Newton steps' % max_newton),
                          ('stalled', 'stalled at the rounding floor of the fp32 products')):
            if status[key].any():
                k = int(np.argmax(status[key]))
                raise RuntimeError('linsvc_ops: the machine of class %s %s with |g| / |g(0)| = %.3g above its threshold '
                                   '%.3g (tol %g); %d of %d machines did' % (classes[col0 + k], what, status['grad_ratio'][k],
                                                                              eps[k], tol, int(status[key].sum()), ncol))
    return classes[pred.cpu().numpy()], W[:D1, :ncol].clone(), status


def accuracy(train_feats, train_labels, test_feats, test_labels):
    """The fraction of test rows LinearSVC() fitted on the train rows predicts correctly: on the kernels (PDAE_LINSVC=hip)
    or by the reference's own call on the host (PDAE_LINSVC=sklearn, svm_probe.evaluate_svm)."""
    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    test_labels = host(test_labels).reshape(-1)
    if backend() == 'sklearn':
        from .svm_probe import evaluate_svm
        return evaluate_svm(host(train_feats), host(train_labels).reshape(-1), host(test_feats), test_labels)
    pred, _, _ = fit_predict(train_feats, train_labels, test_feats)
    return float(np.sum(test_labels == pred)) / pred.shape[0]
