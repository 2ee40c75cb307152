"""The linear-SVM evaluation protocol's classifier on the gfx950 kernels of csrc/svm.hip.

The reference (tools/runner_finetune.py:1038-1049) fits sklearn.svm.SVC(C=c, kernel='linear') -- libsvm's one-vs-one
C-SVC -- for c = 10**i, i in range(-3, 3), on one feature per training cloud and scores it on the test clouds.  Here the
two Gram matrices X X^T and X_te X^T come from the row GEMM (rows.rows_gemm), pdae_svm_ovo_train solves every (class pair,
C) in one launch and pdae_svm_ovo_predict computes the decision values and libsvm's votes:

    pred, dec, status = fit_predict_ovo(train_feats, train_labels, test_feats, Cs)

PDAE_SVM=hip (default) selects these kernels, PDAE_SVM=sklearn the reference's own SVC call on the host
(svm_probe.svc_accuracies); accuracies() dispatches.  What differs from libsvm: the working pair is the maximal violating
pair (first order; libsvm's second-order rule picks j by the gain), there is no shrinking, the Gram matrix is fp32
(libsvm computes fp64 dot products), and a class pair may have at most MAX_PAIR = 2048 members.  Both stop at the same
violation eps, so the decision values agree to what eps leaves open, not bit for bit.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .rows import pad2d, rows_gemm

MAX_PAIR = _lib.CONST['PDAE_SVM_MAX_PAIR']
MAX_ITER = 1000000
SVM_CS = tuple(10 ** i for i in range(-3, 3))         # runner_finetune.py:1039-1040


def backend():
    """'hip' or 'sklearn', from PDAE_SVM."""
    name = os.environ.get('PDAE_SVM', 'hip')
    if name not in ('hip', 'sklearn'):
        raise ValueError('PDAE_SVM=%r: hip or sklearn' % name)
    return name


def class_layout(labels):
    """labels (n,) -> (classes, order, class_ptr): the distinct labels ascending (np.unique, as sklearn's classes_), the
    samples in class order (a stable sort: libsvm groups the classes and keeps each one's samples in input order) and the
    classes' ranges class_ptr[k] .. class_ptr[k + 1] in that order."""
    labels = np.asarray(labels).reshape(-1)
    classes, inverse = np.unique(labels, return_inverse=True)
    order = np.argsort(inverse, kind='stable').astype(np.int32)
    class_ptr = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(classes)))]).astype(np.int32)
    return classes, order, class_ptr


def pairs(K):
    """The one-vs-one problems in libsvm's (and decision_function_shape='ovo') column order: (0,1), (0,2), ..., (K-2,K-1)."""
    return [(p, q) for p in range(K) for q in range(p + 1, K)]


def coef_row(p, q):
    """The row of dual_coef_ (K - 1 rows) in which the samples of class p hold their coefficient against class q."""
    return q - 1 if q > p else q


def vote(dec, K):
    """libsvm's vote on decision values dec (..., P) -> class indices (...): dec > 0 votes for the pair's first class, else
    for its second; the first class with the most votes (the host twin of pdae_svm_ovo_predict's, for tests)."""
    dec = np.asarray(dec)
    votes = np.zeros(dec.shape[:-1] + (K,), np.int64)
    for k, (p, q) in enumerate(pairs(K)):
        first = dec[..., k] > 0
        votes[..., p] += first
        votes[..., q] += ~first
    return votes.argmax(-1)


def _padded(x):
    """x (r, D) fp32 on the device -> (r4, D4) with zero rows / columns up to multiples of 4 (the row GEMM reduces and
    writes in multiples of 4; zeros change no dot product)."""
    r, d = x.shape
    pr, pc = (-r) % 4, (-d) % 4
    x = x.contiguous()
    return pad2d(x, pr, pc) if pr or pc else x


def _require_feats(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('svm_ops: %s must be a tensor on the GPU (PDAE_SVM=sklearn is the host path)' % name)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError('svm_ops: %s must be a 2-D fp32 tensor' % name)
    return t.detach()


def fit_predict_ovo(train_feats, train_labels, test_feats, Cs=SVM_CS, eps=1e-3, max_iter=MAX_ITER):
    """SVC(C=c, kernel='linear', tol=eps).fit(train).predict(test) for every c of Cs at once.

    train_feats (n, D), test_feats (m, D): fp32 on the device; train_labels (n,): host array or tensor.
    -> pred (nC, m) numpy, the predicted labels; dec (nC, m, P) fp64 on the device, the pairwise decision values in
    sklearn's decision_function_shape='ovo' order; status: dict of classes (K,), iters (nC, P), capped (nC, P) bool,
    gap (nC, P), and coef (nC, K - 1, n), rho (nC, P) on the device (dual_coef_ with its columns over ALL training samples
    in class order, intercept_ = -rho).  Raises when a problem hit max_iter, naming the pair and the C."""
    X, Xt = _require_feats(train_feats, 'train_feats'), _require_feats(test_feats, 'test_feats')
    if X.shape[1] != Xt.shape[1]:
        raise ValueError('svm_ops: train and test features differ in width')
    if isinstance(train_labels, torch.Tensor):
        train_labels = train_labels.detach().cpu().numpy()
    classes, order, class_ptr = class_layout(train_labels)
    n, m, K, nC = X.shape[0], Xt.shape[0], len(classes), len(Cs)
    if order.shape[0] != n:
        raise ValueError('svm_ops: %d labels for %d feature rows' % (order.shape[0], n))
    if K < 2:
        raise ValueError('svm_ops: the number of classes has to be greater than one')
    P = K * (K - 1) // 2
    dev = X.device
    cptr = (ctypes.c_int * (K + 1))(*class_ptr.tolist())
    cs = (ctypes.c_double * nC)(*[float(c) for c in Cs])
    order_d = torch.from_numpy(order).to(dev)
    coef = torch.empty((nC, K - 1, n), device=dev, dtype=torch.float64)
    rho = torch.empty((nC, P), device=dev, dtype=torch.float64)
    gap = torch.empty((nC, P), device=dev, dtype=torch.float64)
    st = torch.empty((nC, P, 2), device=dev, dtype=torch.int32)
    # a layout the solver refuses (a pair above MAX_PAIR members, too many classes or Cs, max_iter < 1) raises here,
    # before anything is launched
    handle = _lib.lib()
    _lib._check(handle, 'pdae_svm_ovo_supported', handle.pdae_svm_ovo_supported(n, K, nC, cptr, cs, int(max_iter)))
    Xp = _padded(X)
    G = rows_gemm(Xp, Xp)                                # (n4, n4)
    _lib.call('pdae_svm_ovo_train', X, n, G.shape[1], K, nC, _lib.ptr(G), _lib.ptr(order_d), cptr, cs, float(eps),
              int(max_iter), _lib.ptr(coef), _lib.ptr(rho), _lib.ptr(st), _lib.ptr(gap))
    del G
    Gte = rows_gemm(_padded(Xt), Xp)                     # (m4, n4)
    dec = torch.empty((nC, m, P), device=dev, dtype=torch.float64)
    pred = torch.empty((nC, m), device=dev, dtype=torch.int32)
    _lib.call('pdae_svm_ovo_predict', X, m, n, Gte.shape[1], K, nC, _lib.ptr(Gte), _lib.ptr(order_d), cptr, _lib.ptr(coef),
              _lib.ptr(rho), _lib.ptr(dec), _lib.ptr(pred))
    st_h = st.cpu().numpy()
    status = dict(classes=classes, iters=st_h[..., 0], capped=st_h[..., 1] != 0, gap=gap.cpu().numpy(), coef=coef, rho=rho)
    if status['capped'].any():
        ci, k = (int(v) for v in np.argwhere(status['capped'])[0])
        p, q = pairs(K)[k]
        raise RuntimeError('svm_ops: the solver hit max_iter = %d on the class pair (%s, %s) at C = %g (violation %.3g, '
                           'eps %g); %d of %d problems did' % (max_iter, classes[p], classes[q], Cs[ci],
                                                               status['gap'][ci, k], eps, int(status['capped'].sum()), nC * P))
    return classes[pred.cpu().numpy()], dec, status


def accuracies(train_feats, train_labels, test_feats, test_labels, Cs=SVM_CS):
    """model_tl.score(test) of SVC(C=c, kernel='linear') per c of Cs, as fractions: on the kernels (PDAE_SVM=hip) or by the
    reference's own call on the host (PDAE_SVM=sklearn)."""
    def host(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    test_labels = host(test_labels).reshape(-1)
    if backend() == 'sklearn':
        from .svm_probe import svc_accuracies
        return svc_accuracies(host(train_feats), host(train_labels).reshape(-1), host(test_feats), test_labels, Cs)
    pred, _, _ = fit_predict_ovo(train_feats, train_labels, test_feats, Cs)
    return [float(np.mean(pred[i] == test_labels)) for i in range(len(Cs))]
