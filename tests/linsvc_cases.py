"""Shared by tests/test_linsvc_cpu.py and tests/test_gpu_linsvc.py: the seeded shapes, sklearn's fits on them (computed
once per session) and an fp64 restatement of LinearSVC's objective.

Run as a program it is the child process of the end-to-end validation test:
    python tests/linsvc_cases.py validate      (PDAE_LINSVC picks the fit)
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> n, m, D, K, class separation, uneven class sizes.  The separations keep the share of test rows whose two best
# decision values of LinearSVC()'s own fit lie closer than delta under 2 % (test_linsvc_cpu.py checks it).
SHAPES = {
    'small': (300, 200, 20, 5, 1.5, False),            # the smallest case with every code path
    'ragged': (517, 203, 37, 7, 1.0, False),           # n, m, D, D + 1 off the multiples of 4
    'uneven40': (260, 100, 64, 40, 1.0, True),         # the probe's K, class sizes ~ 1 / (k + 1), the last class 2 members
    'wide': (1200, 400, 384, 40, 0.5, False),          # the probe's width
    'd_gt_n': (128, 64, 200, 4, 0.6, False),           # D > n: sklearn's dual='auto' takes the dual
}
SEED = 11
EXCLUDED_CAP = 0.02


@functools.lru_cache(maxsize=None)
def features(name):
    """-> train (n, D) f32, train_labels, test (m, D) f32, test_labels.  Labels are 3 k + 5: not their own indices."""
    from point_dae_amd.synthetic import class_features
    n, m, D, K, sep, uneven = SHAPES[name]
    sizes = None
    if uneven:
        sizes = 1.0 / (1.0 + np.arange(K))
        sizes[-1] = 0.0
    xtr, ytr, xte, yte = class_features(n, m, D, K, sep=sep, seed=SEED, sizes=sizes)
    return xtr, 3 * ytr + 5, xte, 3 * yte + 5


def with_ones(x):
    return np.concatenate([np.asarray(x, np.float64), np.ones((len(x), 1))], 1)


def objective(W, x, Y, C=1.0):
    """fp64: f (ncol,) and the gradient (D + 1, ncol) of f_k(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_ik a_i.w)^2 at the
    columns of W, a_i = [x_i, 1], Y (n, ncol) of +-1."""
    A = with_ones(x)
    R = np.maximum(0.0, 1.0 - Y * (A @ W))
    return 0.5 * (W * W).sum(0) + C * (R * R).sum(0), W - 2.0 * C * (A.T @ (Y * R))


def sk_weights(clf):
    """[coef_, intercept_] per column: (D + 1, ncol)."""
    return np.concatenate([clf.coef_, np.reshape(clf.intercept_, (-1, 1))], 1).T


@functools.lru_cache(maxsize=None)
def w_ref(name):
    """The optimum by LinearSVC(dual=False, tol=1e-10, max_iter=10000); the widest shape's takes liblinear 40 s and is
    stored (tests/golden/linsvc_ref_d.npz, make_linsvc_fixture.py)."""
    if name == 'wide':
        f = np.load(os.path.join(ROOT, 'tests', 'golden', 'linsvc_ref_d.npz'))
        n, m, D, K, _, _ = SHAPES[name]
        assert f['shape'].tolist() == [n, m, D, K, SEED] and float(f['sep']) == SHAPES[name][4]
        return f['W_ref']
    from sklearn.svm import LinearSVC
    xtr, ytr, _, _ = features(name)
    return sk_weights(LinearSVC(dual=False, tol=1e-10, max_iter=10000).fit(xtr, ytr))


@functools.lru_cache(maxsize=None)
def default_fit(name):
    """LinearSVC()'s own fit -> (pred (m,), excluded (m,) bool): the rows whose two best decision values lie closer than
    delta = 1e-3 * the largest absolute decision value."""
    from sklearn.svm import LinearSVC
    xtr, ytr, xte, _ = features(name)
    clf = LinearSVC().fit(xtr, ytr)
    return clf.predict(xte), excluded_rows(clf.decision_function(xte))


def excluded_rows(dec):
    dec = np.asarray(dec)
    delta = 1e-3 * np.abs(dec).max()
    if dec.ndim == 1:                                  # two classes: one machine, the runner-up is its negative
        return 2.0 * np.abs(dec) < delta
    top = np.sort(dec, 1)
    return top[:, -1] - top[:, -2] < delta


def four_class_clouds(count, N, seed):
    """labelled_clouds' three families and a fourth: boxes flattened to a third of their height."""
    from point_dae_amd.synthetic import labelled_clouds
    x, y = labelled_clouds(count, N, seed=seed)
    flat = (np.arange(count) % 4 == 3) & (y == 1)
    x[flat, :, 2] *= 1.0 / 3.0
    x[flat] /= np.sqrt((x[flat] ** 2).sum(2)).max(1)[:, None, None]
    y[flat] = 3
    return x, y


def _validate_child():
    """svm_probe.validate on a depth-2 encoder and two loaders of the same synthetic labelled clouds; prints its line and
    the share of test rows LinearSVC()'s own fit on the same features leaves within delta."""
    import random
    import torch
    from sklearn.svm import LinearSVC
    from point_dae_amd import builder, linsvc_ops, svm_probe
    from point_dae_amd.config import cfg_from_yaml_file
    config = cfg_from_yaml_file(os.path.join(
        ROOT, 'cfgs', 'pretrain_PointCAE_transformer_dropout_patch_affine_r3_maskpatch_p0005_whole.yaml'))
    config.model.NAME = 'PointCAE_transformer_fc_global_folding_local'
    config.model.transformer_config.depth = 2
    config.model.transformer_config.decoder_depth = 1
    random.seed(3), np.random.seed(3), torch.manual_seed(3)
    net = builder.model_builder(config.model).cuda()
    net.corrupt_type = ['Drop-Patch']

    def loader(x, y, bs=16):
        return [('ModelNet', i, (torch.from_numpy(x[i:i + bs]), torch.from_numpy(y[i:i + bs]))) for i in range(0, len(x), bs)]
    tr = te = four_class_clouds(64, 1024, 21)            # (the same clouds twice: test_gpu_linsvc.test_validate_end_to_end)
    extract = svm_probe.extract_features

    def same_draws(model, data, npoints):                # both passes corrupt the clouds alike: the rows scored are the rows fitted
        random.seed(5), np.random.seed(5), torch.manual_seed(5)
        return extract(model, data, npoints)
    svm_probe.extract_features = same_draws
    config.dataset.extra_train = {'others': {'npoints': 1024}}
    seen = {}
    fit_hip, fit_host = linsvc_ops.accuracy, svm_probe.evaluate_svm

    def on_device(tr_f, tr_l, te_f, te_l):
        seen.update(tr_f=tr_f.cpu().numpy(), tr_l=tr_l.cpu().numpy(), te_f=te_f.cpu().numpy(), path='hip')
        return fit_hip(tr_f, tr_l, te_f, te_l)

    def on_host(tr_f, tr_l, te_f, te_l):
        seen.update(tr_f=tr_f, tr_l=tr_l, te_f=te_f, path='sklearn')
        return fit_host(tr_f, tr_l, te_f, te_l)
    linsvc_ops.accuracy, svm_probe.evaluate_svm = on_device, on_host
    svm_probe.validate(net, loader(*tr), loader(*te), 7, config)
    clf = LinearSVC().fit(seen['tr_f'], seen['tr_l'])
    dec = clf.decision_function(seen['te_f'])
    top = np.sort(dec, 1)
    print('PATH %s CLASSES %d EXCLUDED %.6f' % (seen['path'], len(clf.classes_), excluded_rows(dec).mean()))
    print('smallest gap of the two best decision values: %.1f delta; rows scored differ from rows fitted by %.3g'
          % ((top[:, -1] - top[:, -2]).min() / (1e-3 * np.abs(dec).max()), np.abs(seen['te_f'] - seen['tr_f']).max()))


if __name__ == '__main__':
    assert sys.argv[1:] == ['validate'], sys.argv
    _validate_child()
