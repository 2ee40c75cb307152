"""The device LinearSVC (csrc/linsvc.hip, point_dae_amd/linsvc_ops.py) against sklearn on the host, on the seeded shapes of
tests/linsvc_cases.py: the optimum, the stopping rule, the predictions, the accuracy, bit-reproducibility, the refusals and
the pretraining runner's validate() end to end.

Measured on an MI355X, max|W - W_ref| / max|W_ref| with the fit run to the fp32 products' floor (tol = 1e-8, where the
classes end stalled, capped or at a threshold no default fit asks for): MEASURED_W_ERR below.  Each shape's bound is four
times its value -- the four covers the scatter of a rounding-level quantity -- under a ceiling of 1e-3: more is a wrong
objective, not rounding.  At the default tol = 1e-4 the same metric is 2e-3 .. 1.4e-1 (sklearn's own default fit: 4e-5 ..
2.4e-1): liblinear's stopping rule is loose, which is why the optimum is compared at the floor.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

import linsvc_cases as cases
import proc_util

pytestmark = pytest.mark.gpu
ROOT = cases.ROOT
NAMES = list(cases.SHAPES)
MEASURED_W_ERR = {'small': 2.186e-07, 'ragged': 1.930e-07, 'uneven40': 1.199e-07, 'wide': 3.884e-06, 'd_gt_n': 1.186e-07}


def w_bound(name):
    return min(4.0 * MEASURED_W_ERR[name], 1e-3)


@functools.lru_cache(maxsize=None)
def device_features(name):
    xtr, ytr, xte, yte = cases.features(name)
    return torch.from_numpy(xtr).cuda(), ytr, torch.from_numpy(xte).cuda(), yte


@functools.lru_cache(maxsize=None)
def fit(name, tol=1e-4):
    """-> pred, W (fp64 on the host), status; tol = 1e-8 runs to the products' floor (no class meets it: check=False)."""
    from point_dae_amd import linsvc_ops
    xtr, ytr, xte, _ = device_features(name)
    pred, W, status = linsvc_ops.fit_predict(xtr, ytr, xte, tol=tol, check=tol >= 1e-4)
    return pred, W.double().cpu().numpy(), status


@pytest.mark.parametrize('name', NAMES)
def test_optimum(name):
    _, W, status = fit(name, 1e-8)
    W_ref = cases.w_ref(name)
    assert W.shape == W_ref.shape == (cases.SHAPES[name][2] + 1, cases.SHAPES[name][3])
    err = np.abs(W - W_ref).max() / np.abs(W_ref).max()
    print('%s: max|W - W_ref| / max|W_ref| = %.3e (bound %.3e), Newton steps %d, Hessian products %d, stalled %d capped %d'
          % (name, err, w_bound(name), status['newton_iters'].max(), status['hv_products'], status['stalled'].sum(),
             status['capped'].sum()))
    assert err <= w_bound(name)


@pytest.mark.parametrize('name', NAMES)
def test_converges_by_liblinears_rule(name):
    from point_dae_amd import linsvc_ops
    _, _, status = fit(name)
    _, index = linsvc_ops.label_layout(cases.features(name)[1])
    threshold = linsvc_ops.stopping_eps(index, len(status['classes']), 1e-4)
    print('%s: Newton steps %s, Hessian products %d, max ratio / threshold %.3f'
          % (name, status['newton_iters'].max(), status['hv_products'], (status['grad_ratio'] / threshold).max()))
    assert not status['capped'].any() and not status['stalled'].any()
    assert np.array_equal(status['threshold'], threshold)
    assert (status['grad_ratio'] <= threshold).all()
    assert np.array_equal(status['classes'], np.unique(cases.features(name)[1]))
    if name == 'uneven40':                               # a class of 2 members against one of 40: the thresholds differ 20-fold
        assert threshold.min() == 1e-4 * 2 / 260 and threshold.max() >= 10 * threshold.min()
        assert status['newton_iters'].min() < status['newton_iters'].max()     # some machines finish early, others go on


@pytest.mark.parametrize('name', NAMES)
def test_predictions(name):
    pred, _, _ = fit(name)
    ref_pred, excluded = cases.default_fit(name)
    assert excluded.mean() <= cases.EXCLUDED_CAP
    differ = pred != ref_pred
    print('%s: %d of %d predictions differ, %d rows excluded' % (name, differ.sum(), len(pred), excluded.sum()))
    assert not (differ & ~excluded).any(), np.flatnonzero(differ & ~excluded)


@pytest.mark.parametrize('name', NAMES)
def test_accuracy(name, monkeypatch):
    from point_dae_amd import linsvc_ops
    from point_dae_amd.svm_probe import evaluate_svm
    xtr, ytr, xte, yte = device_features(name)
    monkeypatch.setenv('PDAE_LINSVC', 'hip')
    got = linsvc_ops.accuracy(xtr, torch.from_numpy(ytr).cuda(), xte, torch.from_numpy(yte))
    want = evaluate_svm(*cases.features(name))
    _, excluded = cases.default_fit(name)
    print('%s: accuracy %.4f, sklearn %.4f' % (name, got, want))
    assert abs(got - want) <= excluded.mean() + 1e-12
    monkeypatch.setenv('PDAE_LINSVC', 'sklearn')
    assert linsvc_ops.accuracy(xtr, ytr, xte, yte) == want


def test_two_classes_are_one_machine():
    """sklearn's binary case: coef_ has one row, the machine of classes[1]."""
    from sklearn.svm import LinearSVC
    from point_dae_amd import linsvc_ops
    xtr, ytr, xte, _ = cases.features('small')
    keep, keep_te = ytr <= 8, slice(0, 64)               # the labels 5 and 8
    x, y = xtr[keep], ytr[keep]
    pred, W, status = linsvc_ops.fit_predict(torch.from_numpy(x).cuda(), y, torch.from_numpy(xte[keep_te]).cuda())
    assert W.shape == (21, 1) and status['newton_iters'].shape == (1,) and status['classes'].tolist() == [5, 8]
    clf = LinearSVC().fit(x, y)
    excluded = cases.excluded_rows(clf.decision_function(xte[keep_te]))
    assert not ((pred != clf.predict(xte[keep_te])) & ~excluded).any()
    ref = cases.sk_weights(LinearSVC(dual=False, tol=1e-10, max_iter=10000).fit(x, y))
    _, W8, _ = linsvc_ops.fit_predict(torch.from_numpy(x).cuda(), y, torch.from_numpy(xte[keep_te]).cuda(), tol=1e-8, check=False)
    assert np.abs(W8.double().cpu().numpy() - ref).max() / np.abs(ref).max() <= 1e-3      # (no measured bound: the ceiling)


def test_bit_reproducible():
    from point_dae_amd import _lib, linsvc_ops
    xtr, ytr, xte, _ = device_features('ragged')
    _lib.set_deterministic(True)
    try:
        _, W1, s1 = linsvc_ops.fit_predict(xtr, ytr, xte)
        _, W2, s2 = linsvc_ops.fit_predict(xtr, ytr, xte)
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(W1, W2) and np.array_equal(s1['grad_ratio'], s2['grad_ratio'])
    assert np.array_equal(s1['newton_iters'], s2['newton_iters'])


def test_refusals():
    from point_dae_amd import _lib, linsvc_ops
    calls = []
    prev, _lib.CALL_HOOK = _lib.CALL_HOOK, lambda name, args: calls.append(name)
    try:
        x = torch.rand(130, 8, device='cuda')
        with pytest.raises(RuntimeError, match='PDAE_LINSVC_MAX_CLASSES'):
            linsvc_ops.fit_predict(x, np.arange(130) % 65, x)
        with pytest.raises(RuntimeError, match='greater than one'):
            linsvc_ops.fit_predict(x, np.zeros(130, np.int64), x)
        with pytest.raises(RuntimeError, match='empty'):
            linsvc_ops.fit_predict(x[:0], np.zeros(0, np.int64), x)
        assert calls == []                               # refused before any launch
    finally:
        _lib.CALL_HOOK = prev
    xtr, ytr, xte, _ = device_features('uneven40')
    with pytest.raises(RuntimeError, match=r'the machine of class \d+ took max_newton = 1 Newton steps'):
        linsvc_ops.fit_predict(xtr, ytr, xte, max_newton=1)
    with pytest.raises(RuntimeError, match='GPU'):
        linsvc_ops.fit_predict(xtr.cpu(), ytr, xte)


def _validate(backend):
    env = dict(os.environ, PDAE_LINSVC=backend)
    r = proc_util.run([sys.executable, os.path.join(ROOT, 'tests', 'linsvc_cases.py'), 'validate'], 600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('[Validation] EPOCH: ')]
    assert len(line) == 1 and re.fullmatch(r'\[Validation\] EPOCH: 7  acc = \d\.\d{4}', line[0]), r.stdout[-2000:]
    tail = re.search(r'PATH (\w+) CLASSES (\d+) EXCLUDED ([\d.]+)', r.stdout)
    assert tail and tail.group(1) == backend and tail.group(2) == '4', r.stdout[-2000:]
    return float(line[0].split('acc = ')[1]), float(tail.group(3))


def test_validate_end_to_end():
    """svm_probe.validate under PDAE_LINSVC=hip and =sklearn, each in a fresh process: the two lines agree within the share
    of test rows the reference fit leaves within delta (+ 1e-4: the line prints four decimals).

    Both loaders hold the same 64 clouds under the same corruption draws, so the rows scored are the rows fitted.  On
    64 x 384 features of an untrained encoder liblinear's dual solver stops at max_iter = 1000 with a ConvergenceWarning,
    24 % from the optimum, and labels 5 of 48 UNSEEN clouds differently from its own optimum (LinearSVC(dual=False,
    tol=1e-10)), on rows whose two best decision values lie 3 .. 22 delta apart; the device fit lands 5e-4 from the optimum
    and labels every one of them as the optimum does (measured on an MI355X: 0.5625 against the comparator's 0.6042).  An
    unconverged fit is no comparator for rows it has not seen; the rows it was fitted on it has pushed past the margin."""
    acc_hip, share_hip = _validate('hip')
    acc_host, share_host = _validate('sklearn')
    print('validate: hip %.4f sklearn %.4f, excluded share %.4f / %.4f' % (acc_hip, acc_host, share_hip, share_host))
    assert max(share_hip, share_host) <= cases.EXCLUDED_CAP
    assert abs(acc_hip - acc_host) <= max(share_hip, share_host) + 1e-4
    assert acc_hip > 0.5                                 # (the largest class is 26 of the 64 clouds)
