"""Writes tests/golden/linsvc_ref_d.npz: the optimum of sklearn's LinearSVC on the widest shape of tests/test_gpu_linsvc.py.

LinearSVC(dual=False, tol=1e-10, max_iter=10000) takes liblinear about 40 s on the (1200, 384) features with 40 classes,
too long for a test that runs with every suite; the other shapes' references are fitted in the test itself.  The file
holds W_ref (D + 1, K) fp64 = [coef_, intercept_] per column and the generator's arguments; the test regenerates the
features from them and checks the stored optimum against its own fp64 gradient before using it.

    python tests/golden/make_linsvc_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from sklearn.svm import LinearSVC
    from point_dae_amd.synthetic import class_features
    n, m, D, K, sep, seed = 1200, 400, 384, 40, 0.5, 11
    xtr, ytr, _, _ = class_features(n, m, D, K, sep=sep, seed=seed)
    ref = LinearSVC(dual=False, tol=1e-10, max_iter=10000).fit(xtr, ytr)
    w = np.concatenate([ref.coef_, ref.intercept_[:, None]], 1).T
    np.savez_compressed(os.path.join(HERE, 'linsvc_ref_d.npz'), W_ref=w, shape=np.array([n, m, D, K, seed]),
                        sep=np.array(sep), n_iter=np.array(ref.n_iter_))
    print('W_ref', w.shape, 'n_iter', ref.n_iter_)


if __name__ == '__main__':
    main()
