"""Writes tests/golden/forest_sklearn.npz: a small fully grown scikit-learn forest as its raw ``tree_`` arrays, fp16 test rows
and clf.predict on them, so that the conversion and the vote are pinned where scikit-learn is absent.

    python tests/golden/make_golden_forest.py

Needs scikit-learn (written with 1.7.2) and numpy, nothing else.  12 trees, F = 32, 4 classes, 400 training rows of
overlapping blobs (100 to 160 nodes per tree), 2000 test rows.  Per tree t the file holds children_left_t, children_right_t,
feature_t, threshold_t (fp64, as scikit-learn keeps it) and value_t [nodes][4]; x_test fp16 [2000][32]; predict int64 [2000];
classes int64 [4]; n_features.
"""
import os

import numpy as np
from sklearn.ensemble import RandomForestClassifier

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    rng = np.random.default_rng(20)
    mu = 0.5 * rng.standard_normal((4, 32))
    y = rng.integers(0, 4, 400)
    x = (mu[y] + rng.standard_normal((400, 32))).astype(np.float16)
    yt = rng.integers(0, 4, 2000)
    xt = (mu[yt] + rng.standard_normal((2000, 32))).astype(np.float16)
    clf = RandomForestClassifier(n_estimators=12, random_state=0).fit(x.astype(np.float32), y)
    out = {'x_test': xt, 'predict': clf.predict(xt.astype(np.float32)).astype(np.int64), 'classes': clf.classes_.astype(np.int64),
           'n_features': np.asarray(32, np.int64), 'n_trees': np.asarray(12, np.int64)}
    for t, est in enumerate(clf.estimators_):
        tr = est.tree_
        out[f'children_left_{t}'] = tr.children_left.astype(np.int32)
        out[f'children_right_{t}'] = tr.children_right.astype(np.int32)
        out[f'feature_{t}'] = tr.feature.astype(np.int32)
        out[f'threshold_{t}'] = tr.threshold.astype(np.float64)
        out[f'value_{t}'] = tr.value.reshape(tr.node_count, -1).astype(np.float64)
    path = os.path.join(HERE, 'forest_sklearn.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', [int(e.tree_.node_count) for e in clf.estimators_], 'nodes')


if __name__ == '__main__':
    main()
