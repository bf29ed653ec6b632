"""CPU: random-forest classification -- the C-ABI surface of vittf_forest_decide (declared, exported, argument checks without
a launch), floor16 exhaustively, validate(), the CART fit of vit_tf_amd.forest (exactness on its training rows, determinism,
independence of the trees, its limits) and its held-out accuracy beside scikit-learn's, from_sklearn against clf.predict, the
golden scikit-learn forest, the model files, and the refusals of classify_features.py --classifier forest.
"""
import ctypes as C
import functools
import os
import re
import time

import numpy as np
import pytest

import vit_tf_amd as vt
from vit_tf_amd import _lib
import forest_data as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
forest = vt.forest


def as_dict(m):
    return dict(tree_offset=m.tree_offset, feature=m.feature, threshold=m.threshold, left=m.left, right=m.right, value=m.value)


def as_model(fr, F, names=None):
    c = fr['value'].shape[1]
    return forest.ForestModel(names or [str(i) for i in range(c)], np.arange(c), F, fr['tree_offset'], fr['feature'], fr['threshold'],
                              fr['left'], fr['right'], fr['value'])


# ---------------------------------------------------------------------------- 1. ABI surface
def _call(lib, f=384, nvox=1000, trees=10, classes=3, max_depth=12, feat=1, nodes=1, leaf_values=1, tree_offset=1, labels=1,
          addr=0x1000, votes=None):
    """vittf_forest_decide on placeholder addresses: only calls the argument checks refuse are made with it."""
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_forest_decide(p(feat), f, nvox, p(nodes), p(leaf_values), p(tree_offset), trees, classes, max_depth, p(labels),
                                   votes, None)


def test_forest_entry_is_declared_exported_and_validates():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    for name, want in (('CLASSES', 8), ('TREES', 4096), ('NODES', 65535), ('DEPTH', 64)):
        assert int(re.search(r'#define\s+VITTF_FOREST_MAX_' + name + r'\s+(\d+)', header).group(1)) == want == getattr(_lib, 'FOREST_MAX_' + name)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    assert re.search(r'\bint\s+vittf_forest_decide\s*\(', header), 'vittf_forest_decide is not declared in include/vittf.h'
    assert 'vittf_forest_decide' in _lib.SIGNATURES and hasattr(lib, 'vittf_forest_decide')
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    for f in (0, 16, 48, 1056, -32):
        assert _call(lib, f=f) == INVALID, f
    for c in (0, 1, 9):
        assert _call(lib, classes=c) == INVALID, c
    for t in (0, -1, 4097):
        assert _call(lib, trees=t) == INVALID, t
    for d in (-1, 65):
        assert _call(lib, max_depth=d) == INVALID, d
    for nvox in (0, -5):
        assert _call(lib, nvox=nvox) == INVALID, nvox
    for missing in ('feat', 'nodes', 'leaf_values', 'tree_offset', 'labels'):
        assert _call(lib, **{missing: 0}) == INVALID, missing
    for addr in (0x1001, 0x1002, 0x1004, 0x1008):            # feat: 2 bytes, tree_offset: 4, nodes: 8, leaf rows: 16
        assert _call(lib, addr=addr) == INVALID, addr
    assert _call(lib, votes=C.c_void_p(0x1002)) == INVALID   # a misaligned optional array alone


# ---------------------------------------------------------------------------- 2. floor16
def test_floor16_keeps_every_comparison_with_every_finite_fp16():
    """x <= t equals x <= floor16(t) for ALL 63 488 finite fp16 x, for thresholds of every kind the conversions meet."""
    rng = np.random.default_rng(0)
    x = fd.ALL_FINITE_F16
    assert x.size == 63488
    some = x[rng.integers(0, x.size, 300)].astype(np.float64)
    pairs = np.sort(rng.standard_normal((300, 2)).astype(np.float16), axis=1).astype(np.float32)
    sub = np.asarray([2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -24, -2.0 ** -24, -2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 1e-30, -1e-30])
    t = np.concatenate([((pairs[:, 0] + pairs[:, 1]) / np.float32(2)).astype(np.float64),     # fp32 midpoints of fp16 neighbours-to-be
                        some, np.nextafter(some, np.inf), np.nextafter(some, -np.inf), some * (1 + 1e-4), some * (1 - 1e-4),
                        [0.0, -0.0, np.inf, -np.inf], sub,
                        [65504.0, 65505.0, 65519.9, 65520.0, 70000.0, 1e300, -65504.0, -65504.1, -65520.0, -70000.0, -1e300]])
    xf = x.astype(np.float64)
    for name, fl in (('vt.forest.floor16', forest.floor16), ('forest_data.floor16', fd.floor16)):
        got = fl(t)
        assert got.dtype == np.float16 and got.shape == t.shape
        g = got.astype(np.float64)
        assert (g <= t).all(), name
        want = xf[None, :] <= t[:, None]
        assert np.array_equal(xf[None, :] <= g[:, None], want), name
        assert np.array_equal(x[None, :] <= got[:, None], want), f'{name}: compared as fp16 numbers'
    assert np.array_equal(forest.floor16(t).astype(np.float64), fd.floor16(t).astype(np.float64))
    assert forest.floor16(np.inf) == np.inf and forest.floor16(-np.inf) == -np.inf and forest.floor16(1e300) == 65504
    assert forest.floor16(-65504.1) == -np.inf and forest.floor16(-1e-30) == -2.0 ** -24
    with pytest.raises(ValueError):
        forest.floor16([0.0, np.nan])


# ---------------------------------------------------------------------------- 3. validate
def test_validate_refuses_what_could_leave_a_tree_or_spin():
    rng = np.random.default_rng(1)
    good = fd.random_forest(rng, 5, 32, 3)
    m = as_model(good, 32)
    assert m.max_depth == fd.depth_of(good) and m.trees == 5

    def broken(**changes):
        fr = {k: v.copy() for k, v in good.items()}
        for k, fn in changes.items():
            fn(fr[k])
        return fr
    inner = int(np.flatnonzero(good['feature'] >= 0)[-1])
    local = inner - good['tree_offset'][np.searchsorted(good['tree_offset'], inner, side='right') - 1]

    def put(i, v):
        return lambda a: a.__setitem__(i, v)
    for what, fr in (('child == parent', broken(left=put(inner, local))),
                     ('child before parent', broken(right=put(inner, max(local - 1, 0)))),
                     ('child out of range', broken(right=put(inner, 70000))),
                     ('child in the next tree', broken(left=put(int(np.flatnonzero(good['feature'][:good['tree_offset'][1]] >= 0)[0]),
                                                                 int(good['tree_offset'][1])))),
                     ('feature >= F', broken(feature=put(inner, 32))),
                     ('feature < -1', broken(feature=put(inner, -2))),
                     ('NaN threshold', broken(threshold=put(inner, np.nan)))):
        with pytest.raises(ValueError):
            as_model(fr, 32)
            pytest.fail(what)
    assert as_model(_full_tree(0), 32).max_depth == 15        # 65535 nodes: the most a tree may have
    for extra in (1, 2):                                      # 65536 nodes (whatever they hold) and a proper tree of 65537
        with pytest.raises(ValueError, match='nodes'):
            as_model(_full_tree(extra), 32)
    with pytest.raises(ValueError, match='deeper'):
        as_model(fd.forest_of([fd.chain_tree(rng, 32, 2, 65)]), 32)
    assert as_model(fd.forest_of([fd.chain_tree(rng, 32, 2, 64)]), 32).max_depth == 64
    with pytest.raises(ValueError, match='classes'):
        as_model(fd.forest_of([fd.leaf_tree(list(range(9)))]), 32)
    with pytest.raises(ValueError, match='classes'):
        as_model(fd.forest_of([fd.leaf_tree([7])]), 32)
    with pytest.raises(ValueError, match='trees'):
        as_model(fd.forest_of([fd.leaf_tree([1, 2])] * 4097), 32)
    assert as_model(fd.forest_of([fd.leaf_tree([1, 2])] * 4096), 32).max_depth == 0
    for f in (0, 48, 1056):
        with pytest.raises(ValueError, match='F must'):
            as_model(good, f)
    # two parents for one node (a DAG), and a node nobody points to
    with pytest.raises(ValueError, match='exactly one'):
        fr = fd.forest_of([fd.stump(0, 0.0, [1, 0], [0, 1])])
        fr['right'][0] = 1
        as_model(fr, 32)


def _full_tree(extra):
    """The full binary tree of depth 15 in breadth-first order (65535 nodes); extra = 2 splits its last leaf, extra = 1 only
    appends one node."""
    n = 65535 + extra
    i = np.arange(n)
    inner = i < 32767
    fr = dict(feature=np.where(inner, i % 32, -1).astype(np.int32), threshold=np.zeros(n, np.float16),
              left=np.where(inner, 2 * i + 1, -1).astype(np.int32), right=np.where(inner, 2 * i + 2, -1).astype(np.int32),
              value=np.ones((n, 2), np.uint16), tree_offset=np.asarray([0, n], np.int64))
    if extra == 2:
        fr['feature'][65534], fr['left'][65534], fr['right'][65534] = 0, 65535, 65536
    return fr


# ---------------------------------------------------------------------------- 4. the fit
@functools.lru_cache(None)
def _planted(n, F, classes, seed):
    x, y = fd.blobs(n, F, classes, 1.0, seed)
    assert np.unique(x, axis=0).shape[0] == n                 # distinct rows
    return x, y


def test_fit_without_bootstrap_classifies_every_training_row():
    """Fully grown CART on distinct rows, every tree seeing every row: every tree alone is right on every training row."""
    for F, classes, mf in ((32, 3, 'sqrt'), (96, 6, 'all'), (32, 8, 5), (64, 2, 0.25)):
        x, y = _planted(240, F, classes, F + classes)
        m = forest.fit(x, y + 3, trees=6, max_features=mf, bootstrap=False, seed=2)
        assert m.labels.tolist() == list(range(3, 3 + classes)) and m.trees == 6 and m.n_features == F
        for t in range(6):
            one = {k: v for k, v in as_dict(m).items()}
            lo, hi = m.tree_offset[t], m.tree_offset[t + 1]
            one = {k: (v[lo:hi] if k != 'tree_offset' else np.asarray([0, hi - lo])) for k, v in one.items()}
            votes, labels, _ = fd.walk(one, np.ascontiguousarray(x.T))
            assert np.array_equal(labels, y), (F, classes, mf, t)
            assert set(np.unique(votes)) <= {0, 65535}       # pure leaves


def test_fit_is_deterministic_and_its_trees_independent():
    x, y = _planted(300, 32, 4, 9)
    a, b = forest.fit(x, y, trees=16, seed=5), forest.fit(x, y, trees=16, seed=5)
    for k in ('tree_offset', 'feature', 'threshold', 'left', 'right', 'value'):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    first = forest.fit(x, y, trees=8, seed=5)
    n8 = int(first.tree_offset[-1])
    assert np.array_equal(a.tree_offset[:9], first.tree_offset)
    for k in ('feature', 'threshold', 'left', 'right', 'value'):
        assert getattr(a, k)[:n8].tobytes() == getattr(first, k).tobytes(), k
    assert forest.fit(x, y, trees=8, seed=6).feature.tobytes() != first.feature.tobytes()
    # the thresholds are fp16 values between two training values; the children come behind their parents
    inner = a.feature >= 0
    assert a.threshold.dtype == np.float16 and np.isfinite(a.threshold[inner]).all()


def test_fit_honours_max_depth_and_min_samples_leaf():
    x, y = fd.blobs(600, 32, 4, 0.3, 3)                       # overlapping: fully grown trees are deep
    full = forest.fit(x, y, trees=4, seed=1)
    assert full.max_depth > 6
    m = forest.fit(x, y, trees=4, max_depth=3, seed=1)
    assert m.max_depth == 3 and fd.depth_of(as_dict(m)) == 3
    leaf = m.feature < 0
    sums = m.value.astype(np.int64).sum(1)
    assert (np.abs(sums - 65535) <= m.classes / 2).all() and (m.value[leaf].max(1) < 65535).any()       # impure leaves, shares sum to 1
    m = forest.fit(x, y, trees=3, min_samples_leaf=25, bootstrap=False, seed=1)
    xt = np.ascontiguousarray(x.T)
    ends = fd.walk(as_dict(m), xt)[2]
    for t in range(3):
        assert np.bincount(ends[t]).max() >= 25 and np.bincount(ends[t])[np.bincount(ends[t]) > 0].min() >= 25
    sums = m.value.astype(np.int64).sum(1)
    assert (np.abs(sums - 65535) <= m.classes / 2).all()


def test_fit_refuses_bad_arguments():
    x, y = _planted(240, 32, 3, 35)
    for kw in (dict(trees=0), dict(trees=4097), dict(max_depth=0), dict(max_depth=65), dict(min_samples_leaf=0),
               dict(max_features=0), dict(max_features=33), dict(max_features=1.5), dict(max_features='log2'),
               dict(class_names=['a'])):
        with pytest.raises(ValueError):
            forest.fit(x, y, **{'trees': 2, **kw})
    with pytest.raises(ValueError):
        forest.fit(x, np.zeros(240, np.int64), trees=2)       # one class
    with pytest.raises(ValueError):
        forest.fit(x, np.arange(240) % 9, trees=2)            # nine classes
    with pytest.raises(ValueError):
        forest.fit(x[:, :24], y, trees=2)                     # F = 24


# ---------------------------------------------------------------------------- 5. beside scikit-learn
def test_held_out_accuracy_beside_scikit_learn():
    """Same hyper-parameters (128 trees, sqrt, fully grown, bootstrap) on overlapping blobs: our accuracy on 20 000 held-out
    rows is within three binomial standard errors 3 sqrt(p (1 - p) / n) of scikit-learn's measured accuracy p."""
    ens = pytest.importorskip('sklearn.ensemble')
    xtr, ytr = fd.blobs(1500, 32, 4, 0.35, 1)
    xte, yte = fd.blobs(20000, 32, 4, 0.35, 2)
    t0 = time.time()
    m = forest.fit(xtr, ytr, trees=128, seed=0)
    t1 = time.time()
    clf = ens.RandomForestClassifier(128, random_state=0).fit(xtr, ytr)
    t2 = time.time()
    ours = float((fd.walk(as_dict(m), np.ascontiguousarray(xte.T))[1] == yte).mean())
    p = float(clf.score(xte, yte))
    margin = 3 * np.sqrt(p * (1 - p) / yte.size)
    print(f'held-out accuracy: ours {ours:.4f}, scikit-learn {p:.4f}, margin {margin:.4f}; fit time ours {t1 - t0:.2f} s '
          f'(model.fit_time {m.fit_time:.2f} s), scikit-learn {t2 - t1:.2f} s')
    assert abs(ours - p) <= margin


@functools.lru_cache(None)
def _probe_rows():
    """The recipe of the parity cases: 6 classes, F = 384, class means 0.08 N(0, 1), unit noise, 3000 train, 20 000 test."""
    return fd.blobs(3000, 384, 6, 0.08, 1) + fd.blobs(20000, 384, 6, 0.08, 2)


@pytest.mark.parametrize('trees,max_features', [(64, 'sqrt'), (16, None)])
def test_from_sklearn_fully_grown_equals_predict(trees, max_features):
    ens = pytest.importorskip('sklearn.ensemble')
    xtr, ytr, xte, _ = _probe_rows()
    clf = ens.RandomForestClassifier(trees, max_features=max_features, random_state=0, n_jobs=8).fit(xtr, ytr)
    pr = np.sort(clf.predict_proba(xte), axis=1)
    ties = int((pr[:, -1] - pr[:, -2] == 0).sum())
    m = forest.from_sklearn(clf)
    assert m.trees == trees and m.n_features == 384 and m.labels.tolist() == list(range(6))
    assert set(np.unique(m.value[m.feature < 0])) <= {0, 65535}          # fully grown: every leaf is pure
    labels = fd.walk(as_dict(m), np.ascontiguousarray(xte.T))[1]
    print(f'{trees} trees, max_features {max_features}: {m.n_nodes} nodes, depth {m.max_depth}, {ties} rows with tied top two')
    assert ties >= 100                                        # the tie rule is exercised
    assert np.array_equal(labels, clf.predict(xte))


def test_from_sklearn_with_impure_leaves():
    """max_depth = 8: the labels equal clf.predict wherever its top-two predict_proba margin exceeds 1 / 65535 + 1e-9; the rows
    below that margin may be at most 1 % of the test rows (measured with scikit-learn 1.7.2 and these seeds: 18 of 20 000 =
    0.09 %, and none of them labelled differently)."""
    ens = pytest.importorskip('sklearn.ensemble')
    xtr, ytr, xte, _ = _probe_rows()
    clf = ens.RandomForestClassifier(64, max_depth=8, random_state=0, n_jobs=8).fit(xtr, ytr)
    pr = np.sort(clf.predict_proba(xte), axis=1)
    clear = pr[:, -1] - pr[:, -2] > 1 / 65535 + 1e-9
    m = forest.from_sklearn(clf)
    assert m.max_depth == 8 and (m.value[m.feature < 0].max(1) < 65535).any()
    labels = fd.walk(as_dict(m), np.ascontiguousarray(xte.T))[1]
    print(f'{int((~clear).sum())} of {clear.size} rows below the margin, {int((labels != clf.predict(xte)).sum())} labels differ overall')
    assert (~clear).mean() <= 0.01
    assert np.array_equal(labels[clear], clf.predict(xte)[clear])


def golden_model(golden_dir):
    """(ForestModel, x_test fp16 [2000][32], predict int64 [2000]) of tests/golden/forest_sklearn.npz."""
    with np.load(os.path.join(golden_dir, 'forest_sklearn.npz'), allow_pickle=False) as z:
        trees = [tuple(z[f'{k}_{t}'] for k in ('children_left', 'children_right', 'feature', 'threshold', 'value'))
                 for t in range(int(z['n_trees']))]
        return forest.from_tree_arrays(trees, int(z['n_features']), labels=z['classes']), z['x_test'], z['predict']


def test_golden_sklearn_forest(golden_dir):
    m, x, want = golden_model(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, 'forest_sklearn.npz')) < 256 * 1024
    assert m.trees == 12 and m.n_features == 32 and m.classes == 4 and x.dtype == np.float16 and x.shape == (2000, 32)
    assert np.array_equal(m.labels[fd.walk(as_dict(m), np.ascontiguousarray(x.T))[1]], want)


def test_from_tree_arrays_reorders_nodes():
    """A tree whose children come BEFORE their parents (the root still first) is re-ordered, not refused."""
    fr = fd.stump(3, 0.5, [65535, 0], [0, 65535])
    m = forest.from_tree_arrays([(np.asarray([2, -1, 1, -1, -1]), np.asarray([4, -1, 3, -1, -1]), np.asarray([3, -2, 5, -2, -2]),
                                  np.asarray([0.5, -2.0, 0.25, -2.0, -2.0]), np.asarray([[2, 2], [3, 0], [3, 1], [0, 1], [0., 4]]))], 32)
    assert m.max_depth == 2 and m.feature.tolist() == [3, 5, -1, -1, -1] and m.left.tolist() == [1, 3, -1, -1, -1]
    assert m.value[:, 0].tolist() == [32768, 49151, 0, 65535, 0] and fr['value'][1, 0] == 65535


# ---------------------------------------------------------------------------- 6. files
def test_model_files_round_trip_and_refuse_each_other(tmp_path):
    x, y = _planted(240, 32, 3, 35)
    m = forest.fit(x, y * 2, trees=5, max_depth=4, seed=3, class_names=['bg', 'a', 'b'])
    forest.save_model(m, tmp_path / 'rf.npz')
    with np.load(tmp_path / 'rf.npz', allow_pickle=False) as z:          # plain arrays only
        assert set(z.files) == set(forest.ForestModel.ARRAYS)
        assert all(z[k].dtype != object for k in z.files)
    back = forest.load_model(tmp_path / 'rf.npz')
    for k in ('labels', 'tree_offset', 'feature', 'threshold', 'left', 'right', 'value'):
        assert getattr(back, k).tobytes() == getattr(m, k).tobytes() and getattr(back, k).dtype == getattr(m, k).dtype, k
    assert back.class_names == ['bg', 'a', 'b'] and back.labels.tolist() == [0, 2, 4] and back.max_depth == m.max_depth
    assert back.n_features == 32 and back.fit_time == m.fit_time > 0
    assert forest.is_forest_file(tmp_path / 'rf.npz')
    import svm_data
    xs, ts, gamma = svm_data.planted(32, 2, 10, 0)
    vt.svm.save_model(vt.svm.fit(xs, ts, gamma=gamma), tmp_path / 'svm.npz')
    assert not forest.is_forest_file(tmp_path / 'svm.npz')
    with pytest.raises(ValueError, match='SVM model file'):
        forest.load_model(tmp_path / 'svm.npz')
    with pytest.raises(ValueError, match='not an SVM model file'):
        vt.svm.load_model(tmp_path / 'rf.npz')
    np.save(tmp_path / 'a.npy', np.zeros(3))
    np.savez(tmp_path / 'other.npz', a=np.zeros(3))
    (tmp_path / 'junk.npz').write_bytes(b'PK\x03\x04 not a zip')
    for name in ('a.npy', 'other.npz', 'junk.npz'):
        with pytest.raises(ValueError):
            forest.load_model(tmp_path / name)
    arrays = dict(np.load(tmp_path / 'rf.npz'))
    arrays['left'] = arrays['left'].copy()
    arrays['left'][0] = 0                                     # a corrupt file: the root is its own child
    np.savez(tmp_path / 'corrupt.npz', **arrays)
    with pytest.raises(ValueError, match='not larger than its parent'):
        forest.load_model(tmp_path / 'corrupt.npz')


# ---------------------------------------------------------------------------- 7. the command line's refusals
@pytest.mark.parametrize('argv,flag', [(['--normalize'], 'normalize'), (['--trees', '0'], 'trees'), (['--trees', '5000'], 'trees'),
                                       (['--max-features', '0'], 'max-features'), (['--gamma', '0.5'], 'gamma'),
                                       (['--C', '1.0'], 'C'), (['--kernel', 'rbf'], 'kernel'), (['--tol', '0.001'], 'tol'),
                                       (['--max-depth', '65'], 'max-depth'), (['--min-samples-leaf', '0'], 'min-samples-leaf'),
                                       (['--max-features', 'log2'], 'max-features')])
def test_command_line_refuses_before_the_device(tmp_path, capsys, monkeypatch, argv, flag):
    import classify_features
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('the device was asked for'))
    with pytest.raises(SystemExit) as e:
        classify_features.main(['--data', str(tmp_path), '--classifier', 'forest'] + argv)
    assert e.value.code == 1
    assert f'Invalid argument for --{flag}' in capsys.readouterr().out


def test_command_line_model_file_decides_the_classifier(tmp_path, capsys):
    import classify_features
    x, y = _planted(240, 32, 3, 35)
    forest.save_model(forest.fit(x, y, trees=2, max_depth=2), tmp_path / 'rf.npz')
    with pytest.raises(SystemExit) as e:                     # the forest file against an explicit --classifier svm
        classify_features.main(['--data', str(tmp_path), '--classifier', 'svm', '--model', str(tmp_path / 'rf.npz')])
    assert e.value.code == 1 and 'does not hold a svm model' in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:                     # implied: the forest's refusal of --gamma shows which side ran
        classify_features.main(['--data', str(tmp_path), '--gamma', '1', '--model', str(tmp_path / 'rf.npz')])
    assert e.value.code == 1 and 'does not apply to --classifier forest' in capsys.readouterr().out
    assert classify_features.forest_tag(40.0, 'uniform', 256) == '40.0uniform_rf256'
    assert classify_features.forest_tag(0.0, 'annotated', 64, 12, 'all', False) == '0.0annotated_rf64_d12_all_nobg'
    assert classify_features.forest_tag(5.0, 'both', 8, None, 20) == '5.0both_rf8_mf20'
