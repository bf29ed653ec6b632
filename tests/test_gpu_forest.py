"""GPU: vittf_forest_decide against the numpy walk of tests/forest_data.py -- votes and labels exactly (integers), over every
tile width, ragged and unaligned voxel counts and tree counts around the tree groups; the edge semantics of the comparison,
the tie rule, the uint32 headroom; fitted and golden models through vt.forest.predict; classify_features.py --classifier forest
end to end.
"""
import itertools
import json
import os
import shutil

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import forest_data as fd

pytestmark = pytest.mark.gpu
forest = vt.forest
F_CYCLE = (32, 64, 96, 128, 160, 256, 288, 384, 512, 544, 768, 1024)      # both ends of every tile: 1024, 512, 256, 128, 64 voxels


def as_dict(m):
    return dict(tree_offset=m.tree_offset, feature=m.feature, threshold=m.threshold, left=m.left, right=m.right, value=m.value)


def as_model(fr, F):
    c = fr['value'].shape[1]
    return forest.ForestModel([str(i) for i in range(c)], np.arange(c), F, fr['tree_offset'], fr['feature'], fr['threshold'],
                              fr['left'], fr['right'], fr['value'])


def _run(gpu, model, x, want_votes=True):
    """(labels uint8 [nvox], votes uint32 [C][nvox] or None) as numpy, of one call on the fp16 volume x [F][nvox]."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    labels, votes = forest.decide(xd, model, want_votes)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), None if votes is None else votes.cpu().numpy()


def _check(gpu, fr, F, x, tag):
    model = as_model(fr, F)
    assert model.max_depth == fd.depth_of(fr)                 # the call gets the true depth: no slack
    want_votes, want_labels, ends = fd.walk(fr, x)
    labels, votes = _run(gpu, model, x)
    assert votes.dtype == np.uint32 and votes.shape == want_votes.shape and labels.dtype == np.uint8
    assert np.array_equal(votes.astype(np.uint64), want_votes), tag
    assert np.array_equal(labels, want_labels), tag
    assert np.array_equal(_run(gpu, model, x, want_votes=False)[0], labels), f'{tag}: votes = NULL changes the labels'
    return want_votes, want_labels, ends


# ---------------------------------------------------------------------------- 1. exact votes and labels
@pytest.mark.parametrize('trees', [1, 3, 64, 257])
def test_votes_and_labels_equal_the_numpy_walk(gpu, trees):
    """trees: fewer than the 2 .. 16 tree groups of a workgroup, fewer than 4 x the groups, a multiple, a remainder.  nvox 250 /
    257 / 805 / 256: an unaligned row, odd rows, a ragged tail, the aligned path; 2053 = 32 tiles of 64 voxels (2 of 1024) and
    5 more.  F cycles through both ends of every tile width; 3077 voxels = three tiles of the widest (1024 voxels, F <= 64) and
    5 more."""
    rng = np.random.default_rng(trees)
    for k, (classes, nvox) in enumerate(itertools.product((2, 3, 8), (250, 257, 805, 256, 2053))):
        F = F_CYCLE[(k + trees) % len(F_CYCLE)]
        x = rng.standard_normal((F, nvox)).astype(np.float16)
        fr = fd.random_forest(rng, trees, F, classes, depth=9, leaves=40)
        _check(gpu, fr, F, x, (trees, classes, nvox, F))
    for F in (32, 64):
        x = rng.standard_normal((F, 3077)).astype(np.float16)
        _check(gpu, fd.random_forest(rng, trees, F, 5, depth=9, leaves=40), F, x, (trees, 5, 3077, F))


# ---------------------------------------------------------------------------- 2. edge semantics
def test_edge_semantics_of_the_comparison(gpu):
    """Equality goes left; -0 and +0 are equal in both orders; negative thresholds; +inf always left, -inf never (finite x); a
    single-leaf tree; the depth-40 chain walked to its end; max_depth passed is the true depth.  Every case is asserted to
    occur in the data."""
    rng = np.random.default_rng(7)
    F, nvox, c = 32, 257, 3
    x = rng.standard_normal((F, nvox)).astype(np.float16)
    x[0, ::3] = np.float16(1.5)                               # equal to tree 0's threshold
    x[1, ::2], x[1, 1::2] = np.float16(-0.0), np.float16(0.0)
    x[2] = x[1]
    x[:, 5] = np.float16(100.0)                               # voxel 5 is above every threshold of the chain
    x[:, 6] = np.float16(-100.0)
    L, R = [65535, 0, 0], [0, 65535, 0]
    trees = [fd.stump(0, 1.5, L, R), fd.stump(1, 0.0, L, R), fd.stump(2, -0.0, L, R), fd.stump(3, -0.75, L, R),
             fd.stump(4, np.inf, L, R), fd.stump(5, -np.inf, L, R), fd.leaf_tree([1, 2, 3]), fd.chain_tree(rng, F, c, 40, first=8)]
    fr = fd.forest_of(trees)
    assert np.signbit(x[1, 0]) and not np.signbit(x[1, 1]) and np.signbit(fr['threshold'][fr['tree_offset'][2]])
    assert fd.depth_of(fr) == 40
    votes, labels, ends = _check(gpu, fr, F, x, 'edges')
    assert (x[0] == np.float16(1.5)).sum() >= 80 and (ends[0][x[0] == np.float16(1.5)] == 1).all()        # equal: left
    assert (ends[1][[0, 1, 2, 3]] == 1).all() and (ends[2][[0, 1, 2, 3]] == 1).all()                        # -0 <= +0 and +0 <= -0
    assert {1, 2} == set(ends[3]) and (x[3] < 0).any()                                                    # a negative threshold splits
    assert (ends[4] == 1).all() and (ends[5] == 2).all()                                                  # +inf: left, -inf: right
    assert (ends[6] == 0).all()
    assert ends[7][5] == 80 and ends[7][6] == 1 and len(set(ends[7])) > 5                                 # the chain, to its last leaf
    # each tree alone too: a forest whose only tree is the chain (depth 40 exactly), or the single leaf (depth 0)
    for t in (fd.chain_tree(rng, F, c, 40, first=8), fd.leaf_tree([9, 9, 1])):
        _check(gpu, fd.forest_of([t]), F, x, 'alone')


def test_walk_is_bounded_by_max_depth(gpu):
    """The entry stops after max_depth steps whatever the nodes say: with max_depth one short of the chain's depth the voxels
    that would have gone further cast no vote, the others vote as before (the host never sends such a call: validate()
    computes the depth itself)."""
    rng = np.random.default_rng(8)
    F, nvox = 32, 130
    x = rng.standard_normal((F, nvox)).astype(np.float16)
    x[:, 3] = np.float16(100.0)
    fr = fd.forest_of([fd.chain_tree(rng, F, 2, 6)])
    model = as_model(fr, F)
    want, _, ends = fd.walk(fr, x)
    model.max_depth = 5
    labels, votes = _run(gpu, model, x)
    cut = ends[0] >= 11                                       # the two deepest nodes: 6 steps away
    assert cut[3] and not cut.all()
    assert (votes[:, cut] == 0).all() and np.array_equal(votes[:, ~cut].astype(np.uint64), want[:, ~cut])
    assert (labels[cut] == 0).all()


# ---------------------------------------------------------------------------- 3. ties and range
def test_tie_rule_lowest_index_wins(gpu):
    x = np.random.default_rng(0).standard_normal((32, 70)).astype(np.float16)
    for rows, label in (([[5, 5, 1], [2, 2, 0]], 0),                   # two-way tie at the front
                        ([[1, 7, 3], [0, 0, 4]], 1),                   # two-way tie between the later classes
                        ([[4, 4, 4], [65535, 65535, 65535]], 0),       # three-way
                        ([[0, 0, 0, 0, 0, 0, 0, 0]], 0),               # all equal (zero)
                        ([[1, 2, 9, 9, 3, 9, 0, 9]], 2)):
        fr = fd.forest_of([fd.leaf_tree(r) for r in rows])
        votes, labels, _ = _check(gpu, fr, 32, x, rows)
        top = votes[:, 0] == votes[:, 0].max()
        assert top.sum() >= 2 and (labels == label).all() and int(np.flatnonzero(top)[0]) == label


def test_vote_range_4096_trees(gpu):
    """4096 single-leaf trees with 65535 for one class: the vote is 4096 x 65535 exactly."""
    x = np.zeros((32, 100), np.float16)
    fr = fd.forest_of([fd.leaf_tree([0, 65535])] * 4096)
    labels, votes = _run(gpu, as_model(fr, 32), x)
    assert (votes[1] == 4096 * 65535).all() and (votes[0] == 0).all() and (labels == 1).all()
    assert 4096 * 65535 == 268431360 < 2 ** 32


# ---------------------------------------------------------------------------- 4. fitted and golden models
@pytest.mark.parametrize('n,F', [(600, 32), (1500, 384)])
def test_fitted_model_predict(gpu, n, F):
    xtr, ytr = fd.blobs(n, F, 5, 0.5 if F == 32 else 0.15, seed=n)
    model = forest.fit(xtr, ytr, trees=32, seed=4)
    vol = fd.blobs(20 * 12 * 9, F, 5, 0.5 if F == 32 else 0.15, seed=n + 1)[0]
    feat = np.ascontiguousarray(vol.T).reshape(F, 20, 12, 9)
    want_votes, want_labels, _ = fd.walk(as_dict(model), feat.reshape(F, -1))
    idx, votes = forest.predict(feat, model, return_votes=True)
    assert idx.shape == (20, 12, 9) and idx.dtype == torch.uint8 and idx.is_cuda and votes.shape == (5, 20, 12, 9)
    assert np.array_equal(idx.cpu().numpy().reshape(-1), want_labels)
    assert np.array_equal(votes.cpu().numpy().reshape(5, -1).astype(np.uint64), want_votes)
    assert int(want_votes.sum(0).max()) <= 32 * 65535
    idx2, votes2 = forest.predict(torch.from_numpy(feat).to(gpu), model, return_votes=True)
    assert idx2.cpu().numpy().tobytes() == idx.cpu().numpy().tobytes() and votes2.cpu().numpy().tobytes() == votes.cpu().numpy().tobytes()
    assert np.array_equal(forest.predict(feat, model).cpu().numpy(), idx.cpu().numpy())
    with pytest.raises(ValueError):
        forest.predict(np.zeros((F + 32, 4, 4, 4), np.float16), model)


def test_golden_sklearn_forest(gpu, golden_dir):
    """The 2000 golden rows as a [32][2000] volume: the labels equal the stored clf.predict."""
    with np.load(os.path.join(golden_dir, 'forest_sklearn.npz'), allow_pickle=False) as z:
        trees = [tuple(z[f'{k}_{t}'] for k in ('children_left', 'children_right', 'feature', 'threshold', 'value'))
                 for t in range(int(z['n_trees']))]
        model = forest.from_tree_arrays(trees, int(z['n_features']), labels=z['classes'])
        x, want = z['x_test'], z['predict']
    labels, _ = _run(gpu, model, np.ascontiguousarray(x.T), want_votes=False)
    assert np.array_equal(model.labels[labels], want)


# ---------------------------------------------------------------------------- 5. the command line
def _planted_dir(d, seed=5):
    """A 16^3 x 96 directory with labels: background and two classes in slabs; the files as predict_ntf.py's contract has them
    (volume and labels are stored flipped on axis -3, the features belong to the flipped volume)."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((32, 32, 32), np.uint8)
    lab[10:22, 4:28, 4:16] = 1
    lab[10:22, 4:28, 16:28] = 2
    mu = 0.6 * np.random.default_rng(seed + 100).standard_normal((3, 96))
    feats = (mu[lab[::2, ::2, ::2]] + rng.standard_normal((16, 16, 16, 96))).astype(np.float16)
    d.mkdir()
    np.save(d / 'volume.npy', np.flip(lab.astype(np.float16), axis=-3))
    np.save(d / 'labels.npy', np.flip(lab, axis=-3))
    np.save(d / 'v_features.npy', np.ascontiguousarray(np.moveaxis(feats, -1, 0)))
    return lab


def _main(argv):
    import classify_features
    with pytest.raises(SystemExit) as e:
        classify_features.main(argv)
    return e.value.code


def test_command_line_end_to_end(gpu, tmp_path, capsys):
    lab = _planted_dir(tmp_path / 'a')
    a = tmp_path / 'a'
    args = ['--data', str(a), '--num-samples', '40', '--sampling-mode', 'uniform', '--classifier', 'forest', '--trees', '24', '--votes']
    assert _main(args) == 0
    assert 'do not apply to --classifier forest' in capsys.readouterr().out
    tag = '40.0uniform_rf24'
    pred = np.load(a / f'rf_pred{tag}.npy')
    assert pred.dtype == np.uint8 and pred.shape == (16, 16, 16) and set(np.unique(pred)) <= {0, 1, 2}
    model = forest.load_model(a / f'rf_model{tag}.npz')
    assert model.labels.tolist() == [0, 1, 2] and model.class_names == ['background', 'ntf1', 'ntf2'] and model.trees == 24
    metrics = json.load(open(a / f'rf_metrics{tag}.json'))
    assert {'mAcc', 'mIoU', 'mF1', 'iou', 'confusion_matrix', 'fit_time', 'predict_time', 'n_trees', 'n_nodes', 'max_depth'} <= set(metrics)
    assert 'n_sv' not in metrics and (metrics['n_trees'], metrics['n_nodes'], metrics['max_depth']) == (24, model.n_nodes, model.max_depth)
    print(f"classify_features.py --classifier forest on the planted directory: mIoU {metrics['mIoU']:.3f}, mAcc {metrics['mAcc']:.3f}")
    assert metrics['mIoU'] > 0.5 and (pred == lab[::2, ::2, ::2]).mean() > 0.9
    # rf_votes: the formula over the votes of vt.forest.predict, in the order of the model's classes
    feats = np.load(a / 'v_features.npy')
    idx, votes = forest.predict(feats, model, return_votes=True)
    assert np.array_equal(model.labels[idx.cpu().numpy()], pred)
    conf = np.load(a / f'rf_votes{tag}.npy')
    assert conf.dtype == np.uint8 and conf.shape == (3, 16, 16, 16)
    assert np.array_equal(conf, (votes.cpu().numpy().astype(np.int64) * 255 // (24 * 65535)).astype(np.uint8))
    assert conf.max() > 200
    # a second run exits early; --overwrite gives the same bytes
    before = {p.name: p.read_bytes() for p in a.glob('rf_*.npy')}
    assert len(before) == 2
    assert _main(args) == 0
    assert 'Already inferred RF preds' in capsys.readouterr().out
    assert _main(args + ['--overwrite']) == 0
    assert {p.name: p.read_bytes() for p in a.glob('rf_*.npy')} == before
    again = forest.load_model(a / f'rf_model{tag}.npz')
    for name in ('tree_offset', 'feature', 'threshold', 'left', 'right', 'value'):
        assert getattr(again, name).tobytes() == getattr(model, name).tobytes(), name
    # --model on a copy of the directory reproduces the prediction; the classifier is implied by the file
    (tmp_path / 'c').mkdir()
    for fn in ('volume.npy', 'labels.npy', 'v_features.npy'):
        shutil.copy(a / fn, tmp_path / 'c' / fn)
    assert _main(['--data', str(tmp_path / 'c'), '--model', str(a / f'rf_model{tag}.npz')]) == 0
    assert np.array_equal(np.load(tmp_path / 'c' / 'rf_pred0.0annotated_rf24.npy'), pred)
    assert not (tmp_path / 'c' / 'rf_model0.0annotated_rf24.npz').exists()
    # the other flags reach the fit and the tag
    assert _main(['--data', str(tmp_path / 'c'), '--num-samples', '40', '--sampling-mode', 'uniform', '--classifier', 'forest',
                  '--trees', '8', '--max-depth', '3', '--max-features', 'all', '--no-bootstrap', '--background', 'none']) == 0
    small = forest.load_model(tmp_path / 'c' / 'rf_model40.0uniform_rf8_d3_all_nobg.npz')
    assert small.trees == 8 and small.max_depth <= 3 and small.labels.tolist() == [1, 2]
    assert set(np.unique(np.load(tmp_path / 'c' / 'rf_pred40.0uniform_rf8_d3_all_nobg.npy'))) <= {1, 2}
    # the default classifier in the same directory still writes the SVM's files under the SVM's tag
    assert _main(['--data', str(a), '--num-samples', '40', '--sampling-mode', 'uniform']) == 0
    svm_pred = np.load(a / 'svm_pred40.0uniform_rbf.npy')
    assert svm_pred.dtype == np.uint8 and svm_pred.shape == (16, 16, 16)
    assert (a / 'svm_model40.0uniform_rbf.npz').exists() and (a / 'svm_metrics40.0uniform_rbf.json').exists()
    assert vt.load_model(a / 'svm_model40.0uniform_rbf.npz').kernel == 'rbf'
