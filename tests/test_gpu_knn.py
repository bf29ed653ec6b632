"""GPU: vittf_knn_decide (through vt.knn.decide) against the fp64 oracle of tests/knn_data.py -- exact cases (every similarity an
integer: labels, scores, neighbours and similarities equal bit for bit, ties included), real-valued banks (every similarity,
neighbour set and score within its worst-case bound, the labels the arg-max of the call's own scores and the oracle's on
every clear voxel), vt.knn.predict and classify_features.py --classifier knn end to end.
"""
import itertools
import json
import shutil

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import knn_data
import svm_data

pytestmark = pytest.mark.gpu
knn = vt.knn


def _run(gpu, model, x, vn=None, scores=True, neighbours=True):
    """(labels, scores, nn_index, nn_sim) as numpy (None where not asked for), of one call on the fp16 volume x [F][nvox]."""
    xd = torch.from_numpy(np.array(x)).to(gpu)                # (a copy: the shared cases are read-only)
    out = knn.decide(xd, model, None if vn is None else torch.as_tensor(vn).to(gpu), want_scores=scores, want_neighbours=neighbours)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


# ---------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('n_bank', [1, 31, 32, 33, 200])
def test_exact_cases_bit_for_bit(gpu, n_bank):
    """Integer features and an integer bank with copied rows, no norms, uniform weights: every similarity is an exact integer
    and ties are frequent, so labels, scores, nn_index and nn_sim equal the oracle exactly.  n_bank 1 / 31 / 32 / 33 / 200:
    one lane half empty, a padded chunk, a full one, the ring's turn, several turns; nvox 250 / 257 / 805 / 256: an unaligned
    row, odd rows, a ragged tail, the aligned path; k = 1, 5 and min(32, n_bank) (k = n_bank included): each list capacity."""
    cross_half_ties = score_ties = 0
    for i, (classes, nvox) in enumerate(itertools.product((2, 3, 8), (250, 257, 805, 256))):
        F = (32, 96, 384, 768)[(i + n_bank + i // 4) % 4]
        bank, cls, x = knn_data.int_case(n_bank, nvox, F, classes, seed=1000 * n_bank + i)
        sim = knn_data.similarities(bank, x)
        assert np.array_equal(sim, np.rint(sim)) and np.abs(sim).max() < 2 ** 24
        for k in sorted({1, min(5, n_bank), min(32, n_bank)}):
            model = knn_data.model_of(bank, cls, classes, k, 'uniform')
            want_labels, want_scores, want_idx, want_sim = knn_data.oracle(bank, cls, classes, k, x, weights='uniform', sim=sim)
            labels, scores, idx, nsim = _run(gpu, model, x)
            tag = (n_bank, classes, nvox, F, k)
            assert np.array_equal(nsim.astype(np.float64), want_sim), tag
            assert np.array_equal(idx, want_idx), tag
            assert np.array_equal(scores.astype(np.float64), want_scores), tag
            assert np.array_equal(labels, want_labels), tag
            assert _run(gpu, model, x, scores=False, neighbours=False)[0].tobytes() == labels.tobytes(), tag
            # did the data exercise the two tie rules?  equal similarities at the edge of the list in different lane halves ...
            if k < n_bank:
                nxt = np.take_along_axis(sim, np.argsort(-sim, axis=0, kind='stable')[k:k + 1], 0)[0]
                edge = (sim == want_sim[-1][None, :]) & (want_sim[-1] == nxt)[None, :]
                halves = knn_data.half_of(np.arange(n_bank))[:, None]
                cross_half_ties += int(((edge & (halves == 0)).any(0) & (edge & (halves == 1)).any(0)).sum())
            # ... and equal best class scores
            top = np.sort(want_scores, axis=0)
            score_ties += int((top[-1] == top[-2]).sum())
    print(f'n_bank = {n_bank}: {cross_half_ties} voxel runs with a tie across the lane halves at the k-th rank, {score_ties} with equal best scores')
    if n_bank >= 31:
        assert cross_half_ties >= 100 and score_ties >= 100    # (these generators give over a thousand of each)


# ---------------------------------------------------------------------------- 2. and 3. real-valued banks
def _check_real(gpu, bank, cls, classes, x, tag):
    xd = torch.from_numpy(np.array(x)).to(gpu)
    vn = vt.similarity.voxel_norms(xd.reshape(x.shape[0], -1, 1, 1)).reshape(-1).cpu().numpy()
    assert np.allclose(vn, svm_data.host_norms(x), rtol=1e-6)
    sim = knn_data.similarities(bank, x, vn)                   # the oracle and the kernel are given the same norms
    bnd = knn_data.sim_bound(bank, x, vn)
    bmax = bnd.max(0)
    order = np.sort(sim, axis=0)[::-1]
    for k in knn_data.REAL_KS:
        for weights, T in knn_data.REAL_WEIGHTS:
            model = knn_data.model_of(bank, cls, classes, k, weights, T)
            labels, scores, idx, nsim = _run(gpu, model, x, vn)
            what = f'{tag} k = {k} {weights} T = {T}'
            # every similarity within its bound of the fp64 similarity of the sample it names
            assert idx.min() >= 0 and idx.max() < bank.shape[0], what
            true = np.take_along_axis(sim, idx.astype(np.int64), 0)
            err = np.take_along_axis(bnd, idx.astype(np.int64), 0)
            ratio = (np.abs(nsim.astype(np.float64) - true) / err).max()
            assert ratio <= 1.0, f'{what}: a similarity is off by {ratio:.2f} bounds'
            # distinct, and in the kernel's own order: larger similarity first, then the lower index
            assert (np.diff(np.sort(idx, axis=0), axis=0) > 0).all(), what
            assert ((nsim[:-1] > nsim[1:]) | ((nsim[:-1] == nsim[1:]) & (idx[:-1] < idx[1:]))).all(), what
            # the set: nothing returned lies below the fp64 k-th largest by more than the two bounds, nothing above it by more
            # than the two bounds is missing (the second bound: the largest of the voxel, whichever sample it belongs to)
            kth = order[k - 1]
            assert (true >= kth[None, :] - err - bmax[None, :]).all(), what
            present = np.zeros(sim.shape, bool)
            np.put_along_axis(present, idx.astype(np.int64), True, 0)
            assert not (~present & (sim > kth[None, :] + bnd + bmax[None, :])).any(), what
            # the scores: the formula in fp64 on the call's own neighbours
            ncls = cls[idx]
            want = knn_data.scores_of(nsim, ncls, classes, weights, T)
            sb = knn_data.score_bound(nsim, ncls, classes, weights, T)
            serr = np.abs(scores.astype(np.float64) - want)
            assert (serr <= sb).all(), f'{what}: a score is off by {(serr / np.maximum(sb, 1e-300)).max():.2f} bounds'
            assert np.array_equal(labels, np.argmax(scores, 0)), f'{what}: the labels are not the arg-max of the scores written'
            # the labels against the oracle on every clear voxel; the share left out is capped
            out, want_labels = knn_data.unclear(bank, cls, classes, k, x, vn, weights, T, sim=sim, bnd=bnd)
            print(f'{what}: S = {bank.shape[0]}, sim error / bound {ratio:.3f}, score error {serr.max():.2e}, unclear {100 * out.mean():.2f} %, '
                  f'labels differing from the oracle {int((labels != want_labels).sum())}')
            assert out.mean() <= knn_data.MAX_UNCLEAR, what
            assert np.array_equal(labels[~out], want_labels[~out]), what
            # optional outputs and a second call
            assert _run(gpu, model, x, vn, scores=False, neighbours=False)[0].tobytes() == labels.tobytes(), f'{what}: NULL outputs change the labels'
            assert _run(gpu, model, x, vn, scores=True, neighbours=False)[1].tobytes() == scores.tobytes(), what
            again = _run(gpu, model, x, vn)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (labels, scores, idx, nsim))), f'{what}: a second call gives other bytes'


@pytest.mark.parametrize('case', knn_data.REAL_CASES)
def test_real_valued_banks_within_the_bounds(gpu, case):
    bank, cls, x = knn_data.real_case(*case)
    _check_real(gpu, bank, cls, case[1], x, f'{case}')
    if case == knn_data.NORM_CASE:                             # the aligned load path: 800 voxels in 16-byte aligned rows
        _check_real(gpu, bank, cls, case[1], np.ascontiguousarray(x[:, :800]), f'{case} aligned')


# ---------------------------------------------------------------------------- 4. predict and the command line
def _planted_dir(d, seed=5):
    """tests/test_gpu_svm.py's 16^3 x 96 directory with labels: background and two classes in slabs; the files as
    predict_ntf.py's contract has them (volume and labels are stored flipped on axis -3)."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((32, 32, 32), np.uint8)
    lab[10:22, 4:28, 4:16] = 1
    lab[10:22, 4:28, 16:28] = 2
    mu = svm_data.centres(96, 3, seed)
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


ACCURACY_MARGIN = 0.005


def test_predict_and_the_command_line_end_to_end(gpu, tmp_path, capsys):
    """The planted directory: --classifier knn writes its files; --probs; --model FILE on a second directory reproduces
    vt.knn.predict byte for byte; the accuracy on the planted slabs is at least that of the SVM run (--normalize, the same
    samples: the same seed draws them) minus ACCURACY_MARGIN.  Measured on the first run: k-NN 0.9995 (2 of 4096 voxels
    wrong), SVM 0.9978 (9 wrong): the k-NN is ahead, and the margin of 0.005 (20 voxels) is about twice the SVM's own error
    count -- what a different draw of the 40 samples per class could move either figure by."""
    lab = _planted_dir(tmp_path / 'a')
    truth = lab[::2, ::2, ::2]
    args = ['--data', str(tmp_path / 'a'), '--num-samples', '40', '--sampling-mode', 'uniform']
    assert _main(args + ['--classifier', 'knn', '--probs', '--normalize']) == 0           # --normalize: accepted, changes nothing
    tag = '40.0uniform_knn20'
    pred = np.load(tmp_path / 'a' / f'knn_pred{tag}.npy')
    assert pred.dtype == np.uint8 and pred.shape == (16, 16, 16) and set(np.unique(pred)) <= {0, 1, 2}
    model = vt.load_model(tmp_path / 'a' / f'knn_model{tag}.npz')
    assert isinstance(model, vt.KnnModel) and model.labels.tolist() == [0, 1, 2] and model.class_names == ['background', 'ntf1', 'ntf2']
    assert (model.k, model.temperature, model.weights, model.n_features) == (20, 0.07, 'softmax', 96)
    metrics = json.load(open(tmp_path / 'a' / f'knn_metrics{tag}.json'))
    assert {'mAcc', 'mIoU', 'mF1', 'iou', 'confusion_matrix', 'fit_time', 'predict_time', 'n_bank', 'k', 'temperature', 'weights'} <= set(metrics)
    assert 'n_sv' not in metrics and (metrics['n_bank'], metrics['k'], metrics['temperature'], metrics['weights']) == (model.n_bank, 20, 0.07, 'softmax')
    probs = np.load(tmp_path / 'a' / f'knn_probs{tag}.npy')
    assert probs.dtype == np.uint8 and probs.shape == (3, 16, 16, 16)
    assert (np.abs(probs.astype(np.int64).sum(0) - 255) <= 3).all()
    assert np.array_equal(np.argmax(probs, 0)[probs.max(0) > 128], np.searchsorted(model.labels, pred)[probs.max(0) > 128])
    # vt.knn.predict: the same volume, its scores and their arg-max
    feats = np.load(tmp_path / 'a' / 'v_features.npy')
    idx, scores = knn.predict(feats, model, return_scores=True)
    assert idx.shape == (16, 16, 16) and idx.dtype == torch.uint8 and idx.is_cuda and scores.shape == (3, 16, 16, 16)
    assert np.array_equal(model.labels[idx.cpu().numpy()], pred)
    assert np.array_equal(scores.reshape(3, -1).argmax(0).cpu().numpy(), idx.reshape(-1).cpu().numpy())
    assert np.array_equal(knn.probabilities(scores).cpu().numpy(), probs)
    # a second run exits early; --model on a second directory reproduces the prediction and writes no model; the tags
    capsys.readouterr()
    assert _main(args + ['--classifier', 'knn']) == 0
    assert 'Already inferred KNN preds' in capsys.readouterr().out
    (tmp_path / 'b').mkdir()
    for fn in ('volume.npy', 'labels.npy', 'v_features.npy'):
        shutil.copy(tmp_path / 'a' / fn, tmp_path / 'b' / fn)
    assert _main(['--data', str(tmp_path / 'b'), '--model', str(tmp_path / 'a' / f'knn_model{tag}.npz')]) == 0
    again = np.load(tmp_path / 'b' / 'knn_pred0.0annotated_knn20.npy')
    assert again.tobytes() == model.labels[knn.predict(feats, model).cpu().numpy()].tobytes() == pred.tobytes()
    assert not (tmp_path / 'b' / 'knn_model0.0annotated_knn20.npz').exists()
    assert _main(args + ['--classifier', 'knn', '--k', '1', '--temperature', '1', '--knn-weights', 'uniform', '--background', 'none']) == 0
    one = np.load(tmp_path / 'a' / 'knn_pred40.0uniform_knn1_t1_uni_nobg.npy')
    assert set(np.unique(one)) <= {1, 2} and vt.load_model(tmp_path / 'a' / 'knn_model40.0uniform_knn1_t1_uni_nobg.npz').k == 1
    # the SVM on the same samples, in the same geometry
    assert _main(args + ['--normalize']) == 0
    svm_pred = np.load(tmp_path / 'a' / 'svm_pred40.0uniform_rbf_norm.npy')
    acc, svm_acc = float((pred == truth).mean()), float((svm_pred == truth).mean())
    print(f'planted directory: k-NN accuracy {acc:.4f} (mIoU {metrics["mIoU"]:.3f}), SVM accuracy {svm_acc:.4f}, bank {model.n_bank}')
    assert acc >= svm_acc - ACCURACY_MARGIN
