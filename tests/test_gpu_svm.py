"""GPU: vittf_svm_rbf_decide / vittf_svm_linear_decide against the fp64 oracle of tests/svm_data.py -- exact cases (every
decision an integer: equality bit for bit), real-valued planted models (every decision within its worst-case bound, the labels
the vote over the call's own decisions), vt.svm.predict and classify_features.py end to end.
"""
import itertools
import json
import shutil

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import svm_data
from pca_data import planted_int

pytestmark = pytest.mark.gpu
svm = vt.svm


def _run(gpu, model, x, vn=None, want_decision=True):
    """(labels uint8 [nvox], decisions fp32 [P][nvox] or None) as numpy, of one call on the fp16 volume x [F][nvox]."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    labels, dec = svm.decide(xd, model, None if vn is None else torch.as_tensor(vn).to(gpu), want_decision)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), None if dec is None else dec.cpu().numpy()


def _int_model(rng, kernel, F, classes, n_sv, w=None):
    P = classes * (classes - 1) // 2
    names = [str(i) for i in range(classes)]
    if kernel == 'linear':
        return svm.SvmModel('linear', 0.0, 1.0, False, names, np.arange(classes), np.zeros((1, F), np.float16), [0],
                            np.zeros((P, 1), np.float32), rng.integers(-4, 5, size=P), w=w)
    sv = rng.standard_normal((n_sv, F)).astype(np.float16)
    return svm.SvmModel('rbf', 0.0, 1.0, False, names, np.arange(classes), sv, np.sort(rng.integers(0, classes, size=n_sv)),
                        rng.integers(-3, 4, size=(P, n_sv)), rng.integers(-4, 5, size=P))


# ---------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('n_sv', [1, 31, 32, 33, 200])
def test_rbf_exact_cases_with_gamma_zero(gpu, n_sv):
    """gamma = 0: every kernel value is exactly 1, small integer coefficients and intercepts make every decision an exact
    integer: labels and decisions equal the oracle bit for bit.  n_sv pads the last chunk / turns the ring; 1, 3 and 28 pairs
    fill one or both lane halves; nvox 250 / 257 / 805 / 256: an unaligned row, odd rows, a ragged tail, the aligned path."""
    rng = np.random.default_rng(n_sv)
    zeros = ties = 0
    for k, (classes, nvox) in enumerate(itertools.product((2, 3, 8), (250, 257, 805, 256))):
        F = (32, 96, 384, 768)[(k + n_sv) % 4]
        x = rng.standard_normal((F, nvox)).astype(np.float16)
        model = _int_model(rng, 'rbf', F, classes, n_sv)
        if k % 2:                                             # a decision of exactly 0 votes for the second class
            model.intercept[0] = -model.pair_coef[0].sum()
        want = svm_data.oracle(model, x)
        assert np.array_equal(want, np.rint(want)) and np.abs(want).max() < 2 ** 20
        labels, dec = _run(gpu, model, x)
        assert np.array_equal(dec.astype(np.float64), want), (classes, nvox, F)
        assert np.array_equal(labels, svm.vote(want, classes)), (classes, nvox, F)
        assert np.array_equal(_run(gpu, model, x, want_decision=False)[0], labels)
        zeros += int((want[:, 0] == 0).any())
        votes = np.zeros(classes, int)
        for p, (i, j) in enumerate(svm.pair_list(classes)):
            votes[i if want[p, 0] > 0 else j] += 1
        ties += int((votes == votes.max()).sum() > 1)
    assert zeros >= 6 and ties >= 1                           # both rules were exercised by these models


def test_rbf_exact_vote_rules(gpu):
    """Crafted decisions: a three-way tie (the lowest index wins), all zeros (every pair votes for its second class), a tie
    between two later classes."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((32, 257)).astype(np.float16)
    for classes, decisions, label in ((3, [1, -1, 1], 0), (8, [0] * 28, 7), (4, [-1, -1, 1, 1, -1, -1], 1), (4, [-1, -1, -1, 0, 1, 1], 2),
                                      (3, [-2, -3, 0], 2)):
        model = _int_model(rng, 'rbf', 32, classes, 5)
        model.intercept[:] = np.asarray(decisions) - model.pair_coef.sum(1)
        want = svm_data.oracle(model, x)
        assert np.array_equal(want[:, 0], decisions) and svm.vote(want, classes)[0] == label
        labels, dec = _run(gpu, model, x)
        assert np.array_equal(dec.astype(np.float64), want) and (labels == label).all(), (classes, decisions)


@pytest.mark.parametrize('F', [32, 384, 1024])
def test_linear_exact_cases(gpu, F):
    """Integer features (|x| <= 8) and integer w (|w| <= 3): every decision is an integer below 2^24, exact in fp32."""
    rng = np.random.default_rng(F)
    zeros = 0
    for classes, nvox in itertools.product((2, 3, 8), (250, 257, 805, 256)):
        x = planted_int(F, nvox, seed=nvox + classes)
        P = classes * (classes - 1) // 2
        model = _int_model(rng, 'linear', F, classes, 1, w=rng.integers(-3, 4, size=(P, F)))
        model.intercept[0] = -(model.w[0].astype(np.float64) @ x[:, 0])            # voxel 0: a decision of exactly 0
        want = model.w.astype(np.float64) @ x + model.intercept.astype(np.float64)[:, None]
        assert want[0, 0] == 0 and np.abs(want).max() < 2 ** 24
        labels, dec = _run(gpu, model, x.astype(np.float16))
        assert np.array_equal(dec.astype(np.float64), want), (classes, nvox)
        assert np.array_equal(labels, svm.vote(want, classes)), (classes, nvox)
        assert np.array_equal(_run(gpu, model, x.astype(np.float16), want_decision=False)[0], labels)
        zeros += int((want == 0).sum())
    assert zeros >= 12


# ---------------------------------------------------------------------------- 2. real-valued models
def _check_real(gpu, model, x, vn, tag):
    want = svm_data.oracle(model, x, vn)
    bnd = svm_data.bound(model, x, vn)
    labels, dec = _run(gpu, model, x, vn)
    err = np.abs(dec.astype(np.float64) - want)
    print(f'{tag}: S = {model.sv.shape[0]}, max error {err.max():.3e}, max error / bound {(err / bnd).max():.3f}, '
          f'ambiguous {100 * svm_data.ambiguous(want, bnd).mean():.2f} %')
    assert (err <= bnd).all(), f'{tag}: a decision is off by {(err / bnd).max():.2f} bounds'
    assert np.array_equal(labels, svm.vote(dec, model.classes)), 'the labels are not the vote over the decisions written'
    clear = ~svm_data.ambiguous(want, bnd)
    assert np.array_equal(labels[clear], svm.vote(want, model.classes)[clear])
    assert np.array_equal(_run(gpu, model, x, vn, want_decision=False)[0], labels), 'decision = NULL changes the labels'
    labels2, dec2 = _run(gpu, model, x, vn)
    assert labels2.tobytes() == labels.tobytes() and dec2.tobytes() == dec.tobytes(), 'a second call gives other bytes'


@pytest.mark.parametrize('kernel', svm.KERNELS)
@pytest.mark.parametrize('case', svm_data.REAL_CASES)
def test_real_valued_models_within_the_bound(gpu, case, kernel):
    model, x, _ = svm_data.real_case(*case, kernel=kernel)
    _check_real(gpu, model, x, None, f'{case} {kernel}')
    if case == svm_data.NORM_CASE:
        # the aligned load path (800 voxels in 16-byte aligned rows), and the same volume divided by its voxel norms
        _check_real(gpu, model, np.ascontiguousarray(x[:, :800]), None, f'{case} {kernel} aligned')
        model, x, _ = svm_data.real_case(*case, kernel=kernel, normalize=True)
        xd = torch.from_numpy(x).to(gpu)
        vn = vt.similarity.voxel_norms(xd.reshape(x.shape[0], -1, 1, 1)).reshape(-1).cpu().numpy()
        assert np.allclose(vn, svm_data.host_norms(x), rtol=1e-6)
        _check_real(gpu, model, x, vn, f'{case} {kernel} voxel_norm')


# ---------------------------------------------------------------------------- 3. predict and the command line
def _planted_dir(d, seed=5):
    """A 16^3 x 96 directory with labels: background and two classes in slabs; the files as predict_ntf.py's contract has them
    (volume and labels are stored flipped on axis -3, the features belong to the flipped volume)."""
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


def test_predict_and_the_command_line_end_to_end(gpu, tmp_path, capsys):
    lab = _planted_dir(tmp_path / 'a')
    args = ['--data', str(tmp_path / 'a'), '--num-samples', '40', '--sampling-mode', 'uniform']
    assert _main(args) == 0
    tag = '40.0uniform_rbf'
    pred = np.load(tmp_path / 'a' / f'svm_pred{tag}.npy')
    assert pred.dtype == np.uint8 and pred.shape == (16, 16, 16) and set(np.unique(pred)) <= {0, 1, 2}
    model = vt.load_model(tmp_path / 'a' / f'svm_model{tag}.npz')
    assert model.labels.tolist() == [0, 1, 2] and model.class_names == ['background', 'ntf1', 'ntf2'] and model.kernel == 'rbf'
    metrics = json.load(open(tmp_path / 'a' / f'svm_metrics{tag}.json'))
    assert {'mAcc', 'mIoU', 'mF1', 'iou', 'confusion_matrix', 'fit_time', 'predict_time', 'n_sv'} <= set(metrics)
    assert metrics['n_sv'] == model.sv.shape[0]
    print(f"classify_features.py on the planted directory: mIoU {metrics['mIoU']:.3f}, mAcc {metrics['mAcc']:.3f}, n_sv {metrics['n_sv']}")
    assert metrics['mIoU'] > 0.5                              # three classes: chance is about 0.2
    assert (pred == lab[::2, ::2, ::2]).mean() > 0.9
    # vt.svm.predict: the same volume, its decisions and their vote
    feats = np.load(tmp_path / 'a' / 'v_features.npy')
    idx, dec = svm.predict(feats, model, return_decision=True)
    assert idx.shape == (16, 16, 16) and idx.dtype == torch.uint8 and idx.is_cuda and dec.shape == (3, 16, 16, 16)
    assert np.array_equal(model.labels[idx.cpu().numpy()], pred)
    assert np.array_equal(svm.vote(dec.reshape(3, -1).cpu().numpy(), 3), idx.reshape(-1).cpu().numpy())
    # a second run exits early; the same flags in a fresh copy give the same bytes; --model reproduces the prediction
    capsys.readouterr()
    assert _main(args) == 0
    assert 'Already inferred SVM preds' in capsys.readouterr().out
    for name in ('b', 'c'):
        (tmp_path / name).mkdir()
        for fn in ('volume.npy', 'labels.npy', 'v_features.npy'):
            shutil.copy(tmp_path / 'a' / fn, tmp_path / name / fn)
    assert _main(['--data', str(tmp_path / 'b'), '--num-samples', '40', '--sampling-mode', 'uniform']) == 0
    assert (tmp_path / 'b' / f'svm_pred{tag}.npy').read_bytes() == (tmp_path / 'a' / f'svm_pred{tag}.npy').read_bytes()
    again = vt.load_model(tmp_path / 'b' / f'svm_model{tag}.npz')              # (an .npz carries time stamps: compare the arrays)
    for name in ('sv', 'pair_coef', 'intercept', 'sv_class', 'n_iter'):
        assert getattr(again, name).tobytes() == getattr(model, name).tobytes(), name
    assert _main(['--data', str(tmp_path / 'c'), '--model', str(tmp_path / 'a' / f'svm_model{tag}.npz')]) == 0
    assert np.array_equal(np.load(tmp_path / 'c' / 'svm_pred0.0annotated_rbf.npy'), pred)
    assert not (tmp_path / 'c' / 'svm_model0.0annotated_rbf.npz').exists()
    # the linear kernel, the background drawn from the border shell (all background in this volume), normalised voxels
    assert _main(['--data', str(tmp_path / 'c'), '--num-samples', '40', '--sampling-mode', 'uniform', '--kernel', 'linear',
                  '--background', 'border', '--normalize']) == 0
    lin = np.load(tmp_path / 'c' / 'svm_pred40.0uniform_linear_norm.npy')
    assert vt.load_model(tmp_path / 'c' / 'svm_model40.0uniform_linear_norm.npz').normalize
    assert (lin == lab[::2, ::2, ::2]).mean() > 0.9
