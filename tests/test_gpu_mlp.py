"""GPU: vittf_mlp_decide against the fp64 oracle of tests/mlp_data.py -- exact cases (every layer an integer: logits equal bit
for bit), fitted real-valued heads (every logit within its worst-case bound, the labels the arg-max wherever the margin
exceeds the bounds, the uint8 probabilities against the softmax of the call's own logits), the range-safe hand-over,
vt.mlp.predict and classify_features.py --classifier mlp end to end.
"""
import itertools
import json
import shutil

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import mlp_data

pytestmark = pytest.mark.gpu
mlp = vt.mlp


def _run(gpu, model, x, vn=None, want_logits=True, want_probs=False):
    """(labels, logits or None, probs or None) as numpy, of one call on the fp16 volume x [F][nvox]."""
    xd = torch.from_numpy(np.array(x, order='C')).to(gpu)
    labels, z, p = mlp.decide(xd, model, None if vn is None else torch.from_numpy(np.array(vn)).to(gpu), want_logits, want_probs)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), None if z is None else z.cpu().numpy(), None if p is None else p.cpu().numpy()


# ---------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('head', mlp_data.HEADS, ids=str)
@pytest.mark.parametrize('F', mlp_data.FS)
def test_exact_cases(gpu, F, head):
    """Integer features, sparse integer weights and biases: every layer is an integer far below 2^24 (test_mlp_cpu.py checks
    the cases), so the logits equal the oracle bit for bit and the labels its arg-max, with and without want_logits.  nvox
    250 / 257 / 805 / 256: an unaligned row, odd rows, a ragged tail, the aligned path; classes 2, 3, 8: one or both lane halves."""
    rng = np.random.default_rng(1000 * F + 7 * sum(head) + len(head))
    for classes, nvox in itertools.product(mlp_data.CLASSES, mlp_data.NVOX):
        model = mlp_data.int_model(rng, F, head, classes)
        x = mlp_data.int_voxels(rng, F, nvox)
        want = mlp_data.logits(model, x)
        labels, z, _ = _run(gpu, model, x)
        assert np.array_equal(z.astype(np.float64), want), (classes, nvox)
        assert np.array_equal(labels, mlp_data.argmax(want)), (classes, nvox)
        assert np.array_equal(_run(gpu, model, x, want_logits=False)[0], labels), (classes, nvox)


@pytest.mark.parametrize('head', [(), (64,), (96, 32)], ids=str)
def test_ties_take_the_lowest_index(gpu, head):
    """A duplicated output row and an all-zero last layer: equal logits give the lowest index; both kinds occur."""
    rng = np.random.default_rng(5)
    tied_top = zero = 0
    for classes, nvox in itertools.product((2, 3, 8), (257, 256)):
        x = mlp_data.int_voxels(rng, 96, nvox)
        model = mlp_data.int_model(rng, 96, head, classes, tie='rows')
        want = mlp_data.logits(model, x)
        labels, z, _ = _run(gpu, model, x)
        assert np.array_equal(z.astype(np.float64), want) and np.array_equal(z[0], z[1])
        assert np.array_equal(labels, mlp_data.argmax(want))
        top = want.max(0) == want[0]
        assert (labels[top] == 0).all() and not (labels == 1).any()
        tied_top += int(top.sum())
        model = mlp_data.int_model(rng, 96, head, classes, tie='zero')
        labels, z, p = _run(gpu, model, x, want_probs=True)
        assert not z.any() and not labels.any()
        assert (p == int(np.floor(255.0 / classes + 0.5))).all()
        zero += nvox
    assert tied_top > 0 and zero > 0


# ---------------------------------------------------------------------------- 2. real cases
def _check_real(gpu, index, normalize):
    model, x, vn, want, b = mlp_data.real_case(index, normalize)
    labels, z, p = _run(gpu, model, x, vn, want_probs=True)
    err = np.abs(z.astype(np.float64) - want)
    print(f'case {mlp_data.REAL_CASES[index]} norm={normalize}: max |logit error| {err.max():.3e}, max error / bound '
          f'{(err / b).max():.3f}, largest bound {b.max():.3e}')
    assert (err <= b).all()
    clear = ~mlp_data.ambiguous(want, b)
    assert np.array_equal(labels[clear], mlp_data.argmax(want)[clear])
    assert np.array_equal(labels, mlp_data.argmax(z))                      # the arg-max of the call's own logits everywhere
    soft = mlp_data.softmax255(z)
    perr = np.abs(p.astype(np.float64) - soft)
    print(f'    max |probs - 255 softmax| {perr.max():.6f} (allowed {0.5 + mlp_data.PROB_EPS:.6f})')
    assert (perr <= 0.5 + mlp_data.PROB_EPS).all()
    l2, z2, p2 = _run(gpu, model, x, vn, want_probs=True)
    assert l2.tobytes() == labels.tobytes() and z2.tobytes() == z.tobytes() and p2.tobytes() == p.tobytes()
    assert np.array_equal(_run(gpu, model, x, vn, want_logits=False)[0], labels)


@pytest.mark.parametrize('index', range(len(mlp_data.REAL_CASES)))
def test_real_cases(gpu, index):
    """Fitted heads: every logit within its bound, the labels the oracle's wherever the voxel is not ambiguous, the uint8
    probabilities within 0.5 + PROB_EPS of 255 softmax of the call's own logits; a second call gives the same bytes."""
    _check_real(gpu, index, False)


def test_real_case_with_voxel_norm(gpu):
    _check_real(gpu, mlp_data.NORM_CASE, True)


# ---------------------------------------------------------------------------- 3. the range rule
@pytest.mark.parametrize('head', [(32,), (256, 256)], ids=str)
@pytest.mark.parametrize('power', [-40, 14, 40])
def test_hand_over_is_range_safe(gpu, head, power):
    """The hand-over scales every voxel's activations by its own power of two, so hidden activations far outside the fp16
    range (2^40 times the integer case's, far beyond 65504) or far below it (2^-40) change nothing: with the first layer
    scaled by 2^power the logits are exactly 2^power times the oracle's integers (the last bias scaled alike)."""
    rng = np.random.default_rng(11)
    base = mlp_data.int_model(rng, 96, head, 3)
    x = mlp_data.int_voxels(rng, 96, 805)
    k = np.float32(2.0 ** power)
    weights = [base.weights[0] * k] + base.weights[1:]
    biases = [base.biases[0] * k] + base.biases[1:-1] + [base.biases[-1] * k]
    if len(head) == 2:
        biases[1] = base.biases[1] * k
    model = mlp.MlpModel(base.class_names, base.labels, 96, False, head, weights, biases)
    hidden = mlp_data.layer_values(model, x)[0].max()
    assert hidden > 2.0 ** 17 if power > 0 else hidden < 2.0 ** -30
    want = mlp_data.logits(model, x)
    labels, z, _ = _run(gpu, model, x)
    assert np.array_equal(z.astype(np.float64), want)
    assert np.array_equal(labels, mlp_data.argmax(want))


def test_unsafe_head_is_refused_before_any_launch():
    with pytest.raises(ValueError, match='2\\^100'):
        rng = np.random.default_rng(0)
        base = mlp_data.int_model(rng, 96, (32,), 3)
        mlp.MlpModel(base.class_names, base.labels, 96, False, (32,), [base.weights[0] * np.float32(2.0 ** 90), base.weights[1]], base.biases)


# ---------------------------------------------------------------------------- 4. predict on a volume
def test_predict_on_a_volume(gpu):
    model, x, _, want, b = mlp_data.real_case(1)
    vol = torch.from_numpy(np.ascontiguousarray(x[:, :792])).reshape(96, 8, 9, 11)
    labels, probs = mlp.predict(vol.to(gpu), model, return_probs=True)
    assert labels.shape == (8, 9, 11) and labels.dtype == torch.uint8 and probs.shape == (3, 8, 9, 11) and probs.dtype == torch.uint8
    flat, _, p = _run(gpu, model, x[:, :792], want_probs=True)
    assert np.array_equal(labels.cpu().numpy().reshape(-1), flat) and np.array_equal(probs.cpu().numpy().reshape(3, -1), p)
    assert np.array_equal(mlp.predict(vol.to(gpu), model).cpu().numpy(), labels.cpu().numpy())
    # a model that asks for normalised voxels gets the norms of vt.similarity.voxel_norms
    nmodel, _, _, _, _ = mlp_data.real_case(mlp_data.NORM_CASE, True)
    got = mlp.predict(vol.to(gpu), nmodel).cpu().numpy().reshape(-1)
    vn = vt.similarity.voxel_norms(vol.to(gpu).reshape(96, -1, 1, 1))
    assert np.array_equal(got, _run(gpu, nmodel, x[:, :792], vn.cpu().numpy(), want_logits=False)[0])


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
    a = tmp_path / 'a'
    lab = _planted_dir(a)
    args = ['--data', str(a), '--num-samples', '40', '--sampling-mode', 'uniform', '--classifier', 'mlp', '--hidden', '32', '--probs']
    assert _main(args) == 0
    capsys.readouterr()
    tag = '40.0uniform_mlp32'
    pred = np.load(a / f'mlp_pred{tag}.npy')
    assert pred.dtype == np.uint8 and pred.shape == (16, 16, 16) and set(np.unique(pred)) <= {0, 1, 2}
    model = mlp.load_model(a / f'mlp_model{tag}.npz')
    assert model.labels.tolist() == [0, 1, 2] and model.class_names == ['background', 'ntf1', 'ntf2'] and model.hidden == (32,)
    assert not model.normalize and model.n_features == 96 and model.loss_history.size == 100
    metrics = json.load(open(a / f'mlp_metrics{tag}.json'))
    assert {'mAcc', 'mIoU', 'mF1', 'iou', 'confusion_matrix', 'fit_time', 'predict_time', 'n_params', 'hidden', 'final_loss',
            'train_accuracy'} <= set(metrics)
    assert 'n_sv' not in metrics and metrics['hidden'] == [32] and metrics['n_params'] == 97 * 32 + 33 * 3 == model.n_params
    assert metrics['final_loss'] == model.final_loss and metrics['train_accuracy'] == model.train_accuracy
    print(f"classify_features.py --classifier mlp --hidden 32 on the planted directory: mIoU {metrics['mIoU']:.3f}, "
          f"mAcc {metrics['mAcc']:.3f}, training accuracy {model.train_accuracy:.3f}")
    assert metrics['mIoU'] > 0.5 and (pred == lab[::2, ::2, ::2]).mean() > 0.9
    # labels against the oracle wherever the margin exceeds the bounds; mlp_probs: the softmax of the call's logits
    feats = np.load(a / 'v_features.npy')
    x = feats.reshape(96, -1)
    want, b = mlp_data.logits(model, x), mlp_data.bound(model, x)
    clear = ~mlp_data.ambiguous(want, b)
    assert clear.mean() >= 0.99
    assert np.array_equal(pred.reshape(-1)[clear], model.labels[mlp_data.argmax(want)][clear])
    conf = np.load(a / f'mlp_probs{tag}.npy')
    assert conf.dtype == np.uint8 and conf.shape == (3, 16, 16, 16)
    _, z, p = _run(gpu, model, x, want_probs=True)
    assert np.array_equal(conf.reshape(3, -1), p)
    assert (np.abs(p.astype(np.float64) - mlp_data.softmax255(z)) <= 0.5 + mlp_data.PROB_EPS).all() and conf.max() > 200
    # a second run exits early; --overwrite gives the same bytes
    before = {q.name: q.read_bytes() for q in a.glob('mlp_*.npy')}
    assert len(before) == 2
    assert _main(args) == 0
    assert 'Already inferred MLP preds' in capsys.readouterr().out
    assert _main(args + ['--overwrite']) == 0
    assert {q.name: q.read_bytes() for q in a.glob('mlp_*.npy')} == before
    again = mlp.load_model(a / f'mlp_model{tag}.npz')
    assert all(s.tobytes() == t.tobytes() for s, t in zip(again.weights + again.biases, model.weights + model.biases))
    # --model on a second volume: the classifier is implied by the file, nothing is fitted or saved
    c = tmp_path / 'c'
    lab_c = _planted_dir(c, seed=6)
    assert _main(['--data', str(c), '--model', str(a / f'mlp_model{tag}.npz'), '--probs']) == 0
    pred_c = np.load(c / 'mlp_pred0.0annotated_mlp32.npy')
    idx = mlp.predict(np.load(c / 'v_features.npy'), model).cpu().numpy()
    assert np.array_equal(model.labels[idx], pred_c) and pred_c.shape == lab_c[::2, ::2, ::2].shape
    assert (c / 'mlp_probs0.0annotated_mlp32.npy').exists() and not (c / 'mlp_model0.0annotated_mlp32.npz').exists()
    # the linear probe with normalised voxels and no background: the flags reach the fit and the tag
    assert _main(['--data', str(c), '--num-samples', '40', '--sampling-mode', 'uniform', '--classifier', 'mlp', '--normalize',
                  '--background', 'none', '--epochs', '5', '--lr', '0.01', '--batch', '32', '--weight-decay', '0']) == 0
    probe = mlp.load_model(c / 'mlp_model40.0uniform_mlp_norm_nobg.npz')
    assert probe.hidden == () and probe.normalize and probe.labels.tolist() == [1, 2] and probe.loss_history.size == 5
    assert set(np.unique(np.load(c / 'mlp_pred40.0uniform_mlp_norm_nobg.npy'))) <= {1, 2}
    assert not (c / 'mlp_probs40.0uniform_mlp_norm_nobg.npy').exists()
    shutil.rmtree(c)


def test_command_line_handcrafted_equals_one_decide_call(gpu, tmp_path):
    """--features handcrafted --classifier mlp streams the volume slab by slab: byte for byte what ONE decide call on the
    composed matrix gives, the labels and the probabilities."""
    import voxel_features_data as vd
    vf = vt.voxel_features
    volume, lab = vd.boxes_volume(seed=2)
    a = tmp_path / 'a'
    a.mkdir()
    np.save(a / 'volume.npy', np.flip(volume, axis=-3))
    np.save(a / 'labels.npy', np.flip(lab, axis=-3))
    assert _main(['--data', str(a), '--num-samples', '40', '--features', 'handcrafted', '--classifier', 'mlp', '--hidden', '32', '--probs']) == 0
    tag = '40.0both_hand_mlp32'
    pred, conf = np.load(a / f'mlp_pred{tag}.npy'), np.load(a / f'mlp_probs{tag}.npy')
    model = mlp.load_model(a / f'mlp_model{tag}.npz')
    assert model.n_features == 32 and pred.shape == volume.shape and conf.shape == (3,) + volume.shape
    vol = torch.from_numpy(volume).to(gpu)
    labels, _, probs = mlp.decide(vf.compose(vol, vf.stats(vol)), model, None, False, True)
    assert model.labels[labels.cpu().numpy()].tobytes() == pred.tobytes()
    assert probs.cpu().numpy().tobytes() == conf.tobytes()
    for slab in (4104, 1 << 24):                              # several slabs or one: the same bytes
        got, p = vf.classify(vol, model, slab_voxels=slab, want_votes=True)
        assert got.cpu().numpy().tobytes() == labels.cpu().numpy().tobytes() and p.cpu().numpy().tobytes() == conf.tobytes()
        assert vf.classify(vol, model, slab_voxels=slab).cpu().numpy().tobytes() == labels.cpu().numpy().tobytes()
    print(f'--features handcrafted --classifier mlp --hidden 32: accuracy on the two boxes {(pred == lab).mean():.3f}')
