"""CPU: vt.knn's host side -- the model checks and refusals, files, fit, the command line's tags and refused flags -- and the
oracle and the conditions of tests/knn_data.py that the GPU tests rely on.  Nothing here touches a device.
"""
import numpy as np
import pytest

import vit_tf_amd as vt
from vit_tf_amd import _lib
import knn_data
import svm_data

knn = vt.knn


def _model(s=40, f=32, classes=3, k=5, temperature=0.07, weights='softmax', seed=0):
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((s, f)).astype(np.float16)
    cls = np.sort(rng.integers(0, classes, size=s))
    return knn.KnnModel(bank, cls, k, temperature, weights, [f'c{i}' for i in range(classes)], np.arange(classes))


def test_the_binding_lists_the_entries():
    lib = _lib.load()
    for name in ('vittf_knn_workspace_bytes', 'vittf_knn_decide'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.KNN_MAX_K, _lib.KNN_MAX_CLASSES, _lib.KNN_MAX_BANK) == (32, 8, 65536)
    # ceil(n_bank / 32) images of 32 rows of 2 FP + 16 bytes and 32 words; 0 for a refused shape
    assert lib.vittf_knn_workspace_bytes(32, 1) == 64 * 32 + 640
    assert lib.vittf_knn_workspace_bytes(96, 33) == 2 * (64 * 128 + 640)
    assert lib.vittf_knn_workspace_bytes(384, 4096) == 128 * (64 * 384 + 640)
    assert lib.vittf_knn_workspace_bytes(768, 65536) == 2048 * (64 * 768 + 640)
    for f, s in ((48, 10), (0, 10), (800, 10), (1024, 10), (32, 0), (32, 65537)):
        assert lib.vittf_knn_workspace_bytes(f, s) == 0, (f, s)


def test_the_c_entry_checks_its_arguments_before_any_launch():
    """Every refusal returns before the first launch, so host buffers stand in for device memory here."""
    import ctypes as C
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    base = (C.addressof(buf) + 15) & ~15

    def call(f=32, nvox=100, n_bank=40, classes=3, k=5, inv_t=1.0, feat=base, bank=base, cls=base, norm=None, labels=base,
             scores=None, idx=None, sim=None, ws=base, ws_bytes=1 << 15):
        return lib.vittf_knn_decide(feat, f, nvox, bank, cls, n_bank, classes, k, inv_t, norm, labels, scores, idx, sim, ws, ws_bytes, None)
    INVALID, WORKSPACE = -1, -2
    need = lib.vittf_knn_workspace_bytes(32, 40)
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    for bad in (dict(f=48), dict(f=800), dict(f=0), dict(nvox=0), dict(n_bank=0), dict(n_bank=65537), dict(classes=1), dict(classes=9),
                dict(k=0), dict(k=33), dict(k=41), dict(n_bank=4, k=5), dict(inv_t=-1.0), dict(inv_t=float('inf')),
                dict(inv_t=float('nan')), dict(feat=None), dict(bank=None), dict(cls=None), dict(labels=None),
                dict(ws=None), dict(feat=base + 1), dict(bank=base + 1), dict(norm=base + 2), dict(scores=base + 2), dict(idx=base + 1),
                dict(sim=base + 2), dict(ws=base + 8)):
        assert call(**bad) == INVALID, bad


def test_model_checks_and_refusals():
    m = _model()
    assert (m.classes, m.n_features, m.n_bank, m.k) == (3, 32, 40, 5) and m.normalize
    assert m.inv_temperature == float(np.float32(1 / 0.07)) and _model(weights='uniform').inv_temperature == 0.0
    with pytest.raises(ValueError, match='more than the 20 samples'):
        _model(s=20, k=21)
    with pytest.raises(ValueError, match=r'k must be in 1\.\.32'):
        _model(k=33)
    with pytest.raises(ValueError, match=r'k must be in 1\.\.32'):
        _model(k=0)
    with pytest.raises(ValueError, match='bank_class'):
        knn.KnnModel(m.bank, np.full(40, 3), 5, 0.07, 'softmax', m.class_names, m.labels)            # class out of range
    with pytest.raises(ValueError, match='bank_class'):
        knn.KnnModel(m.bank, m.bank_class[::-1], 5, 0.07, 'softmax', m.class_names, m.labels)        # not ascending
    with pytest.raises(ValueError, match='multiple of 32'):
        _model(f=48)
    with pytest.raises(ValueError, match='multiple of 32'):
        _model(f=800)
    for t in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            _model(temperature=t)
    with pytest.raises(ValueError, match='temperature'):
        _model(temperature=1e-39)                                                                      # log2(e) / T leaves fp32
    with pytest.raises(ValueError, match='weights'):
        _model(weights='gauss')
    with pytest.raises(ValueError, match='classes'):
        knn.KnnModel(m.bank, np.zeros(40), 5, 0.07, 'softmax', ['a'], [0])
    with pytest.raises(ValueError, match='classes'):
        knn.KnnModel(m.bank, np.zeros(40), 5, 0.07, 'softmax', [str(i) for i in range(9)], np.arange(9))
    with pytest.raises(ValueError, match='finite'):
        knn.KnnModel(np.full((4, 32), np.inf), np.zeros(4), 1, 0.07, 'softmax', ['a', 'b'], [0, 1])
    with pytest.raises(ValueError, match='labels ascending'):
        knn.KnnModel(m.bank, m.bank_class, 5, 0.07, 'softmax', m.class_names, [2, 1, 0])
    knn.KnnModel(m.bank[:1], [0], 1, 0.07, 'uniform', ['a', 'b'], [0, 7])                            # one sample, k = S = 1


def test_fit_normalises_rounds_once_and_sorts_by_class(capsys):
    xs, t, _ = svm_data.planted(96, 3, 20, seed=3)
    rng = np.random.default_rng(0)
    perm = rng.permutation(t.size)
    values = np.asarray([5, 0, 9])[t]                                     # label values, not indices
    a = knn.fit(xs[perm], values[perm], class_names=['bg', 'five', 'nine'])
    b = knn.fit(xs[perm], values[perm], class_names=['bg', 'five', 'nine'])
    for name in ('bank', 'bank_class', 'labels'):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert (a.k, a.temperature, a.weights) == (20, 0.07, 'softmax') and a.labels.tolist() == [0, 5, 9]
    assert a.bank.dtype == np.float16 and a.bank_class.dtype == np.uint8 and np.all(np.diff(a.bank_class.astype(int)) >= 0)
    order = np.argsort(values[perm], kind='stable')
    x64 = xs[perm][order].astype(np.float64)
    want = (x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))).astype(np.float16)
    assert a.bank.tobytes() == want.tobytes()                             # fp64 normalisation, one rounding, sample order kept
    assert np.array_equal(a.bank_class, np.searchsorted([0, 5, 9], values[perm][order]))
    assert capsys.readouterr().out == ''
    c = knn.fit(xs[:6], t[:6] + np.arange(6) % 2, k=20)                   # k is clipped to S, with a note
    assert c.k == 6 and 'using k = 6' in capsys.readouterr().out
    with pytest.raises(ValueError, match='targets'):
        knn.fit(xs, t[:-1])
    with pytest.raises(ValueError, match='class names'):
        knn.fit(xs, t, class_names=['a'])
    with pytest.raises(ValueError, match='classes'):
        knn.fit(xs, np.zeros_like(t))


def test_save_and_load_round_trip(tmp_path):
    m = _model(s=33, f=96, classes=4, k=7, temperature=0.5, weights='uniform', seed=4)
    knn.save_model(m, tmp_path / 'm.npz')
    assert knn.is_knn_file(tmp_path / 'm.npz')
    with np.load(tmp_path / 'm.npz', allow_pickle=False) as z:
        assert set(z.files) == set(knn.KnnModel.ARRAYS) and str(z['format'][()]) == 'vittf-knn-1'
    for back in (knn.load_model(tmp_path / 'm.npz'), vt.load_model(tmp_path / 'm.npz')):
        assert isinstance(back, vt.KnnModel)
        for name in ('bank', 'bank_class', 'labels'):
            assert getattr(back, name).tobytes() == getattr(m, name).tobytes() and getattr(back, name).dtype == getattr(m, name).dtype
        assert (back.k, back.temperature, back.weights, back.class_names) == (m.k, m.temperature, m.weights, m.class_names)
    knn.save_model(back, tmp_path / 'again.npz')
    with np.load(tmp_path / 'm.npz') as z0, np.load(tmp_path / 'again.npz') as z1:
        for key in z0.files:
            assert z0[key].tobytes() == z1[key].tobytes() and z0[key].dtype == z1[key].dtype, key
    # other files are refused, and vt.load_model still reads an SVM model
    np.savez(tmp_path / 'other.npz', a=np.zeros(3))
    np.save(tmp_path / 'plain.npy', np.zeros(3))
    (tmp_path / 'junk.npz').write_bytes(b'not a zip file')
    for name in ('other.npz', 'plain.npy', 'junk.npz'):
        assert not knn.is_knn_file(tmp_path / name)
        with pytest.raises(ValueError):
            knn.load_model(tmp_path / name)
    with np.load(tmp_path / 'm.npz') as z:
        arrays = {k: z[k] for k in z.files}
    np.savez(tmp_path / 'wide.npz', **{**arrays, 'bank': arrays['bank'].astype(np.float32)})
    np.savez(tmp_path / 'short.npz', **{k: v for k, v in arrays.items() if k != 'k'})
    for name in ('wide.npz', 'short.npz'):
        with pytest.raises(ValueError):
            knn.load_model(tmp_path / name)
    xs, t, gamma = svm_data.planted(32, 2, 8, seed=1)
    vt.save_model(vt.svm.fit(xs, t, gamma=gamma), tmp_path / 'svm.npz')
    assert isinstance(vt.load_model(tmp_path / 'svm.npz'), vt.SvmModel) and not knn.is_knn_file(tmp_path / 'svm.npz')


def test_tags_and_paths(tmp_path):
    import classify_features as cf
    assert cf.knn_tag(200.0, 'both') == '200.0both_knn20'
    assert cf.knn_tag(0.0, 'annotated', 5, 0.07, 'softmax', False) == '0.0annotated_knn5_nobg'
    assert cf.knn_tag(40.0, 'uniform', 1, 1.0, 'uniform') == '40.0uniform_knn1_t1_uni'
    assert cf.knn_tag(40.0, 'surface', 32, 0.5) == '40.0surface_knn32_t0.5'
    names = [p.name for p in cf.knn_paths(tmp_path, '200.0both_knn20')]
    assert names == ['knn_pred200.0both_knn20.npy', 'knn_model200.0both_knn20.npz', 'knn_metrics200.0both_knn20.json',
                     'knn_probs200.0both_knn20.npy']
    assert all(p.parent == tmp_path for p in cf.knn_paths(tmp_path, 'x'))
    # the other classifiers' names are what they were
    assert cf.svm_tag(200.0, 'both', 'rbf') == '200.0both_rbf' and cf.forest_tag(200.0, 'both', 256) == '200.0both_rf256'
    assert cf.mlp_tag(200.0, 'both') == '200.0both_mlp'


@pytest.mark.parametrize('flags', [['--kernel', 'rbf'], ['--C', '2'], ['--gamma', 'scale'], ['--tol', '1e-3'], ['--votes'],
                                   ['--features', 'handcrafted'], ['--features', 'intensity'], ['--k', '0'], ['--k', '33'],
                                   ['--temperature', '0'], ['--temperature', '-1'], ['--temperature', 'nan']])
def test_refused_flags_exit_1_before_any_device_use(tmp_path, capsys, monkeypatch, flags):
    import classify_features as cf

    def no_device(*a, **k):
        raise AssertionError('the device was asked for')
    monkeypatch.setattr(_lib, 'require_device', no_device)
    with pytest.raises(SystemExit) as e:
        cf.main(['--data', str(tmp_path), '--classifier', 'knn', '--num-samples', '10'] + flags)
    assert e.value.code == 1
    assert f'Invalid argument for --{flags[0][2:]}' in capsys.readouterr().out


def test_a_model_file_of_another_classifier_is_refused(tmp_path, capsys):
    import classify_features as cf
    knn.save_model(_model(), tmp_path / 'bank.npz')
    for kind in ('svm', 'forest', 'mlp'):
        with pytest.raises(SystemExit) as e:
            cf.main(['--data', str(tmp_path), '--classifier', kind, '--model', str(tmp_path / 'bank.npz')])
        assert e.value.code == 1 and 'Invalid argument for --model' in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------- the oracle and its conditions
def test_oracle_orders_ties_by_index_and_breaks_score_ties_low():
    bank = np.zeros((6, 32), np.float16)
    bank[:, 0] = [1, 2, 2, 1, 2, 0]
    cls = np.asarray([0, 0, 1, 1, 2, 2], np.uint8)
    x = np.zeros((32, 2), np.float16)
    x[0] = [1, -1]
    labels, scores, idx, sim = knn_data.oracle(bank, cls, 3, 4, x, weights='uniform')
    assert idx[:, 0].tolist() == [1, 2, 4, 0] and sim[:, 0].tolist() == [2, 2, 2, 1]
    assert idx[:, 1].tolist() == [5, 0, 3, 1] and scores[:, 0].tolist() == [2, 1, 1] and labels.tolist() == [0, 0]
    labels, scores, _, _ = knn_data.oracle(bank, cls, 3, 3, x, weights='uniform')
    assert scores[:, 0].tolist() == [1, 1, 1] and labels[0] == 0                       # a three-way tie: the lowest class
    labels, scores, _, _ = knn_data.oracle(bank, cls, 3, 4, x, weights='softmax', temperature=0.5)
    assert np.allclose(scores[:, 0], [1 + np.exp(-2.0), 1, 1]) and np.allclose(scores[:, 1], [np.exp(-2.0) + np.exp(-4.0), np.exp(-2.0), 1])


def test_oracle_agrees_with_scikit_learn_without_ties():
    neighbors = pytest.importorskip('sklearn.neighbors')
    F, classes, per_class, nvox = 96, 3, 40, 805
    bank, cls, x = knn_data.real_case(F, classes, per_class, nvox)
    # scikit-learn's cosine metric divides by the norm of the bank rows too: give both sides rows of unit norm in fp64 (the
    # oracle takes any arrays), so that the two orders can differ only where similarities agree to ~1e-16
    bank = bank.astype(np.float64)
    bank = bank / np.sqrt((bank * bank).sum(1, keepdims=True))
    vn = np.sqrt((x.astype(np.float64) ** 2).sum(0))
    for k in (1, 5, 20):
        labels, scores, idx, sim = knn_data.oracle(bank, cls, classes, k, x, vn, weights='uniform')
        clf = neighbors.KNeighborsClassifier(n_neighbors=k, metric='cosine', algorithm='brute', weights='uniform')
        clf.fit(bank, cls)
        got_idx = clf.kneighbors(x.astype(np.float64).T, return_distance=False)
        full = knn_data.similarities(bank, x, vn)
        kth = np.sort(full, axis=0)[::-1][:k + 1]
        untied = np.all(np.diff(kth, axis=0) < -1e-9, axis=0)                          # no ties among the k + 1 nearest
        assert untied.mean() > 0.95
        assert np.array_equal(got_idx.T[:, untied], idx[:, untied])
        clear = untied & ((np.sort(scores, axis=0)[-1] - np.sort(scores, axis=0)[-2]) > 0)     # sklearn breaks vote ties its own way
        assert np.array_equal(clf.predict(x.astype(np.float64).T)[clear], labels[clear])


@pytest.mark.parametrize('case', knn_data.REAL_CASES)
def test_the_share_of_unclear_voxels_is_capped_on_every_gpu_case(case):
    """The condition of tests/test_gpu_knn.py's label check, for the oracle alone (host norms)."""
    F, classes, per_class, nvox = case
    bank, cls, x = knn_data.real_case(*case)
    vn = svm_data.host_norms(x)
    sim, bnd = knn_data.similarities(bank, x, vn), knn_data.sim_bound(bank, x, vn)
    for k in knn_data.REAL_KS:
        for weights, T in knn_data.REAL_WEIGHTS:
            out, _ = knn_data.unclear(bank, cls, classes, k, x, vn, weights, T, sim=sim, bnd=bnd)
            print(f'{case} k = {k} {weights} T = {T}: {100 * out.mean():.2f} % unclear')
            assert out.mean() <= knn_data.MAX_UNCLEAR, (case, k, weights, T, out.mean())


def test_the_exact_cases_hold_exact_integers_and_ties():
    for n_bank in (1, 31, 32, 33, 200):
        bank, cls, x = knn_data.int_case(n_bank, 257, 768, 8, seed=n_bank)
        sim = knn_data.similarities(bank, x)
        assert np.array_equal(sim, np.rint(sim)) and np.abs(sim).max() < 2 ** 24 and np.abs(bank).max() <= 3 and np.abs(x).max() <= 8
        assert np.all(np.diff(cls.astype(int)) >= 0) and cls.max() < 8
        if n_bank >= 31:
            same = (sim[:, None, 0] == sim[None, :, 0]) & (knn_data.half_of(np.arange(n_bank))[:, None] != knn_data.half_of(np.arange(n_bank))[None, :])
            assert same.any()
