"""CPU: support-vector classification -- the C-ABI surface of vittf_svm_rbf_decide / vittf_svm_linear_decide (declared,
exported, argument checks without a launch), the fp64 solver of vit_tf_amd.svm on planted data and against scikit-learn,
from_libsvm, the model files, every refusal of classify_features.py, and the condition the GPU label test rests on.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import svm_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_svm_rbf_workspace_bytes', 'vittf_svm_rbf_decide', 'vittf_svm_linear_decide')
svm = vt.svm


# ---------------------------------------------------------------------------- 1. ABI surface
def _rbf(lib, f=384, nvox=1000, n_sv=100, classes=3, gamma=0.5, feat=1, sv=1, coef=1, intercept=1, labels=1, ws=1,
         ws_bytes=1 << 40, addr=0x1000, vn=None, dec=None):
    """vittf_svm_rbf_decide on placeholder addresses: only calls the argument checks refuse are made with it."""
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_svm_rbf_decide(p(feat), f, nvox, p(sv), p(coef), p(intercept), n_sv, classes, gamma, vn, p(labels), dec,
                                    p(ws), ws_bytes, None)


def _lin(lib, f=384, nvox=1000, classes=3, feat=1, w=1, intercept=1, labels=1, addr=0x1000, vn=None, dec=None):
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_svm_linear_decide(p(feat), f, nvox, p(w), p(intercept), classes, vn, p(labels), dec, None)


def test_svm_entries_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    assert int(re.search(r'#define\s+VITTF_SVM_MAX_CLASSES\s+(\d+)', header).group(1)) == 8 == _lib.SVM_MAX_CLASSES
    assert int(re.search(r'#define\s+VITTF_SVM_MAX_SV\s+(\d+)', header).group(1)) == 65536 == _lib.SVM_MAX_SV
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    for f in (0, 16, 48, 800, 1024, 1056):                    # the RBF entry stops at 768
        assert _rbf(lib, f=f) == INVALID, f
        assert lib.vittf_svm_rbf_workspace_bytes(f, 100, 3) == 0
    for f in (0, 16, 48, 1056):
        assert _lin(lib, f=f) == INVALID, f
    for c in (0, 1, 9):
        assert _rbf(lib, classes=c) == INVALID and _lin(lib, classes=c) == INVALID, c
        assert lib.vittf_svm_rbf_workspace_bytes(384, 100, c) == 0
    for n_sv in (0, -1, 65537):
        assert _rbf(lib, n_sv=n_sv) == INVALID, n_sv
        assert lib.vittf_svm_rbf_workspace_bytes(384, n_sv, 3) == 0
    assert _rbf(lib, nvox=0) == INVALID and _lin(lib, nvox=0) == INVALID
    for gamma in (-1.0, float('nan'), float('inf')):
        assert _rbf(lib, gamma=gamma) == INVALID, gamma
    for missing in ('feat', 'sv', 'coef', 'intercept', 'labels', 'ws'):
        assert _rbf(lib, **{missing: 0}) == INVALID, missing
    for missing in ('feat', 'w', 'intercept', 'labels'):
        assert _lin(lib, **{missing: 0}) == INVALID, missing
    assert _rbf(lib, addr=0x1001) == INVALID and _lin(lib, addr=0x1001) == INVALID       # feat and sv hold 2-byte values
    assert _rbf(lib, addr=0x1002) == INVALID and _lin(lib, addr=0x1002) == INVALID       # the fp32 arrays
    assert _rbf(lib, addr=0x1004) == INVALID                                             # ws: 16 bytes
    for bad in (dict(vn=C.c_void_p(0x1002)), dict(dec=C.c_void_p(0x1002))):              # a misaligned optional array alone
        assert _rbf(lib, **bad) == INVALID and _lin(lib, **bad) == INVALID
    assert _rbf(lib, ws_bytes=0) == WORKSPACE
    last = 0
    for f, n_sv, c, fp in ((32, 1, 2, 32), (64, 33, 3, 128), (384, 1024, 6, 384), (384, 4096, 6, 384), (768, 65536, 8, 768)):
        need = lib.vittf_svm_rbf_workspace_bytes(f, n_sv, c)
        assert need == 256 + -(-n_sv // 32) * (64 * fp + 5760) and need > last         # one image per 32 support vectors
        assert _rbf(lib, f=f, n_sv=n_sv, classes=c, ws_bytes=need - 1) == WORKSPACE
        last = need
    assert lib.vittf_svm_rbf_workspace_bytes(384, 33, 3) > lib.vittf_svm_rbf_workspace_bytes(384, 32, 3)


def test_python_entries_refuse_bad_shapes_before_the_device():
    x, t, _ = svm_data.planted(32, 2, 10, 0)
    with pytest.raises(ValueError):
        svm.fit(x, np.zeros(20, np.int64))                    # one class
    with pytest.raises(ValueError):
        svm.fit(x, np.arange(20))                             # 20 classes
    with pytest.raises(ValueError):
        svm.fit(x[:, :24], t)                                 # F = 24
    with pytest.raises(ValueError):
        svm.fit(x, t, kernel='poly')
    with pytest.raises(ValueError):
        svm.fit(np.zeros((2 * 4097, 32), np.float16), np.repeat([0, 1], 4097))        # more than 4096 samples of a class


# ---------------------------------------------------------------------------- 2. the solver on planted data
@pytest.mark.parametrize('kernel', svm.KERNELS)
@pytest.mark.parametrize('F,classes,per', [(32, 2, 40), (96, 3, 40), (96, 8, 40)])
def test_solver_reaches_the_kkt_conditions(F, classes, per, kernel):
    x, t, gamma = svm_data.planted(F, classes, per, seed=F + classes)
    tol = 1e-3
    m = svm.fit(x, t, kernel=kernel, gamma=gamma, tol=tol)
    assert m.classes == classes and m.pair_coef.shape == (m.pairs, m.sv.shape[0]) and m.sv.dtype == np.float16
    assert (m.kkt_violation <= tol).all() and (m.n_iter > 0).all()
    assert m.n_support.sum() == m.sv.shape[0] and np.array_equal(np.bincount(m.sv_class, minlength=classes), m.n_support)
    xs = x.astype(np.float64)
    for p, (i, j) in enumerate(svm.pair_list(classes)):       # the dual itself, in fp64, on this pair's samples
        idx = np.concatenate([np.flatnonzero(t == i), np.flatnonzero(t == j)])
        y = np.where(t[idx] == i, 1.0, -1.0)
        a, rho, it, viol = svm.solve_pair(svm.kernel_matrix(xs[idx], xs[idx], kernel, gamma), y, 1.0, tol)
        assert viol <= tol and it == m.n_iter[p]
        assert a.min() >= 0.0 and a.max() <= 1.0
        assert abs((a * y).sum()) <= 1e-12 * np.abs(a).sum()
        assert np.float32(-rho) == m.intercept[p]
        # the model's row holds alpha y of exactly these samples, and zeros for the other classes
        inpair = np.isin(m.sv_class, (i, j))
        assert not m.pair_coef[p, ~inpair].any()
        assert np.array_equal(np.sort(m.pair_coef[p, inpair][m.pair_coef[p, inpair] != 0]), np.sort((a * y)[a != 0].astype(np.float32)))
    again = svm.fit(x, t, kernel=kernel, gamma=gamma, tol=tol)
    for name in ('sv', 'sv_class', 'pair_coef', 'intercept', 'w', 'n_iter', 'kkt_violation'):
        assert getattr(again, name).tobytes() == getattr(m, name).tobytes(), name
    if kernel == 'linear':
        # folded from the fp64 coefficients and rounded once: within one rounding of each fp32 coefficient and one of w itself
        c64, s64 = m.pair_coef.astype(np.float64), m.sv.astype(np.float64)
        assert m.w.dtype == np.float32 and (np.abs(m.w - c64 @ s64) <= 2.0 ** -23 * (np.abs(c64) @ np.abs(s64))).all()
    # the training points are separated far better than chance
    assert (svm.vote(svm_data.oracle(m, x.T), classes) == t).mean() > 0.9


def test_gamma_scale_is_scikit_learns_definition():
    x, t, gamma = svm_data.planted(32, 2, 40, 1)
    assert svm.fit(x, t).gamma == pytest.approx(1.0 / (32 * x.astype(np.float64).var()), rel=1e-15) == pytest.approx(gamma, rel=1e-15)


# ---------------------------------------------------------------------------- 3. against scikit-learn
def test_solver_is_as_close_to_a_tight_svc_as_scikit_learn_itself(capsys):
    """Planted (64, 4, 500) at 20 000 fresh points.  Truth: SVC(tol=1e-9).  Both solvers stop on the same criterion at 1e-6 but
    break working-set ties and average rho differently; the factor 4 covers that."""
    SVC = pytest.importorskip('sklearn.svm').SVC
    x, t, gamma = svm_data.planted(64, 4, 500, seed=7)
    pts, _ = svm_data.voxels(64, 4, 20000, seed=7)
    xs = x.astype(np.float64)
    truth = SVC(C=1.0, kernel='rbf', gamma=gamma, tol=1e-9, decision_function_shape='ovo', cache_size=500).fit(xs, t)
    loose = SVC(C=1.0, kernel='rbf', gamma=gamma, tol=1e-6, decision_function_shape='ovo', cache_size=500).fit(xs, t)
    ref = truth.decision_function(pts.T.astype(np.float64))
    err_sk = np.abs(loose.decision_function(pts.T.astype(np.float64)) - ref).max()
    m = svm.fit(x, t, gamma=gamma, tol=1e-6)
    K = svm.kernel_matrix(m.sv, pts.T, 'rbf', gamma)
    # the fp64 solution before the model rounds it to fp32 is not kept: compare the model's decisions, whose coefficient
    # rounding (2^-24 relative per term) is part of what this library returns
    err = np.abs((m.pair_coef.astype(np.float64) @ K + m.intercept.astype(np.float64)[:, None]).T - ref).max()
    with capsys.disabled():
        print(f'\nsvm.fit(tol=1e-6) vs SVC(tol=1e-9): {err:.3e}; SVC(tol=1e-6): {err_sk:.3e}; ratio {err / err_sk:.2f}')
    assert err <= 4 * err_sk


# ---------------------------------------------------------------------------- 4. from_libsvm
@pytest.mark.parametrize('kernel', svm.KERNELS)
@pytest.mark.parametrize('classes', [2, 3, 5])
def test_from_libsvm_reproduces_scikit_learn(classes, kernel):
    """The SVC is fitted on fp16-representable samples and its coefficients are rounded to fp32 in place, so that it carries
    exactly the numbers the model stores; its decisions then agree with the oracle's to 1e-9 relative."""
    SVC = pytest.importorskip('sklearn.svm').SVC
    x, t, gamma = svm_data.planted(32, classes, 30, seed=classes)
    clf = SVC(C=1.0, kernel=kernel, gamma=gamma, decision_function_shape='ovo').fit(x.astype(np.float64), t)
    for name in ('dual_coef_', '_dual_coef_', 'intercept_', '_intercept_'):
        setattr(clf, name, getattr(clf, name).astype(np.float32).astype(np.float64))
    m = svm.from_libsvm(clf.support_vectors_, clf.dual_coef_, clf.n_support_, clf.intercept_, kernel=kernel, gamma=gamma)
    assert np.array_equal(m.sv.astype(np.float64), clf.support_vectors_) and m.classes == classes
    pts, _ = svm_data.voxels(32, classes, 3000, seed=classes)
    dec = svm_data.oracle(m, pts)
    ref = clf.decision_function(pts.T.astype(np.float64))
    ref = ref[:, None] if ref.ndim == 1 else ref
    if classes == 2:
        ref = -ref                                            # scikit-learn's binary decision is positive for classes_[1]
    assert np.abs(dec.T - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.array_equal(svm.vote(dec, classes), clf.predict(pts.T.astype(np.float64)))
    # libsvm layout: rho instead of intercept_, no binary flip
    flip = -1.0 if classes == 2 else 1.0
    m2 = svm.from_libsvm(clf.support_vectors_, flip * clf.dual_coef_, clf.n_support_, -flip * clf.intercept_, kernel=kernel,
                         gamma=gamma, layout='libsvm')
    assert m2.pair_coef.tobytes() == m.pair_coef.tobytes() and m2.intercept.tobytes() == m.intercept.tobytes()
    with pytest.raises(ValueError):
        svm.from_libsvm(clf.support_vectors_, clf.dual_coef_[:, :-1], clf.n_support_, clf.intercept_)


def test_vote_rules():
    """> 0 votes for i, exactly 0 for j; the lowest index wins a tie."""
    d = np.array([[1.0, 0.0, -1.0, 1.0],                     # (0,1)
                  [1.0, 0.0, 1.0, -1.0],                     # (0,2)
                  [1.0, 0.0, 1.0, 1.0]])                     # (1,2)
    assert svm.vote(d, 3).tolist() == [0, 2, 1, 0]            # column 1: zeros vote for j; column 3: one vote each -> 0
    assert svm.pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


# ---------------------------------------------------------------------------- 5. files
def _model(kernel='rbf', F=32, classes=3):
    x, t, gamma = svm_data.planted(F, classes, 12, seed=3)
    return svm.fit(x, t + 1, kernel=kernel, gamma=gamma, class_names=[f'c{i}' for i in range(classes)])


@pytest.mark.parametrize('kernel', svm.KERNELS)
def test_model_file_round_trips_without_pickle(tmp_path, kernel):
    m = _model(kernel)
    vt.save_model(m, tmp_path / 'm.npz')
    with np.load(tmp_path / 'm.npz', allow_pickle=False) as z:
        assert set(z.files) == set(vt.SvmModel.ARRAYS)
        assert z['sv'].dtype == np.float16 and z['pair_coef'].dtype == np.float32 and z['labels'].dtype == np.uint8
    back = vt.load_model(tmp_path / 'm.npz')
    for name in vt.SvmModel.ARRAYS:
        a, b = getattr(back, name), getattr(m, name)
        assert (a.tobytes() == b.tobytes() and a.dtype == b.dtype and a.shape == b.shape) if isinstance(a, np.ndarray) else a == b, name
    assert back.labels.tolist() == [1, 2, 3] and back.class_names == ['c0', 'c1', 'c2']


def test_load_model_refusals(tmp_path):
    m = _model()
    vt.save_model(m, tmp_path / 'm.npz')
    arrays = dict(np.load(tmp_path / 'm.npz', allow_pickle=False))
    bad = {'missing': {k: v for k, v in arrays.items() if k != 'intercept'},
           'coef_shape': dict(arrays, pair_coef=arrays['pair_coef'][:, :-1]),
           'intercept_shape': dict(arrays, intercept=arrays['intercept'][:-1]),
           'sv_dtype': dict(arrays, sv=arrays['sv'].astype(np.float32)),
           'w_shape': dict(arrays, w=np.zeros((3, 32), np.float32)),
           'class_count': dict(arrays, labels=arrays['labels'][:-1]),
           'sv_class': dict(arrays, sv_class=arrays['sv_class'][::-1].copy()),
           'kernel': dict(arrays, kernel=np.asarray('poly'))}
    for name, arr in bad.items():
        np.savez(tmp_path / f'{name}.npz', **arr)
        with pytest.raises(ValueError):
            vt.load_model(tmp_path / f'{name}.npz')
    (tmp_path / 'broken.npz').write_bytes(b'PK\x03\x04 not a zip archive')
    np.save(tmp_path / 'array.npy', np.zeros((4, 32), np.float32))
    vt.save_clustering(vt.Clustering(torch.zeros(2, 32), torch.tensor([1, 1]), torch.tensor(0.0, dtype=torch.float64),
                                     torch.zeros(1, dtype=torch.float64), 1, True), tmp_path / 'c.npz')
    for name in ('broken.npz', 'array.npy', 'c.npz'):
        with pytest.raises(ValueError):
            vt.load_model(tmp_path / name)


# ---------------------------------------------------------------------------- 6. command line
def _main(argv):
    import classify_features
    with pytest.raises(SystemExit) as e:
        classify_features.main(argv)
    return e.value.code


def test_tag_and_paths():
    import classify_features as cf
    assert cf.svm_tag(0.0, 'annotated', 'rbf') == '0.0annotated_rbf'
    assert cf.svm_tag(100.0, 'both', 'linear', normalize=True) == '100.0both_linear_norm'
    assert cf.svm_tag(0.5, 'surface', 'rbf', True, False) == '0.5surface_rbf_norm_nobg'
    pred, model, metrics = cf.output_paths('/x', 'T')
    assert (str(pred), str(model), str(metrics)) == ('/x/svm_predT.npy', '/x/svm_modelT.npz', '/x/svm_metricsT.json')


def test_classify_features_cli_refusals(tmp_path, monkeypatch, capsys):
    """Every exit-1 case, each with its message, and the early exit 0, all before anything touches the device."""
    def boom(*a, **k):
        raise AssertionError('a refused command line reached the GPU entry')

    vt.save_model(_model('rbf', 32), tmp_path / 'm32.npz')
    for name in ('sample', 'predict', 'fit'):
        monkeypatch.setattr(svm, name, boom)
    d = tmp_path / 'case'
    d.mkdir()
    out = lambda: capsys.readouterr().out                     # noqa: E731
    out()
    assert _main(['--data', str(tmp_path / 'nope')]) == 1
    assert 'Invalid argument for --data' in out()
    for flag, bad in (('--num-samples', '-1'), ('--C', '0'), ('--C', '-2'), ('--tol', '0'), ('--gamma', 'auto'), ('--gamma', '-0.5')):
        assert _main(['--data', str(d), flag, bad]) == 1, (flag, bad)
        assert f'Invalid argument for {flag}' in out()
    assert _main(['--data', str(d), '--model', str(tmp_path / 'nope.npz')]) == 1
    assert 'Invalid argument for --model' in out()
    np.savez(tmp_path / 'other.npz', sv=np.zeros((2, 32), np.float16))
    assert _main(['--data', str(d), '--model', str(tmp_path / 'other.npz')]) == 1
    assert 'Invalid argument for --model' in out()
    assert _main(['--data', str(d), '--background', 'labels']) == 1          # no labels.npy
    assert 'Invalid argument for --background' in out()
    assert _main(['--data', str(d), '--num-samples', '10']) == 1
    assert 'Invalid argument for --num-samples: Cannot sample labels' in out()
    assert _main(['--data', str(d)]) == 1                                    # no annotations.npy
    assert 'Invalid argument for --num-samples' in out()
    np.save(d / 'annotations.npy', {'a': np.zeros((2, 3), np.int64), 'b': np.ones((2, 3), np.int64)}, allow_pickle=True)
    assert _main(['--data', str(d)]) == 1
    assert 'Invalid argument for --data' in out()                            # no volume.npy
    np.save(d / 'volume.npy', np.zeros((12, 12, 12), np.float16))
    assert _main(['--data', str(d)]) == 1
    assert 'No features found' in out()
    np.save(d / 'v_features.npy', np.zeros((48, 6, 6, 6), np.float16))
    assert _main(['--data', str(d)]) == 1
    assert 'F = 48 is not a multiple of 32' in out()
    np.save(d / 'v_features.npy', np.zeros((1024, 3, 3, 3), np.float16))
    assert _main(['--data', str(d)]) == 1
    assert 'Invalid argument for --kernel' in out()                          # the message points at reduce_features.py
    assert _main(['--data', str(d), '--kernel', 'rbf']) == 1
    assert 'reduce_features.py' in out()
    np.save(d / 'v_features.npy', np.zeros((64, 6, 6, 6), np.float16))
    assert _main(['--data', str(d), '--model', str(tmp_path / 'm32.npz')]) == 1
    assert 'Invalid argument for --model: fitted on F = 32' in out()
    # existing outputs: exit 0 early, with the tag of the flags (or of the model)
    (d / 'svm_pred0.0annotated_rbf.npy').write_bytes(b'')
    assert _main(['--data', str(d)]) == 0
    assert 'Already inferred SVM preds' in out()
    (d / 'svm_pred0.0annotated_linear_norm_nobg.npy').write_bytes(b'')
    assert _main(['--data', str(d), '--kernel', 'linear', '--normalize', '--background', 'none']) == 0
    assert 'Already inferred SVM preds' in out()
    assert _main(['--data', str(d), '--model', str(tmp_path / 'm32.npz'), '--background', 'none']) == 1       # labels 1..3: _nobg
    assert 'fitted on F = 32' in out()
    (d / 'svm_pred0.0annotated_rbf_nobg.npy').write_bytes(b'')
    assert _main(['--data', str(d), '--model', str(tmp_path / 'm32.npz')]) == 0
    assert 'Already inferred SVM preds' in out()


# ---------------------------------------------------------------------------- 7. the condition on the GPU cases
@pytest.mark.parametrize('kernel', svm.KERNELS)
@pytest.mark.parametrize('case', svm_data.REAL_CASES)
def test_few_voxels_of_the_gpu_cases_are_within_the_bound_of_a_tie(case, kernel, capsys):
    """The GPU test compares labels only where no pair's decision is within its bound of 0: at most 2 % of the voxels may be
    exempt, or the comparison would say little."""
    for normalize in ((False, True) if case == svm_data.NORM_CASE else (False,)):
        model, x, vn = svm_data.real_case(*case, kernel=kernel, normalize=normalize)
        dec = svm_data.oracle(model, x, vn)
        bnd = svm_data.bound(model, x, vn)
        share = svm_data.ambiguous(dec, bnd).mean()
        with capsys.disabled():
            print(f'\n{case} {kernel} norm={normalize}: S = {model.sv.shape[0]}, bound max {bnd.max():.2e} median {np.median(bnd):.2e}, '
                  f'|dec| median {np.median(np.abs(dec)):.2e}, ambiguous {100 * share:.2f} %')
        assert np.isfinite(bnd).all() and (bnd > 0).all()
        assert share <= 0.02
