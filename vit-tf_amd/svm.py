"""Support-vector classification of a feature volume from annotated voxels: the learned counterpart of the similarity query,
and the supervised companion of pca.py and kmeans.py.  A one-vs-one C-SVC as libsvm and scikit-learn define it, with an RBF
or a linear kernel.

``fit`` is host work in fp64 over a few thousand samples (like the k-means++ start and the PCA eigenproblem): per pair of
classes the C-SVC dual is solved on the precomputed kernel matrix by SMO with libsvm's second-order working-set selection
(Fan, Chen, Lin 2005), without shrinking, until the maximal KKT violation is at most ``tol``.  The samples are rounded to fp16
first, so the solver sees exactly the support vectors the kernel evaluates.  ``predict`` is the pass over the volume: for every
voxel and every support vector a dot product, an exponential and a second contraction against the dual coefficients, then the
vote -- libvittf's vittf_svm_rbf_decide / vittf_svm_linear_decide (svm.hip).  There is no CPU path for it.

Conventions (those of the C entries): classes are numbered 0..C-1 in ascending order of their label value; the P = C (C-1) / 2
pairs are ordered (0,1), (0,2), ..., (C-2,C-1); for the pair (i, j) a decision > 0 votes for i, anything else for j; the class
with the most votes wins, the lowest index among equal counts.  scikit-learn is not imported anywhere.
"""
import numpy as np
import torch

from . import _classify, _lib
from ._classify import round_samples, sample                                                    # noqa: F401
from ._featvol import _np

KERNELS = ('rbf', 'linear')
MAX_SAMPLES_PER_CLASS = 4096          # a pair's fp64 kernel matrix is then at most 8192^2 x 8 bytes = 512 MB
TAU = 1e-12                           # libsvm's floor of the curvature of a working pair


class SvmModel:
    """A fitted (or imported) one-vs-one C-SVC as plain arrays:
      kernel 'rbf' | 'linear', gamma, C (floats), normalize (bool: the voxels are divided by their L2 norm first)
      class_names [C] str, labels uint8 [C] (the value a label volume carries for each class, ascending)
      sv fp16 [S][F], sv_class int32 [S] (ascending), pair_coef fp32 [P][S] (zero where the class of the support vector is not
      in the pair), intercept fp32 [P], w fp32 [P][F] (linear kernel: sum_s pair_coef[p][s] sv_s folded in fp64, rounded once;
      empty for rbf)
      fit statistics: n_iter int64 [P], kkt_violation fp64 [P], n_support int32 [C]."""
    ARRAYS = ('kernel', 'gamma', 'C', 'normalize', 'class_names', 'labels', 'sv', 'sv_class', 'pair_coef', 'intercept', 'w',
              'n_iter', 'kkt_violation', 'n_support')

    def __init__(self, kernel, gamma, C, normalize, class_names, labels, sv, sv_class, pair_coef, intercept, w=None,
                 n_iter=None, kkt_violation=None, n_support=None):
        if kernel not in KERNELS:
            raise ValueError(f'kernel must be one of {KERNELS}, got {kernel!r}')
        self.kernel, self.gamma, self.C, self.normalize = str(kernel), float(gamma), float(C), bool(normalize)
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        self.class_names = [str(n) for n in class_names]
        self.sv = np.ascontiguousarray(sv, dtype=np.float16)
        self.sv_class = np.ascontiguousarray(sv_class, dtype=np.int32).reshape(-1)
        self.pair_coef = np.ascontiguousarray(pair_coef, dtype=np.float32)
        self.intercept = np.ascontiguousarray(intercept, dtype=np.float32).reshape(-1)
        c = self.labels.size
        p = c * (c - 1) // 2
        if self.sv.ndim != 2:
            raise ValueError(f'sv must be [S][F], got {self.sv.shape}')
        s, f = self.sv.shape
        if w is None or np.size(w) == 0:
            w = fold_linear(self.pair_coef, self.sv) if self.kernel == 'linear' else np.zeros((0, f), np.float32)
        self.w = np.ascontiguousarray(w, dtype=np.float32)
        self.n_iter = np.zeros(p, np.int64) if n_iter is None else np.ascontiguousarray(n_iter, dtype=np.int64).reshape(-1)
        self.kkt_violation = (np.zeros(p, np.float64) if kkt_violation is None
                              else np.ascontiguousarray(kkt_violation, dtype=np.float64).reshape(-1))
        self.n_support = (np.bincount(self.sv_class, minlength=c).astype(np.int32) if n_support is None
                          else np.ascontiguousarray(n_support, dtype=np.int32).reshape(-1))
        self._check()

    @property
    def classes(self):
        return int(self.labels.size)

    @property
    def n_features(self):
        return int(self.sv.shape[1])

    @property
    def pairs(self):
        return self.classes * (self.classes - 1) // 2

    def _check(self):
        c, p = self.classes, self.pairs
        s, f = self.sv.shape
        _classify.check_classes(self.class_names, self.labels, _lib.SVM_MAX_CLASSES)
        if not 1 <= s <= _lib.SVM_MAX_SV:
            raise ValueError(f'support vectors must number 1..{_lib.SVM_MAX_SV}, got {s}')
        _classify.check_f(f)
        if self.sv_class.shape != (s,) or np.any(np.diff(self.sv_class) < 0) or self.sv_class.min() < 0 or self.sv_class.max() >= c:
            raise ValueError('sv_class must hold the class 0..C-1 of every support vector, ascending')
        if self.pair_coef.shape != (p, s) or self.intercept.shape != (p,):
            raise ValueError(f'pair_coef {self.pair_coef.shape} / intercept {self.intercept.shape} are not [{p}][{s}] / [{p}]')
        if self.w.shape != ((p, f) if self.kernel == 'linear' else (0, f)):
            raise ValueError(f'w {self.w.shape} does not fit a {self.kernel} model of {p} pairs and F = {f}')
        if self.n_iter.shape != (p,) or self.kkt_violation.shape != (p,) or self.n_support.shape != (c,):
            raise ValueError('the fit statistics do not fit the number of pairs / classes')
        if not (np.isfinite(self.gamma) and self.gamma >= 0 and np.isfinite(self.pair_coef).all() and np.isfinite(self.intercept).all()):
            raise ValueError('gamma, pair_coef and intercept must be finite, gamma not negative')

    def decide_slab(self, x, want_extra):
        """(labels, the fp32 decisions [P][n] or None) of the (F, n) matrix x, without voxel norms."""
        return decide(x, self, None, want_extra)


def pair_list(classes):
    """[(i, j)] in the order of the decisions: (0,1), (0,2), ..., (C-2,C-1)."""
    return [(i, j) for i in range(classes) for j in range(i + 1, classes)]


def fold_linear(pair_coef, sv):
    """fp32 [P][F]: w_p = sum_s pair_coef[p][s] sv_s in fp64, rounded once."""
    return (np.asarray(pair_coef, np.float64) @ np.asarray(sv, np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the solver (fp64, host)
def solve_pair(K, y, C=1.0, tol=1e-3, max_iter=None):
    """The C-SVC dual  min 0.5 a' Q a - e' a,  0 <= a <= C,  y' a = 0  (Q_ij = y_i y_j K_ij) by SMO with the working-set
    selection WSS 2 of Fan, Chen, Lin (2005), as libsvm's Solver does it without shrinking.  K fp64 [n][n], y +-1 [n].
    Stops when m(a) - M(a) <= tol, measured on a gradient recomputed from a (not the running one).
    Returns (alpha fp64 [n], rho, iterations, violation); decisions are sum_i alpha_i y_i K(x_i, x) - rho."""
    n = y.size
    y = y.astype(np.float64)
    if max_iter is None:
        max_iter = max(10_000_000, 100 * n)
    a = np.zeros(n)
    G = -np.ones(n)
    QD = np.diag(K).copy()
    pos = y > 0
    it = 0
    viol = np.inf
    while True:
        yG = y * G
        up = np.where(pos, a < C, a > 0)
        low = np.where(pos, a > 0, a < C)
        mg = np.where(up, -yG, -np.inf)
        i = int(np.argmax(mg))
        gmax = mg[i]
        gmax2 = np.max(np.where(low, yG, -np.inf))
        if gmax + gmax2 <= tol or it >= max_iter:
            G = (K @ (a * y)) * y - 1.0                  # the stopping rule holds for the exact gradient too, or the loop goes on
            yG = y * G
            viol = float(np.max(np.where(up, -yG, -np.inf)) + np.max(np.where(low, yG, -np.inf)))
            if viol <= tol or it >= max_iter:
                break
            continue
        Ki = K[i]
        b = gmax + yG
        quad = QD[i] + QD - 2.0 * Ki
        quad = np.where(quad > 0, quad, TAU)
        obj = np.where(low & (b > 0), -(b * b) / quad, np.inf)
        j = int(np.argmin(obj))
        Kj = K[j]
        ai, aj = a[i], a[j]
        if y[i] != y[j]:
            q = QD[i] + QD[j] - 2.0 * Ki[j]              # = QD_i + QD_j + 2 Q_ij
            q = q if q > 0 else TAU
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0.0, diff
            elif ni < 0:
                ni, nj = 0.0, -diff
            if diff > 0:
                if ni > C:
                    ni, nj = C, C - diff
            elif nj > C:
                nj, ni = C, C + diff
        else:
            q = QD[i] + QD[j] - 2.0 * Ki[j]
            q = q if q > 0 else TAU
            delta = (G[i] - G[j]) / q
            tot = ai + aj
            ni, nj = ai - delta, aj + delta
            if tot > C:
                if ni > C:
                    ni, nj = C, tot - C
            elif nj < 0:
                nj, ni = 0.0, tot
            if tot > C:
                if nj > C:
                    nj, ni = C, tot - C
            elif ni < 0:
                ni, nj = 0.0, tot
        a[i], a[j] = ni, nj
        G += (y[i] * (ni - ai)) * (y * Ki) + (y[j] * (nj - aj)) * (y * Kj)
        it += 1
    # rho as libsvm's calculate_rho
    free = (a > 0) & (a < C)
    if free.any():
        rho = float(yG[free].sum() / free.sum())
    else:
        at_up, at_low = a >= C, a <= 0
        ub = np.min(np.where((at_up & ~pos) | (at_low & pos), yG, np.inf))
        lb = np.max(np.where((at_up & pos) | (at_low & ~pos), yG, -np.inf))
        rho = float((ub + lb) / 2)
    return a, rho, it, viol


def kernel_matrix(A, B, kernel, gamma):
    """fp64 K(a_i, b_j) for the rows of A and B, the formulas evaluated literally: exp(-gamma |a - b|^2) or a . b."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if kernel == 'linear':
        return A @ B.T
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    return np.exp(-gamma * np.maximum(d2, 0.0))


def fit(samples, targets, kernel='rbf', C=1.0, gamma='scale', tol=1e-3, max_iter=None, normalize=False, class_names=None):
    """SvmModel of a one-vs-one C-SVC on samples [n][F] with integer targets [n] (label values 0..255; the classes are their
    distinct values, ascending).  The samples are rounded to fp16 first (after the L2 normalisation when `normalize`, which the
    model then asks of every voxel too); gamma='scale' is 1 / (F var(samples)) of the rounded samples, as scikit-learn defines
    it.  Per pair: solve_pair on the fp64 kernel matrix.  At most 4096 samples per class.  Deterministic."""
    if kernel not in KERNELS:
        raise ValueError(f'kernel must be one of {KERNELS}, got {kernel!r}')
    x16 = round_samples(samples, normalize)
    x = x16.astype(np.float64)
    n, f = x.shape
    values, index, names = _classify.class_table(targets, class_names, n, _lib.SVM_MAX_CLASSES, f)
    c = values.size
    if not (C > 0 and np.isfinite(C)) or not tol > 0:
        raise ValueError('C and tol must be positive')
    members = [np.flatnonzero(index == k) for k in range(c)]
    for v, m in zip(values, members):
        if m.size > MAX_SAMPLES_PER_CLASS:
            raise ValueError(f'class {v} has {m.size} samples, more than {MAX_SAMPLES_PER_CLASS}')
    if isinstance(gamma, str):
        if gamma != 'scale':
            raise ValueError(f"gamma must be 'scale' or a number, got {gamma!r}")
        var = float(x.var())
        gamma = 1.0 / (f * var) if var > 0 else 1.0
    gamma = float(gamma)
    if not (np.isfinite(gamma) and gamma >= 0):
        raise ValueError(f'gamma must be finite and not negative, got {gamma}')
    _classify.check_names(names, c)
    pairs = pair_list(c)
    alphas, rhos, iters, viols = [], [], [], []
    for i, j in pairs:
        idx = np.concatenate([members[i], members[j]])
        y = np.concatenate([np.ones(members[i].size), -np.ones(members[j].size)])
        K = kernel_matrix(x[idx], x[idx], kernel, gamma)
        a, rho, it, viol = solve_pair(K, y, float(C), float(tol), max_iter)
        alphas.append((idx, a * y))
        rhos.append(rho)
        iters.append(it)
        viols.append(viol)
    is_sv = np.zeros(n, bool)
    for idx, ay in alphas:
        is_sv[idx[ay != 0]] = True
    order = np.concatenate([m[is_sv[m]] for m in members])           # by class, in sample order inside a class
    if order.size == 0:
        raise ValueError('the fit found no support vector')
    slot = np.full(n, -1)
    slot[order] = np.arange(order.size)
    coef = np.zeros((len(pairs), order.size))
    for p, (idx, ay) in enumerate(alphas):
        keep = ay != 0
        coef[p, slot[idx[keep]]] = ay[keep]
    sv_class = np.concatenate([np.full(int(is_sv[m].sum()), k) for k, m in enumerate(members)])
    return SvmModel(kernel, gamma, C, normalize, names, values, x16[order], sv_class, coef, -np.asarray(rhos),
                    w=fold_linear(coef, x16[order]) if kernel == 'linear' else None, n_iter=iters, kkt_violation=viols)


def from_libsvm(support_vectors, dual_coef, n_support, intercept, kernel='rbf', gamma=0.0, C=1.0, normalize=False,
                class_names=None, labels=None, layout='sklearn'):
    """SvmModel from arrays in libsvm / scikit-learn layout (only arrays go in: nothing is imported): support_vectors [S][F]
    grouped by class, n_support [C], dual_coef [C-1][S] -- for a support vector of class c, row k holds its coefficient in the
    pair of c with the k-th OTHER class -- and one constant per pair.
    layout='sklearn': `intercept` is ``intercept_`` (= -rho) and, in the BINARY case, scikit-learn has flipped the sign of both
    ``dual_coef_`` and ``intercept_`` (so that a positive decision means classes_[1]); the flip is undone here, so that a
    positive decision votes for class 0 like in every other case.  layout='libsvm': `intercept` is libsvm's rho, no flip.
    The support vectors are rounded to fp16 and the coefficients to fp32: fit the source model on fp16-representable samples
    if the decisions are to agree to more than that."""
    if layout not in ('sklearn', 'libsvm'):
        raise ValueError(f"layout must be 'sklearn' or 'libsvm', got {layout!r}")
    sv = round_samples(support_vectors)
    nsup = _np(n_support, np.int64).reshape(-1)
    c = nsup.size
    dual = _np(dual_coef, np.float64)
    b = _np(intercept, np.float64).reshape(-1)
    pairs = pair_list(c)
    if c < 2 or dual.shape != (c - 1, sv.shape[0]) or nsup.sum() != sv.shape[0] or b.size != len(pairs):
        raise ValueError(f'dual_coef {dual.shape}, n_support {nsup.tolist()}, intercept [{b.size}] and {sv.shape[0]} support '
                         'vectors do not describe one model')
    if layout == 'libsvm':
        b = -b
    elif c == 2:
        dual, b = -dual, -b
    start = np.concatenate(([0], np.cumsum(nsup)))
    coef = np.zeros((len(pairs), sv.shape[0]))
    for p, (i, j) in enumerate(pairs):
        coef[p, start[i]:start[i + 1]] = dual[j - 1, start[i]:start[i + 1]]
        coef[p, start[j]:start[j + 1]] = dual[i, start[j]:start[j + 1]]
    values = np.arange(c) if labels is None else labels
    names = [str(v) for v in np.asarray(values).reshape(-1)] if class_names is None else class_names
    return SvmModel(kernel, gamma, C, normalize, names, values, sv, np.repeat(np.arange(c), nsup), coef, b)


def vote(decision, classes):
    """uint8 [n]: the one-vs-one vote over decisions [P][n] (numpy): > 0 votes for i, anything else for j; the lowest index
    wins among equal counts."""
    d = np.asarray(decision)
    votes = np.zeros((classes, d.shape[1]), np.int64)
    for p, (i, j) in enumerate(pair_list(classes)):
        pos = d[p] > 0
        votes[i] += pos
        votes[j] += ~pos
    return np.argmax(votes, axis=0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- files
def save_model(model, path):
    """An .npz holding exactly SvmModel.ARRAYS as plain arrays (no pickled objects)."""
    arrays = {'kernel': np.asarray(model.kernel), 'gamma': np.asarray(model.gamma, np.float64), 'C': np.asarray(model.C, np.float64),
              'normalize': np.asarray(model.normalize), 'class_names': np.asarray(model.class_names, dtype=np.str_),
              'labels': model.labels, 'sv': model.sv, 'sv_class': model.sv_class, 'pair_coef': model.pair_coef,
              'intercept': model.intercept, 'w': model.w, 'n_iter': model.n_iter, 'kkt_violation': model.kkt_violation,
              'n_support': model.n_support}
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def load_model(path):
    """The SvmModel of a file save_model wrote; ValueError for anything else (a missing key, shapes that disagree, another
    .npz, a .npy, a damaged file)."""
    dtypes = {'sv': np.float16, 'pair_coef': np.float32, 'intercept': np.float32, 'w': np.float32, 'labels': np.uint8}
    with _classify.open_model(path, 'an SVM model', SvmModel.ARRAYS, dtypes) as z:
        if z['w'].ndim != 2:
            raise ValueError(f"w is {z['w'].shape}, not [P][F]")
        return SvmModel(str(z['kernel'][()]), float(z['gamma']), float(z['C']), bool(z['normalize']), _classify.names_of(z),
                        z['labels'], z['sv'], z['sv_class'], z['pair_coef'], z['intercept'], w=z['w'], n_iter=z['n_iter'],
                        kkt_violation=z['kkt_violation'], n_support=z['n_support'])


# ---------------------------------------------------------------------------------------------- the GPU pass
def decide(x, model, voxel_norm=None, want_decision=False):
    """(labels uint8 [nvox], decision fp32 [P][nvox] or None) on the device for the (F, nvox) fp16 device matrix `x`: one
    vittf_svm_rbf_decide or vittf_svm_linear_decide call."""
    lib = _lib.require_device()
    f, nvox = x.shape
    _classify.check_model_f(f, model)
    if model.kernel == 'rbf' and f > 768:
        raise ValueError(f'the RBF kernel takes F <= 768, got {f}: reduce the volume first (reduce_features.py)')
    dev = x.device
    c, p = model.classes, model.pairs
    labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
    dec = torch.empty((p, nvox), dtype=torch.float32, device=dev) if want_decision else None
    b = torch.from_numpy(model.intercept).to(dev)
    vn = _classify.norm_argument(voxel_norm, nvox, dev)
    with torch.cuda.device(dev):
        if model.kernel == 'rbf':
            sv = torch.from_numpy(model.sv).to(dev)
            coef = torch.from_numpy(model.pair_coef).to(dev)
            s = sv.shape[0]
            ws_bytes = lib.vittf_svm_rbf_workspace_bytes(f, s, c)
            if ws_bytes == 0:
                raise ValueError(f'vittf_svm_rbf_decide refuses F = {f}, {s} support vectors, {c} classes')
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.vittf_svm_rbf_decide(_lib.ptr(x), f, nvox, _lib.ptr(sv), _lib.ptr(coef), _lib.ptr(b), s, c, model.gamma,
                                                _lib.ptr(vn), _lib.ptr(labels), _lib.ptr(dec), _lib.ptr(ws), ws_bytes,
                                                _lib.stream_ptr()), 'vittf_svm_rbf_decide')
        else:
            w = torch.from_numpy(model.w).to(dev)
            _lib.check(lib.vittf_svm_linear_decide(_lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), c, _lib.ptr(vn), _lib.ptr(labels),
                                                   _lib.ptr(dec), _lib.stream_ptr()), 'vittf_svm_linear_decide')
    return labels, dec


def predict(feat, model, return_decision=False):
    """uint8 device tensor with the voxel shape of `feat` (F, W', H', D'): the class INDEX 0..C-1 of every voxel
    (model.labels[index] is the value a label volume carries); with return_decision also the fp32 [P] + voxel shape decisions
    the vote was taken over.  A model fitted with `normalize` has the voxels divided by their norms (vt.similarity.voxel_norms)."""
    return _classify.predict_volume(feat, model, lambda x, m, vn: decide(x, m, vn, return_decision), model.normalize)
