"""Test data, the fp64 oracle and the error bounds shared by tests/test_svm_cpu.py and tests/test_gpu_svm.py (no test in here).

Data (``planted``): class centres N(0, 0.6^2) per feature, samples = centre + N(0, 1), rounded to fp16; gamma = 1 / (F var),
C = 1; everything from a seeded ``default_rng``.  ``voxels`` draws fresh points of the same mixture as an [F][nvox] volume.

Oracle (``oracle``): fp64 numpy on the fp16 features and the model's arrays, the formulas evaluated literally:
    dec_p(x) = sum_s pair_coef[p][s] K(x, sv_s) + intercept[p],   K = exp(-gamma |x - s|^2)  or  x . s,
x divided by the fp32 voxel norm the call is given, when it is given one.

Bound of vittf_svm_rbf_decide per decision value (``rbf_bound``), worst case, u = 2^-24, no fitted constant.  Kernel side:
  d2  the kernel forms  fl(|x|^2) + fl(|s|^2) - 2 fl(s . x):  three fp32 accumulations of F exact fp16 products in some order
      (at most F u relative to the sum of the magnitudes, each), and 4 further roundings (the sum, the fused multiply-add, the
      reciprocal of the norm twice):  |delta d2| <= g T,  g = (F + 12) u / (1 - (F + 12) u),  T = |x|^2 + |s|^2 + 2 sum_f |x_f s_f|;
      the clamp at 0 moves towards the true value
  a   the exponent gamma d2: gamma is rounded to fp32, times log2(e) rounded, the product rounded:  |delta a| <= gamma |delta d2|
      + 3 u gamma (d2 + |delta d2|)
  K   v_exp_f32 is good to 1 ulp = 2 u relative, results below 2^-126 may be flushed to 0:
      |delta K| <= K expm1(|delta a|) + 2 u K exp(|delta a|) + 2^-126
Second contraction, with c' = coef / sigma, sigma = 2^e > max |coef| the kernel's power-of-two scale (exact), Kc = K + |delta K|:
  split   c' = hi + lo + e_c and Kc = hi + lo + e_K with |e| <= 2^-22 |value| + 2^-25 (a lo half in the fp16 subnormal range);
          the product lo x lo is dropped: <= (2^-11 |c'| + 2^-25)(2^-11 Kc + 2^-25).  Terms with coef = 0 are exactly 0.
  sum     3 exact fp16 x fp16 products per non-zero coefficient, fp32 accumulation in some order:  (3 nnz_p) u (1 + 2^-9) sum |c| Kc
  last    dec = fl(acc sigma + intercept): u |dec|
``linear_bound`` is tests/pca_data.py's project_bound for w (fp16 hi + lo, fp32 accumulation, (F + 8) u) with 4 more roundings
(reciprocal norm, the fused multiply-add with the intercept) and the distance of the model's fp32 w from the literal fp64 fold.
"""
import numpy as np

from vit_tf_amd import svm

U = 2.0 ** -24


def centres(F, classes, seed):
    return 0.6 * np.random.default_rng(seed).standard_normal((classes, F))


def planted(F, classes, per_class, seed):
    """(samples fp16 [classes * per_class][F], targets int64, gamma): `per_class` points around each planted centre."""
    rng = np.random.default_rng(seed + 1000)
    mu = centres(F, classes, seed)
    t = np.repeat(np.arange(classes), per_class)
    x = (mu[t] + rng.standard_normal((t.size, F))).astype(np.float16)
    return x, t, 1.0 / (F * float(x.astype(np.float64).var()))


def voxels(F, classes, nvox, seed):
    """(fp16 [F][nvox], class of every voxel): fresh points of the mixture planted(F, classes, ., seed) draws from."""
    rng = np.random.default_rng(seed + 2000)
    mu = centres(F, classes, seed)
    t = rng.integers(0, classes, size=nvox)
    return np.ascontiguousarray((mu[t] + rng.standard_normal((nvox, F))).astype(np.float16).T), t


def _xhat(x, voxel_norm):
    x = np.asarray(x, np.float64)
    return x if voxel_norm is None else x / np.asarray(voxel_norm, np.float64)[None, :]


def oracle(model, x, voxel_norm=None):
    """fp64 [P][nvox]: the decisions of `model` for the fp16 volume x [F][nvox], evaluated literally."""
    xh = _xhat(x, voxel_norm)
    K = svm.kernel_matrix(model.sv, xh.T, model.kernel, model.gamma)                # [S][nvox]
    return model.pair_coef.astype(np.float64) @ K + model.intercept.astype(np.float64)[:, None]


def rbf_bound(model, x, voxel_norm=None):
    """fp64 [P][nvox]: the bound of the module docstring for every decision of vittf_svm_rbf_decide."""
    xh = _xhat(x, voxel_norm)
    s = model.sv.astype(np.float64)
    F = s.shape[1]
    x2, s2 = (xh * xh).sum(0), (s * s).sum(1)
    d2 = np.maximum(s2[:, None] + x2[None, :] - 2.0 * (s @ xh), 0.0)
    g = (F + 12) * U / (1.0 - (F + 12) * U)
    dd2 = g * (s2[:, None] + x2[None, :] + 2.0 * (np.abs(s) @ np.abs(xh)))
    da = model.gamma * dd2 + 3 * U * model.gamma * (d2 + dd2)
    K = np.exp(-model.gamma * d2)
    dK = K * np.expm1(da) + 2 * U * K * np.exp(da) + 2.0 ** -126
    Kc = K + dK
    A = np.abs(model.pair_coef.astype(np.float64))
    M = (A > 0).astype(np.float64)
    cmax = A.max()
    sigma = 2.0 ** np.frexp(cmax)[1] if cmax > 0 else 1.0
    AK, MK, A1, nnz = A @ Kc, M @ Kc, A.sum(1)[:, None], M.sum(1)[:, None]
    split = 2.0 ** -21 * AK + 2.0 ** -25 * (A1 + sigma * MK)
    lolo = 2.0 ** -22 * AK + 2.0 ** -36 * (A1 + sigma * MK) + sigma * 2.0 ** -50 * nnz
    acc = 3 * nnz * U * (1 + 2.0 ** -9) * AK
    b = A @ dK + split + lolo + acc
    return b + U * (np.abs(oracle(model, x, voxel_norm)) + b)


def linear_bound(model, x, voxel_norm=None):
    """fp64 [P][nvox]: the bound of vittf_svm_linear_decide against the literal oracle."""
    xh = _xhat(x, voxel_norm)
    F = xh.shape[0]
    w64 = model.pair_coef.astype(np.float64) @ model.sv.astype(np.float64)
    w = model.w.astype(np.float64)
    b = np.abs(model.intercept.astype(np.float64))[:, None]
    return ((F + 12) * U * (np.abs(w) @ np.abs(xh) + b) + 2.0 ** -25 * np.abs(xh).sum(0)[None, :]
            + np.abs(w - w64) @ np.abs(xh))


def bound(model, x, voxel_norm=None):
    return (rbf_bound if model.kernel == 'rbf' else linear_bound)(model, x, voxel_norm)


def host_norms(x):
    """fp32 [nvox]: what vittf_voxel_norm returns to within its own rounding -- max(|x_v|, 1e-12); the oracle and the kernel
    are given the SAME array, so its rounding is in neither bound."""
    return np.maximum(np.sqrt((np.asarray(x, np.float64) ** 2).sum(0)), 1e-12).astype(np.float32)


# the real-valued GPU cases (F, classes, samples per class, nvox); test_svm_cpu.py checks the condition on them
REAL_CASES = ((32, 2, 40, 805), (96, 3, 40, 805), (96, 8, 40, 805), (384, 4, 64, 2085), (768, 3, 48, 1029))
NORM_CASE = (96, 3, 40, 805)          # also run with voxel_norm
_models = {}


def real_case(F, classes, per_class, nvox, kernel='rbf', normalize=False):
    """(model, x fp16 [F][nvox], voxel_norm or None) of a real-valued case: fitted once per process and shared."""
    key = (F, classes, per_class, nvox, kernel, normalize)
    if key not in _models:
        xs, t, gamma = planted(F, classes, per_class, seed=F + classes)
        x, _ = voxels(F, classes, nvox, seed=F + classes)
        vn = host_norms(x) if normalize else None
        if normalize:
            gamma = 1.0 / (F * float(svm.round_samples(xs, True).astype(np.float64).var()))
        _models[key] = (svm.fit(xs, t, kernel=kernel, C=1.0, gamma=gamma, tol=1e-3, normalize=normalize), x, vn)
    return _models[key]


def ambiguous(dec, bnd):
    """bool [nvox]: some pair's decision is within its bound of 0 -- the vote of such a voxel may legitimately differ."""
    return (np.abs(dec) <= bnd).any(0)
