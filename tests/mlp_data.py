"""Test data, the fp64 oracle and the error bounds shared by tests/test_mlp_cpu.py and tests/test_gpu_mlp.py (no test in here).

Oracle (``logits``): fp64 numpy on the fp16 features and the model's fp32 arrays, evaluated literally:
    a_0 = x (/ the fp32 voxel norm the call is given),  z_l = W_l a_l + b_l,  a_{l+1} = max(z_l, 0),  logits = the last z.

Bound of vittf_mlp_decide per logit (``bound``), worst case against that oracle, u = 2^-24, no fitted constant.  It follows the
arithmetic mlp.hip states, layer by layer; dz_l is the bound on |computed z_l - exact z_l|, and a^ <= a + dz_{l-1} bounds the
computed activations (ReLU is 1-Lipschitz):
  scale   W' = W 2^-e exactly, e = frexp(max |W|) exponent - 11 (the largest entry lies in [2^10, 2^11))
  split   W' = hi + lo + d with |d| <= 2^-22 |W'| + 2^-25: the relative part is two fp16 roundings (2^-11 each), the
          absolute part a lo (or hi) half in the fp16 subnormal range (spacing 2^-24).  In W's units the floor is 2^(e - 25).
  sums    the matrix core adds n exact fp16 x fp16 products into an fp32 accumulator (n = 2 F in layer 0: hi and lo;
          n = 3 in_l later: hi hi, hi lo, lo hi).  How it aligns the 16 products of an instruction is not documented to round
          to nearest, so every addition is allowed a whole ulp: g(n) = 2 n u / (1 - 2 n u), relative to the sum of the
          magnitudes, which the halves inflate by at most (1 + 2^-9).
  layer 0 epilogue: 1 / norm (correctly rounded division: u; 3 u allowed), acc * (1 / norm) (u), the fused multiply-add with
          the bias (u of the result):  dz_0 = E (1 + u) + u |z_0|,  E = (2^-22 + g(2 F)(1 + 2^-9) + 4 u) |W| |x^| + 2^(e-25) |x^|_1
  hand-over  a' = a^ 2^-s exactly, the voxel's largest a' in [2^10, 2^11), so 2^s <= 2^-10 max_j a^_j;  a' = hi + lo + d as above:
          in a's units |d| <= 2^-22 a^ + 2^(s - 25).  The product lo x lo is left out: <= (2^-11 |W'| + 2^-25)(2^-11 a' + 2^-25).
          All of split, split and lo x lo together:  <= 2^-20 |W| a^  +  2^(e - 24) |a^|_1  +  2^(s - 24) |W|_1  (each floor
          doubled to cover its cross terms)
  layer l > 0:  dz_l = |W_l| dz_{l-1}  +  (2^-20 + g(3 in)(1 + 2^-9)) |W_l| a^  +  2^(e-24) |a^|_1  +  2^(s-24) |W_l|_1 row sums,
          then the one rounding of the fused multiply-add (acc 2^s is exact):  dz_l <- dz_l (1 + u) + u |z_l|

``PROB_EPS``: the kernel's uint8 probabilities against 255 softmax of ITS OWN fp32 logits evaluated in fp64 are within
0.5 + PROB_EPS.  d = fl(z_c - max z) (u), t = fl(d fl(log2 e)) (2 u more), e_c = v_exp_f32(t), good to 1 ulp = 2 u.  A class with
|d| > 32 has softmax < 2^-46 on both sides (1e-6 of slack covers it and flushed subnormals); otherwise e_c is off by at most
r = expm1(96 u) + 2 u relative, the sum S of up to 8 of them by r + 7 u, p = fl(e_c / S) by 2 r + 8 u + u, and
y = fma(255, p, 0.5) by 256 u absolute: |y - (255 softmax + 0.5)| <= 255 (2 r + 9 u) + 256 u + 1e-6 = PROB_EPS (3.1e-3);
the floor then lies within 0.5 + PROB_EPS of 255 softmax.

Data: ``int_model`` / ``int_voxels`` are the exact cases (integer features |x| <= 4, sparse integer weights of about 6
non-zeros a row in -4..4, integer biases in -8..8: every layer is an integer far below 2^24, see ``int_magnitudes``);
``planted`` / ``voxels`` / ``real_case`` are the real ones (svm_data's mixture: class centres N(0, 0.6^2), samples = centre +
N(0, 1), fp16), fitted by vt.mlp.fit itself with 20 epochs; ``separable`` moves the centres five times as far apart.
"""
import functools

import numpy as np

from vit_tf_amd import mlp

U = 2.0 ** -24
_R = np.expm1(96 * U) + 2 * U
PROB_EPS = 255 * (2 * _R + 9 * U) + 256 * U + 1e-6

FS = (32, 96, 384, 1024)
HEADS = ((), (32,), (64,), (256,), (96, 32), (256, 256))
CLASSES = (2, 3, 8)
NVOX = (250, 257, 805, 256)
REAL_CASES = ((32, 2, (), 805), (96, 3, (32,), 805), (96, 8, (64,), 805), (384, 4, (256, 64), 2085), (1024, 3, (256,), 1029))
NORM_CASE = 1                                  # the real case that also runs with voxel_norm


# ---------------------------------------------------------------------------- oracle
def layer_values(model, x, voxel_norm=None):
    """[z_0, z_1, ..., logits] in fp64, each [out][nvox]."""
    a = np.asarray(x, np.float64)
    if voxel_norm is not None:
        a = a / np.asarray(voxel_norm, np.float64)[None, :]
    out = []
    for i, (w, b) in enumerate(zip(model.weights, model.biases)):
        z = w.astype(np.float64) @ a + b.astype(np.float64)[:, None]
        out.append(z)
        a = np.maximum(z, 0.0)
    return out


def logits(model, x, voxel_norm=None):
    """fp64 [C][nvox]."""
    return layer_values(model, x, voxel_norm)[-1]


def argmax(z):
    """uint8 [nvox]: the lowest index among equal logits."""
    return np.argmax(z, axis=0).astype(np.uint8)


def softmax255(z):
    """fp64 [C][nvox]: 255 softmax over axis 0."""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(0, keepdims=True))
    return 255.0 * e / e.sum(0, keepdims=True)


# ---------------------------------------------------------------------------- bound
def _gamma(n):
    return 2 * n * U / (1 - 2 * n * U)


def _scale(w):
    m = float(np.abs(w).max())
    return 2.0 ** (np.frexp(m)[1] - 11) if m > 0 else 1.0


def bound(model, x, voxel_norm=None):
    """fp64 [C][nvox]: the bound of the module docstring for every logit."""
    xh = np.abs(np.asarray(x, np.float64))
    if voxel_norm is not None:
        xh = xh / np.asarray(voxel_norm, np.float64)[None, :]
    zs = layer_values(model, x, voxel_norm)
    dz = None
    for i, (w, z) in enumerate(zip(model.weights, zs)):
        aw = np.abs(w.astype(np.float64))
        sc = _scale(aw)
        n_in = aw.shape[1]
        if i == 0:
            e = (2.0 ** -22 + _gamma(2 * n_in) * (1 + 2.0 ** -9) + 4 * U) * (aw @ xh) + sc * 2.0 ** -25 * xh.sum(0)[None, :]
        else:
            a_up = np.maximum(zs[i - 1], 0.0) + dz
            s = 2.0 ** -10 * a_up.max(0) + 2.0 ** -116
            e = (aw @ dz + (2.0 ** -20 + _gamma(3 * n_in) * (1 + 2.0 ** -9)) * (aw @ a_up) + sc * 2.0 ** -24 * a_up.sum(0)[None, :]
                 + 2.0 ** -24 * aw.sum(1)[:, None] * s[None, :])
        dz = e * (1 + U) + U * np.abs(z)
    return dz


def ambiguous(z, b):
    """bool [nvox]: the top-two margin of the logits z is within the sum of their bounds b."""
    order = np.argsort(-z, axis=0, kind='stable')
    cols = np.arange(z.shape[1])
    i0, i1 = order[0], order[1]
    return z[i0, cols] - z[i1, cols] <= b[i0, cols] + b[i1, cols]


# ---------------------------------------------------------------------------- exact cases
def int_model(rng, F, head, classes, tie=None):
    """An MlpModel of sparse small integers.  tie='rows': output row 1 repeats row 0; tie='zero': the last layer is zero."""
    dims = (F,) + tuple(head) + (classes,)
    weights, biases = [], []
    for i in range(len(dims) - 1):
        w = rng.integers(-4, 5, size=(dims[i + 1], dims[i])) * (rng.random((dims[i + 1], dims[i])) < 6.0 / dims[i])
        weights.append(w.astype(np.float32))
        biases.append(rng.integers(-8, 9, size=dims[i + 1]).astype(np.float32))
    if tie == 'rows':
        weights[-1][1], biases[-1][1] = weights[-1][0], biases[-1][0]
    elif tie == 'zero':
        weights[-1][:], biases[-1][:] = 0, 0
    return mlp.MlpModel([str(i) for i in range(classes)], np.arange(classes), F, False, head, weights, biases)


def int_voxels(rng, F, nvox):
    return rng.integers(-4, 5, size=(F, nvox)).astype(np.float16)


def int_magnitudes(model, x):
    """(is every value of every layer an integer, the largest sum_k |W_jk| |a_k| + |b_j| over the layers, the largest hidden
    activation): the exact cases need True, < 2^24 (every partial sum of the accumulation is then exact) and < 2^21 (the
    activation's hi + lo halves then hold it exactly)."""
    a = np.asarray(x, np.float64)
    whole, big, act = True, 0.0, 0.0
    for i, (w, b) in enumerate(zip(model.weights, model.biases)):
        w, b = w.astype(np.float64), b.astype(np.float64)
        z = w @ a + b[:, None]
        whole = whole and bool(np.array_equal(z, np.rint(z)))
        big = max(big, float((np.abs(w) @ np.abs(a) + np.abs(b)[:, None]).max()))
        a = np.maximum(z, 0.0)
        if i + 1 < len(model.weights):
            act = max(act, float(a.max()))
    return whole, big, act


# ---------------------------------------------------------------------------- real cases
def centres(F, classes, seed):
    return 0.6 * np.random.default_rng(seed).standard_normal((classes, F))


def planted(F, classes, per_class, seed):
    """(samples fp16 [classes * per_class][F], targets int64)."""
    rng = np.random.default_rng(seed + 1000)
    mu = centres(F, classes, seed)
    t = np.repeat(np.arange(classes), per_class)
    return (mu[t] + rng.standard_normal((t.size, F))).astype(np.float16), t


def separable(F, classes, per_class, seed):
    """(samples fp16, targets): the same mixture with the centres five times as far apart (N(0, 3^2) per feature): classes
    that a linear head separates."""
    rng = np.random.default_rng(seed + 3000)
    mu = 5.0 * centres(F, classes, seed)
    t = np.repeat(np.arange(classes), per_class)
    return (mu[t] + rng.standard_normal((t.size, F))).astype(np.float16), t


def voxels(F, classes, nvox, seed):
    """fp16 [F][nvox]: fresh points of the mixture planted(F, classes, ., seed) draws from."""
    rng = np.random.default_rng(seed + 2000)
    mu = centres(F, classes, seed)
    t = rng.integers(0, classes, size=nvox)
    return np.ascontiguousarray((mu[t] + rng.standard_normal((nvox, F))).astype(np.float16).T)


def host_norms(x):
    """fp32 [nvox]: the voxels' L2 norms (fp64 sum, rounded once) -- any positive fp32 array serves as voxel_norm."""
    return np.sqrt((np.asarray(x, np.float64) ** 2).sum(0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_case(index, normalize=False):
    """(model, x fp16 [F][nvox], voxel_norm or None, oracle logits, bound) of REAL_CASES[index]; computed once a process."""
    F, classes, head, nvox = REAL_CASES[index]
    s, t = planted(F, classes, 60, 10 + index)
    # (unit-norm features are 1 / sqrt(F) small: the normalised head needs a larger step to learn anything in 20 epochs)
    model = mlp.fit(s, t, hidden=head, epochs=20, lr=0.05 if normalize else 1e-3, seed=index, normalize=normalize)
    x = voxels(F, classes, nvox, 10 + index)
    vn = host_norms(x) if normalize else None
    for a in (x,) if vn is None else (x, vn):
        a.setflags(write=False)
    return model, x, vn, logits(model, x, vn), bound(model, x, vn)
