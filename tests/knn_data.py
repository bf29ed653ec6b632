"""Test data, the fp64 oracle and the error bounds shared by tests/test_knn_cpu.py and tests/test_gpu_knn.py (no test in here).

Data: ``real_case`` -- tests/svm_data.py's planted mixture (``planted`` for the bank, ``voxels`` for the volume, seed = F +
classes), the bank made by vt.knn.fit (L2-normalised in fp64, rounded once to fp16, sorted by class); ``int_case`` -- integer
features (tests/pca_data.py's planted_int, |x| <= 8) against an integer bank in -3..3 with some rows copied into a row of the
other lane half (rows 4 i .. 4 i + 3 of a chunk of 32 lie in half i % 2), so that every similarity is an exact integer below
2^24 in any summation order and equal similarities are frequent.

Oracle (``oracle``): fp64 numpy on the fp16 arrays, the contract evaluated literally: sim = bank @ x (divided by the fp32 voxel
norm the call is given, when it is given one); the neighbours by a stable descending argsort (larger sim first, then lower
index); w_j = 1 or exp((sim_j - sim_1) / T); scores[c] = the sum of w_j over the ranks of class c; label = the first arg-max.

Bounds, worst case, u = 2^-24, no fitted constant.
  sim     (``sim_bound``) the kernel forms fl(fl(sum_f s_f x_f) fl(1 / norm)): F exact fp16 products accumulated in fp32 in some
          order (at most F u relative to the sum of the magnitudes) and the roundings of the reciprocal and of the product,
          with the allowance tests/svm_data.py makes for the accumulation inside the MFMA:
          |delta sim| <= g sum_f |s_f x_f| / norm + 2^-126,  g = (F + 12) u / (1 - (F + 12) u)   (a denormal product may be flushed)
  scores  (``score_bound``) against the formula evaluated in fp64 ON GIVEN neighbours (the call's own nn_sim / nn_index):
          uniform weights are small integers, exact.  softmax: the kernel forms e' = fl(fl(s_j - s_1) c), c = fl32(log2(e)
          fl32(1 / T)): four roundings, |e' - e| <= t |e| with t = 4 u / (1 - 4 u) (e = (s_j - s_1) log2(e) / T); v_exp_f32 is
          good to 1 ulp = 2 u relative and may flush a result below 2^-126:
              |delta w_j| <= w_j expm1(t |e| ln 2) + 2 u w_j exp(t |e| ln 2) + 2^-126
          and the k additions of a class's sum (adding 0 for another class is exact):  k u / (1 - k u) times the sum of the
          (w_j + |delta w_j|) of the class.  With ``sim_err`` (a bound of every nn_sim against the TRUE similarity) the exponent
          is further off by (err_j + err_1) / T: the bound of the kernel's scores against the oracle's on the same neighbours.
Which voxels' labels must agree with the oracle (``unclear``): a voxel is left out only if its fp64 top-two score margin is within
twice the score bound (sim errors included) plus, when a sample outside the oracle's k neighbours lies within the two sim
bounds of the k-th neighbour, twice the k-th weight (the k-th neighbour may then be another sample, which moves w_k from one
class to another).  The share left out is capped at 2 % per case (``MAX_UNCLEAR``): a condition on the data, checked on the
CPU for the oracle alone (tests/test_knn_cpu.py) and again with the norms of the GPU run.
"""
import numpy as np

from vit_tf_amd import knn
import svm_data
from pca_data import planted_int

U = 2.0 ** -24
MAX_UNCLEAR = 0.02
REAL_CASES = svm_data.REAL_CASES
NORM_CASE = svm_data.NORM_CASE
REAL_KS = (1, 20, 32)
REAL_WEIGHTS = (('softmax', 0.07), ('softmax', 1.0), ('uniform', 0.07))
_cases = {}


def half_of(index):
    """The lane half that holds bank row `index`: rows 4 i .. 4 i + 3 of a chunk of 32 lie in half i % 2."""
    return (np.asarray(index) >> 2) & 1


def real_case(F, classes, per_class, nvox):
    """(bank fp16 [S][F], bank_class uint8 [S], x fp16 [F][nvox]) of a real-valued case: built once per process and shared."""
    key = (F, classes, per_class, nvox)
    if key not in _cases:
        xs, t, _ = svm_data.planted(F, classes, per_class, seed=F + classes)
        x, _ = svm_data.voxels(F, classes, nvox, seed=F + classes)
        m = knn.fit(xs, t, k=1)
        x.setflags(write=False)                                # (the tests upload copies)
        _cases[key] = (m.bank, m.bank_class, x)
    return _cases[key]


def model_of(bank, bank_class, classes, k, weights='softmax', temperature=0.07):
    return knn.KnnModel(bank, bank_class, k, temperature, weights, [str(i) for i in range(classes)], np.arange(classes))


def int_case(n_bank, nvox, F, classes, seed):
    """(bank fp16 [n_bank][F] of integers in -3..3, bank_class uint8 ascending, x fp16 [F][nvox] of integers |x| <= 8): some
    rows are copies of a row of the other lane half and, where there is one, of another class."""
    rng = np.random.default_rng(seed)
    bank = rng.integers(-3, 4, size=(n_bank, F)).astype(np.float64)
    cls = np.sort(rng.integers(0, classes, size=n_bank)).astype(np.uint8)
    rows = np.arange(n_bank)
    for i in rng.permutation(n_bank)[:max(1, n_bank // 8)]:
        other = rows[half_of(rows) != half_of(i)]
        if other.size:
            pick = other[cls[other] != cls[i]] if (cls[other] != cls[i]).any() else other
            bank[rng.choice(pick)] = bank[i]
    x = planted_int(F, nvox, seed=seed + 1)
    return bank.astype(np.float16), cls, x.astype(np.float16)


def similarities(bank, x, voxel_norm=None):
    """fp64 [S][nvox]."""
    sim = np.asarray(bank, np.float64) @ np.asarray(x, np.float64)
    return sim if voxel_norm is None else sim / np.asarray(voxel_norm, np.float64)[None, :]


def weights_of(nn_sim, weights, temperature):
    nn_sim = np.asarray(nn_sim, np.float64)
    return np.ones_like(nn_sim) if weights == 'uniform' else np.exp((nn_sim - nn_sim[:1]) / temperature)


def scores_of(nn_sim, nn_class, classes, weights, temperature):
    """fp64 [C][nvox]: the formula on given neighbours (nn_sim [k][nvox], nn_class [k][nvox])."""
    w = weights_of(nn_sim, weights, temperature)
    return np.stack([np.where(nn_class == c, w, 0.0).sum(0) for c in range(classes)])


def oracle(bank, bank_class, classes, k, x, voxel_norm=None, weights='softmax', temperature=0.07, sim=None):
    """(labels uint8 [nvox], scores fp64 [C][nvox], nn_index int64 [k][nvox], nn_sim fp64 [k][nvox]), evaluated literally."""
    if sim is None:
        sim = similarities(bank, x, voxel_norm)
    nn_index = np.argsort(-sim, axis=0, kind='stable')[:k]
    nn_sim = np.take_along_axis(sim, nn_index, 0)
    scores = scores_of(nn_sim, np.asarray(bank_class)[nn_index], classes, weights, temperature)
    return np.argmax(scores, 0).astype(np.uint8), scores, nn_index, nn_sim


def sim_bound(bank, x, voxel_norm=None):
    """fp64 [S][nvox]: the bound of every similarity the kernel forms."""
    F = bank.shape[1]
    g = (F + 12) * U / (1.0 - (F + 12) * U)
    mag = np.abs(np.asarray(bank, np.float64)) @ np.abs(np.asarray(x, np.float64))
    if voxel_norm is not None:
        mag = mag / np.asarray(voxel_norm, np.float64)[None, :]
    return g * mag + 2.0 ** -126


def score_bound(nn_sim, nn_class, classes, weights, temperature, sim_err=None):
    """fp64 [C][nvox]: the bound of the kernel's scores against scores_of on the same neighbours (module docstring)."""
    nn_sim = np.asarray(nn_sim, np.float64)
    k = nn_sim.shape[0]
    if weights == 'uniform':
        return np.zeros((classes, nn_sim.shape[1]))
    w = weights_of(nn_sim, weights, temperature)
    t = 4 * U / (1 - 4 * U)
    de = t * np.abs(nn_sim - nn_sim[:1]) / temperature                      # in natural units: |e| ln 2 = |s_j - s_1| / T
    if sim_err is not None:
        de = de + (sim_err + sim_err[:1]) / temperature
    dw = w * np.expm1(de) + 2 * U * w * np.exp(de) + 2.0 ** -126
    dw[0] = 0.0                                                             # w_1 = exp2(0) = 1 exactly, on both sides
    out = []
    for c in range(classes):
        mine = nn_class == c
        out.append(np.where(mine, dw, 0.0).sum(0) + k * U / (1 - k * U) * np.where(mine, w + dw, 0.0).sum(0))
    return np.stack(out)


def unclear(bank, bank_class, classes, k, x, voxel_norm, weights, temperature, sim=None, bnd=None):
    """(bool [nvox], oracle labels): the voxels whose label may legitimately differ from the oracle's (module docstring)."""
    sim = similarities(bank, x, voxel_norm) if sim is None else sim
    bnd = sim_bound(bank, x, voxel_norm) if bnd is None else bnd
    labels, scores, nn_index, nn_sim = oracle(bank, bank_class, classes, k, x, voxel_norm, weights, temperature, sim=sim)
    nn_err = np.take_along_axis(bnd, nn_index, 0)
    sb = score_bound(nn_sim, np.asarray(bank_class)[nn_index], classes, weights, temperature, sim_err=nn_err)
    top2 = np.sort(scores, axis=0)[-2:]
    margin = top2[1] - top2[0]
    outside = np.ones(sim.shape, bool)
    np.put_along_axis(outside, nn_index, False, 0)
    near = (outside & (sim + bnd >= (nn_sim[-1] - nn_err[-1])[None, :])).any(0)          # within the two bounds of the k-th
    wk = weights_of(nn_sim, weights, temperature)[-1]
    allowance = 2.0 * sb.max(0) + np.where(near, 2.0 * wk, 0.0)
    return (margin <= allowance) & (allowance > 0), labels            # (an exact tie of exact scores is decided by the rule)
