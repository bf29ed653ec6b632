"""The test side's own statement of what a forest computes, independent of vit_tf_amd.forest: a numpy walk of the plain
arrays (votes and labels), floor16 by table look-up, builders of synthetic forests as arrays (not fitted), and planted data.

A forest here is a dict of the arrays ForestModel keeps: tree_offset int64 [T + 1], feature int32 [nodes] (-1: leaf), threshold
fp16 [nodes], left / right int32 [nodes] (indices inside the tree), value uint16 [nodes][C].
"""
import numpy as np

_BITS = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
ALL_FINITE_F16 = _BITS[np.isfinite(_BITS)]                           # all 63 488 finite fp16 values (both zeros)
_TABLE = np.sort(_BITS[~np.isnan(_BITS)].astype(np.float64))         # -inf .. +inf, ascending


def floor16(t):
    """The largest fp16 <= t, looked up in the sorted table of all fp16 values (t fp64, not NaN)."""
    t = np.asarray(t, np.float64)
    return _TABLE[np.searchsorted(_TABLE, t, side='right') - 1].astype(np.float16)


def walk(forest, x, max_depth=None):
    """(votes uint64 [C][nvox], labels uint8 [nvox], leaf int64 [T][nvox]: the tree-local node every walk ended on) of the fp16
    matrix x [F][nvox]: at an inner node left when x[feature] <= threshold (fp16 numbers), the vote the sum of the leaves'
    values, the label its first maximum.  max_depth=None walks until every voxel sits on a leaf."""
    x = np.asarray(x)
    assert x.dtype == np.float16
    off = forest['tree_offset']
    trees, nvox = off.size - 1, x.shape[1]
    votes = np.zeros((forest['value'].shape[1], nvox), np.uint64)
    ends = np.zeros((trees, nvox), np.int64)
    cols = np.arange(nvox)
    for t in range(trees):
        node = np.zeros(nvox, np.int64)
        d = 0
        while True:
            g = off[t] + node
            f = forest['feature'][g]
            inner = f >= 0
            if not inner.any() or (max_depth is not None and d >= max_depth):
                break
            go = x[np.maximum(f, 0), cols] <= forest['threshold'][g]
            node = np.where(inner, np.where(go, forest['left'][g], forest['right'][g]), node)
            d += 1
        assert not inner.any(), 'a walk was cut short on an inner node'
        votes += forest['value'][off[t] + node].T.astype(np.uint64)
        ends[t] = node
    return votes, np.argmax(votes, axis=0).astype(np.uint8), ends


def depth_of(forest):
    """The depth of the deepest tree, by following every node's level."""
    off = forest['tree_offset']
    best = 0
    for t in range(off.size - 1):
        n = off[t + 1] - off[t]
        level = np.zeros(n, np.int64)
        for i in range(n):                                           # children come behind their parents
            if forest['feature'][off[t] + i] >= 0:
                level[forest['left'][off[t] + i]] = level[forest['right'][off[t] + i]] = level[i] + 1
        best = max(best, int(level.max()))
    return best


# ---------------------------------------------------------------------------------------------- builders
def random_tree(rng, F, classes, depth, leaves, thresholds=None):
    """One random binary tree of exactly `leaves` leaves and no node deeper than `depth`: a random leaf is split until the
    count is reached.  Thresholds are N(0, 1) rounded to fp16 (or drawn from `thresholds`), values random uint16."""
    assert 1 <= leaves <= 2 ** depth
    feature, thr, left, right, level = [-1], [0.0], [-1], [-1], [0]
    open_leaves = [0]
    n_leaves = 1
    while n_leaves < leaves:
        cand = [i for i in open_leaves if level[i] < depth]
        i = cand[int(rng.integers(len(cand)))]
        open_leaves.remove(i)
        feature[i] = int(rng.integers(F))
        thr[i] = float(rng.standard_normal()) if thresholds is None else float(thresholds[int(rng.integers(len(thresholds)))])
        left[i], right[i] = len(feature), len(feature) + 1
        for _ in range(2):
            feature.append(-1); thr.append(0.0); left.append(-1); right.append(-1); level.append(level[i] + 1)
            open_leaves.append(len(feature) - 1)
        n_leaves += 1
    n = len(feature)
    return dict(feature=np.asarray(feature, np.int32), threshold=np.asarray(thr).astype(np.float16), left=np.asarray(left, np.int32),
                right=np.asarray(right, np.int32), value=rng.integers(0, 65536, size=(n, classes)).astype(np.uint16))


def chain_tree(rng, F, classes, depth, first=0):
    """Every inner node has a leaf as its left child and the next inner node as its right one: depth `depth`, 2 depth + 1 nodes;
    the k-th inner node tests feature (first + k) % F against a threshold in (-1, 1).  A voxel whose every feature is above
    every threshold reaches the deepest leaf."""
    n = 2 * depth + 1
    feature, left, right = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    thr = np.zeros(n, np.float16)
    for k in range(depth):
        i = 2 * k
        feature[i], left[i], right[i] = (first + k) % F, i + 1, i + 2
        thr[i] = np.float16(rng.uniform(-1, 1))
    return dict(feature=feature, threshold=thr, left=left, right=right, value=rng.integers(0, 65536, size=(n, classes)).astype(np.uint16))


def leaf_tree(values):
    """A tree that is one leaf with the given uint16 values."""
    return dict(feature=np.asarray([-1], np.int32), threshold=np.zeros(1, np.float16), left=np.asarray([-1], np.int32),
                right=np.asarray([-1], np.int32), value=np.asarray(values, np.uint16).reshape(1, -1))


def stump(feature, threshold, left_values, right_values):
    """Root + two leaves; the root's own value row is zeros."""
    c = len(left_values)
    return dict(feature=np.asarray([feature, -1, -1], np.int32), threshold=np.asarray([threshold, 0, 0], np.float16),
                left=np.asarray([1, -1, -1], np.int32), right=np.asarray([2, -1, -1], np.int32),
                value=np.asarray([[0] * c, left_values, right_values], np.uint16))


def forest_of(trees):
    """The concatenation of tree dicts, with tree_offset."""
    out = {k: np.concatenate([t[k] for t in trees]) for k in ('feature', 'threshold', 'left', 'right', 'value')}
    out['tree_offset'] = np.concatenate(([0], np.cumsum([t['feature'].size for t in trees]))).astype(np.int64)
    return out


def random_forest(rng, trees, F, classes, depth=8, leaves=24):
    return forest_of([random_tree(rng, F, classes, depth, int(rng.integers(1, leaves + 1))) for _ in range(trees)])


# ---------------------------------------------------------------------------------------------- planted data
def blobs(n, F, classes, spread, seed, means_seed=0):
    """(x fp16 [n][F], y int64 [n]): class means `spread` N(0, 1) (fixed by means_seed), unit noise."""
    mu = spread * np.random.default_rng(means_seed).standard_normal((classes, F))
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    return (mu[y] + rng.standard_normal((n, F))).astype(np.float16), y
