"""Random-forest classification of a feature volume from annotated voxels: the second learned classifier beside svm.py, the
counterpart of scikit-learn's RandomForestClassifier as the reference's baseline uses it.

``fit`` is host work over a few thousand samples: CART with Gini impurity in numpy, fp64 bookkeeping, the samples rounded to
fp16 first.  It is much slower than scikit-learn's Cython (seconds per hundred trees at 3000 x 384 with 'sqrt', far longer with
'all'); ``from_sklearn`` takes a forest fitted there instead.  ``predict`` is the pass over the volume -- every voxel walks every
tree -- libvittf's vittf_forest_decide (forest.hip).  There is no CPU path for it.  scikit-learn is not imported anywhere.

Three rules make the forest exact and safe:
  * thresholds are fp16, rounded towards -inf: the features are fp16, and for an fp16 x and any real t, x <= t exactly when
    x <= floor16(t), the largest fp16 <= t.  A forest fitted in fp32 or fp64 converts without changing a decision.  The
    comparison is numeric (-0 == +0; +-inf thresholds are allowed); feature volumes must be finite.
  * leaves hold fixed-point class shares, value[c] = floor(p_c 65535 + 0.5) as uint16; a voxel's vote for class c is the uint32
    sum of value[leaf_t][c] over the trees (at most 4096 x 65535 < 2^32) and its label the arg-max, the lowest class index
    among equal votes: scikit-learn's soft vote (predict_proba averaged, first maximum) in integers.  For fully grown trees
    every value is 0 or 65535 and the vote IS clf.predict; with impure leaves the two can differ only where the averaged
    top-two margin is below 1 / 65535.
  * trees are stored in topological order (left > i and right > i for every inner node i) and the walk is bounded by
    max_depth, the depth of the deepest tree: validate() refuses everything else on the host, before any upload.
"""
import numpy as np
import torch

from . import _classify, _lib
from ._classify import round_samples, sample                        # noqa: F401  (the training rows of every classifier)

FORMAT = 'vittf-forest-1'


def floor16(t):
    """fp16 array: the largest fp16 <= t for every real t (fp64; +-inf stay; values beyond +-65504 give 65504 / -inf).
    ValueError for NaN."""
    t = np.asarray(t, np.float64)
    if np.isnan(t).any():
        raise ValueError('a threshold is NaN')
    with np.errstate(over='ignore'):
        h = t.astype(np.float16)
        below = np.nextafter(h, np.float16(-np.inf))
    return np.where(h.astype(np.float64) > t, below, h).astype(np.float16)


def fixed_point(p):
    """uint16: floor(p 65535 + 0.5) of class shares p in [0, 1]."""
    return np.floor(np.asarray(p, np.float64) * 65535.0 + 0.5).astype(np.uint16)


class ForestModel:
    """A fitted (or imported) forest as plain arrays, the trees concatenated:
      class_names [C] str, labels uint8 [C] (the value a label volume carries for each class, ascending), n_features
      tree_offset int64 [T + 1]: tree t owns the nodes tree_offset[t] .. tree_offset[t + 1] - 1, the first is its root
      feature int32 [nodes] (-1 marks a leaf), threshold fp16 [nodes] (a voxel goes left when x[feature] <= threshold)
      left, right int32 [nodes] (indices inside the tree; -1 at a leaf), value uint16 [nodes][C] (fixed_point of the class
      shares of the training rows that reached the node)
      fit statistics: fit_time (seconds, 0 for an imported model).
    The constructor validates (see validate)."""
    ARRAYS = ('format', 'class_names', 'labels', 'n_features', 'tree_offset', 'feature', 'threshold', 'left', 'right', 'value',
              'fit_time')
    normalize = False                                                 # thresholds on single features: no geometry to normalise

    def __init__(self, class_names, labels, n_features, tree_offset, feature, threshold, left, right, value, fit_time=0.0):
        self.class_names = [str(n) for n in class_names]
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        self.n_features = int(n_features)
        self.tree_offset = np.ascontiguousarray(tree_offset, dtype=np.int64).reshape(-1)
        self.feature = np.ascontiguousarray(feature, dtype=np.int32).reshape(-1)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float16).reshape(-1)
        self.left = np.ascontiguousarray(left, dtype=np.int32).reshape(-1)
        self.right = np.ascontiguousarray(right, dtype=np.int32).reshape(-1)
        self.value = np.ascontiguousarray(value, dtype=np.uint16)
        self.fit_time = float(fit_time)
        self.max_depth = self.validate()

    @property
    def classes(self):
        return int(self.labels.size)

    @property
    def trees(self):
        return int(self.tree_offset.size - 1)

    @property
    def n_nodes(self):
        return int(self.feature.size)

    def validate(self):
        """The depth of the deepest tree; ValueError unless the arrays describe 1..4096 proper binary trees of at most 65535
        nodes and depth 64 over 2..8 classes, every inner node's children behind it and inside its tree, every node but the
        roots the child of exactly one node, features in 0..F-1, no NaN threshold.  What passes cannot make a walk leave its
        tree or run longer than the depth returned."""
        c, f = self.classes, self.n_features
        _classify.check_classes(self.class_names, self.labels, _lib.FOREST_MAX_CLASSES)
        _classify.check_f(f)
        off = self.tree_offset
        t = off.size - 1
        if not 1 <= t <= _lib.FOREST_MAX_TREES:
            raise ValueError(f'trees must number 1..{_lib.FOREST_MAX_TREES}, got {t}')
        n = self.feature.size
        sizes = np.diff(off)
        if off[0] != 0 or off[-1] != n or (sizes < 1).any():
            raise ValueError('tree_offset must ascend strictly from 0 to the number of nodes')
        if sizes.max() > _lib.FOREST_MAX_NODES:
            raise ValueError(f'a tree has {int(sizes.max())} nodes, more than {_lib.FOREST_MAX_NODES}')
        if not (self.threshold.shape == self.left.shape == self.right.shape == (n,)) or self.value.shape != (n, c):
            raise ValueError(f'feature, threshold, left, right must be [{n}] and value [{n}][{c}]')
        inner = self.feature >= 0
        if (self.feature[inner] >= f).any() or (self.feature < -1).any():
            raise ValueError(f'a feature index is outside 0..{f - 1} (-1 marks a leaf)')
        if np.isnan(self.threshold[inner]).any():
            raise ValueError('a threshold is NaN')
        tree = np.repeat(np.arange(t), sizes)
        local = np.arange(n) - off[tree]
        for name, child in (('left', self.left), ('right', self.right)):
            ch = child[inner].astype(np.int64)
            if (ch <= local[inner]).any():
                raise ValueError(f'a {name} child index is not larger than its parent: the trees must be in topological order')
            if (ch >= sizes[tree[inner]]).any():
                raise ValueError(f'a {name} child index is outside its tree')
        kids = np.concatenate([self.left[inner].astype(np.int64) + off[tree[inner]], self.right[inner].astype(np.int64) + off[tree[inner]]])
        parents = np.bincount(kids, minlength=n)
        expect = np.ones(n, np.int64)
        expect[off[:-1]] = 0
        if not np.array_equal(parents, expect):
            raise ValueError('every node but a root must be the child of exactly one node')
        # depth: level by level from the roots (every node is reached once: the loop ends after the deepest level)
        frontier = off[:-1].copy()
        depth = 0
        while True:
            fi = frontier[inner[frontier]]
            if fi.size == 0:
                break
            depth += 1
            if depth > _lib.FOREST_MAX_DEPTH:
                raise ValueError(f'a tree is deeper than {_lib.FOREST_MAX_DEPTH}')
            frontier = np.concatenate([self.left[fi] + off[tree[fi]], self.right[fi] + off[tree[fi]]])
        return depth

    def decide_slab(self, x, want_extra):
        """(labels, the uint32 votes [C][n] or None) of the (F, n) matrix x."""
        return decide(x, self, want_extra)


# ---------------------------------------------------------------------------------------------- the fit (fp64, host)
def _n_candidates(max_features, f):
    if isinstance(max_features, str):
        if max_features == 'sqrt':
            return max(1, int(np.sqrt(f)))
        if max_features == 'all':
            return f
        raise ValueError(f"max_features must be 'sqrt', 'all', an int or a fraction, got {max_features!r}")
    if max_features is None:
        return f
    if isinstance(max_features, (int, np.integer)) and not isinstance(max_features, bool):
        if not 1 <= max_features <= f:
            raise ValueError(f'max_features must be in 1..{f}, got {max_features}')
        return int(max_features)
    if isinstance(max_features, (float, np.floating)) and 0.0 < max_features <= 1.0:
        return max(1, int(max_features * f))
    raise ValueError(f"max_features must be 'sqrt', 'all', an int in 1..F or a fraction in (0, 1], got {max_features!r}")


def _best_split(cols, onehot, feats, min_leaf):
    """The best split of the node's rows among the ascending feature indices `feats`, cols [n][k] their columns: (feature, threshold fp64) or
    None when no feature separates two rows with min_leaf rows on either side.  Per feature: sort, cumulative class counts,
    maximise sum_c L_c^2 / n_L + sum_c R_c^2 / n_R (the Gini decrease up to constants of the node); the first maximum in
    (feature, threshold) order wins."""
    n = cols.shape[0]
    order = np.argsort(cols, axis=0, kind='stable')
    xs = np.take_along_axis(cols, order, axis=0)
    lc = np.cumsum(onehot[order], axis=0)[:-1]                       # [n-1][k][C]: the classes of the first i + 1 rows
    nl = np.arange(1, n, dtype=np.float64)[:, None]
    nr = n - nl
    total = lc[-1] + onehot[order[-1]]                               # [k][C]
    score = (lc * lc).sum(2) / nl + ((total - lc) ** 2).sum(2) / nr
    ok = (xs[1:] > xs[:-1]) & (nl >= min_leaf) & (nr >= min_leaf)
    if not ok.any():
        return None
    score = np.where(ok, score, -np.inf).T                           # [k][n-1]: feature-major, thresholds ascending
    j, i = np.unravel_index(int(np.argmax(score)), score.shape)
    return int(feats[j]), (xs[i, j] + xs[i + 1, j]) / 2.0


def _grow(x, y, c, k, max_depth, min_leaf, rng):
    """One tree on the rows x [n][F] (fp64 copies of fp16 values), classes y in 0..c-1: lists (feature, threshold fp64, left,
    right, counts) in creation order, children created behind their parent."""
    f = x.shape[1]
    eye = np.eye(c)
    feature, threshold, left, right, counts = [-1], [0.0], [-1], [-1], [None]
    stack = [(0, np.arange(x.shape[0]), 0)]
    while stack:
        node, idx, depth = stack.pop()
        yn = y[idx]
        cnt = np.bincount(yn, minlength=c)
        counts[node] = cnt
        if cnt.max() == idx.size or idx.size < 2 * min_leaf or idx.size < 2 or (max_depth is not None and depth >= max_depth):
            continue
        perm = rng.permutation(f)
        split = None
        for s in range(0, f, k):                                     # keep drawing while every drawn feature is constant here
            feats = np.sort(perm[s:s + k])
            cols = x[np.ix_(idx, feats)]
            varies = cols.max(0) > cols.min(0)
            if varies.any():
                split = _best_split(cols[:, varies], eye[yn], feats[varies], min_leaf)
                break
        if split is None:
            continue
        go_left = x[idx, split[0]] <= split[1]
        l, r = len(feature), len(feature) + 1
        for lst, fill in ((feature, -1), (threshold, 0.0), (left, -1), (right, -1), (counts, None)):
            lst += [fill, fill]
        feature[node], threshold[node], left[node], right[node] = split[0], split[1], l, r
        stack.append((r, idx[~go_left], depth + 1))
        stack.append((l, idx[go_left], depth + 1))
    return feature, threshold, left, right, np.asarray(counts, np.float64)


def fit(samples, targets, trees=256, max_features='sqrt', max_depth=None, min_samples_leaf=1, bootstrap=True, seed=0,
        class_names=None):
    """ForestModel of `trees` CART trees (Gini) on samples [n][F] with integer targets [n] (label values 0..255; the classes
    are their distinct values, ascending).  The samples are rounded to fp16 first.  Tree t draws from its own stream
    np.random.default_rng([seed, t]) -- its bootstrap rows (n draws with replacement) and, at every node, max_features
    candidate features without replacement ('sqrt', 'all', an int, or a fraction of F), drawing on while all drawn ones are
    constant on the node -- so a tree does not depend on how many are built, and the same seed gives the same bytes.  A split
    is the best Gini decrease, the lowest feature and then the lowest threshold among equals; the threshold the midpoint of
    the two neighbouring values, then floor16.  Slower than scikit-learn's Cython: model.fit_time reports the seconds."""
    import time
    t0 = time.time()
    x16 = round_samples(samples)
    x = x16.astype(np.float64)
    n, f = x.shape
    values, y, names = _classify.class_table(targets, class_names, n, _lib.FOREST_MAX_CLASSES, f)
    c = values.size
    if not 1 <= int(trees) <= _lib.FOREST_MAX_TREES:
        raise ValueError(f'trees must number 1..{_lib.FOREST_MAX_TREES}, got {trees}')
    if max_depth is not None and not 1 <= int(max_depth) <= _lib.FOREST_MAX_DEPTH:
        raise ValueError(f'max_depth must be in 1..{_lib.FOREST_MAX_DEPTH} or None, got {max_depth}')
    if not int(min_samples_leaf) >= 1:
        raise ValueError(f'min_samples_leaf must be at least 1, got {min_samples_leaf}')
    k = _n_candidates(max_features, f)
    _classify.check_names(names, c)
    parts = []
    for tr in range(int(trees)):
        rng = np.random.default_rng([int(seed), tr])
        rows = rng.integers(0, n, size=n) if bootstrap else np.arange(n)
        parts.append(_grow(x[rows], y[rows], c, k, None if max_depth is None else int(max_depth), int(min_samples_leaf), rng))
    return _assemble(parts, names, values, f, time.time() - t0)


def _assemble(parts, names, labels, f, fit_time=0.0):
    """ForestModel of per-tree (feature, threshold fp64, left, right, class weights [nodes][C]) in topological order."""
    off = np.concatenate(([0], np.cumsum([len(p[0]) for p in parts])))
    w = np.concatenate([np.asarray(p[4], np.float64).reshape(len(p[0]), -1) for p in parts])
    tot = w.sum(1, keepdims=True)
    if (w < 0).any() or (tot <= 0).any():
        raise ValueError('the class weights of a node are negative or all zero')
    feature = np.concatenate([np.asarray(p[0], np.int64) for p in parts])
    thr = floor16(np.concatenate([np.asarray(p[1], np.float64) for p in parts]))
    thr[feature < 0] = 0
    return ForestModel(names, labels, f, off, np.maximum(feature, -1), thr, np.concatenate([np.asarray(p[2], np.int64) for p in parts]),
                       np.concatenate([np.asarray(p[3], np.int64) for p in parts]), fixed_point(w / tot), fit_time)


def _topological(feature, threshold, left, right, value):
    """The tree's arrays re-ordered breadth-first from node 0 when a child index is not larger than its parent's."""
    inner = left >= 0
    idx = np.arange(left.size)
    if (left[inner] > idx[inner]).all() and (right[inner] > idx[inner]).all():
        return feature, threshold, left, right, value
    order, seen = [0], {0}
    for i in order:                                                  # (grows while it is walked)
        if left[i] >= 0:
            for ch in (int(left[i]), int(right[i])):
                if ch in seen or len(order) > left.size:
                    raise ValueError('a tree of the forest is not a tree')
                seen.add(ch)
                order.append(ch)
    order = np.asarray(order)
    new = np.full(left.size, -1, np.int64)
    new[order] = np.arange(order.size)
    remap = lambda ch: np.where(ch[order] >= 0, new[np.maximum(ch[order], 0)], -1)           # noqa: E731
    return feature[order], threshold[order], remap(left), remap(right), value[order]


def from_tree_arrays(trees, n_features, class_names=None, labels=None):
    """ForestModel from the public arrays of scikit-learn's ``tree_`` objects: `trees` is a sequence of (children_left,
    children_right, feature, threshold, value) with value [nodes][C] or [nodes][1][C] (class shares, or counts as older
    versions store them; a leaf has children_left == -1).  floor16 on the thresholds, value rows normalised, nodes re-ordered
    where a child does not come behind its parent."""
    parts = []
    for cl, cr, feat, thr, val in trees:
        cl, cr = np.asarray(cl, np.int64).reshape(-1), np.asarray(cr, np.int64).reshape(-1)
        val = np.asarray(val, np.float64)
        val = val.reshape(val.shape[0], -1)
        leaf = cl < 0
        feat = np.where(leaf, -1, np.asarray(feat, np.int64).reshape(-1))
        thr = np.where(leaf, 0.0, np.asarray(thr, np.float64).reshape(-1))
        parts.append(_topological(feat, thr, np.where(leaf, -1, cl), np.where(leaf, -1, cr), val))
    if not parts:
        raise ValueError('the forest has no trees')
    c = parts[0][4].shape[1]
    values = np.arange(c) if labels is None else np.asarray(labels).reshape(-1)
    names = [str(v) for v in values] if class_names is None else class_names
    return _assemble(parts, names, values, int(n_features))


def from_sklearn(clf, class_names=None, labels=None):
    """ForestModel of a fitted RandomForestClassifier / ExtraTreesClassifier, or of anything with ``estimators_[i].tree_``
    (only those public arrays are read; nothing is imported).  labels: the label value of each class, default ``clf.classes_``
    when those are integers in 0..255, else 0..C-1.  On fp16-valued rows the model's vote equals clf.predict exactly for fully
    grown trees (see the module's text for impure leaves)."""
    trees = [(e.tree_.children_left, e.tree_.children_right, e.tree_.feature, e.tree_.threshold, e.tree_.value) for e in clf.estimators_]
    if labels is None:
        cls = np.asarray(getattr(clf, 'classes_', []))
        if cls.size and np.issubdtype(cls.dtype, np.integer) and cls.min() >= 0 and cls.max() <= 255:
            labels = cls
    return from_tree_arrays(trees, int(clf.estimators_[0].tree_.n_features), class_names, labels)


# ---------------------------------------------------------------------------------------------- files
def save_model(model, path):
    """An .npz holding exactly ForestModel.ARRAYS as plain arrays (no pickled objects)."""
    arrays = {'format': np.asarray(FORMAT), 'class_names': np.asarray(model.class_names, dtype=np.str_), 'labels': model.labels,
              'n_features': np.asarray(model.n_features, np.int64), 'tree_offset': model.tree_offset, 'feature': model.feature,
              'threshold': model.threshold, 'left': model.left, 'right': model.right, 'value': model.value,
              'fit_time': np.asarray(model.fit_time, np.float64)}
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def is_forest_file(path):
    """True when `path` is an .npz that names itself a forest model (the command line picks the classifier of --model by it)."""
    return _classify.file_format(path) == FORMAT


def load_model(path):
    """The ForestModel of a file save_model wrote; ValueError for anything else (an SVM model file, a missing key, arrays that
    validate() refuses, another .npz, a .npy, a damaged file)."""
    dtypes = {'labels': np.uint8, 'tree_offset': np.int64, 'feature': np.int32, 'threshold': np.float16, 'left': np.int32,
              'right': np.int32, 'value': np.uint16}
    svm_file = (('sv', 'pair_coef'), 'is an SVM model file, not a forest (vt.svm.load_model reads it)')
    with _classify.open_model(path, 'a forest model', ForestModel.ARRAYS, dtypes, foreign=svm_file) as z:
        if str(z['format'][()]) != FORMAT:
            raise ValueError(f"format {str(z['format'][()])!r} is not {FORMAT!r}")
        return ForestModel(_classify.names_of(z), z['labels'], int(z['n_features']), z['tree_offset'], z['feature'], z['threshold'],
                           z['left'], z['right'], z['value'], float(z['fit_time']))


# ---------------------------------------------------------------------------------------------- the GPU pass
def pack(model):
    """(nodes uint32 [nodes][2], leaf_values uint16 [leaves][8], tree_offset uint32 [T + 1]) as vittf_forest_decide takes them
    (include/vittf.h): an inner node is {feature | threshold bits << 16, left | right << 16}, a leaf {0xFFFF, its row in
    leaf_values}; the leaves are numbered in node order."""
    leaf = model.feature < 0
    nodes = np.empty((model.n_nodes, 2), np.uint32)
    thr = model.threshold.view(np.uint16).astype(np.uint32)
    nodes[:, 0] = np.where(leaf, 0xFFFF, model.feature.astype(np.uint32) | (thr << 16))
    rows = np.cumsum(leaf) - 1
    nodes[:, 1] = np.where(leaf, rows, model.left.astype(np.uint32) | (model.right.astype(np.uint32) << 16))
    values = np.zeros((int(leaf.sum()), 8), np.uint16)
    values[:, :model.classes] = model.value[leaf]
    return nodes, values, model.tree_offset.astype(np.uint32)


def decide(x, model, want_votes=False):
    """(labels uint8 [nvox], votes uint32 [C][nvox] or None) on the device for the (F, nvox) fp16 device matrix `x`: one
    vittf_forest_decide call."""
    lib = _lib.require_device()
    f, nvox = x.shape
    _classify.check_model_f(f, model)
    dev = x.device
    nodes, values, off = (torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int16)).to(dev) for a in pack(model))
    labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
    votes = torch.empty((model.classes, nvox), dtype=torch.uint32, device=dev) if want_votes else None
    with torch.cuda.device(dev):
        _lib.check(lib.vittf_forest_decide(_lib.ptr(x), f, nvox, _lib.ptr(nodes), _lib.ptr(values), _lib.ptr(off), model.trees,
                                           model.classes, model.max_depth, _lib.ptr(labels), _lib.ptr(votes), _lib.stream_ptr()),
                   'vittf_forest_decide')
    return labels, votes


def predict(feat, model, return_votes=False):
    """uint8 device tensor with the voxel shape of `feat` (F, W', H', D'): the class INDEX 0..C-1 of every voxel
    (model.labels[index] is the value a label volume carries); with return_votes also the uint32 [C] + voxel shape votes,
    each at most trees x 65535."""
    return _classify.predict_volume(feat, model, lambda x, m, vn: decide(x, m, return_votes), False)
