"""Weighted k-nearest-neighbour classification of a feature volume from annotated voxels: the k-NN of the DINO evaluation
protocol (Caron et al. 2021, after Wu et al. 2018) -- cosine similarity, the k = 20 nearest labelled samples, weights
exp(sim / 0.07), the arg-max of the per-class sums.  The learned counterpart of predict_ntf.py's "mean similarity to the
annotations" rule: it keeps the closest annotations instead of averaging all of them.

There is NO fit: the model is the bank of annotated samples itself (L2-normalised in fp64, rounded once to fp16, sorted by
class), so adding or removing an annotation reclassifies the volume at the cost of one pass.  ``predict`` is that pass: every
voxel against every bank sample on the matrix cores and a per-voxel top-k in registers -- libvittf's vittf_knn_decide
(knn.hip).  There is no CPU path for it.

Conventions (those of the C entry): classes are numbered 0..C-1 in ascending order of their label value; sim = bank_s . x_v /
|x_v| in fp32; the neighbours are the k samples that come first under "larger sim first, then lower sample index", rank 1 the
nearest; w_j = 1 ('uniform') or exp((sim_j - sim_1) / T) ('softmax': the common factor exp(sim_1 / T) of the protocol's
weights is divided out, which changes no arg-max and cannot overflow); scores[c] = the sum of w_j over the ranks of class c in
rank order; the label is the arg-max, the lowest class among equal scores.  scikit-learn is not imported anywhere.
"""
import numpy as np
import torch

from . import _classify, _lib
from ._classify import round_samples, sample                         # noqa: F401  (sample: the one of every classifier)

FORMAT = 'vittf-knn-1'
WEIGHTS = ('softmax', 'uniform')


class KnnModel:
    """A bank of labelled samples as plain arrays:
      bank fp16 [S][F] (the rows as the kernel multiplies them), bank_class uint8 [S] (0..C-1, ascending)
      k (1..32, at most S), temperature (> 0), weights 'softmax' | 'uniform'
      class_names [C] str, labels uint8 [C] (the value a label volume carries for each class, ascending)."""
    ARRAYS = ('format', 'bank', 'bank_class', 'k', 'temperature', 'weights', 'class_names', 'labels')
    normalize = True                                                  # the geometry is always cosine

    def __init__(self, bank, bank_class, k, temperature, weights, class_names, labels):
        self.bank = np.ascontiguousarray(bank, dtype=np.float16)
        self.bank_class = np.ascontiguousarray(bank_class, dtype=np.uint8).reshape(-1)
        self.k, self.temperature, self.weights = int(k), float(temperature), str(weights)
        self.class_names = [str(n) for n in class_names]
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        self._check()

    @property
    def classes(self):
        return int(self.labels.size)

    @property
    def n_features(self):
        return int(self.bank.shape[1])

    @property
    def n_bank(self):
        return int(self.bank.shape[0])

    @property
    def inv_temperature(self):
        """What vittf_knn_decide is given: 0 for uniform weights, else fl32(1 / T)."""
        return 0.0 if self.weights == 'uniform' else float(np.float32(1.0 / self.temperature))

    def _check(self):
        c = self.classes
        if self.weights not in WEIGHTS:
            raise ValueError(f'weights must be one of {WEIGHTS}, got {self.weights!r}')
        _classify.check_classes(self.class_names, self.labels, _lib.KNN_MAX_CLASSES)
        if self.bank.ndim != 2:
            raise ValueError(f'bank must be [S][F], got {self.bank.shape}')
        s, f = self.bank.shape
        if not 1 <= s <= _lib.KNN_MAX_BANK:
            raise ValueError(f'bank samples must number 1..{_lib.KNN_MAX_BANK}, got {s}')
        _classify.check_f(f, 768, ': reduce the volume first (reduce_features.py)')
        if not np.isfinite(self.bank).all():
            raise ValueError('a bank sample is not finite in fp16')
        if self.bank_class.shape != (s,) or np.any(np.diff(self.bank_class.astype(np.int64)) < 0) or self.bank_class.max() >= c:
            raise ValueError('bank_class must hold the class 0..C-1 of every bank sample, ascending')
        if not 1 <= self.k <= _lib.KNN_MAX_K:
            raise ValueError(f'k must be in 1..{_lib.KNN_MAX_K}, got {self.k}')
        if self.k > s:
            raise ValueError(f'k = {self.k} is more than the {s} samples of the bank')
        if not (np.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError(f'temperature must be positive and finite, got {self.temperature}')
        if self.weights == 'softmax':
            with np.errstate(over='ignore'):
                c32 = np.float32(np.float64(np.float32(1.0 / self.temperature)) * 1.4426950408889634074)
            if not (np.isfinite(c32) and c32 > 0):
                raise ValueError(f'temperature {self.temperature} leaves the fp32 range as log2(e) / T')


def fit(samples, targets, k=20, temperature=0.07, weights='softmax', class_names=None):
    """KnnModel on samples [n][F] with integer targets [n] (label values 0..255; the classes are their distinct values,
    ascending).  No optimisation: the samples are L2-normalised in fp64, rounded once to fp16 and sorted by class (in sample
    order inside a class).  k is clipped to n, with a printed note.  Deterministic."""
    x16 = round_samples(samples, normalize=True)
    n = x16.shape[0]
    values, index, names = _classify.class_table(targets, class_names, n)
    _classify.check_names(names, values.size)
    k = int(k)
    if 1 <= n < k:
        print(f'Note: k = {k} is more than the {n} samples of the bank: using k = {n}')
        k = n
    order = np.argsort(index, kind='stable')
    return KnnModel(x16[order], index[order], k, temperature, weights, names, values)


# ---------------------------------------------------------------------------------------------- files
def save_model(model, path):
    """An .npz holding exactly KnnModel.ARRAYS as plain arrays (no pickled objects), format = 'vittf-knn-1'."""
    arrays = {'format': np.asarray(FORMAT), 'bank': model.bank, 'bank_class': model.bank_class, 'k': np.asarray(model.k, np.int64),
              'temperature': np.asarray(model.temperature, np.float64), 'weights': np.asarray(model.weights),
              'class_names': np.asarray(model.class_names, dtype=np.str_), 'labels': model.labels}
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def is_knn_file(path):
    """True when `path` is an .npz that names itself a k-NN bank (the command line picks the classifier of --model by it)."""
    return _classify.file_format(path) == FORMAT


def load_model(path):
    """The KnnModel of a file save_model wrote; ValueError for anything else."""
    dtypes = {'bank': np.float16, 'bank_class': np.uint8, 'labels': np.uint8}
    with _classify.open_model(path, 'a k-NN bank', KnnModel.ARRAYS, dtypes, FORMAT) as z:
        return KnnModel(z['bank'], z['bank_class'], int(z['k']), float(z['temperature']), str(z['weights'][()]), _classify.names_of(z),
                        z['labels'])


# ---------------------------------------------------------------------------------------------- the GPU pass
def decide(x, model, voxel_norm=None, want_scores=False, want_neighbours=False):
    """(labels uint8 [nvox], scores fp32 [C][nvox] or None, nn_index int32 [k][nvox] or None, nn_sim fp32 [k][nvox] or None)
    on the device for the (F, nvox) fp16 device matrix `x`: one vittf_knn_decide call."""
    lib = _lib.require_device()
    f, nvox = x.shape
    _classify.check_model_f(f, model, 'the bank holds')
    model._check()                                     # bank_class < classes: the C entry trusts it
    dev = x.device
    c, k, s = model.classes, model.k, model.n_bank
    labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
    scores = torch.empty((c, nvox), dtype=torch.float32, device=dev) if want_scores else None
    nn_index = torch.empty((k, nvox), dtype=torch.int32, device=dev) if want_neighbours else None
    nn_sim = torch.empty((k, nvox), dtype=torch.float32, device=dev) if want_neighbours else None
    vn = _classify.norm_argument(voxel_norm, nvox, dev)
    with torch.cuda.device(dev):
        bank = torch.from_numpy(model.bank).to(dev)
        cls = torch.from_numpy(model.bank_class).to(dev)
        ws_bytes = lib.vittf_knn_workspace_bytes(f, s)
        if ws_bytes == 0:
            raise ValueError(f'vittf_knn_decide refuses F = {f}, {s} bank samples')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.vittf_knn_decide(_lib.ptr(x), f, nvox, _lib.ptr(bank), _lib.ptr(cls), s, c, k, model.inv_temperature,
                                        _lib.ptr(vn), _lib.ptr(labels), _lib.ptr(scores), _lib.ptr(nn_index), _lib.ptr(nn_sim),
                                        _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'vittf_knn_decide')
    return labels, scores, nn_index, nn_sim


def predict(feat, model, return_scores=False):
    """uint8 device tensor with the voxel shape of `feat` (F, W', H', D'): the class INDEX 0..C-1 of every voxel
    (model.labels[index] is the value a label volume carries); with return_scores also the fp32 [C] + voxel shape scores the
    arg-max was taken over.  The voxels are divided by their norms (vt.similarity.voxel_norms): the geometry is cosine."""
    return _classify.predict_volume(feat, model, lambda x, m, vn: decide(x, m, vn, want_scores=return_scores)[:2], True)


def probabilities(scores):
    """uint8, the shape of `scores` [C][...]: floor(255 score_c / sum_c score + 0.5) (the scores are positive: w_1 = 1)."""
    s = scores.double()
    return torch.floor(255.0 * s / s.sum(0, keepdim=True) + 0.5).to(torch.uint8)
