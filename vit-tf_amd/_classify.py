"""What the classifiers of feature volumes (svm.py, forest.py, mlp.py, knn.py) share on the host: the class table of a fit
and its checks, the training rows (``round_samples``, ``sample``), the .npz model files, and the wrapper around a decision pass
over a whole volume.  Internal: the four modules re-export what tests and tools use.

Every model has ``classes``, ``n_features``, ``normalize``, ``labels`` and ``class_names``; those that can classify a matrix
without voxel norms (all but the k-NN bank, whose geometry is cosine) have ``decide_slab(x, want_extra) -> (labels, extra)``,
which vt.voxel_features streams the hand-crafted features through."""
import contextlib
import zipfile

import numpy as np
import torch

from . import _lib
from ._featvol import _as_matrix, _np, _on_device


# ---------------------------------------------------------------------------------------------- checks
def check_f(f, most=1024, advice=''):
    if f % 32 or not 32 <= f <= most:
        raise ValueError(f'F must be a multiple of 32 in 32..{most}, got {f}{advice}')


def check_classes(class_names, labels, most):
    """A model's class table: 2..most classes, one name each, the label values ascending."""
    c = labels.size
    if not 2 <= c <= most:
        raise ValueError(f'classes must be in 2..{most}, got {c}')
    if len(class_names) != c or np.any(np.diff(labels.astype(np.int64)) <= 0):
        raise ValueError('class_names and labels must hold one entry per class, the labels ascending')


def class_table(targets, class_names, n, most=None, f=None):
    """(values, index, names) of a fit on n samples: the distinct label values of `targets` ascending, the class index
    0..C-1 of every sample, and the class names as text (the values when class_names is None; check_names counts them, where
    the fit has always done so: behind its own argument checks).  ValueError unless there are n targets in 0..255 and (when
    `most` is given) 2..most classes; `f` is checked on the way (check_f)."""
    t = _np(targets, np.int64).reshape(-1)
    if t.size != n:
        raise ValueError(f'{t.size} targets for {n} samples')
    if f is not None:
        check_f(f)
    if n and (t.min() < 0 or t.max() > 255):
        raise ValueError('targets must be label values in 0..255')
    values, index = np.unique(t, return_inverse=True)
    c = values.size
    if most is not None and not 2 <= c <= most:
        raise ValueError(f'classes must be in 2..{most}, got {c}')
    names = [str(v) for v in values] if class_names is None else [str(s) for s in class_names]
    return values, index.reshape(-1), names


def check_names(names, c):
    if len(names) != c:
        raise ValueError(f'{len(names)} class names for {c} classes')


# ---------------------------------------------------------------------------------------------- training rows
def round_samples(samples, normalize=False):
    """The samples as the solver and the kernel see them: fp64 [n][F] -> (divided by max(|row|, 1e-12) when `normalize`) ->
    rounded to fp16."""
    x = _np(samples, np.float64)
    if x.ndim != 2:
        raise ValueError(f'samples must be [n][F], got {x.shape}')
    if normalize:
        x = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    with np.errstate(over='ignore'):
        h = x.astype(np.float16)
    if not np.isfinite(h).all():
        raise ValueError('a sample is not finite in fp16')
    return h


def sample(feat, annotations, volume_shape, normalize=False):
    """(samples fp32 [n][F] device tensor, targets int64 [n] numpy): the features at the annotated voxels, sampled the way
    compute_similarities samples its queries (trilinear, rel = (abs + 0.5) / extent * 2 - 1 in fp32, the voxel norms passed on
    when `normalize`).  annotations: {name: (n, 3) voxel coordinates in the volume of `volume_shape`}; the target of the i-th
    key is i."""
    lib = _lib.require_device()
    from .similarity import _device_features, voxel_norms
    dev = torch.device('cuda', torch.cuda.current_device())
    fv = _device_features(feat, dev)
    f, n0, n1, n2 = fv.shape
    coords = [torch.as_tensor(v).reshape(-1, 3) for v in annotations.values()]
    targets = np.concatenate([np.full(int(c.shape[0]), i, np.int64) for i, c in enumerate(coords)])
    ext = torch.tensor([[int(s) for s in tuple(volume_shape)[-3:]]], dtype=torch.float32)
    rel = ((torch.cat(coords).float() + 0.5) / ext * 2.0 - 1.0).to(dev).contiguous()
    vn = voxel_norms(fv) if normalize else None
    out = torch.empty((rel.shape[0], f), dtype=torch.float32, device=dev)
    _lib.check(lib.vittf_sample_features(_lib.ptr(fv), 1, f, n0, n1, n2, _lib.ptr(rel), rel.shape[0], _lib.SAMPLE_MODES['bilinear'],
                                         _lib.ptr(vn), _lib.ptr(out), _lib.stream_ptr()), 'vittf_sample_features')
    return out, targets


# ---------------------------------------------------------------------------------------------- files
def file_format(path):
    """What an .npz model file names itself: the string under its `format` key, '' when it has none (an SVM model), None when
    `path` cannot be read as an .npz.  One open: the command line picks the classifier of --model by it."""
    try:
        with np.load(path, allow_pickle=False) as z:
            return str(z['format'][()]) if 'format' in z.files else ''
    except Exception:
        return None


@contextlib.contextmanager
def open_model(path, what, required, dtypes, fmt=None, foreign=None):
    """The open archive of a model file, for the body of a load_model: `what` is the kind in words ('an SVM model'), `required`
    the keys it must hold, `dtypes` {key: dtype} those that are checked, `fmt` the string its `format` key must hold (None: not
    looked at here), `foreign` (keys, words): a file holding all of `keys` is refused as f'{path} {words}'.  ValueError for
    anything else than such a file; a TypeError or IndexError of the body becomes one too."""
    try:
        z = np.load(path, allow_pickle=False)
    except zipfile.BadZipFile as e:
        raise ValueError(f'{path} is not a readable .npz: {e}') from None
    if not isinstance(z, np.lib.npyio.NpzFile):
        raise ValueError(f'{path} is not an .npz of {what}')
    with z:
        if fmt is not None and ('format' not in z.files or str(z['format'][()]) != fmt):
            raise ValueError(f'{path} is not {what} file (format {fmt})')
        if foreign is not None and set(foreign[0]) <= set(z.files):
            raise ValueError(f'{path} {foreign[1]}')
        missing = sorted(set(required) - set(z.files))
        if missing:
            raise ValueError(f'{path} is not {what} file: it lacks {missing}')
        try:
            for k, dt in dtypes.items():
                if z[k].dtype != dt:
                    raise ValueError(f'{k} is {z[k].dtype}, not {np.dtype(dt)}')
            yield z
        except (TypeError, IndexError) as e:
            raise ValueError(f'{path} is not {what} file: {e}') from None


def names_of(z):
    return [str(s) for s in z['class_names'].reshape(-1)]


# ---------------------------------------------------------------------------------------------- the GPU pass
def check_model_f(f, model, holds='the model was fitted on'):
    if f != model.n_features:
        raise ValueError(f'{holds} F = {model.n_features} features, the volume has F = {f}')


def norm_argument(voxel_norm, nvox, dev):
    """The voxel_norm argument of a decide call as the fp32 device vector [nvox] the C entry takes (None stays None)."""
    if voxel_norm is None:
        return None
    vn = torch.as_tensor(voxel_norm).to(dev, torch.float32).contiguous().reshape(-1)
    if vn.numel() != nvox:
        raise ValueError(f'voxel_norm has {vn.numel()} entries for {nvox} voxels')
    return vn


def predict_volume(feat, model, decide, normalize):
    """The body of the four predict functions: labels with the voxel shape of `feat` (F, W', H', D') from
    decide(x, model, voxel_norm) -> (labels [nvox], extra [rows][nvox] or None) on its (F, nvox) matrix, the voxel norms
    (vt.similarity.voxel_norms) passed when `normalize`; (labels, extra as [rows] + voxel shape) when there is an extra."""
    x0 = _on_device(feat)
    x = _as_matrix(x0)
    vn = None
    if normalize:
        from .similarity import voxel_norms
        vn = voxel_norms(x.reshape(x.shape[0], -1, 1, 1))
    labels, extra = decide(x, model, vn)
    shape = tuple(x0.shape[1:])
    labels = labels.reshape(shape)
    return labels if extra is None else (labels, extra.reshape((extra.shape[0],) + shape))
