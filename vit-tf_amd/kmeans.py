"""k-means clustering of a feature volume: Lloyd's algorithm (squared Euclidean distance) over the dense features, the
unsupervised companion of the PCA colour volume -- a first partition of the volume before a single voxel is annotated, as
a uint8 label volume the samplers, erosion masks and confusion matrix take as it is.

The two passes over the volume of an iteration run in libvittf (kmeans.hip): ``assign`` (the nearest centroid of every
voxel) and ``cluster_sums`` (the per-cluster feature sums in fp64 and the cluster sizes).  Everything between them is host
work in fp64 over c x F numbers: the k-means++ start (``init_centroids``, on a subsample), the centroid update, the inertia,
the stopping rule and the final renumbering; those functions and the clustering files need no GPU.  Deterministic: the same
seed and the same volume give the same bytes.
"""
import zipfile
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._featvol import _as_matrix, _np, _on_device, workspace

Clustering = namedtuple('Clustering', ['centroids', 'counts', 'inertia', 'inertia_history', 'n_iter', 'converged'])
Clustering.__doc__ = """centroids fp32 [c][F] (numbered by descending voxel count), counts int64 [c] and inertia (fp64 scalar
tensor, sum_v |x_v - m_label(v)|^2) of the partition the centroids are the means of, inertia_history fp64 [n_iter] (one value
per iteration, never increasing), n_iter int, converged bool."""

_FIELDS = Clustering._fields
INIT_SAMPLE = 16384            # voxel columns init_centroids looks at


# ---------------------------------------------------------------------------------------------- the two GPU passes
def assign(feat, centroids):
    """uint8 device tensor with the voxel shape of `feat` (F, n0, n1, n2): the index of the nearest centroid (fp32 [c][F]) of
    every voxel, the lowest index among equal scores, through vittf_kmeans_assign.  The score is m_c . x - 0.5 |m_c|^2; the
    second term is computed in fp64 from the fp32 centroids and rounded once."""
    x0 = _on_device(feat)
    labels, _ = _assign(_as_matrix(x0), centroids, False)
    return labels.reshape(tuple(x0.shape[1:]))


def _assign(x, centroids, want_best):
    lib = _lib.require_device()
    f, nvox = x.shape
    cent = _centroids(centroids, f).to(x.device)
    c = cent.shape[0]
    half = half_sq(cent).to(x.device)
    labels = torch.empty((nvox,), dtype=torch.uint8, device=x.device)
    best = torch.empty((nvox,), dtype=torch.float32, device=x.device) if want_best else None
    with torch.cuda.device(x.device):
        _lib.check(lib.vittf_kmeans_assign(_lib.ptr(x), f, nvox, _lib.ptr(cent), _lib.ptr(half), c, _lib.ptr(labels),
                                           _lib.ptr(best), _lib.stream_ptr()), 'vittf_kmeans_assign')
    return labels, best


def cluster_sums(feat, labels, c):
    """(sums fp64 [c][F], counts int64 [c]) on the device through vittf_kmeans_sums: the feature sums and sizes of the clusters
    0..c-1 of a uint8 label volume over `feat`; a voxel labelled >= c (255: masked out) contributes nowhere."""
    lib = _lib.require_device()
    x = _as_matrix(feat)
    f, nvox = x.shape
    c = _check_c(c)
    lab = torch.as_tensor(labels)
    if lab.dtype != torch.uint8 or lab.numel() != nvox:
        raise ValueError(f'labels must be uint8 with one entry per voxel ({nvox}), got {lab.dtype} {tuple(lab.shape)}')
    lab = lab.to(x.device).contiguous()
    sums = torch.empty((c, f), dtype=torch.float64, device=x.device)
    counts = torch.empty((c,), dtype=torch.int64, device=x.device)
    ws, ws_bytes = workspace(lib.vittf_kmeans_sums_workspace_bytes(f, nvox, c), x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.vittf_kmeans_sums(_lib.ptr(x), f, nvox, _lib.ptr(lab), c, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(ws),
                                         ws_bytes, _lib.stream_ptr()), 'vittf_kmeans_sums')
    return sums, counts


# ---------------------------------------------------------------------------------------------- host arithmetic (fp64)
def half_sq(centroids):
    """fp32 [c]: 0.5 |m_c|^2 in fp64 from the fp32 centroids, rounded once."""
    m = torch.as_tensor(centroids).detach().to(torch.float64)
    return (0.5 * (m * m).sum(1)).float()


def init_centroids(feat, c, seed=0):
    """k-means++ start, fp32 [c][F] on the host: every centroid is a voxel column of `feat` (array or tensor, (F, ...)).
    Runs in fp64 over a seeded subsample of min(nvox, 16384) columns (gathered with torch indexing, so a device volume is not
    copied whole); all randomness comes from numpy.random.default_rng(seed).  A host array needs no GPU."""
    c = _check_c(c)
    t = feat if isinstance(feat, torch.Tensor) else torch.as_tensor(np.asarray(feat))
    if t.ndim < 2:
        raise ValueError(f'features must be (F, ...) with at least one voxel dimension, got {tuple(t.shape)}')
    t = t.reshape(t.shape[0], -1)
    nvox = t.shape[1]
    if c > nvox:
        raise ValueError(f'{c} clusters of {nvox} voxels')
    rng = np.random.default_rng(seed)
    if nvox > INIT_SAMPLE:
        pick = np.sort(rng.choice(nvox, size=INIT_SAMPLE, replace=False))
        t = t[:, torch.from_numpy(pick).to(t.device)]
    x = t.detach().to('cpu', torch.float64).T.contiguous().numpy()           # [m][F]
    m = x.shape[0]
    chosen = [int(rng.integers(m))]
    d2 = ((x - x[chosen[0]]) ** 2).sum(1)
    for _ in range(1, c):
        total = d2.sum()
        if total > 0:
            i = int(rng.choice(m, p=d2 / total))
        else:                                                                 # fewer distinct columns than clusters
            i = int(rng.choice(np.setdiff1d(np.arange(m), chosen)))
        chosen.append(i)
        d2 = np.minimum(d2, ((x - x[i]) ** 2).sum(1))
    return torch.from_numpy(x[chosen]).float()


def update_centroids(centroids, sums, counts):
    """fp32 [c][F]: m_c = sums_c / n_c in fp64, rounded once; an empty cluster keeps its centroid."""
    old = torch.as_tensor(centroids).detach().to('cpu', torch.float32)
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64)
    n = torch.as_tensor(counts).detach().to('cpu', torch.int64)
    mean = (s / n.clamp_min(1).double()[:, None]).float()
    return torch.where((n > 0)[:, None], mean, old)


def inertia_from_sums(sum_sq, sums, counts):
    """sum_v |x_v - mean_label(v)|^2 = sum_v |x_v|^2 - sum_c |sums_c|^2 / n_c in fp64 (the means being sums_c / n_c): no
    further pass over the volume.  `sum_sq`: sum_v |x_v|^2 over the voxels the sums cover."""
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64)
    n = torch.as_tensor(counts).detach().to('cpu', torch.int64)
    per = (s * s).sum(1) / n.clamp_min(1).double()
    return float(sum_sq) - float(per[n > 0].sum())


def renumber(centroids, counts):
    """(centroids, counts, order) numbered by descending voxel count, the lower old index first among equal counts;
    order[new] = old."""
    n = torch.as_tensor(counts).detach().to('cpu', torch.int64).numpy()
    order = np.lexsort((np.arange(n.size), -n))
    idx = torch.from_numpy(order)
    return torch.as_tensor(centroids)[idx].contiguous(), torch.from_numpy(n[order]), idx


def fit(feat, c, seed=0, max_iter=50, tol=1e-4, init=None):
    """(labels, Clustering) of Lloyd's k-means with c clusters over a feature volume (F, n0, n1, n2).
    Start: `init` (fp32 [c][F]) or init_centroids(feat, c, seed).  Every iteration: assign, cluster_sums, m_c = sums_c / n_c
    (update_centroids), the inertia of that partition (inertia_from_sums).  It stops when the summed squared centroid shift
    is <= tol x the mean per-feature variance of the volume (scikit-learn's rule; converged), when no centroid changed at all
    (converged), or after max_iter iterations.  The clusters are then renumbered by descending voxel count and `labels`
    (uint8 device tensor, the voxel shape of `feat`) is one last assign against the renumbered centroids."""
    c = _check_c(c)
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    x0 = _on_device(feat)
    x = _as_matrix(x0)
    f, nvox = x.shape
    if c > nvox:
        raise ValueError(f'{c} clusters of {nvox} voxels')
    cent = _centroids(init, f) if init is not None else init_centroids(x, c, seed)
    if cent.shape[0] != c:
        raise ValueError(f'init holds {cent.shape[0]} centroids, {c} clusters were asked for')
    sum_sq = _sum_sq(x)
    history, threshold, converged = [], None, False
    for _ in range(int(max_iter)):
        labels, _ = _assign(x, cent, False)
        sums, counts = cluster_sums(x, labels, c)
        sums, counts = sums.cpu(), counts.cpu()
        if threshold is None:              # every voxel carries a label below c: the sums add up to the volume's
            mean = sums.sum(0) / nvox
            threshold = tol * max(sum_sq / nvox - float((mean * mean).sum()), 0.0) / f
        new = update_centroids(cent, sums, counts)
        history.append(inertia_from_sums(sum_sq, sums, counts))
        shift = float(((new.double() - cent.double()) ** 2).sum())
        unchanged = torch.equal(new, cent)
        cent = new
        if unchanged or shift <= threshold:
            converged = True
            break
    cent, counts, _ = renumber(cent, counts)
    labels, _ = _assign(x, cent, False)
    result = Clustering(cent, counts, torch.tensor(history[-1], dtype=torch.float64),
                        torch.tensor(history, dtype=torch.float64), len(history), converged)
    return labels.reshape(tuple(x0.shape[1:])), result


# ---------------------------------------------------------------------------------------------- files
def save_clustering(clustering, path):
    """An .npz holding exactly the Clustering fields as plain arrays (no pickled objects)."""
    arrays = {'centroids': _np(clustering.centroids, np.float32), 'counts': _np(clustering.counts, np.int64),
              'inertia': _np(clustering.inertia, np.float64).reshape(()),
              'inertia_history': _np(clustering.inertia_history, np.float64).reshape(-1),
              'n_iter': np.asarray(int(clustering.n_iter), dtype=np.int64), 'converged': np.asarray(bool(clustering.converged))}
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def load_clustering(path):
    """The Clustering of a file save_clustering wrote; ValueError for anything else (another .npz, a .npy, a damaged file)."""
    try:
        z = np.load(path, allow_pickle=False)
    except zipfile.BadZipFile as e:
        raise ValueError(f'{path} is not a readable .npz: {e}') from None
    if not isinstance(z, np.lib.npyio.NpzFile):
        raise ValueError(f'{path} is not an .npz of a clustering')
    with z:
        if set(z.files) != set(_FIELDS):
            raise ValueError(f'{path} holds {sorted(z.files)}: not a clustering file ({sorted(_FIELDS)})')
        return Clustering(torch.from_numpy(z['centroids'].astype(np.float32)), torch.from_numpy(z['counts'].astype(np.int64)),
                          torch.tensor(float(z['inertia']), dtype=torch.float64),
                          torch.from_numpy(z['inertia_history'].astype(np.float64)), int(z['n_iter']), bool(z['converged']))


# ---------------------------------------------------------------------------------------------- helpers
def _check_c(c):
    c = int(c)
    if not 2 <= c <= _lib.KMEANS_MAX_C:
        raise ValueError(f'clusters must be in 2..{_lib.KMEANS_MAX_C}, got {c}')
    return c


def _centroids(centroids, f):
    cent = torch.as_tensor(centroids).detach().to(torch.float32).contiguous()
    if cent.ndim != 2 or cent.shape[1] != f:
        raise ValueError(f'centroids {tuple(cent.shape)} are not [c][F = {f}]')
    _check_c(cent.shape[0])
    return cent


def _sum_sq(x, chunk=1 << 15):
    """sum_v |x_v|^2 of the (F, nvox) device matrix in fp64 (in voxel chunks: no fp64 copy of the volume)."""
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for v in range(0, x.shape[1], chunk):
        total += x[:, v:v + chunk].double().square().sum()
    return float(total)
