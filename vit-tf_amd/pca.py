"""PCA reduction of a feature volume: the first principal components of the dense features, as the DINOv2 / DINOv3
papers show them -- three as a colour volume, 16 to 64 as a compact volume the similarity queries take unchanged, or a
basis fitted on one volume and applied to others.

The two passes over the volume run in libvittf (pca.hip): ``feature_gram`` (X X^T and the row sums in fp64) and
``project`` (fp16(V x - offset)).  The F x F eigenproblem between them is host work in fp64 (``basis_from_gram``), like
the weight preparation; that function, the basis files and ``rgb_volume`` need no GPU.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._featvol import _as_matrix, _np, _on_device, workspace

Basis = namedtuple('Basis', ['components', 'mean', 'explained_variance', 'total_variance', 'center', 'offset'])
Basis.__doc__ = """components fp32 [k][F] (orthonormal rows, descending variance), mean fp32 [F] (zeros when not centred),
explained_variance fp64 [k], total_variance fp64 scalar tensor (the trace of the covariance), center bool, offset fp32 [k] =
components @ mean in fp64, rounded once."""

_FIELDS = Basis._fields


def feature_gram(feat):
    """(gram, sums): fp64 [F][F] = X X^T and fp64 [F] = X 1 of a feature volume (F, n0, n1, n2) (or (F, nvox)), X its
    (F, nvox) matrix, on the device through vittf_feature_gram.  `feat`: array or tensor, converted to fp16 on the device as
    similarity._device_features does; a contiguous fp16 device tensor is used where it lies (a view at an odd 2-byte offset too)."""
    lib = _lib.require_device()
    x = _as_matrix(feat)
    f, nvox = x.shape
    gram = torch.empty((f, f), dtype=torch.float64, device=x.device)
    sums = torch.empty((f,), dtype=torch.float64, device=x.device)
    ws, ws_bytes = workspace(lib.vittf_feature_gram_workspace_bytes(f, nvox), x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.vittf_feature_gram(_lib.ptr(x), f, nvox, _lib.ptr(gram), _lib.ptr(sums), _lib.ptr(ws), ws_bytes,
                                          _lib.stream_ptr()), 'vittf_feature_gram')
    return gram, sums


def basis_from_gram(gram, sums, nvox, k, center=True):
    """The top-k eigenpairs of the covariance behind a Gram matrix, in fp64 on the host (no GPU).
    center=True: mean = sums / nvox, cov = (gram - nvox outer(mean, mean)) / (nvox - 1).
    center=False: mean = 0, cov = gram / nvox; then (V x) . (V y) approximates x . y, which keeps raw-dot similarities
    (predict_ntf.py) meaningful on the reduced volume.
    Every component's sign makes its entry of largest magnitude positive (lowest index on ties); eigenvalues are clamped at 0."""
    g = torch.as_tensor(gram).detach().to('cpu', torch.float64)
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64)
    f = g.shape[0]
    nvox, k = int(nvox), int(k)
    if g.shape != (f, f) or s.shape != (f,):
        raise ValueError(f'gram {tuple(g.shape)} / sums {tuple(s.shape)} are not [F][F] / [F]')
    if not 1 <= k <= f:
        raise ValueError(f'components must be in 1..{f}, got {k}')
    if nvox < 1:
        raise ValueError('nvox must be at least 1')
    if center:
        mean = s / nvox
        cov = (g - nvox * torch.outer(mean, mean)) / max(nvox - 1, 1)
    else:
        mean = torch.zeros(f, dtype=torch.float64)
        cov = g / nvox
    evals, evecs = torch.linalg.eigh(cov)
    evals, comps = evals.flip(0)[:k].clamp_min(0.0), evecs.flip(1)[:, :k].T.contiguous()      # [k][F], descending
    big = comps.abs().argmax(dim=1)                      # first index of the largest magnitude
    sign = torch.sign(comps[torch.arange(k), big])
    comps = comps * torch.where(sign == 0, torch.ones_like(sign), sign)[:, None]
    offset = comps @ mean
    return Basis(comps.float(), mean.float(), evals, torch.trace(cov).clamp_min(0.0), bool(center), offset.float())


def fit_basis(feat, k, center=True):
    """basis_from_gram of the volume's Gram matrix (one pass over the volume on the GPU, eigenproblem on the host)."""
    x = _as_matrix(feat)
    gram, sums = feature_gram(x)
    return basis_from_gram(gram, sums, x.shape[1], k, center)


def project(feat, basis):
    """fp16 (k, n0, n1, n2) device tensor (k, then the voxel dimensions of `feat`): fp16(components @ x - offset) per voxel, through vittf_feature_project."""
    lib = _lib.require_device()
    x0 = _on_device(feat)
    x = _as_matrix(x0)
    f, nvox = x.shape
    comp = torch.as_tensor(basis.components).to(x.device, torch.float32).contiguous()
    k = comp.shape[0]
    if comp.shape[1] != f:
        raise ValueError(f'the basis was fitted on F = {comp.shape[1]} features, the volume has F = {f}')
    if not 1 <= k <= _lib.PCA_MAX_K:
        raise ValueError(f'a projection takes 1..{_lib.PCA_MAX_K} components, the basis has {k}')
    off = torch.as_tensor(basis.offset).to(x.device, torch.float32).contiguous() if basis.center else None
    spatial = tuple(x0.shape[1:])
    out = torch.empty((k, *spatial), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.vittf_feature_project(_lib.ptr(x), f, nvox, _lib.ptr(comp), _lib.ptr(off), k, _lib.ptr(out),
                                             _lib.stream_ptr()), 'vittf_feature_project')
    return out


def reduce_features(feat, k, center=True):
    """(reduced fp16 (k, n0, n1, n2) device tensor, Basis): fit_basis + project, the volume uploaded once."""
    x = _on_device(feat)
    basis = fit_basis(x, k, center)
    return project(x, basis), basis


def save_basis(basis, path):
    """An .npz holding exactly the Basis fields as plain arrays (no pickled objects)."""
    arrays = {'components': _np(basis.components, np.float32), 'mean': _np(basis.mean, np.float32),
              'explained_variance': _np(basis.explained_variance, np.float64),
              'total_variance': _np(basis.total_variance, np.float64).reshape(()),
              'center': np.asarray(bool(basis.center)), 'offset': _np(basis.offset, np.float32)}
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def load_basis(path):
    with np.load(path, allow_pickle=False) as z:
        if set(z.files) != set(_FIELDS):
            raise ValueError(f'{path} holds {sorted(z.files)}: not a basis file ({sorted(_FIELDS)})')
        return Basis(torch.from_numpy(z['components'].astype(np.float32)), torch.from_numpy(z['mean'].astype(np.float32)),
                     torch.from_numpy(z['explained_variance'].astype(np.float64)),
                     torch.tensor(float(z['total_variance']), dtype=torch.float64), bool(z['center']),
                     torch.from_numpy(z['offset'].astype(np.float32)))


def rgb_volume(reduced):
    """uint8 (n0, n1, n2, 3): the first three components of a reduced volume (k >= 3, n0, n1, n2), each channel mapped from
    its 1st..99th percentile onto 0..255 and clipped.  Host numpy over 3 nvox values."""
    r = reduced.detach().cpu().numpy() if isinstance(reduced, torch.Tensor) else np.asarray(reduced)
    if r.ndim != 4 or r.shape[0] < 3:
        raise ValueError(f'an RGB volume needs (k >= 3, n0, n1, n2), got {tuple(r.shape)}')
    out = np.empty((*r.shape[1:], 3), dtype=np.uint8)
    for c in range(3):
        ch = r[c].astype(np.float32)
        lo, hi = np.percentile(ch, [1.0, 99.0])
        scale = 255.0 / (hi - lo) if hi > lo else 0.0
        out[..., c] = np.clip(np.rint((ch - lo) * scale), 0, 255).astype(np.uint8)
    return out
