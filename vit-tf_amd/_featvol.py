"""A feature volume as the kernels of pca.py and kmeans.py take it: a contiguous fp16 device tensor (F, ...) seen as its
(F, nvox) matrix, and the fp64 workspace their reductions add their partials in."""
import numpy as np
import torch


def workspace(nbytes, device):
    """(fp64 device tensor of at least `nbytes` bytes, nbytes): what a vittf_*_workspace_bytes call asked for."""
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device), nbytes


def _np(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t), dtype=dtype)


def _on_device(feat):
    """The volume as a contiguous fp16 device tensor (F, ...) with the features in front and any number of voxel dimensions
    behind them (vt.feature_volume squeezes singleton ones away); one that already is such a tensor is used where it lies."""
    t = feat if isinstance(feat, torch.Tensor) else torch.as_tensor(np.asarray(feat))
    if t.ndim < 2:
        raise ValueError(f'features must be (F, ...) with at least one voxel dimension, got {tuple(t.shape)}')
    if t.is_cuda and t.dtype == torch.float16 and t.is_contiguous():
        return t
    return t.to(device=t.device if t.is_cuda else _device(), dtype=torch.float16).contiguous()


def _as_matrix(feat):
    x = _on_device(feat)
    x = x.reshape(x.shape[0], -1)
    f, nvox = x.shape
    if f % 32 or not 32 <= f <= 1024:
        raise ValueError(f'F must be a multiple of 32 in 32..1024, got {f}')
    if nvox < 1:
        raise ValueError('the volume has no voxels')
    return x


def _device():
    return torch.device('cuda', torch.cuda.current_device())
