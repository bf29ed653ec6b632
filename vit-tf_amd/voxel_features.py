"""Hand-crafted per-voxel features of a scalar volume at its own resolution: the 11-channel vector of the reference's
classical baseline (predict_svm_rf.py:25-65) as rows of the fp16 (F, nvox) matrix vt.svm.decide and vt.forest.decide take.

With I = V / max(V) the raw channels are: 0 the intensity I; 1 the gradient magnitude sqrt(gx^2 + gy^2 + gz^2) of central
differences g = 0.5 (I[+1] - I[-1]), a neighbour outside the volume counting as 0 (zero padding); 2..7 I at (i0+1), (i1+1),
(i2+1), (i0-1), (i1-1), (i2-1), a neighbour outside the volume being the border voxel itself (replicate padding); 8..10 the
position i / n - 0.5 along each axis.  Every channel is standardised over the whole volume with its mean and unbiased std
(``stats``: fp64 sums in a fixed order, libvittf's vittf_voxel_feature_stats) and rounded once to fp16 (``compose``:
vittf_voxel_features, any range or list of voxels).  ``channels=1`` is the intensity alone, standardised too -- the reference
feeds the raw intensity there; standardising is an increasing affine map, which leaves a forest's decisions and an RBF
machine with gamma='scale' unchanged up to rounding and keeps CT-range values representable in fp16.

The decision kernels take F as a multiple of 32: the rows are embedded in a zeroed 32-row matrix (``pad_to``), so a model
fitted on these features has F = 32 -- like one fitted on a 32-component PCA volume; a model file does not say which.
``classify`` never builds the (32, nvox) matrix of a whole volume (8.6 GB at 512^3): it streams contiguous voxel ranges
through compose and the decision pass in one reusable (32, slab) buffer.  There is no CPU path.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._featvol import _device

CHANNELS = _lib.VOXFEAT_CHANNELS
MIN_DIM, MAX_DIM = 2, 2048

VoxelStats = namedtuple('VoxelStats', 'vmax mean std')
VoxelStats.__doc__ = """vmax: max(V) (a Python float holding an fp32 value); mean, std: fp64 numpy [11] of the raw channels."""


def check_shape(shape):
    """The (n0, n1, n2) of a volume the entries take; ValueError otherwise (a dimension of 1 makes a coordinate channel
    constant, and standardising it divides by zero)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or any(not MIN_DIM <= s <= MAX_DIM for s in shape):
        raise ValueError(f'the volume must be 3-D with every dimension in {MIN_DIM}..{MAX_DIM}, got {shape}')
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f'the volume must have fewer than 2^31 voxels, got {shape}')
    return shape


def _volume(volume):
    """The volume as a contiguous fp32 device tensor (n0, n1, n2) (singleton dimensions squeezed away first)."""
    t = volume if isinstance(volume, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(volume))
    if t.ndim != 3:
        t = t.squeeze()
    check_shape(t.shape)
    if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous():
        return t
    return t.to(device=t.device if t.is_cuda else _device(), dtype=torch.float32).contiguous()


def _check_stats(st, channels):
    if not (np.isfinite(st.vmax) and st.vmax > 0):
        raise ValueError(f'the maximum of the volume must be finite and positive, got {st.vmax}')
    bad = ~(np.isfinite(st.mean[:channels]) & np.isfinite(st.std[:channels]) & (st.std[:channels] > 0))
    if bad.any():
        raise ValueError(f'channel(s) {np.flatnonzero(bad).tolist()} cannot be standardised: mean {st.mean[:channels][bad].tolist()}, '
                         f'std {st.std[:channels][bad].tolist()} (a constant volume?)')


def stats(volume):
    """VoxelStats of the volume: its maximum (vittf_volume_minmax) and the fp64 means and unbiased stds of the 11 raw
    channels (vittf_voxel_feature_stats; the same volume gives the same bytes).  ValueError for a shape outside the limits,
    a maximum that is not finite and positive, or a channel whose std is 0 or not finite."""
    lib = _lib.require_device()
    vol = _volume(volume)
    dev = vol.device
    n0, n1, n2 = vol.shape
    with torch.cuda.device(dev):
        mm = torch.empty(2, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.vittf_minmax_workspace_bytes(), dtype=torch.uint8, device=dev)
        _lib.check(lib.vittf_volume_minmax(_lib.ptr(vol), vol.numel(), _lib.ptr(mm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   'vittf_volume_minmax')
        vmax = float(mm[1].item())
        if not (np.isfinite(vmax) and vmax > 0):
            raise ValueError(f'the maximum of the volume must be finite and positive, got {vmax}')
        nbytes = lib.vittf_voxel_feature_stats_workspace_bytes(n0, n1, n2)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = torch.empty((2, CHANNELS), dtype=torch.float64, device=dev)
        _lib.check(lib.vittf_voxel_feature_stats(_lib.ptr(vol), n0, n1, n2, vmax, _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_ptr()),
                   'vittf_voxel_feature_stats')
        host = out.cpu().numpy()
    st = VoxelStats(vmax, host[0].copy(), host[1].copy())
    _check_stats(st, CHANNELS)
    return st


_volume_stats = stats                                                # (compose and slabs take an argument called stats)


def _device_stats(st, dev):
    return torch.from_numpy(np.stack([np.asarray(st.mean, np.float64), np.asarray(st.std, np.float64)])).to(dev)


def _compose_into(lib, vol, st, st_dev, channels, index, start, n, out):
    """Rows 0..channels-1 of the contiguous fp16 device matrix out [rows][n] <- the n voxels index[:] or start ...."""
    n0, n1, n2 = vol.shape
    _lib.check(lib.vittf_voxel_features(_lib.ptr(vol), n0, n1, n2, st.vmax, _lib.ptr(st_dev), channels, _lib.ptr(index), start, n,
                                        _lib.ptr(out), out.stride(0), _lib.stream_ptr()), 'vittf_voxel_features')


def _check_channels(channels, pad_to=32):
    if channels not in (1, CHANNELS):
        raise ValueError(f'channels must be {CHANNELS} or 1, got {channels}')
    if pad_to < channels:
        raise ValueError(f'pad_to must be at least channels = {channels}, got {pad_to}')


def compose(volume, stats=None, channels=CHANNELS, start=0, count=None, voxels=None, pad_to=32):
    """fp16 device matrix [pad_to][n]: row c < channels holds the standardised channel c of the n voxels `voxels` (any
    integer sequence of linear indices v = (i0 n1 + i1) n2 + i2, duplicates allowed) or, without them, of the `count` voxels
    from `start` (default: to the end of the volume); the rows from `channels` up are zero.  A voxel's bits are the same
    however it is addressed.  stats: what ``stats(volume)`` gave (computed here when None).  ValueError for an index or a
    range outside the volume."""
    lib = _lib.require_device()
    _check_channels(channels, pad_to)
    vol = _volume(volume)
    st = _volume_stats(vol) if stats is None else stats
    _check_stats(st, channels)
    dev = vol.device
    nvox = vol.numel()
    index = None
    if voxels is not None:
        idx = np.ascontiguousarray(voxels.detach().cpu().numpy() if isinstance(voxels, torch.Tensor) else np.asarray(voxels)).reshape(-1)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f'voxels must be integers, got {idx.dtype}')
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= nvox):
            raise ValueError(f'a voxel index is outside 0..{nvox - 1}')
        start, n = 0, int(idx.size)
        index = torch.from_numpy(idx).to(dev)
    else:
        start = int(start)
        n = nvox - start if count is None else int(count)
        if start < 0 or n < 0 or start + n > nvox:
            raise ValueError(f'the range {start} .. {start + n} is outside the {nvox} voxels of the volume')
    out = torch.zeros((pad_to, n), dtype=torch.float16, device=dev)
    if n:
        with torch.cuda.device(dev):
            _compose_into(lib, vol, st, _device_stats(st, dev), channels, index, start, n, out)
    return out


def linear_index(coords, shape):
    """int64 numpy [n]: v = (i0 n1 + i1) n2 + i2 of integer voxel coordinates (n, 3); ValueError for one outside the volume."""
    c = torch.as_tensor(coords).reshape(-1, 3).cpu().numpy()
    if c.size and not np.issubdtype(c.dtype, np.integer):
        if not np.array_equal(c, np.round(c)):
            raise ValueError('annotation coordinates must be whole voxels')
    c = c.astype(np.int64)
    ext = np.asarray(shape, np.int64)
    if c.size and ((c < 0).any() or (c >= ext).any()):
        raise ValueError(f'an annotation lies outside the volume {tuple(int(s) for s in shape)}')
    return (c[:, 0] * ext[1] + c[:, 1]) * ext[2] + c[:, 2]


def sample(volume, annotations, stats, channels=CHANNELS, pad_to=32):
    """(samples fp32 [n][pad_to] device tensor, targets int64 [n] numpy) with vt.svm.sample's contract: the features of the
    annotated voxels themselves (the reference samples trilinearly at the voxel centres of a same-size grid, which is that
    voxel).  annotations: {name: (n, 3) voxel coordinates}; the target of the i-th key is i.  ValueError for a coordinate
    outside the volume."""
    vol = _volume(volume)
    coords = [torch.as_tensor(v).reshape(-1, 3) for v in annotations.values()]
    targets = np.concatenate([np.full(int(c.shape[0]), i, np.int64) for i, c in enumerate(coords)]) if coords else np.zeros(0, np.int64)
    idx = np.concatenate([linear_index(c, vol.shape) for c in coords]) if coords else np.zeros(0, np.int64)
    x = compose(vol, stats, channels, voxels=idx, pad_to=pad_to)
    return x.float().t().contiguous(), targets


def slabs(volume, model, channels=CHANNELS, stats=None, slab_voxels=1 << 24, want_votes=False):
    """Generator over contiguous voxel ranges: (start, n, labels uint8 [n], votes) of each, the device tensors one decision
    call left (votes: vt.forest.decide's uint32 [C][n], vt.svm.decide's fp32 decisions [P][n] or vt.mlp.decide's uint8
    probabilities [C][n]; None unless want_votes).
    The ranges start at multiples of 8 and share one [32][slab] buffer.  ``classify`` is built on it."""
    lib = _lib.require_device()
    _check_channels(channels)
    vol = _volume(volume)
    st = _volume_stats(vol) if stats is None else stats
    _check_stats(st, channels)
    if not hasattr(model, 'decide_slab'):                     # (a KnnModel has none: its geometry needs the voxel norms)
        raise ValueError(f'model must be a ForestModel, an SvmModel or an MlpModel, got {type(model).__name__}')
    if model.n_features != 32:
        raise ValueError(f'the model was fitted on F = {model.n_features} features, the hand-crafted features have F = 32')
    if model.normalize:
        raise ValueError('a model fitted with normalize is not built for the hand-crafted features')
    slab = int(slab_voxels)
    if slab < 8 or slab % 8:
        raise ValueError(f'slab_voxels must be a positive multiple of 8, got {slab_voxels}')
    dev = vol.device
    nvox = vol.numel()
    slab = min(slab, (nvox + 7) // 8 * 8)
    with torch.cuda.device(dev):
        st_dev = _device_stats(st, dev)
        buf = torch.zeros(32 * slab, dtype=torch.float16, device=dev)
        for start in range(0, nvox, slab):
            n = min(slab, nvox - start)
            x = buf[:32 * n].view(32, n)
            if n != slab:
                x.zero_()                                           # the rows lie elsewhere in the buffer now
            _compose_into(lib, vol, st, st_dev, channels, None, start, n, x)
            yield (start, n) + tuple(model.decide_slab(x, want_votes))


def classify(volume, model, channels=CHANNELS, stats=None, slab_voxels=1 << 24, want_votes=False):
    """uint8 device volume of class INDICES 0..C-1 (model.labels[index] is the value a label volume carries): the model's
    decision for every voxel's hand-crafted features, slab by slab (slab_voxels voxels at a time, a multiple of 8: one
    reusable [32][slab] buffer, 1 GiB at the default) -- byte for byte what one decide call on compose()'s whole matrix gives.
    model: a ForestModel, an SvmModel or an MlpModel with F = 32.  With want_votes also the forest's uint32 votes, the
    machine's fp32 decisions or the head's uint8 probabilities, [C or P] + the volume's shape."""
    vol = _volume(volume)
    out = torch.empty(vol.numel(), dtype=torch.uint8, device=vol.device)
    votes = None
    for start, n, labels, v in slabs(vol, model, channels, stats, slab_voxels, want_votes):
        out[start:start + n] = labels
        if want_votes:
            bits = v if v.dtype == torch.uint8 else v.view(torch.int32)     # (uint32 votes: copied as their bits)
            if votes is None:
                votes, dtype = torch.empty((v.shape[0], vol.numel()), dtype=bits.dtype, device=vol.device), v.dtype
            votes[:, start:start + n] = bits
    out = out.reshape(tuple(vol.shape))
    if want_votes:
        votes = votes.view(dtype)
    return (out, votes.reshape((votes.shape[0],) + tuple(vol.shape))) if want_votes else out
