"""Connected components of uint8 label, mask and similarity volumes: from "voxels of a class" to "objects".

``label`` numbers the separate bodies of a set (libvittf's components.hip: union-find in LDS per tile, union-find over the
tile seams, flatten); ``sizes`` / ``table`` count them, ``relabel`` renumbers them by size into a uint8 volume,
``largest_island`` keeps a similarity map inside the largest island of its thresholded set (the reference's
tests/test_connected_components.py) and ``remove_small`` drops every body below a size.  A label is 1 + the smallest linear
index of its component, so the same volume gives the same bytes.  Torch only allocates, sorts and indexes; the passes over the
volume are HIP kernels and there is no CPU path for them.
"""
import numpy as np
import torch

from . import _lib

TILE = _lib.CC_TILE           # voxels along (n0, n1, n2) of the tile of the LDS pass
EACH_VALUE = -2               # select: every value but 255 is foreground, neighbours link only within one value
MAX_VOXELS = 2 ** 31 - 2


def _check_volume(volume):
    t = volume if isinstance(volume, torch.Tensor) else torch.as_tensor(np.asarray(volume))
    if t.dtype != torch.uint8:
        raise ValueError(f'the volume must be uint8, got {t.dtype}')
    if t.ndim != 3:
        raise ValueError(f'the volume must have 3 dimensions, got {tuple(t.shape)}')
    if min(t.shape) < 1 or t.numel() > MAX_VOXELS:
        raise ValueError(f'a volume of shape {tuple(t.shape)} cannot be labelled (1 .. 2^31 - 2 voxels)')
    return t


def _check_rule(select, connectivity):
    if isinstance(select, bool) or not isinstance(select, (int, np.integer)) or not -2 <= int(select) <= 255:
        raise ValueError(f'select must be a value 0..255, -1 (non-zero) or -2 (each value), got {select!r}')
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (1, 2, 3):
        raise ValueError(f'connectivity must be 1 (6 neighbours), 2 (18) or 3 (26), got {connectivity!r}')
    return int(select), int(connectivity)


def _device_volume(t):
    return t.to(device=t.device if t.is_cuda else torch.device('cuda', torch.cuda.current_device())).contiguous()


def label(volume, select=-1, connectivity=1):
    """int32 device tensor of the volume's shape: 0 for background, else 1 + the smallest linear index of the voxel's
    component (vittf_label_components).  volume: uint8 (n0, n1, n2) numpy array, CPU or device tensor.  select 0..255: the set
    {volume == select}; -1: {volume != 0}; -2: every value but 255, linked only within one value.  connectivity 1, 2, 3 = 6,
    18, 26 neighbours (scipy's generate_binary_structure(3, connectivity))."""
    t = _check_volume(volume)
    select, connectivity = _check_rule(select, connectivity)
    lib = _lib.require_device()
    src = _device_volume(t)
    n0, n1, n2 = (int(n) for n in src.shape)
    labels = torch.empty((n0, n1, n2), dtype=torch.int32, device=src.device)
    ws_bytes = lib.vittf_components_workspace_bytes(n0, n1, n2)
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.vittf_label_components(_lib.ptr(src), n0, n1, n2, select, connectivity, _lib.ptr(labels), _lib.ptr(ws),
                                              ws_bytes, _lib.stream_ptr()), 'vittf_label_components')
    return labels


def _check_labels(labels):
    t = torch.as_tensor(labels)
    if t.dtype != torch.int32 or not 1 <= t.numel() <= MAX_VOXELS:
        raise ValueError(f'labels must be a non-empty int32 volume, got {t.dtype} {tuple(t.shape)}')
    return t


def sizes(labels):
    """int32 device tensor [nvox]: sizes[l - 1] = voxels carrying label l (vittf_component_sizes)."""
    t = _check_labels(labels)
    lib = _lib.require_device()
    lab = _device_volume(t)
    out = torch.empty((lab.numel(),), dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.check(lib.vittf_component_sizes(_lib.ptr(lab), lab.numel(), _lib.ptr(out), _lib.stream_ptr()),
                   'vittf_component_sizes')
    return out


def table_from_sizes(sizes):
    """(ids, counts) of a sizes vector (CPU or device tensor): the labels that occur, by descending voxel count, the lower
    label first among equal counts; ids and counts int64."""
    s = torch.as_tensor(sizes).reshape(-1)
    ids = s.nonzero().reshape(-1)                       # ascending
    counts, order = torch.sort(s[ids].to(torch.int64), descending=True, stable=True)
    return ids[order] + 1, counts


def table(labels):
    """(ids, counts) of a label volume of ``label``: see table_from_sizes; device tensors."""
    return table_from_sizes(sizes(labels))


def relabel(labels, ids, max_islands=255):
    """uint8 volume (on the device of `labels`): island ids[r] becomes r + 1 for r < max_islands (at most 255); background
    and every other island become 0."""
    if not 1 <= int(max_islands) <= 255:
        raise ValueError(f'max_islands must be in 1..255, got {max_islands}')
    lab = _check_labels(labels)
    keep = torch.as_tensor(ids).reshape(-1)[:int(max_islands)].to(lab.device, torch.int64)
    lut = torch.zeros((lab.numel() + 1,), dtype=torch.uint8, device=lab.device)
    lut[keep] = torch.arange(1, keep.numel() + 1, device=lab.device).to(torch.uint8)
    return lut[lab]


def _filter(src, labels, comp_sizes, min_size, keep_label, fill):
    lib = _lib.require_device()
    dst = torch.empty_like(src)
    with torch.cuda.device(src.device):
        _lib.check(lib.vittf_filter_components(_lib.ptr(src), _lib.ptr(labels), _lib.ptr(comp_sizes), src.numel(), int(min_size),
                                               int(keep_label), int(fill), _lib.ptr(dst), _lib.stream_ptr()),
                   'vittf_filter_components')
    return dst


def largest_island(map_u8, threshold, connectivity=1):
    """The uint8 map kept inside the largest island of {map > threshold} and 0 elsewhere (device tensor); among islands of
    equal size the one with the lowest voxel index.  An empty set gives an all-zero map."""
    t = _check_volume(map_u8)
    _, connectivity = _check_rule(-1, connectivity)
    _lib.require_device()
    src = _device_volume(t)
    mask = (src > int(threshold)).to(torch.uint8)
    labels = label(mask, -1, connectivity)
    ids, _ = table(labels)
    if ids.numel() == 0:
        return torch.zeros_like(src)
    return _filter(src, labels, None, 0, int(ids[0]), 0)


def remove_small(volume, min_size, select=-1, connectivity=1, fill=0):
    """The volume with every voxel outside the set, and every component of the set with fewer than min_size voxels, replaced
    by `fill` (uint8 device tensor)."""
    t = _check_volume(volume)
    select, connectivity = _check_rule(select, connectivity)
    if not 0 <= int(fill) <= 255:
        raise ValueError(f'fill must be in 0..255, got {fill}')
    _lib.require_device()
    src = _device_volume(t)
    labels = label(src, select, connectivity)
    return _filter(src, labels, sizes(labels), int(min_size), 0, fill)
