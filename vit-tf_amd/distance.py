"""Exact Euclidean distance transforms of uint8 volumes and the boundary scores of a segmentation that rest on them.

``edt`` gives every voxel its distance to the nearest SITE, a voxel of a chosen set (libvittf's distance.hip: one pass per axis,
wave scans along the contiguous axis, lower envelopes of parabolas in LDS along the other two); ``signed`` the signed distance
field of a label; ``surface`` the boundary voxels of a mask; ``surface_distances`` and ``surface_scores`` the Hausdorff
distance, its 95th percentile, the average symmetric surface distance and the surface Dice of a prediction against a target.
Unit spacing is exact integer arithmetic; a ``spacing`` takes the fp64 path of anisotropic voxels.  Torch only allocates,
takes square roots and gathers; the percentile and the means are host arithmetic over the surface voxels.  The transforms and
the erosion are HIP kernels and there is no CPU path for them.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .components import _check_volume, _device_volume

MAX_DIM = _lib.EDT_MAX_DIM
NO_SITE = _lib.EDT_NO_SITE
SCORE_KEYS = ('hd', 'hd95', 'assd', 'nsd', 'n_surface_target', 'n_surface_pred')


def _check_edt_volume(volume):
    t = _check_volume(volume)
    if max(t.shape) > MAX_DIM or t.numel() >= 2 ** 31:
        raise ValueError(f'a volume of shape {tuple(t.shape)} cannot be transformed (every dimension <= {MAX_DIM}, fewer than '
                         '2^31 voxels)')
    return t


def _check_value(value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not -1 <= int(value) <= 255:
        raise ValueError(f'value must be 0..255 or -1 (non-zero), got {value!r}')
    return int(value)


def _check_spacing(spacing):
    """None, or the three voxel spacings along (n0, n1, n2) as finite positive floats."""
    if spacing is None:
        return None
    try:
        sp = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f'spacing must be three positive numbers, got {spacing!r}') from None
    if len(sp) != 3 or not all(np.isfinite(s) and s > 0 and np.isfinite(s * s) and s * s > 0 for s in sp):
        raise ValueError(f'spacing must be three finite positive numbers, got {spacing!r}')
    return sp


def edt_sq(volume, value=-1, invert=False, spacing=None, return_sites=False):
    """Squared distances on the device: int32 (vittf_edt_sq, exact) without a spacing, fp32 (vittf_edt_sq_weighted) with one.
    A volume without a site holds NO_SITE (int32) or inf (fp32).  With return_sites also the int32 volume of linear indices
    of a nearest site (-1 without one).  See ``edt`` for the arguments."""
    t = _check_edt_volume(volume)
    value = _check_value(value)
    sp = _check_spacing(spacing)
    lib = _lib.require_device()
    src = _device_volume(t)
    n0, n1, n2 = (int(n) for n in src.shape)
    d2 = torch.empty((n0, n1, n2), dtype=torch.int32 if sp is None else torch.float32, device=src.device)
    sites = torch.empty((n0, n1, n2), dtype=torch.int32, device=src.device) if return_sites else None
    ws_bytes = lib.vittf_edt_workspace_bytes(n0, n1, n2)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=src.device)
    mode = 1 if invert else 0
    with torch.cuda.device(src.device):
        if sp is None:
            _lib.check(lib.vittf_edt_sq(_lib.ptr(src), n0, n1, n2, value, mode, _lib.ptr(d2), _lib.ptr(sites), _lib.ptr(ws), ws_bytes,
                                        _lib.stream_ptr()), 'vittf_edt_sq')
        else:
            w2 = (C.c_double * 3)(*(s * s for s in sp))
            _lib.check(lib.vittf_edt_sq_weighted(_lib.ptr(src), n0, n1, n2, value, mode, w2, _lib.ptr(d2), _lib.ptr(sites),
                                                 _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'vittf_edt_sq_weighted')
    return (d2, sites) if return_sites else d2


def edt(volume, value=-1, invert=False, spacing=None, squared=False, return_indices=False):
    """The distance of every voxel to the nearest site of a uint8 (n0, n1, n2) volume (numpy array, CPU or device tensor); 0 on
    a site.  The sites are {volume == value} for value 0..255 and {volume != 0} for value -1; with invert the complement of
    that set.  scipy.ndimage.distance_transform_edt(mask, sampling=spacing), the distance to the nearest zero of a mask, is
    edt(mask, invert=True, spacing=spacing).

    spacing None: unit voxels, exact int32 arithmetic; squared=True then returns the int32 squared distances.  spacing
    (s0, s1, s2): anisotropic voxels, fp64 arithmetic rounded once to fp32.  Otherwise fp32 distances (device tensor), the
    square root taken in torch.  A volume without a site gives inf everywhere (and, squared without a spacing, NO_SITE).
    return_indices: also an int32 (3, n0, n1, n2) device tensor, the coordinates of a nearest site as scipy returns them
    (-1 without a site); among equally near sites the choice is fixed but need not be scipy's."""
    got = edt_sq(volume, value, invert, spacing, return_sites=return_indices)
    d2, sites = got if return_indices else (got, None)
    if squared and spacing is None:
        out = d2
    else:
        out = d2.to(torch.float32)
        if spacing is None:
            out = torch.where(d2 == NO_SITE, torch.full_like(out, float('inf')), out)
        if not squared:
            out = out.sqrt()
    if not return_indices:
        return out
    n1, n2 = int(sites.shape[1]), int(sites.shape[2])
    plane = torch.div(sites, n1 * n2, rounding_mode='floor')
    rest = sites - plane * (n1 * n2)
    row = torch.div(rest, n2, rounding_mode='floor')
    index = torch.stack((plane, row, rest - row * n2)).to(torch.int32)
    return out, torch.where(sites[None] < 0, torch.full_like(index, -1), index)


def signed(volume, value, spacing=None):
    """The signed distance field of the set {volume == value} (value -1: {volume != 0}): fp32 device tensor, positive outside
    the set and negative inside, edt(to the set) - edt(to its complement).

    Half-voxel convention: both distances are measured between voxel centres, to the nearest voxel of the OTHER set, so a
    voxel next to the boundary holds +1 or -1 (times the spacing), never 0: the zero level lies between the voxel centres,
    half a voxel from either.  A volume that is all set gives -inf, one without the set +inf."""
    value = _check_value(value)
    outside = edt(volume, value, False, spacing)            # 0 inside
    inside = edt(volume, value, True, spacing)              # 0 outside
    return torch.where(outside > 0, outside, -inside)


def _erode(src, class_id, connectivity):
    lib = _lib.require_device()
    n0, n1, n2 = (int(n) for n in src.shape)
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        _lib.check(lib.vittf_erode_mask(_lib.ptr(src), n0, n1, n2, int(class_id), int(connectivity), _lib.ptr(out),
                                        _lib.stream_ptr()), 'vittf_erode_mask')
    return out


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (1, 2, 3):
        raise ValueError(f'connectivity must be 1 (6 neighbours), 2 (18) or 3 (26), got {connectivity!r}')
    return int(connectivity)


def _class_surface(src, class_id, connectivity=1):
    """uint8 0/1 device volume: the voxels of {src == class_id} ({src != 0} for -1) that the erosion removes."""
    member = (src != 0) if class_id < 0 else (src == class_id)
    return (member & (_erode(src, class_id, connectivity) == 0)).to(torch.uint8)


def surface(mask, connectivity=1):
    """The surface of the set {mask != 0}: mask & ~erode(mask), a uint8 0/1 device tensor.  The erosion is vittf_erode_mask,
    scipy.ndimage.binary_erosion with generate_binary_structure(3, connectivity) and scipy's default border_value 0: outside
    the volume counts as background, so a voxel of the mask on the volume's border is always surface."""
    t = _check_edt_volume(mask)
    connectivity = _check_connectivity(connectivity)
    _lib.require_device()
    return _class_surface(_device_volume(t), -1, connectivity)


def _pair(target, pred):
    t, p = _check_edt_volume(target), _check_edt_volume(pred)
    if tuple(t.shape) != tuple(p.shape):
        raise ValueError(f'target {tuple(t.shape)} and prediction {tuple(p.shape)} differ in shape')
    return t, p


def _directed(surf_a, surf_b, spacing):
    """fp32 distances from the voxels of surface a to surface b (inf when b is empty)."""
    return edt(surf_b, -1, False, spacing)[surf_a != 0]


def surface_distances(target, pred, class_id, spacing=None):
    """(target -> pred, pred -> target): two fp32 device vectors, the distance of every surface voxel of {target == class_id}
    to the nearest surface voxel of {pred == class_id} and the reverse (``surface`` with connectivity 1; one transform per
    surface, a masked gather in torch).  A vector is empty when its own surface is, and holds inf when the other one is."""
    t, p = _pair(target, pred)
    class_id = _check_value(class_id)
    _lib.require_device()
    st, sp = _class_surface(_device_volume(t), class_id), _class_surface(_device_volume(p), class_id)
    return _directed(st, sp, spacing), _directed(sp, st, spacing)


def scores_from_distances(t2p, p2t, tolerance=1.0):
    """The scores of one class from its two directed distance sets (anything np.asarray takes), in fp64:
    hd the largest distance of both sets; hd95 numpy.percentile(both sets concatenated, 95), linear interpolation; assd the
    mean of the two directed means; nsd the share of the voxels of both sets within `tolerance`.  Both sets empty: nan, nan,
    nan and nsd 1; one empty (the class is missing from one volume): inf, inf, inf and nsd 0."""
    a, b = np.asarray(t2p, np.float64).reshape(-1), np.asarray(p2t, np.float64).reshape(-1)
    out = {'n_surface_target': a.size, 'n_surface_pred': b.size}
    if a.size == 0 or b.size == 0:
        absent = a.size == 0 and b.size == 0
        out.update({k: float('nan') if absent else float('inf') for k in ('hd', 'hd95', 'assd')}, nsd=1.0 if absent else 0.0)
        return out
    both = np.concatenate((a, b))
    out.update(hd=float(both.max()), hd95=float(np.percentile(both, 95)), assd=float((a.mean() + b.mean()) / 2),
               nsd=float((both <= tolerance).sum() / both.size))
    return out


def surface_scores(target, pred, classes=None, spacing=None, tolerance=1.0):
    """Boundary scores of a predicted uint8 label volume against the target, per class: a dict of numpy arrays of length C,
    entry c for classes[c] (default: 1 .. the largest value of either volume).
      hd                the Hausdorff distance: the largest surface distance in either direction;
      hd95              numpy.percentile(the two directed distance sets concatenated, 95), linear interpolation, in fp64.
                        This is MedPy's hd95; the other definition in circulation, the larger of the two directed 95th
                        percentiles, gives different numbers;
      assd              the average symmetric surface distance as the mean of the two directed means;
      nsd               the surface Dice at `tolerance`: the share of the surface voxels of both volumes that lie within
                        `tolerance` of the other surface;
      n_surface_target, n_surface_pred   the surface voxel counts (int64).
    Distances are in voxels, or in the unit of `spacing` (s0, s1, s2).  A class absent from both volumes gets nan for hd, hd95
    and assd and nsd 1 (nothing to find, nothing found); a class absent from one of them gets inf and nsd 0."""
    t, p = _pair(target, pred)
    spacing = _check_spacing(spacing)
    if not (np.isfinite(tolerance) and tolerance >= 0):
        raise ValueError(f'tolerance must be a finite number >= 0, got {tolerance!r}')
    _lib.require_device()
    td, pd = _device_volume(t), _device_volume(p)
    if classes is None:
        classes = range(1, int(max(td.max().item(), pd.max().item())) + 1)
    classes = [_check_value(c) for c in classes]
    rows = []
    for c in classes:
        st, sp = _class_surface(td, c), _class_surface(pd, c)
        if not bool(st.any()) or not bool(sp.any()):                 # nothing to measure: no transform
            rows.append(scores_from_distances(np.empty(int(st.sum().item())), np.empty(int(sp.sum().item())), tolerance))
            continue
        rows.append(scores_from_distances(_directed(st, sp, spacing).cpu().numpy(), _directed(sp, st, spacing).cpu().numpy(),
                                          tolerance))
    return {k: np.array([r[k] for r in rows], dtype=np.int64 if k.startswith('n_') else np.float64) for k in SCORE_KEYS}
