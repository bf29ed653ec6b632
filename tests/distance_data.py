"""Volumes and the CPU restatement of the distance-transform tests (tests/test_distance_cpu.py, tests/test_gpu_distance.py):
scipy.ndimage.distance_transform_edt, a brute-force fp64 minimum over all sites, and the surface scores written out from
their definitions (scipy's binary_erosion, a percentile by hand).  Nothing here imports the code under test."""
import functools

import numpy as np
from scipy import ndimage

# where the kernels can go wrong: odd sizes with a row longer than a wave; a cube of many tiles; a long middle axis; degenerate
# axes; the longest line on each axis (the narrowest LDS tile)
SHAPES = ((5, 7, 67), (64, 64, 64), (3, 130, 9), (1, 1, 300), (40, 1, 33), (2, 3, 2048), (2, 2048, 3), (2048, 2, 2))
SMALL = tuple(s for s in SHAPES if s[0] * s[1] * s[2] <= 100000)        # a brute-force minimum is affordable
MASKS = ('corner', 'centre', 'three', 'half', 'all', 'sphere', 'box')
SPACINGS = ((0.7, 0.7, 2.5), (3.0, 0.25, 1.0))
RULES = ((-1, 0), (3, 0), (3, 1), (0, 1), (-1, 1))                       # (value, mode)


def _seed(shape, name):
    return [MASKS.index(name), *shape]


@functools.lru_cache(maxsize=None)
def sites(shape, name):
    """bool volume of the sites of a named pattern (read-only)."""
    m = np.zeros(shape, bool)
    rng = np.random.default_rng(_seed(shape, name))
    idx = np.indices(shape)
    if name == 'corner':
        m[0, 0, 0] = True
    elif name == 'centre':
        m[tuple(n // 2 for n in shape)] = True
    elif name == 'three':
        m.reshape(-1)[rng.choice(m.size, 3, replace=False)] = True
    elif name == 'half':
        m = rng.random(shape) < 0.5
    elif name == 'all':
        m[:] = True
    elif name == 'sphere':
        c = [(n - 1) / 2 for n in shape]
        r = max(1.0, 0.3 * max(shape))
        m = sum((idx[a] - c[a]) ** 2 for a in range(3)) <= r * r
    elif name == 'box':                                                   # touches the low border of every axis
        m[:max(1, shape[0] // 2), :max(1, shape[1] // 3), :max(1, shape[2] // 4)] = True
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


def volume(shape, name, value, mode):
    """A uint8 volume whose sites under the rule (value, mode) are sites(shape, name); the other voxels hold assorted values."""
    s = sites(shape, name)
    rng = np.random.default_rng(_seed(shape, name) + [value + 1, mode])
    if value < 0:
        in_set, other = rng.integers(1, 256, shape), np.zeros(shape, np.int64)
    else:
        other = rng.integers(0, 255, shape)
        other += other >= value                                           # anything but `value`
        in_set = np.full(shape, value)
    return np.where(s != bool(mode), in_set, other).astype(np.uint8)


def is_site(vol, value, mode):
    return ((vol != 0) if value < 0 else (vol == value)) != bool(mode)


def scipy_d2(site_mask, spacing=None):
    """fp64 squared distances of scipy.ndimage.distance_transform_edt; None for a volume without a site."""
    if not site_mask.any():
        return None
    return ndimage.distance_transform_edt(~site_mask, sampling=spacing) ** 2


def brute_d2(site_mask, spacing=None, chunk=1 << 22):
    """fp64 min over all sites of sum_a w_a (x_a - s_a)^2, w = spacing^2 (1 without); inf for a volume without a site.  Every
    product is one rounding; with unit spacing everything is an exact integer."""
    w2 = [1.0, 1.0, 1.0] if spacing is None else [float(s) * float(s) for s in spacing]
    shape = site_mask.shape
    s = np.nonzero(site_mask)
    out = np.full(site_mask.size, np.inf)
    if s[0].size == 0:
        return out.reshape(shape)
    # per axis: table[x, site] = w (x - site_x)^2
    tables = [w2[a] * (np.arange(shape[a], dtype=np.float64)[:, None] - s[a][None, :].astype(np.float64)) ** 2 for a in range(3)]
    vox = np.indices(shape).reshape(3, -1)
    step = max(1, chunk // s[0].size)
    for lo in range(0, site_mask.size, step):
        v = vox[:, lo:lo + step]
        out[lo:lo + step] = (tables[0][v[0]] + tables[1][v[1]] + tables[2][v[2]]).min(axis=1)
    return out.reshape(shape)


@functools.lru_cache(maxsize=None)
def want_int(shape, name):
    """int64 squared index distances from scipy (rint of its fp64 squares), read-only; None without a site."""
    d2 = scipy_d2(sites(shape, name))
    if d2 is None:
        return None
    d2 = np.rint(d2).astype(np.int64)
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def want_brute(shape, name, spacing=None):
    d2 = brute_d2(sites(shape, name), spacing)
    d2.setflags(write=False)
    return d2


def d2_bound(shape, spacing):
    """D2 = sum_a w_a (n_a - 1)^2: no squared distance in the volume is larger."""
    return float(sum(float(s) ** 2 * (n - 1) ** 2 for s, n in zip(spacing, shape)))


def site_d2(index, spacing=None):
    """fp64 squared distance of every voxel to the site whose coordinates index (3, n0, n1, n2) names."""
    w2 = [1.0, 1.0, 1.0] if spacing is None else [float(s) * float(s) for s in spacing]
    own = np.indices(index.shape[1:])
    return sum(w2[a] * (own[a] - index[a].astype(np.int64)).astype(np.float64) ** 2 for a in range(3))


# ---------------------------------------------------------------------------- surface scores, from their definitions
def surface(mask, connectivity=1):
    mask = np.asarray(mask, bool)
    return mask & ~ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, connectivity))


def directed(surf_a, surf_b, spacing=None):
    """fp64 distances from every voxel of surface a to the nearest voxel of surface b (inf when b is empty)."""
    if not surf_b.any():
        return np.full(int(surf_a.sum()), np.inf)
    return ndimage.distance_transform_edt(~surf_b, sampling=spacing)[surf_a]


def percentile(values, q):
    """The q-th percentile with linear interpolation between the order statistics (numpy's default), written out."""
    v = np.sort(np.asarray(values, np.float64))
    rank = (v.size - 1) * q / 100.0
    lo = int(np.floor(rank))
    hi = min(lo + 1, v.size - 1)
    return float(v[lo] + (v[hi] - v[lo]) * (rank - lo))


def scores_from_sets(a, b, tolerance=1.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = {'n_surface_target': a.size, 'n_surface_pred': b.size}
    if a.size == 0 and b.size == 0:
        out.update(hd=np.nan, hd95=np.nan, assd=np.nan, nsd=1.0)
    elif a.size == 0 or b.size == 0:
        out.update(hd=np.inf, hd95=np.inf, assd=np.inf, nsd=0.0)
    else:
        both = np.concatenate((a, b))
        out.update(hd=max(a.max(), b.max()), hd95=percentile(both, 95), assd=0.5 * (a.sum() / a.size + b.sum() / b.size),
                   nsd=(np.count_nonzero(a <= tolerance) + np.count_nonzero(b <= tolerance)) / (a.size + b.size))
    return out


def surface_scores(target, pred, classes, spacing=None, tolerance=1.0):
    rows = []
    for c in classes:
        st, sp = surface(target == c), surface(pred == c)
        rows.append(scores_from_sets(directed(st, sp, spacing), directed(sp, st, spacing), tolerance))
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def ball(shape, centre, radius, value=1, into=None):
    vol = np.zeros(shape, np.uint8) if into is None else into
    idx = np.indices(shape)
    vol[sum((idx[a] - centre[a]) ** 2 for a in range(3)) <= radius * radius] = value
    return vol
