"""Shared by the voxel-feature tests: an fp64 numpy restatement of the 11 hand-crafted channels (include/vittf.h's table,
written from that table), the per-element bound of the fp16 result, and the test volumes.

The bound of a composed element (test_gpu_voxel_features.py asserts got within 1.0 of it):
    |got - want64| <= ulp16(want64) + 16 * 2^-24 * T,    T = (S + |mean_c| + std_c) / std_c + |want64| (1 + mean_c^2 / var_c)
S the largest magnitude among the channel's inputs at the voxel (|I|; the six zero-padded neighbours for the gradient; the
neighbour's value; 0.5 for a coordinate) and ulp16(x) = 2^(max(floor(log2 |x|), -14) - 10): one rounding to fp16, at most
about ten fp32 operations on operands no larger than S, and the statistics' own error.
"""
import functools

import numpy as np

CHANNELS = 11
SHAPES = ((2, 2, 2), (5, 7, 9), (12, 10, 14), (33, 17, 65), (3, 4, 130))
CONTENTS = ('uniform', 'ct')
E2E_SHAPE = (24, 20, 28)


def linear(shape, i0, i1, i2):
    return (i0 * shape[1] + i1) * shape[2] + i2


def uniform_volume(shape, seed=0):
    """fp32 volume of fp16-representable values in [0, 1)."""
    rng = np.random.default_rng([seed, *shape])
    return (rng.integers(0, 2048, shape) / 2048.0).astype(np.float32)


def ct_volume(shape, seed=1):
    """fp32 volume of integers in [-1000, 3000)."""
    rng = np.random.default_rng([seed, *shape])
    return rng.integers(-1000, 3000, shape).astype(np.float32)


@functools.lru_cache(None)
def volume(shape, content):
    v = uniform_volume(shape) if content == 'uniform' else ct_volume(shape)
    v.setflags(write=False)
    return v


def boxes_volume(shape=E2E_SHAPE, seed=2):
    """(fp32 volume, uint8 labels): two constant-plus-noise boxes (values 0.55 and 0.9, labels 1 and 2) in a background of
    0.15, noise uniform in +-0.04."""
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    n0, n1, n2 = shape
    lab[n0 // 6: n0 // 2, n1 // 5: 4 * n1 // 5, n2 // 7: 3 * n2 // 7] = 1
    lab[n0 // 2: 5 * n0 // 6, n1 // 5: 4 * n1 // 5, 4 * n2 // 7: 6 * n2 // 7] = 2
    base = np.asarray([0.15, 0.55, 0.9])[lab]
    return (base + rng.uniform(-0.04, 0.04, shape)).astype(np.float32), lab


def _shift(a, axis, step, mode):
    """a shifted so that out[i] = a[i + step] along `axis`; outside the volume 0 ('zero') or the border voxel ('replicate')."""
    pad = [(1, 1) if k == axis else (0, 0) for k in range(3)]
    p = np.pad(a, pad, mode='constant' if mode == 'zero' else 'edge')
    sl = [slice(None)] * 3
    sl[axis] = slice(1 + step, 1 + step + a.shape[axis])
    return p[tuple(sl)]


def raw_channels(vol):
    """(raw fp64 [11][n0][n1][n2], S fp64 the same shape): the channels before standardising and the largest magnitude among
    each channel's inputs at each voxel."""
    v = np.asarray(vol, np.float64)
    assert v.ndim == 3
    i = v / v.max()
    raw = np.empty((CHANNELS,) + v.shape)
    s = np.empty_like(raw)
    raw[0], s[0] = i, np.abs(i)
    g2 = np.zeros_like(i)
    smax = np.zeros_like(i)
    for axis in range(3):
        up, dn = _shift(i, axis, 1, 'zero'), _shift(i, axis, -1, 'zero')
        g2 += (0.5 * (up - dn)) ** 2
        smax = np.maximum(smax, np.maximum(np.abs(up), np.abs(dn)))
    raw[1], s[1] = np.sqrt(g2), smax
    for axis in range(3):
        raw[2 + axis] = _shift(i, axis, 1, 'replicate')
        raw[5 + axis] = _shift(i, axis, -1, 'replicate')
    s[2:8] = np.abs(raw[2:8])
    grid = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in v.shape], indexing='ij')
    for axis in range(3):
        raw[8 + axis] = grid[axis] / v.shape[axis] - 0.5
    s[8:] = 0.5
    return raw, s


@functools.lru_cache(None)
def _reference(shape, content):
    return reference(volume(shape, content))


def reference(vol):
    """dict of the fp64 restatement: raw [11][...], S, mean [11], std [11] (unbiased), want [11][nvox] standardised."""
    raw, s = raw_channels(vol)
    flat = raw.reshape(CHANNELS, -1)
    mean, std = flat.mean(1), flat.std(1, ddof=1)
    want = (flat - mean[:, None]) / std[:, None]
    out = dict(raw=raw, S=s.reshape(CHANNELS, -1), mean=mean, std=std, want=want)
    for a in out.values():
        a.setflags(write=False)
    return out


def cached_reference(shape, content):
    """reference() of volume(shape, content), computed once per session and read-only."""
    return _reference(tuple(shape), content)


def ulp16(x):
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def fp32_term(ref, want=None):
    """16 * 2^-24 * T per element [11][nvox] (T with `want` in the place of the fp64 restatement when given)."""
    want = ref['want'] if want is None else np.asarray(want, np.float64)
    mean, std = ref['mean'][:, None], ref['std'][:, None]
    t = (ref['S'] + np.abs(mean) + std) / std + np.abs(want) * (1.0 + mean * mean / (std * std))
    return 16.0 * 2.0 ** -24 * t


def bound(ref, want=None, fp32_factor=1.0):
    """ulp16(want) + fp32_factor * fp32_term per element."""
    w = ref['want'] if want is None else np.asarray(want, np.float64)
    return ulp16(w) + fp32_factor * fp32_term(ref, w)


def border_mask(shape):
    """bool [nvox]: the voxels with a neighbour outside the volume."""
    m = np.zeros(shape, bool)
    for axis in range(3):
        sl = [slice(None)] * 3
        for edge in (0, -1):
            sl[axis] = edge
            m[tuple(sl)] = True
    return m.reshape(-1)


def stats_bounds(ref, nvox):
    """(bound of |mean - mean64| [11], bound of |var / var64 - 1| [11]): an fp64 recursive sum of n terms at worst, plus the
    fp32 evaluation of V / m and of the gradient before accumulation."""
    eps = nvox * 2.0 ** -52 + 4 * 2.0 ** -24
    mean, std = ref['mean'], ref['std']
    return eps * (np.abs(mean) + std), eps * (1.0 + mean * mean / (std * std))
