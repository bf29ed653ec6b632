"""Volumes and the scipy oracle of the connected-component tests (tests/test_gpu_components.py)."""
import functools

import numpy as np
from scipy import ndimage

from vit_tf_amd._lib import CC_TILE

T0, T1, T2 = CC_TILE
# every size at which the kernels take another path: one voxel, one row over a tile edge, below / at / above one tile in every
# dimension, several tiles with ragged ends in every dimension, and one long-row volume
SHAPES = ((1, 1, 1), (1, 1, T2 + 1), (3, 5, 7), (T0 - 1, T1 - 1, T2 - 1), (T0, T1, T2), (T0 + 1, T1 + 1, T2 + 1),
          (2 * T0 + 1, 3 * T1 + 1, 2 * T2 + 2), (40, 40, 260))
PERCOLATION = {1: 0.31, 2: 0.14, 3: 0.10}        # site-percolation thresholds of the 6-, 18- and 26-neighbour lattices (about)


def oracle_labels(mask, connectivity):
    """scipy.ndimage.label with generate_binary_structure(3, connectivity), renumbered to 1 + the lowest linear index of
    every component (int32, 0 for background)."""
    lab, n = ndimage.label(mask, ndimage.generate_binary_structure(3, connectivity))
    flat = lab.reshape(-1)
    comps, first = np.unique(flat, return_index=True)
    lut = np.zeros(n + 1, np.int64)
    lut[comps] = first + 1
    lut[0] = 0
    return lut[flat].reshape(mask.shape).astype(np.int32)


def oracle_each_value(vol, connectivity):
    """select = -2: every value but 255, linked only within one value -- a scipy loop over the values."""
    out = np.zeros(vol.shape, np.int32)
    for v in np.unique(vol):
        if v != 255:
            out += oracle_labels(vol == v, connectivity)           # the sets are disjoint
    return out


def noise(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def serpentine(shape):
    """A one-voxel-wide path: every second row of every second plane, consecutive rows joined at alternating ends, consecutive
    planes joined by one voxel -- a single 6-connected component of about a quarter of the voxels that crosses every seam."""
    n0, n1, n2 = shape
    vol = np.zeros(shape, np.uint8)
    vol[::2, ::2, :] = 1
    for i1 in range(1, n1, 2):
        if i1 + 1 < n1:
            vol[::2, i1, n2 - 1 if (i1 // 2) % 2 == 0 else 0] = 1
    vol[1::2, 0, 0] = 1
    return vol


def checkerboard(shape):
    i0, i1, i2 = np.indices(shape)
    return ((i0 + i1 + i2) % 2 == 0).astype(np.uint8)


def corner_slabs():
    """Two blocks that touch only across one tile corner: one component under connectivity 3, two under 1 and 2."""
    vol = np.zeros((2 * T0, 2 * T1, 2 * T2), np.uint8)
    vol[:T0, :T1, :T2] = 1
    vol[T0:, T1:, T2:] = 1
    return vol


def value_blocks(shape, seed, block=(2, 3, 5)):
    """Values 0..5 and 255 in random blocks: a cluster-like volume with masked-out voxels."""
    rng = np.random.default_rng(seed)
    coarse = tuple(-(-n // b) for n, b in zip(shape, block))
    vals = rng.choice(np.array([0, 1, 2, 3, 4, 5, 255], np.uint8), size=coarse)
    for axis, b in enumerate(block):
        vals = np.repeat(vals, b, axis=axis)
    return np.ascontiguousarray(vals[:shape[0], :shape[1], :shape[2]])


@functools.lru_cache(maxsize=None)
def patterns(shape, connectivity):
    """{name: uint8 volume} of one shape for one connectivity; built once, shared: nobody writes to them."""
    seed = 1000 * connectivity + sum(shape)
    out = {'zeros': np.zeros(shape, np.uint8), 'ones': np.ones(shape, np.uint8),
           'percolation': noise(shape, PERCOLATION[connectivity], seed), 'half': noise(shape, 0.5, seed + 1),
           'dense': noise(shape, 0.9, seed + 2), 'serpentine': serpentine(shape), 'checkerboard': checkerboard(shape)}
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, connectivity, name):
    want = oracle_labels(patterns(shape, connectivity)[name] != 0, connectivity)
    want.setflags(write=False)
    return want


def largest_island_recipe(sim, threshold, connectivity=1):
    """The reference script's recipe with scipy: threshold, label, keep the map inside the largest island (among equal
    sizes the one with the lowest voxel index), zero elsewhere; an empty set gives zeros."""
    lab = oracle_labels(sim > threshold, connectivity)
    if not lab.any():
        return np.zeros_like(sim)
    ids, counts = np.unique(lab[lab > 0], return_counts=True)           # ids ascend: argmax takes the lowest of a tie
    return np.where(lab == ids[np.argmax(counts)], sim, 0).astype(sim.dtype)
