"""Host-only cases, reference and pass criterion for the bilateral solver on the device (csrc/bilateral.hip): torch and
numpy on the CPU, no GPU, no library call.  tests/test_bls_data_cpu.py checks every property the GPU tests of
tests/test_gpu_bilateral.py rest on, so that a failure there is the kernels' and not the generator's.

Why the comparison can be per voxel.  Every case has sim_shape == sim.shape == volume.shape, so the trilinear source index
of output voxel o is exactly o with weight 1 (both resizes are the identity), and an integer-valued volume with minimum 0
and maximum 255, which the uint8 stage maps to itself.  Device and oracle then see the same uint8 reference, hence the same
Sobel confidences (fp32, same operations in the same order, none fused), keys and vertices; what remains between them is the order of fp64 sums
(atomic splats, tree reductions) and fp64 contraction, about 1e-15 relative.  That can flip the final rounding to fp32 and
no more: one spacing, a second one is margin.  No share of the voxels is exempt.

The reference is oracle.bilateral.refine_similarity with the case's grid parameters and one thing replaced: the square
root of the Sobel magnitude.  torch's float32 CPU sqrt is not correctly rounded -- on one build it misses IEEE by one spacing
at 0.6 % to 0.9 % of the voxels of these cases on an Intel Xeon and at 12 % on an AMD EPYC, so the fp32 reference itself
moved by up to 2 spacings from one machine to the other -- while sqrtf on the device is.  `exact_sqrt` is the correctly
rounded one on every machine, and with it the Sobel magnitude is five IEEE single operations on both sides."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import bilateral as obil

SPACINGS = 2                               # allowed |got - ref| inside the box, in fp32 spacings of |ref|
TINY = np.finfo(np.float32).tiny           # ref == 0: the spacing of the smallest normal number


def _case(name, shape, centre, radius, box, gp=None, mask='ball', volume='smooth', zero=False, seed=0, rect=None):
    return SimpleNamespace(name=name, shape=shape, centre=centre, radius=radius, box=box, gp=gp or {}, mask=mask,
                           volume=volume, zero=zero, seed=seed, rect=rect)


# box = what crop_bounds(sim, 0.1, 2) has to give: the ball's voxels are those nearer than `radius` to the centre.
# seed: the first with which the case meets every condition of test_bls_data_cpu.py (c, e: a seed without a zero-confidence
# vertex; d: one whose reference does not move under 1e-12 noise; g, i, j: the three ways the 27-voxel crop can come out).
CASES = [
    # all lo != 0 and crop extent != volume extent: Box.lo*, d1 / d2 addressing of the sobel, key, splat and slice kernels
    _case('a_interior', (37, 50, 29), (20, 22, 12), 9, ((10, 31), (12, 33), (2, 23))),
    # the pad clamped at a low face on axis 0, the box up to the high face on axis 1
    _case('b_faces', (24, 70, 33), (3, 60, 16), 8, ((0, 13), (51, 70), (7, 26))),
    # 59^3 crop, 52 x 30^3 = 1 404 000 device keys: 1372 rank blocks, two per thread of rank_scan_kernel; ~119 000 vertices:
    # many solver workgroups; 262 000 voxels: the grid-stride loop of bbox_kernel
    _case('c_rank_blocks', (64, 62, 66), (31, 30, 32), 28, ((2, 61), (1, 60), (3, 62)), gp={'sigma_spatial': 2}, seed=1),
    # non-integer sigma_spatial, 64 luma bins with the multiples of 4 on bin edges
    _case('d_sigma2p5_luma4', (40, 40, 40), (20, 19, 21), 15, ((4, 37), (3, 36), (5, 38)), gp={'sigma_spatial': 2.5, 'sigma_luma': 4}, seed=1),
    # sigma_luma = 1: 255 luma bins (grey 255 has the float64 luma 254.99999999999997), one short of LUMA_BINS_MAX
    _case('e_luma1', (37, 50, 29), (20, 22, 12), 9, ((10, 31), (12, 33), (2, 23)), gp={'sigma_luma': 1}, seed=2),
    # nz = 1: Sobel's z difference sees only padding; sim non-zero on a rectangle
    _case('f_thin', (1, 40, 33), (0, 20, 16), 15, ((0, 1), (7, 33), (4, 28)), mask='rect', rect=((0, 1), (9, 31), (6, 26))),
    # a single voxel above the threshold in a corner of a white-noise volume: ~22 vertices, one of them with zero confidence
    # -> NaN through the CG -> nan_to_num: the crop comes back all zero
    _case('g_zero_confidence', (20, 24, 28), (19, 0, 27), 1, ((17, 20), (0, 3), (25, 28)), mask='voxel', volume='noise', zero=True, seed=3),
    # sigma_spatial = 1: every voxel its own vertex (31^3 = 29 791, 52 x 31^3 keys: two rank blocks per thread again); the
    # voxel of the largest gradient has zero confidence, so the crop comes back all zero and only the counts are checked
    _case('h_sigma1', (32, 32, 32), (16, 16, 16), 14, ((1, 32), (1, 32), (1, 32)), gp={'sigma_spatial': 1}, zero=True),
    # g with another seed: the one voxel above the threshold is the one of the largest gradient, so splat(target x confidence)
    # is all zero and the solver returns it at once (scipy's |b| = 0 exit, cg_residual_kernel's) -- no NaN involved
    _case('i_zero_rhs', (20, 24, 28), (19, 0, 27), 1, ((17, 20), (0, 3), (25, 28)), mask='voxel', volume='noise', zero=True, seed=1),
    # g with a third seed: no zero-confidence vertex, and the CG converges at its fourth test -- the only live case that
    # stops before cg_maxiter, i.e. that needs the device's convergence latch (a to f run all 25 iterations)
    _case('j_converges', (20, 24, 28), (19, 0, 27), 1, ((17, 20), (0, 3), (25, 28)), mask='voxel', volume='noise', seed=0),
]
LIVE = [c for c in CASES if not c.zero]
WITH_MUTANTS = LIVE[:6]                     # a to f; j has 27 voxels, 24 of them exactly 0 before and after: too little to break
BY_NAME = {c.name: c for c in CASES}


def box_slices(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def box_volume(box):
    return int(np.prod([hi - lo for lo, hi in box]))


@functools.lru_cache(maxsize=None)
def data(name):
    """(volume, sim) of a case, both fp32 of the case's shape.

    volume: 200 x Gaussian blob (0.25 at the ball's surface) + 25 x rand, rounded and clamped to 0..255 -- smooth, so that no
    vertex ends up with zero confidence; white noise for case g.  One voxel outside the box is set to 0 and one to 255.
    sim: blob + 0.1 x rand inside the ball (> 0.1 everywhere there), exactly 0 outside."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + c.seed)
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in c.shape], indexing='ij')
    d2 = (zz - c.centre[0]) ** 2 + (yy - c.centre[1]) ** 2 + (xx - c.centre[2]) ** 2
    blob = torch.exp(-d2 / (2 * (0.6 * c.radius) ** 2)).float()
    if c.volume == 'noise':
        volume = torch.randint(0, 256, c.shape, generator=g).float()
    else:
        volume = (blob * 200 + 25 * torch.rand(c.shape, generator=g)).round().clamp(0, 255)
    if c.mask == 'rect':
        inside = torch.zeros(c.shape, dtype=torch.bool)
        inside[box_slices(c.rect)] = True
    else:
        inside = d2 < c.radius ** 2
    outside_box = torch.ones(c.shape, dtype=torch.bool)
    outside_box[box_slices(c.box)] = False
    free = outside_box.reshape(-1).nonzero()[:, 0]
    volume.view(-1)[free[0]] = 0.0
    volume.view(-1)[free[-1]] = 255.0
    if c.mask == 'voxel':
        sim = torch.zeros(c.shape)
        sim[c.centre] = 0.7
    else:
        sim = torch.where(inside, blob + 0.1 * torch.rand(c.shape, generator=g), torch.zeros(()))
    return volume.contiguous(), sim.float().contiguous()


def exact_sqrt(s):
    """Correctly rounded float32 square root: the float64 root (IEEE) rounded to float32 -- 53 >= 2 x 24 + 2 bits, so the
    second rounding cannot change the result."""
    return torch.from_numpy(np.sqrt(s.numpy().astype(np.float64)).astype(np.float32))


def confidence(ref_u8):
    return obil.sobel_confidence(ref_u8, sqrt=exact_sqrt)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp32 reference of the case, trace of the oracle run): computed once and shared; do not write to it."""
    c = BY_NAME[name]
    volume, sim = data(name)
    trace = {}
    ref = obil.refine_similarity(sim, volume, c.shape, grid_params=c.gp, trace=trace, confidence=confidence)
    return ref, trace


# ---------------------------------------------------------------------------------------------- criterion
def compare(got, ref, sim, box):
    """got against ref: inside the box the error in fp32 spacings of |ref| (of the smallest normal number where ref == 0),
    outside the box the number of voxels that are not bit-equal to the input sim."""
    got, ref, sim = (np.ascontiguousarray(torch.as_tensor(t).numpy(), dtype=np.float32) for t in (got, ref, sim))
    sl = box_slices(box)
    gi, ri = got[sl], ref[sl]
    spacing = np.spacing(np.maximum(np.abs(ri), TINY)).astype(np.float64)
    with np.errstate(invalid='ignore'):
        err = np.abs(gi.astype(np.float64) - ri.astype(np.float64)) / spacing
    err = np.where(np.isfinite(gi), err, np.inf)
    outside = np.ones(got.shape, dtype=bool)
    outside[sl] = False
    worst = int(err.argmax())
    return SimpleNamespace(not_bit_equal=int((gi.view(np.int32) != ri.view(np.int32)).sum()), worst=float(err.reshape(-1)[worst]),
                           worst_at=tuple(int(i) + lo for i, (lo, _) in zip(np.unravel_index(worst, err.shape), box)),
                           voxels=err.size, moved_outside=int((got.view(np.int32) != sim.view(np.int32))[outside].sum()))


def passes(r):
    return r.worst <= SPACINGS and r.moved_outside == 0


def check(got, name, what=''):
    """The GPU tests' assertion for a live case; prints the figures first."""
    c = BY_NAME[name]
    ref, _ = reference(name)
    r = compare(got, ref, data(name)[1], c.box)
    print(f'{name}{what}: {r.not_bit_equal} of {r.voxels} box voxels not bit-equal, largest error {r.worst:.3g} spacings '
          f'(at {r.worst_at}), {r.moved_outside} voxels outside the box moved')
    assert r.moved_outside == 0, f'{name}{what}: {r.moved_outside} voxels outside the box differ from the input'
    assert r.worst <= SPACINGS, (f'{name}{what}: voxel {r.worst_at}: got {float(torch.as_tensor(got)[r.worst_at])!r}, reference '
                                 f'{float(ref[r.worst_at])!r}: {r.worst:.3g} fp32 spacings, {SPACINGS} allowed')
    return r


def check_zero(got, name, what=''):
    """Cases g and h: the crop exactly zero, the outside bit-equal to the input."""
    c = BY_NAME[name]
    got = torch.as_tensor(got)
    sim = data(name)[1]
    crop = got[box_slices(c.box)]
    outside = torch.ones(c.shape, dtype=torch.bool)
    outside[box_slices(c.box)] = False
    moved = int((got.view(torch.int32) != sim.view(torch.int32))[outside].sum())
    print(f'{name}{what}: {int((crop.view(torch.int32) != 0).sum())} of {crop.numel()} box voxels not +0.0, {moved} voxels outside the box moved')
    assert bool((crop.view(torch.int32) == 0).all()) and moved == 0


# ---------------------------------------------------------------------------------------------- mutants of the oracle
def _with(change):
    def make(ref_u8, sigma_spatial, sigma_luma, sigma_chroma):
        grid = obil.Grid(ref_u8, sigma_spatial, sigma_luma, sigma_chroma)
        change(grid)
        return grid
    return make


def _drop_link(grid):
    """One entry of the neighbour table lost: a link (one direction only) of a vertex in the middle of the id range, in the
    first of -x, +x, ... that has links at all."""
    nb = next(nb for nb in grid.neighbours if (nb >= 0).any())
    have = np.flatnonzero(nb >= 0)
    nb[have[have.size // 2]] = -1


def _skip_voxel(grid):
    """One voxel in the middle of the crop reaches no splat (count, confidence, target)."""
    skip, plain = grid.npixels // 2, grid.splat
    grid.splat = lambda x: plain(np.where(np.arange(grid.npixels) == skip, 0.0, x))


RANK_SCAN_KEYS = 1024 * 1024               # keys in front of the second block of every rank_scan_kernel thread pair


def _shift_ids(grid):
    """The voxels behind key 1024 * 1024 get the vertex in front of theirs: a prefix that misses one."""
    behind = grid.key_of_voxel >= RANK_SCAN_KEYS
    assert behind.any() and not behind.all()
    grid.vertex_of_voxel = np.where(behind, grid.vertex_of_voxel - 1, grid.vertex_of_voxel)


def _centre_10(grid):
    nbs = grid.neighbours
    grid.blur = lambda y: 10 * y + sum(np.where(nb >= 0, y[np.maximum(nb, 0)], 0.0) for nb in nbs)


def perturbed_splats(eps, seed):
    """Every splat multiplied by 1 + eps x randn per vertex: a stand-in for another order of the fp64 sums."""
    def change(grid):
        rng, plain = np.random.default_rng(seed), grid.splat
        grid.splat = lambda x: plain(x) * (1.0 + eps * rng.standard_normal(grid.nvertices))
    return _with(change)


GRID_MUTANTS = {'link dropped': _with(_drop_link), 'voxel not splatted': _with(_skip_voxel), 'centre weight 10': _with(_centre_10)}
SHIFTED_IDS = _with(_shift_ids)


def refine_with(name, grid=None, shift=None):
    """The reference's steps on the case's uint8 image with another Grid, or with the crop origin moved by shift =
    (axis, +-1): the crop is read and written back one voxel off.  Without either it is the reference itself
    (test_bls_data_cpu.py)."""
    c = BY_NAME[name]
    ref, trace = reference(name)
    box = [list(b) for b in c.box]
    if shift is not None:
        axis, step = shift
        box[axis] = [box[axis][0] + step, box[axis][1] + step]
        assert 0 <= box[axis][0] and box[axis][1] <= c.shape[axis]
    sl = box_slices(box)
    out = data(name)[1].clone()
    out[sl] = obil.solve(out[sl], trace['ref_u8'][sl], c.gp, grid=grid, confidence=confidence)
    return out


def origin_shift(name):
    """An (axis, step) that keeps the moved crop inside the volume."""
    c = BY_NAME[name]
    for axis in (2, 1, 0):
        if c.box[axis][1] < c.shape[axis]:
            return axis, 1
        if c.box[axis][0] > 0:
            return axis, -1
    raise AssertionError(name)


def mutant_factor(name, out):
    """By how much a mutant's output breaks the criterion inside the case's box: largest error / allowed error."""
    c = BY_NAME[name]
    return compare(out, reference(name)[0], data(name)[1], c.box).worst / SPACINGS


# ---------------------------------------------------------------------------------------------- the trilinear stage alone
U = 2.0 ** -24                             # one fp32 rounding, relative
TRILINEAR_SHAPES = [((7, 5, 9), (20, 18, 22)),        # upscaling by non-integer factors
                    ((31, 25, 40), (17, 12, 23)),     # downscaling
                    ((1, 6, 5), (4, 13, 9)),          # an axis of size 1: i0 == i1 == 0 on it
                    ((6, 11, 5), (13, 11, 8))]        # an identity axis: source index o, weight 1


def _lin_coord(out_size, in_size, fused=True):
    """lin_coord of bilateral.hip (area_pixel_compute_source_index, align_corners=False) in numpy float32, one rounded
    operation per line: (i0, i1, w0, w1) for every output index.  The kernel takes scale * (o + 0.5) - 0.5 as one fmaf, one
    rounding, which is also what a build of the CPU operator with multiply-add contraction computes; fused=False rounds the
    product first, as a build without it does (test_bls_data_cpu.py)."""
    f32 = np.float32
    o = np.arange(out_size, dtype=np.float32)
    scale = f32(in_size) / f32(out_size)
    if fused:
        src = (np.float64(scale) * (o.astype(np.float64) + 0.5) - 0.5).astype(np.float32)     # the product is exact in fp64
    else:
        src = scale * (o + f32(0.5))
        src = src - f32(0.5)
    src = np.where(src < 0, f32(0), src).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.where(i0 < in_size - 1, i0 + 1, i0)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    w0 = (f32(1) - w1).astype(np.float32)
    return i0, i1, w0, w1


def trilinear_ref(src, out_shape, fused=True):
    """(ref, bound), float64 arrays of out_shape: the eight-corner blend in fp64 with fp32 indices and weights, and
    8 x 2^-24 x max |corner| per voxel.

    The bound.  The kernel blends along x, then y, then z; every blend is fl(fl(w0 a) + fl(w1 b)): three rounded operations,
    seven in the three nested blends of one output value counted along the longest chain (2 + 2 + 3), and a corner value
    passes through two of them per level, six in all, each within 2^-24 relative.  The weights are non-negative and
    w0 + w1 <= 1 + 2^-24 per level (w0 = fl(1 - w1)), so every intermediate is at most (1 + 2^-24) ** 9 max |corner| and the
    result differs from the exact blend of the same fp32 weights by less than ((1 + 2^-24) ** 6 - 1) (1 + 2^-24) ** 3 max |corner|
    < 8 x 2^-24 max |corner|."""
    s = np.asarray(src, dtype=np.float64)
    co = [_lin_coord(o, n, fused) for o, n in zip(out_shape, s.shape)]
    ref = np.zeros(out_shape)
    big = np.zeros(out_shape)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                corner = s[np.ix_(co[0][a], co[1][b], co[2][c])]
                wz, wy, wx = co[0][2 + a].astype(np.float64), co[1][2 + b].astype(np.float64), co[2][2 + c].astype(np.float64)
                ref += wz[:, None, None] * wy[None, :, None] * wx[None, None, :] * corner
                big = np.maximum(big, np.abs(corner))
    return ref, 8 * U * big
