"""Host-only data, references and error bounds for the kernels of the interactive refinement loop -- vittf_topk_voxels,
vittf_sample_features, vittf_similarity_maps_f32 in modes 1 and 2, vittf_mean_pairwise_distance (csrc/prototypes.hip,
csrc/similarity.hip) -- and the Python functions on top: numpy and torch on the CPU, no GPU, no library call.
tests/test_refine_data_cpu.py checks every property the GPU tests of tests/test_gpu_refine.py rest on; the class-map
reference and its bound are tests/sim_data.py's (class_maps_ref with mode and expo)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import sim_data as sd

U = sd.U
F32 = np.float32


# ============================================================================================== 1. top-K: exact
TOPK_NVOX = (1, 63, 1024, 1025, 3000, 5000)
TOPK_K = (1, 2, 9, 35, 1024, 1025, None)          # None: k = nvox
TOPK_KINDS = ('normal', 'ties', 'digit0', 'digit1', 'digit2', 'digit3', 'thresholded', 'signed_zeros', 'kth_negative_zero')
CHUNK, WAVE = 1024, 64                            # voxels of one compaction round of the kernel, lanes of one ballot
DIGIT_MASKS = (0x000000ff, 0x0000ff00, 0x00ff0000, 0x7f000000)


def topk_ks(nvox):
    return sorted({nvox if k is None else k for k in TOPK_K if k is None or k <= nvox})


def topk_ref(maps, k):
    """The expression the kernel replaces (infer.py:95-96), map by map: int64 [maps][k]."""
    out = []
    for s in torch.as_tensor(maps):
        kth = torch.topk(s.flatten(), k, largest=True, sorted=True).values[-1]
        out.append((s >= kth).nonzero()[:k, 0])
    return torch.stack(out)


def order_keys(values):
    """numpy restatement of the kernel's order_key: uint32 keys that order like the floats, -0.0 with the key of +0.0."""
    b = np.ascontiguousarray(values, dtype=F32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(F32).copy())


def topk_maps(nvox, k, seed=0):
    """One fp32 map [nvox] per kind of TOPK_KINDS, for this k: {kind: tensor}.
      normal             randn, mixed signs, +inf and -inf present (nvox >= 3)
      ties               four levels; the k-th value is tied, with tied voxels on both sides of index 64 and of index 1024
      digit0..3          keys that differ only in bits 0-7, 8-15, 16-23, 24-30: 1 + j 2^-23, 1 + j 2^-15, the bits
                         0x3f000000 + (j << 16) (0.5 to just below 2: the exponent's low bit and the mantissa's top seven) and
                         j << 24 (0 and powers of four times 1 or 2^-64: exponent bits only), j < 256 (j < 128)
      thresholded        +0.0 but for m = k // 2 positive voxels in the last third of the map: the k-th value is 0 and the
                         expression keeps the FIRST k voxels (every voxel is >= 0), whether they are positive or not
      signed_zeros       the same with -0.0 on a third of the zero voxels, among them index 0, one behind the first
                         positive voxel and the last voxel
      kth_negative_zero  m positive voxels, fewer than k - m voxels of +0.0, the others -0.0 or negative: the k-th largest
                         value is a zero that only the -0.0 voxels can supply"""
    g = torch.Generator().manual_seed(1000 * nvox + 7 * k + seed)
    out = {}
    s = torch.randn(nvox, generator=g)
    if nvox >= 3:
        p = torch.randperm(nvox, generator=g)
        s[p[0]], s[p[1]] = float('inf'), -float('inf')
    out['normal'] = s
    t = torch.randint(0, 4, (nvox,), generator=g).float() * 0.5 - 0.75
    kth = torch.topk(t, k).values[-1]
    for i in (WAVE - 1, WAVE, CHUNK - 1, CHUNK):      # the tie straddles the wave and the chunk boundary
        if i < nvox:
            t[i] = kth
    out['ties'] = t
    j = torch.randint(0, 256, (nvox,), generator=g).numpy().astype(np.uint32)
    out['digit0'] = _from_bits(0x3f800000 + j)
    out['digit1'] = _from_bits(0x3f800000 + (j << 8))
    out['digit2'] = _from_bits(0x3f000000 + (j << 16))
    out['digit3'] = _from_bits((j & 0x7f) << 24)
    m = k // 2
    s = torch.zeros(nvox)
    tail = torch.arange(nvox - max(nvox // 3, m), nvox)
    pos = tail[torch.randperm(len(tail), generator=g)[:m]]
    s[pos] = torch.rand(m, generator=g) + 0.01
    out['thresholded'] = s
    z = s.clone()
    zero = (s == 0).nonzero()[:, 0]
    neg = zero[torch.rand(len(zero), generator=g) < 1 / 3]
    z[neg] = -0.0
    for i in (0, nvox - 1, int(pos.min()) + 1 if m else 1):
        if 0 <= i < nvox and s[i] == 0:
            z[i] = -0.0
    out['signed_zeros'] = z
    order = torch.randperm(nvox, generator=g)
    n_pz = (k - m) // 2                               # fewer +0.0 than the k - m that are still wanted
    n_nz = (k - m - n_pz) + (nvox - k) // 2           # enough -0.0 to reach k, and some more
    kz = -torch.rand(nvox, generator=g) - 0.01
    kz[order[:m]] = torch.rand(m, generator=g) + 0.01
    kz[order[m:m + n_pz]] = 0.0
    kz[order[m + n_pz:m + n_pz + n_nz]] = -0.0
    out['kth_negative_zero'] = kz
    assert list(out) == list(TOPK_KINDS)
    return out


def topk_stack(nvox, k):
    """[kinds][nvox], in TOPK_KINDS order (a call takes the first 8 maps, a second call the ninth)."""
    return torch.stack(list(topk_maps(nvox, k).values())).contiguous()


def distance_map(n=600, seed=3):
    """take_most_dissimilar's use: one map of n mean cosine distances, 1 - mean_j cos: (0, 2) values that crowd near one value."""
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(n, 24, generator=g) + 0.5, dim=1)
    return (1.0 - (x @ x.T).mean(0)).float().reshape(1, n).contiguous()


# ============================================================================================== 2. sampling
SAMPLE_GRIDS = ((1, 1, 1), (2, 3, 5), (6, 5, 7), (9, 1, 33))
SAMPLE_F = (1, 32, 33, 384)


def sample_pos32(r, n):
    """sample_pos of csrc/similarity.hip, every operation rounded to fp32: ((r + 1) * n - 1) / 2."""
    r = np.asarray(r, dtype=F32)
    return ((r + F32(1.0)) * F32(n) - F32(1.0)) / F32(2.0)


def rel_for_pos(pos, n):
    """An fp32 relative coordinate whose sample_pos32 is EXACTLY pos (a multiple of 0.5), or None: the rel -> position map is
    ill-conditioned where it matters (voxel centres, cell faces), so the points are chosen by their fp32 position."""
    y = (2.0 * pos + 1.0) / n                          # r + 1
    r0 = F32(y - 1.0)
    cands = [r0]
    lo = hi = r0
    for _ in range(8):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        cands += [lo, hi]
    for r in cands:
        if float(sample_pos32(r, n)) == pos:
            return F32(r)
    return None


def sample_points(grid, seed=0, n_random=24):
    """fp32 rel [A][3] in volume dim order and the index ranges of its kinds (.kinds: {name: slice}):
      centres   every voxel centre: integer positions, weights exactly 0 / 1
      faces     every voxel centre moved by +0.5 along one axis, and by -0.5 for the first voxel of the axis: the nearest tie
                (Not every such position is an fp32 coordinate's: (r + 1) * n must round to 2 pos + 1 exactly, and below
                pos = n / 4 the fp32 spacing of r near -1 times n can step over it -- the first voxels of an axis of 3 or
                more.  Those points are sampled at the nearest coordinate and listed as near_centres / near_faces: held to
                the emulation and the bound like every point, but not to the voxel's own value.)
      corners   all combinations of exactly -1 and +1 (positions -0.5 and n - 0.5)
      outside   random points up to 1.5 voxels outside on either side of every axis (positions in [-1.5, n + 0.5]), and for
                every axis and side one point more than one voxel outside on that axis: all eight corners outside
      interior  random points with all eight corners inside (grids with at least two voxels per axis), else anywhere inside"""
    g = np.random.default_rng(seed + 31 * int(np.prod(grid)))
    exact = [{p: rel_for_pos(p, n) for p in np.arange(-0.5, n, 0.5)} for n in grid]
    rel1 = [{p: F32((2.0 * p + 1.0) / n - 1.0) if r is None else r for p, r in d.items()} for d, n in zip(exact, grid)]
    vox = np.stack(np.meshgrid(*[np.arange(n) for n in grid], indexing='ij'), -1).reshape(-1, 3)
    pts, kinds = [], {}

    def add(name, positions):
        """positions whose three coordinates are exact go to `name`, the others (nearest fp32 coordinate) to near_`name`"""
        hit = [all(exact[ax][float(p[ax])] is not None for ax in range(3)) for p in positions]
        for kind, keep in ((name, True), ('near_' + name, False)):
            sel = [p for p, h in zip(positions, hit) if h == keep]
            start = sum(len(p) for p in pts)
            pts.append(np.array([[rel1[ax][float(p[ax])] for ax in range(3)] for p in sel], dtype=F32).reshape(-1, 3))
            kinds[kind] = slice(start, start + len(sel))

    add('centres', vox.astype(float))
    faces = []
    for ax in range(3):
        e = np.zeros(3); e[ax] = 0.5
        faces += [v + e for v in vox] + [v - e for v in vox if v[ax] == 0]
    add('faces', faces)
    start = sum(len(p) for p in pts)
    pts.append(np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=F32))
    kinds['corners'] = slice(start, start + 8)
    start += 8
    span = np.array([2.0 / n for n in grid])           # rel per voxel
    out = g.uniform(-1 - 1.0 * span, 1 + 1.0 * span, size=(n_random, 3))
    side = g.integers(0, 3, size=n_random)             # at least one axis beyond the volume's face
    for i, ax in enumerate(side):
        out[i, ax] = (1 + g.uniform(0, 1.0) * span[ax]) * (1 if i % 2 else -1)
    gone = []
    for ax in range(3):
        for sgn in (-1, 1):
            p = g.uniform(-1, 1, size=3); p[ax] = sgn * (1 + 0.8 * span[ax]); gone.append(p)   # position -1.3 or n + 0.3
    pts.append(np.concatenate([out, np.array(gone)]).astype(F32))
    kinds['outside'] = slice(start, start + n_random + 6)
    kinds['all_outside'] = slice(start + n_random, start + n_random + 6)
    start += n_random + 6
    inner = np.array([g.uniform(-1 + s, 1 - s, size=n_random) if n > 1 else g.uniform(-0.001, 0.001, size=n_random) for n, s in zip(grid, span)]).T
    pts.append(inner.astype(F32))
    kinds['interior'] = slice(start, start + n_random)
    return SimpleNamespace(rel=np.ascontiguousarray(np.concatenate(pts), dtype=F32), kinds=kinds)


def sample_volume(grid, f, half, seed=0):
    """(feat [F][n0][n1][n2] fp32 or fp16 tensor, vnorm fp32 [nvox]): randn * 2 values -- fp32 volumes keep all 24 bits --,
    one all-zero voxel (the last), whose norm is the 1e-12 clamp of F.normalize."""
    g = torch.Generator().manual_seed(seed + 17 * f + int(np.prod(grid)))
    feat = torch.randn(f, *grid, generator=g) * 2
    feat[:, -1, -1, -1] = 0.0
    feat = feat.half() if half else feat
    vnorm = feat.double().reshape(f, -1).norm(dim=0).clamp_min(1e-12).float()
    return feat.contiguous(), vnorm.contiguous()


def _corner_terms(feat, rel, vnorm, dtype):
    """Per point and feature, the eight (value, weight) pairs in the kernel's order tnw .. bse, in `dtype` arithmetic from
    the fp32 positions: values [8][A][F] (0 outside the volume), weights [8][A], inside [8][A]."""
    fv = np.asarray(feat.float().numpy() if isinstance(feat, torch.Tensor) else feat)
    f, n0, n1, n2 = fv.shape
    flat = fv.reshape(f, -1)
    pos = [sample_pos32(rel[:, ax], n) for ax, n in enumerate((n0, n1, n2))]             # iz, iy, ix: fp32
    fl = [np.floor(p) for p in pos]
    one = dtype(1.0)
    w1 = [p.astype(dtype) - q.astype(dtype) for p, q in zip(pos, fl)]
    w0 = [(q.astype(dtype) + one) - p.astype(dtype) for p, q in zip(pos, fl)]
    vals, wgts, ins = [], [], []
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                z, y, x = fl[0].astype(np.int64) + cz, fl[1].astype(np.int64) + cy, fl[2].astype(np.int64) + cx
                w = ((w1[2] if cx else w0[2]) * (w1[1] if cy else w0[1])) * (w1[0] if cz else w0[0])     # (x * y) * z
                inside = (x >= 0) & (x < n2) & (y >= 0) & (y < n1) & (z >= 0) & (z < n0)
                vox = np.where(inside, (z * n1 + y) * n2 + x, 0)
                v = flat[:, vox].T.astype(dtype)                                           # [A][F]
                if vnorm is not None:
                    v = v / np.asarray(vnorm)[vox].astype(dtype)[:, None]
                vals.append(np.where(inside[:, None], v, dtype(0.0)))
                wgts.append(w.astype(dtype))
                ins.append(inside)
    return np.stack(vals), np.stack(wgts), np.stack(ins)


def sample_emulate(feat, rel, mode, vnorm=None):
    """float32 restatement of the kernel's stated order: sample_pos with each operation rounded; nearest: the voxel at
    rint (half to even) of the position; trilinear: corners tnw .. bse, weight (x * y) * z, res = fl(res + fl(val * w))
    over the corners inside the volume.  fp32 [A][F]."""
    fv = feat.float().numpy()
    f, n0, n1, n2 = fv.shape
    if mode == 'nearest':
        z, y, x = [np.rint(sample_pos32(rel[:, ax], n)).astype(np.int64) for ax, n in enumerate((n0, n1, n2))]
        inside = (x >= 0) & (x < n2) & (y >= 0) & (y < n1) & (z >= 0) & (z < n0)
        vox = np.where(inside, (z * n1 + y) * n2 + x, 0)
        v = fv.reshape(f, -1)[:, vox].T
        if vnorm is not None:
            v = v / np.asarray(vnorm, dtype=F32)[vox][:, None]
        return np.where(inside[:, None], v, F32(0.0)).astype(F32)
    vals, wgts, ins = _corner_terms(feat, rel, vnorm, F32)
    res = np.zeros(vals.shape[1:], dtype=F32)
    for v, w, i in zip(vals, wgts, ins):
        term = (v * w[:, None]).astype(F32)
        res = np.where(i[:, None], (res + term).astype(F32), res)
    return res


SAMPLE_ROUNDINGS = 13     # see sample_ref


def sample_ref(feat, rel, mode, vnorm=None):
    """(ref, bound), float64 [A][F]: the same operation in fp64 from the same fp32 positions, and what an fp32 kernel of the
    stated order may differ by.  Trilinear: a term val * w goes through at most
        5  roundings of the weight: one per 1-D weight (ix - fx, (fx + 1) - ix; exact in fp64) and two products,
        1  for val * w,
        7  additions (the first one, to 0, is exact; eight corners),
    13 in all, and one more where voxel_norm divides val: bound = 13 (14) * 2^-24 * sum over the corners inside of |w v|.
    (The second-order terms are 78 * 2^-48 of that sum; the eighth corner's term sees 7 roundings, not 13.)  Nearest: the
    voxel itself, exactly; one rounding of the quotient with voxel_norm."""
    if mode == 'nearest':
        f = feat.shape[0]
        n0, n1, n2 = feat.shape[1:]
        z, y, x = [np.rint(sample_pos32(rel[:, ax], n)).astype(np.int64) for ax, n in enumerate((n0, n1, n2))]
        inside = (x >= 0) & (x < n2) & (y >= 0) & (y < n1) & (z >= 0) & (z < n0)
        vox = np.where(inside, (z * n1 + y) * n2 + x, 0)
        v = feat.double().numpy().reshape(f, -1)[:, vox].T
        if vnorm is not None:
            v = v / np.asarray(vnorm, dtype=np.float64)[vox][:, None]
        ref = np.where(inside[:, None], v, 0.0)
        return ref, (U * np.abs(ref) if vnorm is not None else np.zeros_like(ref))
    vals, wgts, _ = _corner_terms(feat.double().numpy(), rel, None if vnorm is None else np.asarray(vnorm, dtype=np.float64), np.float64)
    terms = vals * wgts[:, :, None]
    count = SAMPLE_ROUNDINGS + (1 if vnorm is not None else 0)
    return terms.sum(0), count * U * np.abs(terms).sum(0)


def grid_sample_cpu(feat, rel, mode):
    """The operator the reference runs (infer.py:48-72), on the CPU in fp32: [A][F]."""
    grid = torch.from_numpy(np.ascontiguousarray(rel[:, ::-1]))[None, None, None]          # x <-> last volume dim
    out = F.grid_sample(feat.float()[None], grid, mode=mode, padding_mode='zeros', align_corners=False)
    return out[0, :, 0, 0].T.contiguous().numpy()


# ============================================================================================== 3. class maps, modes 1 and 2
GRID_SPLIT = sd.TWO_TILES                         # 8 x 8 x 12 = 768 voxels: % 4 == 0, more than 256 * 2
MODE2_GROUPS = ((3,) * 7, (8, 8, 8), (2,) * 12, (35, 35))
MODE2_EXPO = (1.0, 1.5, 2.0)
MODE1_COUNTS = ((17,), (1030,))
LATTICE2_W = (1.0, 1.5, -0.5, -1.0, 4.0)          # mode 2 on the lattice: clamp(w, 0, 1) ** expo is 0 or 1 for every expo
LATTICE2_ACT = (1.0, 1.0, 0.0, 0.0, 1.0)


def form_of(grid, f, split):
    """The VALU kernel vittf_similarity_maps_f32 must report for a mode 1 / 2 call (sim_route.h)."""
    return 'sim_accumulate_split' if split and f % 4 == 0 and int(np.prod(grid)) % 4 == 0 else 'sim_accumulate'


def mode2_data(grid, counts, f, half, seed, normalized=True):
    """sim_data.correlated's volume (fp16, or its fp32 original) with queries scaled so that the dots spread over
    [-0.6, 5]: query a is its volume column times a factor between -0.6 and 5 (columns correlate at about 0.33, the own
    voxel at 1) plus 0.02 randn -- some dots below 0, some above 1."""
    g = torch.Generator().manual_seed(seed)
    x = sd._volume(grid, f, g)
    x = F.normalize(x, dim=0) if normalized else x
    X = x.half() if half else x.float()
    a = int(sum(counts))
    vnorm = None if normalized else X.double().norm(dim=0).clamp_min(1e-12).float()
    cols = torch.randint(0, X.shape[1], (a,), generator=g)
    base = X.float()[:, cols].T
    if not normalized:
        base = base / vnorm[cols][:, None]
    scale = torch.linspace(-0.6, 5.0, a)[torch.randperm(a, generator=g)]
    scale[torch.as_tensor(sd.starts_of(counts)[1:] - 1, dtype=torch.long)] = 1.5      # the last query of a group counts: dropping it shows
    q = (base * scale[:, None] + 0.02 * torch.randn(a, f, generator=g)).float().contiguous()
    return SimpleNamespace(X=X.contiguous(), q=q, counts=tuple(counts), vnorm=vnorm, grid=tuple(grid), f=f)


def unit_queries(grid, half, seed=0):
    """The K_LOG measurement's data: a volume of 48 features with arbitrary values in (-0.2, 1.2) (fp32: all 24 bits; fp16:
    fp16 values) and the 48 one-hot queries e_f in groups of one, so that s(f, v) = x_fv EXACTLY in any order of summation
    and clamp(s) ** 1 = clamp(x_fv) is known exactly."""
    g = torch.Generator().manual_seed(seed + 5)
    nvox = int(np.prod(grid))
    x = torch.rand(48, nvox, generator=g) * 1.4 - 0.2
    x[:, ::7] = torch.exp2(-torch.rand(48, len(range(0, nvox, 7)), generator=g) * 20)      # small arguments: |log2 c| up to 20
    X = x.half() if half else x.float()
    return SimpleNamespace(X=X.contiguous(), q=torch.eye(48).contiguous(), counts=(1,) * 48, vnorm=None, grid=tuple(grid), f=48)


def k_log_observed(got, d):
    """What K_LOG would have to be for the worst argument of a unit_queries call with expo = 1:
    (|got - c| / c - 2 * 2^-24) / (ln 2 * 2^-24 * max(|log2 c|, 1)) over c in (0, 1); (worst, its c)."""
    c = d.X.double().clamp(0.0, 1.0)
    live = (c > 2.0 ** -120) & (c < 1)
    dev = ((torch.as_tensor(got).double() - c).abs() / c.clamp_min(1e-300) - 2 * U) / (np.log(2.0) * U * c.clamp_min(1e-300).log2().abs().clamp_min(1.0))
    dev = torch.where(live, dev, torch.zeros_like(dev))
    i = int(dev.argmax())
    return float(dev.flatten()[i]), float(c.flatten()[i])


def mode2_exact_points(d):
    """(mask [groups][nvox], value fp32 [groups][nvox]): where every query of a group sits on an exact point of mode 2
    (s + e_s <= 0 or s - e_s >= 1, sim_data.class_maps_ref), the map is fl32(ones / n) bit for bit."""
    Xd, qd = d.X.double(), d.q.double()
    s = qd @ Xd
    e_s = (d.f + 8) * U * (qd.abs() @ Xd.abs()) + 0.5 * U * Xd.abs().sum(0)
    if d.vnorm is not None:
        nv = d.vnorm.double()
        e_s = (e_s + U * (s.abs() + e_s)) / nv
        s = s / nv
    zero, one = s + e_s <= 0, s - e_s >= 1
    st = sd.starts_of(d.counts)
    mask = torch.stack([(zero | one)[st[c]:st[c + 1]].all(0) for c in range(len(d.counts))])
    ones = torch.stack([one[st[c]:st[c + 1]].sum(0) for c in range(len(d.counts))]).float()
    return mask, ones / torch.tensor(d.counts, dtype=torch.float32)[:, None]


def lattice2(grid, counts, f, seed):
    """sim_data.lattice with the weights LATTICE2_W: one-hot queries on 0 / 1 features, so s is 0 or the weight, and
    clamp(s, 0, 1) ** expo is exactly 0 or 1 for every expo -- 1.5 is clamped, -0.5 and -1 are cut.  .sums: exact sum_a a."""
    d = sd.lattice(grid, counts, f, seed)
    w_idx = torch.tensor([sd.LATTICE_W.index(float(w)) for w in d.q[torch.arange(len(d.feat)), d.feat]])
    q = torch.zeros_like(d.q)
    q[torch.arange(len(d.feat)), d.feat] = torch.tensor(LATTICE2_W)[w_idx]
    act = torch.tensor(LATTICE2_ACT, dtype=torch.float64)[w_idx]
    lit = d.X[d.feat].double()
    st = sd.starts_of(counts)
    sums = torch.stack([(act[st[c]:st[c + 1], None] * lit[st[c]:st[c + 1]]).sum(0) for c in range(len(counts))])
    return SimpleNamespace(X=d.X, q=q.contiguous(), counts=tuple(counts), vnorm=None, grid=tuple(grid), f=f, sums=sums, act=act, feat=d.feat)


def lattice1_candidates(d):
    """Mode 1 on sim_data.lattice: the dots are 0 or a weight, their sum S is exact in fp32 in any order, t = S / n is one
    IEEE division, and where(t >= 0.25, t * t * sqrt(t), 0) is three correctly rounded operations: fp32 [3][classes][nvox],
    the activation of fl(S / n) and of its two fp32 neighbours (no more is assumed of the division than one ulp; a power-of-two
    count divides exactly: the first candidate)."""
    w = d.q[torch.arange(len(d.feat)), d.feat].double()
    lit = d.X[d.feat].double()
    st = sd.starts_of(d.counts)
    S = torch.stack([(w[st[c]:st[c + 1], None] * lit[st[c]:st[c + 1]]).sum(0) for c in range(len(d.counts))])
    assert torch.equal(S.float().double(), S)
    t = S.float().numpy() / np.array(d.counts, dtype=F32)[:, None]            # one fp32 division (S is exact in fp32)
    out = []
    for cand in (t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf))):
        with np.errstate(invalid='ignore'):
            a = (cand * cand).astype(F32) * np.sqrt(np.maximum(cand, F32(0))).astype(F32)
        out.append(np.where(cand >= F32(0.25), a.astype(F32), F32(0.0)))
    return torch.from_numpy(np.stack(out)), S


def _thresh_pow32(t):
    """where(t >= 0.25, t * t * sqrt(t), 0) in numpy float32: three correctly rounded operations, like the kernel's (torch's
    CPU sqrt is not correctly rounded on every machine)."""
    x = t.numpy()
    a = (x * x).astype(F32) * np.sqrt(np.maximum(x, F32(0.0))).astype(F32)
    return torch.from_numpy(np.where(x >= F32(0.25), a.astype(F32), F32(0.0)))


def emulate_modes(d, mode, expo=0.0, mutant=None):
    """float32 torch restatement of the VALU kernels in mode 1 (sum of the dots, / n, where(t >= 0.25) t * t * sqrt(t)) and
    mode 2 (exp2(expo * log2(clamp(s, 0, 1))), group sum, / n), and subtly wrong kernels:
      'expo_2.5'     mode 2: exponent 2.5 whatever expo says        'no_clamp'    mode 2: no clamp at 1
      'mean_16'      the sum divided by the 16 of a chunk            'act_first'   mode 1: the activation before the mean
      'drop_last'    the last annotation of every class left out of its sum (the count stays)"""
    s = d.q @ d.X.float()
    if d.vnorm is not None:
        s = s / d.vnorm
    st = sd.starts_of(d.counts)
    out = torch.empty(len(d.counts), d.X.shape[1])

    class _Div:                                      # numpy's IEEE division (torch divides by a scalar with a reciprocal)
        def __init__(self, n):
            self.n = np.float32(n)

        def __rtruediv__(self, t):
            return torch.from_numpy(t.numpy() / self.n)
    for c, n in enumerate(d.counts):
        rows = s[st[c]:st[c + 1] - (1 if mutant == 'drop_last' else 0)]
        div = _Div(16 if mutant == 'mean_16' else n)
        if mode == 1:
            if mutant == 'act_first':
                out[c] = _thresh_pow32(rows).sum(0) / div
                continue
            out[c] = _thresh_pow32(rows.sum(0) / div)
        else:
            cl = rows.clamp_min(0.0) if mutant == 'no_clamp' else rows.clamp(0.0, 1.0)
            e = np.float32(2.5 if mutant == 'expo_2.5' else expo)
            a = torch.where(cl > 0, torch.exp2(e * torch.log2(cl.clamp_min(1e-45))), torch.zeros_like(cl))
            out[c] = (a.sum(0) if a.shape[0] else torch.zeros(d.X.shape[1])) / div
    return out


def mode1_seed(counts, normalized):
    """Seeds of the mode-1 data (sim_data.correlated on GRID_SPLIT / ODD), chosen on reference-only quantities: the edge
    shares of sim_data.check_edge_share."""
    return 101 + int(sum(counts)) + (0 if normalized else 1)


@functools.lru_cache(maxsize=None)
def modes_case(mode, grid, counts, f, half, expo, normalized):
    """The data set of one mode 1 / 2 GPU case with its reference attached, computed once per process."""
    if mode == 1:
        d = sd.correlated(grid, counts, f, mode1_seed(counts, normalized), normalized)
    else:
        d = mode2_data(grid, counts, f, half, 211 + f + int(sum(counts)) + len(counts), normalized)
    d.ref, d.bound, d.edge = sd.class_maps_ref(d.X, d.q, d.counts, d.vnorm, mode=mode, expo=expo)
    return d


# The shapes of the mode 1 / 2 GPU cases: the odd grid has no split form (both settings of VITTF_SIM_SPLIT report
# sim_accumulate), F = 50 falls to the plain kernel on the split grid, the others take the split form there.
MODES_SHAPES = ((sd.ODD, 384), (GRID_SPLIT, 48), (GRID_SPLIT, 50), (GRID_SPLIT, 64), (GRID_SPLIT, 384))
LATTICE1_COUNTS = ((17,), (1030,), (16,), (64, 3))        # mode 1 takes any class list; two powers of two for the exact quotient


def shape_id(shape):
    return f'{"x".join(map(str, shape[0]))}-f{shape[1]}'


def counts_id(counts):
    return f'{counts[0]}x{len(counts)}' if len(set(counts)) == 1 and len(counts) > 1 else '-'.join(map(str, counts))


# ============================================================================================== 4. mean pairwise distance
PAIR_N = (1, 2, 60, 257, 600)
PAIR_F = (1, 24, 384, 1000, 8192)
PAIR_KINDS = ('random', 'scaled_1e3', 'scaled_1e-3', 'zero_row', 'twins')


def pair_kind(n, f):
    """A Latin square over the 25 shapes: every kind meets every n and every f once."""
    return PAIR_KINDS[(PAIR_N.index(n) + PAIR_F.index(f)) % len(PAIR_KINDS)]


def pair_rows(n, f, kind, seed=0):
    """fp32 rows [n][f]: randn + 0.3 (so that the cosines have a mean), scaled by 1e3 or 1e-3, with one all-zero row (the
    1e-8 clamp of F.cosine_similarity) or one pair of identical rows (a euclidean term of exactly 0)."""
    g = torch.Generator().manual_seed(seed + 13 * n + f)
    x = torch.randn(n, f, generator=g) + 0.3
    if kind == 'scaled_1e3':
        x = x * 1e3
    elif kind == 'scaled_1e-3':
        x = x * 1e-3
    elif kind == 'zero_row':
        x[n // 2] = 0.0
    elif kind == 'twins' and n >= 2:
        x[n - 1] = x[n // 3]
    return x.float().contiguous()


def pair_ref(x, measure):
    """(ref, bound) float64 [n] of vittf_mean_pairwise_distance: fp64 row by row, and the fp32 kernel's distance from it.
    Cosine.  dot and the two squared norms are f-term fp32 FMA chains: |dot^ - dot| <= f u sum|a b|, n^ = n (1 + f u); the
    correctly rounded sqrt halves that and adds one rounding, the product of the two norms one more, the division another:
        e_ij = (f u sum_c |a_c b_c| / den + |cos_ij| (f + 4) u) (1 + 2 (f + 4) u),    den = max(|a|, 1e-8) max(|b|, 1e-8)
    (a zero row has dot = 0 and gives exactly 0).  Euclidean.  d_c = a_c - b_c is one rounding, its square two, the chain f:
    d2^ = d2 (1 + (f + 2) u); the sqrt halves it and adds one:  e_ij = |a - b| (f / 2 + 2) u (1 + (f + 2) u); identical
    rows give exactly 0.  The terms are added and divided by n in fp64 ((n + 2) 2^-53 of their sum), the mean is rounded to
    fp32 (u |mean|) and cosine's 1 - mean once more (u |1 - mean|)."""
    xd = torch.as_tensor(x).double()
    n, f = xd.shape
    if measure == 'cosine':
        norm = xd.norm(dim=1).clamp_min(1e-8)
        den = norm[:, None] * norm[None]
        cos = (xd @ xd.T) / den
        e = (f * U * (xd.abs() @ xd.abs().T) / den + cos.abs() * (f + 4) * U) * (1 + 2 * (f + 4) * U)
        mean = cos.mean(0)
        bound = e.mean(0) * (1 + 2 * U) + (n + 2) * 2.0 ** -53 * cos.abs().mean(0) + U * mean.abs() + U * (1 - mean).abs()
        return 1.0 - mean, bound
    dist = _cdist64(xd)
    e = dist * (f / 2 + 2) * U * (1 + (f + 2) * U)
    mean = dist.mean(0)
    return mean, e.mean(0) * (1 + 2 * U) + (n + 2) * 2.0 ** -53 * mean + U * mean


def _cdist64(xd):
    """fp64 distances: by differences while that is small, else from the Gram matrix (the cancellation costs 2^-53 f of the
    squared norms, nothing beside f 2^-24 of the distance for rows that are not near-copies) with identical rows set to 0."""
    n, f = xd.shape
    if n * n * f <= 2 ** 25:
        return torch.cdist(xd, xd, compute_mode='donot_use_mm_for_euclid_dist')
    sq = (xd * xd).sum(1)
    dist = (sq[:, None] + sq[None] - 2 * (xd @ xd.T)).clamp_min(0).sqrt()
    same = (xd[:, None, :64] == xd[None, :, :64]).all(-1)
    for i, j in same.nonzero().tolist():
        if torch.equal(xd[i], xd[j]):
            dist[i, j] = 0.0
    return dist


def pair_emulate(x, measure, mutant=None):
    """float32 torch restatement (matrix products for the chains); 'stride_once': the j loop that never takes its second
    trip (rows from 256 on are missing from the sum, the count stays)."""
    x = torch.as_tensor(x).float()
    n = x.shape[0]
    if measure == 'cosine':
        norm = (x * x).sum(1).sqrt().clamp_min(1e-8)
        t = (x @ x.T) / (norm[:, None] * norm[None])
    else:
        t = torch.cdist(x, x, compute_mode='donot_use_mm_for_euclid_dist')
    if mutant == 'stride_once':
        t = t[:256]
    mean = (t.double().sum(0) / n).float()
    return 1.0 - mean if measure == 'cosine' else mean


DISSIMILAR = SimpleNamespace(n=600, f=24, k=35)


def dissimilar_rows(measure):
    """take_most_dissimilar end to end: 600 rows of 24 features whose lengths and directions spread (so that the mean
    distances do), with the seed chosen on fp64 quantities: the gap between the 35th and the 36th largest distance exceeds
    the sum of their bounds (tests/test_refine_data_cpu.py asserts it)."""
    g = torch.Generator().manual_seed({'cosine': 2, 'euclidean': 2}[measure])
    n, f = DISSIMILAR.n, DISSIMILAR.f
    x = torch.randn(n, f, generator=g) + torch.linspace(0.0, 2.0, n)[torch.randperm(n, generator=g)][:, None]
    x = x * (0.5 + torch.rand(n, 1, generator=g))
    return x.float().contiguous()


def dissimilar_gap(x, measure):
    """(fp64 set of the k most dissimilar rows, gap between the k-th and (k+1)-th distance, the sum of their bounds)."""
    ref, bound = pair_ref(x, measure)
    order = torch.argsort(ref, descending=True)
    a, b = order[DISSIMILAR.k - 1], order[DISSIMILAR.k]
    return set(order[:DISSIMILAR.k].tolist()), float(ref[a] - ref[b]), float(bound[a] + bound[b])


# ============================================================================================== 5. resample_topk
RESAMPLE = SimpleNamespace(grid=GRID_SPLIT, classes=2, annotations=3, f=48)


def resample_data(half, seed=0):
    """(feat [F][8][8][12] unit columns in fp16 or fp32, sims fp32 [2][3][8][8][12]): similarity maps quantised to 64
    levels, so the k-th value of a map is usually tied."""
    g = torch.Generator().manual_seed(seed + 77)
    x = F.normalize(sd._volume(RESAMPLE.grid, RESAMPLE.f, g), dim=0)
    feat = (x.half() if half else x.float()).reshape(RESAMPLE.f, *RESAMPLE.grid).contiguous()
    sims = (torch.rand(RESAMPLE.classes, RESAMPLE.annotations, *RESAMPLE.grid, generator=g) * 64).floor() / 64
    return feat, sims.float().contiguous()


def resample_ref(feat, sims, K, expo, mode):
    """resample_topk's stages on the CPU: the expression's indices [groups][K], their relative coordinates as the Python
    function forms them (fp32, one operation at a time), the queries of section 2's emulation, and section 3's mode-2
    reference: (idx, ref, bound), ref / bound float64 [groups][nvox]."""
    dims = tuple(feat.shape[1:])
    groups = sims.shape[0] * sims.shape[1]
    idx = topk_ref(sims.reshape(groups, -1), K)
    flat = idx.reshape(-1)
    coords = torch.stack((flat // (dims[1] * dims[2]), (flat // dims[2]) % dims[1], flat % dims[2]), -1).float()
    rel = ((coords + 0.5) / torch.tensor(dims, dtype=torch.float32) * 2.0 - 1.0).numpy()
    q = torch.from_numpy(sample_emulate(feat, rel, mode))
    ref, bound, _ = sd.class_maps_ref(feat.reshape(feat.shape[0], -1), q, (K,) * groups, mode=2, expo=expo)
    return idx, q, ref, bound
