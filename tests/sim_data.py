"""Host-only data, fp64 reference and error bound for the fp32 class maps of the similarity kernels (csrc/sim_mfma.hip,
csrc/similarity.hip): torch on the CPU, no GPU, no library call.  tests/test_sim_data_cpu.py checks every property the GPU
tests of tests/test_gpu_similarity_maps.py rest on, so that a failure there is the kernel's and not the generator's.

Conventions: a volume X is fp16 [F][nvox] (the F-major file layout), queries q are fp32 [A][F] in class order, `counts` are
the annotations per class; a class map is map[c][v] = mean over the class's annotations of where(s >= 0.25, s, 0) ** 2.5
with s = q . x_v (divided by vnorm[v] on the cosine path): predict_ntf.py:65, 71-72."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                            # half an ulp of fp32, relative: one rounding
TILE = 256                                # voxels of one matrix-core workgroup tile


def starts_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- reference and bound
K_LOG = 3.71                              # v_log_f32: absolute error of log2 c in units of 2^-24 max(|log2 c|, 1); MEASURED, see below
TINY_F32 = 2.0 ** -126                    # smallest normal fp32: what a flushed denormal argument or result can cost


def class_maps_ref(X, q, counts, vnorm=None, mode=0, expo=0.0):
    """fp64 class maps and a bound on what an fp32 kernel may differ by: (ref, bound, edge), each [classes][nvox]; ref and
    bound are float64, edge is bool.  mode 0 (below) is predict_ntf's map, modes 1 and 2 (at the end) are the two other
    forms vittf_similarity_maps_f32 takes; X is the fp16 volume, for mode 2 also an fp32 one.

    The bound is derived from the arithmetic the kernels state, entry by entry; none of its constants is fitted.

    Dot product.  The volume is fp16 exactly and a product of an fp16 and an fp32 value (or of two fp16 halves) is exact in
    fp32.  The matrix-core kernels split a query into fp16 hi + lo halves: q = hi + lo up to 2^-22 |q| (lo is rounded to 11
    bits of a remainder below 2^-11 |q|), and a lo half below the fp16 normal range is rounded to a multiple of 2^-24,
    i.e. is off by at most 2^-25 per element.  The exact products are accumulated in fp32; every rounding on the way costs
    at most 2^-24 of the magnitudes summed so far, and F roundings is the worst case of the forms in use: a single FMA
    chain over the F features (sim_accumulate), four quarter chains and two adds (sim_accumulate_split), and 2 F / 16
    MFMA steps, each of which adds its 16 products to the accumulator with fewer roundings than 8 FMAs would.  Together
        e_s = (F + 8) 2^-24 sum_f |q_f x_fv| + 2^-25 sum_f |x_fv|:
    worst-case accumulation, the split (4 of the 8) and the lo half that underflows -- the projection's bound of
    DESIGN.md 4.8.  On the cosine path the fp32 quotient s / nv adds one rounding: e_s <- (e_s + 2^-24 (|s| + e_s)) / nv
    and s <- s / nv.

    Activation.  Where s + e_s < 0.25 both sides give exactly 0.  Elsewhere t -> t ** 2.5 has the increasing derivative
    2.5 t ** 1.5, so moving s by e_s moves it by at most 2.5 max(s + e_s, 0.25) ** 1.5 e_s, and s * s * sqrt(s) with a
    correctly rounded sqrt is three roundings, (1 + 2^-24) ** 3 - 1 < 4 * 2^-24 relative also after the move:
        e_a = 2.5 max(s + e_s, 0.25) ** 1.5 e_s + 4 * 2^-24 a.

    Threshold.  Where |s - 0.25| <= e_s the fp32 and the fp64 value may fall on different sides of 0.25; one side is then 0
    and the other at most (0.25 + e_s) ** 2.5, which is added to e_a of that pair, and edge[c][v] is set if the class has
    such a pair at voxel v.  The entry stays in the comparison.

    Class mean.  The n_c non-negative activations are summed in fp32, in any order, and divided by n_c: at most
    (n_c - 1) + 1 roundings, (n_c + 2) 2^-24 sum_a a with the second-order terms.  So
        bound[c][v] = (sum_a e_a + (n_c + 2) 2^-24 sum_a a) / n_c.

    Mode 1 (mean of the dots first: t = (sum_a s_a) / n_c, then where(t >= 0.25, t, 0) ** 2.5; VALU kernels only, whose
    FMA chain over an fp32 or fp16 volume has the F roundings e_s already counts).  The n_c dots are summed in fp32 in any
    order and divided: e_t = (sum_a e_s + (n_c + 2) 2^-24 sum_a |s_a|) / n_c.  Activation and threshold are those of mode 0
    applied once, to t with e_t; edge marks |t - 0.25| <= e_t, and no class mean follows: bound = e_a(t, e_t).

    Mode 2 (resample_topk: a = clamp(s, 0, 1) ** expo per query, group mean; expo >= 1).  The kernel computes
    c = min(max(s, 0), 1) and a = c > 0 ? exp2(expo * log2 c) : 0 with v_log_f32 and v_exp_f32.
      Exact points, no constant: s + e_s <= 0 gives 0 on both sides; s - e_s >= 1 gives c = 1, log2 1 = 0, expo * 0 = 0,
      exp2 0 = 1 on both sides.  e_a = 0 there.
      Elsewhere the clamp is 1-Lipschitz and c ** expo has the increasing derivative expo c ** (expo - 1), so moving s by e_s
      moves a by at most expo hi ** (expo - 1) e_s with hi = min(s + e_s, 1).  On the computed c (anywhere in [lo, hi],
      lo = max(s - e_s, 2^-149)) the exponent p = expo log2 c is off by
          dp = expo K_LOG 2^-24 lg + 2^-24 expo lg (1 + K_LOG 2^-24),     lg = max(|log2 lo|, 1):
      v_log_f32's absolute error K_LOG 2^-24 max(|log2 c|, 1) times expo, and the one rounding of the product (expo = 1:
      none, the term stays); 2 ** (p + dp) = 2 ** p (1 + expm1(ln 2 dp)); v_exp_f32 adds 1 ulp = 2 * 2^-24 relative, as
      tests/svm_data.py and tests/knn_data.py assume of it; a denormal c or result may be flushed, 2^-126 absolute:
          e_a = expo hi ** (expo - 1) e_s + hi ** expo (expm1(ln 2 dp) (1 + 2 * 2^-24) + 2 * 2^-24) + 2^-126.
      K_LOG is the one constant that is measured, not derived: vittf_similarity_maps_f32 in mode 2 with expo = 1 on data
      whose dots are exact (tests/refine_data.py: unit_queries; c ** 1 = c is then known exactly and the whole deviation is
      the two instructions'), about 28000 arguments in (0, 1) from an fp32 volume and as many from an fp16 one.  Worst observed
      (|got - c| / c - 2 * 2^-24) / (ln 2 * 2^-24 max(|log2 c|, 1)) on an MI355X: 1.8534 (at c = 1.485e-5: 0.93 ulp of
      log2 c = -16.04; fp16 volume 1.8013; the same in both kernel forms).  K_LOG = 3.71 is twice that, because a sample
      of the arguments was measured and not all of them.
    The group mean is mode 0's: bound = (sum_a e_a + (n_c + 2) 2^-24 sum_a a) / n_c.  edge is all False."""
    assert mode in (0, 1, 2) and (mode != 2 or expo >= 1.0)
    Xd = torch.as_tensor(X).double()
    qd = torch.as_tensor(q).double()
    f, nvox = Xd.shape
    assert qd.shape == (int(sum(counts)), f)
    Xa = Xd.abs()
    xabs = Xa.sum(0)
    nv = None if vnorm is None else torch.as_tensor(vnorm).double()
    ref = torch.empty(len(counts), nvox, dtype=torch.float64)
    bound = torch.empty_like(ref)
    edge = torch.empty(len(counts), nvox, dtype=torch.bool)
    st = starts_of(counts)
    for c, n in enumerate(counts):                        # class by class: a 1024-annotation class is 70 MB per array
        qc = qd[st[c]:st[c + 1]]
        s = qc @ Xd
        e_s = (f + 8) * U * (qc.abs() @ Xa) + 0.5 * U * xabs
        if nv is not None:
            e_s = (e_s + U * (s.abs() + e_s)) / nv
            s = s / nv
        if mode == 1:
            e_s = ((e_s.sum(0) + (n + 2) * U * s.abs().sum(0)) / n)[None]
            s, n = (s.sum(0) / n)[None], 1
        elif mode == 2:
            lo, hi = (s - e_s).clamp(2.0 ** -149, 1.0), (s + e_s).clamp(0.0, 1.0)
            lg = lo.log2().abs().clamp_min(1.0)
            dp = expo * K_LOG * U * lg + U * expo * lg * (1 + K_LOG * U)
            a = s.clamp(0.0, 1.0) ** expo
            e_a = expo * hi ** (expo - 1) * e_s + hi ** expo * (torch.expm1(np.log(2.0) * dp) * (1 + 2 * U) + 2 * U) + TINY_F32
            e_a = torch.where((s + e_s <= 0) | (s - e_s >= 1), torch.zeros_like(s), e_a)
            total = a.sum(0)
            ref[c] = total / n
            bound[c] = (e_a.sum(0) + (n + 2) * U * total) / n
            edge[c] = False
            continue
        a = torch.where(s >= 0.25, s, torch.zeros_like(s)) ** 2.5
        live = s + e_s >= 0.25
        near = (s - 0.25).abs() <= e_s
        e_a = torch.where(live, 2.5 * (s + e_s).clamp_min(0.25) ** 1.5 * e_s + 4 * U * a, torch.zeros_like(s))
        e_a = e_a + near * (0.25 + e_s) ** 2.5
        total = a.sum(0)
        ref[c] = total / n
        bound[c] = e_a.sum(0) if mode == 1 else (e_a.sum(0) + (n + 2) * U * total) / n
        edge[c] = near.any(0)
    return ref, bound, edge


def worst(got, ref, bound):
    """(ratio, class, voxel) of the entry with the largest |got - ref| / bound; an entry with bound 0 must be exact."""
    err = (torch.as_tensor(got).double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i // ref.shape[1], i % ref.shape[1]


def where_in_kernel(v):
    """Voxel -> the matrix-core kernels' coordinates: 256-voxel tile, wave of the workgroup, lane (voxel of the wave's 32)."""
    return f'tile {v // TILE}, wave {v % TILE // 32}, lane {v % 32}'


# ---------------------------------------------------------------------------------------------- data
def _volume(grid, f, g):
    """The recipe of tests/test_gpu_kernels.py's matrix-core cases: unit-norm randn columns plus 0.7 of one column, so that
    every pair of voxels has a cosine of about 0.33 +- 0.05 and the 0.25 threshold cuts through the distribution."""
    nvox = int(np.prod(grid))
    x = F.normalize(torch.randn(f, nvox, generator=g), dim=0)
    return x + 0.7 * x[:, nvox // 3:nvox // 3 + 1]


def correlated(grid, counts, f, seed, normalized=True):
    """X fp16 unit columns (normalized=False: left at their norm of about 1.2, vnorm = max(|x_v|_2, 1e-12) in fp32 for the
    cosine path); queries = (normalised) volume columns at random voxels + 0.02 randn in fp32, not fp16-representable."""
    g = torch.Generator().manual_seed(seed)
    x = _volume(grid, f, g)
    X = (F.normalize(x, dim=0) if normalized else x).half()
    a = int(sum(counts))
    vnorm = None if normalized else X.double().norm(dim=0).clamp_min(1e-12).float()
    cols = torch.randint(0, X.shape[1], (a,), generator=g)
    base = X.float()[:, cols].T
    if not normalized:
        base = base / vnorm[cols][:, None]
    q = (base + 0.02 * torch.randn(a, f, generator=g)).float().contiguous()
    return SimpleNamespace(X=X.contiguous(), q=q, counts=tuple(counts), vnorm=vnorm, grid=tuple(grid), f=f)


def coherent_tails(grid, counts, f, seed):
    """Annotation a targets its own voxel v_a with the query h (1 + 2^-12), h the fp16 column of v_a: exact in fp32 (11 + 12
    bits), fp16(q) == h (the tail is below half an fp16 ulp of h), and every lo-half product with x_{v_a} = h is positive.
    A kernel that loses the lo halves moves s(a, v_a) by 2^-12 sum_f h_f ** 2 = 2^-12, ten times e_s.  .targets: v_a."""
    g = torch.Generator().manual_seed(seed)
    X = F.normalize(_volume(grid, f, g), dim=0).half()
    a = int(sum(counts))
    assert a <= X.shape[1], 'every annotation needs a voxel of its own'
    targets = torch.randperm(X.shape[1], generator=g)[:a]
    h = X[:, targets].T.float()
    q = (h * (1.0 + 2.0 ** -12)).contiguous()
    assert torch.equal(q.double(), h.double() * (1.0 + 2.0 ** -12)) and torch.equal(q.half().float(), h)
    return SimpleNamespace(X=X.contiguous(), q=q, counts=tuple(counts), vnorm=None, grid=tuple(grid), f=f, targets=targets)


LATTICE_W = (1.0, 0.25, 0.125, -1.0, 4.0)          # query weights ...
LATTICE_ACT = (1.0, 2.0 ** -5, 0.0, 0.0, 32.0)     # ... and their activations: 0.25 sits ON the threshold (>=, not >)
_LATTICE_CYCLE = (1, 0, 4, 2, 1, 0, 3, 4)          # weights of the inner annotations of a class, by position


def lattice(grid, counts, f, seed):
    """Data on which the maps are exact.  Feature entries are 0 or 1 (a quarter lit, seeded), annotation i of a class is
    w_i e_{f_i}: one-hot, weight from LATTICE_W, so s(i, v) is 0 or w_i, the activation 0 or LATTICE_ACT, and sum_a a at
    (class, voxel) a multiple of 2^-5 below 2^15 * 32: every dot product, product and sum is exact in fp32 in any order, and
    the hi + lo split has lo = 0.  The first annotation of a class weighs 1 (odd classes: 0.25) and the last one 4 (the padding
    row behind a class and the neighbouring class's first query both count), the others cycle through all five weights, so the sum
    changes by 2^-5, 1 or 32 wherever an annotation with a non-zero activation is dropped, duplicated or counted into the
    next class and its feature is lit.  The features of a class are a seeded permutation (more annotations than features:
    several share one).  .sums: the exact sum_a a, float64 [classes][nvox]; .act, .feat: per annotation."""
    g = torch.Generator().manual_seed(seed)
    nvox = int(np.prod(grid))
    bits = torch.rand(f, nvox, generator=g) < 0.25
    w_idx, feat = [], []
    for c, n in enumerate(counts):
        perm = torch.randperm(f, generator=g)
        for i in range(n):
            w_idx.append(c % 2 if i == 0 else 4 if i == n - 1 else _LATTICE_CYCLE[(i - 1) % len(_LATTICE_CYCLE)])
            feat.append(int(perm[i % f]))
    w_idx, feat = torch.tensor(w_idx), torch.tensor(feat)
    a = len(feat)
    q = torch.zeros(a, f)
    q[torch.arange(a), feat] = torch.tensor(LATTICE_W)[w_idx]
    act = torch.tensor(LATTICE_ACT, dtype=torch.float64)[w_idx]
    lit = bits[feat].double()                                                     # [A][nvox]
    st = starts_of(counts)
    sums = torch.stack([(act[st[c]:st[c + 1], None] * lit[st[c]:st[c + 1]]).sum(0) for c in range(len(counts))])
    return SimpleNamespace(X=bits.half().contiguous(), q=q.contiguous(), counts=tuple(counts), vnorm=None, grid=tuple(grid), f=f,
                           sums=sums, act=act, feat=feat)


# ---------------------------------------------------------------------------------------------- the GPU cases
# One row per call of vittf_similarity_maps_f32 that tests/test_gpu_similarity_maps.py makes: the kernel form it must reach
# (asserted by name), the switches the library reads per call, and the smallest shapes at which that form can go wrong.
# tests/test_sim_data_cpu.py walks the same list for the reference-only conditions.
Case = functools.partial(SimpleNamespace, f=384)
G, ODD, TWO_TILES, CUBE, BIG, TINY = (24, 20, 18), (7, 9, 11), (8, 8, 12), (16, 16, 16), (48, 48, 50), (2, 2, 2)
ONE_BLOCK = {'VITTF_SIM_MFMA_VB': '1'}
TWO_BLOCKS = {'VITTF_SIM_MFMA_VB': '2', 'VITTF_SIM_MFMA_MIN': '2'}
FEW = {'VITTF_SIM_MFMA_MIN': '1'}
VALU = {'VITTF_SIM_MFMA_MIN': '1000000'}
SWITCHES = ('VITTF_SIM_MFMA_MIN', 'VITTF_SIM_MFMA_VB', 'VITTF_SIM_SPLIT')

GPU_CASES = [
    # sim_mfma_kernel, LDS-DMA, one voxel block per wave: 8640 voxels = 33.75 tiles
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=G, counts=(70, 3, 33)),
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=G, counts=(32, 33, 64, 1)),            # chunk boundaries
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=G, counts=(1024, 200)),
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=G, counts=(2,) * 40),                  # > 32 classes: device tables
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=G, counts=tuple(range(1, 34))),
    # 8 voxels: every staged chunk is the clamped one.  (One class of at most 32 annotations is the few-query kernel's, see
    # below, so the one-block kernel gets the 9 with a second class behind it.)
    Case(kernel='sim_mfma_kernel', env=ONE_BLOCK, grid=TINY, counts=(9, 2)),
    # strided loads: rows that are not 16-byte aligned
    Case(kernel='sim_mfma_kernel', env={}, grid=ODD, counts=(70, 3, 33)),
    # two voxel blocks per wave
    Case(kernel='sim_mfma_kernel<2 voxel blocks>', env=TWO_BLOCKS, grid=G, counts=(70, 3, 33)),
    Case(kernel='sim_mfma_kernel<2 voxel blocks>', env=TWO_BLOCKS, grid=G, counts=(1024, 3)),
    Case(kernel='sim_mfma_kernel<2 voxel blocks>', env=TWO_BLOCKS, grid=TWO_TILES, counts=(70, 3, 33)),   # second half of the last workgroup: behind the volume
    Case(kernel='sim_mfma_kernel<2 voxel blocks>', env=TWO_BLOCKS, grid=CUBE, counts=(1,) * 5 + (40,)),
    # F = 768: two 48 KB units per query chunk
    Case(kernel='sim_mfma_kernel<F 768>', env={}, grid=CUBE, counts=(70, 3, 33), f=768),
    Case(kernel='sim_mfma_kernel<F 768>', env={}, grid=CUBE, counts=(2,) * 40, f=768),
    Case(kernel='sim_mfma_kernel<F 768>', env={}, grid=G, counts=(70, 3, 33), f=768),
    Case(kernel='sim_mfma_kernel<F 768>', env={}, grid=G, counts=(2,) * 40, f=768),
    # the persistent few-query kernel: 34 tiles with the last one partial; the row-group test at 7 / 8 / 9
    *[Case(kernel='sim_mfma_few_kernel', env=FEW, grid=G, counts=(n,)) for n in (1, 7, 8, 9, 31, 32)],
    Case(kernel='sim_mfma_few_kernel', env=FEW, grid=BIG, counts=(16,)),     # 450 tiles: one to two per persistent workgroup
    Case(kernel='sim_mfma_few_kernel', env=FEW, grid=TINY, counts=(3,)),
    Case(kernel='sim_mfma_few_kernel', env=ONE_BLOCK, grid=TINY, counts=(9,)),   # (where one class of 9 goes, whatever VB says)
    # the VALU kernels: classes across several 16-annotation chunks, maps re-read between chunks; the odd voxel count has no
    # split form (8-byte loads), both settings run the plain kernel there
    Case(kernel='sim_accumulate_split', env={**VALU, 'VITTF_SIM_SPLIT': '1'}, grid=G, counts=(70, 3, 33)),
    Case(kernel='sim_accumulate', env={**VALU, 'VITTF_SIM_SPLIT': '0'}, grid=G, counts=(70, 3, 33)),
    Case(kernel='sim_accumulate', env={**VALU, 'VITTF_SIM_SPLIT': '1'}, grid=ODD, counts=(17, 16, 1, 40)),
    Case(kernel='sim_accumulate', env={**VALU, 'VITTF_SIM_SPLIT': '0'}, grid=ODD, counts=(17, 16, 1, 40)),
]


def case_id(case):
    counts = case.counts
    cs = f'{counts[0]}x{len(counts)}' if len(counts) > 4 and len(set(counts)) == 1 else \
        f'{counts[0]}..{counts[-1]}' if len(counts) > 8 else '-'.join(map(str, counts))
    env = '.'.join(f'{k.rsplit("_", 1)[1].lower()}{v}' for k, v in sorted(case.env.items())) or 'default'
    form = case.kernel.replace('<2 voxel blocks>', '_vb2').replace('<F 768>', '_f768')
    return f'{form}-{"x".join(map(str, case.grid))}-a{cs}-{env}'


def seed_of(case):
    """Cases on the same shapes share their data (and the reference computed from it).  The base was chosen on reference-only
    quantities: the edge shares of check_edge_share, and that the one query the 'drop_last' / 'pad_row' emulations move is
    above the threshold on at least 90 % of the voxels (tests/test_sim_data_cpu.py) -- where it is below, miscounting it
    changes nothing."""
    return 19 + sum(case.grid) * 131 + case.f + 17 * len(case.counts) + int(sum(case.counts))


@functools.lru_cache(maxsize=None)
def _data(kind, grid, counts, f, seed, normalized):
    if kind == 'correlated':
        d = correlated(grid, counts, f, seed, normalized)
    elif kind == 'tails':
        d = coherent_tails(grid, counts, f, seed)
    else:
        return lattice(grid, counts, f, seed)
    d.ref, d.bound, d.edge = class_maps_ref(d.X, d.q, d.counts, d.vnorm)
    return d


def case_data(case, kind, normalized=True):
    """The case's data set with its reference attached (.ref, .bound, .edge; the lattice has .sums), computed once per
    process and shared by every test that asks; nobody writes to it."""
    return _data(kind, tuple(case.grid), tuple(case.counts), case.f, seed_of(case), normalized)


def has_tails(case):
    return int(sum(case.counts)) <= int(np.prod(case.grid))


EDGE_CAP, EDGE_CAP_SMALL, SMALL_CLASS = 0.10, 0.01, 100


def check_edge_share(d):
    """The widened bound stays the exception: at most 10 % of the entries overall and 1 % of those of classes of at most
    100 annotations sit on the threshold.  Reference-only quantities; a seed that breaks a cap is replaced, never the cap."""
    small = torch.tensor([n <= SMALL_CLASS for n in d.counts])
    share = float(d.edge.float().mean())
    share_small = float(d.edge[small].float().mean()) if bool(small.any()) else 0.0
    assert share <= EDGE_CAP and share_small <= EDGE_CAP_SMALL, (share, share_small)
    return share, share_small


# ---------------------------------------------------------------------------------------------- fp32 emulations
def emulate(d, mutant=None):
    """float32 torch restatement of the matrix-core arithmetic -- hi @ X + lo @ X, s * s * sqrt(s) above the threshold, the
    class sum and the division -- and three subtly wrong kernels:
      'no_lo'      the queries rounded once to fp16;
      'drop_last'  the last annotation of every class left out of its sum (the count stays);
      'pad_row'    every class that is padded to its 32-query chunk counts the neighbouring query in one of its zero rows:
                   the next class's first one, for the last class the previous class's last one."""
    X = d.X.float()
    hi = d.q.half().float()
    lo = (d.q - hi).half().float()
    s = hi @ X if mutant == 'no_lo' else hi @ X + lo @ X
    if d.vnorm is not None:
        s = s / d.vnorm
    a = torch.where(s >= 0.25, s * s * s.clamp_min(0).sqrt(), torch.zeros_like(s))
    st = starts_of(d.counts)
    out = torch.empty(len(d.counts), X.shape[1])
    for c, n in enumerate(d.counts):
        rows = a[st[c]:st[c + 1] - (1 if mutant == 'drop_last' else 0)]
        total = rows.sum(0) if rows.shape[0] else torch.zeros(X.shape[1])
        if mutant == 'pad_row' and n % 32 and len(d.counts) > 1:
            total = total + a[st[c + 1] if c + 1 < len(d.counts) else st[c] - 1]
        out[c] = total / np.float32(n)
    return out
