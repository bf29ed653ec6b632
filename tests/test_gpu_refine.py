"""GPU: the kernels of the interactive refinement loop at their edges -- vittf_topk_voxels (exact, against the expression
it replaces), vittf_sample_features (bit-equal to the stated fp32 order, within a derived bound of fp64),
vittf_similarity_maps_f32 in modes 1 and 2 (per entry against fp64, both VALU kernel forms, fp16 and fp32 volumes),
vittf_mean_pairwise_distance (per row against fp64), and resample_topk / take_most_dissimilar / sample_features3d on top.
Data, references and bounds are tests/refine_data.py's and tests/sim_data.py's;
tests/test_refine_data_cpu.py shows that the data has the properties named here and that subtly wrong kernels would fail."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import refine_data as rd
import sim_data as sd

pytestmark = pytest.mark.gpu

GUARD, GUARD_INT, GUARDS = 7.0, -77, 4
INVALID_ARG = -1                     # VITTF_ERR_INVALID_ARG


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- 1. top-K
def _topk(lib, gpu, maps, k):
    """vittf_topk_voxels on maps [m][nvox] (host): int64 [m][k]; GUARDS ints behind idx_out must stay untouched."""
    m, nvox = maps.shape
    idx = torch.full((m * k + GUARDS,), GUARD_INT, dtype=torch.int32, device=gpu)
    md = maps.contiguous().to(gpu)
    _lib.check(lib.vittf_topk_voxels(_lib.ptr(md), m, nvox, k, _lib.ptr(idx), _lib.stream_ptr()), 'vittf_topk_voxels')
    host = idx.cpu()
    assert host[m * k:].tolist() == [GUARD_INT] * GUARDS, 'wrote past idx_out'
    return host[:m * k].view(m, k).long()


@pytest.mark.parametrize('nvox', rd.TOPK_NVOX)
def test_topk_is_the_expression(gpu, nvox):
    """Every k of rd.TOPK_K on every kind of map (mixed signs with infinities, a tied k-th value across the wave and chunk
    boundaries, one radix digit at a time, a thresholded map, signed zeros): integer equality with
    topk(s, k).values[-1]; (s >= kth).nonzero()[:k], eight maps in one call and one in a second."""
    lib = _lib.load()
    for k in rd.topk_ks(nvox):
        maps = rd.topk_stack(nvox, k)
        want = rd.topk_ref(maps, k)
        got = torch.cat([_topk(lib, gpu, maps[:8], k), _topk(lib, gpu, maps[8:], k)])
        for i, kind in enumerate(rd.TOPK_KINDS):
            bad = (got[i] != want[i]).nonzero()
            assert len(bad) == 0, (f'{kind}, nvox {nvox}, k {k}: {len(bad)} of {k} indices differ, first at position {int(bad[0])}: '
                                   f'got {int(got[i][bad[0]])}, expression {int(want[i][bad[0]])}')
    print(f'top-K nvox {nvox}: k {rd.topk_ks(nvox)} x {len(rd.TOPK_KINDS)} kinds exact')


def test_topk_of_a_distance_map(gpu):
    """take_most_dissimilar's use: one map of 600 mean distances, k = 35."""
    s = rd.distance_map()
    assert torch.equal(_topk(_lib.load(), gpu, s, 35), rd.topk_ref(s, 35))


def test_topk_refusals(gpu):
    lib = _lib.load()
    maps = torch.zeros(2, 10, device=gpu)
    idx = torch.full((32,), GUARD_INT, dtype=torch.int32, device=gpu)
    for nmaps, nvox, k in ((2, 10, 11), (2, 10, 0), (2, 10, -1), (0, 10, 3), (-1, 10, 3)):
        assert lib.vittf_topk_voxels(_lib.ptr(maps), nmaps, nvox, k, _lib.ptr(idx), _lib.stream_ptr()) == INVALID_ARG, (nmaps, nvox, k)
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [GUARD_INT] * 32


# ---------------------------------------------------------------------------------------------- 2. sampling
def _sample(lib, gpu, feat, rel, mode, vnorm):
    f, (n0, n1, n2) = feat.shape[0], feat.shape[1:]
    a = rel.shape[0]
    out = torch.full((a * f + 1,), GUARD, device=gpu)
    fd, rd_, vd = feat.to(gpu), torch.from_numpy(rel).to(gpu), None if vnorm is None else vnorm.to(gpu)
    _lib.check(lib.vittf_sample_features(_lib.ptr(fd), int(feat.dtype == torch.float16), f, n0, n1, n2, _lib.ptr(rd_), a,
                                         _lib.SAMPLE_MODES[mode], _lib.ptr(vd), _lib.ptr(out), _lib.stream_ptr()), 'vittf_sample_features')
    host = out.cpu()
    assert float(host[-1]) == GUARD, 'wrote past the output'
    return host[:-1].view(a, f).numpy()


@pytest.mark.parametrize('f', rd.SAMPLE_F)
@pytest.mark.parametrize('grid', rd.SAMPLE_GRIDS, ids=str)
def test_sample_features(gpu, grid, f):
    """fp32 and fp16 storage, with and without voxel norms, both modes, at every voxel centre and cell-face midpoint that fp32
    coordinates reach, up to 1.5 voxels outside, on -1 and +1 and inside: every entry within the derived bound of fp64;
    nearest bit-equal to the gather (ties to the even voxel); trilinear bit-equal to the float32 emulation of the stated
    order, which is F.grid_sample on the CPU bit for bit (tests/test_refine_data_cpu.py)."""
    lib = _lib.load()
    p = rd.sample_points(grid)
    worst = 0.0
    for half in (False, True):
        feat, vnorm = rd.sample_volume(grid, f, half)
        for vn in (None, vnorm):
            for mode in ('nearest', 'bilinear'):
                what = f'{grid} f {f} {"fp16" if half else "fp32"} {"norm" if vn is not None else "raw"} {mode}'
                got = _sample(lib, gpu, feat, p.rel, mode, vn)
                ref, bound = rd.sample_ref(feat, p.rel, mode, vn)
                err = np.abs(got.astype(np.float64) - ref)
                assert (err <= bound).all(), (what, int((err > bound).sum()), float(err.max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0)))
                emu = rd.sample_emulate(feat, p.rel, mode, vn)
                diff = got.view(np.int32) != emu.view(np.int32)
                a, ff = (int(x[0]) for x in np.nonzero(diff)) if diff.any() else (0, 0)
                assert not diff.any(), (f'{what}: {int(diff.sum())} of {diff.size} entries differ from the float32 emulation, first at point {a} '
                                        f'(rel {p.rel[a].tolist()}), feature {ff}: got {got[a, ff]!r}, emulation {emu[a, ff]!r}')
                c = p.kinds['centres']
                near = rd.sample_emulate(feat, p.rel[c], 'nearest', vn)
                assert np.array_equal(got[c].view(np.int32), near.view(np.int32)), what      # weights exactly 0 / 1: the voxel itself
                assert not got[p.kinds['all_outside']].any(), what
    print(f'sampling {grid} f {f}: worst error / bound {worst:.4f}; trilinear and nearest bit-equal to the float32 emulation')


def test_sample_features3d_python(gpu):
    """The Python function on top: same bits, ([M,] C, A, F) shape, rel_coords left alone."""
    grid, f = (6, 5, 7), 32
    p = rd.sample_points(grid)
    feat, _ = rd.sample_volume(grid, f, True)
    rel = torch.from_numpy(p.rel.copy()).reshape(1, -1, 3)
    for mode in ('nearest', 'bilinear'):
        got = vt.sample_features3d(feat.to(gpu), rel, mode)
        assert got.shape == (1, 1, rel.shape[1], f) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().reshape(-1, f).numpy().view(np.int32), rd.sample_emulate(feat, p.rel, mode).view(np.int32))
    assert np.array_equal(rel.reshape(-1, 3).numpy(), p.rel)


# ---------------------------------------------------------------------------------------------- 3. class maps, modes 1 and 2
def _maps(lib, gpu, d, mode, expo, split, monkeypatch):
    """One vittf_similarity_maps_f32 call: maps [classes][nvox] on the host.  Asserts the kernel form by name, the guard float
    behind the maps, and that the per-class maxima at the head of the workspace (0xff before the call) are maps.amax(1)."""
    for k in sd.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('VITTF_SIM_SPLIT', str(split))
    classes, a = len(d.counts), int(sum(d.counts))
    n0, n1, n2 = d.grid
    nvox = n0 * n1 * n2
    feat, qf = d.X.to(gpu), d.q.to(gpu)
    vnorm = None if d.vnorm is None else d.vnorm.to(gpu)
    starts = sd.starts_of(d.counts)
    ws_bytes = lib.vittf_similarity_workspace_bytes(classes, 0, a)
    ws = torch.full((ws_bytes,), 0xff, dtype=torch.uint8, device=gpu)
    out = torch.full((classes * nvox + 1,), GUARD, device=gpu)
    _lib.check(lib.vittf_similarity_maps_f32(_lib.ptr(feat), int(d.X.dtype == torch.float16), d.f, n0, n1, n2, _lib.ptr(qf),
                                             starts.ctypes.data_as(C.POINTER(C.c_int32)), classes, mode, float(expo), _lib.ptr(vnorm),
                                             _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'vittf_similarity_maps_f32')
    torch.cuda.synchronize()
    host = out.cpu()
    maps = host[:-1].view(classes, nvox)
    name = _lib.kernel_name('similarity')
    assert name == rd.form_of(d.grid, d.f, split), f'routing: {name} ran with VITTF_SIM_SPLIT={split} on {d.grid}, f {d.f}'
    assert float(host[-1]) == GUARD, 'wrote past the last map'
    assert bool(torch.isfinite(maps).all())
    maxima = ws[:4 * classes].cpu().view(torch.float32)
    assert torch.equal(_bits(maxima), _bits(maps.amax(dim=1))), (maxima.tolist(), maps.amax(dim=1).tolist())
    return maps


def _within(maps, d, what):
    ratio, c, v = sd.worst(maps, d.ref, d.bound)
    assert ratio <= 1.0, (f'{what}: class {c} ({d.counts[c]} annotations), voxel {v}: got {float(maps[c, v])!r}, fp64 {float(d.ref[c, v])!r}, '
                          f'bound {float(d.bound[c, v]):.3e}, error / bound {ratio:.2f}; '
                          f'{int(((maps.double() - d.ref).abs() > d.bound).sum())} of {maps.numel()} entries outside')
    return ratio


@pytest.mark.parametrize('counts', rd.MODE2_GROUPS, ids=rd.counts_id)
@pytest.mark.parametrize('shape', rd.MODES_SHAPES, ids=rd.shape_id)
def test_mode2_within_fp64_bound(gpu, monkeypatch, shape, counts):
    """clamp(s, 0, 1) ** expo, group mean: fp16 and fp32 volumes, expo 1, 1.5 and 2, both settings of VITTF_SIM_SPLIT (the
    split form where the shape has one), dots below 0 and above 1; groups that fill a chunk with more than MAXC classes
    ((2,) * 12) and that span three chunks ((35, 35)).  Every entry within the bound; where all queries of a group sit on
    exact points (0 or 1) the map is fl(ones / n) bit for bit.  The cosine path once per case (expo 1.5, fp16)."""
    lib = _lib.load()
    grid, f = shape
    worst = 0.0
    for split in (1, 0):
        for half in (True, False):
            for expo in rd.MODE2_EXPO:
                d = rd.modes_case(2, grid, counts, f, half, expo, True)
                maps = _maps(lib, gpu, d, 2, expo, split, monkeypatch)
                worst = max(worst, _within(maps, d, f'mode 2 {rd.shape_id(shape)} {"fp16" if half else "fp32"} expo {expo} split {split}'))
                mask, value = rd.mode2_exact_points(d)
                assert torch.equal(_bits(maps[mask]), _bits(value[mask])), (half, expo, split)
                assert float(maps.max()) > 0.1
        d = rd.modes_case(2, grid, counts, f, True, 1.5, False)
        worst = max(worst, _within(_maps(lib, gpu, d, 2, 1.5, split, monkeypatch), d, f'mode 2 {rd.shape_id(shape)} cosine split {split}'))
    print(f'mode 2 {rd.shape_id(shape)} groups {rd.counts_id(counts)}: worst error / bound {worst:.4f}')


@pytest.mark.parametrize('counts', rd.MODE1_COUNTS, ids=rd.counts_id)
@pytest.mark.parametrize('shape', rd.MODES_SHAPES, ids=rd.shape_id)
def test_mode1_within_fp64_bound(gpu, monkeypatch, shape, counts):
    """The mean of the dots first, then where(t >= 0.25, t, 0) ** 2.5: one class of 17 annotations (two passes) and one of
    1030 (65 passes), with and without voxel norms, both settings of VITTF_SIM_SPLIT.  An fp32 volume is refused."""
    lib = _lib.load()
    grid, f = shape
    worst = 0.0
    for normalized in (True, False):
        d = rd.modes_case(1, grid, counts, f, True, 0.0, normalized)
        sd.check_edge_share(d)
        for split in (1, 0):
            maps = _maps(lib, gpu, d, 1, 0.0, split, monkeypatch)
            assert float(maps.max()) > 0.01
            worst = max(worst, _within(maps, d, f'mode 1 {rd.shape_id(shape)} {"unit" if normalized else "cosine"} split {split}'))
    print(f'mode 1 {rd.shape_id(shape)} counts {counts}: worst error / bound {worst:.4f}')
    wide = rd.modes_case(1, grid, counts, f, True, 0.0, True)
    wide = rd.SimpleNamespace(X=wide.X.float(), q=wide.q, counts=wide.counts, vnorm=None, grid=wide.grid, f=wide.f)
    with pytest.raises(_lib.VittfError):
        _maps(lib, gpu, wide, 1, 0.0, 1, monkeypatch)


def test_v_log_f32_measurement(gpu, monkeypatch):
    """The measurement behind sim_data.K_LOG: mode 2 with expo = 1 on one-hot queries, where clamp(s) ** 1 is a volume entry
    exactly and the whole deviation is v_log_f32's and v_exp_f32's.  Prints the worst observed figure; K_LOG is twice the
    figure first measured, so the observed one is at most K_LOG / 2 -- and the bound holds."""
    lib = _lib.load()
    for half in (False, True):
        d = rd.unit_queries(rd.GRID_SPLIT, half)
        d.ref, d.bound, d.edge = sd.class_maps_ref(d.X, d.q, d.counts, mode=2, expo=1.0)
        for split in (1, 0):
            maps = _maps(lib, gpu, d, 2, 1.0, split, monkeypatch)
            k, c = rd.k_log_observed(maps, d)
            dev = ((maps.double() - d.ref).abs() / d.ref.clamp_min(1e-300))[(d.ref > 2.0 ** -120) & (d.ref < 1)]
            print(f'v_log_f32 + v_exp_f32, {"fp16" if half else "fp32"} volume, split {split}: K_LOG observed {k:.4f} (at c = {c!r}); '
                  f'worst relative deviation of exp2(log2 c) from c {float(dev.max()) / sd.U:.3f} * 2^-24 over {dev.numel()} arguments')
            assert k <= sd.K_LOG / 2 + 1e-9, (k, sd.K_LOG)
            _within(maps, d, 'unit queries')
            exact = (d.ref == 0) | (d.ref == 1)
            assert torch.equal(maps[exact].double(), d.ref[exact])


@pytest.mark.parametrize('counts', rd.LATTICE1_COUNTS, ids=rd.counts_id)
def test_lattice_mode1_exact(gpu, monkeypatch, counts):
    """0 / 1 features and one-hot queries: the sum of the dots is exact in fp32 in any order, so the map is the activation
    (three correctly rounded operations) of the sum divided by n -- of the correctly rounded quotient or, no more being
    assumed of the division than one ulp, of a neighbour; of the quotient itself where n is a power of two."""
    lib = _lib.load()
    for grid, f in ((rd.GRID_SPLIT, 48), (sd.ODD, 384)):
        d = sd.lattice(grid, counts, f, 5)
        cand, _ = rd.lattice1_candidates(d)
        for split in (1, 0):
            maps = _maps(lib, gpu, d, 1, 0.0, split, monkeypatch)
            hit = (_bits(maps)[None] == _bits(cand)).any(0)
            assert bool(hit.all()), (grid, split, int((~hit).sum()), maps[~hit][:4].tolist(), cand[0][~hit][:4].tolist())
            pow2 = torch.tensor([k & (k - 1) == 0 for k in counts])
            assert torch.equal(_bits(maps[pow2]), _bits(cand[0][pow2]))
            assert float(maps.max()) > 0


@pytest.mark.parametrize('counts', rd.MODE2_GROUPS, ids=rd.counts_id)
def test_lattice_mode2_exact(gpu, monkeypatch, counts):
    """One-hot queries of weight 1, 1.5, -0.5, -1, 4 on 0 / 1 features: every activation is exactly 0 or 1 for every
    exponent (log2 1 = 0), so the map is the exact count divided by n: within one ulp, bit-equal for a power of two."""
    lib = _lib.load()
    n = torch.tensor(counts, dtype=torch.float64)[:, None]
    pow2 = torch.tensor([k & (k - 1) == 0 for k in counts])
    for grid, f in ((rd.GRID_SPLIT, 48), (sd.ODD, 384)):
        d = rd.lattice2(grid, counts, f, 5)
        want = d.sums / n
        ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
        for half in (True, False):
            d.X = d.X.half() if half else d.X.float()
            for expo in rd.MODE2_EXPO:
                for split in (1, 0):
                    maps = _maps(lib, gpu, d, 2, expo, split, monkeypatch)
                    off = (maps.double() - want).abs()
                    assert bool((off <= ulp).all()), (grid, half, expo, split, int((off > ulp).sum()))
                    assert torch.equal(maps[pow2].double(), want[pow2])
        assert float(d.sums.max()) >= 1.0


# ---------------------------------------------------------------------------------------------- 4. mean pairwise distance
def _pairwise(lib, gpu, x, measure):
    n, f = x.shape
    dist = torch.full((n + 1,), GUARD, device=gpu)
    xd = x.to(gpu)
    _lib.check(lib.vittf_mean_pairwise_distance(_lib.ptr(xd), n, f, 0 if measure == 'cosine' else 1, _lib.ptr(dist), _lib.stream_ptr()),
               'vittf_mean_pairwise_distance')
    host = dist.cpu()
    assert float(host[-1]) == GUARD, 'wrote past dist'
    return host[:-1]


@pytest.mark.parametrize('f', rd.PAIR_F)
@pytest.mark.parametrize('n', rd.PAIR_N)
def test_mean_pairwise_distance(gpu, n, f):
    """Both measures per row against fp64, within the bound derived from the FMA chains, the sqrt, the division and the
    fp64 mean: n below, at and beyond the 256 threads that stride over the rows; f from 1 to the 8192 the LDS row holds; random
    rows, rows scaled by 1e3 and 1e-3, a zero row (the 1e-8 clamp) and identical rows (a euclidean term of exactly 0), one
    kind per shape so that every kind meets every n and every f."""
    lib = _lib.load()
    kind = rd.pair_kind(n, f)
    x = rd.pair_rows(n, f, kind)
    for measure in ('cosine', 'euclidean'):
        ref, bound = rd.pair_ref(x, measure)
        got = _pairwise(lib, gpu, x, measure)
        err = (got.double() - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0).double())
        i = int(ratio.argmax())
        print(f'pairwise {measure} n {n} f {f} {kind}: worst error / bound {float(ratio[i]):.4f} (row {i})')
        assert float(ratio[i]) <= 1.0, (measure, kind, i, float(got[i]), float(ref[i]), float(bound[i]))
    if kind == 'twins' and n == 2:
        assert _pairwise(lib, gpu, x, 'euclidean').tolist() == [0.0, 0.0]


def test_mean_pairwise_distance_refusals(gpu):
    lib = _lib.load()
    x = torch.zeros(4, 8193, device=gpu)
    dist = torch.full((4,), GUARD, device=gpu)
    assert lib.vittf_mean_pairwise_distance(_lib.ptr(x), 4, 8193, 0, _lib.ptr(dist), _lib.stream_ptr()) == INVALID_ARG
    assert lib.vittf_mean_pairwise_distance(_lib.ptr(x), 4, 8192, 2, _lib.ptr(dist), _lib.stream_ptr()) == INVALID_ARG
    assert lib.vittf_mean_pairwise_distance(_lib.ptr(x), 0, 8192, 0, _lib.ptr(dist), _lib.stream_ptr()) == INVALID_ARG
    torch.cuda.synchronize()
    assert dist.cpu().tolist() == [GUARD] * 4


@pytest.mark.parametrize('measure', ['cosine', 'euclidean'])
def test_take_most_dissimilar_end_to_end(gpu, measure):
    """600 rows, 35 prototypes: the fp64 gap between the 35th and the 36th distance exceeds the sum of their bounds (asserted
    here on the CPU, nothing skipped), so the selected set must be the fp64 set."""
    x = rd.dissimilar_rows(measure)
    chosen, gap, bounds = rd.dissimilar_gap(x, measure)
    assert gap > bounds
    got = vt.similarity.take_most_dissimilar(x, rd.DISSIMILAR.k, measure)
    assert got.shape == (rd.DISSIMILAR.k, rd.DISSIMILAR.f)
    rows = {tuple(r.tolist()): i for i, r in enumerate(x)}
    assert len(rows) == rd.DISSIMILAR.n
    assert {rows[tuple(r.tolist())] for r in got} == chosen


# ---------------------------------------------------------------------------------------------- 5. resample_topk
@pytest.mark.parametrize('mode', ['nearest', 'bilinear'])
@pytest.mark.parametrize('K', [3, 8])
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_resample_topk_beyond_one_workgroup(gpu, half, K, mode):
    """2 classes x 3 annotations on 8 x 8 x 12 voxels, f = 48: the indices vittf_topk_voxels picks on the (tied) maps are the
    expression's, and every entry of resample_topk's result is within the mode-2 bound of the fp64 map of the queries sampled
    at those voxels (the float32 emulation of section 2, which the kernel equals bit for bit).  An fp16 volume returns fp16:
    one more rounding, 2^-11 relative (2^-25 absolute below the normal range)."""
    feat, sims = rd.resample_data(half)
    idx, q, ref, bound = rd.resample_ref(feat, sims, K, 2.0, mode)
    got_idx = _topk(_lib.load(), gpu, sims.reshape(6, -1), K)
    assert torch.equal(got_idx, idx)
    got = vt.similarity.resample_topk(feat, sims, K, 2.0, mode)
    assert got.shape == (1, 2, 3, 8, 8, 12) and got.dtype == (torch.float16 if half else torch.float32) and got.is_cuda
    maps = got.cpu().reshape(6, -1)
    if half:
        bound = bound + 2.0 ** -11 * (ref.abs() + bound) + 2.0 ** -25
    ratio, c, v = sd.worst(maps, ref, bound)
    print(f'resample_topk {"fp16" if half else "fp32"} K {K} {mode}: worst error / bound {ratio:.4f}')
    assert ratio <= 1.0, (c, v, float(maps[c, v]), float(ref[c, v]), float(bound[c, v]))
    assert float(maps.max()) > 0.3
