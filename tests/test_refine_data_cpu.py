"""CPU: the host side of the refinement-loop tests (tests/refine_data.py) -- that every generated map, point and row set has
the property its name claims, that the float32 emulations of the stated arithmetic meet the derived bounds (and the operator
the reference runs, bit for bit, where there is one), and that subtly wrong variants leave them: the GPU tests of
tests/test_gpu_refine.py can fail, and when they do it is the kernel's doing."""
import numpy as np
import pytest
import torch

import refine_data as rd
import sim_data as sd


def _bits(t):
    return torch.as_tensor(t).contiguous().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. top-K
def _select_by_keys(keys, k):
    kth = np.sort(keys)[len(keys) - k]
    return np.nonzero(keys >= kth)[0][:k]


def _old_keys(values):
    b = _bits(values)
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


@pytest.mark.parametrize('nvox', rd.TOPK_NVOX)
def test_topk_maps_have_their_properties(nvox):
    differs = 0
    for k in rd.topk_ks(nvox):
        maps = rd.topk_maps(nvox, k)
        ref = rd.topk_ref(torch.stack(list(maps.values())), k)
        assert ref.shape == (len(rd.TOPK_KINDS), k) and not any(bool(torch.isnan(m).any()) for m in maps.values())
        for row, (kind, s) in zip(ref, maps.items()):
            # the radix select on the kernel's keys is the expression, on every map
            assert np.array_equal(_select_by_keys(rd.order_keys(s.numpy()), k), row.numpy()), (kind, k)
            kth = torch.topk(s, k).values[-1]
            if kind == 'normal' and nvox >= 3:
                assert bool(torch.isposinf(s).any()) and bool(torch.isneginf(s).any()) and bool((s > 0).any()) and bool((s < 0).any())
            if kind == 'ties':
                tied = (s == kth).nonzero()[:, 0]
                assert len(s.unique()) <= 4
                if nvox > rd.WAVE:
                    assert bool((tied < rd.WAVE).any()) and bool((tied >= rd.WAVE).any())
                if nvox > rd.CHUNK:
                    assert bool((tied < rd.CHUNK).any()) and bool((tied >= rd.CHUNK).any())
                if nvox >= 1024 and k < nvox:
                    assert int((s >= kth).sum()) > k                    # the cut goes through the tie
            if kind.startswith('digit'):
                keys, mask = rd.order_keys(s.numpy()), rd.DIGIT_MASKS[int(kind[-1])]
                assert not ((keys ^ keys[0]) & np.uint32(~mask & 0xffffffff)).any()
                assert nvox < 63 or len(np.unique(keys)) >= 32
            if kind == 'thresholded':
                assert int((s > 0).sum()) == k // 2 < k and not (_bits(s)[(s == 0).numpy()]).any() and float(kth) == 0.0
                assert row.tolist() == list(range(k))
                assert k < 4 or k // 2 > nvox // 3 or int((s[:k] > 0).sum()) < k // 2   # not simply the positive voxels
            if kind == 'signed_zeros':
                assert torch.equal(s, maps['thresholded']) and row.tolist() == list(range(k))       # equal as floats
                neg = _bits(s) == 0x80000000
                assert nvox < 3 or (neg.any() and (_bits(s) == 0).any())
                assert nvox == 1 or k // 2 >= nvox - 1 or neg[0]
                differs += int(not np.array_equal(_select_by_keys(_old_keys(s), k), row.numpy()))
            if kind == 'kth_negative_zero':
                b = _bits(s)
                assert int((s > 0).sum()) + int((b == 0).sum()) < k <= int((s >= 0).sum()) and float(kth) == 0.0
                assert k == nvox or bool((s < 0).any())
    # a key that orders -0.0 below +0.0 selects other voxels on the signed-zero maps
    assert nvox < 3 or differs >= 1


def test_distance_map():
    s = rd.distance_map()
    assert s.shape == (1, 600) and float(s.min()) > 0 and float(s.max()) < 2
    assert rd.topk_ref(s, 35).shape == (1, 35)


# ---------------------------------------------------------------------------------------------- 2. sampling
@pytest.mark.parametrize('grid', rd.SAMPLE_GRIDS, ids=str)
def test_sample_points_have_their_properties(grid):
    p = rd.sample_points(grid)
    pos = np.stack([rd.sample_pos32(p.rel[:, ax], n) for ax, n in enumerate(grid)], 1).astype(np.float64)
    c, fc = pos[p.kinds['centres']], pos[p.kinds['faces']]
    assert len(c) >= 1 and np.array_equal(c, np.round(c)) and (c >= 0).all() and (c < np.array(grid)).all()
    half = fc - np.floor(fc) == 0.5
    assert len(fc) >= 6 and (half.sum(1) == 1).all() and np.array_equal(fc[~half], np.round(fc[~half]))
    assert fc.min() == -0.5 and (fc.max(0) == np.array(grid) - 0.5).all()                  # the outer faces too
    # every voxel is a centre or a near-centre; an axis of at most two voxels has all its centres exact
    assert len(c) + (p.kinds['near_centres'].stop - p.kinds['near_centres'].start) == int(np.prod(grid))
    assert max(grid) > 2 or len(c) == int(np.prod(grid))
    k = pos[p.kinds['corners']]
    assert set(np.unique(np.abs(p.rel[p.kinds['corners']]))) == {1.0} and ((k == -0.5) | (k == np.array(grid) - 0.5)).all()
    o = pos[p.kinds['outside']]
    assert (o >= -1.5 - 1e-5).all() and (o <= np.array(grid) + 0.5 + 1e-5).all() and ((o < -0.5) | (o > np.array(grid) - 0.5)).any(1).all()
    gone = pos[p.kinds['all_outside']]
    assert ((gone < -1) | (gone > np.array(grid))).any(1).all()
    i = pos[p.kinds['interior']]
    assert (i > -0.5).all() and (i < np.array(grid) - 0.5).all()
    if min(grid) > 1:
        assert (i >= 0).all() and (i <= np.array(grid) - 1).all()


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('grid', rd.SAMPLE_GRIDS, ids=str)
def test_sampling_emulation_is_the_operator(grid, half):
    """The float32 emulation of the kernel's stated order is F.grid_sample(align_corners=False) on the CPU bit for bit, in
    both modes -- also on the nearest ties and outside the volume --, lies within the derived bound of the fp64 value, and
    has the exact values the point kinds promise.  With voxel norms there is no operator to compare with: bound only."""
    p = rd.sample_points(grid)
    for f in (1, 33):
        feat, vnorm = rd.sample_volume(grid, f, half)
        flat = feat.float().reshape(f, -1).numpy()
        assert not flat[:, -1].any() and float(vnorm[-1]) == np.float32(1e-12) and (len(vnorm) == 1 or float(vnorm[:-1].min()) > 1e-3)
        for mode in ('nearest', 'bilinear'):
            emu = rd.sample_emulate(feat, p.rel, mode)
            assert emu.dtype == np.float32 and np.array_equal(emu.view(np.int32), rd.grid_sample_cpu(feat, p.rel, mode).view(np.int32)), mode
            for vn in (None, vnorm):
                got = rd.sample_emulate(feat, p.rel, mode, vn)
                ref, bound = rd.sample_ref(feat, p.rel, mode, vn)
                assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (mode, vn is not None)
                assert not got[p.kinds['all_outside']].any()
            # centres: the voxel itself in both modes
            z, y, x = [np.rint(rd.sample_pos32(p.rel[p.kinds['centres'], ax], n)).astype(int) for ax, n in enumerate(grid)]
            assert np.array_equal(emu[p.kinds['centres']], flat[:, (z * grid[1] + y) * grid[2] + x].T)
    # the tie goes to the even voxel: position 0.5 -> voxel 0, 1.5 -> voxel 2, -0.5 -> voxel 0 (inside), n - 0.5 -> n if that is even
    assert np.rint(np.float32(0.5)) == 0 and np.rint(np.float32(1.5)) == 2 and np.rint(np.float32(-0.5)) == 0


def test_fused_sampling_is_not_the_operator(monkeypatch):
    """What the kernel did before: one rounding for (r + 1) * n - 1, and val * w going into the sum unrounded.  Either moves
    some of the random points' values by a last bit -- the bit-equality the GPU test asks for can fail."""
    grid = (6, 5, 7)
    p = rd.sample_points(grid, n_random=200)
    feat, _ = rd.sample_volume(grid, 32, False)
    right = rd.sample_emulate(feat, p.rel, 'bilinear')

    def fused_pos(r, n):
        r = np.asarray(r, dtype=np.float32)
        return ((r + np.float32(1.0)).astype(np.float64) * n - 1.0).astype(np.float32) / np.float32(2.0)
    with monkeypatch.context() as m:
        m.setattr(rd, 'sample_pos32', fused_pos)
        moved = rd.sample_emulate(feat, p.rel, 'bilinear')
    assert 0 < int((moved != right).sum())
    vals, wgts, ins = rd._corner_terms(feat, p.rel, None, np.float32)
    res = np.zeros(vals.shape[1:], dtype=np.float32)
    for v, w, i in zip(vals, wgts, ins):
        res = np.where(i[:, None], (res.astype(np.float64) + v.astype(np.float64) * w[:, None]).astype(np.float32), res)
    assert 0 < int((res != right).sum())
    ref, bound = rd.sample_ref(feat, p.rel, 'bilinear')
    assert (np.abs(res - ref) <= bound).all()                     # ... while the fp64 bound alone would not have noticed


# ---------------------------------------------------------------------------------------------- 3. class maps, modes 1 and 2
def _ratio(got, d):
    err = (got.double() - d.ref).abs()
    return torch.where(d.bound > 0, err / d.bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0).double())


def test_mode_references_by_hand():
    """Two voxels, three queries: mode 1 takes the mean first (0.25 is kept), mode 2 clamps at 0 and 1."""
    X = torch.tensor([[1.0, 0.5], [0.0, 0.5]]).half()
    q = torch.tensor([[1.0, 0.0], [0.25, 0.0], [-0.5, 0.0]])
    ref, bound, edge = sd.class_maps_ref(X, q, (3,), mode=1)
    assert ref[0].tolist() == pytest.approx([0.25 ** 2.5, 0.0], rel=1e-15) and edge.tolist() == [[True, False]]
    assert float(bound[0, 0]) >= 0.25 ** 2.5 and float(bound[0, 1]) == 0.0
    ref, bound, edge = sd.class_maps_ref(X, q * 4, (2, 1), mode=2, expo=2.0)
    assert ref.tolist() == [[1.0, (1 + 0.25) / 2], [0.0, 0.0]] and not bool(edge.any())      # 4 -> 1, 2 -> 1, 0.5 ** 2, -2 -> 0
    ref, bound, _ = sd.class_maps_ref(X, q, (2, 1), mode=2, expo=1.5)
    assert ref[0].tolist() == pytest.approx([(1 + 0.25 ** 1.5) / 2, (0.5 ** 1.5 + 0.125 ** 1.5) / 2], rel=1e-15) and ref[1].tolist() == [0.0, 0.0]
    assert 0 < float(bound[0].max()) < 1e-5 and float(bound[1].max()) == 0.0
    ref_n, _, _ = sd.class_maps_ref(X, q, (2, 1), vnorm=torch.tensor([2.0, 1.0]), mode=2, expo=1.0)
    assert ref_n[0].tolist() == pytest.approx([(0.5 + 0.125) / 2, (0.5 + 0.125) / 2], rel=1e-15)
    # mode 0 is untouched by the new arguments
    a, b = sd.class_maps_ref(X, q, (2, 1)), sd.class_maps_ref(X, q, (2, 1), None, 0, 0.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('counts', rd.MODE1_COUNTS, ids=rd.counts_id)
@pytest.mark.parametrize('shape', rd.MODES_SHAPES, ids=rd.shape_id)
def test_mode1_emulation_and_mutants(shape, counts):
    """The float32 emulation stays within the bound; the activation before the mean, the mean over 16 and one dropped
    annotation leave it by a wide margin; check_edge_share's caps hold and both sides of the threshold occur."""
    grid, f = shape
    for normalized in (True, False):
        d = rd.modes_case(1, grid, counts, f, True, 0.0, normalized)
        sd.check_edge_share(d)
        assert float(d.ref.max()) > 0.01 and (f >= 384 or 0.5 < float((d.ref > 0).float().mean()) < 1.0)
        assert float(_ratio(rd.emulate_modes(d, 1), d).max()) <= 1.0
        # (one of 1030 dots moves the mean by a thousandth: outside the bound on nearly every voxel, but not a hundred times)
        for mutant, least in (('act_first', 10.0), ('mean_16', 10.0), ('drop_last', 10.0 if sum(counts) < 100 else 1.0)):
            wrong = _ratio(rd.emulate_modes(d, 1, mutant=mutant), d)
            share = float((wrong > least).float().mean())
            print(f'mode 1, {rd.shape_id(shape)}, counts {counts}, {mutant}: {100 * share:.1f} % of the voxels beyond {least:g} x bound')
            assert share >= 0.5, (mutant, share)


@pytest.mark.parametrize('counts', rd.MODE2_GROUPS, ids=rd.counts_id)
@pytest.mark.parametrize('shape', rd.MODES_SHAPES, ids=rd.shape_id)
def test_mode2_emulation_and_mutants(shape, counts):
    grid, f = shape
    for half in (True, False):
        for expo in rd.MODE2_EXPO:
            d = rd.modes_case(2, grid, counts, f, half, expo, True)
            s = d.q.double() @ d.X.double()
            assert float((s < 0).float().mean()) > 0.005 and float((s > 1).float().mean()) > 0.02      # both clamps at work
            got = rd.emulate_modes(d, 2, expo)
            assert float(_ratio(got, d).max()) <= 1.0
            mask, value = rd.mode2_exact_points(d)
            assert torch.equal(got[mask], value[mask])
            mutants = ['no_clamp', 'mean_16', 'drop_last'] + (['expo_2.5'] if expo == 2.0 else [])
            for mutant in mutants:
                if mutant == 'mean_16' and set(counts) == {16}:
                    continue
                wrong = _ratio(rd.emulate_modes(d, 2, expo, mutant=mutant), d)
                share = float((wrong > 100.0).float().mean())
                assert share >= (0.02 if mutant == 'no_clamp' else 0.5), (mutant, expo, share)    # (no_clamp: where a dot is above 1)
    cos = rd.modes_case(2, grid, counts, f, True, 1.5, False)
    assert cos.vnorm is not None and float(_ratio(rd.emulate_modes(cos, 2, 1.5), cos).max()) <= 1.0


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_unit_queries_are_exact(half):
    """The K_LOG measurement's premise: every dot product is a volume entry, exactly, whatever the order of summation; an exact
    kernel scores 0, one whose log2 is off by 3 * 2^-24 max(|log2 c|, 1) scores 3."""
    d = rd.unit_queries(rd.GRID_SPLIT, half)
    assert torch.equal(d.q.sum(0), torch.ones(48)) and torch.equal(d.q.sum(1), torch.ones(48)) and set(d.q.unique().tolist()) == {0.0, 1.0}
    assert torch.equal((d.q.double() @ d.X.double()), d.X.double())
    c = d.X.double().clamp(0, 1)
    live = (c > 0) & (c < 1)
    assert int(live.sum()) > 25000 and float(c[live].log2().abs().max()) > 15 and float((d.X.double() < 0).float().mean()) > 0.05
    assert rd.k_log_observed(c, d)[0] == 0.0
    off = torch.exp2(c.clamp_min(1e-300).log2() + 3 * sd.U * c.clamp_min(1e-300).log2().abs().clamp_min(1.0)) * (1 + 2 * sd.U)
    assert rd.k_log_observed(torch.where(live, off, c), d)[0] == pytest.approx(3.0, rel=1e-3)
    ref, bound, _ = sd.class_maps_ref(d.X, d.q, d.counts, mode=2, expo=1.0)
    assert torch.equal(ref, c) and float(_ratio(rd.emulate_modes(d, 2, 1.0), rd.SimpleNamespace(ref=ref, bound=bound)).max()) <= 1.0
    assert 0 < sd.K_LOG <= 8


@pytest.mark.parametrize('counts', rd.LATTICE1_COUNTS, ids=rd.counts_id)
def test_lattice_mode1(counts):
    """Mode 1 on the lattice: the emulation is the activation of the correctly rounded quotient (first candidate); the sum
    of dots differs from mode 0's sum of activations, so the two modes cannot be confused."""
    d = sd.lattice(rd.GRID_SPLIT, counts, 48, 5)
    cand, S = rd.lattice1_candidates(d)
    got = rd.emulate_modes(d, 1)
    assert torch.equal(got, cand[0]) and float(cand[0].max()) > 0 and not torch.equal(S, d.sums)
    assert not torch.equal(rd.emulate_modes(d, 1, mutant='drop_last'), got)
    assert not torch.equal(rd.emulate_modes(d, 1, mutant='act_first'), got)


@pytest.mark.parametrize('counts', rd.MODE2_GROUPS, ids=rd.counts_id)
def test_lattice_mode2(counts):
    d = rd.lattice2(rd.GRID_SPLIT, counts, 48, 5)
    assert set(d.q[d.q != 0].tolist()) <= set(rd.LATTICE2_W) and int((d.q != 0).sum()) == sum(counts)
    n = torch.tensor(counts, dtype=torch.float64)[:, None]
    want = d.sums / n
    for expo in rd.MODE2_EXPO:
        ref, bound, _ = sd.class_maps_ref(d.X, d.q, counts, mode=2, expo=expo)
        assert torch.equal(ref, want)
        got = rd.emulate_modes(d, 2, expo)
        ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
        assert bool(((got.double() - want).abs() <= ulp).all())
        pow2 = torch.tensor([c & (c - 1) == 0 for c in counts])
        assert torch.equal(got[pow2].double(), want[pow2])
        assert not torch.equal(rd.emulate_modes(d, 2, expo, mutant='no_clamp'), got)
        assert not torch.equal(rd.emulate_modes(d, 2, expo, mutant='drop_last'), got)
    mask, value = rd.mode2_exact_points(d)
    assert torch.equal(value[mask].double(), want.float().double()[mask])


# ---------------------------------------------------------------------------------------------- 4. mean pairwise distance
def _pair_ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0).double())


@pytest.mark.parametrize('measure', ['cosine', 'euclidean'])
@pytest.mark.parametrize('n', rd.PAIR_N)
def test_pairwise_emulation_and_kinds(n, measure):
    kinds = set()
    for f in rd.PAIR_F:
        kind = rd.pair_kind(n, f)
        kinds.add(kind)
        x = rd.pair_rows(n, f, kind)
        assert x.shape == (n, f) and x.dtype == torch.float32
        if kind == 'zero_row':
            assert not x[n // 2].any()
        if kind == 'twins' and n >= 2:
            assert torch.equal(x[n - 1], x[n // 3]) and n - 1 != n // 3
        if kind.startswith('scaled'):
            assert float(x.abs().mean()) == pytest.approx(0.84 * float(kind.split('_')[1]), rel=0.6)
        if n * n * f > 600 * 600 * 1000:
            continue                                          # (the reference of the largest shape is the GPU test's to compute)
        ref, bound = rd.pair_ref(x, measure)
        got = rd.pair_emulate(x, measure)
        r = _pair_ratio(got, ref, bound)
        assert float(r.max()) <= 1.0, (f, kind, float(r.max()))
        if kind == 'twins' and n == 2 and measure == 'euclidean':
            assert ref.tolist() == [0.0, 0.0]
        if n > 256:
            wrong = rd.pair_emulate(x, measure, 'stride_once')
            assert float(_pair_ratio(wrong, ref, bound).median()) > 5.0
    assert kinds == set(rd.PAIR_KINDS)


@pytest.mark.parametrize('measure', ['cosine', 'euclidean'])
def test_dissimilar_rows_have_a_gap(measure):
    x = rd.dissimilar_rows(measure)
    chosen, gap, bounds = rd.dissimilar_gap(x, measure)
    print(f'{measure}: gap between the 35th and 36th distance {gap:.3e}, their bounds {bounds:.3e}')
    assert x.shape == (600, 24) and len(chosen) == 35 and gap > 2 * bounds


# ---------------------------------------------------------------------------------------------- 5. resample_topk
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
def test_resample_data(half):
    feat, sims = rd.resample_data(half)
    assert feat.shape == (48, 8, 8, 12) and sims.shape == (2, 3, 8, 8, 12) and feat.dtype == (torch.float16 if half else torch.float32)
    tied = 0
    for K, mode in ((3, 'nearest'), (8, 'bilinear')):
        idx, q, ref, bound = rd.resample_ref(feat, sims, K, 2.0, mode)
        assert idx.shape == (6, K) and q.shape == (6 * K, 48) and ref.shape == bound.shape == (6, 768)
        flat = sims.reshape(6, -1)
        for g in range(6):
            kth = torch.topk(flat[g], K).values[-1]
            tied += int((flat[g] >= kth).sum()) > K
        assert float(ref.max()) > 0.3 and float(bound.max()) < 1e-4
    assert tied >= 3
