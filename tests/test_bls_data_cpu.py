"""CPU: the host side of the bilateral-solver tests (tests/bls_data.py) -- every case is what it is meant to be (exact
uint8 stage, the intended crop box, no zero-confidence vertex, a CG that cannot stop on another iteration on the device), the
criterion of the GPU tests is far above the noise of reordered fp64 sums and far below what five subtly wrong solvers do, and
the trilinear reference agrees with F.interpolate.  Prints, per case, the box, the vertex count, the perturbation result and
the mutant factors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bilateral as obil
import bls_data as bd

LIVE = [c.name for c in bd.LIVE]
ZERO = [c.name for c in bd.CASES if c.zero]


# ---------------------------------------------------------------------------------------------- the cases are sound
@pytest.mark.parametrize('name', [c.name for c in bd.CASES])
def test_case_inputs(name):
    """Integer-valued volume with minimum 0 and maximum 255 whose uint8 image is the volume itself (so the identity resize and
    to_u8_kernel leave nothing to rounding), and the crop box the case is meant to have."""
    c = bd.BY_NAME[name]
    volume, sim = bd.data(name)
    ref, trace = bd.reference(name)
    assert volume.shape == sim.shape == ref.shape == c.shape and volume.dtype == sim.dtype == ref.dtype == torch.float32
    assert float(volume.min()) == 0.0 and float(volume.max()) == 255.0 and torch.equal(volume, volume.round())
    assert trace['ref_u8'].dtype == torch.uint8 and torch.equal(trace['ref_u8'].float(), volume)
    resized = F.interpolate(sim[None, None], c.shape, mode='trilinear')[0, 0]
    assert torch.equal(resized.view(torch.int32), sim.view(torch.int32))                 # the resize is the identity, bit for bit
    lo, hi = obil.crop_bounds(sim, 0.1, 2)
    assert tuple(zip(lo.tolist(), hi.tolist())) == c.box == tuple((s.start, s.stop) for s in trace['box'])
    outside = torch.ones(c.shape, dtype=torch.bool)
    outside[bd.box_slices(c.box)] = False
    assert bool((sim[outside] == 0).all()) and torch.equal(ref[outside], sim[outside])
    grid = trace['grid']
    assert grid.npixels == bd.box_volume(c.box)
    print(f'{name}: box {c.box} = {grid.npixels} voxels, {grid.nvertices} vertices, key space (luma, z, y, x) {grid.dims}')


@pytest.mark.parametrize('name', [c.name for c in bd.CASES])
def test_confidence_is_ieee(name):
    """The reference's Sobel confidence is what single IEEE operations give (numpy float32, sqrt included), bit for bit, and
    the oracle's own (torch.sqrt) is within one spacing of the magnitude of it."""
    c = bd.BY_NAME[name]
    u8 = bd.reference(name)[1]['ref_u8'][bd.box_slices(c.box)]
    p = np.pad(u8.numpy().astype(np.float32) / np.float32(255), 1)
    h = np.float32(0.5)
    dx = h * p[1:-1, 1:-1, 2:] - h * p[1:-1, 1:-1, :-2]
    dy = h * p[1:-1, 2:, 1:-1] - h * p[1:-1, :-2, 1:-1]
    dz = h * p[2:, 1:-1, 1:-1] - h * p[:-2, 1:-1, 1:-1]
    s = (dx * dx + dy * dy) + dz * dz
    assert s.dtype == np.float32
    g = np.sqrt(s.astype(np.float64)).astype(np.float32)
    assert np.array_equal(bd.exact_sqrt(torch.from_numpy(s)).numpy(), g)
    below, above = np.nextafter(g, np.float32(0)).astype(np.float64), np.nextafter(g, np.float32(np.inf)).astype(np.float64)
    s64, g64 = s.astype(np.float64), g.astype(np.float64)
    assert (np.abs(g64 * g64 - s64) <= np.abs(below * below - s64)).all() and (np.abs(g64 * g64 - s64) <= np.abs(above * above - s64)).all()
    want = g.max() - g
    assert np.array_equal(bd.confidence(u8).numpy(), want)
    theirs = obil.sobel_confidence(u8).numpy()
    g_theirs = torch.sqrt(torch.from_numpy(s)).numpy()
    print(f'{name}: torch.sqrt differs from the correctly rounded root at {int((g_theirs != g).sum())} of {g.size} voxels, the '
          f'confidence at {int((theirs != want).sum())}')
    assert (np.abs(g_theirs.astype(np.float64) - g64) <= np.spacing(g)).all()


def test_what_the_cases_are_for():
    by = bd.BY_NAME
    a, b = by['a_interior'], by['b_faces']
    assert all(lo > 0 and hi < n for (lo, hi), n in zip(a.box, a.shape))
    assert b.box[0][0] == 0 and b.centre[0] - (b.radius - 1) - 2 < 0 and b.box[1][1] == b.shape[1]      # clamped low, at the high face
    # device key space: luma bins of the table x spatial bins of the crop; more than 1024 blocks of 1024 keys
    for name in ('c_rank_blocks', 'h_sigma1'):
        c = by[name]
        lut, _, _ = obil.yuv_bins_of_grey(obil.GRID_PARAMS['sigma_luma'], obil.GRID_PARAMS['sigma_chroma'])
        keys = (int(lut.max()) + 1) * int(np.prod([int((hi - lo - 1) / c.gp['sigma_spatial']) + 1 for lo, hi in c.box]))
        assert keys > 1024 * 1024 and (keys + 1023) // 1024 > 1024
        grid = bd.reference(name)[1]['grid']
        assert (grid.key_of_voxel >= bd.RANK_SCAN_KEYS).any() and (grid.key_of_voxel < bd.RANK_SCAN_KEYS).any()
    assert bd.reference('c_rank_blocks')[1]['grid'].nvertices > 100_000
    assert bd.reference('h_sigma1')[1]['grid'].nvertices == 31 ** 3                      # every voxel its own vertex
    # sigma_luma = 1: 255 bins of the 256 the library takes -- the float64 luma of grey 255 is 254.99999999999997
    assert int(obil.yuv_bins_of_grey(4, 5)[0].max()) + 1 == 64 and int(obil.yuv_bins_of_grey(1, 5)[0].max()) + 1 == 255
    assert bd.reference('e_luma1')[1]['grid'].dims[0] > 64
    f = by['f_thin']
    assert f.shape[0] == 1 and bd.reference('f_thin')[1]['grid'].dims[1] == 1


@pytest.mark.parametrize('name', LIVE)
def test_live_case_conditions(name):
    """No zero-confidence vertex and no NaN; at every convergence test of the CG the residual is at least 1 % away from
    atol, so that fp64 reordering (1e-15) cannot make the device stop on another iteration; the solve changes the map."""
    c = bd.BY_NAME[name]
    ref, trace = bd.reference(name)
    assert float(trace['w_splat'].min()) > 0.0
    assert bool(torch.isfinite(ref).all())
    ratios = np.asarray(trace['residual_norms']) / trace['atol']
    assert ratios.size >= 1 and np.isfinite(ratios).all()
    assert not ((ratios > 0.99) & (ratios < 1.01)).any(), ratios
    sl = bd.box_slices(c.box)
    moved = (ref[sl] - bd.data(name)[1][sl]).abs()
    assert float(moved.max()) > 1e-3
    print(f'{name}: min splat(confidence) {float(trace["w_splat"].min()):.3g}, {ratios.size} convergence tests, residual / atol '
          f'{ratios.min():.3g} .. {ratios.max():.3g}, the solve moves {int((moved > 0).sum())} of {moved.numel()} box voxels, by up to {float(moved.max()):.3g}')


def test_only_the_small_case_converges():
    """a to f run into cg_maxiter; j_converges stops at its third test, with the residual seven orders below atol."""
    for name in LIVE:
        trace = bd.reference(name)[1]
        ratios = np.asarray(trace['residual_norms']) / trace['atol']
        if name == 'j_converges':
            assert ratios.size == 3 and ratios[-1] < 1e-3 and ratios[-2] > 1e3
        else:
            assert ratios.size == obil.SOLVER_PARAMS['cg_maxiter'] and ratios.min() > 100


@pytest.mark.parametrize('name', ZERO)
def test_zero_cases(name):
    """g, h: a vertex with zero confidence, NaN through the CG, an all-zero crop after nan_to_num; i: an all-zero right-hand
    side, returned at once."""
    c = bd.BY_NAME[name]
    ref, trace = bd.reference(name)
    crop = ref[bd.box_slices(c.box)]
    assert bool((crop.view(torch.int32) == 0).all())
    if name == 'i_zero_rhs':
        assert trace['atol'] == 0.0 and trace['residual_norms'] == [] and float(trace['w_splat'].min()) > 0.0
    else:
        assert float(trace['w_splat'].min()) == 0.0 and trace['atol'] > 0.0
        assert len(trace['residual_norms']) == obil.SOLVER_PARAMS['cg_maxiter'] and np.isnan(trace['residual_norms']).all()
    bd.check_zero(ref, name)
    wrong = ref.clone()
    wrong[c.box[0][0], c.box[1][0], c.box[2][0]] = -0.0                                  # even a negative zero is seen
    with pytest.raises(AssertionError):
        bd.check_zero(wrong, name)


# ---------------------------------------------------------------------------------------------- the GPU tests can fail
def test_refine_with_is_the_reference():
    for name in ('a_interior', 'b_faces'):
        assert torch.equal(bd.refine_with(name).view(torch.int32), bd.reference(name)[0].view(torch.int32))
        bd.check(bd.reference(name)[0], name)


@pytest.mark.parametrize('name', LIVE)
def test_reordering_noise_is_below_the_criterion(name):
    """Splats perturbed by 1e-12 relative -- three orders above what another summation order does -- leave the fp32
    reference bit-identical, over three seeds; 1e-9 moves voxels by one spacing at the most."""
    ref = bd.reference(name)[0]
    for seed in (0, 1, 2):
        out = bd.refine_with(name, grid=bd.perturbed_splats(1e-12, seed))
        differ = int((out.view(torch.int32) != ref.view(torch.int32)).sum())
        print(f'{name}: splats x (1 + 1e-12 randn), seed {seed}: {differ} voxels differ')
        assert differ == 0
    r = bd.compare(bd.refine_with(name, grid=bd.perturbed_splats(1e-9, 0)), ref, bd.data(name)[1], bd.BY_NAME[name].box)
    print(f'{name}: splats x (1 + 1e-9 randn): {r.not_bit_equal} of {r.voxels} voxels differ, by at most {r.worst:.3g} spacings')
    assert bd.passes(r) and r.worst <= 1.0


def _mutants(name):
    m = [(what, dict(grid=make)) for what, make in bd.GRID_MUTANTS.items()]
    m.append(('crop origin off by one', dict(shift=bd.origin_shift(name))))
    if name == 'c_rank_blocks':
        m.append(('vertex ids shifted behind key 1024 * 1024', dict(grid=bd.SHIFTED_IDS)))
    return m


@pytest.mark.parametrize('name', [c.name for c in bd.WITH_MUTANTS])
def test_mutants_break_the_criterion(name):
    """Each subtly wrong solver breaks the criterion inside the box on at least one voxel by a factor of at least 100."""
    c = bd.BY_NAME[name]
    ref, sim = bd.reference(name)[0], bd.data(name)[1]
    for what, how in _mutants(name):
        out = bd.refine_with(name, **how)
        r = bd.compare(out, ref, sim, c.box)
        factor = bd.mutant_factor(name, out)
        print(f'{name}: {what}: criterion broken by a factor of {factor:.3g} at {r.worst_at}; {r.not_bit_equal} of {r.voxels} box '
              f'voxels differ, {r.moved_outside} outside the box')
        assert not bd.passes(r)
        assert factor >= 100, (name, what, factor)
        with pytest.raises(AssertionError):
            bd.check(out, name, f' ({what})')
        if 'origin' in what:
            assert r.moved_outside > 0


def test_compare_by_hand():
    """The criterion on a 1 x 1 x 4 map with the box [1:3]: spacings of |ref|, the smallest normal spacing at ref == 0, NaN
    counted as wrong, the outside compared by bits."""
    box = ((0, 1), (0, 1), (1, 3))
    sim = torch.tensor([[[0.0, 0.5, 0.5, 0.0]]])
    ref = torch.tensor([[[0.0, 1.0, 0.0, 0.0]]])
    one = float(np.spacing(np.float32(1.0)))
    r = bd.compare(torch.tensor([[[0.0, 1.0 + 2 * one, 0.0, 0.0]]]), ref, sim, box)
    assert (r.worst, r.not_bit_equal, r.moved_outside, r.voxels, r.worst_at) == (2.0, 1, 0, 2, (0, 0, 1)) and bd.passes(r)
    assert not bd.passes(bd.compare(torch.tensor([[[0.0, 1.0 + 3 * one, 0.0, 0.0]]]), ref, sim, box))
    tiny = float(np.spacing(np.float32(bd.TINY)))
    assert bd.passes(bd.compare(torch.tensor([[[0.0, 1.0, 2 * tiny, 0.0]]]), ref, sim, box))
    assert not bd.passes(bd.compare(torch.tensor([[[0.0, 1.0, 3 * tiny, 0.0]]]), ref, sim, box))
    assert not bd.passes(bd.compare(torch.tensor([[[0.0, float('nan'), 0.0, 0.0]]]), ref, sim, box))
    assert not bd.passes(bd.compare(torch.tensor([[[-0.0, 1.0, 0.0, 0.0]]]), ref, sim, box))
    assert not bd.passes(bd.compare(torch.tensor([[[0.0, 1.0, 0.0, 1e-45]]]), ref, sim, box))


# ---------------------------------------------------------------------------------------------- the trilinear reference
@pytest.mark.parametrize('src_shape,out_shape', bd.TRILINEAR_SHAPES)
def test_trilinear_reference(src_shape, out_shape):
    """F.interpolate(mode='trilinear') on the CPU lies within the derived bound of the fp64 blend everywhere, and a blend with
    align_corners=True does not.  The source index scale * (o + 0.5) - 0.5 is one rounding in the kernel (fmaf) and in a
    CPU operator built with multiply-add contraction (the AVX2 / AVX-512 kernels of torch 2.10), two in a build without: the
    weights of a few output indices then differ by one spacing of the index, which is up to 1.5 bounds at
    (7, 5, 9) -> (20, 18, 22).  So the operator is held to the reference of its own convention, whichever that is here; the
    GPU test holds the kernel to the fused one."""
    src = torch.randn(src_shape, generator=torch.Generator().manual_seed(sum(out_shape)))
    ref, bound = bd.trilinear_ref(src.numpy(), out_shape)
    assert ref.shape == bound.shape == tuple(out_shape) and ref.dtype == np.float64
    want = F.interpolate(src[None, None], out_shape, mode='trilinear')[0, 0].numpy().astype(np.float64)
    plain_ref, plain_bound = bd.trilinear_ref(src.numpy(), out_shape, fused=False)
    fused, plain = np.abs(want - ref) / bound, np.abs(want - plain_ref) / plain_bound
    print(f'{src_shape} -> {out_shape}: F.interpolate / bound: {fused.max():.3g} with the kernel\'s fused source index, {plain.max():.3g} '
          f'with the unfused one; the two references differ by up to {(np.abs(ref - plain_ref) / bound).max():.3g} bounds')
    assert fused.max() <= 1.0 or plain.max() <= 1.0
    for axis, (n, o) in enumerate(zip(src_shape, out_shape)):
        for fused in (True, False):
            i0, i1, w0, w1 = bd._lin_coord(o, n, fused)
            assert i0.min() >= 0 and i1.max() <= n - 1 and ((i1 == i0) | (i1 == i0 + 1)).all() and (w1 >= 0).all() and (w1 < 1).all()
            if n == o:
                assert (i0 == np.arange(o)).all() and (w1 == 0).all() and (w0 == 1).all()
            if n == 1:
                assert (i0 == 0).all() and (i1 == 0).all()
    # the other convention of the same operator is far outside
    other = F.interpolate(src[None, None], out_shape, mode='trilinear', align_corners=True)[0, 0].numpy().astype(np.float64)
    assert (np.abs(other - ref) > 100 * bound).mean() > 0.25


def test_trilinear_reference_by_hand():
    """2 -> 4 along x: source indices -0.25 (clamped to 0), 0.25, 0.75, 1.25 (i1 clamped)."""
    src = np.array([[[1.0, 3.0]]], dtype=np.float32)
    ref, bound = bd.trilinear_ref(src, (1, 1, 4))
    assert ref.reshape(-1).tolist() == [1.0, 1.5, 2.5, 3.0]
    assert bound.reshape(-1).tolist() == [8 * bd.U * 3.0] * 4      # the zero-weight corner counts
