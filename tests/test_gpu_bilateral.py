"""GPU: vittf_bilateral_refine (csrc/bilateral.hip) voxel by voxel against the fp64 oracle, on the cases of
tests/bls_data.py whose resize and uint8 stages are exact: every voxel of the crop box within two fp32 spacings of the
reference, every voxel outside it bit-equal to the input, the vertex and voxel counts exact -- with crop boxes away from
the origin and clamped at faces, more than 1024 rank blocks, 64 and 255 luma bins, a one-voxel-thick volume, NaN through
the CG, an all-zero right-hand side and a CG that converges early; the kept one-workgroup solver in a child process; and the
trilinear stage on its own against an fp64 blend.

tests/test_bls_data_cpu.py shows that the cases are what they claim, that reordered fp64 sums stay three orders of magnitude
below the criterion and that a dropped neighbour link, a voxel that is not splatted, vertex ids shifted behind a rank-scan
boundary, a crop origin off by one and a wrong blur weight each break it by a factor above 1000."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_tf_amd as vt
import bls_data as bd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_runs = {}                    # case name -> [(map on the host, info)] of two calls on the same inputs


def _refine_twice(gpu, name):
    if name not in _runs:
        c = bd.BY_NAME[name]
        volume, sim = (t.to(gpu) for t in bd.data(name))
        _runs[name] = []
        for _ in range(2):
            info = {}
            got = vt.bilateral.refine_similarity(sim, volume, c.shape, grid_params=c.gp, info=info)
            _runs[name].append((got.cpu(), info))
        assert torch.equal(sim.cpu(), bd.data(name)[1]) and torch.equal(volume.cpu(), bd.data(name)[0])     # inputs untouched
    return _runs[name]


def _check(got, info, name, what):
    c = bd.BY_NAME[name]
    grid = bd.reference(name)[1]['grid']
    assert got.shape == c.shape and got.dtype == torch.float32
    assert info == {'vertices': grid.nvertices, 'voxels': bd.box_volume(c.box)}, (info, grid.nvertices, bd.box_volume(c.box))
    if c.zero:
        bd.check_zero(got, name, what)
    else:
        bd.check(got, name, what)


@pytest.mark.parametrize('name', [c.name for c in bd.CASES])
def test_refine_per_voxel(gpu, name):
    """info['vertices'] is the oracle's vertex count and info['voxels'] the box volume, exactly.  Live cases: every box voxel
    within 2 fp32 spacings of the reference, none exempt, every voxel outside the box bit-equal to the input.  Zero cases:
    the crop exactly +0.0.  A second call on the same inputs meets the same criterion (not the same bytes: the splat adds
    fp64 atomically)."""
    first, second = _refine_twice(gpu, name)
    _check(*first, name, '')
    _check(*second, name, ' (second call)')


@pytest.mark.parametrize('names', [('a_interior', 'c_rank_blocks')], ids=['a-c'])
def test_one_workgroup_solver(gpu, tmp_path, names):
    """VITTF_BLS_SOLVER=0, the first-version solve_kernel the library keeps: the same criterion.  The switch is
    read once per process, so the calls run in a fresh child (this file as a script)."""
    out = tmp_path / 'solver0.npz'
    env = dict(os.environ, PYTHONPATH=ROOT, VITTF_BLS_SOLVER='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out), *names], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr + r.stdout
    with np.load(out) as z:
        for name in names:
            info = dict(zip(('vertices', 'voxels'), (int(v) for v in z[name + '_info'])))
            _check(torch.from_numpy(z[name]), info, name, ' (one-workgroup solver)')


@pytest.mark.parametrize('src_shape,out_shape', bd.TRILINEAR_SHAPES)
def test_trilinear_stage(gpu, src_shape, out_shape):
    """trilinear_kernel alone: with crop_threshold = 1e30 nothing is above the threshold and vittf_bilateral_refine returns the
    resized map unrefined.  Every voxel within 8 x 2^-24 x max |corner| of the fp64 blend of the same fp32 indices and
    weights (bls_data.trilinear_ref has the derivation; the source index is one fmaf, as in lin_coord).  F.interpolate on the
    CPU is printed against it, not asserted equal: the voxels where the two differ are held to the same bound of the fp64
    blend.  A build of that operator which rounds the product of scale * (o + 0.5) - 0.5 before the subtraction has other
    weights at a few output indices (test_bls_data_cpu.py: up to 1.5 bounds from this reference at the first shape)."""
    src = torch.randn(src_shape, generator=torch.Generator().manual_seed(sum(out_shape)))
    volume = torch.rand((4, 5, 6), generator=torch.Generator().manual_seed(1))
    info = {}
    got = vt.bilateral.refine_similarity(src.to(gpu), volume.to(gpu), out_shape, crop_threshold=1e30, info=info).cpu()
    assert info == {'vertices': 0, 'voxels': 0} and got.shape == tuple(out_shape) and got.dtype == torch.float32
    ref, bound = bd.trilinear_ref(src.numpy(), out_shape)
    g = got.numpy().astype(np.float64)
    assert np.isfinite(g).all() and float(bound.min()) > 0
    ratio = np.abs(g - ref) / bound
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    cpu = F.interpolate(src[None, None], out_shape, mode='trilinear')[0, 0].numpy()
    differ = got.numpy().view(np.int32) != cpu.view(np.int32)
    print(f'{src_shape} -> {out_shape}: worst error / bound {ratio.max():.3g} at {tuple(int(i) for i in at)}; {int(differ.sum())} of '
          f'{differ.size} voxels differ from F.interpolate on the CPU, by up to '
          f'{(np.abs(g - cpu.astype(np.float64)) / bound).max():.3g} bounds; those are within {ratio[differ].max() if differ.any() else 0.0:.3g} '
          f'bounds of the fp64 blend')
    assert ratio.max() <= 1.0, (at, float(got[at]), float(ref[at]), float(bound[at]))
    assert not differ.any() or ratio[differ].max() <= 1.0


def _child(out, names):
    """What test_one_workgroup_solver starts: the named cases through refine_similarity in this process, saved for the parent."""
    assert os.environ.get('VITTF_BLS_SOLVER') == '0'
    gpu = torch.device('cuda', 0)
    saved = {}
    for name in names:
        c = bd.BY_NAME[name]
        volume, sim = (t.to(gpu) for t in bd.data(name))
        info = {}
        got = vt.bilateral.refine_similarity(sim, volume, c.shape, grid_params=c.gp, info=info)
        saved[name] = got.cpu().numpy()
        saved[name + '_info'] = np.array([info['vertices'], info['voxels']], dtype=np.int64)
    np.savez(out, **saved)


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2:])
