"""GPU: connected components -- vittf_label_components, vittf_component_sizes, vittf_filter_components, vit_tf_amd.components,
label_islands.py and predict_ntf.py --largest-island.

Everything is exact: labels are compared with scipy.ndimage.label(mask, generate_binary_structure(3, c)), renumbered to 1 + the
lowest linear index of every component (components_data.oracle_labels), with np.array_equal; sizes with np.bincount; the filter
with numpy.  There is no tolerance anywhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import components_data as cd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cc = vt.components
BIG = (128, 128, 128)


def _labels(vol, select=-1, connectivity=1):
    return cc.label(vol, select, connectivity).cpu().numpy()


def _raw_sizes(labels_dev):
    n = labels_dev.numel()
    sizes = torch.full((n,), -7, dtype=torch.int32, device=labels_dev.device)      # the call zeroes it
    _lib.check(_lib.load().vittf_component_sizes(_lib.ptr(labels_dev), n, _lib.ptr(sizes), _lib.stream_ptr()))
    return sizes


def _bincount(labels, n):
    return np.bincount(labels.reshape(-1), minlength=n + 1)[1:].astype(np.int32)


# ---------------------------------------------------------------------------- 1. labels against scipy
@pytest.mark.parametrize('connectivity', [1, 2, 3])
@pytest.mark.parametrize('shape', cd.SHAPES)
def test_labels_match_scipy(gpu, shape, connectivity):
    for name, vol in cd.patterns(shape, connectivity).items():
        got = cc.label(vol, -1, connectivity)
        assert got.dtype == torch.int32 and tuple(got.shape) == shape and got.is_cuda
        want = cd.oracle(shape, connectivity, name)
        assert np.array_equal(got.cpu().numpy(), want), (name, int((got.cpu().numpy() != want).sum()))
    want = cd.oracle(shape, connectivity, 'checkerboard')
    ncomp = len(np.unique(want[want > 0]))
    if connectivity == 1:
        assert ncomp == int(cd.checkerboard(shape).sum())                               # no links at all
    elif sum(n > 1 for n in shape) >= 2:
        assert ncomp == 1                                                               # one body through the edge diagonals
    want = cd.oracle(shape, connectivity, 'serpentine')
    assert len(np.unique(want[want > 0])) == 1                                          # one component


@pytest.mark.parametrize('connectivity', [1, 2, 3])
def test_slabs_touching_across_a_tile_corner(gpu, connectivity):
    vol = cd.corner_slabs()
    got = _labels(vol, -1, connectivity)
    assert np.array_equal(got, cd.oracle_labels(vol != 0, connectivity))
    assert len(np.unique(got[got > 0])) == (1 if connectivity == 3 else 2)


def test_labels_at_size_sizes_and_determinism(gpu):
    """128^3 at the 6-neighbour percolation threshold: components snake through many tiles.  The only case at size."""
    vol = cd.noise(BIG, cd.PERCOLATION[1], 7)
    dev = torch.from_numpy(vol).to(gpu)
    first = cc.label(dev, -1, 1)
    want = cd.oracle_labels(vol != 0, 1)
    assert np.array_equal(first.cpu().numpy(), want)
    again = cc.label(dev, -1, 1)
    assert torch.equal(first, again)                                                    # the same bytes
    sizes = _raw_sizes(first)
    assert np.array_equal(sizes.cpu().numpy(), _bincount(want, want.size))
    assert torch.equal(cc.sizes(first), sizes)
    ids, counts = cc.table(first)
    u, c = np.unique(want[want > 0], return_counts=True)
    order = np.lexsort((u, -c))
    assert np.array_equal(ids.cpu().numpy(), u[order]) and np.array_equal(counts.cpu().numpy(), c[order])


@pytest.mark.parametrize('name', ['dense', 'ones', 'percolation', 'zeros'])
def test_component_sizes_match_bincount(gpu, name):
    """One giant component (every add of a workgroup lands on one label), the percolation case (many labels: the LDS table
    overflows into direct adds) and the empty volume; a volume that is no whole number of chunks."""
    shape = (40, 40, 260)
    want = cd.oracle(shape, 1, name)
    dev = torch.from_numpy(want.copy()).to(gpu)
    assert np.array_equal(_raw_sizes(dev).cpu().numpy(), _bincount(want, want.size))
    small = torch.from_numpy(cd.oracle((3, 5, 7), 1, name).copy()).to(gpu)
    assert np.array_equal(_raw_sizes(small).cpu().numpy(), _bincount(small.cpu().numpy(), small.numel()))


# ---------------------------------------------------------------------------- 2. select modes
@pytest.mark.parametrize('connectivity', [1, 2, 3])
def test_select_modes(gpu, connectivity):
    shape = (2 * cd.T0 + 1, 3 * cd.T1 + 1, 2 * cd.T2 + 2)
    vol = cd.value_blocks(shape, 11 + connectivity)
    assert set(np.unique(vol)) == {0, 1, 2, 3, 4, 5, 255}
    each = cd.oracle_each_value(vol, connectivity)
    assert np.array_equal(_labels(vol, -2, connectivity), each)
    assert (each[vol == 255] == 0).all() and (each[vol != 255] > 0).all()
    for v in (0, 3, 255, 7):                                                            # 7 does not occur: all background
        assert np.array_equal(_labels(vol, v, connectivity), cd.oracle_labels(vol == v, connectivity)), v
    assert np.array_equal(_labels(vol, -1, connectivity), cd.oracle_labels(vol != 0, connectivity))
    # a source at a 1-byte offset, as a CPU tensor and as a numpy array
    flat = torch.zeros(vol.size + 1, dtype=torch.uint8, device=gpu)
    flat[1:] = torch.from_numpy(vol).reshape(-1).to(gpu)
    view = flat[1:].reshape(shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert np.array_equal(cc.label(view, -2, connectivity).cpu().numpy(), each)
    assert np.array_equal(cc.label(torch.from_numpy(vol), -2, connectivity).cpu().numpy(), each)


# ---------------------------------------------------------------------------- 3. filter
def _raw_filter(src, labels, sizes, min_size, keep_label, fill, in_place):
    dst = src if in_place else torch.full_like(src, 99)
    _lib.check(_lib.load().vittf_filter_components(_lib.ptr(src), _lib.ptr(labels), _lib.ptr(sizes), src.numel(), min_size, keep_label,
                                                   fill, _lib.ptr(dst), _lib.stream_ptr()))
    return dst.cpu().numpy()


@pytest.mark.parametrize('offset', [0, 1])
def test_filter_components_matches_numpy(gpu, offset):
    """min_size 1, 2, largest, largest + 1 and keep_label, in place and out of place; offset 1: byte-aligned volumes (the
    one-voxel-per-thread kernel), offset 0: the four-voxel kernel with its ragged tail (nvox % 4 == 2)."""
    shape = (5, 9, 66)
    vol = cd.value_blocks(shape, 5)
    vol = np.where((vol == 255) | (vol == 0), 0, vol + 3).astype(np.uint8)             # background 0, bodies of values 4..8
    want_lab = cd.oracle_labels(vol != 0, 1)
    labels = cc.label(vol, -1, 1)
    assert np.array_equal(labels.cpu().numpy(), want_lab)
    sizes = cc.sizes(labels)
    counts = _bincount(want_lab, want_lab.size)
    largest = int(counts.max())
    assert largest > 2
    size_of = np.concatenate(([0], counts))[want_lab]

    def device_copy():
        flat = torch.zeros(vol.size + offset, dtype=torch.uint8, device=gpu)
        flat[offset:] = torch.from_numpy(vol).reshape(-1).to(gpu)
        return flat[offset:].reshape(shape)

    for in_place in (False, True):
        for fill in (0, 200):
            for min_size in (1, 2, largest, largest + 1):
                want = np.where((want_lab != 0) & (size_of >= min_size), vol, fill).astype(np.uint8)
                got = _raw_filter(device_copy(), labels, sizes, min_size, 0, fill, in_place)
                assert np.array_equal(got, want), (in_place, fill, min_size)
            keep = int(want_lab[want_lab > 0].max())
            want = np.where(want_lab == keep, vol, fill).astype(np.uint8)
            assert np.array_equal(_raw_filter(device_copy(), labels, None, 1, keep, fill, in_place), want), (in_place, fill)
    want = np.where((want_lab != 0) & (size_of >= 3), vol, 17).astype(np.uint8)
    assert np.array_equal(cc.remove_small(vol, 3, fill=17).cpu().numpy(), want)
    assert (cc.remove_small(vol, largest + 1).cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------- 4. largest island
def test_largest_island_against_the_scipy_recipe(gpu):
    rng = np.random.default_rng(3)
    shape = (2 * cd.T0 + 1, 3 * cd.T1 + 1, 2 * cd.T2 + 2)
    coarse = rng.integers(0, 256, size=(3, 5, 9)).astype(np.uint8)                      # blobs of 3 x 5 x 15 voxels
    sim = np.repeat(np.repeat(np.repeat(coarse, 3, 0), 5, 1), 15, 2)[:shape[0], :shape[1], :shape[2]].copy()
    sim ^= rng.integers(0, 8, size=shape).astype(np.uint8)                              # the kept values are not constant
    for thr, connectivity in ((69, 1), (160, 1), (200, 2), (200, 3)):
        want = cd.largest_island_recipe(sim, thr, connectivity)
        assert 0 < (want != 0).sum() < (sim > thr).sum(), 'the case has one island only'
        got = cc.largest_island(sim, thr, connectivity)
        assert got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), (thr, connectivity)
    # an empty set: all zero (the reference raises there)
    assert (cc.largest_island(sim, 255).cpu().numpy() == 0).all()
    assert (cc.largest_island(np.zeros(shape, np.uint8), 0).cpu().numpy() == 0).all()
    # two islands of equal size: the one with the lower voxel index wins; the comparison is strict
    tie = np.zeros(shape, np.uint8)
    tie[1, 2, 3:9] = 90
    tie[5, 20, 100:106] = 200
    tie[7, 7, 7] = 70                                                                   # == threshold: not in the set
    want = np.zeros(shape, np.uint8)
    want[1, 2, 3:9] = 90
    assert np.array_equal(cc.largest_island(tie, 70).cpu().numpy(), want)
    assert np.array_equal(cd.largest_island_recipe(tie, 70), want)


# ---------------------------------------------------------------------------- 5. command lines
def _run(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    return subprocess.run([sys.executable, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_label_islands_cli(gpu, tmp_path):
    shape = (9, 25, 130)
    vol = cd.value_blocks(shape, 21, block=(3, 4, 6))
    src = tmp_path / 'v_clusters6.npy'
    np.save(src, vol)
    r = _run('label_islands.py', '--labels', str(src), '--each-value', '--min-size', '4')
    assert r.returncode == 0, r.stderr + r.stdout
    isl_path, table_path = tmp_path / 'v_clusters6_islands.npy', tmp_path / 'v_clusters6_islands.npz'
    isl = np.load(isl_path)
    assert isl.dtype == np.uint8 and isl.shape == shape
    each = cd.oracle_each_value(vol, 1)
    u, c = np.unique(each[each > 0], return_counts=True)
    order = np.lexsort((u, -c))
    u, c = u[order], c[order]
    keep = c >= 4
    u, c = u[keep][:255], c[keep][:255]
    assert len(u) > 3 and c[0] >= c[-1] >= 4
    want = np.zeros(each.size + 1, np.uint8)
    want[u] = np.arange(1, len(u) + 1)
    assert np.array_equal(isl, want[each])
    with np.load(table_path, allow_pickle=False) as z:
        assert set(z.files) == {'sizes', 'lowest_index', 'values'}
        assert np.array_equal(z['sizes'], c) and z['sizes'].dtype == np.int64
        assert np.array_equal(z['lowest_index'], u - 1) and z['lowest_index'].dtype == np.int64
        assert np.array_equal(z['values'], vol.reshape(-1)[u - 1]) and z['values'].dtype == np.uint8
        assert 255 not in z['values']
    first = (isl_path.read_bytes(), table_path.read_bytes())
    r = _run('label_islands.py', '--labels', str(src), '--each-value', '--min-size', '4', '--overwrite')
    assert r.returncode == 0, r.stderr + r.stdout
    assert first == (isl_path.read_bytes(), table_path.read_bytes())


def test_ntf_largest_island_flag(gpu, tmp_path):
    """predict_ntf.py on a small directory with fixed annotations of one class (the fixture of the pipeline test), with and
    without --largest-island: the flag only adds the `isl` file, its prediction is the label rule on the map after the scipy
    recipe, a subset of the plain prediction, and the plain run is what it was.  Then two classes in process: each map is cut
    at its own class threshold.  (With several classes a voxel whose winning class is cut away may fall to another class, so
    only the foreground as a whole is a subset there.)"""
    import predict_ntf
    d = tmp_path / 'case'
    d.mkdir()
    g = torch.Generator().manual_seed(5)
    vol = torch.rand((32, 32, 32), generator=g).numpy().astype(np.float32)
    coarse = torch.randn((1, 32, 4, 4, 4), generator=g)
    feats = torch.nn.functional.interpolate(coarse, size=(16, 16, 16), mode='trilinear', align_corners=False)[0]
    feats = torch.nn.functional.normalize(feats, dim=0).half()
    ann = {'ntf1': np.array([[3, 4, 5], [4, 5, 6], [6, 4, 3]])}
    np.save(d / 'volume.npy', vol)
    np.save(d / 'v_features16.npy', {'k': feats.numpy()}, allow_pickle=True)
    np.save(d / 'annotations.npy', ann, allow_pickle=True)
    r = _run('predict_ntf.py', '--data', str(d))
    assert r.returncode == 0, r.stderr + r.stdout
    plain_path, isl_path = d / 'ntf_pred0.0annotated.npy', d / 'ntf_pred0.0annotatedisl.npy'
    assert plain_path.exists() and not isl_path.exists()
    plain_bytes = plain_path.read_bytes()
    r = _run('predict_ntf.py', '--data', str(d), '--largest-island')
    assert r.returncode == 0, r.stderr + r.stdout
    assert isl_path.exists() and plain_path.read_bytes() == plain_bytes
    plain, isl = np.load(plain_path), np.load(isl_path)
    # both against the in-process calls on the inputs predict_ntf.py prepares (the volume flipped on axis -3)
    flipped = np.flip(vol, axis=-3).copy()
    tann = {k: torch.from_numpy(v) for k, v in ann.items()}
    sims = vt.compute_similarities(flipped, feats, tann)
    assert np.array_equal(plain, vt.assign_labels(sims, predict_ntf.ct_org_thresholds))
    kept = {k: torch.from_numpy(cd.largest_island_recipe(v.numpy(), int(predict_ntf.ct_org_thresholds[i] * 255)))
            for i, (k, v) in enumerate(sims.items())}
    assert np.array_equal(isl, vt.assign_labels(kept, predict_ntf.ct_org_thresholds))
    assert set(np.unique(plain)) == {0, 1} and (isl == 1).any()
    assert not ((isl == 1) & (plain != 1)).any()
    two = dict(tann, ntf2=torch.tensor([[25, 20, 27], [27, 22, 26]]))
    sims = vt.compute_similarities(flipped, feats, two, keep_on_device=True)
    got = predict_ntf.keep_largest_islands(sims)
    assert list(got) == ['ntf1', 'ntf2']
    for i, k in enumerate(got):
        want = cd.largest_island_recipe(sims[k].cpu().numpy(), int(predict_ntf.ct_org_thresholds[i] * 255))
        assert np.array_equal(got[k].cpu().numpy(), want), k
    assert not ((predict_ntf.assign_labels(got) != 0) & (predict_ntf.assign_labels(sims) == 0)).any()
