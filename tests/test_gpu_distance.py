"""GPU: Euclidean distance transform and surface scores -- vittf_edt_sq, vittf_edt_sq_weighted, vit_tf_amd.distance and
score_labels.py.

The integer path is exact: every voxel equals rint(scipy.ndimage.distance_transform_edt ** 2) and, on the volumes small enough
for it, the fp64 brute-force minimum over all sites (distance_data), with np.array_equal.  The weighted path is held to
|got - want| <= 2^-24 want + 2^-40 D2 against the fp64 brute force (test_weighted_path_within_the_bound).  The feature
transform is checked by what it promises -- a site, at the returned distance -- not against scipy's choice among ties.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import distance_data as dd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dist = vt.distance


def _rule(k):
    return dd.RULES[k % len(dd.RULES)]


def _raw(gpu, vol, value=-1, mode=0, w2=None, sites=True):
    """The C entry itself on a device copy of vol: (status, d2, site); outputs pre-filled with a pattern the call must replace."""
    lib = _lib.load()
    src = torch.from_numpy(np.ascontiguousarray(vol)).to(gpu)
    n0, n1, n2 = vol.shape
    d2 = torch.full(vol.shape, -7, dtype=torch.int32 if w2 is None else torch.float32, device=gpu)
    site = torch.full(vol.shape, -7, dtype=torch.int32, device=gpu) if sites else None
    ws_bytes = lib.vittf_edt_workspace_bytes(n0, n1, n2)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=gpu)
    if w2 is None:
        rc = lib.vittf_edt_sq(_lib.ptr(src), n0, n1, n2, value, mode, _lib.ptr(d2), _lib.ptr(site), _lib.ptr(ws), ws_bytes,
                              _lib.stream_ptr())
    else:
        rc = lib.vittf_edt_sq_weighted(_lib.ptr(src), n0, n1, n2, value, mode, (C.c_double * 3)(*w2), _lib.ptr(d2), _lib.ptr(site),
                                       _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, d2, site


# ---------------------------------------------------------------------------- 1. integer path, exact
@pytest.mark.parametrize('shape', dd.SHAPES)
def test_integer_path_is_exact(gpu, shape):
    for k, name in enumerate(dd.MASKS):
        value, mode = _rule(k)
        vol = dd.volume(shape, name, value, mode)
        got = dist.edt(torch.from_numpy(vol).to(gpu), value, bool(mode), squared=True)
        assert got.dtype == torch.int32 and tuple(got.shape) == shape and got.is_cuda
        got = got.cpu().numpy()
        want = dd.want_int(shape, name)
        assert np.array_equal(got, want), (name, value, mode, int((got != want).sum()))
        if shape in dd.SMALL:
            assert np.array_equal(got.astype(np.float64), dd.want_brute(shape, name)), (name, value, mode)


@pytest.mark.parametrize('value,mode', dd.RULES)
def test_every_site_rule(gpu, value, mode):
    shape = (5, 7, 67)
    for name in ('three', 'half', 'box'):
        vol = dd.volume(shape, name, value, mode)
        rc, d2, _ = _raw(gpu, vol, value, mode, sites=False)
        assert rc == 0
        assert np.array_equal(d2.cpu().numpy(), dd.want_int(shape, name)), (name, value, mode)
        got = dist.edt(vol, value, bool(mode))                                          # numpy in, fp32 distances out
        assert got.dtype == torch.float32
        assert np.allclose(got.cpu().numpy(), np.sqrt(dd.want_int(shape, name).astype(np.float64)), rtol=2e-7, atol=0), name


# ---------------------------------------------------------------------------- 2. feature transform
@pytest.mark.parametrize('shape', dd.SHAPES)
def test_feature_transform_names_a_site_at_the_distance(gpu, shape):
    for k, name in enumerate(dd.MASKS):
        value, mode = _rule(k + 2)
        vol = dd.volume(shape, name, value, mode)
        rc, d2, site = _raw(gpu, vol, value, mode)
        assert rc == 0
        d2, site = d2.cpu().numpy(), site.cpu().numpy().astype(np.int64)
        assert np.array_equal(d2, dd.want_int(shape, name)), name
        assert site.min() >= 0 and site.max() < vol.size
        assert dd.sites(shape, name).reshape(-1)[site.reshape(-1)].all(), name         # every index is a site
        index = np.stack(np.unravel_index(site, shape))
        assert np.array_equal(dd.site_d2(index), d2.astype(np.float64)), name          # at the returned distance
    # the Python layer: scipy's (3, n0, n1, n2) layout
    name = 'three'
    d, index = dist.edt(dd.volume(shape, name, -1, 0), return_indices=True)
    assert index.dtype == torch.int32 and tuple(index.shape) == (3, *shape)
    assert np.array_equal(dd.site_d2(index.cpu().numpy()), dd.want_int(shape, name).astype(np.float64))
    assert np.allclose(d.cpu().numpy(), np.sqrt(dd.want_int(shape, name).astype(np.float64)), rtol=2e-7, atol=0)


@pytest.mark.parametrize('spacing', dd.SPACINGS)
def test_weighted_feature_transform(gpu, spacing):
    shape = (5, 7, 67)
    w2 = [s * s for s in spacing]
    slack = 2.0 ** -40 * dd.d2_bound(shape, spacing)
    for name in ('three', 'half', 'sphere'):
        rc, d2, site = _raw(gpu, dd.volume(shape, name, -1, 0), w2=w2)
        assert rc == 0
        site = site.cpu().numpy().astype(np.int64)
        assert dd.sites(shape, name).reshape(-1)[site.reshape(-1)].all(), name
        at_site = dd.site_d2(np.stack(np.unravel_index(site, shape)), spacing)
        want = dd.want_brute(shape, name, spacing)
        assert (np.abs(at_site - want) <= slack).all(), name
        assert (np.abs(d2.cpu().numpy().astype(np.float64) - at_site) <= 2.0 ** -24 * at_site + slack).all(), name


# ---------------------------------------------------------------------------- 3. no site, determinism
@pytest.mark.parametrize('shape', [(5, 7, 67), (3, 130, 9), (1, 1, 300)])
def test_volume_without_a_site(gpu, shape):
    vol = np.full(shape, 4, np.uint8)
    for value, mode in ((7, 0), (4, 1), (-1, 1)):
        rc, d2, site = _raw(gpu, vol, value, mode)
        assert rc == 0                                                                  # VITTF_OK
        assert bool((d2 == _lib.EDT_NO_SITE).all()) and bool((site == -1).all()), (value, mode)
        rc, d2, site = _raw(gpu, vol, value, mode, w2=(0.49, 0.49, 6.25))
        assert rc == 0
        assert bool(torch.isinf(d2).all()) and bool((d2 > 0).all()) and bool((site == -1).all()), (value, mode)
    for spacing in (None, (0.7, 0.7, 2.5)):
        d, index = dist.edt(vol, 7, spacing=spacing, return_indices=True)
        assert d.dtype == torch.float32 and bool(torch.isinf(d).all()) and bool((index == -1).all())
        assert bool(torch.isinf(dist.edt(vol, 7, spacing=spacing, squared=spacing is not None)).all())
    assert bool((dist.edt(vol, 7, squared=True) == dist.NO_SITE).all())
    sd = dist.signed(vol, 4)
    assert bool(torch.isinf(sd).all()) and bool((sd < 0).all())                          # all inside
    sd = dist.signed(vol, 7)
    assert bool(torch.isinf(sd).all()) and bool((sd > 0).all())                          # all outside


def test_two_calls_give_the_same_bytes(gpu):
    shape = (64, 64, 64)
    vol = dd.volume(shape, 'half', -1, 0)
    sparse = dd.volume(shape, 'three', -1, 0)
    for v in (vol, sparse):
        for w2 in (None, (0.49, 0.49, 6.25)):
            _, d_a, s_a = _raw(gpu, v, w2=w2)
            _, d_b, s_b = _raw(gpu, v, w2=w2)
            assert torch.equal(d_a, d_b) and torch.equal(s_a, s_b)
            _, d_c, _ = _raw(gpu, v, w2=w2, sites=False)                                 # and without the feature transform
            assert torch.equal(d_a, d_c)


# ---------------------------------------------------------------------------- 4. weighted path
@pytest.mark.parametrize('spacing', dd.SPACINGS)
@pytest.mark.parametrize('shape', dd.SMALL)
def test_weighted_path_within_the_bound(gpu, shape, spacing):
    """|got - want| <= 2^-24 want + 2^-40 D2, want the fp64 brute-force minimum, D2 = sum_a w2[a] (n_a - 1)^2.
    2^-24 want is the single rounding to fp32.  2^-40 D2 covers the fp64 envelope arithmetic: every intermediate is at most
    2 D2, every operation rounds at 2^-53 (six roundings on the value's way through the three passes), and a comparison or a
    separator that rounding decides the other way exchanges only two sites whose values differ by that much."""
    w2 = [s * s for s in spacing]
    D2 = dd.d2_bound(shape, spacing)
    for k, name in enumerate(dd.MASKS):
        value, mode = _rule(k + 1)
        vol = dd.volume(shape, name, value, mode)
        got = dist.edt(torch.from_numpy(vol).to(gpu), value, bool(mode), spacing=spacing, squared=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        got = got.cpu().numpy().astype(np.float64)
        want = dd.want_brute(shape, name, spacing)
        err = np.abs(got - want)
        bound = 2.0 ** -24 * want + 2.0 ** -40 * D2
        print(f'{shape} {spacing} {name}: max err {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}')
        assert (err <= bound).all(), (name, float((err / bound).max()))
        rc, raw, _ = _raw(gpu, vol, value, mode, w2=w2, sites=False)
        assert rc == 0 and np.array_equal(raw.cpu().numpy().astype(np.float64), got)    # the Python layer adds nothing


@pytest.mark.parametrize('shape', dd.SHAPES)
def test_unit_spacing_equals_the_integer_path(gpu, shape):
    for name in ('three', 'half', 'sphere'):
        vol = torch.from_numpy(dd.volume(shape, name, -1, 0)).to(gpu)
        exact = dist.edt_sq(vol)
        weighted = dist.edt_sq(vol, spacing=(1, 1, 1))
        assert weighted.dtype == torch.float32 and torch.equal(weighted, exact.to(torch.float32)), name


# ---------------------------------------------------------------------------- 5. surfaces, signed distance, scores
def _boxes(shape=(24, 20, 18), shift=3):
    t = np.zeros(shape, np.uint8)
    t[4:12, 5:14, 3:11] = 1
    p = np.zeros(shape, np.uint8)
    p[4 + shift:12 + shift, 5:14, 3:11] = 1
    return t, p


def test_surface_and_signed_match_scipy(gpu):
    from scipy import ndimage
    vol = dd.ball((20, 23, 70), (8, 11, 30), 7)
    vol[:3, :, :5] = 1                                                                 # a part on the volume's border
    for connectivity in (1, 2, 3):
        got = dist.surface(vol, connectivity)
        assert got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy().astype(bool), dd.surface(vol != 0, connectivity)), connectivity
    assert bool(dist.surface(np.ones((4, 5, 6), np.uint8))[0].all())                   # border voxels of a mask are surface
    for spacing in (None, (0.7, 0.7, 2.5)):
        want = ndimage.distance_transform_edt(vol == 0, sampling=spacing) - ndimage.distance_transform_edt(vol != 0, sampling=spacing)
        got = dist.signed(vol, 1, spacing).cpu().numpy()
        assert np.allclose(got, want, rtol=5e-7, atol=0), spacing      # fp32: the rounding of d2, then the square root
        assert (np.abs(got) >= (1.0 if spacing is None else 0.7) * (1 - 1e-6)).all()     # the zero level lies between voxels


def test_surface_scores_of_shifted_and_identical_boxes(gpu):
    t, p = _boxes()
    s = dist.surface_scores(t, p)
    assert set(s) == set(dist.SCORE_KEYS) and all(len(v) == 1 for v in s.values())
    assert s['hd'][0] == 3.0 and s['hd95'][0] == 3.0                                   # exactly
    want = dd.surface_scores(t, p, [1])
    for k in dist.SCORE_KEYS:
        assert s[k][0] == pytest.approx(want[k][0], rel=1e-6), k
    assert s['n_surface_target'][0] == s['n_surface_pred'][0] == 8 * 9 * 8 - 6 * 7 * 6
    same = dist.surface_scores(t, t, [1])
    assert same['hd'][0] == 0 and same['hd95'][0] == 0 and same['assd'][0] == 0 and same['nsd'][0] == 1.0
    a, b = dist.surface_distances(t, p, 1)
    assert a.dtype == torch.float32 and a.numel() == b.numel() == s['n_surface_target'][0]
    assert float(a.max()) == 3.0 and float(b.max()) == 3.0


@pytest.mark.parametrize('spacing', [None, (0.7, 0.7, 2.5)])
def test_surface_scores_of_spheres_match_the_restatement(gpu, spacing):
    shape = (40, 36, 44)
    t = dd.ball(shape, (19, 17, 21), 12)
    dd.ball(shape, (8, 8, 8), 4, value=2, into=t)                                      # class 2: only in the target
    p = dd.ball(shape, (20, 18, 20), 9)
    classes = [1, 2, 3]                                                                # class 3: in neither
    got = dist.surface_scores(torch.from_numpy(t).to(gpu), p, classes, spacing, tolerance=2.0)
    want = dd.surface_scores(t, p, classes, spacing, tolerance=2.0)
    for k in dist.SCORE_KEYS:
        assert got[k].shape == (3,)
        assert got[k][0] == pytest.approx(want[k][0], rel=1e-6), k
    assert got['hd'][0] > 3 and 0 < got['nsd'][0] < 1
    assert got['hd'][1] == np.inf and got['hd95'][1] == np.inf and got['assd'][1] == np.inf and got['nsd'][1] == 0.0
    assert np.isnan(got['hd'][2]) and np.isnan(got['hd95'][2]) and np.isnan(got['assd'][2]) and got['nsd'][2] == 1.0
    assert got['n_surface_target'].tolist() == want['n_surface_target'].tolist()
    assert got['n_surface_pred'].tolist() == want['n_surface_pred'].tolist() and got['n_surface_pred'][1] == 0
    default = dist.surface_scores(t, p, spacing=spacing)                               # classes default to 1 .. max
    assert len(default['hd']) == 2 and default['hd'][0] == got['hd'][0]


# ---------------------------------------------------------------------------- 6. command line, end to end
def test_score_labels_end_to_end(gpu, tmp_path, capsys):
    import score_labels
    shape = (32, 32, 32)
    t = dd.ball(shape, (15, 15, 15), 9)
    dd.ball(shape, (5, 26, 6), 3, value=2, into=t)
    p = dd.ball(shape, (16, 14, 15), 8)
    dd.ball(shape, (6, 26, 6), 3, value=2, into=p)
    np.save(tmp_path / 'labels.npy', t)
    np.save(tmp_path / 'mlp_pred3.npy', p)
    argv = ['--target', str(tmp_path / 'labels.npy'), '--pred', str(tmp_path / 'mlp_pred3.npy'), '--spacing', '0.7', '0.7', '2.5',
            '--tolerance', '1.5']
    with pytest.raises(SystemExit) as e:
        score_labels.main(argv)
    assert e.value.code == 0
    got = json.load(open(tmp_path / 'mlp_pred3_surface.json'))
    assert set(got) == {'classes', *dist.SCORE_KEYS, 'overlap', 'spacing', 'tolerance', 'grid', 'target_grid', 'time'}
    assert got['classes'] == [1, 2] and got['grid'] == [32, 32, 32] and got['spacing'] == [0.7, 0.7, 2.5] and got['tolerance'] == 1.5
    want = dist.surface_scores(t, p, [1, 2], (0.7, 0.7, 2.5), 1.5)
    for k in dist.SCORE_KEYS:
        assert got[k] == want[k].tolist(), k
    acc, prec, rec, f1, iou, cm = vt.scores.scores(t, p)
    assert set(got['overlap']) == {'labels', 'accuracy', 'precision', 'recall', 'f1', 'iou', 'confusion_matrix'}
    assert got['overlap']['labels'] == [0, 1, 2] and got['overlap']['accuracy'] == float(acc)
    assert got['overlap']['iou'] == iou.tolist() and got['overlap']['confusion_matrix'] == cm.tolist()
    with pytest.raises(SystemExit) as e:
        score_labels.main(argv)                                                         # refuses to overwrite
    assert e.value.code == 1 and 'Cache file already exists' in capsys.readouterr().out
    # a target on a finer grid is resampled to the prediction's, and its spacing scaled with it
    np.save(tmp_path / 'fine.npy', np.repeat(np.repeat(np.repeat(t, 2, 0), 2, 1), 2, 2))
    with pytest.raises(SystemExit) as e:
        score_labels.main(['--target', str(tmp_path / 'fine.npy'), '--pred', str(tmp_path / 'mlp_pred3.npy'), '--spacing', '0.35',
                           '0.35', '1.25', '--tolerance', '1.5', '--overwrite'])
    assert e.value.code == 0
    fine = json.load(open(tmp_path / 'mlp_pred3_surface.json'))
    assert fine['target_grid'] == [64, 64, 64] and fine['spacing'] == [0.7, 0.7, 2.5]
    for k in dist.SCORE_KEYS:
        assert fine[k] == got[k], k
