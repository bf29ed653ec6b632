"""CPU: the volume renderer -- the C-ABI surface of vittf_render_prepare / vittf_render_occupancy_bytes / vittf_render_occupancy /
vittf_render (declared, exported, every argument error without a launch), the host arithmetic of vit_tf_amd.render (camera, PNG
writer, composite, default tables), the invariants of the fp64 restatement the GPU tests compare against (tests/render_data.py)
and the refusals of render_volume.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import render_data as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NAMES = ('vittf_render_prepare', 'vittf_render_occupancy_bytes', 'vittf_render_occupancy', 'vittf_render')
render = vt.render


def _p(on, addr=0x1000):
    return C.c_void_p(addr) if on else None


def _f(values):
    return None if values is None else (C.c_float * len(values))(*values)


def _i(values):
    return None if values is None else (C.c_int32 * len(values))(*values)


CAMERA = [0, 0, -10, 4, 0, 0, 0, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]


def _render(lib, shape=(8, 9, 10), spacing=(1, 1, 1), table=0x1000, maps=0x1000, classes=2, grid=(4, 4, 4), lo=(10, 20), hi=(200, 210),
            rgbs=(1, 0, 0, 1, 0, 1, 0, 2), occ=0, camera=CAMERA, size=(16, 16), dt=0.5, shade=(0.3, 0.7, 1.0), q=0x1000, out=0x1000):
    """vittf_render on placeholder addresses: only calls the argument checks refuse are made with it."""
    return lib.vittf_render(_p(q, q), *shape, _f(spacing), _p(table, table), _p(maps, maps), classes, *grid, _i(lo), _i(hi), _f(rgbs),
                            _p(occ, occ), _f(camera), *size, dt, _f(shade), _p(out, out), None)


def _occupancy(lib, shape=(8, 9, 10), table=0x1000, maps=0x1000, classes=2, grid=(4, 4, 4), lo=(10, 20), q=0x1000, occ=0x1000):
    return lib.vittf_render_occupancy(_p(q, q), *shape, _p(table, table), _p(maps, maps), classes, *grid, _i(lo), _p(occ, occ), None)


# ---------------------------------------------------------------------------- 1. ABI surface
def test_render_entries_are_declared_exported_and_the_abi_stays_6():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    for name, value in (('MAX_DIM', 2048), ('MAX_IMAGE', 8192), ('MAX_CLASSES', 8)):
        assert int(re.search(r'#define\s+VITTF_RENDER_' + name + r'\s+(\d+)', header).group(1)) == getattr(_lib, 'RENDER_' + name) == value
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    assert vt.render is not None and 'render' in dir(vt)
    assert 'render.hip' in open(os.path.join(ROOT, 'vit-tf_amd', 'csrc', 'Makefile')).read()


BAD_SHAPES = ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-3, 8, 8), (2049, 8, 8), (8, 2049, 8), (8, 8, 2049), (2048, 2048, 512),
              (2048, 1024, 1024))


def test_occupancy_bytes_counts_bricks_and_refuses_shapes():
    lib = _lib.load()
    for shape, want in (((2, 2, 2), 1), ((8, 8, 8), 1), ((9, 8, 8), 2), ((9, 11, 13), 2 * 2 * 2), ((40, 24, 17), 5 * 3 * 3),
                        ((512, 512, 512), 64 ** 3), ((2048, 2047, 512), 256 * 256 * 64)):
        assert lib.vittf_render_occupancy_bytes(*shape) == want, shape
    for shape in BAD_SHAPES:
        assert lib.vittf_render_occupancy_bytes(*shape) == 0, shape


def test_prepare_argument_errors_return_invalid_without_a_launch():
    lib = _lib.load()
    call = lambda vol=0x1000, n=100, vmin=0.0, vmax=1.0, q=0x1000: lib.vittf_render_prepare(_p(vol, vol), n, vmin, vmax, _p(q, q), None)   # noqa: E731
    assert call(vol=0) == INVALID and call(q=0) == INVALID
    for n in (0, -1, 2 ** 31):
        assert call(n=n) == INVALID, n
    for vmin, vmax in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('nan')), (0.0, float('inf')), (-float('inf'), 0.0),
                       (-1.7e308, 1.7e308)):
        assert call(vmin=vmin, vmax=vmax) == INVALID, (vmin, vmax)
    assert call(vol=0x1004) == INVALID and call(q=0x1002) == INVALID          # 16-byte loads, 8-byte stores


def test_occupancy_argument_errors_return_invalid_without_a_launch():
    lib = _lib.load()
    for missing in ('q', 'table', 'occ', 'maps'):
        assert _occupancy(lib, **{missing: 0}) == INVALID, missing
    assert _occupancy(lib, lo=None) == INVALID
    for shape in BAD_SHAPES:
        assert _occupancy(lib, shape=shape) == INVALID, shape
        assert _occupancy(lib, grid=shape) == INVALID, shape
    for classes in (-1, 9, 100):
        assert _occupancy(lib, classes=classes, lo=(1,) * 9) == INVALID, classes
    for lo in ((-1, 5), (5, 256)):
        assert _occupancy(lib, lo=lo) == INVALID, lo
    assert _occupancy(lib, table=0x1004) == INVALID and _occupancy(lib, q=0x1001) == INVALID


def test_render_argument_errors_return_invalid_without_a_launch():
    lib = _lib.load()
    for missing in ('q', 'table', 'out', 'maps'):
        assert _render(lib, **{missing: 0}) == INVALID, missing
    for missing in ('spacing', 'camera', 'shade', 'lo', 'hi', 'rgbs'):
        assert _render(lib, **{missing: None}) == INVALID, missing
    for shape in BAD_SHAPES:
        assert _render(lib, shape=shape) == INVALID, shape
        assert _render(lib, grid=shape) == INVALID, shape
    for classes in (-1, 9):
        assert _render(lib, classes=classes, lo=(1,) * 9, hi=(2,) * 9, rgbs=(1,) * 36) == INVALID, classes
    for lo, hi in (((-1, 5), (9, 9)), ((5, 5), (5, 9)), ((5, 5), (9, 4)), ((5, 5), (9, 256)), ((255, 5), (255, 9))):
        assert _render(lib, lo=lo, hi=hi) == INVALID, (lo, hi)
    for size in ((0, 16), (16, 0), (-1, 16), (8193, 16), (16, 8193)):
        assert _render(lib, size=size) == INVALID, size
    for dt in (0.0, -0.5, float('nan'), float('inf'), 1e-9):                   # 1e-9: more than 2^22 samples along a ray
        assert _render(lib, dt=dt) == INVALID, dt
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        for axis in range(3):
            sp = [1.0, 1.0, 1.0]
            sp[axis] = bad
            assert _render(lib, spacing=sp) == INVALID, (bad, axis)
    for at in range(18):
        for bad in (float('nan'), float('inf')):
            cam = list(CAMERA)
            cam[at] = bad
            assert _render(lib, camera=cam) == INVALID, (at, bad)
    cam = list(CAMERA)
    cam[9:12] = [0, 0, 0]                                                       # no forward direction
    assert _render(lib, camera=cam) == INVALID
    for shade in ((-0.1, 0.5, 1.0), (0.5, -0.1, 1.0), (0.5, 0.5, 0.0), (0.5, 0.5, -1.0), (float('nan'), 0.5, 1.0), (0.5, 0.5, float('inf'))):
        assert _render(lib, shade=shade) == INVALID, shade
    for at, bad in ((3, -1.0), (7, float('nan')), (0, float('inf')), (5, float('nan'))):      # strengths >= 0, everything finite
        rgbs = [1, 0, 0, 1, 0, 1, 0, 2]
        rgbs[at] = bad
        assert _render(lib, rgbs=rgbs) == INVALID, (at, bad)
    assert _render(lib, table=0x1008) == INVALID and _render(lib, out=0x1008) == INVALID and _render(lib, q=0x1001) == INVALID


def test_python_entries_refuse_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a refused call reached the device')

    monkeypatch.setattr(_lib, 'require_device', boom)
    vol = np.zeros((4, 5, 6), np.float32)
    for bad in (vol.astype(np.float64), vol[0], np.zeros((1, 5, 6), np.float32), np.zeros((2, 2, 2049), np.float32)):
        with pytest.raises(ValueError):
            render.prepare(bad)
    with pytest.raises(ValueError):
        render.prepare(vol, vmin=float('nan'))
    q = torch.zeros((4, 5, 6), dtype=torch.uint16)
    cam = render.Camera.orbit(0, 0, shape=(4, 5, 6))
    table = torch.as_tensor(render.ramp_table())
    ok = dict(camera=cam, size=(8, 8))
    for bad in (dict(q=q.to(torch.int32)), dict(q=q[0]), dict(camera=None), dict(size=(0, 8)), dict(size=(8, 8193)), dict(size=8),
                dict(spacing=(1, 1)), dict(spacing=(1, 0, 1)), dict(step=0), dict(step=float('nan')), dict(step='a'),
                dict(table=table[:, :3]), dict(table=table.double()), dict(table=-table),
                dict(maps=np.zeros((9, 4, 4, 4), np.uint8)), dict(maps=np.zeros((2, 4, 4, 4), np.int32)), dict(maps=np.zeros((4, 4, 4), np.uint8)),
                dict(maps=np.zeros((2, 1, 4, 4), np.uint8)), dict(maps=np.zeros((2, 4, 4, 4), np.uint8), lo=[1, 2, 3]),
                dict(maps=np.zeros((2, 4, 4, 4), np.uint8), lo=200, hi=100), dict(maps=np.zeros((2, 4, 4, 4), np.uint8), hi=256),
                dict(maps=np.zeros((2, 4, 4, 4), np.uint8), lo=1.5), dict(maps=np.zeros((2, 4, 4, 4), np.uint8), strengths=[1.0, -1.0]),
                dict(maps=np.zeros((2, 4, 4, 4), np.uint8), colors=[(1, 1, 1)]), dict(shading=(0.5, 0.5, 0.0)), dict(shading=(0.5, 0.5)),
                dict(occupancy='yes'), dict(out=torch.zeros((8, 8, 3)))):
        kw = {'q': q, **ok, **bad}
        with pytest.raises(ValueError):
            render.render(kw.pop('q'), kw.pop('camera'), kw.pop('size'), **kw)
    with pytest.raises(ValueError):
        render.occupancy(q, table[:10])
    with pytest.raises(ValueError):
        render.occupancy(q.float(), table)
    for bad in (np.zeros((4, 4, 4), np.int32), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            render.maps_from_labels(bad)
    with pytest.raises(ValueError):
        render.maps_from_labels(np.full((4, 4, 4), 9, np.uint8))                 # nine classes
    with pytest.raises(ValueError):
        render.maps_from_labels(np.zeros((4, 4, 4), np.uint8))                   # none


# ---------------------------------------------------------------------------- 2. host arithmetic
def test_maps_from_labels_are_one_hot_0_255():
    lab = np.random.default_rng(0).integers(0, 4, (5, 6, 7)).astype(np.uint8)
    maps = render.maps_from_labels(lab)
    assert maps.dtype == torch.uint8 and tuple(maps.shape) == (3, 5, 6, 7)
    for c in range(3):
        assert np.array_equal(maps[c].numpy(), np.where(lab == c + 1, 255, 0))
    two = render.maps_from_labels(lab, [3, 0])
    assert np.array_equal(two[0].numpy(), np.where(lab == 3, 255, 0)) and np.array_equal(two[1].numpy(), np.where(lab == 0, 255, 0))


def test_orbit_camera_vectors():
    shape, spacing = (40, 24, 17), (1.0, 1.0, 2.5)
    ext = np.asarray(shape) * np.asarray(spacing)
    centre, radius = ext / 2, np.linalg.norm(ext) / 2
    for az, el in ((0, 0), (30, 20), (135, -40), (10, 90), (200, -90)):
        for fov in (None, 40.0):
            cam = render.Camera.orbit(az, el, fov=fov, shape=shape, spacing=spacing, aspect=4 / 3)
            v = cam.vectors().astype(np.float64)
            assert v.shape == (6, 3) and cam.vectors().dtype == np.float32
            eye, ox, oy, fwd, dx, dy = v
            out = np.array([np.cos(np.radians(el)) * np.cos(np.radians(az)), np.cos(np.radians(el)) * np.sin(np.radians(az)),
                            np.sin(np.radians(el))])
            assert np.allclose(fwd, -out, atol=1e-6) and np.isclose(np.linalg.norm(fwd), 1, atol=1e-6)
            to_centre = centre - eye
            assert np.allclose(to_centre / np.linalg.norm(to_centre), fwd, atol=1e-5)          # it looks at the centre
            assert np.linalg.norm(to_centre) > radius                                            # from outside the box
            right, up = (ox, oy) if fov is None else (dx, dy)
            other = (dx, dy) if fov is None else (ox, oy)
            assert not np.any(other[0]) and not np.any(other[1])
            assert abs(right @ fwd) < 1e-5 and abs(up @ fwd) < 1e-5 and abs(right @ up) < 1e-4
            assert np.allclose(np.cross(right, up) / np.linalg.norm(np.cross(right, up)), -fwd, atol=1e-5)    # right-handed image
            if abs(el) < 89:
                assert up[2] > 0                                                                 # axis 2 points up
            if fov is None:
                assert np.isclose(np.linalg.norm(oy), radius, rtol=1e-6) and np.isclose(np.linalg.norm(ox), radius * 4 / 3, rtol=1e-6)
            else:
                assert np.isclose(np.linalg.norm(dy), np.tan(np.radians(20.0)), rtol=1e-6)
                assert np.isclose(np.linalg.norm(dx), np.tan(np.radians(20.0)) * 4 / 3, rtol=1e-6)
    near = render.Camera.orbit(0, 0, distance=3.0, shape=shape, spacing=spacing)
    assert np.allclose(np.asarray(near.eye), centre + [3.0, 0, 0], atol=1e-5)
    for bad in (dict(fov=0), dict(fov=180), dict(distance=-1), dict(aspect=0), dict(spacing=(1, 0, 1)), dict(shape=(1, 4, 4))):
        kw = {'shape': shape, **bad}
        with pytest.raises(ValueError):
            render.Camera.orbit(0, 0, **kw)
    with pytest.raises(ValueError):
        render.Camera.orbit(float('nan'), 0, shape=shape)


def test_write_png_decodes_to_the_same_bytes(tmp_path):
    rng = np.random.default_rng(1)
    for shape in ((17, 33, 3), (5, 7, 4), (9, 4), (1, 1, 3)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        render.write_png(tmp_path / 'a.png', img)
        assert np.array_equal(rd.decode_png(tmp_path / 'a.png').reshape(shape), img)
    render.write_png(tmp_path / 't.png', torch.as_tensor(img))
    assert np.array_equal(rd.decode_png(tmp_path / 't.png').reshape(img.shape), img)
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros((4,), np.uint8)):
        with pytest.raises(ValueError):
            render.write_png(tmp_path / 'b.png', bad)


def test_composite_and_default_tables():
    rgba = np.array([[[0, 0, 0, 0], [0.25, 0.5, 0.75, 1.0], [0.1, 0.1, 0.1, 0.5], [2.0, -1.0, 0.5, 1.0]]], np.float32)
    got = render.composite(rgba, (1.0, 0.0, 0.5))
    assert got.dtype == np.uint8 and got.shape == (1, 4, 3)
    assert got.tolist() == [[[255, 0, 128], [64, 128, 191], [153, 26, 89], [255, 0, 128]]]
    assert torch.equal(render.composite(torch.as_tensor(rgba), (1.0, 0.0, 0.5)), torch.as_tensor(got))
    with pytest.raises(ValueError):
        render.composite(rgba[..., :3])
    for table in (render.ramp_table(), render.context_table()):
        assert table.dtype == np.float32 and table.shape == (256, 4) and np.isfinite(table).all()
        assert (table[:, 3] >= 0).all() and table[0, 3] == 0 and (np.diff(table[:, 3]) >= 0).all() and table[255, 3] > 0
    assert render.context_table()[255, 3] < render.ramp_table()[255, 3]
    # a slab of the reference length has the stated opacity
    assert np.isclose(1 - np.exp(-render.sigma_from_opacity(0.9, 32.0) * 32.0), 0.9, rtol=1e-12)
    assert len(render.PALETTE) == 8 and len(set(render.PALETTE)) == 8


# ---------------------------------------------------------------------------- 3. the restatement's own invariants
def test_scenes_cover_the_cases():
    shapes = {rd.SCENES[n][0] for n in rd.SCENES}
    assert {(9, 11, 13), (32, 32, 32), (40, 24, 17)} <= shapes
    assert {rd.SCENES[n][2] for n in rd.SCENES} >= {(5, 6, 7), (8, 8, 8)}
    assert {rd.SCENES[n][3] for n in rd.SCENES} == {0, 1, 3, 8}
    assert {rd.SCENES[n][4] for n in rd.SCENES} == {(64, 48), (33, 17)}
    assert {rd.SCENES[n][5] for n in rd.SCENES} == {'axis0', 'axis1', 'axis2', 'oblique', 'outside', 'inside', 'miss'}
    assert {rd.SCENES[n][6] for n in rd.SCENES} == {(1, 1, 1), (1, 1, 2.5)}
    assert {rd.SCENES[n][7] for n in rd.SCENES} == {0.5, 1.0}
    assert {rd.SCENES[n][8] for n in rd.SCENES} == {rd.SHADE, rd.FLAT}
    for name in ('axis0_c0', 'axis1_c1', 'axis2_c3'):                              # exactly axis-parallel rays
        d = rd.rays(rd.scene(name), np.float32)[1]
        assert ((d == 0).sum(0) == 2).all(), name
    s = rd.scene('inside_c3')                                                     # the eye really is inside the box
    assert (s['camera'][0] > 0).all() and (s['camera'][0] < np.asarray(s['q'].shape) * s['spacing']).all()
    touching = rd.scene('outside_c8')['q']
    assert touching[0].max() > 30000 and touching[:, :, 0].max() > 30000         # matter on the border
    assert rd.scene('axis2_c3')['q'][0].max() < 2000                             # air border elsewhere
    q = rd.scene('axis0_c0')
    assert q['q'].dtype == np.uint16 and q['q'].min() == 0 and q['q'].max() == 65535


def test_reference_invariants_and_both_kinds_of_tolerance():
    stops, runs = [], []
    for name in rd.SCENES:
        img64, img32, tmin = rd.references(name)
        w, h = rd.scene(name)['size']
        assert img64.shape == (h, w, 4) and img64.dtype == np.float64 and img32.dtype == np.float32
        assert np.isfinite(img64).all() and np.isfinite(img32).all()
        assert (img64 >= 0).all() and img64[..., 3].max() <= 1.0 and img32[..., 3].max() <= 1.0
        tol, own, _ = rd.tolerance(name)
        if name in rd.ZERO_SCENES:
            assert not img64.any() and not img32.any() and tol == 0.0, name      # missing rays, all-zero sigma: exact zeros
            continue
        assert img64[..., 3].max() > 0.2 and 0 < own < 1e-4, (name, own)
        (stops if tmin < 2.0 ** -9 else runs).append(name)
        assert tol == 8 * own + (2.0 ** -10 if tmin < 2.0 ** -9 else 0.0)
    assert len(stops) >= 2 and len(runs) >= 2, (stops, runs)                     # one of each kind at the least
    first, last = rd.rays(rd.scene('miss_c1'), np.float64)[2:]
    assert (first > last).all()
    some = rd.references('outside_c8')[0]
    assert not some[0, 0].any() and some[..., 3].max() > 0.9                      # a corner ray misses, a central one is opaque


def test_halving_the_step_converges():
    s = dict(rd.scene('oblique_c3'))
    imgs = []
    for dt in (1.0, 0.5, 0.25):
        s['dt'] = dt
        imgs.append(rd.reference(s, np.float64)[0])
    coarse, fine = np.abs(imgs[0] - imgs[1]).max(), np.abs(imgs[1] - imgs[2]).max()
    assert 0 < fine < coarse, (coarse, fine)


def test_occupancy_rule_is_not_vacuous_and_hides_no_sample():
    for name in rd.OCCUPANCY_SCENES:
        s = rd.scene(name)
        occ, top = rd.occupancy(s), rd.sample_sigma_by_brick(s)
        assert occ.shape == tuple((n + 7) // 8 for n in s['q'].shape) == top.shape
        assert (occ == 0).any() and (occ == 1).any(), name
        assert not ((occ == 0) & (top > 0)).any(), name
        assert (top > 0).any(), name


# ---------------------------------------------------------------------------- 4. command line
def _main(argv):
    import render_volume
    with pytest.raises(SystemExit) as e:
        render_volume.main(argv)
    return e.value.code


def test_render_volume_cli_refusals(tmp_path, monkeypatch, capsys):
    """Every exit-1 case with its message, all before anything touches the device; the frame names."""
    import render_volume

    def boom(*a, **k):
        raise AssertionError('a refused command line reached the GPU entry')

    for entry in ('prepare', 'render', 'occupancy'):
        monkeypatch.setattr(vt.render, entry, boom)
    monkeypatch.setattr(_lib, 'require_device', boom)
    assert render_volume.frame_paths(tmp_path / 'a.png', None) == [tmp_path / 'a.png']
    assert render_volume.frame_paths(tmp_path / 'a.png', 3) == [tmp_path / f'a_00{k}.png' for k in range(3)]
    d = tmp_path / 'case'
    d.mkdir()
    out = lambda: capsys.readouterr().out                     # noqa: E731
    assert _main(['--data', str(d)]) == 1
    assert 'Invalid argument for --data (File does not exist)' in out()
    np.save(d / 'volume.npy', np.zeros((6, 7, 8), np.float16))
    np.save(d / 'pred.npy', np.ones((3, 4, 4), np.uint8))
    np.save(d / 'nine.npy', np.full((3, 4, 4), 9, np.uint8))
    np.save(d / 'none.npy', np.zeros((3, 4, 4), np.uint8))
    np.save(d / 'i32.npy', np.ones((3, 4, 4), np.int32))
    np.save(d / 'maps9.npy', np.zeros((9, 3, 4, 4), np.uint8))
    np.save(d / 'maps3d.npy', np.zeros((3, 4, 4), np.uint8))
    np.save(d / 'sims9.npy', {f'c{k}': np.zeros((3, 4, 4), np.uint8) for k in range(9)}, allow_pickle=True)
    np.save(d / 'ragged.npy', {'a': np.zeros((3, 4, 4), np.uint8), 'b': np.zeros((3, 4, 5), np.uint8)}, allow_pickle=True)
    np.save(d / 'tf3.npy', np.zeros((256, 3), np.float32))
    (d / 'broken.npy').write_bytes(b'not an array')
    base = ['--data', str(d)]
    with pytest.raises(SystemExit) as e:
        render_volume.main(base + ['--maps', 'maps9.npy', '--labels', 'pred.npy'])          # one of the two
    assert e.value.code == 2
    capsys.readouterr()
    for flag, name, text in (('--labels', 'nine.npy', 'labels up to 9, at most 8 classes'), ('--labels', 'none.npy', 'no label above 0'),
                             ('--labels', 'i32.npy', 'expected a uint8 (W, H, D) label volume'), ('--labels', 'broken.npy', 'not a readable .npy'),
                             ('--labels', 'nope.npy', '(File does not exist)'), ('--maps', 'maps9.npy', '9 classes, at most 8'),
                             ('--maps', 'sims9.npy', '9 classes, at most 8'), ('--maps', 'maps3d.npy', "expected uint8 (C, W', H', D') maps"),
                             ('--maps', 'ragged.npy', 'differ in shape'), ('--maps', 'nope.npy', '(File does not exist)'),
                             ('--tf', 'tf3.npy', 'expected a finite float32 (256, 4) table')):
        assert _main(base + [flag, name]) == 1, (flag, name)
        text_out = out()
        assert f'Invalid argument for {flag}' in text_out and text in text_out, (flag, name, text_out)
    for argv, flag in ((['--spacing', '1', '0', '1'], '--spacing'), (['--spacing', '1', 'nan', '1'], '--spacing'), (['--size', '0', '8'], '--size'),
                       (['--size', '8', '8193'], '--size'), (['--fov', '0'], '--fov'), (['--fov', '180'], '--fov'), (['--step', '0'], '--step'),
                       (['--step', 'nan'], '--step'), (['--lo', '200', '--hi', '100'], '--lo / --hi'), (['--hi', '256'], '--lo / --hi'),
                       (['--lo', '-1'], '--lo / --hi'), (['--background', '0', '2', '0'], '--background'), (['--turntable', '0'], '--turntable'),
                       (['--azimuth', 'nan'], '--azimuth')):
        assert _main(base + argv) == 1, argv
        assert f'Invalid argument for {flag}' in out(), argv
    (d / 'render.png').write_bytes(b'keep')
    assert _main(base) == 1
    assert 'Cache file already exists' in out() and (d / 'render.png').read_bytes() == b'keep'
    (d / 'turn_001.png').write_bytes(b'keep')
    assert _main(base + ['--turntable', '3', '--output', str(d / 'turn.png')]) == 1             # any frame in the way
    assert 'Cache file already exists' in out()
    assert _main(base + ['--output', str(d / 'missing_dir' / 'r.png')]) == 1
    assert 'Invalid argument for --output (Cannot write to location)' in out()
