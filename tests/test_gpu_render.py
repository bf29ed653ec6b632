"""GPU: the volume renderer (render.hip through vit_tf_amd.render) against the fp64 restatement of tests/render_data.py.

prepare and occupancy are integer results and must equal the restatement; an image is compared per pixel and channel with
the scene's own tolerance, 8 max|ref32 - ref64| (+ 2^-10 where a reference ray gets below T = 2^-9), the float32 run being the
restatement's, never the kernel's.  Every image test prints the three figures; DESIGN.md 4.17 lists them as measured.
"""
import zlib

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import render_data as rd

pytestmark = pytest.mark.gpu
render = vt.render
_DEVICE = {}


def _camera(s):
    return render.Camera(*(tuple(float(x) for x in v) for v in s['camera']))


def _inputs(name, dev):
    """(scene, q, table, maps) with the arrays on the device, uploaded once per scene."""
    if name not in _DEVICE:
        s = rd.scene(name)
        _DEVICE[name] = (s, render.prepare(torch.as_tensor(s['volume']).to(dev)), torch.as_tensor(s['table']).to(dev),
                         None if s['maps'] is None else torch.as_tensor(s['maps']).to(dev))
    return _DEVICE[name]


def _render(name, dev, occupancy='auto', out=None):
    s, q, table, maps = _inputs(name, dev)
    return render.render(q, _camera(s), s['size'], spacing=s['spacing'], table=table, maps=maps, lo=s['lo'] or None, hi=s['hi'] or None,
                         colors=s['colors'], strengths=s['strengths'], step=s['dt'], shading=tuple(float(v) for v in s['shade']),
                         occupancy=occupancy, out=out)


@pytest.mark.parametrize('shape', [(9, 11, 13), (40, 24, 17), (32, 32, 33)])
def test_prepare_equals_the_restatement(gpu, shape):
    vol = rd.volume(shape, seed=3, touch_border=True)
    got = render.prepare(torch.as_tensor(vol).to(gpu))
    assert got.dtype == torch.uint16 and tuple(got.shape) == shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), rd.prepare(vol))
    lo, hi = -400.0, 712.5                                                        # a window inside the range clamps both ways
    got = render.prepare(vol, lo, hi).cpu().numpy()
    assert np.array_equal(got, rd.prepare(vol, lo, hi)) and got.min() == 0 and got.max() == 65535
    with pytest.raises(ValueError):
        render.prepare(np.zeros(shape, np.float32))                               # a constant volume has no range


@pytest.mark.parametrize('name', rd.OCCUPANCY_SCENES)
def test_occupancy_equals_the_integer_rule_and_hides_no_sample(gpu, name):
    s, q, table, maps = _inputs(name, gpu)
    want = rd.occupancy(s)
    assert (want == 0).any() and (want == 1).any()                                # not vacuous
    got = render.occupancy(q, table, maps, s['lo'] or None).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    top = rd.sample_sigma_by_brick(s)
    assert not ((got == 0) & (top > 0)).any()                                     # no empty brick holds a sample with sigma > 0


@pytest.mark.parametrize('name', sorted(rd.SCENES))
def test_image_matches_the_fp64_restatement(gpu, name):
    s = rd.scene(name)
    img64 = rd.references(name)[0]
    tol, own, tmin = rd.tolerance(name)
    got = _render(name, gpu)
    w, h = s['size']
    assert got.dtype == torch.float32 and tuple(got.shape) == (h, w, 4) and got.is_cuda
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - img64).max())
    print(f'{name}: kernel error {err:.3e}, float32 restatement {own:.3e}, tolerance {tol:.3e}, smallest T {tmin:.3e}')
    if name in rd.ZERO_SCENES:
        assert not bool(got.any())                                                # exactly 0, 0, 0, 0 everywhere
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize('name', sorted(rd.SCENES))
def test_grid_and_no_grid_give_the_same_bytes(gpu, name):
    with_grid, without = _render(name, gpu), _render(name, gpu, occupancy=None)
    assert torch.equal(with_grid, without)
    s, q, table, maps = _inputs(name, gpu)
    given = _render(name, gpu, occupancy=render.occupancy(q, table, maps, s['lo'] or None))
    assert torch.equal(with_grid, given)


def test_two_calls_agree_and_a_filled_buffer_is_replaced(gpu):
    for name in ('outside_c8', 'miss_c1', 'axis2_c3'):
        first = _render(name, gpu)
        w, h = rd.scene(name)['size']
        out = torch.full((h, w, 4), float('nan'), device=gpu)
        back = _render(name, gpu, out=out)
        assert back is out and torch.equal(first, out)
        assert torch.equal(first, _render(name, gpu))


def test_label_volume_through_maps_from_labels(gpu):
    """Labels on a coarser grid: the one-hot maps render like any other maps, and the labelled bodies show in their colours."""
    s = dict(rd.scene('oblique_c3'))
    idx = np.indices((8, 8, 8))
    labels = np.zeros((8, 8, 8), np.uint8)
    labels[(idx[0] < 4) & (idx[1] >= 2) & (idx[1] < 6) & (idx[2] >= 2) & (idx[2] < 6)] = 1
    labels[(idx[0] >= 5) & (idx[1] >= 3) & (idx[2] >= 3)] = 2
    maps = render.maps_from_labels(torch.as_tensor(labels).to(gpu))
    assert maps.is_cuda and tuple(maps.shape) == (2, 8, 8, 8)
    s.update(maps=maps.cpu().numpy(), lo=[64, 64], hi=[192, 192], colors=np.asarray(render.PALETTE[:2], np.float32),
             strengths=np.asarray([0.6, 0.6], np.float32), table=rd.table('zero'))
    img64, tmin = rd.reference(s, np.float64)
    img32, _ = rd.reference(s, np.float32)
    assert tmin < 2.0 ** -9                                                       # strong classes: rays reach the stop
    tol = 8 * float(np.abs(img32 - img64).max()) + rd.STOP
    q = render.prepare(torch.as_tensor(s['volume']).to(gpu))
    got = render.render(q, _camera(s), s['size'], table=s['table'], maps=maps, lo=64, hi=192, strengths=[0.6, 0.6], step=s['dt'],
                        shading=tuple(float(v) for v in s['shade']))
    assert img64[..., 3].max() > 0.9
    assert float(np.abs(got.cpu().numpy() - img64).max()) <= tol


def test_render_volume_end_to_end(gpu, tmp_path, capsys):
    """render_volume.py --data DIR --labels ntf_pred*.npy: the PNG's pixels are composite(render(...)) of the same arguments."""
    import render_volume
    vol = rd.volume((40, 24, 17), seed=5)
    np.save(tmp_path / 'volume.npy', vol.astype(np.float16))
    flipped = np.flip(vol.astype(np.float16).astype(np.float32), axis=-3).copy()
    pred = np.zeros((20, 12, 9), np.uint8)
    pred[4:12, 3:9, 2:7] = 1
    pred[13:18, 2:6, 4:8] = 3
    np.save(tmp_path / 'ntf_pred0.0annotated.npy', pred)
    argv = ['--data', str(tmp_path), '--labels', 'ntf_pred0.0annotated.npy', '--size', '96', '64', '--spacing', '1', '1', '2.5',
            '--azimuth', '40', '--elevation', '25', '--background', '0.1', '0.2', '0.3']
    with pytest.raises(SystemExit) as e:
        render_volume.main(argv)
    assert e.value.code == 0 and 'Rendering saved to' in capsys.readouterr().out
    got = rd.decode_png(tmp_path / 'render.png')
    cam = render.Camera.orbit(40, 25, shape=(40, 24, 17), spacing=(1, 1, 2.5), aspect=96 / 64)
    rgba = render.render(render.prepare(flipped), cam, (96, 64), spacing=(1, 1, 2.5), maps=render.maps_from_labels(pred, [1, 2, 3]),
                         lo=64, hi=192, step=0.5)
    want = render.composite(rgba, (0.1, 0.2, 0.3)).cpu().numpy()
    assert got.shape == (64, 96, 3) and np.array_equal(got, want)
    assert len({tuple(p) for p in want.reshape(-1, 3)}) > 50 and rgba[..., 3].max() > 0.5          # a picture, not a blank
    with pytest.raises(SystemExit) as e:
        render_volume.main(argv)                                                                    # no --overwrite
    assert e.value.code == 1
    with pytest.raises(SystemExit) as e:
        render_volume.main(argv + ['--turntable', '2', '--fov', '35', '--no-shading', '--output', str(tmp_path / 'turn.png')])
    assert e.value.code == 0
    a, b = rd.decode_png(tmp_path / 'turn_000.png'), rd.decode_png(tmp_path / 'turn_001.png')
    assert a.shape == b.shape == (64, 96, 3) and not np.array_equal(a, b)
    assert zlib.crc32(a.tobytes()) != zlib.crc32(got.tobytes())
