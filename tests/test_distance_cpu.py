"""CPU: Euclidean distance transform and surface scores -- the C-ABI surface of vittf_edt_workspace_bytes / vittf_edt_sq /
vittf_edt_sq_weighted (declared, exported, every argument error without a launch), the restatement the GPU tests compare
against (tests/distance_data.py) checked against closed forms, the host arithmetic of vit_tf_amd.distance, and the command line
of score_labels.py.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import distance_data as dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_edt_workspace_bytes', 'vittf_edt_sq', 'vittf_edt_sq_weighted')
dist = vt.distance


def _p(on, addr=0x1000):
    return C.c_void_p(addr) if on else None


def _edt(lib, shape=(8, 8, 8), value=-1, mode=0, src=1, d2=1, site=1, ws=1, ws_bytes=1 << 40, d2_addr=0x1000, site_addr=0x1000,
         ws_addr=0x1000, w2=None):
    """vittf_edt_sq (w2 None) or vittf_edt_sq_weighted on placeholder addresses: only calls the argument checks refuse are
    made with it (nothing is launched, nothing is dereferenced on the device)."""
    if w2 is None:
        return lib.vittf_edt_sq(_p(src, 0x1001), *shape, value, mode, _p(d2, d2_addr), _p(site, site_addr), _p(ws, ws_addr),
                                ws_bytes, None)
    w = None if w2 == 'null' else (C.c_double * 3)(*w2)
    return lib.vittf_edt_sq_weighted(_p(src, 0x1001), *shape, value, mode, w, _p(d2, d2_addr), _p(site, site_addr),
                                     _p(ws, ws_addr), ws_bytes, None)


# ---------------------------------------------------------------------------- 1. ABI surface
def test_edt_entries_are_declared_exported_and_the_abi_stays_6():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    assert int(re.search(r'#define\s+VITTF_EDT_MAX_DIM\s+(\d+)', header).group(1)) == _lib.EDT_MAX_DIM == vt.distance.MAX_DIM == 2048
    assert int(re.search(r'#define\s+VITTF_EDT_NO_SITE\s+(\d+)', header).group(1)) == _lib.EDT_NO_SITE == 2 ** 31 - 1
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    assert vt.distance is not None and 'distance' in dir(vt)


@pytest.mark.parametrize('w2', [None, (1.0, 4.0, 0.25)], ids=['integer', 'weighted'])
def test_edt_argument_errors_return_invalid_without_a_launch(w2):
    lib = _lib.load()
    for missing in ('src', 'd2', 'ws'):
        assert _edt(lib, w2=w2, **{missing: 0}) == INVALID, missing
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (2049, 8, 8), (8, 2049, 8), (8, 8, 2049), (2 ** 31 - 1, 1, 1)):
        assert _edt(lib, shape=shape, w2=w2) == INVALID, shape
        assert lib.vittf_edt_workspace_bytes(*shape) == 0
    for shape in ((2048, 2048, 512), (2048, 1024, 1024), (2048, 2048, 2048)):         # 2^31 voxels and more
        assert _edt(lib, shape=shape, w2=w2) == INVALID, shape
        assert lib.vittf_edt_workspace_bytes(*shape) == 0
    for value in (-2, 256, 1000):
        assert _edt(lib, value=value, w2=w2) == INVALID, value
    for mode in (-1, 2, 7):
        assert _edt(lib, mode=mode, w2=w2) == INVALID, mode
    for addr in (0x1001, 0x1002):
        assert _edt(lib, d2_addr=addr, w2=w2) == INVALID and _edt(lib, site_addr=addr, w2=w2) == INVALID, addr
    assert _edt(lib, ws_addr=0x1004, w2=w2) == INVALID                                # the fp64 part is 8-byte aligned
    # the workspace status, after the arguments
    need = lib.vittf_edt_workspace_bytes(8, 8, 8)
    assert _edt(lib, ws_bytes=need - 1, w2=w2) == WORKSPACE and _edt(lib, ws_bytes=0, w2=w2) == WORKSPACE
    assert _edt(lib, ws_bytes=0, mode=2, w2=w2) == INVALID
    assert _edt(lib, shape=(2048, 2047, 512), ws_bytes=1 << 20, w2=w2) == WORKSPACE     # just under 2^31 voxels is a volume


def test_weighted_entry_refuses_bad_weights():
    lib = _lib.load()
    assert _edt(lib, w2='null') == INVALID
    for bad in (0.0, -1.0, float('inf'), float('nan'), -float('inf')):
        for axis in range(3):
            w2 = [1.0, 2.0, 3.0]
            w2[axis] = bad
            assert _edt(lib, w2=w2) == INVALID, (bad, axis)
    assert _edt(lib, w2=(1e-300, 1.0, 1e300), ws_bytes=0) == WORKSPACE                  # finite and positive: accepted


def test_workspace_grows_with_the_volume():
    lib = _lib.load()
    sizes = [lib.vittf_edt_workspace_bytes(*s) for s in ((1, 1, 1), (3, 5, 7), (2, 3, 2048), (64, 64, 64), (512, 512, 512))]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and sizes[0] > 0
    for shape in ((1, 1, 1), (3, 5, 7), (64, 64, 64), (2048, 2047, 512)):
        nvox = shape[0] * shape[1] * shape[2]
        assert lib.vittf_edt_workspace_bytes(*shape) == (8 * nvox + 255) // 256 * 256 + (4 * nvox + 255) // 256 * 256


def test_python_entries_refuse_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a refused call reached the device')

    monkeypatch.setattr(_lib, 'require_device', boom)
    d = dist
    vol = np.zeros((3, 4, 5), np.uint8)
    for bad in (vol.astype(np.int32), vol.astype(bool), np.zeros((4, 5), np.uint8), np.zeros((0, 4, 5), np.uint8),
                np.zeros((1, 1, 2049), np.uint8)):
        with pytest.raises(ValueError):
            d.edt(bad)
        with pytest.raises(ValueError):
            d.surface(bad)
    for value in (-2, 256, 1.5, None, True):
        with pytest.raises(ValueError):
            d.edt(vol, value=value)
        with pytest.raises(ValueError):
            d.signed(vol, value)
    for spacing in ((1, 2), (1, 2, 0), (1, -1, 1), (1, float('inf'), 1), (1, float('nan'), 1), 'abc', 3.0):
        with pytest.raises(ValueError):
            d.edt(vol, spacing=spacing)
        with pytest.raises(ValueError):
            d.surface_scores(vol, vol, [1], spacing=spacing)
    with pytest.raises(ValueError):
        d.surface(vol, connectivity=4)
    with pytest.raises(ValueError):
        d.surface_distances(vol, np.zeros((3, 4, 6), np.uint8), 1)
    with pytest.raises(ValueError):
        d.surface_scores(vol, vol, [1], tolerance=-1.0)


# ---------------------------------------------------------------------------- 2. the restatement against closed forms
def test_single_corner_site_is_the_sum_of_squares():
    for shape in ((5, 7, 67), (3, 130, 9), (40, 1, 33)):
        i, j, k = np.indices(shape)
        assert np.array_equal(dd.want_int(shape, 'corner'), i * i + j * j + k * k)
        assert np.array_equal(dd.want_brute(shape, 'corner'), (i * i + j * j + k * k).astype(np.float64))
        sp = (0.7, 0.7, 2.5)
        want = 0.7 ** 2 * i * i + 0.7 ** 2 * j * j + 2.5 ** 2 * k * k
        assert np.allclose(dd.want_brute(shape, 'corner', sp), want, rtol=1e-15, atol=0)


def test_brute_force_equals_scipy_with_and_without_sampling():
    for shape in ((5, 7, 67), (3, 130, 9), (1, 1, 300)):
        for name in dd.MASKS:
            s = dd.sites(shape, name)
            assert s.any()
            assert np.array_equal(dd.want_brute(shape, name), dd.want_int(shape, name).astype(np.float64)), (shape, name)
            for sp in dd.SPACINGS:
                got, ref = dd.want_brute(shape, name, sp), dd.scipy_d2(s, sp)
                assert np.allclose(got, ref, rtol=1e-12, atol=0), (shape, name, sp)
    none = np.zeros((3, 4, 5), bool)
    assert dd.scipy_d2(none) is None and np.isinf(dd.brute_d2(none)).all()


def test_volumes_encode_their_sites_under_every_rule():
    for value, mode in dd.RULES:
        for name in ('three', 'half', 'all'):
            vol = dd.volume((5, 7, 67), name, value, mode)
            assert vol.dtype == np.uint8
            assert np.array_equal(dd.is_site(vol, value, mode), dd.sites((5, 7, 67), name)), (value, mode, name)


def test_scores_on_hand_made_distance_sets():
    a, b = [0.0, 1.0, 2.0, 3.0], [1.0, 1.0, 5.0, 0.5, 0.5, 0.0]
    for f in (dd.scores_from_sets, vt.distance.scores_from_distances):
        r = f(a, b, tolerance=1.0)
        assert r['hd'] == 5.0
        assert r['assd'] == pytest.approx((6.0 / 4 + 8.0 / 6) / 2, rel=1e-15)
        assert r['nsd'] == pytest.approx(7 / 10, rel=1e-15)                      # 0, 1 | 1, 1, .5, .5, 0
        # sorted: 0 0 .5 .5 1 1 1 2 3 5; rank 0.95 * 9 = 8.55 -> 3 + 0.55 * 2
        assert r['hd95'] == pytest.approx(4.1, rel=1e-14)
        assert r['hd95'] == pytest.approx(float(np.percentile(np.array(a + b), 95)), rel=1e-15)
        assert (r['n_surface_target'], r['n_surface_pred']) == (4, 6)
        assert f(a, b, tolerance=0.0)['nsd'] == pytest.approx(2 / 10)
        one = f([2.5], [2.5])
        assert one['hd'] == one['hd95'] == one['assd'] == 2.5 and one['nsd'] == 0.0
    rng = np.random.default_rng(5)
    for n in (1, 2, 19, 20, 21, 1000):
        v = rng.random(n) * 10
        assert dd.percentile(v, 95) == pytest.approx(float(np.percentile(v, 95)), rel=1e-14)


def test_absent_class_rule():
    for f in (dd.scores_from_sets, vt.distance.scores_from_distances):
        both = f([], [])
        assert np.isnan(both['hd']) and np.isnan(both['hd95']) and np.isnan(both['assd']) and both['nsd'] == 1.0
        assert (both['n_surface_target'], both['n_surface_pred']) == (0, 0)
        for r in (f([], [np.inf, np.inf]), f([np.inf], [])):
            assert r['hd'] == np.inf and r['hd95'] == np.inf and r['assd'] == np.inf and r['nsd'] == 0.0
    # through the volumes: class 2 only in the target, class 3 in neither
    t = dd.ball((12, 12, 12), (5, 5, 5), 3)
    t[10, 10, 10] = 2
    p = dd.ball((12, 12, 12), (5, 6, 5), 3)
    s = dd.surface_scores(t, p, [1, 2, 3])
    assert np.isfinite(s['hd'][0]) and s['hd'][1] == np.inf and np.isnan(s['hd'][2])
    assert s['nsd'][1] == 0.0 and s['nsd'][2] == 1.0 and s['n_surface_target'].tolist()[1:] == [1, 0]


def test_restated_surface_counts_border_voxels():
    full = np.ones((4, 5, 6), bool)
    inner = np.zeros_like(full)
    inner[1:-1, 1:-1, 1:-1] = True
    assert np.array_equal(dd.surface(full), ~inner)                                 # the volume's border is surface
    box = np.zeros((9, 9, 9), bool)
    box[2:7, 2:7, 2:7] = True
    assert dd.surface(box).sum() == 5 ** 3 - 3 ** 3
    shifted = np.roll(box, 1, axis=0)
    d = dd.directed(dd.surface(box), dd.surface(shifted))
    assert d.max() == 1.0 and d.min() == 0.0


# ---------------------------------------------------------------------------- 3. command line
def _main(argv):
    import score_labels
    with pytest.raises(SystemExit) as e:
        score_labels.main(argv)
    return e.value.code


def test_score_labels_cli_refusals_and_output_name(tmp_path, monkeypatch, capsys):
    """Every exit-1 case with its message, all before anything touches the device; the default output name."""
    import score_labels

    def boom(*a, **k):
        raise AssertionError('a refused command line reached the GPU entry')

    monkeypatch.setattr(vt.distance, 'surface_scores', boom)
    monkeypatch.setattr(_lib, 'require_device', boom)
    assert score_labels.default_output(tmp_path / 'ntf_pred16.0uniform.npy') == tmp_path / 'ntf_pred16.0uniform_surface.json'
    assert score_labels.default_output('v_clusters4_islands.npy').name == 'v_clusters4_islands_surface.json'
    assert score_labels.grid_spacing(None, (4, 4, 4), (8, 8, 8)) is None
    assert score_labels.grid_spacing((1.0, 2.0, 3.0), (4, 6, 8), (8, 6, 2)) == [0.5, 2.0, 12.0]
    tgt, prd = tmp_path / 'labels.npy', tmp_path / 'x_pred.npy'
    np.save(tgt, np.zeros((3, 4, 5), np.uint8))
    np.save(prd, np.zeros((3, 4, 5), np.uint8))
    out = lambda: capsys.readouterr().out                     # noqa: E731
    out()
    with pytest.raises(SystemExit) as e:
        score_labels.main(['--target', str(tgt)])                                  # --pred is required
    assert e.value.code == 2
    capsys.readouterr()
    for bad in ('-1', '256'):
        assert _main(['--target', str(tgt), '--pred', str(prd), '--classes', '1', bad]) == 1
        assert f'Invalid argument for --classes: {bad} is outside 0..255' in out()
    for bad in (['0', '1', '1'], ['1', '-2', '1'], ['1', '1', 'inf'], ['nan', '1', '1']):
        assert _main(['--target', str(tgt), '--pred', str(prd), '--spacing', *bad]) == 1
        assert 'Invalid argument for --spacing' in out()
    for bad in ('-0.5', 'nan', 'inf'):
        assert _main(['--target', str(tgt), '--pred', str(prd), '--tolerance', bad]) == 1
        assert 'Invalid argument for --tolerance' in out()
    assert _main(['--target', str(tmp_path / 'nope.npy'), '--pred', str(prd)]) == 1
    assert 'Invalid argument for --target (File does not exist)' in out()
    assert _main(['--target', str(tgt), '--pred', str(tmp_path / 'nope.npy')]) == 1
    assert 'Invalid argument for --pred (File does not exist)' in out()
    np.save(tmp_path / 'i32.npy', np.zeros((3, 4, 5), np.int32))
    np.save(tmp_path / 'flat.npy', np.zeros((4, 5), np.uint8))
    np.save(tmp_path / 'dict.npy', {'k': np.zeros((3, 4, 5), np.uint8)}, allow_pickle=True)
    (tmp_path / 'broken.npy').write_bytes(b'not an array')
    for bad in ('i32.npy', 'flat.npy', 'dict.npy', 'broken.npy'):
        assert _main(['--target', str(tgt), '--pred', str(tmp_path / bad)]) == 1, bad
        assert 'Invalid argument for --pred' in out(), bad
        assert _main(['--target', str(tmp_path / bad), '--pred', str(prd)]) == 1, bad
        assert 'Invalid argument for --target' in out(), bad
    (tmp_path / 'x_pred_surface.json').write_text('{}')
    assert _main(['--target', str(tgt), '--pred', str(prd)]) == 1
    assert 'Cache file already exists' in out()
    assert (tmp_path / 'x_pred_surface.json').read_text() == '{}'                      # untouched
    assert _main(['--target', str(tgt), '--pred', str(prd), '--output', str(tmp_path / 'missing_dir' / 's.json')]) == 1
    assert 'Invalid argument for --output (Cannot write to location)' in out()


def test_score_labels_cli_writes_the_scores(tmp_path, monkeypatch, capsys):
    """The accepted command line with the GPU functions replaced: the file name, the keys, the classes and the spacing that
    reach surface_scores, --overwrite."""
    import score_labels
    calls = []

    def fake_scores(target, pred, classes=None, spacing=None, tolerance=1.0):
        calls.append((tuple(np.asarray(target).shape), tuple(pred.shape), list(classes), spacing, tolerance))
        return dd.surface_scores(np.asarray(target), np.asarray(pred), classes, spacing, tolerance)

    def fake_resize(vol, out_shape):
        idx = [np.minimum((np.arange(o) * (n / o)).astype(np.int64), n - 1) for n, o in zip(vol.shape, out_shape)]
        return vol[np.ix_(*idx)]

    monkeypatch.setattr(vt.distance, 'surface_scores', fake_scores)
    monkeypatch.setattr(vt.scores, 'resize_nearest_u8', fake_resize)
    monkeypatch.setattr(score_labels, 'overlap_scores', lambda t, p: {'accuracy': float((t == p).mean())})
    t = dd.ball((16, 16, 16), (7, 7, 7), 5)
    dd.ball((16, 16, 16), (3, 12, 12), 2, value=2, into=t)
    p = dd.ball((8, 8, 8), (3, 4, 3), 2)
    tgt, prd = tmp_path / 'labels.npy', tmp_path / 'ntf_pred0.0annotated.npy'
    np.save(tgt, t)
    np.save(prd, p)
    assert _main(['--target', str(tgt), '--pred', str(prd), '--spacing', '1', '1', '2.5', '--tolerance', '2']) == 0
    assert calls == [((8, 8, 8), (8, 8, 8), [1, 2], [2.0, 2.0, 5.0], 2.0)]
    got = json.load(open(tmp_path / 'ntf_pred0.0annotated_surface.json'))
    assert set(got) == {'classes', *vt.distance.SCORE_KEYS, 'overlap', 'spacing', 'tolerance', 'grid', 'target_grid', 'time'}
    assert got['classes'] == [1, 2] and got['grid'] == [8, 8, 8] and got['target_grid'] == [16, 16, 16]
    assert got['spacing'] == [2.0, 2.0, 5.0] and got['tolerance'] == 2.0 and got['time'] >= 0
    assert all(len(got[k]) == 2 for k in vt.distance.SCORE_KEYS)
    assert np.isfinite(got['hd'][0]) and got['hd'][1] == np.inf and got['nsd'][1] == 0.0     # class 2 is not predicted
    assert 'Surface scores saved to' in capsys.readouterr().out
    assert _main(['--target', str(tgt), '--pred', str(prd)]) == 1                              # no --overwrite
    assert _main(['--target', str(tgt), '--pred', str(prd), '--classes', '1', '--overwrite']) == 0
    assert calls[-1] == ((8, 8, 8), (8, 8, 8), [1], None, 1.0)
    assert json.load(open(tmp_path / 'ntf_pred0.0annotated_surface.json'))['spacing'] is None
