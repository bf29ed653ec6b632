"""CPU: the hand-crafted voxel features -- the C-ABI surface of vittf_voxel_feature_stats / vittf_voxel_features (declared,
exported, every refusal without a launch), the fp64 restatement of tests/voxel_features_data.py against the golden output of
the reference's own compose_features, the host-side checks of vt.voxel_features, the output tags and the refusals of
classify_features.py --features.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vit_tf_amd as vt
from vit_tf_amd import _lib
import voxel_features_data as vd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_voxel_feature_stats_workspace_bytes', 'vittf_voxel_feature_stats', 'vittf_voxel_features')


def _p(addr):
    return C.c_void_p(addr) if addr else None


def _stats(lib, shape=(8, 9, 10), vmax=1.0, vol=0x1000, stats=0x2000, ws=0x3000, ws_bytes=None):
    """vittf_voxel_feature_stats on placeholder addresses: only calls the argument checks refuse are made with it."""
    if ws_bytes is None:
        ws_bytes = lib.vittf_voxel_feature_stats_workspace_bytes(*shape) or 1 << 20
    return lib.vittf_voxel_feature_stats(_p(vol), *shape, vmax, _p(stats), _p(ws), ws_bytes, None)


def _compose(lib, shape=(8, 9, 10), vmax=1.0, channels=11, vol=0x1000, stats=0x2000, index=0, v0=0, n=100, out=0x4000, stride=None):
    return lib.vittf_voxel_features(_p(vol), *shape, vmax, _p(stats), channels, _p(index), v0, n, _p(out), n if stride is None else stride,
                                    None)


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    assert int(re.search(r'#define\s+VITTF_VOXFEAT_CHANNELS\s+(\d+)', header).group(1)) == 11 == _lib.VOXFEAT_CHANNELS == vt.voxel_features.CHANNELS
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    assert vt.voxel_features.classify and vt.voxel_features.compose and vt.voxel_features.sample and vt.voxel_features.stats


def test_workspace_query():
    lib = _lib.load()
    ws = lib.vittf_voxel_feature_stats_workspace_bytes
    assert ws(2, 2, 2) == 128 and ws(16, 32, 32) == 128 and ws(16, 32, 33) == 256      # 128 bytes per 16384 voxels
    assert ws(512, 512, 512) == 8192 * 128
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8), (2049, 8, 8), (8, 2049, 8), (8, 8, 2049), (2048, 2048, 512)):
        assert ws(*shape) == 0, shape
    assert ws(2048, 2048, 511) > 0                                                      # nvox = 2^31 - 2^22


def test_stats_entry_refuses_without_a_launch():
    lib = _lib.load()
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (2049, 8, 8), (8, 8, 2049), (2048, 2048, 512), (0, 8, 8), (-2, 8, 8)):
        assert _stats(lib, shape=shape) == INVALID, shape
    for vmax in (0.0, -1.0, float('inf'), float('nan')):
        assert _stats(lib, vmax=vmax) == INVALID, vmax
    for missing in ('vol', 'stats', 'ws'):
        assert _stats(lib, **{missing: 0}) == INVALID, missing
    for kw in (dict(vol=0x1002), dict(vol=0x1001), dict(stats=0x2004), dict(ws=0x3004), dict(ws=0x3001)):
        assert _stats(lib, **kw) == INVALID, kw
    assert _stats(lib, shape=(16, 32, 33), ws_bytes=255) == WORKSPACE
    assert _stats(lib, ws_bytes=0) == WORKSPACE


def test_compose_entry_refuses_without_a_launch():
    lib = _lib.load()
    nvox = 8 * 9 * 10
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (2049, 8, 8), (8, 8, 2049), (2048, 2048, 512)):
        assert _compose(lib, shape=shape, n=1) == INVALID, shape
    for vmax in (0.0, -1.0, float('inf'), float('nan')):
        assert _compose(lib, vmax=vmax) == INVALID, vmax
    for missing in ('vol', 'stats', 'out'):
        assert _compose(lib, **{missing: 0}) == INVALID, missing
    for kw in (dict(vol=0x1002), dict(stats=0x2004), dict(out=0x4001), dict(index=0x5004), dict(index=0x5001)):
        assert _compose(lib, **kw) == INVALID, kw
    for channels in (0, 2, 10, 12, 32, -1):
        assert _compose(lib, channels=channels) == INVALID, channels
    # ranges outside the volume, an empty call, a stride shorter than a row
    for kw in (dict(v0=-1), dict(v0=nvox, n=1), dict(v0=nvox - 99, n=100), dict(v0=0, n=nvox + 1), dict(n=0), dict(n=-5),
               dict(n=100, stride=99), dict(v0=1 << 40, n=1), dict(index=0x5000, n=0), dict(index=0x5000, n=1 << 31),
               dict(index=0x5000, n=100, stride=64)):
        assert _compose(lib, **kw) == INVALID, kw


def test_restatement_agrees_with_the_reference_golden(golden_dir):
    """The fp64 restatement of tests/voxel_features_data.py against the fp32 output of the reference's compose_features, inside
    the fp32 term of the bound alone (measured: 0.063 of it)."""
    path = os.path.join(golden_dir, 'voxel_features.npz')
    assert os.path.getsize(path) < 256 * 1024
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ['ct_features', 'ct_volume', 'uniform_features', 'uniform_volume']
        for content, shape in (('uniform', (12, 10, 14)), ('ct', (9, 17, 5))):
            vol, gold = z[f'{content}_volume'], z[f'{content}_features']
            assert vol.dtype == np.float32 and vol.shape == shape and gold.dtype == np.float32 and gold.shape == (11,) + shape
            assert np.array_equal(vol, vd.uniform_volume(shape) if content == 'uniform' else vd.ct_volume(shape))
            ref = vd.reference(vol)
            ratio = np.abs(gold.reshape(11, -1).astype(np.float64) - ref['want']) / vd.fp32_term(ref)
            print(f'{content} {shape}: restatement vs golden, largest |diff| / fp32 term per channel {ratio.max(1).round(3).tolist()}')
            assert ratio.max() <= 1.0
            # the two paddings are told apart: at a border voxel the zero-padded and the replicated neighbour differ
            raw = ref['raw']
            assert raw[2][-1].tolist() == raw[0][-1].tolist() and raw[5][0].tolist() == raw[0][0].tolist()
            gx_border = 0.5 * (0.0 - raw[0][-2])
            assert np.all(np.abs(raw[1][-1]) >= np.abs(gx_border) - 1e-12)


def test_restatement_basics():
    ref = vd.cached_reference((5, 7, 9), 'ct')
    assert np.allclose(ref['want'].mean(1), 0, atol=1e-12) and np.allclose(ref['want'].std(1, ddof=1), 1, atol=1e-12)
    n = np.asarray([5.0, 7.0, 9.0])
    nvox = 5 * 7 * 9
    assert np.allclose(ref['mean'][8:], -0.5 / n, atol=1e-15)
    assert np.allclose(ref['std'][8:], np.sqrt((n * n - 1) / (12 * n * n) * nvox / (nvox - 1)), rtol=1e-13)
    assert vd.ulp16(1.0) == 2.0 ** -10 and vd.ulp16(0.0) == 2.0 ** -24 and vd.ulp16(-3.9) == 2.0 ** -9
    assert vd.border_mask((2, 2, 2)).all() and vd.border_mask((5, 7, 9)).sum() == nvox - 3 * 5 * 7


def test_host_side_checks_need_no_device():
    vf = vt.voxel_features
    assert vf.check_shape((2, 2048, 3)) == (2, 2048, 3)
    for shape in ((1, 4, 4), (4, 4), (4, 4, 2049), (2048, 2048, 512), (2, 3, 4, 5)):
        with pytest.raises(ValueError):
            vf.check_shape(shape)
    assert vf.linear_index([[0, 0, 0], [1, 2, 3], [4, 6, 8]], (5, 7, 9)).tolist() == [0, vd.linear((5, 7, 9), 1, 2, 3), 5 * 7 * 9 - 1]
    for bad in ([[5, 0, 0]], [[0, -1, 0]], [[0, 0, 9]], [[0.5, 0, 0]]):
        with pytest.raises(ValueError):
            vf.linear_index(bad, (5, 7, 9))
    st = vf.VoxelStats(1.0, np.zeros(11), np.ones(11))
    vf._check_stats(st, 11)
    for broken in (vf.VoxelStats(0.0, np.zeros(11), np.ones(11)), vf.VoxelStats(float('nan'), np.zeros(11), np.ones(11)),
                   vf.VoxelStats(1.0, np.zeros(11), np.concatenate([np.ones(10), [0.0]])),
                   vf.VoxelStats(1.0, np.full(11, np.inf), np.ones(11)), vf.VoxelStats(1.0, np.zeros(11), np.full(11, np.nan))):
        with pytest.raises(ValueError):
            vf._check_stats(broken, 11)
    vf._check_stats(vf.VoxelStats(1.0, np.zeros(11), np.concatenate([np.ones(10), [0.0]])), 1)      # channel 0 alone is fine


def test_tags():
    import classify_features as cf
    assert cf.svm_tag(200.0, 'both', 'rbf', features='handcrafted') == '200.0both_hand_rbf'
    assert cf.svm_tag(200.0, 'both', 'linear', False, False, 'intensity') == '200.0both_intensity_linear_nobg'
    assert cf.forest_tag(200.0, 'both', 256, features='intensity') == '200.0both_intensity_rf256'
    assert cf.forest_tag(40.0, 'uniform', 8, 3, 'all', False, 'handcrafted') == '40.0uniform_hand_rf8_d3_all_nobg'
    assert cf.output_paths('d', cf.svm_tag(200.0, 'both', 'rbf', features='handcrafted'))[0].name == 'svm_pred200.0both_hand_rbf.npy'
    assert cf.forest_paths('d', cf.forest_tag(200.0, 'both', 256, features='intensity'))[0].name == 'rf_pred200.0both_intensity_rf256.npy'
    # the default-feature tags, character for character what they were
    assert cf.svm_tag(40.0, 'uniform', 'rbf') == cf.svm_tag(40.0, 'uniform', 'rbf', features='dino') == '40.0uniform_rbf'
    assert cf.svm_tag(0.0, 'annotated', 'linear', True, False) == '0.0annotated_linear_norm_nobg'
    assert cf.forest_tag(40.0, 'uniform', 256) == cf.forest_tag(40.0, 'uniform', 256, features='dino') == '40.0uniform_rf256'
    assert cf.forest_tag(0.0, 'annotated', 64, 12, 'all', False) == '0.0annotated_rf64_d12_all_nobg'
    assert cf.forest_tag(5.0, 'both', 8, None, 20) == '5.0both_rf8_mf20'


def _refused(argv, capsys, monkeypatch):
    import classify_features
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('the device was asked for'))
    with pytest.raises(SystemExit) as e:
        classify_features.main(argv)
    assert e.value.code == 1
    return capsys.readouterr().out


@pytest.mark.parametrize('features', ['handcrafted', 'intensity'])
@pytest.mark.parametrize('classifier', ['svm', 'forest'])
def test_command_line_refuses_normalize(tmp_path, capsys, monkeypatch, features, classifier):
    out = _refused(['--data', str(tmp_path), '--features', features, '--classifier', classifier, '--normalize'], capsys, monkeypatch)
    assert 'Invalid argument for --normalize' in out


def test_command_line_refuses_a_model_of_another_width(tmp_path, capsys, monkeypatch):
    import forest_data as fd
    import svm_data
    x, y = fd.blobs(120, 64, 3, 1.0, 3)
    vt.forest.save_model(vt.forest.fit(x, y, trees=2, max_depth=2), tmp_path / 'rf64.npz')
    out = _refused(['--data', str(tmp_path), '--features', 'handcrafted', '--model', str(tmp_path / 'rf64.npz')], capsys, monkeypatch)
    assert 'Invalid argument for --model' in out and 'F = 64' in out
    xs, ts, gamma = svm_data.planted(64, 2, 10, 0)
    vt.svm.save_model(vt.svm.fit(xs, ts, gamma=gamma), tmp_path / 'svm64.npz')
    out = _refused(['--data', str(tmp_path), '--features', 'intensity', '--model', str(tmp_path / 'svm64.npz')], capsys, monkeypatch)
    assert 'Invalid argument for --model' in out and 'F = 64' in out


@pytest.mark.parametrize('shape', [(1, 8, 8), (8, 8, 1)])
def test_command_line_refuses_a_flat_volume(tmp_path, capsys, monkeypatch, shape):
    np.save(tmp_path / 'volume.npy', np.random.default_rng(0).random(shape).astype(np.float16))
    np.save(tmp_path / 'labels.npy', (np.arange(int(np.prod(shape))) % 3).astype(np.uint8).reshape(shape))
    out = _refused(['--data', str(tmp_path), '--features', 'handcrafted', '--num-samples', '5'], capsys, monkeypatch)
    assert 'Invalid argument for --features' in out and '2..2048' in out
