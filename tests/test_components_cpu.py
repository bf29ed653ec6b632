"""CPU: connected components -- the C-ABI surface of vittf_label_components / vittf_component_sizes / vittf_filter_components
(declared, exported, argument checks without a launch), the host side of vit_tf_amd.components (refusals before the device,
the ordering of `table`, the cut-off of `relabel`), every refusal of label_islands.py and the output tag of predict_ntf.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_components_workspace_bytes', 'vittf_label_components', 'vittf_component_sizes', 'vittf_filter_components')
cc = vt.components


def _p(on, addr=0x1000):
    return C.c_void_p(addr) if on else None


def _label(lib, shape=(8, 8, 8), select=-1, connectivity=1, src=1, labels=1, ws=1, ws_bytes=1 << 40, labels_addr=0x1000,
           ws_addr=0x1000):
    """vittf_label_components on placeholder addresses: only calls the argument checks refuse are made with it."""
    return lib.vittf_label_components(_p(src, 0x1001), *shape, select, connectivity, _p(labels, labels_addr), _p(ws, ws_addr),
                                      ws_bytes, None)


def _sizes(lib, nvox=512, labels=1, sizes=1, labels_addr=0x1000, sizes_addr=0x1000):
    return lib.vittf_component_sizes(_p(labels, labels_addr), nvox, _p(sizes, sizes_addr), None)


def _filter(lib, nvox=512, src=1, labels=1, sizes=1, dst=1, min_size=1, keep_label=0, fill=0, labels_addr=0x1000,
            sizes_addr=0x1000):
    return lib.vittf_filter_components(_p(src, 0x1001), _p(labels, labels_addr), _p(sizes, sizes_addr), nvox, min_size, keep_label,
                                       fill, _p(dst, 0x1003), None)


def test_component_entries_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    tile = tuple(int(re.search(r'#define\s+VITTF_CC_TILE%d\s+(\d+)' % i, header).group(1)) for i in range(3))
    assert tile == _lib.CC_TILE == cc.TILE
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    # vittf_label_components
    for missing in ('src', 'labels', 'ws'):
        assert _label(lib, **{missing: 0}) == INVALID, missing
    for addr in (0x1001, 0x1002):
        assert _label(lib, labels_addr=addr) == INVALID and _label(lib, ws_addr=addr) == INVALID, addr
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)):
        assert _label(lib, shape=shape) == INVALID, shape
        assert lib.vittf_components_workspace_bytes(*shape) == 0
    big = (2 ** 31 - 1, 1, 1)                                 # one voxel more than a label can number
    for shape in (big, big[::-1], (2048, 2048, 512), (65536, 65536, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert _label(lib, shape=shape) == INVALID, shape
        assert lib.vittf_components_workspace_bytes(*shape) == 0
    for select in (-3, 256):
        assert _label(lib, select=select) == INVALID, select
    for connectivity in (0, 4, -1):
        assert _label(lib, connectivity=connectivity) == INVALID, connectivity
    for shape in ((1, 1, 1), (3, 5, 7), (64, 64, 64), (2 ** 31 - 2, 1, 1), (1, 1, 2 ** 31 - 2)):
        nvox = shape[0] * shape[1] * shape[2]
        need = lib.vittf_components_workspace_bytes(*shape)
        assert need == (4 * nvox + 255) // 256 * 256
        assert _label(lib, shape=shape, ws_bytes=need - 1) == WORKSPACE, shape
    assert _label(lib, ws_bytes=0) == WORKSPACE
    assert _label(lib, ws_bytes=0, connectivity=4) == INVALID         # a bad argument is reported before the workspace
    # vittf_component_sizes
    for missing in ('labels', 'sizes'):
        assert _sizes(lib, **{missing: 0}) == INVALID, missing
    assert _sizes(lib, labels_addr=0x1002) == INVALID and _sizes(lib, sizes_addr=0x1001) == INVALID
    for nvox in (0, -1, 2 ** 31 - 1):
        assert _sizes(lib, nvox=nvox) == INVALID, nvox
    # vittf_filter_components
    for missing in ('src', 'labels', 'dst'):
        assert _filter(lib, **{missing: 0}) == INVALID, missing
    assert _filter(lib, sizes=0, keep_label=0) == INVALID            # sizes may be NULL only with a keep_label
    assert _filter(lib, labels_addr=0x1002, keep_label=1) == INVALID and _filter(lib, sizes_addr=0x1002) == INVALID
    for fill in (256, -1):
        assert _filter(lib, fill=fill) == INVALID, fill
    assert _filter(lib, keep_label=-1) == INVALID
    for nvox in (0, 2 ** 31 - 1):
        assert _filter(lib, nvox=nvox) == INVALID, nvox


def test_python_entries_refuse_before_the_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a refused call reached the device')

    monkeypatch.setattr(_lib, 'require_device', boom)
    vol = np.zeros((3, 4, 5), np.uint8)
    for bad in (vol.astype(np.int32), vol.astype(bool), vol.astype(np.float32), torch.zeros(3, 4, 5, dtype=torch.int8)):
        with pytest.raises(ValueError):
            cc.label(bad)
    for bad in (np.zeros((4, 5), np.uint8), np.zeros((1, 3, 4, 5), np.uint8), np.zeros((0, 4, 5), np.uint8)):
        with pytest.raises(ValueError):
            cc.label(bad)
    for select in (-3, 256, 1.5, None, True):
        with pytest.raises(ValueError):
            cc.label(vol, select=select)
    for connectivity in (0, 4, 1.5, None):
        with pytest.raises(ValueError):
            cc.label(vol, connectivity=connectivity)
        with pytest.raises(ValueError):
            cc.largest_island(vol, 3, connectivity=connectivity)
        with pytest.raises(ValueError):
            cc.remove_small(vol, 2, connectivity=connectivity)
    with pytest.raises(ValueError):
        cc.remove_small(vol, 2, fill=256)
    with pytest.raises(ValueError):
        cc.sizes(np.zeros((3, 4, 5), np.int64))
    with pytest.raises(ValueError):
        cc.relabel(torch.zeros((2, 2, 2), dtype=torch.int32), [1], max_islands=256)
    with pytest.raises(ValueError):
        cc.relabel(torch.zeros((2, 2, 2), dtype=torch.int32), [1], max_islands=0)


def test_table_orders_by_count_then_id_on_cpu_tensors():
    sizes = torch.tensor([0, 3, 5, 0, 3, 5, 1, 0, 5], dtype=torch.int32)        # labels 2..9; counts 5 three times, 3 twice
    ids, counts = cc.table_from_sizes(sizes)
    assert ids.tolist() == [3, 6, 9, 2, 5, 7] and counts.tolist() == [5, 5, 5, 3, 3, 1]
    assert ids.dtype == torch.int64 and counts.dtype == torch.int64 and not ids.is_cuda
    ids, counts = cc.table_from_sizes(torch.zeros(7, dtype=torch.int32))         # no component at all
    assert ids.numel() == 0 and counts.numel() == 0
    rng = np.random.default_rng(0)
    s = rng.integers(0, 4, size=1000).astype(np.int32)                           # many ties
    ids, counts = cc.table_from_sizes(torch.from_numpy(s))
    order = np.lexsort((np.arange(1000), -s.astype(np.int64)))
    order = order[s[order] > 0]
    assert np.array_equal(ids.numpy(), order + 1) and np.array_equal(counts.numpy(), s[order])


def test_relabel_cuts_off_at_max_islands():
    lab = torch.tensor([[[0, 1, 1], [4, 4, 4]], [[7, 0, 1], [9, 9, 0]]], dtype=torch.int32)
    ids = [4, 1, 9, 7]                                                           # by descending size, ties by id
    out = cc.relabel(lab, ids)
    assert out.dtype == torch.uint8 and out.shape == lab.shape
    assert out.tolist() == [[[0, 2, 2], [1, 1, 1]], [[4, 0, 2], [3, 3, 0]]]
    assert cc.relabel(lab, ids, max_islands=3).tolist() == [[[0, 2, 2], [1, 1, 1]], [[0, 0, 2], [3, 3, 0]]]
    assert cc.relabel(lab, torch.tensor(ids), max_islands=1).tolist() == [[[0, 0, 0], [1, 1, 1]], [[0, 0, 0], [0, 0, 0]]]
    # more than 255 islands: the 256th and later become background
    many = torch.arange(1, 301, dtype=torch.int32).reshape(3, 10, 10)
    out = cc.relabel(many, torch.arange(1, 301))
    assert out.reshape(-1)[:255].tolist() == list(range(1, 256)) and int(out.reshape(-1)[255:].max()) == 0


# ---------------------------------------------------------------------------- command line
def _main(argv):
    import label_islands
    with pytest.raises(SystemExit) as e:
        label_islands.main(argv)
    return e.value.code


def test_label_islands_cli_refusals(tmp_path, monkeypatch, capsys):
    """Every exit-1 case, each with its message, all before anything touches the device (label would raise)."""
    def boom(*a, **k):
        raise AssertionError('a refused command line reached the GPU entry')

    monkeypatch.setattr(cc, 'label', boom)
    monkeypatch.setattr(_lib, 'require_device', boom)
    src = tmp_path / 'v_clusters4.npy'
    np.save(src, np.zeros((3, 4, 5), np.uint8))
    out = lambda: capsys.readouterr().out                     # noqa: E731
    out()
    for bad in ('-1', '256'):
        assert _main(['--labels', str(src), '--value', bad]) == 1
        assert f'Invalid argument for --value: {bad} is outside 0..255' in out()
    assert _main(['--labels', str(src), '--value', '2', '--each-value']) == 1
    assert 'Invalid argument for --each-value' in out()
    for bad in ('0', '-5'):
        assert _main(['--labels', str(src), '--min-size', bad]) == 1
        assert f'Invalid argument for --min-size: {bad} is below 1' in out()
    for bad in ('0', '256'):
        assert _main(['--labels', str(src), '--max-islands', bad]) == 1
        assert f'Invalid argument for --max-islands: {bad} is outside 1..255' in out()
    assert _main(['--labels', str(tmp_path / 'nope.npy')]) == 1
    assert 'Invalid argument for --labels (File does not exist)' in out()
    np.save(tmp_path / 'i32.npy', np.zeros((3, 4, 5), np.int32))
    np.save(tmp_path / 'flat.npy', np.zeros((4, 5), np.uint8))
    np.save(tmp_path / 'four.npy', np.zeros((2, 3, 4, 5), np.uint8))
    np.save(tmp_path / 'dict.npy', {'k': np.zeros((3, 4, 5), np.uint8)}, allow_pickle=True)
    (tmp_path / 'broken.npy').write_bytes(b'not an array')
    for bad in ('i32.npy', 'flat.npy', 'four.npy', 'dict.npy', 'broken.npy'):
        assert _main(['--labels', str(tmp_path / bad)]) == 1, bad
        assert 'Invalid argument for --labels' in out(), bad
    (tmp_path / 'v_clusters4_islands.npy').write_bytes(b'')
    assert _main(['--labels', str(src)]) == 1
    assert 'Cache file already exists' in out()
    (tmp_path / 'v_clusters4_islands.npy').unlink()
    (tmp_path / 'v_clusters4_islands.npz').write_bytes(b'')                  # the table is protected like the volume
    assert _main(['--labels', str(src)]) == 1
    assert 'Cache file already exists' in out()
    assert _main(['--labels', str(src), '--output', str(tmp_path / 'missing_dir' / 'i.npy')]) == 1
    assert 'Invalid argument for --output (Cannot write to location)' in out()


def test_label_islands_cli_writes_both_files(tmp_path, monkeypatch, capsys):
    """The accepted command line with the GPU functions replaced: names, dtypes, the min-size and max-islands cuts."""
    vol = np.zeros((2, 3, 4), np.uint8)
    vol[0, 0, :3] = 2; vol[1, 2, 2:] = 5; vol[1, 0, 0] = 2; vol[0, 2, :] = 1         # noqa: E702
    lab = np.zeros(vol.shape, np.int32)
    lab[0, 0, :3] = 1; lab[1, 2, 2:] = 23; lab[1, 0, 0] = 13; lab[0, 2, :] = 9        # noqa: E702
    calls = []

    def fake_label(volume, select=-1, connectivity=1):
        calls.append((select, connectivity))
        return torch.from_numpy(lab)

    monkeypatch.setattr(cc, 'label', fake_label)
    monkeypatch.setattr(cc, 'sizes', lambda labels: torch.bincount(labels.reshape(-1).long(), minlength=labels.numel() + 1)[1:].int())
    src = tmp_path / 'v_clusters4.npy'
    np.save(src, vol)
    assert _main(['--labels', str(src), '--each-value', '--connectivity', '2', '--min-size', '2']) == 0
    assert calls == [(-2, 2)]
    isl = np.load(tmp_path / 'v_clusters4_islands.npy')
    assert isl.dtype == np.uint8 and isl.shape == vol.shape
    want = np.zeros(vol.shape, np.uint8)
    want[0, 2, :] = 1; want[0, 0, :3] = 2; want[1, 2, 2:] = 3                         # noqa: E702
    assert np.array_equal(isl, want)
    with np.load(tmp_path / 'v_clusters4_islands.npz', allow_pickle=False) as z:
        assert set(z.files) == {'sizes', 'lowest_index', 'values'}
        assert z['sizes'].tolist() == [4, 3, 2] and z['sizes'].dtype == np.int64
        assert z['lowest_index'].tolist() == [8, 0, 22] and z['values'].tolist() == [1, 2, 5] and z['values'].dtype == np.uint8
    assert '4 islands, 3 kept' in capsys.readouterr().out
    first = [(tmp_path / f).read_bytes() for f in ('v_clusters4_islands.npy', 'v_clusters4_islands.npz')]
    assert _main(['--labels', str(src), '--each-value', '--connectivity', '2', '--min-size', '2', '--overwrite']) == 0
    assert first == [(tmp_path / f).read_bytes() for f in ('v_clusters4_islands.npy', 'v_clusters4_islands.npz')]
    assert _main(['--labels', str(src), '--max-islands', '1', '--output', str(tmp_path / 'one.npy')]) == 0
    assert calls[-1] == (-1, 1)
    assert np.array_equal(np.load(tmp_path / 'one.npy'), (want == 1).astype(np.uint8))
    assert np.load(tmp_path / 'one.npz')['sizes'].tolist() == [4]


def test_predict_ntf_tag_with_and_without_largest_island():
    import predict_ntf
    tag = predict_ntf.pred_tag
    assert tag(16.0, 'uniform') == '16.0uniform' and tag(0.0, 'annotated', False, False) == '0.0annotated'
    assert tag(16.0, 'uniform', True) == '16.0uniformbls'
    assert tag(16.0, 'uniform', False, True) == '16.0uniformisl'
    assert tag(0.0, 'annotated', True, True) == '0.0annotatedblsisl'
