"""GPU: the hand-crafted voxel features -- vittf_voxel_feature_stats against fp64 numpy, vittf_voxel_features per element
against the fp64 restatement of tests/voxel_features_data.py and against the golden output of the reference's own
compose_features, every addressing mode against the dense bits, vt.voxel_features.classify against one decide call on the
dense matrix, and classify_features.py --features end to end.

The per-element bound (voxel_features_data.bound): |got - want64| <= ulp16(want64) + 16 * 2^-24 * T.  On the CPU the
reference's fp32 output, rounded to fp16, stays within 0.497 of it for all shapes: a correct kernel sits near 0.5 and the
tests assert <= 1.0.
"""
import ctypes as C
import functools
import json
import shutil

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import voxel_features_data as vd

pytestmark = pytest.mark.gpu
vf = vt.voxel_features
CASES = [(s, c) for s in vd.SHAPES for c in vd.CONTENTS]
FILL = 0x5555                                                # what untouched fp16 slots hold


def _ids(case):
    return 'x'.join(map(str, case[0])) + '-' + case[1]


@functools.lru_cache(None)
def _dense(shape, content):
    """(device volume, VoxelStats, dense fp16 numpy [32][nvox]) of a test volume: computed once, shared, left unchanged."""
    vol = torch.from_numpy(vd.volume(shape, content)).cuda()
    st = vf.stats(vol)
    x = vf.compose(vol, st).cpu().numpy()
    x.setflags(write=False)
    return vol, st, x


def _raw(vol, st, channels=11, index=None, v0=0, n=None, stride=None, offset=0, rows=32, tail=64):
    """One vittf_voxel_features call into a buffer filled with FILL: out = buffer + offset elements, `rows` rows of `stride`,
    `tail` more elements behind them.  Returns the whole buffer as uint16 numpy."""
    lib = _lib.load()
    n0, n1, n2 = vol.shape
    n = vol.numel() - v0 if n is None else n
    stride = n if stride is None else stride
    buf = torch.full((offset + rows * stride + tail,), FILL, dtype=torch.int16, device=vol.device)
    idx = None if index is None else torch.as_tensor(np.asarray(index, np.int64)).to(vol.device)
    st_dev = vf._device_stats(st, vol.device)
    _lib.check(lib.vittf_voxel_features(_lib.ptr(vol), n0, n1, n2, st.vmax, _lib.ptr(st_dev), channels, _lib.ptr(idx), v0, n,
                                        C.c_void_p(buf.data_ptr() + 2 * offset), stride, _lib.stream_ptr()), 'vittf_voxel_features')
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16)


def _rows(buf, channels, n, stride, offset=0):
    """(the [channels][n] block the call wrote, as fp16; True when every other element of the buffer still holds FILL)."""
    body = buf[offset:offset + 32 * stride].reshape(32, stride)
    got = body[:channels, :n].copy()
    rest = buf.copy()
    rest[offset:offset + 32 * stride].reshape(32, stride)[:channels, :n] = FILL
    return got.view(np.float16), bool((rest == FILL).all())


# ---------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_statistics_against_fp64(gpu, case):
    shape, content = case
    ref = vd.cached_reference(shape, content)
    nvox = int(np.prod(shape))
    vol, st, _ = _dense(shape, content)
    assert st.vmax == float(vd.volume(shape, content).max()) and st.mean.dtype == np.float64 and st.mean.shape == (11,)
    mean_bound, var_bound = vd.stats_bounds(ref, nvox)
    mean_err = np.abs(st.mean - ref['mean'])
    var_err = np.abs(st.std ** 2 / ref['std'] ** 2 - 1.0)
    print(f'{shape} {content}: mean error / bound {np.max(mean_err / mean_bound):.3g}, variance error / bound {np.max(var_err / var_bound):.3g}')
    assert (mean_err <= mean_bound).all(), (mean_err / mean_bound).tolist()
    assert (var_err <= var_bound).all(), (var_err / var_bound).tolist()
    again = vf.stats(vol)
    assert again.vmax == st.vmax and again.mean.tobytes() == st.mean.tobytes() and again.std.tobytes() == st.std.tobytes()


def test_statistics_refuse_what_cannot_be_standardised(gpu):
    with pytest.raises(ValueError, match='standardised'):
        vf.stats(torch.full((4, 5, 6), 2.0))                  # constant: the intensity's std is 0
    with pytest.raises(ValueError, match='maximum'):
        vf.stats(-torch.rand((4, 5, 6)) - 1.0)                # nothing positive
    with pytest.raises(ValueError):
        vf.stats(torch.rand((1, 5, 6)))
    # the C entry reads the statistics back and refuses a zero std itself, without a launch
    vol, st, _ = _dense((5, 7, 9), 'uniform')
    broken = vf.VoxelStats(st.vmax, st.mean, np.concatenate([st.std[:4], [0.0], st.std[5:]]))
    with pytest.raises(vt.VittfError, match='-1'):
        _raw(vol, broken)
    assert _rows(_raw(vol, broken, channels=1), 1, vol.numel(), vol.numel())[1]        # channel 0 alone does not need it


# ---------------------------------------------------------------------------- 2. dense compose
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_dense_compose_per_element(gpu, case):
    shape, content = case
    ref = vd.cached_reference(shape, content)
    nvox = int(np.prod(shape))
    vol, st, x = _dense(shape, content)
    assert x.shape == (32, nvox) and x.dtype == np.float16 and not x[11:].any()
    got = x[:11].astype(np.float64)
    ratio = np.abs(got - ref['want']) / vd.bound(ref)
    border = vd.border_mask(shape)
    print(f'{shape} {content}: largest |got - want64| / bound {ratio.max():.3f} (border voxels {ratio[:, border].max():.3f}), '
          f'per channel {ratio.max(1).round(3).tolist()}')
    assert np.isfinite(got).all()
    assert ratio[:, border].max() <= 1.0, 'border voxels: the two paddings'
    assert ratio.max() <= 1.0
    # rows 11..31, the gap a longer stride leaves and a canary behind the matrix keep their bytes; the strided call (rows
    # not 16-byte aligned: 2-byte stores) gives the bits of the contiguous one
    stride = nvox + 13
    buf = _raw(vol, st, stride=stride, offset=3)
    rows, untouched = _rows(buf, 11, nvox, stride, offset=3)
    assert untouched
    assert rows.tobytes() == x[:11].tobytes()


# ---------------------------------------------------------------------------- 3. the reference's own output
@pytest.mark.parametrize('content,shape', [('uniform', (12, 10, 14)), ('ct', (9, 17, 5))])
def test_against_the_reference_golden(gpu, golden_dir, content, shape):
    """want64 replaced by the reference's fp32 output, the fp32 term doubled: two fp32 evaluations can differ by twice it."""
    with np.load(golden_dir + '/voxel_features.npz', allow_pickle=False) as z:
        volume, gold = z[f'{content}_volume'], z[f'{content}_features'].reshape(11, -1).astype(np.float64)
    assert volume.shape == shape
    ref = vd.reference(volume)
    got = vf.compose(volume).cpu().numpy()[:11].astype(np.float64)
    ratio = np.abs(got - gold) / vd.bound(ref, gold, fp32_factor=2.0)
    print(f'{shape} {content}: largest |got - reference fp32| / bound {ratio.max():.3f}')
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------------------- 4. addressing
@pytest.mark.parametrize('shape', [(5, 7, 9), (33, 17, 65)])
def test_ranges_and_gathers_give_the_dense_bits(gpu, shape):
    vol, st, x = _dense(shape, 'ct')
    nvox = vol.numel()
    rng = np.random.default_rng(nvox)
    n2 = shape[2]
    ranges = [(3, 13), (n2 // 2, 2 * n2 + 5), (0, 1), (nvox - 1, 1), (nvox - 21, 21), (8, 64), (1, nvox - 1), (5, 1024 + 3)]
    for v0, n in ranges:
        if v0 + n > nvox:
            continue
        for offset, stride in ((0, n), (5, n + 8 - n % 8), (1, n + 3)):          # aligned rows; phase 5 with aligned strides; neither
            buf = _raw(vol, st, v0=v0, n=n, stride=stride, offset=offset)
            rows, untouched = _rows(buf, 11, n, stride, offset)
            assert untouched, (v0, n, offset, stride)
            assert rows.tobytes() == x[:11, v0:v0 + n].tobytes(), (v0, n, offset, stride)
        assert vf.compose(vol, st, start=v0, count=n).cpu().numpy().tobytes() == np.ascontiguousarray(x[:, v0:v0 + n]).tobytes()
    for count in (1, 7, 200, 1500):
        idx = rng.integers(0, nvox, count)
        idx[rng.integers(0, count, max(count // 4, 1))] = idx[0]             # duplicates
        idx = np.concatenate([[0, nvox - 1], idx, [nvox - 1, 0]])
        for offset, stride in ((0, idx.size), (2, idx.size + 8 - idx.size % 8)):
            buf = _raw(vol, st, index=idx, n=idx.size, stride=stride, offset=offset)
            rows, untouched = _rows(buf, 11, idx.size, stride, offset)
            assert untouched and rows.tobytes() == np.ascontiguousarray(x[:11][:, idx]).tobytes(), (count, offset)
        assert vf.compose(vol, st, voxels=idx).cpu().numpy().tobytes() == np.ascontiguousarray(x[:, idx]).tobytes()
    # channels = 1 is row 0 of channels = 11, in every mode; rows 1.. are not written
    one = vf.compose(vol, st, channels=1).cpu().numpy()
    assert one[0].tobytes() == x[0].tobytes() and not one[1:].any()
    buf = _raw(vol, st, channels=1, v0=3, n=77, stride=80, offset=1)
    rows, untouched = _rows(buf, 1, 77, 80, 1)
    assert untouched and rows.tobytes() == x[:1, 3:80].tobytes()
    idx = np.asarray([nvox - 1, 0, 5, 5])
    assert vf.compose(vol, st, channels=1, voxels=idx).cpu().numpy()[0].tobytes() == x[0, idx].tobytes()
    for bad in ([nvox], [-1], [0, 2 ** 40]):
        with pytest.raises(ValueError):
            vf.compose(vol, st, voxels=bad)
    for kw in (dict(start=-1), dict(start=nvox - 3, count=4), dict(channels=2), dict(pad_to=8)):
        with pytest.raises(ValueError):
            vf.compose(vol, st, **kw)


# ---------------------------------------------------------------------------- 5. streaming
@functools.lru_cache(None)
def _boxes():
    """The end-to-end volume on the device, its labels, statistics and 40 annotated voxels per class (background included)."""
    volume, lab = vd.boxes_volume()
    rng = np.random.default_rng(3)
    ann = {}
    for name, value in (('ntf1', 1), ('ntf2', 2), ('background', 0)):
        where = np.argwhere(lab == value)
        ann[name] = torch.from_numpy(where[rng.choice(where.shape[0], 40, replace=False)])
    vol = torch.from_numpy(volume).cuda()
    return vol, lab, vf.stats(vol), ann


@functools.lru_cache(None)
def _model(kind, channels=11):
    vol, lab, st, ann = _boxes()
    samples, targets = vf.sample(vol, ann, st, channels)
    assert samples.shape == (120, 32) and samples.dtype == torch.float32 and targets.tolist() == [0] * 40 + [1] * 40 + [2] * 40
    values = np.asarray([1, 2, 0])[targets]
    names = ['background', 'ntf1', 'ntf2']
    if kind == 'forest':
        return vt.forest.fit(samples, values, trees=8, bootstrap=False, seed=1, class_names=names)
    if kind == 'mlp':
        return vt.mlp.fit(samples, values, hidden=(32,), epochs=60, batch=40, lr=1e-2, seed=1, class_names=names)
    return vt.svm.fit(samples, values, kernel=kind, class_names=names)


@pytest.mark.parametrize('kind', ['forest', 'rbf', 'linear', 'mlp'])
def test_classify_streams_the_dense_decision(gpu, kind):
    vol, lab, st, ann = _boxes()
    model = _model(kind)
    nvox = vol.numel()
    x = vf.compose(vol, st)
    decide = {'forest': vt.forest.decide, 'mlp': lambda x, m, v: vt.mlp.decide(x, m, None, False, v)[::2]}.get(
        kind, lambda x, m, v: vt.svm.decide(x, m, None, v))   # votes, probabilities (of a (32,) head) or decisions
    want, want_votes = decide(x, model, True)
    want, want_votes = want.cpu().numpy(), want_votes.cpu().numpy()
    for slab in (4104, 5000, 1 << 24):                        # 4 slabs (last: 1128 voxels), 3 slabs (last: 3440), one
        assert slab % 8 == 0 and (slab > nvox or nvox % slab)
        got = vf.classify(vol, model, stats=st, slab_voxels=slab)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(vol.shape) and got.is_cuda
        assert got.cpu().numpy().tobytes() == want.tobytes(), (kind, slab)
        got, votes = vf.classify(vol, model, stats=st, slab_voxels=slab, want_votes=True)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (kind, slab)
        assert tuple(votes.shape) == (want_votes.shape[0],) + tuple(vol.shape)
        assert votes.cpu().numpy().tobytes() == want_votes.tobytes(), (kind, slab)
    acc = float((model.labels[want] == lab.reshape(-1)).mean())
    print(f'{kind}: accuracy on the two boxes {acc:.3f}')
    assert acc > 0.7
    if kind == 'forest':
        # the gathered training rows are the streamed ones: fully grown trees on distinct rows give every training voxel its class
        for name, value in (('ntf1', 1), ('ntf2', 2), ('background', 0)):
            at = vf.linear_index(ann[name], vol.shape)
            assert (model.labels[want[at]] == value).all(), name
        with pytest.raises(ValueError):
            vf.classify(vol, model, stats=st, slab_voxels=100)            # not a multiple of 8
        one = vf.classify(vol, _model('forest', 1), channels=1, stats=st, slab_voxels=4104).cpu().numpy()
        dense1 = vt.forest.decide(vf.compose(vol, st, channels=1), _model('forest', 1))[0].cpu().numpy()
        assert one.tobytes() == dense1.tobytes()


def test_sample_refuses_annotations_outside_the_volume(gpu):
    vol, lab, st, ann = _boxes()
    for bad in ([[24, 0, 0]], [[0, 0, -1]], [[0, 20, 0]]):
        with pytest.raises(ValueError, match='outside'):
            vf.sample(vol, {'a': torch.tensor(bad)}, st)


# ---------------------------------------------------------------------------- 6. the command line
def _case_dir(d, seed=2):
    volume, lab = vd.boxes_volume(seed=seed)
    d.mkdir()
    np.save(d / 'volume.npy', np.flip(volume, axis=-3))      # the files are stored flipped on axis -3
    np.save(d / 'labels.npy', np.flip(lab, axis=-3))
    return volume, lab


def _main(argv):
    import classify_features
    with pytest.raises(SystemExit) as e:
        classify_features.main(argv)
    return e.value.code


def test_command_line_end_to_end(gpu, tmp_path, capsys, monkeypatch):
    a = tmp_path / 'a'
    volume, lab = _case_dir(a)
    seen = []
    sample = vf.sample
    monkeypatch.setattr(vf, 'sample', lambda vol, ann, *r, **k: (seen.append({n: c.clone() for n, c in ann.items()}), sample(vol, ann, *r, **k))[1])
    base = ['--data', str(a), '--num-samples', '40']
    args = base + ['--features', 'handcrafted', '--classifier', 'forest', '--trees', '8', '--no-bootstrap']
    assert _main(args) == 0
    tag = '40.0both_hand_rf8'
    pred = np.load(a / f'rf_pred{tag}.npy')
    assert pred.dtype == np.uint8 and pred.shape == volume.shape == (24, 20, 28) and set(np.unique(pred)) <= {0, 1, 2}
    model = vt.forest.load_model(a / f'rf_model{tag}.npz')
    assert model.n_features == 32 and model.trees == 8 and model.labels.tolist() == [0, 1, 2]
    assert set(model.feature[model.feature >= 0]) <= set(range(11))          # the zero rows are never split on
    metrics = json.load(open(a / f'rf_metrics{tag}.json'))
    assert {'mAcc', 'mIoU', 'fit_time', 'predict_time', 'n_trees'} <= set(metrics)
    print(f"--features handcrafted, 8 trees: mIoU {metrics['mIoU']:.3f}, mAcc {metrics['mAcc']:.3f}")
    assert (pred == lab).mean() > 0.7
    # every training voxel gets its own class: the gathered training rows and the streamed ones are the same bits
    assert len(seen) == 1 and list(seen[0]) == ['ntf1', 'ntf2', 'background']
    for name, value in (('ntf1', 1), ('ntf2', 2), ('background', 0)):
        c = seen[0][name].numpy()
        assert c.shape[0] > 0 and (lab[c[:, 0], c[:, 1], c[:, 2]] == value).all()
        assert (pred[c[:, 0], c[:, 1], c[:, 2]] == value).all(), name
    before = {p.name: p.read_bytes() for p in a.glob('rf_*.npy')}
    assert list(before) == [f'rf_pred{tag}.npy']
    assert _main(args) == 0 and 'Already inferred RF preds' in capsys.readouterr().out
    assert _main(args + ['--overwrite']) == 0
    assert {p.name: p.read_bytes() for p in a.glob('rf_*.npy')} == before
    again = vt.forest.load_model(a / f'rf_model{tag}.npz')
    for name in ('tree_offset', 'feature', 'threshold', 'left', 'right', 'value'):
        assert getattr(again, name).tobytes() == getattr(model, name).tobytes(), name
    # the intensity alone, with the vote shares written slab by slab
    assert _main(base + ['--features', 'intensity', '--classifier', 'forest', '--trees', '8', '--no-bootstrap', '--votes']) == 0
    tag_i = '40.0both_intensity_rf8'
    pred_i = np.load(a / f'rf_pred{tag_i}.npy')
    conf = np.load(a / f'rf_votes{tag_i}.npy')
    assert pred_i.shape == (24, 20, 28) and conf.dtype == np.uint8 and conf.shape == (3, 24, 20, 28)
    assert np.array_equal(np.asarray([0, 1, 2], np.uint8)[conf.argmax(0)], pred_i) and conf.max() == 255
    assert set(vt.forest.load_model(a / f'rf_model{tag_i}.npz').feature.tolist()) <= {-1, 0}
    assert (a / f'rf_metrics{tag_i}.json').exists()
    # the support-vector machine on the same features, under its own tag
    assert _main(base + ['--features', 'handcrafted', '--classifier', 'svm']) == 0
    svm_pred = np.load(a / 'svm_pred40.0both_hand_rbf.npy')
    assert svm_pred.shape == (24, 20, 28) and svm_pred.dtype == np.uint8 and (svm_pred == lab).mean() > 0.7
    assert vt.svm.load_model(a / 'svm_model40.0both_hand_rbf.npz').sv.shape[1] == 32 and (a / 'svm_metrics40.0both_hand_rbf.json').exists()
    # --model applies the saved forest to a second volume, standardised with its own statistics
    b = tmp_path / 'b'
    volume_b, lab_b = _case_dir(b, seed=7)
    assert _main(['--data', str(b), '--features', 'handcrafted', '--model', str(a / f'rf_model{tag}.npz')]) == 0
    pred_b = np.load(b / 'rf_pred0.0annotated_hand_rf8.npy')
    assert pred_b.shape == (24, 20, 28) and (pred_b == lab_b).mean() > 0.7 and not (b / 'rf_model0.0annotated_hand_rf8.npz').exists()
    want_b = vf.classify(volume_b, model).cpu().numpy()
    assert np.array_equal(model.labels[want_b], pred_b)
    shutil.rmtree(b)
