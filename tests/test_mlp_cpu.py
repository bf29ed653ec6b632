"""CPU: vt.mlp without a device -- the ABI surface of vittf_mlp_decide, the hand-written backward pass and AdamW against
torch, the fit's determinism and accuracy, model files and their refusals, the command line's refusals and tags, and the
conditions the GPU cases of tests/test_gpu_mlp.py rely on (checked with the fp64 oracle of tests/mlp_data.py).
"""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import mlp_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
mlp = vt.mlp


# ---------------------------------------------------------------------------- 1. ABI surface
def _call(lib, f=384, nvox=1000, widths=(64,), classes=3, feat=1, weights=1, biases=1, labels=1, ws=1, addr=0x1000, logits=None,
          vn=None, ws_bytes=1 << 30, layers=None, no_widths=False):
    """vittf_mlp_decide on placeholder addresses: only calls the argument checks refuse are made with it."""
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    arr = None if no_widths else (C.c_int32 * max(len(widths), 1))(*widths)
    return lib.vittf_mlp_decide(p(feat), f, nvox, p(weights), p(biases), arr, len(widths) if layers is None else layers, classes, vn,
                                p(labels), logits, None, p(ws), ws_bytes, None)


def test_mlp_entries_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    for name, want in (('CLASSES', 8), ('LAYERS', 2), ('WIDTH', 256)):
        assert int(re.search(r'#define\s+VITTF_MLP_MAX_' + name + r'\s+(\d+)', header).group(1)) == want == getattr(_lib, 'MLP_MAX_' + name)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    assert re.search(r'\bint\s+vittf_mlp_decide\s*\(', header) and re.search(r'\bsize_t\s+vittf_mlp_workspace_bytes\s*\(', header)
    for name in ('vittf_mlp_decide', 'vittf_mlp_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    for f in (0, 16, 48, 1056, -32):
        assert _call(lib, f=f) == INVALID, f
    for c in (0, 1, 9):
        assert _call(lib, classes=c) == INVALID, c
    for w in ((0,), (16,), (48,), (288,), (64, 31), (32, 32, 32)):
        assert _call(lib, widths=w) == INVALID, w
    assert _call(lib, layers=-1) == INVALID and _call(lib, layers=1, no_widths=True) == INVALID
    for nvox in (0, -5):
        assert _call(lib, nvox=nvox) == INVALID, nvox
    for missing in ('feat', 'weights', 'biases', 'labels', 'ws'):
        assert _call(lib, **{missing: 0}) == INVALID, missing
    for addr in (0x1001, 0x1002, 0x1004, 0x1008):            # feat: 2 bytes, weights and biases: 4, workspace: 16
        assert _call(lib, addr=addr) == INVALID, addr
    assert _call(lib, logits=C.c_void_p(0x1002)) == INVALID and _call(lib, vn=C.c_void_p(0x1002)) == INVALID
    assert _call(lib, ws_bytes=1024) == -2                   # VITTF_ERR_WORKSPACE
    # the workspace: 256 + sum (in / 32) ceil(out / 32) 5120 bytes; 0 for a head the call refuses
    ws = lambda f, w, c: lib.vittf_mlp_workspace_bytes(f, (C.c_int32 * max(len(w), 1))(*w), len(w), c)     # noqa: E731
    assert ws(384, (), 6) == 256 + 12 * 5120
    assert ws(384, (256, 64), 4) == 256 + (12 * 8 + 8 * 2 + 2 * 1) * 5120
    assert ws(384, (48,), 4) == 0 and ws(384, (), 9) == 0 and ws(40, (), 3) == 0
    assert lib.vittf_mlp_workspace_bytes(384, None, 0, 3) == 256 + 12 * 5120


# ---------------------------------------------------------------------------- 2. the backward pass and the optimiser
def _torch_head(weights, biases):
    mods = []
    for i, (w, b) in enumerate(zip(weights, biases)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] if i + 1 == len(weights) else [lin, torch.nn.ReLU()]
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize('hidden', [(), (32,), (64, 32)], ids=str)
def test_backward_pass_equals_autograd(hidden):
    rng = np.random.default_rng(3)
    weights, biases = mlp.init_params((96,) + hidden + (4,), rng)
    x, y = rng.standard_normal((50, 96)), rng.integers(0, 4, size=50)
    loss, gw, gb = mlp.loss_and_grads(weights, biases, x, y)
    head = _torch_head(weights, biases)
    want = torch.nn.functional.cross_entropy(head(torch.from_numpy(x)), torch.from_numpy(y))
    want.backward()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()          # noqa: E731
    assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
    for lin, w, b in zip([m for m in head if isinstance(m, torch.nn.Linear)], gw, gb):
        assert rel(w, lin.weight.grad.numpy()) <= 1e-12 and rel(b, lin.bias.grad.numpy()) <= 1e-12


def test_twenty_adamw_cosine_steps_equal_torch():
    rng = np.random.default_rng(4)
    hidden, epochs, lr, wd = (32,), 20, 1e-2, 1e-2
    weights, biases = mlp.init_params((96,) + hidden + (3,), rng)
    x, y = rng.standard_normal((64, 96)), rng.integers(0, 3, size=64)
    head = _torch_head(weights, biases)
    opt = torch.optim.AdamW(head.parameters(), lr=lr, weight_decay=wd)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs)
    params = [p for pair in zip(weights, biases) for p in pair]
    state = mlp.new_state(params)
    for e in range(epochs):                                   # one step an epoch: the schedule moves with every step
        assert abs(mlp.cosine_lr(lr, e, epochs) - opt.param_groups[0]['lr']) <= 1e-15
        _, gw, gb = mlp.loss_and_grads(weights, biases, x, y)
        mlp.adamw_step(params, [g for pair in zip(gw, gb) for g in pair], state, mlp.cosine_lr(lr, e, epochs), wd)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(head(torch.from_numpy(x)), torch.from_numpy(y)).backward()
        opt.step()
        sched.step()
    for p, q in zip(params, head.parameters()):
        assert np.abs(p - q.detach().numpy()).max() <= 1e-10 * max(1.0, np.abs(p).max())


# ---------------------------------------------------------------------------- 3. fit
def test_fit_is_deterministic():
    x, y = mlp_data.planted(96, 3, 40, 1)
    a = mlp.fit(x, y, hidden=(32,), epochs=5, seed=7)
    b = mlp.fit(x, y, hidden=(32,), epochs=5, seed=7)
    for p, q in zip(a.weights + a.biases, b.weights + b.biases):
        assert p.dtype == np.float32 and p.tobytes() == q.tobytes()
    assert a.loss_history.tobytes() == b.loss_history.tobytes() and a.loss_history.size == 5
    c = mlp.fit(x, y, hidden=(32,), epochs=5, seed=8)
    assert c.weights[0].tobytes() != a.weights[0].tobytes()


@pytest.mark.parametrize('hidden', [(), (32,)], ids=str)
def test_default_fit_separates_a_planted_problem(hidden):
    x, y = mlp_data.separable(96, 3, 200, 2)
    model = mlp.fit(x, y + 1, hidden=hidden, class_names=['a', 'b', 'c'])
    assert model.train_accuracy == 1.0 and model.labels.tolist() == [1, 2, 3] and model.hidden == hidden
    assert model.loss_history.size == 100 and model.loss_history[-1] < model.loss_history[0]
    assert np.array_equal(mlp_data.argmax(mlp_data.logits(model, x.T)), y)
    assert model.n_params == sum((i + 1) * o for i, o in zip((96,) + hidden, hidden + (3,)))


def test_fit_refuses_bad_arguments():
    x, y = mlp_data.planted(96, 3, 10, 1)
    for kw in (dict(hidden=(48,)), dict(hidden=(32, 32, 32)), dict(hidden=(288,)), dict(epochs=0), dict(batch=0), dict(lr=0.0),
               dict(weight_decay=-1.0), dict(class_names=['a'])):
        with pytest.raises(ValueError):
            mlp.fit(x, y, **kw)
    with pytest.raises(ValueError):
        mlp.fit(x[:, :40], y)
    with pytest.raises(ValueError):
        mlp.fit(x, np.zeros_like(y))                           # one class
    with pytest.raises(ValueError):
        mlp.fit(x, np.arange(y.size) % 9)                      # nine classes


# ---------------------------------------------------------------------------- 4. import and files
def test_from_torch_round_trip():
    torch.manual_seed(0)
    head = torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 5))
    for src in (head, head.state_dict()):
        model = mlp.from_torch(src, labels=[0, 2, 3, 5, 9])
        assert model.hidden == (64, 32) and model.n_features == 96 and model.classes == 5 and model.labels.tolist() == [0, 2, 3, 5, 9]
        x = np.random.default_rng(0).standard_normal((96, 33)).astype(np.float16)
        want = head.double()(torch.from_numpy(x.T.astype(np.float64))).detach().numpy().T
        head.float()
        assert np.abs(mlp_data.logits(model, x) - want).max() <= 1e-12
    for bad in (torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.GELU(), torch.nn.Linear(64, 3)),
                torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.ReLU()),
                torch.nn.Sequential(torch.nn.Linear(96, 64, bias=False), torch.nn.ReLU(), torch.nn.Linear(64, 3)),
                torch.nn.Sequential(torch.nn.Linear(96, 48), torch.nn.ReLU(), torch.nn.Linear(48, 3)),
                {'0.weight': torch.zeros(3, 96)}):
        with pytest.raises(ValueError):
            mlp.from_torch(bad)


def _tiny(hidden=(32,), classes=3, F=32):
    rng = np.random.default_rng(0)
    return mlp_data.int_model(rng, F, hidden, classes)


def test_model_files_round_trip_and_refuse_each_other(tmp_path):
    x, y = mlp_data.planted(96, 3, 20, 1)
    model = mlp.fit(x, y, hidden=(32,), epochs=3, normalize=True, class_names=['a', 'b', 'c'])
    mlp.save_model(model, tmp_path / 'm.npz')
    assert mlp.is_mlp_file(tmp_path / 'm.npz')
    back = mlp.load_model(tmp_path / 'm.npz')
    assert back.class_names == ['a', 'b', 'c'] and back.normalize and back.hidden == (32,) and back.n_features == 96
    assert all(p.tobytes() == q.tobytes() for p, q in zip(model.weights + model.biases, back.weights + back.biases))
    assert back.loss_history.tobytes() == model.loss_history.tobytes() and back.train_accuracy == model.train_accuracy
    assert str(np.load(tmp_path / 'm.npz')['format'][()]) == 'vittf-mlp-1'
    assert not vt.forest.is_forest_file(tmp_path / 'm.npz')
    with pytest.raises(ValueError):
        vt.svm.load_model(tmp_path / 'm.npz')
    with pytest.raises(ValueError):
        vt.forest.load_model(tmp_path / 'm.npz')
    np.save(tmp_path / 'a.npy', np.zeros(3))
    np.savez(tmp_path / 'other.npz', a=np.zeros(3))
    (tmp_path / 'junk.npz').write_bytes(b'PK\x03\x04 not a zip')
    for name in ('a.npy', 'other.npz', 'junk.npz'):
        assert not mlp.is_mlp_file(tmp_path / name)
        with pytest.raises(ValueError):
            mlp.load_model(tmp_path / name)
    arrays = dict(np.load(tmp_path / 'm.npz'))
    for key, value in (('weight1', None), ('bias0', arrays['bias0'][:-1]), ('hidden', np.asarray([48])),
                       ('weight0', arrays['weight0'].astype(np.float64)), ('labels', np.asarray([2, 1, 0], np.uint8))):
        broken = dict(arrays)
        if value is None:
            del broken[key]
        else:
            broken[key] = value
        np.savez(tmp_path / 'broken.npz', **broken)
        with pytest.raises(ValueError):
            mlp.load_model(tmp_path / 'broken.npz')


def test_constructor_refuses_every_invalid_model():
    m = _tiny()
    ok = dict(class_names=m.class_names, labels=m.labels, n_features=32, normalize=False, hidden=(32,), weights=m.weights, biases=m.biases)
    mlp.MlpModel(**ok)
    nan_w = [m.weights[0].copy(), m.weights[1]]
    nan_w[0][0, 0] = np.nan
    inf_b = [m.biases[0], m.biases[1].copy()]
    inf_b[1][0] = np.inf
    for bad in (dict(class_names=['a']), dict(labels=[0, 0, 1]), dict(labels=[2, 1, 0]), dict(n_features=48), dict(n_features=64),
                dict(hidden=(64,)), dict(hidden=()), dict(hidden=(32, 32)), dict(weights=m.weights[:1]), dict(biases=m.biases[:1]),
                dict(weights=nan_w), dict(biases=inf_b), dict(weights=[m.weights[0], m.weights[1][:2]]),
                dict(weights=[m.weights[0] * np.float32(2.0 ** 100), m.weights[1]])):
        with pytest.raises(ValueError):
            mlp.MlpModel(**{**ok, **bad})
    with pytest.raises(ValueError):                           # nine classes, 1056 features, a 288-wide layer, three layers
        mlp_data.int_model(np.random.default_rng(0), 32, (), 9)
    for F, head in ((1056, ()), (32, (288,)), (32, (32, 32, 32))):
        with pytest.raises(ValueError):
            mlp_data.int_model(np.random.default_rng(0), F, head, 3)


# ---------------------------------------------------------------------------- 5. the command line's refusals and tags
@pytest.mark.parametrize('argv,flag', [(['--gamma', '0.5'], 'gamma'), (['--C', '1.0'], 'C'), (['--kernel', 'rbf'], 'kernel'),
                                       (['--tol', '0.001'], 'tol'), (['--hidden', '48'], 'hidden'), (['--hidden', '32,32,32'], 'hidden'),
                                       (['--hidden', 'wide'], 'hidden'), (['--hidden', '512'], 'hidden'), (['--epochs', '0'], 'epochs'),
                                       (['--batch', '0'], 'batch'), (['--lr', '0'], 'lr'), (['--weight-decay', '-1'], 'weight-decay'),
                                       (['--normalize', '--features', 'handcrafted'], 'normalize'),
                                       (['--normalize', '--features', 'intensity'], 'normalize')])
def test_command_line_refuses_before_the_device(tmp_path, capsys, monkeypatch, argv, flag):
    import classify_features
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('the device was asked for'))
    with pytest.raises(SystemExit) as e:
        classify_features.main(['--data', str(tmp_path), '--classifier', 'mlp'] + argv)
    assert e.value.code == 1
    assert f'Invalid argument for --{flag}' in capsys.readouterr().out


def test_command_line_model_file_decides_the_classifier_and_tags(tmp_path, capsys):
    import classify_features as cf
    mlp.save_model(_tiny(), tmp_path / 'm.npz')
    with pytest.raises(SystemExit) as e:                     # the MLP file against an explicit --classifier forest
        cf.main(['--data', str(tmp_path), '--classifier', 'forest', '--model', str(tmp_path / 'm.npz')])
    assert e.value.code == 1 and 'does not hold a forest model' in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:                     # implied: the MLP side's refusal of --gamma shows which side ran
        cf.main(['--data', str(tmp_path), '--gamma', '1', '--model', str(tmp_path / 'm.npz')])
    assert e.value.code == 1 and 'does not apply to --classifier mlp' in capsys.readouterr().out
    mlp.save_model(_tiny(F=64), tmp_path / 'm64.npz')
    with pytest.raises(SystemExit) as e:                     # hand-crafted features need F = 32
        cf.main(['--data', str(tmp_path), '--features', 'handcrafted', '--model', str(tmp_path / 'm64.npz')])
    assert e.value.code == 1 and 'fitted on F = 64' in capsys.readouterr().out
    assert cf.mlp_tag(40.0, 'uniform') == '40.0uniform_mlp'
    assert cf.mlp_tag(0.0, 'annotated', (32,), True, False) == '0.0annotated_mlp32_norm_nobg'
    assert cf.mlp_tag(5.0, 'both', (256, 64), features='handcrafted') == '5.0both_hand_mlp256x64'
    assert cf.mlp_tag(5.0, 'both', (), features='intensity', background=False) == '5.0both_intensity_mlp_nobg'
    names = [p.name for p in cf.mlp_paths(tmp_path, '5.0both_mlp32')]
    assert names == ['mlp_pred5.0both_mlp32.npy', 'mlp_model5.0both_mlp32.npz', 'mlp_metrics5.0both_mlp32.json', 'mlp_probs5.0both_mlp32.npy']


# ---------------------------------------------------------------------------- 6. what the GPU cases rely on
def test_exact_cases_are_integers_far_below_2_to_24():
    """The very cases test_gpu_mlp.py::test_exact_cases draws (same generator, same order): every layer an integer, every
    sum of magnitudes below 2^24 (so every partial sum of the fp32 accumulation is exact), every hidden activation below 2^21."""
    for F, head in itertools.product(mlp_data.FS, mlp_data.HEADS):
        rng = np.random.default_rng(1000 * F + 7 * sum(head) + len(head))
        for classes, nvox in itertools.product(mlp_data.CLASSES, mlp_data.NVOX):
            model = mlp_data.int_model(rng, F, head, classes)
            x = mlp_data.int_voxels(rng, F, nvox)
            assert np.abs(x.astype(np.float64)).max() <= 4
            whole, big, act = mlp_data.int_magnitudes(model, x)
            assert whole and big < 2 ** 24 and act < 2 ** 21, (F, head, classes, nvox)


@pytest.mark.parametrize('index,normalize', [(i, False) for i in range(len(mlp_data.REAL_CASES))] + [(mlp_data.NORM_CASE, True)])
def test_real_cases_are_rarely_ambiguous(index, normalize):
    model, x, vn, z, b = mlp_data.real_case(index, normalize)
    F, classes, head, nvox = mlp_data.REAL_CASES[index]
    assert (model.n_features, model.classes, model.hidden, x.shape) == (F, classes, head, (F, nvox))
    assert np.isfinite(b).all() and (b > 0).all()
    assert mlp_data.ambiguous(z, b).mean() <= 0.01
    assert np.unique(mlp_data.argmax(z)).size >= 2             # the head decides something


def test_prob_eps_is_the_documented_sum():
    u = 2.0 ** -24
    r = np.expm1(96 * u) + 2 * u
    assert mlp_data.PROB_EPS == 255 * (2 * r + 9 * u) + 256 * u + 1e-6 and mlp_data.PROB_EPS < 4e-3
