"""CPU: the PCA reduction -- the C-ABI surface of vittf_feature_gram / vittf_feature_project (declared, exported, argument
checks without a launch), vit_tf_amd.pca.basis_from_gram against an independent fp64 SVD of the centred data, the basis
files, and the command lines (infer.py --pca, reduce_features.py) with the GPU functions replaced.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
from pca_data import SHAPES, planted_int, raw_planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_feature_gram_workspace_bytes', 'vittf_feature_gram', 'vittf_feature_project')


# ---------------------------------------------------------------------------- 1. ABI surface
def _gram(lib, f=384, nvox=1000, feat=1, gram=1, sums=1, ws=1, ws_bytes=1 << 40, addr=0x1000):
    """vittf_feature_gram on placeholder addresses: only calls the argument checks refuse are made with it."""
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_feature_gram(p(feat), f, nvox, p(gram), p(sums), p(ws), ws_bytes, None)


def _project(lib, f=384, nvox=1000, k=8, feat=1, comp=1, out=1):
    p = lambda on: C.c_void_p(0x1000) if on else None        # noqa: E731
    return lib.vittf_feature_project(p(feat), f, nvox, p(comp), None, k, p(out), None)


def test_pca_entries_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    run = int(re.search(r'#define\s+VITTF_GRAM_RUN\s+(\d+)', header).group(1))
    assert run <= 4096 and run == _lib.GRAM_RUN
    assert int(re.search(r'#define\s+VITTF_PCA_MAX_K\s+(\d+)', header).group(1)) == 64 == _lib.PCA_MAX_K
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    for f in (0, 16, 48, 1056):
        assert _gram(lib, f=f) == INVALID, f
        assert _project(lib, f=f) == INVALID, f
        assert lib.vittf_feature_gram_workspace_bytes(f, 1000) == 0
    for k in (0, 65):
        assert _project(lib, k=k) == INVALID, k
    assert _gram(lib, nvox=0) == INVALID and _project(lib, nvox=0) == INVALID
    assert lib.vittf_feature_gram_workspace_bytes(384, 0) == 0
    for missing in ('feat', 'gram', 'sums', 'ws'):
        assert _gram(lib, **{missing: 0}) == INVALID, missing
    for missing in ('feat', 'comp', 'out'):
        assert _project(lib, **{missing: 0}) == INVALID, missing
    assert _gram(lib, addr=0x1004) == INVALID                # gram, sums and ws are arrays of doubles
    assert _gram(lib, ws_bytes=0) == WORKSPACE
    for f, nvox in ((32, 1), (384, 64 ** 3), (1024, 128 ** 3)):
        need = lib.vittf_feature_gram_workspace_bytes(f, nvox)
        assert 0 < need < 256 << 20 and need % 8 == 0
        assert _gram(lib, f=f, nvox=nvox, ws_bytes=need - 1) == WORKSPACE


# ---------------------------------------------------------------------------- 2. basis_from_gram
def _svd_reference(x, k):
    """Independent route: SVD of the centred data matrix (no covariance is formed)."""
    xc = x - x.mean(axis=1, keepdims=True)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    return u[:, :k].T, s[:k] ** 2 / (x.shape[1] - 1)


@pytest.mark.parametrize('f,n', SHAPES)
def test_planted_int_has_the_properties_the_gpu_tests_rely_on(f, n):
    x = planted_int(f, n, 11)
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 8
    assert float((np.abs(np.rint(raw_planted(f, n, 11))) > 8).mean()) < 0.01          # clipped values
    x32 = x.astype(np.float32)
    assert np.array_equal((x32 @ x32.T).astype(np.float64), x @ x.T)                  # fp32 summation is exact
    ev = np.linalg.eigvalsh(np.cov(x))[::-1]
    gaps = (ev[:6] - ev[1:7]) / ev[:6]
    assert gaps.min() >= 0.39, gaps


@pytest.mark.parametrize('f,n', SHAPES)
def test_basis_from_gram_matches_an_svd_of_the_centred_data(f, n):
    """Top 6: 1 - |cos| <= 1e-9 (Davis-Kahan: fp64 rounding of the covariance over relative gaps >= 0.39), eigenvalues to 1e-9
    relative, fp32 components orthonormal to 1e-6, the sign rule."""
    k = 6
    x = planted_int(f, n, 11)
    b = vt.basis_from_gram(torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1)), n, k)
    assert b.components.dtype == torch.float32 and b.components.shape == (k, f)
    assert b.mean.dtype == torch.float32 and b.mean.shape == (f,) and b.offset.dtype == torch.float32 and b.offset.shape == (k,)
    assert b.explained_variance.dtype == torch.float64 and b.total_variance.dtype == torch.float64 and b.center is True
    vecs, vals = _svd_reference(x, k)
    comp = b.components.double().numpy()
    cos = np.abs((comp * vecs).sum(1)) / (np.linalg.norm(comp, axis=1) * np.linalg.norm(vecs, axis=1))
    assert (1 - cos <= 1e-9).all(), 1 - cos
    ev = b.explained_variance.numpy()
    assert (np.abs(ev - vals) <= 1e-9 * vals).all() and (np.diff(ev) <= 0).all()
    assert np.abs(comp @ comp.T - np.eye(k)).max() <= 1e-6
    big = np.abs(comp).argmax(axis=1)
    assert (comp[np.arange(k), big] > 0).all()
    assert abs(float(b.total_variance) - np.trace(np.cov(x))) <= 1e-9 * np.trace(np.cov(x))
    assert np.array_equal(b.mean.numpy(), (x.sum(1) / n).astype(np.float32))
    want_off = comp @ (x.sum(1) / n)                        # (the fp32 components here; the basis used its fp64 ones)
    assert np.abs(b.offset.double().numpy() - want_off).max() <= 1e-5 * max(1.0, np.abs(want_off).max())


def test_sign_rule_takes_the_lowest_index_on_ties():
    # covariance with eigenvector (1, -1, 0, ..) / sqrt 2: two entries of equal magnitude, the first one decides
    f = 32
    v = np.zeros(f); v[3], v[7] = -1.0, 1.0
    gram = 5.0 * np.outer(v, v) + np.eye(f) * 1e-3
    b = vt.basis_from_gram(torch.from_numpy(gram), torch.zeros(f, dtype=torch.float64), 10, 1, center=False)
    c = b.components[0].numpy()
    assert c[3] > 0 and c[7] < 0 and abs(abs(c[3]) - abs(c[7])) < 1e-6


def test_uncentred_basis_and_rank_deficiency():
    f, n = 32, 250
    x = planted_int(f, n, 2)
    gram, sums = torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1))
    b = vt.basis_from_gram(gram, sums, n, 4, center=False)
    assert b.center is False and float(b.mean.abs().max()) == 0.0 and float(b.offset.abs().max()) == 0.0
    ev = np.linalg.eigvalsh(x @ x.T / n)[::-1]
    assert np.allclose(b.explained_variance.numpy(), ev[:4], rtol=1e-12)
    assert abs(float(b.total_variance) - np.trace(x @ x.T) / n) <= 1e-12 * np.trace(x @ x.T) / n
    # k beyond the rank: 3 distinct voxels -> a centred rank of 2; the other eigenvalues are clamped at 0, nothing is NaN
    y = np.repeat(planted_int(f, 3, 4), 5, axis=1)
    b = vt.basis_from_gram(torch.from_numpy(y @ y.T), torch.from_numpy(y.sum(1)), y.shape[1], 8)
    assert (b.explained_variance >= 0).all() and torch.isfinite(b.explained_variance).all()
    assert torch.isfinite(b.components).all() and torch.isfinite(b.offset).all() and float(b.explained_variance[2:].max()) < 1e-9
    for bad in (0, f + 1):
        with pytest.raises(ValueError):
            vt.basis_from_gram(gram, sums, n, bad)


def test_basis_file_round_trips_without_pickle(tmp_path):
    x = planted_int(32, 250, 6)
    b = vt.basis_from_gram(torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1)), 250, 5)
    vt.save_basis(b, tmp_path / 'b.npz')
    with np.load(tmp_path / 'b.npz', allow_pickle=False) as z:
        assert set(z.files) == set(vt.Basis._fields)
        assert z['components'].dtype == np.float32 and z['explained_variance'].dtype == np.float64
    back = vt.load_basis(tmp_path / 'b.npz')
    for name in vt.Basis._fields:
        assert torch.equal(torch.as_tensor(getattr(back, name)), torch.as_tensor(getattr(b, name))), name
    np.savez(tmp_path / 'other.npz', components=np.zeros((2, 32), np.float32))
    with pytest.raises(ValueError):
        vt.load_basis(tmp_path / 'other.npz')


def test_rgb_volume_maps_percentiles():
    r = torch.linspace(-1, 1, 3 * 1000).reshape(3, 10, 10, 10).half()
    rgb = vt.rgb_volume(torch.cat([r, r[:1]]))
    assert rgb.shape == (10, 10, 10, 3) and rgb.dtype == np.uint8
    for c in range(3):
        assert rgb[..., c].min() == 0 and rgb[..., c].max() == 255
        assert 0.005 <= float((rgb[..., c] == 0).mean()) <= 0.02 and 0.005 <= float((rgb[..., c] == 255).mean()) <= 0.02
    with pytest.raises(ValueError):
        vt.rgb_volume(r[:2])


# ---------------------------------------------------------------------------- 3. command lines
class _Args:
    cache_path = None
    slice_along = 'all'
    feature_output_size = 64
    overwrite = False


def _name(tmp_path, model, **kw):
    import infer
    a = _Args()
    a.data_path = str(tmp_path / 'vol.npy')
    a.model = model
    for k, v in kw.items():
        setattr(a, k, v)
    return infer.handle_output_path(a).name


def test_output_name_with_pca(tmp_path):
    assert _name(tmp_path, 'vits8') == 'vol_vits8_all_features64.npy'                        # the default name is untouched
    assert _name(tmp_path, 'vits8', pca=None) == 'vol_vits8_all_features64.npy'
    assert _name(tmp_path, 'vits8', pca=8) == 'vol_vits8_all_features64_pca8.npy'
    assert _name(tmp_path, 'vits14_reg', facet='token', layer=-1, pca=8) == 'vol_vits14_reg_all_features64_token_pca8.npy'
    assert _name(tmp_path, 'vits8', facet='key', layer=3, pca=8) == 'vol_vits8_all_features64_L3_pca8.npy'
    assert _name(tmp_path, 'vits8', facet='token', layer=5, pca=8) == 'vol_vits8_all_features64_token_L5_pca8.npy'
    assert _name(tmp_path, 'vits8', pca=8, cache_path=str(tmp_path / 'mine.npy')) == 'mine.npy'
    # the basis a --pca run fits goes beside the file and is protected like it; a run that applies a saved basis writes none
    (tmp_path / 'mine_basis.npz').write_bytes(b'')
    with pytest.raises(SystemExit) as e:
        _name(tmp_path, 'vits8', pca=8, cache_path=str(tmp_path / 'mine.npy'))
    assert e.value.code == 1
    assert _name(tmp_path, 'vits8', pca=8, cache_path=str(tmp_path / 'mine.npy'), overwrite=True) == 'mine.npy'
    assert _name(tmp_path, 'vits8', pca=8, pca_basis='b.npz', cache_path=str(tmp_path / 'mine.npy')) == 'mine.npy'
    assert _name(tmp_path, 'vits8', cache_path=str(tmp_path / 'mine.npy')) == 'mine.npy'


def _fake_gpu(monkeypatch, calls):
    """vt.pca's two GPU passes replaced by their fp64 host expressions (the command line is what is tested here)."""
    def host_project(feat, basis):
        x = torch.as_tensor(feat).double().reshape(feat.shape[0], -1)
        y = basis.components.double() @ x - (basis.offset.double()[:, None] if basis.center else 0.0)
        return y.half().reshape(-1, *feat.shape[1:])

    def fake_project(feat, basis):
        calls.append('project')
        return host_project(feat, basis)

    def fake_reduce(feat, k, center=True):
        calls.append('fit')
        x = torch.as_tensor(feat).double().reshape(feat.shape[0], -1)
        basis = vt.basis_from_gram(x @ x.T, x.sum(1), x.shape[1], k, center)
        return host_project(feat, basis), basis

    monkeypatch.setattr(vt.pca, 'project', fake_project)
    monkeypatch.setattr(vt.pca, 'reduce_features', fake_reduce)


def _main(argv):
    import reduce_features
    with pytest.raises(SystemExit) as e:
        reduce_features.main(argv)
    return e.value.code


def test_reduce_features_cli(tmp_path, monkeypatch, capsys):
    import infer
    import predict_ntf
    calls = []
    _fake_gpu(monkeypatch, calls)
    feats = torch.from_numpy(planted_int(32, 60, 8).reshape(32, 3, 4, 5)).half()
    src = tmp_path / 'v_features6.npy'
    infer.save_features({'t': feats}, src)
    assert _main(['--features', str(src), '--components', '4', '--rgb']) == 0
    assert calls == ['fit']
    out, basis_file, rgb = tmp_path / 'v_features6_pca4.npy', tmp_path / 'v_features6_pca4_basis.npz', tmp_path / 'v_features6_pca_rgb.npy'
    assert out.exists() and basis_file.exists() and rgb.exists()
    saved = np.load(out, allow_pickle=True)[()]
    assert list(saved) == ['t'] and saved['t'].shape == (4, 3, 4, 5) and saved['t'].dtype == np.float16      # the input's letter
    assert predict_ntf.pick_features(saved).shape == (4, 3, 4, 5)
    assert np.load(rgb).shape == (3, 4, 5, 3)
    with np.load(basis_file, allow_pickle=False) as z:
        assert z['components'].shape == (4, 32) and bool(z['center']) is True
    # refusals: an existing output without --overwrite, --rgb below three components, a basis of another width; exit code 1
    capsys.readouterr()
    assert _main(['--features', str(src), '--components', '4']) == 1
    assert 'Cache file already exists' in capsys.readouterr().out
    assert _main(['--features', str(src), '--components', '4', '--overwrite']) == 0
    assert _main(['--features', str(src), '--components', '2', '--rgb']) == 1
    assert 'at least 3 components' in capsys.readouterr().out
    assert not (tmp_path / 'v_features6_pca2.npy').exists()
    wide = torch.from_numpy(planted_int(64, 60, 9).reshape(64, 3, 4, 5)).half()
    np.save(tmp_path / 'wide_features.npy', wide.numpy())                                  # a bare array: letter 'k'
    assert _main(['--features', str(tmp_path / 'wide_features.npy'), '--basis', str(basis_file)]) == 1
    assert 'F = 32' in capsys.readouterr().out
    assert _main(['--features', str(tmp_path / 'nope.npy')]) == 1
    assert _main(['--features', str(src), '--components', '65']) == 1
    # a saved basis is applied, not refitted; --no-center reaches the fit; --output is taken as it is; .pt files work
    calls.clear()
    assert _main(['--features', str(src), '--basis', str(basis_file), '--output', str(tmp_path / 'again.npy')]) == 0
    assert calls == ['project'] and not (tmp_path / 'again_basis.npz').exists()
    assert np.array_equal(np.load(tmp_path / 'again.npy', allow_pickle=True)[()]['t'], saved['t'])
    assert _main(['--features', str(tmp_path / 'wide_features.npy'), '--components', '3', '--no-center',
                  '--output', str(tmp_path / 'w.pt')]) == 0
    w = torch.load(tmp_path / 'w.pt', weights_only=False)
    assert list(w) == ['k'] and w['k'].shape == (3, 3, 4, 5)
    assert vt.load_basis(tmp_path / 'w_basis.npz').center is False


def test_infer_cli_parses_pca(tmp_path, monkeypatch, capsys):
    """main() up to the model constructor: --pca reaches the output name; bad values exit with 1 before anything is loaded."""
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((8, 8, 8), dtype=np.float16))
    seen = {}

    class Stop(Exception):
        pass

    def fake_hipvit(sd, name, **kw):
        raise Stop

    def spy(args):
        path = real(args)
        seen['name'] = path.name
        return path

    real = infer.handle_output_path
    monkeypatch.setattr(infer, 'handle_output_path', spy)
    monkeypatch.setattr(vt, 'HipViT', fake_hipvit)
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.setattr(vt.extract, 'DIST_FORCE', False)
    base = ['--data-path', str(tmp_path / 'vol.npy'), '--synthetic-weights', '0', '--feature-output-size', '4']
    x = planted_int(384, 40, 1)
    vt.save_basis(vt.basis_from_gram(torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1)), 40, 5), tmp_path / 'b.npz')
    for extra, name in (([], 'vol_vits8_all_features4.npy'), (['--pca', '8'], 'vol_vits8_all_features4_pca8.npy'),
                        (['--pca-basis', str(tmp_path / 'b.npz')], 'vol_vits8_all_features4_pca5.npy'),
                        (['--facet', 'token', '--pca', '3'], 'vol_vits8_all_features4_token_pca3.npy')):
        with pytest.raises(Stop):
            infer.main(base + extra)
        assert seen['name'] == name, extra
    for bad in (['--pca', '0'], ['--pca', '65'], ['--pca', '4', '--pca-basis', str(tmp_path / 'b.npz')],
                ['--pca-basis', str(tmp_path / 'missing.npz')]):
        with pytest.raises(SystemExit) as e:
            infer.main(base + bad)
        assert e.value.code == 1, bad
    assert 'Invalid argument for --pca' in capsys.readouterr().out
