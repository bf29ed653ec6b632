"""GPU: the PCA reduction of a feature volume -- vittf_feature_gram, vittf_feature_project, vit_tf_amd.pca and the entry
points (reduce_features.py, infer.py --pca).

Exact cases use integer-valued data (pca_data.planted_int): every product is an integer <= 64 and every fp32 run of at most
VITTF_GRAM_RUN voxels sums exactly, so the Gram matrix, the sums and the projections of small dyadic components must equal
the integer results bit for bit.  Real-valued cases are held to worst-case fp32 bounds written out below.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
from pca_data import planted_int, project_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = _lib.GRAM_RUN

GRAM_F = (32, 64, 96, 384, 768, 1024)
GRAM_N = (1, 7, 16, 250, 256, 1000, RUN + 8, 3 * RUN + 24)
GRAM_CASES = sorted({(f, n) for f in GRAM_F for n in (250, 1000)} | {(f, n) for f in (96, 384) for n in GRAM_N})


def _dev16(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).to(gpu)


# ---------------------------------------------------------------------------- 1. Gram, exact
@pytest.mark.parametrize('f,n', GRAM_CASES)
def test_gram_exact(gpu, f, n):
    x = planted_int(f, n, 1000 * f + n)
    gram, sums = vt.feature_gram(_dev16(x, gpu))
    assert gram.dtype == sums.dtype == torch.float64 and gram.shape == (f, f) and sums.shape == (f,)
    gram, sums = gram.cpu().numpy(), sums.cpu().numpy()
    assert np.array_equal(gram, x @ x.T)
    assert np.array_equal(sums, x.sum(1))
    assert np.array_equal(gram, gram.T)


@pytest.mark.parametrize('f,n,shift', [(96, 1000, 1), (384, 256, 1), (96, 256, 4), (384, 1000, 3)])
def test_gram_exact_on_a_view_at_a_2_byte_aligned_offset(gpu, f, n, shift):
    """The volume as a view `shift` elements into a larger buffer: its rows are not 16-byte aligned whatever n is."""
    x = planted_int(f, n, 7 + f + n)
    buf = torch.full((f * n + 16,), 99.0, dtype=torch.float16, device=gpu)
    buf[shift:shift + f * n] = _dev16(x, gpu).reshape(-1)
    view = buf[shift:shift + f * n].view(f, n)
    assert view.data_ptr() % 16 == 2 * shift and view.is_contiguous()
    gram, sums = vt.feature_gram(view)
    assert np.array_equal(gram.cpu().numpy(), x @ x.T) and np.array_equal(sums.cpu().numpy(), x.sum(1))


def test_gram_exact_beyond_the_workspace_spans(gpu):
    """More runs than the workspace has spans: a workgroup then walks several runs and adds each into its fp64 partial
    (read-add-write), a path no smaller volume reaches.  fp32 runs of VITTF_GRAM_RUN voxels are exact on this data and fp64
    holds the integer totals, so the result is still exact although 64 n > 2^24."""
    f, n = 32, 2 * 128 * RUN + RUN + 40
    x = planted_int(f, n, 5)
    gram, sums = vt.feature_gram(_dev16(x, gpu))
    assert np.array_equal(gram.cpu().numpy(), x @ x.T) and np.array_equal(sums.cpu().numpy(), x.sum(1))


# ---------------------------------------------------------------------------- 2. Gram, real-valued
@pytest.mark.parametrize('n', [1000, 3 * RUN + 24])
def test_gram_real_valued_within_the_fp32_bound(gpu, n):
    """Every entry within (min(n, VITTF_GRAM_RUN) + 1) 2^-24 sum_v |x_iv x_jv| of the fp64 Gram: the worst case of an fp32 sum
    of min(n, RUN) exact products in any order (the fp64 additions across runs are far below it); the sums likewise."""
    f = 384
    g = torch.Generator().manual_seed(n)
    x16 = (torch.randn(f, n, generator=g) + torch.randn(f, 1, generator=g)).half()
    x = x16.double().numpy()
    dev = x16.to(gpu)
    gram, sums = vt.feature_gram(dev)
    gram2, sums2 = vt.feature_gram(dev)
    assert torch.equal(gram, gram2) and torch.equal(sums, sums2)                 # no atomics: the same bits
    gram, sums = gram.cpu().numpy(), sums.cpu().numpy()
    u = (min(n, RUN) + 1) * 2.0 ** -24
    err = np.abs(gram - x @ x.T)
    bound = u * (np.abs(x) @ np.abs(x).T)
    print(f'gram n={n}: max err / bound {float((err / bound).max()):.3e}')
    assert (err <= bound).all()
    assert (np.abs(sums - x.sum(1)) <= u * np.abs(x).sum(1)).all()
    assert np.array_equal(gram, gram.T)


# ---------------------------------------------------------------------------- 3. projection, exact
def _dyadic_components(k, f, seed):
    rng = np.random.default_rng(seed)
    comp = np.zeros((k, f))
    for r in range(k):
        idx = rng.choice(f, size=min(16, f), replace=False)
        comp[r, idx] = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], size=idx.size)
    offset = rng.integers(-512, 513, size=k) * 0.5
    return comp, offset


def _basis(comp, offset):
    k, f = comp.shape
    return vt.Basis(torch.from_numpy(comp).float(), torch.zeros(f), torch.zeros(k, dtype=torch.float64),
                    torch.tensor(0.0, dtype=torch.float64), offset is not None,
                    torch.from_numpy(offset if offset is not None else np.zeros(k)).float())


PROJ_CASES = sorted({(k, f, n) for k in (1, 3, 32, 33, 64) for f, n in ((96, 250), (384, 1000))}
                    | {(33, f, 250) for f in (32, 96, 384, 1024)}
                    | {(k, f, n) for k, f in ((3, 96), (64, 384)) for n in (1, 7, 250, 256, 1000)}
                    | {(64, 32, 7), (1, 32, 256), (1, 1024, 256), (64, 1024, 1), (32, 1024, 7)})


@pytest.mark.parametrize('k,f,n', PROJ_CASES)
def test_project_exact(gpu, k, f, n):
    """Components in {0, +-0.5, +-1, +-2} (at most 16 non-zeros per row), offsets multiples of 0.5 up to 256, integer volume:
    every partial sum is a multiple of 0.5 below 1024 + 256, exact in fp32 in any order; the output is the exact value rounded
    once to fp16."""
    x = planted_int(f, n, 31 * k + f + n)
    comp, offset = _dyadic_components(k, f, k + f + n)
    out = vt.project(_dev16(x, gpu), _basis(comp, offset))
    assert out.dtype == torch.float16 and out.shape == (k, n)
    want = (comp @ x - offset[:, None]).astype(np.float16)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_project_exact_without_offset_and_on_a_volume_shape(gpu):
    f, dims, k = 96, (5, 6, 7), 5
    x = planted_int(f, 210, 3)
    comp, _ = _dyadic_components(k, f, 4)
    out = vt.project(_dev16(x, gpu).reshape(f, *dims), _basis(comp, None))          # center False: a NULL offset
    assert out.shape == (k, *dims)
    assert np.array_equal(out.cpu().numpy().reshape(k, -1), (comp @ x).astype(np.float16))
    lib = _lib.load()                                                               # the raw entry, offset = NULL
    dev, cdev = _dev16(x, gpu), torch.from_numpy(comp).float().to(gpu)
    raw = torch.empty((k, 210), dtype=torch.float16, device=gpu)
    assert lib.vittf_feature_project(_lib.ptr(dev), f, 210, _lib.ptr(cdev), None, k, _lib.ptr(raw), _lib.stream_ptr()) == 0
    assert torch.equal(raw.reshape(k, *dims), out)


def test_volume_with_squeezed_dimensions(gpu):
    """vt.feature_volume squeezes singleton grid dimensions away: (F, n0, n1) and (F, n) volumes reduce like (F, n0, n1, n2)."""
    f, k = 96, 4
    x = planted_int(f, 42, 12)
    dev = _dev16(x, gpu)
    full, basis = vt.reduce_features(dev.reshape(f, 6, 7, 1), k)
    flat, basis3 = vt.reduce_features(dev.reshape(f, 6, 7), k)
    assert full.shape == (k, 6, 7, 1) and flat.shape == (k, 6, 7) and torch.equal(full.reshape(k, -1), flat.reshape(k, -1))
    assert torch.equal(basis.components, basis3.components)
    assert torch.equal(vt.project(x.astype(np.float32).reshape(f, 6, 7), basis).reshape(k, -1), flat.reshape(k, -1))    # a host array


# ---------------------------------------------------------------------------- 4. projection, real-valued
@pytest.mark.parametrize('k,f,n,nnz', [(6, 384, 1000, 384), (64, 384, 250, 384), (33, 384, 257, 384), (33, 1024, 257, 1024),
                                       (33, 1024, 257, 32), (64, 1024, 256, 32)])
def test_project_real_valued_within_the_bound(gpu, k, f, n, nnz):
    """Random unit-norm fp32 components with nnz non-zeros per row, normal fp16 data: every output within
    pca_data.project_bound of the fp64 value,
        0.5 ulp_fp16(y) + (F + 8) 2^-24 (sum_f |v_kf x_fv| + |offset_k|) + 2^-25 sum_f |x_fv|
    (the single rounding; worst-case fp32 accumulation plus the 2^-22 of the hi + lo split; a lo half that underflows).
    Components rounded once to fp16 -- no lo half -- break the bound on this data, so it is not vacuous: at F = 384 with dense
    components, at F = 1024 with 32 non-zeros per row (with 1024 of them the accumulation term alone covers a missing lo half,
    so that case only holds the bound)."""
    g = torch.Generator().manual_seed(k + f + n + nnz)
    x16 = torch.randn(f, n, generator=g).half()
    comp32 = torch.randn(k, f, generator=g)
    if nnz < f:
        mask = torch.zeros(k, f)
        for r in range(k):
            mask[r, torch.randperm(f, generator=g)[:nnz]] = 1.0
        comp32 = comp32 * mask
    comp32 = torch.nn.functional.normalize(comp32, dim=1)
    off32 = torch.randn(k, generator=g)
    x, comp, offset = x16.double().numpy(), comp32.double().numpy(), off32.double().numpy()
    y = comp @ x - offset[:, None]
    bound = project_bound(comp, x, offset, y)
    out = vt.project(x16.to(gpu), _basis(comp, offset)).cpu().double().numpy()
    err = np.abs(out - y)
    print(f'project k={k} f={f} n={n} nnz={nnz}: max err / bound {float((err / bound).max()):.3f}')
    assert (err <= bound).all()
    y16 = (comp32.half().double().numpy() @ x - offset[:, None]).astype(np.float16).astype(np.float64)
    if nnz < 1024:
        assert (np.abs(y16 - y) > bound).any(), 'fp16 components would pass too: the bound does not tell the split apart'


# ---------------------------------------------------------------------------- 5. fit and project end to end
@pytest.mark.parametrize('f,n', [(96, 1000), (384, 4104)])
def test_fit_and_project_end_to_end(gpu, f, n):
    k = 6
    x = planted_int(f, n, f + n)
    dev = _dev16(x, gpu)
    got = vt.fit_basis(dev, k)
    want = vt.basis_from_gram(torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1)), n, k)
    for name in vt.Basis._fields:
        a, b = getattr(got, name), getattr(want, name)
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b)), name
    comp, offset = got.components.double().numpy(), got.offset.double().numpy()
    y = comp @ x - offset[:, None]
    bound = project_bound(comp, x, offset, y)
    reduced, basis2 = vt.reduce_features(dev, k)
    assert torch.equal(basis2.components, got.components)
    out = reduced.cpu().double().numpy()
    assert torch.equal(reduced, vt.project(dev, got))
    assert (np.abs(out - y) <= bound).all()
    # the variance of every reduced row is its eigenvalue, to one fp16 rounding (2^-11), doubled by the square, doubled again
    # for the mean term; the fp64 projection rounded to fp16 must itself be inside (else the data cannot carry the check)
    ev = got.explained_variance.numpy()
    tol = 4 * 2.0 ** -11
    ideal = y.astype(np.float16).astype(np.float64)
    assert (np.abs(ideal.var(axis=1, ddof=1) - ev) <= tol * ev).all()
    rel = np.abs(out.var(axis=1, ddof=1) - ev) / ev
    print(f'end to end f={f} n={n}: variance vs eigenvalue, max relative {float(rel.max()):.2e} (allowed {tol:.2e})')
    assert (rel <= tol).all()


@pytest.mark.parametrize('f,n', [(96, 1000), (384, 4104)])
def test_uncentred_reduction_keeps_dot_products(gpu, f, n):
    """center=False: (V x) . (V y) stays within a bound of x . y computed here in fp64 from the full spectrum: the part of
    x and y outside the kept subspace, |x_perp| |y_perp| (Cauchy-Schwarz on sum_{i > k} (u_i . x)(u_i . y)), plus the fp16
    rounding of the 2 k reduced coordinates (each within e = project_bound of its fp64 value: sum_i |a_i| e_y + |b_i| e_x + e_x e_y)."""
    k = 6
    x = planted_int(f, n, f + n + 1)
    dev = _dev16(x, gpu)
    reduced, basis = vt.reduce_features(dev, k, center=False)
    assert not basis.center and float(basis.mean.abs().max()) == 0.0 and float(basis.offset.abs().max()) == 0.0
    out = reduced.cpu().double().numpy()
    comp = basis.components.double().numpy()
    rng = np.random.default_rng(0)
    ia, ib = rng.integers(0, n, 100), rng.integers(0, n, 100)
    zero = np.zeros(k)
    a, b = comp @ x[:, ia], comp @ x[:, ib]
    ea, eb = project_bound(comp, x[:, ia], zero, a), project_bound(comp, x[:, ib], zero, b)
    perp_a = np.linalg.norm(x[:, ia] - comp.T @ a, axis=0)
    perp_b = np.linalg.norm(x[:, ib] - comp.T @ b, axis=0)
    ortho = np.abs(comp @ comp.T - np.eye(k)).max() * np.linalg.norm(x[:, ia], axis=0) * np.linalg.norm(x[:, ib], axis=0)
    bound = perp_a * perp_b + ortho + (np.abs(a) * eb + np.abs(b) * ea + ea * eb).sum(0)
    exact = (x[:, ia] * x[:, ib]).sum(0)
    got = (out[:, ia] * out[:, ib]).sum(0)
    assert (np.abs(got - exact) <= bound).all()
    assert np.median(bound) < 0.2 * np.median(np.abs(exact)), 'the bound says nothing on this data'


# ---------------------------------------------------------------------------- 6. entry points
def _run(args, env, timeout=300):
    return subprocess.run([sys.executable, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def _plain_env():
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'VITTF_DIST_BACKEND', 'VITTF_DIST_FORCE'):
        env.pop(k, None)
    return env


@pytest.fixture(scope='module')
def reduced_case(gpu, tmp_path_factory):
    """A plain infer.py run (ViT-S/8 on seeded synthetic weights, a 24^3 volume, 6^3 x 384 features) followed by
    reduce_features.py --components 8 on its file: shared by the tests below."""
    d = tmp_path_factory.mktemp('pca')
    vol, _ = vt.synthetic_volume('sphere_filled', 24, 0.2, 3)
    np.save(d / 'v.npy', vol.numpy())
    env = _plain_env()
    common = ['infer.py', '--data-path', str(d / 'v.npy'), '--feature-output-size', '6', '--synthetic-weights', '0']
    r = _run([*common, '--cache-path', str(d / 'plain_features.npy')], env)
    assert r.returncode == 0, r.stderr + r.stdout
    r = _run(['reduce_features.py', '--features', str(d / 'plain_features.npy'), '--components', '8', '--rgb'], env)
    assert r.returncode == 0, r.stderr + r.stdout
    for name in ('plain_features_pca8.npy', 'plain_features_pca8_basis.npz', 'plain_features_pca_rgb.npy'):
        assert (d / name).exists(), name
    return d, env, common


def _same_file(a, b):
    return open(a, 'rb').read() == open(b, 'rb').read()


def test_infer_pca_writes_what_reduce_features_writes(reduced_case):
    d, env, common = reduced_case
    r = _run([*common, '--pca', '8', '--cache-path', str(d / 'direct.npy')], env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _same_file(d / 'direct.npy', d / 'plain_features_pca8.npy')
    assert _same_file(d / 'direct_basis.npz', d / 'plain_features_pca8_basis.npz')
    red = np.load(d / 'direct.npy', allow_pickle=True)[()]
    assert list(red) == ['k'] and red['k'].shape == (8, 6, 6, 6) and red['k'].dtype == np.float16
    rgb = np.load(d / 'plain_features_pca_rgb.npy')
    assert rgb.shape == (6, 6, 6, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, vt.rgb_volume(red['k']))


def test_infer_pca_in_a_one_rank_group(reduced_case):
    """VITTF_DIST_FORCE=1: the one-rank process group; rank 0 reduces and writes the same bytes."""
    import socket
    d, env, common = reduced_case
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = str(sk.getsockname()[1])
    env1 = dict(env, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=port, VITTF_DIST_FORCE='1',
                HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = _run([*common, '--pca', '8', '--cache-path', str(d / 'forced.npy')], env1)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _same_file(d / 'forced.npy', d / 'plain_features_pca8.npy')
    assert _same_file(d / 'forced_basis.npz', d / 'plain_features_pca8_basis.npz')


def test_saved_basis_reproduces_and_the_reduced_file_is_queried(gpu, reduced_case):
    import predict_ntf
    d, env, common = reduced_case
    r = _run(['reduce_features.py', '--features', str(d / 'plain_features.npy'), '--basis', str(d / 'plain_features_pca8_basis.npz'),
              '--output', str(d / 'again.npy')], env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _same_file(d / 'again.npy', d / 'plain_features_pca8.npy')
    feats = predict_ntf.pick_features(np.load(d / 'plain_features_pca8.npy', allow_pickle=True)[()])
    assert feats.shape == (8, 6, 6, 6) and feats.dtype == torch.float16
    ann = {'a': torch.tensor([[3, 4, 5], [20, 10, 12]]), 'b': torch.tensor([[12, 8, 16]])}
    sims = predict_ntf.compute_similarities(np.zeros((24, 24, 24), np.float32), feats, ann)
    assert set(sims) == {'a', 'b'} and all(v.shape == (12, 12, 12) and v.dtype == torch.uint8 for v in sims.values())
