"""CPU: k-means clustering -- the C-ABI surface of vittf_kmeans_assign / vittf_kmeans_sums (declared, exported, argument
checks without a launch), the host arithmetic of vit_tf_amd.kmeans (k-means++ start, centroid update, inertia identity,
renumbering), the clustering files, and every refusal of cluster_features.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
from pca_data import planted_int, raw_planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -2
NAMES = ('vittf_kmeans_assign', 'vittf_kmeans_sums_workspace_bytes', 'vittf_kmeans_sums')
km = vt.kmeans


# ---------------------------------------------------------------------------- 1. ABI surface
def _assign(lib, f=384, nvox=1000, c=8, feat=1, cent=1, labels=1, addr=0x1000):
    """vittf_kmeans_assign on placeholder addresses: only calls the argument checks refuse are made with it."""
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_kmeans_assign(p(feat), f, nvox, p(cent), None, c, p(labels), None, None)


def _sums(lib, f=384, nvox=1000, c=8, feat=1, labels=1, sums=1, counts=1, ws=1, ws_bytes=1 << 40, addr=0x1000):
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_kmeans_sums(p(feat), f, nvox, p(labels), c, p(sums), p(counts), p(ws), ws_bytes, None)


def test_kmeans_entries_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    assert int(re.search(r'#define\s+VITTF_KMEANS_MAX_C\s+(\d+)', header).group(1)) == 64 == _lib.KMEANS_MAX_C
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    for f in (0, 16, 48, 1056):
        assert _assign(lib, f=f) == INVALID, f
        assert _sums(lib, f=f) == INVALID, f
        assert lib.vittf_kmeans_sums_workspace_bytes(f, 1000, 8) == 0
    for c in (0, 1, 65):
        assert _assign(lib, c=c) == INVALID, c
        assert _sums(lib, c=c) == INVALID, c
        assert lib.vittf_kmeans_sums_workspace_bytes(384, 1000, c) == 0
    assert _assign(lib, nvox=0) == INVALID and _sums(lib, nvox=0) == INVALID
    assert lib.vittf_kmeans_sums_workspace_bytes(384, 0, 8) == 0
    for missing in ('feat', 'cent', 'labels'):
        assert _assign(lib, **{missing: 0}) == INVALID, missing
    for missing in ('feat', 'labels', 'sums', 'counts', 'ws'):
        assert _sums(lib, **{missing: 0}) == INVALID, missing
    assert _assign(lib, addr=0x1002) == INVALID              # cent is an array of floats
    assert _sums(lib, addr=0x1004) == INVALID                # sums, counts and ws are arrays of 8-byte values
    # a misaligned half_sq / best alone
    assert lib.vittf_kmeans_assign(C.c_void_p(0x1000), 384, 1000, C.c_void_p(0x1000), C.c_void_p(0x1002), 8, C.c_void_p(0x1000),
                                   None, None) == INVALID
    assert lib.vittf_kmeans_assign(C.c_void_p(0x1000), 384, 1000, C.c_void_p(0x1000), None, 8, C.c_void_p(0x1000),
                                   C.c_void_p(0x1002), None) == INVALID
    assert _sums(lib, ws_bytes=0) == WORKSPACE
    for f, nvox, c in ((32, 1, 2), (384, 64 ** 3, 8), (384, 128 ** 3, 64), (1024, 128 ** 3, 64)):
        need = lib.vittf_kmeans_sums_workspace_bytes(f, nvox, c)
        spans = min(_lib.KMEANS_SPANS, -(-nvox // _lib.GRAM_RUN))
        assert need == spans * ((f // 32) * -(-c // 32) * 1024 + 64) * 8 and 0 < need < 128 << 20
        assert _sums(lib, f=f, nvox=nvox, c=c, ws_bytes=need - 1) == WORKSPACE


def test_python_entries_refuse_bad_shapes_before_the_device():
    x = torch.zeros(32, 10)
    for c in (1, 65):
        with pytest.raises(ValueError):
            km.init_centroids(x, c)
    with pytest.raises(ValueError):
        km.init_centroids(x, 11)                              # more clusters than voxels
    with pytest.raises(ValueError):
        km.init_centroids(torch.zeros(32), 2)


# ---------------------------------------------------------------------------- 2. init_centroids
@pytest.mark.parametrize('f,n,c', [(32, 250, 5), (96, 20000, 64)])
def test_init_centroids_is_seeded_and_picks_distinct_columns(f, n, c):
    """raw_planted columns are distinct (continuous noise).  n = 20000 goes through the subsample of 16384 columns."""
    x = (0.25 * raw_planted(f, n, 3)).astype(np.float16)
    assert np.unique(x.T, axis=0).shape[0] == n
    a = km.init_centroids(x, c, seed=4)
    b = km.init_centroids(torch.from_numpy(x).reshape(f, -1, 10), c, seed=4)           # a tensor, a volume shape: the same
    assert a.dtype == torch.float32 and a.shape == (c, f) and not a.is_cuda
    assert a.numpy().tobytes() == b.numpy().tobytes()
    assert km.init_centroids(x, c, seed=5).numpy().tobytes() != a.numpy().tobytes()
    cols = {x[:, v].astype(np.float32).tobytes(): v for v in range(n)}
    picked = [cols.get(a[i].numpy().tobytes()) for i in range(c)]
    assert None not in picked, 'a centroid is not a column of the input'
    assert len(set(picked)) == c, 'a column was picked twice'


def test_init_centroids_with_fewer_distinct_columns_than_clusters():
    x = np.repeat(planted_int(32, 3, 1), 4, axis=1)           # 12 columns, 3 distinct
    a = km.init_centroids(x, 5, seed=0)
    assert a.shape == (5, 32) and torch.isfinite(a).all()
    assert len({a[i].numpy().tobytes() for i in range(5)}) == 3


# ---------------------------------------------------------------------------- 3. centroid update
def test_update_centroids_and_an_empty_cluster():
    rng = np.random.default_rng(0)
    old = torch.from_numpy(rng.standard_normal((4, 32))).float()
    sums = rng.standard_normal((4, 32)) * 100
    counts = np.array([7, 0, 1, 12345], dtype=np.int64)
    sums[1] = 0.0
    new = km.update_centroids(old, torch.from_numpy(sums), torch.from_numpy(counts))
    assert new.dtype == torch.float32 and new.shape == (4, 32)
    for k in (0, 2, 3):
        assert np.array_equal(new[k].numpy(), (sums[k] / counts[k]).astype(np.float32)), k      # fp64 quotient, rounded once
    assert torch.equal(new[1], old[1])                        # the empty cluster keeps its centroid


# ---------------------------------------------------------------------------- 4. inertia identity
@pytest.mark.parametrize('f,n,c', [(32, 250, 3), (96, 1000, 7)])
def test_inertia_identity_against_the_direct_sum(f, n, c):
    """sum_v |x_v|^2 - sum_c |S_c|^2 / n_c against sum_v |x_v - mean_c(v)|^2, both fp64, on integer data (exact sums): the
    identity loses sum|x|^2 / inertia (here < 10) ulps to cancellation, 1e-12 relative is generous."""
    x = planted_int(f, n, 9)
    labels = np.random.default_rng(1).integers(0, c - 1, size=n)          # the last cluster is empty
    sums = np.stack([x[:, labels == k].sum(1) for k in range(c)])
    counts = np.bincount(labels, minlength=c)
    assert counts[c - 1] == 0
    means = sums[:c - 1] / counts[:c - 1, None]
    direct = float(((x - means[labels].T) ** 2).sum())
    got = km.inertia_from_sums(float((x * x).sum()), torch.from_numpy(sums), torch.from_numpy(counts))
    assert isinstance(got, float) and abs(got - direct) <= 1e-12 * direct


# ---------------------------------------------------------------------------- 5. renumbering
def test_renumber_by_descending_count_with_a_tie():
    cent = torch.arange(5, dtype=torch.float32)[:, None].repeat(1, 32)
    counts = torch.tensor([3, 9, 3, 0, 9])
    new_cent, new_counts, order = km.renumber(cent, counts)
    assert order.tolist() == [1, 4, 0, 2, 3]                  # 9, 9 (lower old index first), 3, 3, 0
    assert new_counts.tolist() == [9, 9, 3, 3, 0] and new_counts.dtype == torch.int64
    assert new_cent[:, 0].tolist() == [1.0, 4.0, 0.0, 2.0, 3.0]


# ---------------------------------------------------------------------------- 6. files
def _clustering(c=4, f=32):
    g = torch.Generator().manual_seed(0)
    return vt.Clustering(torch.randn(c, f, generator=g), torch.tensor([9, 5, 5, 1]), torch.tensor(12.5, dtype=torch.float64),
                         torch.tensor([20.0, 13.0, 12.5], dtype=torch.float64), 3, True)


def test_clustering_file_round_trips_without_pickle(tmp_path):
    cl = _clustering()
    vt.save_clustering(cl, tmp_path / 'c.npz')
    with np.load(tmp_path / 'c.npz', allow_pickle=False) as z:
        assert set(z.files) == set(vt.Clustering._fields)
        assert z['centroids'].dtype == np.float32 and z['counts'].dtype == np.int64 and z['inertia'].dtype == np.float64
    back = vt.load_clustering(tmp_path / 'c.npz')
    for name in vt.Clustering._fields:
        assert torch.equal(torch.as_tensor(getattr(back, name)), torch.as_tensor(getattr(cl, name))), name
    assert back.n_iter == 3 and back.converged is True
    np.savez(tmp_path / 'other.npz', centroids=np.zeros((2, 32), np.float32))
    with pytest.raises(ValueError):
        vt.load_clustering(tmp_path / 'other.npz')
    x = planted_int(32, 250, 6)                               # a basis file is not a clustering file
    vt.save_basis(vt.basis_from_gram(torch.from_numpy(x @ x.T), torch.from_numpy(x.sum(1)), 250, 5), tmp_path / 'b.npz')
    with pytest.raises(ValueError):
        vt.load_clustering(tmp_path / 'b.npz')


# ---------------------------------------------------------------------------- 7. command line
def _main(argv):
    import cluster_features
    with pytest.raises(SystemExit) as e:
        cluster_features.main(argv)
    return e.value.code


def test_cluster_features_cli_refusals(tmp_path, monkeypatch, capsys):
    """Every exit-1 case, each with its message, all before anything touches the device (fit and assign would raise)."""
    import infer

    def boom(*a, **k):
        raise AssertionError('a refused command line reached the GPU entry')

    monkeypatch.setattr(km, 'fit', boom)
    monkeypatch.setattr(km, 'assign', boom)
    feats = torch.from_numpy(planted_int(32, 60, 8).reshape(32, 3, 4, 5)).half()
    src = tmp_path / 'v_features6.npy'
    infer.save_features({'t': feats}, src)
    out = lambda: capsys.readouterr().out                     # noqa: E731
    out()
    for bad in ('1', '65', '0'):
        assert _main(['--features', str(src), '--clusters', bad]) == 1
        assert f'Invalid argument for --clusters: {bad} is outside 2..64' in out()
    assert _main(['--features', str(src)]) == 1               # neither --clusters nor --centroids
    assert 'Invalid argument for --clusters' in out()
    assert _main(['--features', str(src), '--clusters', '61']) == 1          # 60 voxels
    assert 'Invalid argument for --clusters: 61 clusters of 60 voxels' in out()
    np.save(tmp_path / 'odd_features.npy', np.zeros((48, 3, 4, 5), np.float16))
    assert _main(['--features', str(tmp_path / 'odd_features.npy'), '--clusters', '4']) == 1
    assert 'Invalid argument for --features: F = 48' in out()
    np.save(tmp_path / 'wide_features.npy', np.zeros((1056, 3, 4, 5), np.float16))
    assert _main(['--features', str(tmp_path / 'wide_features.npy'), '--clusters', '4']) == 1
    assert 'Invalid argument for --features: F = 1056' in out()
    assert _main(['--features', str(tmp_path / 'nope.npy'), '--clusters', '4']) == 1
    assert 'Invalid argument for --features (File does not exist)' in out()
    (tmp_path / 'v_features6_clusters4.npy').write_bytes(b'')
    assert _main(['--features', str(src), '--clusters', '4']) == 1
    assert 'Cache file already exists' in out()
    (tmp_path / 'v_features6_clusters5_centroids.npz').write_bytes(b'')      # the centroid file is protected like the volume
    assert _main(['--features', str(src), '--clusters', '5']) == 1
    assert 'Cache file already exists' in out()
    assert _main(['--features', str(src), '--clusters', '4', '--output', str(tmp_path / 'missing_dir' / 'l.npy')]) == 1
    assert 'Invalid argument for --output (Cannot write to location)' in out()
    assert _main(['--features', str(src), '--clusters', '4', '--max-iter', '0']) == 1
    assert 'Invalid argument for --max-iter' in out()
    assert _main(['--features', str(src), '--clusters', '4', '--tol', '-1']) == 1
    assert 'Invalid argument for --tol' in out()
    # --centroids: a missing file, a foreign file, another F, a --clusters that disagrees
    assert _main(['--features', str(src), '--centroids', str(tmp_path / 'nope.npz')]) == 1
    assert 'Invalid argument for --centroids' in out()
    np.savez(tmp_path / 'other.npz', centroids=np.zeros((2, 32), np.float32))
    assert _main(['--features', str(src), '--centroids', str(tmp_path / 'other.npz')]) == 1
    assert 'Invalid argument for --centroids' in out()
    (tmp_path / 'broken.npz').write_bytes(b'PK\x03\x04 not a zip archive')
    np.save(tmp_path / 'array.npy', np.zeros((4, 32), np.float32))
    for bad in ('broken.npz', 'array.npy'):
        assert _main(['--features', str(src), '--centroids', str(tmp_path / bad)]) == 1
        assert 'Invalid argument for --centroids' in out(), bad
    vt.save_clustering(_clustering(4, 64), tmp_path / 'c64.npz')
    assert _main(['--features', str(src), '--centroids', str(tmp_path / 'c64.npz')]) == 1
    assert 'Invalid argument for --centroids: fitted on F = 64' in out()
    vt.save_clustering(_clustering(4, 32), tmp_path / 'c32.npz')
    assert _main(['--features', str(src), '--centroids', str(tmp_path / 'c32.npz'), '--clusters', '5']) == 1
    assert 'Invalid argument for --clusters: 5 asked for' in out()


def test_cluster_features_cli_writes_both_files(tmp_path, monkeypatch, capsys):
    """The accepted command line with the GPU functions replaced: names, dtypes, what --centroids skips."""
    import infer
    calls = []

    def fake_fit(feat, c, seed=0, max_iter=50, tol=1e-4, init=None):
        calls.append(('fit', c, seed, max_iter, tol))
        labels = (torch.arange(int(np.prod(feat.shape[1:]))) % c).to(torch.uint8).reshape(feat.shape[1:])
        return labels, _clustering(c, feat.shape[0])

    def fake_assign(feat, centroids):
        calls.append(('assign', int(centroids.shape[0])))
        return (torch.arange(int(np.prod(feat.shape[1:]))) % centroids.shape[0]).to(torch.uint8).reshape(feat.shape[1:])

    monkeypatch.setattr(km, 'fit', fake_fit)
    monkeypatch.setattr(km, 'assign', fake_assign)
    feats = torch.from_numpy(planted_int(32, 60, 8).reshape(32, 3, 4, 5)).half()
    src = tmp_path / 'v_features6.npy'
    infer.save_features({'t': feats}, src)
    assert _main(['--features', str(src), '--clusters', '4', '--seed', '3', '--max-iter', '9', '--tol', '0.5']) == 0
    assert calls == [('fit', 4, 3, 9, 0.5)]
    vol = np.load(tmp_path / 'v_features6_clusters4.npy')     # a bare array: no pickle needed
    assert vol.dtype == np.uint8 and vol.shape == (3, 4, 5)
    assert vt.load_clustering(tmp_path / 'v_features6_clusters4_centroids.npz').centroids.shape == (4, 32)
    line = capsys.readouterr().out
    assert '(32, 3, 4, 5)' in line and '(3, 4, 5)' in line and '3 iterations' in line and 'inertia 12.5' in line and 'sizes [15, 15, 15, 15]' in line
    calls.clear()
    assert _main(['--features', str(src), '--centroids', str(tmp_path / 'v_features6_clusters4_centroids.npz'),
                  '--output', str(tmp_path / 'again.npy')]) == 0
    assert calls == [('assign', 4)] and not (tmp_path / 'again_centroids.npz').exists()
    assert np.array_equal(np.load(tmp_path / 'again.npy'), vol)
    assert _main(['--features', str(src), '--clusters', '4', '--overwrite']) == 0
