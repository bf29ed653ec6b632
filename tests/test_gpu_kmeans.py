"""GPU: k-means clustering of a feature volume -- vittf_kmeans_assign, vittf_kmeans_sums, vit_tf_amd.kmeans and
cluster_features.py.

Exact cases use integer-valued data (pca_data.planted_int, magnitude <= 8) with centroids that are columns of it: every
score m_c . x - 0.5 |m_c|^2 is a half-integer below 2^24 and every per-cluster sum of a run of VITTF_GRAM_RUN voxels an integer
below 2^24, so fp32 is exact in any order and labels, winning scores, sums and counts must equal the fp64 results bit for bit.
Real-valued cases are held to worst-case fp32 bounds written out below.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
from pca_data import planted_int, raw_planted

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = _lib.GRAM_RUN
km = vt.kmeans

# 1 and 2 centroid blocks, the c = 32 / 33 edge, a partial last workgroup, unaligned rows (n = 250, 257)
CASES = ((2, 32, 250), (5, 96, 1000), (32, 384, 257), (33, 384, 4104), (64, 1024, 257))


def _dev16(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).to(gpu)


def _raw_assign(dev, cent, half, gpu):
    """The raw entry: (labels uint8 [n], best fp32 [n]) as numpy arrays; cent fp64 [c][f], half fp64 [c] or None."""
    f, n = dev.shape
    c = cent.shape[0]
    cdev = torch.from_numpy(cent).float().to(gpu)
    hdev = torch.from_numpy(half).float().to(gpu) if half is not None else None
    labels = torch.full((n,), 77, dtype=torch.uint8, device=gpu)
    best = torch.full((n,), float('nan'), dtype=torch.float32, device=gpu)
    rc = _lib.load().vittf_kmeans_assign(_lib.ptr(dev), f, n, _lib.ptr(cdev), _lib.ptr(hdev), c, _lib.ptr(labels), _lib.ptr(best),
                                         _lib.stream_ptr())
    assert rc == 0
    return labels.cpu().numpy(), best.cpu().numpy()


# ---------------------------------------------------------------------------- 1. assignment, exact
def _exact_case(c, f, n, dup):
    x = planted_int(f, n, 17 * c + f + n)
    rng = np.random.default_rng(c + f + n)
    cent = x[:, rng.choice(n, size=c, replace=False)].T.copy()
    if dup:          # equal scores inside a lane, across the lane halves (rows 4..7 of a block are on lanes 32..63) and across blocks
        cent[1] = cent[0]
        cent[c - 1] = cent[5] if c == 33 else cent[2]        # c = 33: block 1 half 0 <- block 0 half 1; c = 64: block 1 half 1 <- block 0 half 0
    half = 0.5 * (cent * cent).sum(1)
    scores = cent @ x - half[:, None]
    assert np.array_equal(scores.astype(np.float32).astype(np.float64), scores) and np.abs(2 * scores).max() < 2 ** 24
    return x, cent, half, scores


@pytest.mark.parametrize('c,f,n', CASES)
def test_assign_exact(gpu, c, f, n):
    x, cent, half, scores = _exact_case(c, f, n, False)
    labels, best = _raw_assign(_dev16(x, gpu), cent, half, gpu)
    assert np.array_equal(labels, scores.argmax(0).astype(np.uint8))          # the first of equal maxima: the lowest index
    assert np.array_equal(best.astype(np.float64), scores.max(0))


@pytest.mark.parametrize('c,f,n', [(33, 384, 4104), (64, 1024, 257)])
def test_assign_exact_with_equal_scores(gpu, c, f, n):
    """Centroid 1 is a copy of centroid 0, centroid c - 1 a copy of one in the other lane half and the other block: the
    copies never win, their originals do (the voxels the centroids were taken from score highest there)."""
    x, cent, half, scores = _exact_case(c, f, n, True)
    want = scores.argmax(0)
    src = 5 if c == 33 else 2
    assert not (want == 1).any() and not (want == c - 1).any() and (want == 0).any() and (want == src).any()
    labels, best = _raw_assign(_dev16(x, gpu), cent, half, gpu)
    assert np.array_equal(labels, want.astype(np.uint8))
    assert np.array_equal(best.astype(np.float64), scores.max(0))


def test_assign_exact_on_a_view_at_a_2_byte_aligned_offset_and_without_half_sq(gpu):
    c, f, n = 5, 96, 1000
    x, cent, half, scores = _exact_case(c, f, n, False)
    buf = torch.full((f * n + 16,), 99.0, dtype=torch.float16, device=gpu)
    buf[1:1 + f * n] = _dev16(x, gpu).reshape(-1)
    view = buf[1:1 + f * n].view(f, n)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    labels, best = _raw_assign(view, cent, half, gpu)
    assert np.array_equal(labels, scores.argmax(0).astype(np.uint8)) and np.array_equal(best.astype(np.float64), scores.max(0))
    labels, best = _raw_assign(view, cent, None, gpu)         # NULL half_sq: zeros
    dots = cent @ x
    assert np.array_equal(labels, dots.argmax(0).astype(np.uint8)) and np.array_equal(best.astype(np.float64), dots.max(0))
    # the Python entry on the same data, on a volume shape: fp64 half_sq rounded once is exact here
    got = km.assign(_dev16(x, gpu).reshape(f, 10, 10, 10), torch.from_numpy(cent).float())
    assert got.dtype == torch.uint8 and got.shape == (10, 10, 10)
    assert np.array_equal(got.cpu().numpy().reshape(-1), scores.argmax(0).astype(np.uint8))


# ---------------------------------------------------------------------------- 2. assignment, real-valued
REAL_CASES = ((5, 96, 1000), (17, 64, 4104), (33, 384, 4104), (64, 1024, 257))


def _lloyd(x, cent, iters):
    """fp64 Lloyd iterations in numpy; an empty cluster keeps its centroid.  Returns (centroids, labels of the last assignment)."""
    cent = cent.copy()
    labels = None
    for _ in range(iters):
        labels = (cent @ x - 0.5 * (cent * cent).sum(1)[:, None]).argmax(0)
        for k in range(cent.shape[0]):
            if (labels == k).any():
                cent[k] = x[:, labels == k].mean(1)
    return cent, labels


@functools.lru_cache(maxsize=None)
def _real_case(c, f, n, kind):
    """x fp16(0.25 raw_planted) as float64; centroids as fp32-representable float64: c random columns ('columns') or those
    after three fp64 Lloyd iterations ('lloyd'); h = fp32(0.5 |m|^2); the fp64 scores and the per-score bound
        e_cv = (F + 8) 2^-24 (sum_f |m_cf x_fv| + |h_c|) + 2^-25 sum_f |x_fv|
    (pca_data.project_bound without the rounding of the result)."""
    x = (0.25 * raw_planted(f, n, 0)).astype(np.float16).astype(np.float64)
    rng = np.random.default_rng(100 + c)
    cent = x[:, rng.choice(n, size=c, replace=False)].T.copy()
    if kind == 'lloyd':
        cent, _ = _lloyd(x, cent, 3)
    cent = cent.astype(np.float32).astype(np.float64)
    h = (0.5 * (cent * cent).sum(1)).astype(np.float32).astype(np.float64)
    scores = cent @ x - h[:, None]
    bound = (f + 8) * 2.0 ** -24 * (np.abs(cent) @ np.abs(x) + np.abs(h)[:, None]) + 2.0 ** -25 * np.abs(x).sum(0)[None, :]
    return x, cent, h, scores, bound


@pytest.mark.parametrize('kind', ['columns', 'lloyd'])
@pytest.mark.parametrize('c,f,n', REAL_CASES)
def test_assign_real_valued(gpu, c, f, n, kind):
    """A voxel is decided when its fp64 margin (best minus second best) exceeds 2 max_c e_cv: it must carry the fp64 label.
    Every other voxel's label must score within e_label + e_best of the fp64 best.  At most 2 % of the voxels may be
    undecided (a condition on the data: 0 - 1.2 % on these inputs)."""
    x, cent, h, scores, bound = _real_case(c, f, n, kind)
    got = km.assign(_dev16(x, gpu), torch.from_numpy(cent).float()).cpu().numpy().astype(np.int64)
    assert got.shape == (n,) and got.max() < c
    order = np.sort(scores, axis=0)
    want = scores.argmax(0)
    decided = order[-1] - order[-2] > 2 * bound.max(0)
    share = 1.0 - float(decided.mean())
    v = np.arange(n)
    gap = scores[want, v] - scores[got, v]
    print(f'assign c={c} f={f} n={n} {kind}: undecided {100 * share:.2f} %, labels differing from fp64 {int((got != want).sum())}, '
          f'max gap / allowed {float((gap / (bound[got, v] + bound[want, v])).max()):.3f}')
    assert share <= 0.02
    assert np.array_equal(got[decided], want[decided])
    assert (gap <= bound[got, v] + bound[want, v]).all()


# ---------------------------------------------------------------------------- 3. sums, exact
def _labels(n, c, seed):
    """Random uint8 labels in 0..c-1 with cluster c // 2 left empty and about 5 % of the voxels labelled 255."""
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.setdiff1d(np.arange(c), [c // 2]), size=n).astype(np.uint8)
    lab[rng.random(n) < 0.05] = 255
    return lab


def _check_sums_exact(gpu, c, f, n, dev=None, x=None):
    x = planted_int(f, n, 3 * c + f + n) if x is None else x
    lab = _labels(n, c, c + n)
    sums, counts = km.cluster_sums(_dev16(x, gpu) if dev is None else dev, torch.from_numpy(lab).to(gpu), c)
    assert sums.dtype == torch.float64 and sums.shape == (c, f) and counts.dtype == torch.int64 and counts.shape == (c,)
    want = np.stack([x[:, lab == k].sum(1) for k in range(c)])
    assert np.array_equal(sums.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(lab[lab < c], minlength=c))
    assert int(counts[c // 2]) == 0 and not sums[c // 2].any()
    return sums, counts


@pytest.mark.parametrize('c,f,n', CASES + ((5, 96, 3 * RUN + 24), (33, 384, 3 * RUN + 24), (64, 768, 1000), (5, 768, 1000)))
def test_sums_exact(gpu, c, f, n):
    _check_sums_exact(gpu, c, f, n)


def test_sums_exact_on_a_view_and_with_labels_between_c_and_32(gpu):
    c, f, n = 5, 96, 1000
    x = planted_int(f, n, 41)
    buf = torch.full((f * n + 16,), 99.0, dtype=torch.float16, device=gpu)
    buf[3:3 + f * n] = _dev16(x, gpu).reshape(-1)
    view = buf[3:3 + f * n].view(f, n)
    assert view.data_ptr() % 16 == 6
    _check_sums_exact(gpu, c, f, n, dev=view, x=x)
    lab = np.random.default_rng(0).integers(0, 40, size=n).astype(np.uint8)        # labels 5..39 contribute nowhere
    sums, counts = km.cluster_sums(view, torch.from_numpy(lab).to(gpu), c)
    assert np.array_equal(sums.cpu().numpy(), np.stack([x[:, lab == k].sum(1) for k in range(c)]))
    assert np.array_equal(counts.cpu().numpy(), np.bincount(lab, minlength=40)[:c])


def test_sums_exact_beyond_the_workspace_spans(gpu):
    """More runs than the workspace has spans: a workgroup then walks two runs and adds the second into its fp64 partial
    (read-add-write), a path no smaller volume reaches.  A second call gives the same bytes on that path too."""
    f, c, n = 32, 3, _lib.KMEANS_SPANS * RUN + 40
    first = _check_sums_exact(gpu, c, f, n)
    again = _check_sums_exact(gpu, c, f, n)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------- 4. sums, real-valued
@pytest.mark.parametrize('c,f,n', [(17, 64, 4104), (33, 384, 4104), (64, 1024, 257)])
def test_sums_real_valued_within_the_fp32_bound(gpu, c, f, n):
    """Every entry within (min(n_c, VITTF_GRAM_RUN) + 1) 2^-24 sum_{v in c} |x_fv| of the fp64 sum: the worst case of an fp32
    sum of min(n_c, RUN) exact terms in any order.  Two calls give the same bytes (no floating-point atomics)."""
    x, cent, h, scores, _ = _real_case(c, f, n, 'lloyd')
    lab = scores.argmax(0).astype(np.uint8)
    dev, ldev = _dev16(x, gpu), torch.from_numpy(lab).to(gpu)
    sums, counts = km.cluster_sums(dev, ldev, c)
    sums2, counts2 = km.cluster_sums(dev, ldev, c)
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, np.bincount(lab, minlength=c))
    worst = 0.0
    for k in range(c):
        xs = x[:, lab == k]
        bound = (min(xs.shape[1], RUN) + 1) * 2.0 ** -24 * np.abs(xs).sum(1)
        err = np.abs(sums[k] - xs.sum(1))
        assert (err <= bound).all(), k
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f'sums c={c} f={f} n={n}: max err / bound {worst:.3e}')


# ---------------------------------------------------------------------------- 5. fit end to end
@functools.lru_cache(maxsize=None)
def _blobs(f, n, c):
    """c well-separated blobs on a lattice: integer fp16 centres in -8..8 drawn once, noise in multiples of 1/64 up to 0.25
    (|noise vector| <= 0.25 sqrt(F), centres tens apart), cluster sizes all different.  Every value is a multiple of 1/64 below
    8.25, so any fp32 sum over a run of 2048 voxels is exact (528 x 2048 < 2^24): the kernel's sums carry no rounding and the
    1e-9 checks below test the host arithmetic, not the luck of a rounding."""
    rng = np.random.default_rng(1000 + f)
    centres = rng.integers(-8, 9, size=(c, f)).astype(np.float64)
    dist = np.linalg.norm(centres[:, None] - centres[None], axis=2) + 1e9 * np.eye(c)
    weights = np.arange(1, c + 1) / (c * (c + 1) / 2)
    planted = rng.permutation(np.repeat(np.arange(c), np.diff(np.rint(np.concatenate([[0], np.cumsum(weights)]) * n).astype(int))))
    x = centres[planted].T + rng.integers(-16, 17, size=(f, n)) / 64.0
    assert planted.size == n and len(set(np.bincount(planted).tolist())) == c and 0.25 * np.sqrt(f) < 0.1 * dist.min() / 2
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x)
    return x, planted


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize('f,n,c', [(96, 1000, 4), (384, 4104, 7)])
def test_fit_end_to_end(gpu, f, n, c):
    seed = 0
    x, planted = _blobs(f, n, c)
    init = km.init_centroids(x, c, seed)
    ref_cent, ref_labels = _lloyd(x, init.double().numpy(), 10)
    assert _same_partition(ref_labels, planted), 'the fp64 reference does not recover the planted partition: choose another seed'
    dev = _dev16(x, gpu)
    labels, res = km.fit(dev, c, seed=seed)
    assert labels.dtype == torch.uint8 and labels.shape == (n,) and labels.is_cuda
    lab = labels.cpu().numpy()
    assert _same_partition(lab, planted)
    sizes = np.bincount(lab, minlength=c)
    assert (np.diff(sizes) <= 0).all() and np.array_equal(res.counts.numpy(), sizes)      # numbered by descending count
    means = np.stack([x[:, lab == k].mean(1) for k in range(c)])
    cent = res.centroids.double().numpy()
    assert res.centroids.dtype == torch.float32 and res.centroids.shape == (c, f)
    assert (np.linalg.norm(cent - means, axis=1) <= 1e-6 * np.linalg.norm(means, axis=1)).all()
    direct = float(((x - means[lab].T) ** 2).sum())
    hist = res.inertia_history.numpy()
    print(f'fit f={f} n={n} c={c}: {res.n_iter} iterations, inertia {float(res.inertia):.6f} (direct {direct:.6f}), history {hist}')
    assert res.inertia.dtype == torch.float64 and abs(float(res.inertia) - direct) <= 1e-9 * direct
    assert hist.shape == (res.n_iter,) and hist[-1] == float(res.inertia) and (np.diff(hist) <= 1e-9 * hist[:-1]).all()
    assert res.converged is True and 1 <= res.n_iter < 50
    labels2, res2 = km.fit(dev, c, seed=seed)
    assert torch.equal(labels, labels2)
    for name in vt.Clustering._fields:
        assert torch.equal(torch.as_tensor(getattr(res, name)), torch.as_tensor(getattr(res2, name))), name
    # the same start handed in, and a volume shape
    labels3, res3 = km.fit(dev.reshape(f, -1, 2), c, init=init)
    assert labels3.shape == (n // 2, 2) and torch.equal(labels3.reshape(-1), labels) and torch.equal(res3.centroids, res.centroids)


# ---------------------------------------------------------------------------- 6. command line
def _run(args, env, timeout=300):
    return subprocess.run([sys.executable, *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_cluster_features_cli(gpu, tmp_path):
    import infer
    f, n, c = 96, 1000, 4
    x, planted = _blobs(f, n, c)
    env = dict(os.environ, PYTHONPATH=ROOT)
    src = tmp_path / 'v_features10.npy'
    infer.save_features({'t': torch.from_numpy(x).half().reshape(f, 10, 10, 10)}, src)
    r = _run(['cluster_features.py', '--features', str(src), '--clusters', str(c)], env)
    assert r.returncode == 0, r.stderr + r.stdout
    vol_path, cent_path = tmp_path / f'v_features10_clusters{c}.npy', tmp_path / f'v_features10_clusters{c}_centroids.npz'
    vol = np.load(vol_path)
    assert vol.dtype == np.uint8 and vol.shape == (10, 10, 10) and _same_partition(vol.reshape(-1), planted)
    saved = vt.load_clustering(cent_path)
    assert saved.centroids.shape == (c, f) and saved.converged and np.array_equal(saved.counts.numpy(), np.bincount(vol.reshape(-1)))
    assert str(saved.counts.tolist()) in r.stdout
    # the in-process fit gives the same bytes as the command line
    labels, res = km.fit(torch.from_numpy(x).half().reshape(f, 10, 10, 10), c)
    assert np.array_equal(labels.cpu().numpy(), vol) and torch.equal(res.centroids, saved.centroids)
    # --centroids: only the assignment, the same volume bit for bit, no second centroid file
    r = _run(['cluster_features.py', '--features', str(src), '--centroids', str(cent_path), '--output', str(tmp_path / 'again.npy')], env)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(tmp_path / 'again.npy', 'rb').read() == open(vol_path, 'rb').read() and not (tmp_path / 'again_centroids.npz').exists()
    # a reduced file from reduce_features.py is taken as it is
    r = _run(['reduce_features.py', '--features', str(src), '--components', '32'], env)
    assert r.returncode == 0, r.stderr + r.stdout
    r = _run(['cluster_features.py', '--features', str(tmp_path / 'v_features10_pca32.npy'), '--clusters', str(c)], env)
    assert r.returncode == 0, r.stderr + r.stdout
    red = np.load(tmp_path / f'v_features10_pca32_clusters{c}.npy')
    assert red.dtype == np.uint8 and red.shape == (10, 10, 10) and red.max() < c
