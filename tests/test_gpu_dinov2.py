"""GPU: DINOv2 (patch 14, LayerScale folded into the weights) through the HIP engine.

* vittf_patch_embed at P = 14 (patch_embed14_mfma_kernel at D = 384, patch_embed_kernel<14> otherwise) against the fp64
  folded conv over the same fp32 pixels and weights: 4e-6 of a row's largest value (fp32 accumulation over 196 taps).
* The engine against the fixtures made with the reference's own compute_qkv (tests/golden/make_golden_dinov2.py).
* Full size: 896 x 896 images (N = 4097) of ViT-S/14 and of 3-block D = 768 / 1024 models against tests/dinov2_ref.py.
* ViT-L/14 at the engine batch extract.engine_batch_for picks (255 slices of N = 4097): accepted, and bit-equal to a small batch.
* infer.py --dino2-model end to end; a 1024-wide feature volume through compute_similarities.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_tf_amd as vt
from vit_tf_amd import _lib
from dinov2_ref import build_dinov2
from helpers import load_golden, rel_fro
from oracle import feature_volume as ofv, similarity as osim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dinov2_sd(arch, seed):
    return vt.synthetic_state_dict(arch, seed, stored_grid=vt.weights.DINOV2_STORED_GRID, layer_scale=True)


# ------------------------------------------------------------------------------------------ patch embedding, P = 14
@pytest.mark.parametrize('d', [128, 384, 768, 1024])
@pytest.mark.parametrize('shape,im_sz', [((20, 12, 30), (14, 28, 42)),            # dim 0 down, dims 1 / 2 up, non-square
                                         ((40, 150, 150), (140, 140, 168))])      # 150 x 101 / 40 x 121 rows: ragged last tiles
def test_patch_embed14(gpu, d, shape, im_sz):
    arch = (d, 1, d // 64, 14)
    sd = _dinov2_sd(arch, 3)
    model = vt.HipViT(sd, arch, 'fp16')
    vol = (torch.rand(shape, generator=_gen(d + shape[0])) * 300 - 100).half().float()
    w_t, b = vt.fold_patch_embed(sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'])
    dvol = vt.DeviceVolume(vol, gpu)
    lo, hi = vol.min(), vol.max()
    for axis in ('z', 'y', 'x'):
        sl, (a, bb) = ofv.AXIS_DIMS[axis]
        rows, cols = im_sz[a], im_sz[bb]
        img = ((vol.permute(sl, a, bb) - lo) / (hi - lo))[:, None]                 # the kernel's fp32 pixel arithmetic
        x_in = F.interpolate(img, size=(rows, cols), mode='nearest')
        taps = F.unfold(x_in.double(), kernel_size=14, stride=14)                  # (S, 196, f0 * f1), k = 14 row + col
        pos = vt.interpolate_pos_embed(sd['pos_embed'], rows, cols, 14)[0].double()
        ref = torch.einsum('skp,kd->spd', taps, w_t.double()) + b.double() + pos[1:]
        cls = (sd['cls_token'][0, 0].double() + pos[0]).expand(ref.shape[0], 1, d)
        ref = torch.cat([cls, ref], dim=1)
        n = ref.shape[0]
        view = dvol.view(axis, im_sz)
        pstruct, _, _ = model.pos_for(rows, cols)
        out = torch.full((n + 1, ref.shape[1], d), 7.0, device=gpu)
        _lib.check(model.lib.vittf_patch_embed(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view), 0,
                                               n, _lib.ptr(out), _lib.stream_ptr()))
        got = out.cpu()
        assert (got[n:] == 7.0).all(), 'wrote past the last row'
        err = (got[:n].double() - ref).abs().amax(dim=-1)
        # both kernels accumulate in fp32 (the generic one 196 FMAs, the matrix-core one 42 MFMA results over exact split
        # products): at K = 196 that rounding alone reaches 1.2e-6 of a row's largest value on the MI355X, for either kernel
        # -- 1e-6 is not reachable by an fp32 sum here; held to 4e-6
        bound = 4e-6 * ref.abs().amax(dim=-1)
        assert bool((err <= bound).all()), (axis, float((err / bound).max()))
        assert _lib.kernel_name('patch_embed') == ('patch_embed14_mfma_kernel' if d == 384 else 'patch_embed_kernel<14>')
        if n > 3:      # rows are independent of the tiling: a sub-range writes the same bits
            part = torch.zeros(2, ref.shape[1], d, device=gpu)
            _lib.check(model.lib.vittf_patch_embed(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view),
                                                   1, 2, _lib.ptr(part), _lib.stream_ptr()))
            assert torch.equal(part.cpu(), got[1:3])


# ------------------------------------------------------------------------------------------ reference-made fixtures
@pytest.mark.parametrize('dt,tol', [('fp16', 1e-3), ('bf16', 8e-3)])
@pytest.mark.parametrize('name', ['dinov2_d128.npz', 'dinov2_d384.npz'])
def test_engine_matches_reference_fixtures(gpu, golden_dir, name, dt, tol):
    import infer
    rec = load_golden(golden_dir, name)
    arch = tuple(int(v) for v in rec['arch'])
    sd = _dinov2_sd(arch, int(rec['seed']))
    assert abs(vt.weights.state_dict_checksum(sd) - float(rec['weights_checksum'])) <= 1e-9 * abs(float(rec['weights_checksum']))
    model = vt.HipViT(sd, arch, dt)
    vol = torch.from_numpy(rec['vol'])
    fos = int(rec['fos'])
    im_sz = tuple(int(v) for v in rec['im_sz'])
    _lib.profiler_enable(True)
    try:
        for ax in 'zyx':
            got = vt.feature_volume(vol, model, fos, ax).cpu()
            ref = torch.from_numpy(rec[f'k_{ax}'])
            assert got.shape == ref.shape and rel_fro(got, ref) < tol, (ax, rel_fro(got, ref))
        torch.cuda.synchronize()
        prof = _lib.profiler_collect()
    finally:
        _lib.profiler_enable(False)
    got = vt.feature_volume(vol, model, fos, 'all').cpu()
    ref = torch.from_numpy(rec['k_all'])
    assert got.shape == ref.shape and rel_fro(got, ref) < tol, rel_fro(got, ref)
    qkv = infer.compute_qkv(vol, model, 14, im_sz, slice_along='z', return_keys=['q', 'k', 'v'])
    for key in 'qkv':
        ref = torch.from_numpy(rec[f'{key}_z'])
        assert qkv[key].shape == ref.shape and rel_fro(qkv[key], ref) < tol, (key, rel_fro(qkv[key], ref))
    if arch[0] == 384:
        assert prof['mlp'][1] > 0, 'the block tail did not run'
        assert _lib.kernel_name('patch_embed') == 'patch_embed14_mfma_kernel'
        assert model.weights.tail_packed and model.weights.qkv_packed


# ------------------------------------------------------------------------------------------ full size, N = 4097
@pytest.mark.parametrize('arch,seed', [('vits14', 0), ((768, 3, 12, 14), 1), ((1024, 3, 16, 14), 2)])
def test_fullsize_896_images(gpu, arch, seed):
    sd = _dinov2_sd(arch, seed)
    model = vt.HipViT(sd, arch, 'fp16')
    vol = (torch.rand((2, 512, 512), generator=_gen(seed)) * 2 - 1).half().float()
    im_sz = (14, 896, 896)                         # x slices: 512 x 512 -> 896 x 896 images, 64 x 64 tokens
    dvol = vt.DeviceVolume(vol, gpu)
    got = vt.k_slices(model, dvol, 'x', im_sz, 0, 2).cpu()
    assert got.shape == (2, 4096, model.embed_dim)
    oracle = build_dinov2(arch, sd)
    imgs = ofv.normalized_slices(vol, 'x')
    with torch.no_grad():
        ref = torch.cat([oracle.last_block_k(F.interpolate(imgs[i:i + 1], size=(896, 896), mode='nearest'))[:, 1:].half()
                         for i in range(2)])
    err = rel_fro(got, ref)
    assert err < 1e-3, err


def test_vitl14_at_the_default_engine_batch(gpu):
    d = 1024
    eb = vt.extract.engine_batch_for(4097, d)
    assert eb == 255
    sd = vt.synthetic_state_dict('vitl14', 4)
    model = vt.HipViT(sd, 'vitl14', 'fp16')
    vol = (torch.rand((eb + 2, 64, 64), generator=_gen(4)) * 2 - 1).half().float()
    im_sz = (14, 896, 896)
    dvol = vt.DeviceVolume(vol, gpu)
    big = vt.k_slices(model, dvol, 'x', im_sz, 0, eb)                 # one engine call of 255 x 4097 rows
    assert big.shape == (eb, 4096, d) and bool(torch.isfinite(big).all())
    for s0, s1, small in ((0, 3, 3), (eb - 4, eb, 2)):
        got = vt.k_slices(model, dvol, 'x', im_sz, s0, s1, engine_batch=small)
        assert torch.equal(got, big[s0:s1]), (s0, s1)
    del big
    # one slice more than the cap is refused by the engine rather than computed with wrapped offsets
    with pytest.raises(vt.VittfError):
        vt.k_slices(model, dvol, 'x', im_sz, 0, eb + 2, engine_batch=eb + 2)


# ------------------------------------------------------------------------------------------ CLI + similarity
def test_infer_cli_dinov2_end_to_end(gpu, tmp_path):
    vol = (torch.rand((20, 24, 28), generator=_gen(5)) * 2 - 1).half().float()
    np.save(tmp_path / 'vol.npy', vol.numpy())
    env = dict(os.environ)
    env.pop('VITTF_WEIGHTS', None)
    env['TORCH_HOME'] = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, 'infer.py'), '--data-path', str(tmp_path / 'vol.npy'), '--dino2-model', 'vits14',
           '--synthetic-weights', '0', '--feature-output-size', '4']
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = tmp_path / 'vol_vits14_all_features4.npy'
    saved = np.load(out, allow_pickle=True)[()]['k']
    model = vt.HipViT(vt.synthetic_state_dict('vits14', 0), 'vits14', 'fp16')
    want = vt.feature_volume(vol, model, 4, 'all').cpu().numpy()
    assert saved.dtype == np.float16 and saved.shape == want.shape
    assert np.array_equal(saved.view(np.int16), want.view(np.int16))


def test_similarities_on_1024_features(gpu):
    g = _gen(6)
    feat = F.normalize(torch.randn((1024, 8, 8, 8), generator=g), dim=0)
    feat = F.normalize((feat + 0.8 * feat[:, 2:3, 3:4, 4:5]).half().float(), dim=0).half()
    vol = torch.zeros((16, 16, 16))
    ann = {'a': torch.tensor([[3, 4, 5], [9, 10, 12]]), 'b': torch.tensor([[12, 8, 1], [1, 1, 1], [5, 15, 11]])}
    sims = vt.compute_similarities(vol, feat, ann)
    want = osim.similarity_maps(tuple(vol.shape), feat.float(), ann)
    for k in ann:
        d = (sims[k].int() - want[k].int()).abs()
        assert int(torch.minimum(d, 256 - d).max()) <= 1, k
