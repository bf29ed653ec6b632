"""GPU: the DINOv2 register models (R register tokens behind CLS, dropped with it) through the HIP engine.

* vittf_patch_embed_reg at P = 8 / 14 / 16, D = 128 .. 1024, R = 4 and 1 against the fp64 folded conv (test_patch_embed14's
  reference and bound): register rows bit-equal to register_tokens, nothing behind the last row, a sub-range of slices
  writes the same bits, R = 0 is vittf_patch_embed.
* vittf_gemm_kfeat_parts_reg with R = 4 against vittf_gemm_kfeat_parts on the same rows without the register rows, bit for
  bit, on the tiled and on the persistent kernel.
* The engine against tests/golden/dinov2_reg_*.npz (made by tests/dinov2_reg_ref.py, which the CPU tests hold against
  transformers.Dinov2WithRegistersModel).
* Full size: 896 x 896 images, N = 4101 (5 keys in the last 64-key tile), ViT-S/14-reg and 3-block D = 768 / 1024 models,
  the fp8 attention path at D = 768.
* qkv_features == three k_features calls; infer.py --dino2-model vits14_reg end to end; the engine's alternative paths.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_tf_amd as vt
from vit_tf_amd import _lib
import dinov2_reg_ref as rr
from helpers import load_golden, rel_fro
from oracle import feature_volume as ofv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5a5a
INVALID = -1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------ 8. patch embedding
EMBED_KERNEL = {(384, 8): 'patch_embed_mfma_kernel', (384, 14): 'patch_embed14_mfma_kernel'}


@pytest.mark.parametrize('registers', [4, 1])
@pytest.mark.parametrize('patch', [8, 14, 16])
@pytest.mark.parametrize('d', [128, 384, 768, 1024])
@pytest.mark.parametrize('shape,grid', [((20, 12, 30), (1, 2, 3)),              # dim 0 down, dims 1 / 2 up, non-square
                                        ((40, 150, 150), (10, 10, 12))])         # 150 x 101 / 40 x 121 rows: ragged last tiles
def test_patch_embed_reg(gpu, d, patch, registers, shape, grid):
    im_sz = tuple(v * patch for v in grid)                   # test_patch_embed14's (14, 28, 42) and (140, 140, 168) at P = 14
    arch = (d, 1, d // 64, patch)
    sd = rr.synthetic_reg(arch, 3, registers)
    model = vt.HipViT(sd, arch, 'fp16')
    assert model.num_register_tokens == registers
    reg = sd['register_tokens'][0]
    reg_dev = reg.to(gpu).contiguous()
    vol = (torch.rand(shape, generator=_gen(d + shape[0])) * 300 - 100).half().float()
    w_t, b = vt.fold_patch_embed(sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'])
    dvol = vt.DeviceVolume(vol, gpu)
    lo, hi = vol.min(), vol.max()
    for axis in ('z', 'y', 'x'):
        sl, (a, bb) = ofv.AXIS_DIMS[axis]
        rows, cols = im_sz[a], im_sz[bb]
        img = ((vol.permute(sl, a, bb) - lo) / (hi - lo))[:, None]                 # the kernel's fp32 pixel arithmetic
        x_in = F.interpolate(img, size=(rows, cols), mode='nearest')
        taps = F.unfold(x_in.double(), kernel_size=patch, stride=patch)            # (S, P * P, f0 * f1)
        pos = rr.interpolate_pos_embed_reg(sd['pos_embed'], rows, cols, patch)[0].double()
        ref = torch.einsum('skp,kd->spd', taps, w_t.double()) + b.double() + pos[1:]
        n = ref.shape[0]
        cls = (sd['cls_token'][0, 0].double() + pos[0]).expand(n, 1, d)
        ref = torch.cat([cls, reg.double().expand(n, -1, -1), ref], dim=1)         # [CLS, registers, patches]
        tokens = ref.shape[1]
        assert tokens == (rows // patch) * (cols // patch) + 1 + registers
        view = dvol.view(axis, im_sz)
        pstruct, _, _ = model.pos_for(rows, cols)
        out = torch.full((n + 1, tokens, d), 7.0, device=gpu)
        _lib.check(model.lib.vittf_patch_embed_reg(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view), 0,
                                                   n, _lib.ptr(reg_dev), registers, _lib.ptr(out), _lib.stream_ptr()))
        got = out.cpu()
        assert (got[n:] == 7.0).all(), 'wrote past the last row'
        assert torch.equal(got[:n, 1:1 + registers].view(torch.int32), reg.expand(n, -1, -1).contiguous().view(torch.int32))
        err = (got[:n].double() - ref).abs().amax(dim=-1)
        bound = 4e-6 * ref.abs().amax(dim=-1)                                      # test_patch_embed14's bound
        assert bool((err <= bound).all()), (axis, float((err / bound).max()))
        assert _lib.kernel_name('patch_embed') == EMBED_KERNEL.get((d, patch), f'patch_embed_kernel<{patch}>')
        if n > 3:      # rows are independent of the tiling: a sub-range writes the same bits
            part = torch.zeros(2, tokens, d, device=gpu)
            _lib.check(model.lib.vittf_patch_embed_reg(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct),
                                                       C.byref(view), 1, 2, _lib.ptr(reg_dev), registers, _lib.ptr(part),
                                                       _lib.stream_ptr()))
            assert torch.equal(part.cpu(), got[1:3])
        # no registers through the new entry point: vittf_patch_embed's bits, and the patch rows above are those rows
        plain = torch.full((n + 1, tokens - registers, d), 7.0, device=gpu)
        old = torch.full((n + 1, tokens - registers, d), 7.0, device=gpu)
        _lib.check(model.lib.vittf_patch_embed_reg(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view), 0,
                                                   n, None, 0, _lib.ptr(plain), _lib.stream_ptr()))
        _lib.check(model.lib.vittf_patch_embed(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view), 0,
                                               n, _lib.ptr(old), _lib.stream_ptr()))
        assert torch.equal(plain, old)
        assert torch.equal(plain[:n, 1:].cpu(), got[:n, 1 + registers:]) and torch.equal(plain[:n, 0].cpu(), got[:n, 0])
    # refused: registers without their rows, counts outside 0 .. 8
    for rows_ptr, count in ((None, registers), (_lib.ptr(reg_dev), -1), (_lib.ptr(reg_dev), 9)):
        assert model.lib.vittf_patch_embed_reg(C.byref(model.cfg), C.byref(model.weights), C.byref(pstruct), C.byref(view), 0, 1,
                                               rows_ptr, count, _lib.ptr(out), _lib.stream_ptr()) == INVALID


# ------------------------------------------------------------------------------------------ 9. K-feature epilogue
def _canary_buf(n, tail, dev):
    return torch.full((n + tail,), CANARY, dtype=torch.int16, device=dev)


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('d', [128, 384, 768])
def test_gemm_kfeat_parts_reg_drops_register_rows(gpu, d, dt):
    lib = _lib.load()
    dtype_id = _lib.DTYPES[dt]
    h16 = torch.float16 if dt == 'fp16' else torch.bfloat16
    g = _gen(d + 1)
    registers, npatch, batch = 4, 64, 20
    tokens = 1 + registers + npatch                       # 69
    rows = tokens * batch - 20                            # 1360 rows: six 256-row / eleven 128-row tiles, the last slice cut short
    a = torch.randn((rows, d), generator=g).to(gpu, h16)
    w = (torch.randn((3 * d, d), generator=g) * d ** -0.5).to(gpu, h16)
    bias = torch.randn(3 * d, generator=g).to(gpu)
    st = _lib.stream_ptr()
    tok = torch.arange(rows, device=gpu) % tokens
    a_plain = a[(tok == 0) | (tok > registers)].contiguous()            # the same rows without the register rows
    rows_plain = rows - registers * batch
    assert a_plain.shape[0] == rows_plain
    out_rows = int((tok > registers).sum())
    assert out_rows == rows_plain - batch
    n_out, tail = out_rows * d, 4096
    ref = [_canary_buf(n_out, tail, gpu) for _ in range(3)]
    assert lib.vittf_gemm_kfeat_parts(_lib.ptr(a_plain), _lib.ptr(w), _lib.ptr(bias), rows_plain, d, d, tokens - registers, 7,
                                      *(_lib.ptr(b) for b in ref), dtype_id, st) == 0
    torch.cuda.synchronize()
    for mask in (7, 2, 5):
        bufs = [_canary_buf(n_out, tail, gpu) for _ in range(3)]
        assert lib.vittf_gemm_kfeat_parts_reg(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), rows, d, d, tokens, registers, mask,
                                              *(_lib.ptr(b) for b in bufs), dtype_id, st) == 0, mask
        torch.cuda.synchronize()
        for p in range(3):
            if (mask >> p) & 1:
                assert torch.equal(bufs[p][:n_out], ref[p][:n_out]), (mask, p)
                assert bool((bufs[p][n_out:] == CANARY).all()), (mask, p, 'canary behind the output')
            else:
                assert bool((bufs[p] == CANARY).all()), (mask, p, 'output of an unset bit')
        assert _lib.kernel_name('gemm') == ('gemm_pp_kernel' if d == 768 else 'gemm_kernel')
    if d == 768:
        # outputs that are not 16-byte aligned: the tiled kernel at K = 768 -- the other leg of the same entry point
        bufs = [_canary_buf(n_out + 8, tail, gpu) for _ in range(3)]
        views = [b[4:4 + n_out] for b in bufs]
        assert lib.vittf_gemm_kfeat_parts_reg(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), rows, d, d, tokens, registers, 7,
                                              *(_lib.ptr(v) for v in views), dtype_id, st) == 0
        torch.cuda.synchronize()
        assert _lib.kernel_name('gemm') == 'gemm_kernel'
        plain = [_canary_buf(n_out + 8, tail, gpu) for _ in range(3)]
        assert lib.vittf_gemm_kfeat_parts(_lib.ptr(a_plain), _lib.ptr(w), _lib.ptr(bias), rows_plain, d, d, tokens - registers,
                                          7, *(_lib.ptr(b[4:4 + n_out]) for b in plain), dtype_id, st) == 0
        torch.cuda.synchronize()
        for p in range(3):
            assert torch.equal(bufs[p], plain[p]), ('tiled', p)
            assert bool((bufs[p][:4] == CANARY).all()) and bool((bufs[p][4 + n_out:] == CANARY).all())
    # R = 0 through the new entry point is the old one
    n0 = (rows - batch) * d
    o_new, o_old = _canary_buf(n0, tail, gpu), _canary_buf(n0, tail, gpu)
    assert lib.vittf_gemm_kfeat_parts_reg(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), rows, d, d, tokens, 0, 2, None,
                                          _lib.ptr(o_new), None, dtype_id, st) == 0
    assert lib.vittf_gemm_kfeat_parts(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), rows, d, d, tokens, 2, None, _lib.ptr(o_old),
                                      None, dtype_id, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o_new, o_old)
    # refused: a register count outside 0 .. 8, slices with no patch token
    b = _canary_buf(n_out, 0, gpu)
    for count, toks in ((-1, tokens), (9, tokens), (4, 5)):
        assert lib.vittf_gemm_kfeat_parts_reg(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), rows, d, d, toks, count, 2, None,
                                              _lib.ptr(b), None, dtype_id, st) == INVALID


# ------------------------------------------------------------------------------------------ 10. fixtures
@pytest.mark.parametrize('dt,tol', [('fp16', 1e-3), ('bf16', 8e-3)])
@pytest.mark.parametrize('name', ['dinov2_reg_d128.npz', 'dinov2_reg_d384.npz'])
def test_engine_matches_reg_fixtures(gpu, golden_dir, name, dt, tol):
    rec = load_golden(golden_dir, name)
    arch = tuple(int(v) for v in rec['arch'])
    registers = int(rec['registers'])
    sd = rr.synthetic_reg(arch, int(rec['seed']), registers)
    assert abs(vt.weights.state_dict_checksum(sd) - float(rec['weights_checksum'])) <= 1e-9 * abs(float(rec['weights_checksum']))
    model = vt.HipViT(sd, arch, dt)
    assert model.num_register_tokens == registers
    vol = torch.from_numpy(rec['vol'])
    fos = int(rec['fos'])
    im_sz = tuple(int(v) for v in rec['im_sz'])
    feat_out = tuple(int(v) for v in rec['feat_out'])
    dvol = vt.DeviceVolume(vol, gpu)
    _lib.profiler_enable(True)
    acc = 0.0
    try:
        for ax in 'zyx':
            sl, (a, b) = ofv.AXIS_DIMS[ax]
            n = vol.shape[sl]
            q, k, v = (t.cpu() for t in vt.extract.qkv_slices(model, dvol, ax, im_sz, 0, n))
            for key, got in (('q', q), ('k', k), ('v', v)):
                ref = torch.from_numpy(rec[f'{key}_{ax}'])
                assert got.shape == ref.shape and rel_fro(got, ref) < tol, (ax, key, rel_fro(got, ref))
            # the un-pooled single-axis volume is those K rows in the reference's layout, and the 'all' volume their pooled sum
            order = [None, None, None]
            order[sl], order[a], order[b] = 0, 1, 2
            grid = k.view(n, im_sz[a] // 14, im_sz[b] // 14, -1).permute(3, *order).contiguous()
            assert torch.equal(vt.feature_volume(vol, model, fos, ax, dvol=dvol).cpu(), grid), ax
            ref_k = torch.from_numpy(rec[f'k_{ax}'])
            ref_grid = ref_k.view(n, im_sz[a] // 14, im_sz[b] // 14, -1).permute(3, *order).contiguous()
            acc = torch.as_tensor(acc) + ofv.adaptive_pool(ref_grid, feat_out).squeeze().half()
        torch.cuda.synchronize()
        prof = _lib.profiler_collect()
    finally:
        _lib.profiler_enable(False)
    got = vt.feature_volume(vol, model, fos, 'all', dvol=dvol).cpu()
    assert got.shape == acc.shape and rel_fro(got, acc) < tol, rel_fro(got, acc)
    if arch[0] == 384:
        assert prof['mlp'][1] > 0, 'the block tail did not run'
        assert _lib.kernel_name('patch_embed') == 'patch_embed14_mfma_kernel'
        assert model.weights.tail_packed and model.weights.qkv_packed


# ------------------------------------------------------------------------------------------ 11. full size, N = 4101
FULL = {'vits14_reg': 0, (768, 3, 12, 14): 1, (1024, 3, 16, 14): 2}


def _full_sd(arch):
    return vt.synthetic_state_dict(arch, FULL[arch]) if isinstance(arch, str) else rr.synthetic_reg(arch, FULL[arch], 4)


def _full_vol(arch):
    return (torch.rand((2, 512, 512), generator=_gen(FULL[arch])) * 2 - 1).half().float()


@functools.lru_cache(maxsize=None)
def _full_reference(arch):
    """fp16 K of the patch tokens of both slices from the CPU restatement (shared by the 16-bit and the fp8 run)."""
    model = rr.build_dinov2_reg(arch, _full_sd(arch))
    imgs = ofv.normalized_slices(_full_vol(arch), 'x')
    return torch.cat([rr.patch_qkv(model, F.interpolate(imgs[i:i + 1], size=(896, 896), mode='nearest'))['k'] for i in range(2)])


@pytest.mark.parametrize('arch,attention,tol', [('vits14_reg', '16bit', 1e-3), ((768, 3, 12, 14), '16bit', 1e-3),
                                                ((1024, 3, 16, 14), '16bit', 1e-3), ((768, 3, 12, 14), 'fp8', 6e-2)])
def test_fullsize_896_images_reg(gpu, arch, attention, tol):
    """512 x 512 slices -> 896 x 896 images, 64 x 64 tokens + CLS + 4 registers: N = 4101, 65 query tiles and 5 keys in the last
    64-key tile.  16-bit: test_fullsize_896_images' bound; fp8 attention: the path's stated tolerance (test_attention_fp8)."""
    model = vt.HipViT(_full_sd(arch), arch, 'fp16', attention=attention)
    assert model.num_register_tokens == 4
    im_sz = (14, 896, 896)
    dvol = vt.DeviceVolume(_full_vol(arch), gpu)
    assert model.tokens_for(dvol.view('x', im_sz)) == 4101
    got = vt.k_slices(model, dvol, 'x', im_sz, 0, 2).cpu()
    assert got.shape == (2, 4096, model.embed_dim) and bool(torch.isfinite(got.float()).all())
    # the two-blocks-per-wave attention kernel (its last key tile ends after the first half step here) / the fp8 kernel ran
    name = _lib.kernel_name('attention')
    assert name == 'attn_pp64_kernel' if attention == '16bit' else name.startswith('attn_fp8_kernel'), name
    err = rel_fro(got, _full_reference(arch))
    print(f'{arch} N=4101 {attention}: rel fro {err:.3e}')
    assert err < tol, err


# ------------------------------------------------------------------------------------------ 12. one pass for q, k, v
@pytest.mark.parametrize('arch', [(128, 2, 2, 14), (384, 2, 6, 14), (768, 2, 12, 14)])
def test_qkv_features_equal_three_k_features_reg(gpu, arch):
    model = vt.HipViT(rr.synthetic_reg(arch, 8, 4), arch, 'fp16')
    vol = (torch.rand((9, 20, 33), generator=_gen(8)) * 2 - 1).half().float()
    im_sz = (28, 56, 70)
    dvol = vt.DeviceVolume(vol, gpu)
    for ax in 'zyx':
        n = vol.shape[ofv.AXIS_DIMS[ax][0]]
        together = vt.extract.qkv_slices(model, dvol, ax, im_sz, 0, n)
        for part in range(3):
            alone = vt.k_slices(model, dvol, ax, im_sz, 0, n, part=part)
            assert torch.equal(together[part], alone), (ax, part)
        sub = vt.extract.qkv_slices(model, dvol, ax, im_sz, 1, 4, engine_batch=2, parts=(2, 0))     # another batching, two thirds
        assert torch.equal(sub[0], together[2][1:4]) and torch.equal(sub[1], together[0][1:4])


# ------------------------------------------------------------------------------------------ 13. CLI
def test_infer_cli_vits14_reg_end_to_end(gpu, tmp_path):
    vol = (torch.rand((20, 24, 28), generator=_gen(5)) * 2 - 1).half().float()
    np.save(tmp_path / 'vol.npy', vol.numpy())
    env = dict(os.environ)
    env.pop('VITTF_WEIGHTS', None)
    env['TORCH_HOME'] = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, 'infer.py'), '--data-path', str(tmp_path / 'vol.npy'), '--dino2-model',
           'vits14_reg', '--synthetic-weights', '0', '--feature-output-size', '4']
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = tmp_path / 'vol_vits14_reg_all_features4.npy'
    saved = np.load(out, allow_pickle=True)[()]['k']
    model = vt.HipViT(vt.synthetic_state_dict('vits14_reg', 0), 'vits14_reg', 'fp16')
    want = vt.feature_volume(vol, model, 4, 'all').cpu().numpy()
    _, feat_out = vt.sizing(vol.shape, 4, 14)
    assert saved.dtype == np.float16 and saved.shape == (384, *feat_out) == want.shape
    assert np.array_equal(saved.view(np.int16), want.view(np.int16))
    # the registers and the resize form reach the output: the plain model on the same shared weights gives other features
    plain = vt.HipViT(vt.synthetic_state_dict('vits14', 0), 'vits14', 'fp16')
    assert rel_fro(vt.feature_volume(vol, plain, 4, 'all').cpu(), want) > 1e-2


# ------------------------------------------------------------------------------------------ 14. alternative paths
def test_optional_paths_agree_with_default_reg(gpu):
    """test_optional_paths_agree_with_default for a register model: 4e-3 between the paths, the bf16 bound against the CPU model."""
    arch = (384, 2, 6, 14)
    sd = rr.synthetic_reg(arch, 9, 4)
    vol = (torch.rand((16, 24, 40), generator=_gen(4)) * 2 - 1).half().float()
    im_sz = (28, 42, 70)
    dvol = vt.DeviceVolume(vol, gpu)

    def run(**kw):
        model = vt.HipViT(sd, arch, 'bf16', **kw)
        return torch.cat([vt.k_slices(model, dvol, ax, im_sz, 0, vol.shape[ofv.AXIS_DIMS[ax][0]], engine_batch=4).cpu().reshape(-1)
                          for ax in 'zyx'])
    base = run()
    assert torch.equal(base, run(fused_tail=True, flags=0))                # the default IS the block-tail kernel, flags 0
    split = run(fused_tail=False)
    sep_ln = run(flags=_lib.CFG_SEPARATE_LN)
    plain_q = run(flags=_lib.CFG_UNSCALED_Q)
    oracle = rr.build_dinov2_reg(arch, sd)
    ref = torch.cat([rr.qkv_axis(vol, oracle, im_sz, ax)['k'].reshape(-1) for ax in 'zyx'])
    for name, other in (('GEMM launches', split), ('separate LayerNorms', sep_ln), ('un-scaled q', plain_q)):
        assert rel_fro(base, other) < 1e-3 * 4, name
        assert rel_fro(other, ref) <= 8e-3, name
    assert rel_fro(base, ref) <= 8e-3
