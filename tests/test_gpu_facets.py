"""GPU: the token facet (final-norm patch tokens, part 3) and the hooked-layer selection through the HIP engine.

The references are the CPU fp32 models of the tree (oracle.dino_vit, tests/dinov2_reg_ref.py, tests/dinov3_ref.py; held against
transformers by the CPU tests, tests/test_facets_cpu.py for this expression):
    token facet of block l = model.norm(model.tokens_before_block(img, l + 1))[:, 1 + R:]
    q / k / v of block l   = blocks[l].attn.qkv(blocks[l].norm1(tokens_before_block(img, l))) in thirds
Bounds: the project's contract for features, relative Frobenius error below 1e-3 with fp16 operands and 8e-3 with bf16 (what
the fixture tests hold K to); the fp8 attention path's own stated 5e-2.

* vittf_token_features on its own: against an fp64 LayerNorm, canary rows behind the output, a sub-range of slices, a batch
  that ends off a 4-row block.
* The token facet per code path: vits8 (block tail + activation-stationary qkv GEMM), vits14_reg (registers dropped),
  dinov3_vits16 (rotation inside the last block), D = 768 (LayerNorm in the residual GEMM's epilogue), D = 1024 (separate
  LayerNorm); ViT-S/14-reg at full size (N = 4101, two slices); fp8 attention at D = 768, N = 4097.
* Layer selection: k and t of block 0, a middle block and the last; layer = depth - 1 is the model built without `layer`.
* One pass: mask 15 writes q, k, v as mask 7 does and t as mask 8 does; vittf_vit_features(mask 2) is vittf_vit_k_features.
* Pipeline: feature_volume(part=3) is pooling + the fp16 z -> y -> x sum of the GPU's own token slices; infer.py --facet token
  end to end, also through the forced one-rank process group; compute_qkv(return_keys=['k', 't']) in one pass.
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
import dinov2_reg_ref as rr
import dinov3_ref as r3
from helpers import rel_fro
from oracle import dino_vit, feature_volume as ofv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5a5a
TOL = {'fp16': 1e-3, 'bf16': 8e-3}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _family(kind, arch, seed):
    """(state dict, CPU fp32 model, register tokens) of a DINO ('v1'), DINOv2-reg ('reg') or DINOv3 ('v3') model."""
    if kind == 'v1':
        sd = vt.synthetic_state_dict(arch, seed)
        return sd, dino_vit.build_vit(arch, sd), 0
    if kind == 'reg':
        sd = vt.synthetic_state_dict(arch, seed) if isinstance(arch, str) else rr.synthetic_reg(arch, seed, 4)
        return sd, rr.build_dinov2_reg(arch, sd), 4
    sd = vt.synthetic_state_dict(arch, seed, dinov3=True)
    return sd, r3.build_dinov3(arch, sd), 4


def _images(vol, axis, rows, cols, minmax=None):
    return F.interpolate(ofv.normalized_slices(vol, axis, minmax), size=(rows, cols), mode='nearest')


def _ref_token(model, registers, x, layer):
    """fp16 token facet of block `layer` for the images x: (B, n, D)."""
    with torch.no_grad():
        return model.norm(model.tokens_before_block(x, layer + 1)).half()[:, 1 + registers:].contiguous()


def _ref_third(model, registers, x, layer, part):
    """fp16 third `part` of blocks[layer].attn.qkv for the patch tokens of x: (B, n, D)."""
    d = model.embed_dim
    blk = model.blocks[layer]
    with torch.no_grad():
        t = blk.attn.qkv(blk.norm1(model.tokens_before_block(x, layer))).half()[:, 1 + registers:]
    return t[..., part * d:(part + 1) * d].contiguous()


def _small_case(arch):
    """A 5-slice volume and image sizes that give 9 x 8 = 72 patch tokens per x slice (more than one 64-key tile)."""
    p = vt.weights.arch_of(arch)[3]
    vol = (torch.rand((5, 24, 20), generator=_gen(p)) * 2 - 1).half().float()
    return vol, (p, 9 * p, 8 * p)


# ------------------------------------------------------------------------------------------ 1. the output kernel
@pytest.mark.parametrize('prefix', [1, 5])
@pytest.mark.parametrize('d', [128, 384, 768, 1024])
def test_token_features_kernel(gpu, d, prefix):
    """Against nn.LayerNorm's arithmetic in fp64.  Bound per element: half a unit of fp16 at the value's size (the one
    rounding, 2^-11 relative) + 1e-5 of the row's largest output for the fp32 statistics and affine map (a few fp32 units
    of values of that size; 1e-5 is ~80 of them, and 50 times below one fp16 unit of such a value)."""
    lib = _lib.load()
    npatch, batch = 9, 3                                    # 27 output rows: the last block of 4 has one idle wave
    tokens = prefix + npatch
    g = _gen(d + prefix)
    x = (torch.randn((batch * tokens, d), generator=g) * 3 + 0.3)
    x[::7] *= 40                                            # some rows far larger than others: the statistics are per row
    gam = 1.0 + 0.3 * torch.randn(d, generator=g)
    bet = 0.2 * torch.randn(d, generator=g)
    eps = 1e-5 if prefix == 5 else 1e-6
    xd, gd, bd = x.to(gpu), gam.to(gpu), bet.to(gpu)
    n_out, tail = batch * npatch * d, 4096
    out = torch.full((n_out + tail,), CANARY, dtype=torch.int16, device=gpu)
    st = _lib.stream_ptr()
    assert lib.vittf_token_features(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(out), batch, tokens, prefix, d, eps, st) == 0
    torch.cuda.synchronize()
    assert _lib.kernel_name('layernorm') == 'token_out_kernel'
    assert bool((out[n_out:] == CANARY).all()), 'canary behind the output'
    got = out[:n_out].view(torch.float16).view(batch, npatch, d).cpu()
    x64 = x.double().view(batch, tokens, d)[:, prefix:]
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    ref = (x64 - mu) / torch.sqrt(var + eps) * gam.double() + bet.double()
    err = (got.double() - ref).abs()
    bound = 2.0 ** -11 * ref.abs() + 1e-5 * ref.abs().amax(-1, keepdim=True)
    assert bool((err <= bound).all()), float((err / bound).max())
    # rows are independent of the launch: the middle slice alone (x and the output both offset) gives the same bits
    one = torch.full((npatch * d + tail,), CANARY, dtype=torch.int16, device=gpu)
    assert lib.vittf_token_features(_lib.ptr(xd[tokens:]), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(one), 1, tokens, prefix, d, eps,
                                    st) == 0
    torch.cuda.synchronize()
    assert torch.equal(one[:npatch * d], out[npatch * d:2 * npatch * d]) and bool((one[npatch * d:] == CANARY).all())
    # the prefix rows are not read: poison them and nothing changes
    poisoned = xd.clone().view(batch, tokens, d)
    poisoned[:, :prefix] = float('nan')
    again = torch.full_like(out, CANARY)
    assert lib.vittf_token_features(_lib.ptr(poisoned), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(again), batch, tokens, prefix, d,
                                    eps, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------ 2. the facet per code path
PATHS = [('v1', 'vits8'), ('reg', 'vits14_reg'), ('v3', 'dinov3_vits16'), ('v1', (768, 3, 12, 8)), ('reg', (1024, 3, 16, 14))]


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('kind,arch', PATHS, ids=[str(a) for _, a in PATHS])
def test_token_facet_matches_reference(gpu, kind, arch, dt):
    sd, oracle, registers = _family(kind, arch, 3)
    model = vt.HipViT(sd, arch, dt)
    assert model.num_register_tokens == registers and model.layer == model.depth - 1
    vol, im_sz = _small_case(arch)
    dvol = vt.DeviceVolume(vol, gpu)
    _lib.profiler_enable(True)
    try:
        got = vt.k_slices(model, dvol, 'x', im_sz, 0, 5, part=3).cpu()
        torch.cuda.synchronize()
        prof = _lib.profiler_collect()
    finally:
        _lib.profiler_enable(False)
    ref = _ref_token(oracle, registers, _images(vol, 'x', im_sz[1], im_sz[2]), model.depth - 1)
    assert got.shape == ref.shape == (5, 72, model.embed_dim) and got.dtype == torch.float16
    e = rel_fro(got, ref)
    print(f'token facet {arch} {dt}: rel fro {e:.3e}')
    assert _lib.kernel_name('layernorm') == 'token_out_kernel'
    # every block ran in full, the hooked projection did not, and the paths are the ones the case is here for
    d = model.embed_dim
    assert prof['attention'][1] == model.depth and prof['gemm'][1] == 0
    if d == 384:
        assert prof['mlp'][1] == model.depth and prof['layernorm'][1] == 2 and _lib.kernel_name('gemm_qkv') == 'gemm_as_kernel'
    elif d == 768:
        assert prof['gemm_fc2'][1] == model.depth and prof['layernorm'][1] == 2
    else:
        assert prof['layernorm'][1] == 2 * model.depth + 1
    assert bool(torch.isfinite(got.float()).all()) and e < TOL[dt], e
    # the final norm is live: the un-normalised stream is far from it
    with torch.no_grad():
        raw = oracle.tokens_before_block(_images(vol, 'x', im_sz[1], im_sz[2]), model.depth)[:, 1 + registers:]
    assert rel_fro(raw, ref) > 5e-2


def test_token_facet_fullsize_vits14_reg(gpu):
    """512 x 512 slices -> 896 x 896 images, 64 x 64 tokens + CLS + 4 registers: N = 4101, two slices, all 12 blocks and the
    final norm (test_fullsize_896_images_reg's inputs)."""
    arch = 'vits14_reg'
    sd, oracle, registers = _family('reg', arch, 0)
    vol = (torch.rand((2, 512, 512), generator=_gen(0)) * 2 - 1).half().float()
    model = vt.HipViT(sd, arch, 'fp16')
    im_sz = (14, 896, 896)
    dvol = vt.DeviceVolume(vol, gpu)
    assert model.tokens_for(dvol.view('x', im_sz)) == 4101
    t, k = (v.cpu() for v in vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 2, parts=(3, 1)))
    assert _lib.kernel_name('attention') == 'attn_pp64_kernel'
    assert torch.equal(k, vt.k_slices(model, dvol, 'x', im_sz, 0, 2).cpu())
    x = _images(vol, 'x', 896, 896)
    ref = torch.cat([_ref_token(oracle, registers, x[i:i + 1], 11) for i in range(2)])
    assert t.shape == ref.shape == (2, 4096, 384)
    e = rel_fro(t, ref)
    print(f'token facet {arch} N=4101 fp16: rel fro {e:.3e}')
    assert bool(torch.isfinite(t.float()).all()) and e < 1e-3, e


def test_token_facet_fp8_attention(gpu):
    """ViT-B/8-shaped (D = 768, 12 heads, patch 8), N = 4097, fp8 attention in every block: the path's own stated 5e-2."""
    arch = (768, 3, 12, 8)
    sd, oracle, _ = _family('v1', arch, 2)
    vol = (torch.rand((2, 128, 128), generator=_gen(2)) * 2 - 1).half().float()
    model = vt.HipViT(sd, arch, 'fp16', attention='fp8')
    im_sz = (8, 512, 512)
    got = vt.k_slices(model, vt.DeviceVolume(vol, gpu), 'x', im_sz, 0, 1, part=3).cpu()
    assert _lib.kernel_name('attention').startswith('attn_fp8_kernel')
    ref = _ref_token(oracle, 0, _images(vol, 'x', 512, 512)[:1], 2)
    assert got.shape == ref.shape == (1, 4096, 768)
    e = rel_fro(got, ref)
    print(f'token facet {arch} N=4097 fp16 + fp8 attention: rel fro {e:.3e}')
    assert bool(torch.isfinite(got.float()).all()) and e < 5e-2, e
    with pytest.raises(ValueError):
        vt.HipViT(vt.synthetic_state_dict((384, 1, 6, 16), 0, dinov3=True), (384, 1, 6, 16), 'fp16', attention='fp8')


# ------------------------------------------------------------------------------------------ 3. layer selection
@pytest.mark.parametrize('kind,arch', [('v1', (384, 4, 6, 8)), ('v3', (384, 4, 6, 16)), ('reg', (768, 4, 12, 14))])
def test_layer_selection(gpu, kind, arch):
    sd, oracle, registers = _family(kind, arch, 6)
    vol, im_sz = _small_case(arch)
    dvol = vt.DeviceVolume(vol, gpu)
    x = _images(vol, 'x', im_sz[1], im_sz[2])
    depth = arch[1]
    last = vt.HipViT(sd, arch, 'fp16')
    k_last = vt.k_slices(last, dvol, 'x', im_sz, 0, 5)
    for layer in (0, 2, depth - 1):
        model = vt.HipViT(sd, arch, 'fp16', layer=layer)
        assert model.layer == layer and model.depth == depth and model.cfg.depth == layer + 1
        t, k = vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 5, parts=(3, 1))
        e_k = rel_fro(k.cpu(), _ref_third(oracle, registers, x, layer, 1))
        e_t = rel_fro(t.cpu(), _ref_token(oracle, registers, x, layer))
        print(f'{arch} layer {layer}: k {e_k:.3e}, t {e_t:.3e}')
        assert e_k < 1e-3 and e_t < 1e-3, (layer, e_k, e_t)
        if layer == depth - 1:
            assert torch.equal(k, k_last), 'layer = depth - 1 is the model built without `layer`'
        else:
            assert rel_fro(k.cpu(), k_last.cpu()) > 1e-2, 'another block, other keys'
    neg = vt.HipViT(sd, arch, 'fp16', layer=-depth)
    first = vt.HipViT(sd, arch, 'fp16', layer=0)
    assert neg.layer == 0 and torch.equal(vt.k_slices(neg, dvol, 'x', im_sz, 0, 5, part=3),
                                          vt.k_slices(first, dvol, 'x', im_sz, 0, 5, part=3))
    for bad in (depth, -depth - 1):
        with pytest.raises(ValueError):
            vt.HipViT(sd, arch, 'fp16', layer=bad)


# ------------------------------------------------------------------------------------------ 4. one pass, old entries
@pytest.mark.parametrize('kind,arch', [('v1', (384, 2, 6, 8)), ('v3', (384, 2, 6, 16)), ('v1', (768, 2, 12, 8)),
                                       ('reg', (1024, 2, 16, 14))])
def test_all_four_facets_from_one_pass(gpu, kind, arch):
    sd, _, _ = _family(kind, arch, 8)
    model = vt.HipViT(sd, arch, 'fp16')
    vol, im_sz = _small_case(arch)
    dvol = vt.DeviceVolume(vol, gpu)
    q7, k7, v7 = vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 5, parts=(0, 1, 2))
    t8 = vt.k_slices(model, dvol, 'x', im_sz, 0, 5, part=3)
    _lib.profiler_enable(True)
    try:
        q, k, v, t = vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 5, parts=(0, 1, 2, 3))
        torch.cuda.synchronize()
        prof = _lib.profiler_collect()
    finally:
        _lib.profiler_enable(False)
    assert prof['patch_embed'][1] == 1 and prof['gemm'][1] == 1 and prof['attention'][1] == model.depth      # ONE forward
    assert torch.equal(q, q7) and torch.equal(k, k7) and torch.equal(v, v7), 'mask 15 against mask 7'
    assert torch.equal(t, t8), 'mask 15 against mask 8'
    # another batching and a sub-range of slices: the same bits
    sub = vt.extract.qkv_slices(model, dvol, 'x', im_sz, 1, 4, engine_batch=2, parts=(3, 1))
    assert torch.equal(sub[0], t8[1:4]) and torch.equal(sub[1], k7[1:4])


def test_features_entry_against_the_old_entries(gpu):
    """vittf_vit_features with mask 2 is vittf_vit_k_features(part 1), bit for bit; the token output stays inside its
    batch * f0*f1 rows (27 of them here: the last block of 4 rows is cut), a sub-range of slices writes the same bits."""
    arch = (384, 2, 6, 8)
    sd = vt.synthetic_state_dict(arch, 9)
    model = vt.HipViT(sd, arch, 'fp16')
    vol = (torch.rand((3, 10, 10), generator=_gen(9)) * 2 - 1).half().float()
    im_sz = (8, 24, 24)                                     # 3 x 3 patches per x slice
    dvol = vt.DeviceVolume(vol, gpu)
    view = dvol.view('x', im_sz)
    pos, _, _ = model.pos_for(24, 24)
    ws = model.workspace(3, 10)
    n_out, tail = 3 * 9 * 384, 4096
    st = _lib.stream_ptr()

    def buf():
        return torch.full((n_out + tail,), CANARY, dtype=torch.int16, device=gpu)
    old, new, tok, untouched = buf(), buf(), buf(), buf()
    lib = model.lib
    common = (C.byref(model.cfg), C.byref(model.weights), C.byref(pos), C.byref(view))
    assert lib.vittf_vit_k_features(*common, 0, 3, 1, _lib.ptr(old), _lib.ptr(ws), ws.numel(), st) == 0
    assert lib.vittf_vit_features(*common, 0, 3, 2, None, 0, None, None, None, None, _lib.ptr(new), None, None, _lib.ptr(ws),
                                  ws.numel(), st) == 0
    assert lib.vittf_vit_features(*common, 0, 3, 8 | 2, None, 0, None, _lib.ptr(model._norm_g), _lib.ptr(model._norm_b),
                                  _lib.ptr(untouched), _lib.ptr(new), None, _lib.ptr(tok), _lib.ptr(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, new) and bool((old[n_out:] == CANARY).all())
    assert bool((tok[n_out:] == CANARY).all()) and bool((untouched == CANARY).all())      # the q pointer of an unset bit is ignored
    assert torch.equal(tok[:n_out].view(torch.float16).view(3, 9, 384), vt.k_slices(model, dvol, 'x', im_sz, 0, 3, part=3))
    one = torch.full((9 * 384 + tail,), CANARY, dtype=torch.int16, device=gpu)
    assert lib.vittf_vit_features(*common, 1, 1, 8, None, 0, None, _lib.ptr(model._norm_g), _lib.ptr(model._norm_b), None, None,
                                  None, _lib.ptr(one), _lib.ptr(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(one[:9 * 384], tok[9 * 384:2 * 9 * 384]) and bool((one[9 * 384:] == CANARY).all())
    # refused as the header says
    for mask, t_ptr, g_ptr in ((0, tok, model._norm_g), (16, tok, model._norm_g), (8, None, model._norm_g), (8, tok, None)):
        assert lib.vittf_vit_features(*common, 0, 3, mask, None, 0, None, _lib.ptr(g_ptr), _lib.ptr(model._norm_b), None, None, None,
                                      _lib.ptr(t_ptr), _lib.ptr(ws), ws.numel(), st) == -1


# ------------------------------------------------------------------------------------------ 5. pipeline
@pytest.mark.parametrize('kind,arch,patch', [('v1', (128, 2, 2, 8), 8), ('reg', (384, 2, 6, 14), 14)])
def test_feature_volume_of_the_token_facet(gpu, kind, arch, patch):
    """feature_volume(part=3): the single-axis volume is the token slices in the reference's layout; 'all' is torch's CPU
    AdaptiveAvgPool3d of them (fp16) summed z -> y -> x in fp16 -- bit for bit, as for the key facet."""
    sd, _, _ = _family(kind, arch, 4)
    model = vt.HipViT(sd, arch, 'fp16')
    vol = (torch.rand((20, 24, 28), generator=_gen(5)) * 2 - 1).half().float()
    fos = 4
    im_sz, feat_out = vt.sizing(tuple(vol.shape), fos, patch)
    dvol = vt.DeviceVolume(vol, gpu)
    acc = 0.0
    for ax in 'zyx':
        sl, (a, b) = ofv.AXIS_DIMS[ax]
        n = vol.shape[sl]
        t = vt.k_slices(model, dvol, ax, im_sz, 0, n, part=3).cpu()
        order = [None, None, None]
        order[sl], order[a], order[b] = 0, 1, 2
        grid = t.view(n, im_sz[a] // patch, im_sz[b] // patch, -1).permute(3, *order).contiguous()
        assert torch.equal(vt.feature_volume(vol, model, fos, ax, dvol=dvol, part=3).cpu(), grid), ax
        acc = torch.as_tensor(acc) + ofv.adaptive_pool(grid, feat_out).squeeze().half()
    got = vt.feature_volume(vol, model, fos, 'all', dvol=dvol, part=3).cpu()
    assert got.dtype == torch.float16 and got.shape == acc.shape == (arch[0], *feat_out)
    assert torch.equal(got, acc)
    assert not torch.equal(got, vt.feature_volume(vol, model, fos, 'all', dvol=dvol).cpu())        # and it is not the key volume


def test_compute_qkv_returns_tokens_in_one_pass(gpu):
    import infer
    arch = (128, 2, 2, 8)
    model = vt.HipViT(vt.synthetic_state_dict(arch, 7), arch, 'fp16')
    vol = (torch.rand((6, 16, 5), generator=_gen(7)) * 2 - 1).half().float()
    im_sz = (64, 128, 40)
    counts = {}
    res = {}
    for keys in ('k', 't', ['q', 'k', 'v', 't']):
        _lib.profiler_enable(True)
        try:
            res[str(keys)] = infer.compute_qkv(vol, model, 8, im_sz, slice_along='z', return_keys=keys)
            torch.cuda.synchronize()
            rec = _lib.profiler_collect()
        finally:
            _lib.profiler_enable(False)
        counts[str(keys)] = rec['patch_embed'][1]
    assert counts['k'] > 0 and len(set(counts.values())) == 1, counts
    both = res[str(['q', 'k', 'v', 't'])]
    assert sorted(both) == ['k', 'q', 't', 'v']
    assert torch.equal(both['t'], res['t']['t']) and torch.equal(both['k'], res['k']['k'])
    pooled = infer.compute_qkv(vol, model, 8, im_sz, pool_fn=torch.nn.AdaptiveAvgPool3d((3, 4, 2)), slice_along='z',
                               return_keys=['t'])['t']
    assert torch.equal(pooled, F.adaptive_avg_pool3d(res['t']['t'], (3, 4, 2)))


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return str(sk.getsockname()[1])


def test_infer_cli_token_facet_end_to_end(gpu, tmp_path):
    """infer.py --facet token --dino2-model vits14_reg: {'t': fp16} under the suffixed name, the library call's bits; the same
    bits through the forced one-rank process group (the slab exchange on the backend); --layer reaches the model."""
    vol = (torch.rand((20, 24, 28), generator=_gen(5)) * 2 - 1).half().float()
    np.save(tmp_path / 'vol.npy', vol.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('VITTF_WEIGHTS', 'WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'VITTF_DIST_BACKEND', 'VITTF_DIST_FORCE'):
        env.pop(k, None)
    env['TORCH_HOME'] = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, 'infer.py'), '--data-path', str(tmp_path / 'vol.npy'), '--dino2-model',
           'vits14_reg', '--synthetic-weights', '0', '--feature-output-size', '4', '--facet', 'token']
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert not (tmp_path / 'vol_vits14_reg_all_features4.npy').exists()
    saved = np.load(tmp_path / 'vol_vits14_reg_all_features4_token.npy', allow_pickle=True)[()]
    assert list(saved) == ['t']
    sd = vt.synthetic_state_dict('vits14_reg', 0)
    model = vt.HipViT(sd, 'vits14_reg', 'fp16')
    want = vt.feature_volume(vol, model, 4, 'all', part=3).cpu().numpy()
    _, feat_out = vt.sizing(vol.shape, 4, 14)
    assert saved['t'].dtype == np.float16 and saved['t'].shape == (384, *feat_out) == want.shape
    assert np.array_equal(saved['t'].view(np.int16), want.view(np.int16))
    # the forced one-rank group: three exchanges on the backend, the same file
    env1 = dict(env, WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=_free_port(),
                VITTF_DIST_FORCE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    res = subprocess.run([*cmd, '--cache-path', str(tmp_path / 'forced.npy')], cwd=ROOT, env=env1, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert 'slab exchanges: 3 over nccl' in res.stdout, res.stdout
    forced = np.load(tmp_path / 'forced.npy', allow_pickle=True)[()]['t']
    assert np.array_equal(forced.view(np.int16), want.view(np.int16))
    # --layer: key facet of block 3, named by its index
    res = subprocess.run([*cmd[:-2], '--layer', '-9'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    k3 = np.load(tmp_path / 'vol_vits14_reg_all_features4_L3.npy', allow_pickle=True)[()]['k']
    want3 = vt.feature_volume(vol, vt.HipViT(sd, 'vits14_reg', 'fp16', layer=3), 4, 'all').cpu().numpy()
    assert np.array_equal(k3.view(np.int16), want3.view(np.int16))
