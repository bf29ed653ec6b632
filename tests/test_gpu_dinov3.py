"""GPU: DINOv3 ViT-S/16, B/16, L/16 (4 register tokens, rotary position embedding) through the HIP engine.

* vittf_rope_qk alone against the fp64 rotation of the same 16-bit inputs with the same fp32 table.
* The engine against tests/golden/dinov3_*.npz and, live, against tests/dinov3_ref.py (which the CPU tests hold against
  transformers.DINOv3ViTModel): ViT-S/16 with 12 blocks at 1024 x 1024 (N = 4101), 3-block D = 768 and D = 1024 models.
* vittf_vit_qkv_features_rope with a NULL table == vittf_vit_qkv_features_reg; the engine's alternative paths; the engine
  batch; the fp8 refusal; a rotation that is silently skipped is caught; infer.py --dino3-model vits16 end to end.
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
import dinov3_ref as r3
from helpers import load_golden, rel_fro
from oracle import feature_volume as ofv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5a5a
INVALID = -1
MANT = {'fp16': 10, 'bf16': 7}
MIN_EXP = {'fp16': -14, 'bf16': -126}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ulp(x, dt):
    """One unit in the last place of the 16-bit type at |x| (fp64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** MIN_EXP[dt]))).clamp_min(MIN_EXP[dt])
    return torch.pow(2.0, e - MANT[dt])


def _rotate64(x, cos, sin, prefix, tokens, heads):
    """fp64 rotation of the q and k thirds of x [rows][3 D] (fp64) with the fp32 table [patches][32]; -> (result, pair term):
    the second tensor is |x cos| + |partner sin| per element (what the fp32 products are bounded by), zero where nothing is
    rotated."""
    rows = x.shape[0]
    d = heads * 64
    tok = torch.arange(rows) % tokens
    patch = tok >= prefix
    t = (tok - prefix).clamp_min(0)
    c = cos.double()[t][:, None, :]                                    # (rows, 1, 32)
    s = sin.double()[t][:, None, :]
    qk = x[:, :2 * d].reshape(rows, 2 * heads, 64)
    lo, hi = qk[..., :32], qk[..., 32:]
    rot = torch.cat((lo * c - hi * s, hi * c + lo * s), dim=-1).reshape(rows, 2 * d)
    mag = torch.cat(((lo * c).abs() + (hi * s).abs(), (hi * c).abs() + (lo * s).abs()), dim=-1).reshape(rows, 2 * d)
    out = x.clone()
    out[patch, :2 * d] = rot[patch]
    term = torch.zeros_like(x)
    term[patch, :2 * d] = mag[patch]
    return out, term


# ------------------------------------------------------------------------------------------ 6. the rotation kernel
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('prefix', [1, 5])
@pytest.mark.parametrize('d', [128, 384, 768, 1024])
def test_rope_qk_kernel(gpu, d, prefix, dt):
    """Bound, per element: one unit in the last place of the 16-bit type at the fp64 result, plus the fp32 arithmetic's own
    error 4 * 2^-24 * (|x cos| + |partner sin|) -- two product roundings and one sum rounding, each 2^-24 relative to terms of
    that size.  The second term is four orders below the unit except where the two products cancel (a result near zero beside
    a partner of order one), where the unit of the tiny result is below fp32's error on the products.
    Round trip (the negated sin table applied to the output): the two roundings in between are each at most half a unit at the
    pair's radius r = sqrt(lo^2 + hi^2), which no intermediate exceeds, and come back through the rotation multiplied by
    |cos| and |sin|; with the last rounding: (0.5 (|cos| + |sin|) + 0.5) units at r, at most 1.21, plus the fp32 term.  One
    unit at the ELEMENT's own size cannot hold for a small element beside a large partner, whatever the kernel does: the
    intermediate already carries half a unit of the large one."""
    lib = _lib.load()
    h16 = torch.float16 if dt == 'fp16' else torch.bfloat16
    heads = d // 64
    f0, f1 = 7, 9                                                   # 63 patches: tokens 64 / 68 -> rows not a multiple of 256 lanes' worth
    tokens, batch = prefix + f0 * f1 - 2, 3                         # 62 + prefix: nothing convenient
    npatch = tokens - prefix
    cos, sin = (t[:npatch].contiguous() for t in vt.weights.rope_table(f0, f1))
    rows = tokens * batch
    g = _gen(d + prefix)
    x = (torch.randn((rows, 3 * d), generator=g) * 1.5).to(h16)
    tail = 4096
    buf = torch.full((rows * 3 * d + tail,), CANARY, dtype=torch.int16, device=gpu)
    buf[:rows * 3 * d] = x.view(torch.int16).reshape(-1).to(gpu)
    cos_d, sin_d, nsin_d = cos.to(gpu), sin.to(gpu), (-sin).to(gpu)
    table = _lib.RopeTable(cos_d.data_ptr(), sin_d.data_ptr(), npatch)
    st = _lib.stream_ptr()
    assert lib.vittf_rope_qk(_lib.ptr(buf), rows, tokens, prefix, heads, C.byref(table), _lib.DTYPES[dt], st) == 0
    torch.cuda.synchronize()
    got_bits = buf.cpu()
    assert bool((got_bits[rows * 3 * d:] == CANARY).all()), 'canary behind the buffer'
    got = got_bits[:rows * 3 * d].view(h16).reshape(rows, 3 * d)
    xb, gb = x.view(torch.int16), got.view(torch.int16)
    assert torch.equal(gb[:, 2 * d:], xb[:, 2 * d:]), 'the v third changed'
    tok = torch.arange(rows) % tokens
    assert torch.equal(gb[tok < prefix], xb[tok < prefix]), 'a prefix row changed'
    ref, term = _rotate64(x.double(), cos, sin, prefix, tokens, heads)
    err = (got.double() - ref).abs()
    bound = _ulp(ref, dt) + 4 * 2.0 ** -24 * term
    worst = float((err / bound).max())
    half = float((err > 0.5 * _ulp(ref, dt) + 4 * 2.0 ** -24 * term).double().mean())
    print(f'rope d={d} prefix={prefix} {dt}: worst error {worst:.3f} of the bound; {half:.2e} of the elements beyond half a unit')
    assert worst <= 1.0
    assert float((got.double() - x.double()).abs().max()) > 0.5           # and it did rotate
    # back with the negated sin table
    back_table = _lib.RopeTable(cos_d.data_ptr(), nsin_d.data_ptr(), npatch)
    assert lib.vittf_rope_qk(_lib.ptr(buf), rows, tokens, prefix, heads, C.byref(back_table), _lib.DTYPES[dt], st) == 0
    torch.cuda.synchronize()
    back_bits = buf.cpu()
    assert bool((back_bits[rows * 3 * d:] == CANARY).all())
    back = back_bits[:rows * 3 * d].view(h16).reshape(rows, 3 * d).double()
    xd = x.double()
    qk = xd[:, :2 * d].reshape(rows, 2 * heads, 2, 32)
    radius = qk.pow(2).sum(2, keepdim=True).sqrt().expand_as(qk).reshape(rows, 2 * d)
    t = (tok - prefix).clamp_min(0)
    cs = (cos.double().abs() + sin.double().abs())[t][:, None, None, :].expand(rows, 2 * heads, 2, 32).reshape(rows, 2 * d)
    rt_bound = (0.5 * cs + 0.5) * _ulp(radius, dt) + 8 * 2.0 ** -24 * radius
    rt_err = (back[:, :2 * d] - xd[:, :2 * d]).abs()
    print(f'  round trip: worst {float((rt_err / rt_bound).max()):.3f} of the bound')
    assert bool((rt_err <= rt_bound).all())
    assert torch.equal(back[:, 2 * d:], xd[:, 2 * d:]) and torch.equal(back[tok < prefix], xd[tok < prefix])
    # refused: a table for another patch count, a buffer that is not 16-byte aligned, no table
    wrong = _lib.RopeTable(cos_d.data_ptr(), sin_d.data_ptr(), npatch - 1)
    assert lib.vittf_rope_qk(_lib.ptr(buf), rows, tokens, prefix, heads, C.byref(wrong), _lib.DTYPES[dt], st) == INVALID
    assert lib.vittf_rope_qk(C.c_void_p(buf.data_ptr() + 2), rows, tokens, prefix, heads, C.byref(table), _lib.DTYPES[dt],
                             st) == INVALID
    assert lib.vittf_rope_qk(_lib.ptr(buf), rows, tokens, prefix, heads, None, _lib.DTYPES[dt], st) == INVALID
    assert lib.vittf_rope_qk(_lib.ptr(buf), rows, tokens, tokens, heads, C.byref(table), _lib.DTYPES[dt], st) == INVALID


# ------------------------------------------------------------------------------------------ 7a. fixtures
@pytest.mark.parametrize('dt,tol', [('fp16', 1e-3), ('bf16', 8e-3)])
@pytest.mark.parametrize('name', ['dinov3_d128.npz', 'dinov3_d384.npz'])
def test_engine_matches_v3_fixtures(gpu, golden_dir, name, dt, tol):
    """fp16: the project's 1e-3 contract bound; bf16: the bound the other fixture tests give the opt-in type."""
    rec = load_golden(golden_dir, name)
    arch = tuple(int(v) for v in rec['arch'])
    sd = r3.synthetic_v3(arch, int(rec['seed']))
    assert abs(vt.weights.state_dict_checksum(sd) - float(rec['weights_checksum'])) <= 1e-9 * abs(float(rec['weights_checksum']))
    model = vt.HipViT(sd, arch, dt)
    assert model.rope and model.num_register_tokens == int(rec['registers']) == 4
    assert abs(model.cfg.ln_eps - 1e-5) < 1e-12
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
                err = rel_fro(got, ref)
                print(f'{name} {dt} {ax} {key}: rel fro {err:.3e}')
                assert got.shape == ref.shape and err < tol, (ax, key, err)
            order = [None, None, None]
            order[sl], order[a], order[b] = 0, 1, 2
            ref_k = torch.from_numpy(rec[f'k_{ax}'])
            ref_grid = ref_k.view(n, im_sz[a] // 16, im_sz[b] // 16, -1).permute(3, *order).contiguous()
            acc = torch.as_tensor(acc) + ofv.adaptive_pool(ref_grid, feat_out).squeeze().half()
        torch.cuda.synchronize()
        prof = _lib.profiler_collect()
    finally:
        _lib.profiler_enable(False)
    got = vt.feature_volume(vol, model, fos, 'all', dvol=dvol).cpu()
    assert got.shape == acc.shape and rel_fro(got, acc) < tol, rel_fro(got, acc)
    assert set(prof) == set(_lib.KERNEL_CLASSES)                       # the rotation has no class of its own
    if arch[0] == 384:
        assert prof['mlp'][1] > 0, 'the block tail did not run'
        assert model.weights.tail_packed and model.weights.qkv_packed


# ------------------------------------------------------------------------------------------ 7b. full size, N = 4101
FULL = {'dinov3_vits16': 0, (768, 3, 12, 16): 1, (1024, 3, 16, 16): 2}


def _full_sd(arch):
    return vt.synthetic_state_dict(arch, FULL[arch], dinov3=True)


def _full_vol(arch):
    return (torch.rand((2, 512, 512), generator=_gen(FULL[arch])) * 2 - 1).half().float()


@functools.lru_cache(maxsize=None)
def _full_reference(arch, identity=False):
    """fp16 q, k, v of the patch tokens of both slices from the CPU restatement."""
    model = r3.build_dinov3(arch, _full_sd(arch))
    model.identity_rope = identity
    imgs = ofv.normalized_slices(_full_vol(arch), 'x')
    res = [r3.patch_qkv(model, F.interpolate(imgs[i:i + 1], size=(1024, 1024), mode='nearest')) for i in range(2)]
    return {key: torch.cat([r[key] for r in res]) for key in r3.PARTS}


@pytest.mark.parametrize('arch', ['dinov3_vits16', (768, 3, 12, 16), (1024, 3, 16, 16)])
def test_fullsize_1024_images_v3(gpu, arch):
    """512 x 512 slices -> 1024 x 1024 images, 64 x 64 tokens + CLS + 4 registers: N = 4101.  q, k and v under the project's
    contract bound 1e-3 (tests/test_gpu_dinov2_reg.py measures 4.0e-4 at these shapes without a rotation)."""
    model = vt.HipViT(_full_sd(arch), arch, 'fp16')
    assert model.rope and model.num_register_tokens == 4 and model.patch_size == 16
    im_sz = (16, 1024, 1024)
    dvol = vt.DeviceVolume(_full_vol(arch), gpu)
    assert model.tokens_for(dvol.view('x', im_sz)) == 4101
    got = [t.cpu() for t in vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 2)]
    assert _lib.kernel_name('attention') == 'attn_pp64_kernel'
    ref = _full_reference(arch)
    errs = {}
    for key, t in zip(r3.PARTS, got):
        assert t.shape == (2, 4096, model.embed_dim) and bool(torch.isfinite(t.float()).all())
        errs[key] = rel_fro(t, ref[key])
    print(f'{arch} N=4101: rel fro ' + ', '.join(f'{k} {e:.3e}' for k, e in errs.items()))
    for key, e in errs.items():
        assert e < 1e-3, (key, e)


# ------------------------------------------------------------------------------------------ 9. a skipped rotation is caught
@pytest.mark.parametrize('arch', [(384, 3, 6, 16), (768, 3, 12, 16)])
def test_identity_table_gives_other_features(gpu, arch):
    """cos = 1, sin = 0 in place of the table (what a skipped rotation computes): far beyond the 1e-3 bound from the real
    features, and what the CPU model computes with the same table."""
    sd = r3.synthetic_v3(arch, 4)
    vol = (torch.rand((6, 40, 56), generator=_gen(6)) * 2 - 1).half().float()
    im_sz = (16, 160, 224)                                           # 10 x 14 tokens
    dvol = vt.DeviceVolume(vol, gpu)
    model = vt.HipViT(sd, arch, 'fp16')
    real = [t.cpu() for t in vt.extract.qkv_slices(model, dvol, 'x', im_sz, 0, 6)]
    oracle = r3.build_dinov3(arch, sd)
    ref = r3.qkv_axis(vol, oracle, im_sz, 'x')
    ident = vt.HipViT(sd, arch, 'fp16')
    _, cos, sin = ident.rope_for(160, 224)
    cos.fill_(1.0)
    sin.zero_()
    skipped = [t.cpu() for t in vt.extract.qkv_slices(ident, dvol, 'x', im_sz, 0, 6)]
    oracle.identity_rope = True
    ref_id = r3.qkv_axis(vol, oracle, im_sz, 'x')
    for i, key in enumerate(r3.PARTS):
        moved = rel_fro(skipped[i], real[i])
        print(f'{arch} {key}: identity table moves the features by {moved:.3e}')
        assert rel_fro(real[i], ref[key]) < 1e-3 and rel_fro(skipped[i], ref_id[key]) < 1e-3
        assert moved > 2e-2, (key, moved)                            # 20 x the bound


# ------------------------------------------------------------------------------------------ 8. entry point, paths, batch
def _call(lib, fn, model, view, batch, table, outs, cfg=None):
    pos, _, _ = model.pos_for(view.out_rows, view.out_cols)
    ws = model.workspace(batch, model.tokens_for(view))
    args = [C.byref(cfg or model.cfg), C.byref(model.weights), C.byref(pos), C.byref(view), 0, batch, 7, _lib.ptr(model._reg),
            model.num_register_tokens]
    if fn == 'vittf_vit_qkv_features_rope':
        args.append(C.byref(table) if table is not None else None)
    return getattr(lib, fn)(*args, *(_lib.ptr(o) for o in outs), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())


@pytest.mark.parametrize('arch', [(128, 2, 2, 16), (384, 2, 6, 16), (768, 2, 12, 16)])
def test_null_table_is_the_reg_entry_point(gpu, arch):
    lib = _lib.load()
    model = vt.HipViT(r3.synthetic_v3(arch, 8), arch, 'fp16')
    vol = (torch.rand((9, 20, 33), generator=_gen(8)) * 2 - 1).half().float()
    im_sz = (32, 64, 80)
    dvol = vt.DeviceVolume(vol, gpu)
    view = dvol.view('x', im_sz)
    npatch = (64 // 16) * (80 // 16)
    n = 9 * npatch * arch[0]

    def bufs():
        return [torch.full((n + 64,), CANARY, dtype=torch.int16, device=gpu) for _ in range(3)]
    new, old, rot = bufs(), bufs(), bufs()
    assert _call(lib, 'vittf_vit_qkv_features_rope', model, view, 9, None, new) == 0
    assert _call(lib, 'vittf_vit_qkv_features_reg', model, view, 9, None, old) == 0
    table, _, _ = model.rope_for(64, 80)
    assert _call(lib, 'vittf_vit_qkv_features_rope', model, view, 9, table, rot) == 0
    torch.cuda.synchronize()
    for a, b, c in zip(new, old, rot):
        assert torch.equal(a, b)
        assert bool((c[n:] == CANARY).all()) and not torch.equal(a, c)
    # a table for another grid, and the fp8 attention path together with a table: refused
    other, _, _ = model.rope_for(64, 64)
    assert _call(lib, 'vittf_vit_qkv_features_rope', model, view, 9, other, rot) == INVALID
    fp8 = _lib.VitConfig(*(getattr(model.cfg, f) for f, _ in _lib.VitConfig._fields_))
    fp8.attention_fp8 = 1
    ws_fp8 = torch.empty(lib.vittf_vit_workspace_bytes(C.byref(fp8), 9, model.tokens_for(view)), dtype=torch.uint8, device=gpu)
    pos, _, _ = model.pos_for(64, 80)
    assert lib.vittf_vit_qkv_features_rope(C.byref(fp8), C.byref(model.weights), C.byref(pos), C.byref(view), 0, 9, 7,
                                           _lib.ptr(model._reg), 4, C.byref(table), *(_lib.ptr(o) for o in rot),
                                           _lib.ptr(ws_fp8), ws_fp8.numel(), _lib.stream_ptr()) == INVALID
    with pytest.raises(ValueError):
        vt.HipViT(r3.synthetic_v3(arch, 8), arch, 'fp16', attention='fp8')


@pytest.mark.parametrize('arch', [(384, 3, 6, 16), (768, 2, 12, 16)])
def test_bits_do_not_depend_on_the_engine_batch_v3(gpu, arch):
    model = vt.HipViT(r3.synthetic_v3(arch, 8), arch, 'fp16')
    vol = (torch.rand((9, 20, 33), generator=_gen(8)) * 2 - 1).half().float()
    im_sz = (32, 64, 80)
    dvol = vt.DeviceVolume(vol, gpu)
    for ax in 'zyx':
        n = vol.shape[ofv.AXIS_DIMS[ax][0]]
        together = vt.extract.qkv_slices(model, dvol, ax, im_sz, 0, n)
        for part in range(3):
            assert torch.equal(together[part], vt.k_slices(model, dvol, ax, im_sz, 0, n, part=part)), (ax, part)
        sub = vt.extract.qkv_slices(model, dvol, ax, im_sz, 1, 4, engine_batch=2, parts=(2, 0))
        assert torch.equal(sub[0], together[2][1:4]) and torch.equal(sub[1], together[0][1:4])


def test_optional_paths_agree_with_default_v3(gpu):
    """test_optional_paths_agree_with_default for a DINOv3 model: 4e-3 between the paths, the bf16 bound against the CPU model.
    Every path rotates: gemm_as (default), vittf_gemm (fused_tail=False), the un-scaled q."""
    arch = (384, 3, 6, 16)
    sd = r3.synthetic_v3(arch, 9)
    vol = (torch.rand((16, 24, 40), generator=_gen(4)) * 2 - 1).half().float()
    im_sz = (32, 48, 80)
    dvol = vt.DeviceVolume(vol, gpu)

    def run(**kw):
        model = vt.HipViT(sd, arch, 'bf16', **kw)
        return torch.cat([vt.k_slices(model, dvol, ax, im_sz, 0, vol.shape[ofv.AXIS_DIMS[ax][0]], engine_batch=4).cpu().reshape(-1)
                          for ax in 'zyx'])
    base = run()
    assert torch.equal(base, run(fused_tail=True, flags=0))
    split = run(fused_tail=False)
    sep_ln = run(flags=_lib.CFG_SEPARATE_LN)
    plain_q = run(flags=_lib.CFG_UNSCALED_Q)
    oracle = r3.build_dinov3(arch, sd)
    ref = torch.cat([r3.qkv_axis(vol, oracle, im_sz, ax)['k'].reshape(-1) for ax in 'zyx'])
    for name, other in (('GEMM launches', split), ('separate LayerNorms', sep_ln), ('un-scaled q', plain_q)):
        assert rel_fro(base, other) < 1e-3 * 4, name
        assert rel_fro(other, ref) <= 8e-3, name
    assert rel_fro(base, ref) <= 8e-3


# ------------------------------------------------------------------------------------------ 10. CLI
def test_infer_cli_dinov3_vits16_end_to_end(gpu, tmp_path):
    vol = (torch.rand((20, 24, 28), generator=_gen(5)) * 2 - 1).half().float()
    np.save(tmp_path / 'vol.npy', vol.numpy())
    env = dict(os.environ)
    env.pop('VITTF_WEIGHTS', None)
    env['TORCH_HOME'] = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, 'infer.py'), '--data-path', str(tmp_path / 'vol.npy'), '--dino3-model',
           'vits16', '--synthetic-weights', '0', '--feature-output-size', '4']
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = tmp_path / 'vol_dinov3_vits16_all_features4.npy'
    saved = np.load(out, allow_pickle=True)[()]['k']
    model = vt.HipViT(vt.synthetic_state_dict('dinov3_vits16', 0), 'dinov3_vits16', 'fp16')
    want = vt.feature_volume(vol, model, 4, 'all').cpu().numpy()
    _, feat_out = vt.sizing(vol.shape, 4, 16)
    assert saved.dtype == np.float16 and saved.shape == (384, *feat_out) == want.shape
    assert np.array_equal(saved.view(np.int16), want.view(np.int16))
