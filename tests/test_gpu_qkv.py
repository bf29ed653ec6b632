"""GPU: compute_qkv's one-pass q / k / v extraction and in-plane adaptive pooling.

* vittf_gemm_kfeat_parts: every requested third bit-equal to vittf_gemm(EPI_KFEAT) on that third's weights, nothing
  written behind an output or into the output of an unset bit, bad masks and NULL pointers refused.
* the K-feature epilogue of both GEMM kernels (fp16 operands) bit-equal to the plain bias epilogue with the dropped rows taken
  out on the host: vittf_gemm_kfeat_parts_reg with and without register rows, and vittf_gemm(EPI_KFEAT).
* vittf_vit_qkv_features: each third bit-equal to vittf_vit_k_features(part) on the engine's four projection paths.
* compute_qkv(return_keys=['q','k','v']) runs the ViT once: as many patch-embedding and K-projection launches as 'k'.
* vittf_pool_slices3d: bit-equal to the CPU F.adaptive_avg_pool3d of the same fp16 features.
* compute_qkv with an AdaptiveAvgPool3d whose in-plane size is not the token grid."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_tf_amd as vt
from helpers import load_golden, TINY_ARCH

pytestmark = pytest.mark.gpu

INVALID = -1
CANARY = 0x5a5a          # int16 pattern behind / inside buffers that must stay untouched
PERMUTE_OUT = {'z': (1, 2, 3, 0), 'y': (1, 2, 0, 3), 'x': (1, 0, 2, 3)}


def _canary_buf(n, tail, dev):
    return torch.full((n + tail,), CANARY, dtype=torch.int16, device=dev)


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('d', [128, 384, 768])
def test_gemm_kfeat_parts_bit_equal_to_single_third(gpu, d, dt):
    lib = vt._lib.load()
    dtype_id = vt._lib.DTYPES[dt]
    h16 = torch.float16 if dt == 'fp16' else torch.bfloat16
    g = torch.Generator().manual_seed(d)
    tokens, batch = 65, 9
    rows = tokens * batch - 20                         # the last slice is cut short: the last row tile is partial
    out_rows = rows - (-(-rows // tokens))             # CLS rows dropped
    a = torch.randn((rows, d), generator=g).to(gpu, h16)
    w = (torch.randn((3 * d, d), generator=g) * d ** -0.5).to(gpu, h16)
    bias = torch.randn(3 * d, generator=g).to(gpu)
    st = vt._lib.stream_ptr()
    n_out, tail = out_rows * d, 4096
    ref = []
    for p in range(3):
        o = torch.empty(n_out, dtype=torch.int16, device=gpu)
        rc = lib.vittf_gemm(vt._lib.ptr(a), vt._lib.ptr(w[p * d:]), vt._lib.ptr(bias[p * d:]), vt._lib.ptr(o), rows, d, d,
                            vt._lib.EPI_KFEAT, tokens, dtype_id, st)
        assert rc == 0
        ref.append(o)
    torch.cuda.synchronize()
    for mask in range(1, 8):
        bufs = [_canary_buf(n_out, tail, gpu) for _ in range(3)]
        rc = lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, mask,
                                        *(vt._lib.ptr(b) for b in bufs), dtype_id, st)
        assert rc == 0, mask
        torch.cuda.synchronize()
        for p in range(3):
            if (mask >> p) & 1:
                assert torch.equal(bufs[p][:n_out], ref[p]), (mask, p)
                assert bool((bufs[p][n_out:] == CANARY).all()), (mask, p, 'canary behind the output')
            else:
                assert bool((bufs[p] == CANARY).all()), (mask, p, 'output of an unset bit')
    assert vt._lib.kernel_name('gemm') == ('gemm_pp_kernel' if d == 768 else 'gemm_kernel')
    if d == 768:
        # an output that is not 16-byte aligned: that third takes the tiled kernel (as its own vittf_gemm call does), the
        # others the persistent one -- two launches, each third still bit-equal to its single-third call on the same pointers
        bufs = [_canary_buf(n_out + 8, tail, gpu) for _ in range(3)]
        views = [bufs[0][4:4 + n_out], bufs[1][8:8 + n_out], bufs[2][:n_out]]       # q at +8 bytes: misaligned
        for p in range(3):
            o = torch.full((n_out + 8,), CANARY, dtype=torch.int16, device=gpu)
            ov = o[4:4 + n_out] if p == 0 else o[:n_out]
            assert lib.vittf_gemm(vt._lib.ptr(a), vt._lib.ptr(w[p * d:]), vt._lib.ptr(bias[p * d:]), vt._lib.ptr(ov), rows,
                                  d, d, vt._lib.EPI_KFEAT, tokens, dtype_id, st) == 0
            torch.cuda.synchronize()
            ref[p] = ov.clone()
        assert lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, 7,
                                          *(vt._lib.ptr(v) for v in views), dtype_id, st) == 0
        torch.cuda.synchronize()
        assert vt._lib.kernel_name('gemm') == 'gemm_kernel'        # the tiled leg launched last
        for p in range(3):
            assert torch.equal(views[p], ref[p]), ('split', p)
        assert bool((bufs[0][:4] == CANARY).all()) and bool((bufs[0][4 + n_out:] == CANARY).all())
    # refused: masks outside 1..7, a NULL output for a set bit
    b = _canary_buf(n_out, 0, gpu)
    for mask in (0, 8, -1):
        assert lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, mask,
                                          vt._lib.ptr(b), vt._lib.ptr(b), vt._lib.ptr(b), dtype_id, st) == INVALID
    for p in range(3):
        ptrs = [vt._lib.ptr(b)] * 3
        ptrs[p] = None
        assert lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, 7,
                                          *ptrs, dtype_id, st) == INVALID
    # the pointer of an unset bit may be NULL
    assert lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, 2,
                                      None, vt._lib.ptr(b), None, dtype_id, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(b, ref[1])


def test_gemm_kfeat_parts_output_beyond_4_gib(gpu):
    """Each output past what a 32-bit buffer descriptor addresses (0xfffffff0 bytes) at D = 768: every third falls back to
    the tiled kernel, as the single-third vittf_gemm(EPI_KFEAT) does -- bit-equal to it, nothing behind the outputs."""
    lib = vt._lib.load()
    d, tokens, batch = 768, 4097, 683
    rows = tokens * batch
    out_rows = rows - batch
    assert out_rows * d * 2 > 0xfffffff0
    g = torch.Generator(device=gpu).manual_seed(1)
    a = (torch.randn((rows, d), generator=g, device=gpu)).half()
    w = (torch.randn((3 * d, d), generator=g, device=gpu) * d ** -0.5).half()
    bias = torch.randn(3 * d, generator=g, device=gpu)
    st = vt._lib.stream_ptr()
    n_out, tail = out_rows * d, 4096
    bufs = [_canary_buf(n_out, tail, gpu) for _ in range(3)]
    assert lib.vittf_gemm_kfeat_parts(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, d, tokens, 5,
                                      *(vt._lib.ptr(b) for b in bufs), vt._lib.FP16, st) == 0
    torch.cuda.synchronize()
    assert vt._lib.kernel_name('gemm') == 'gemm_kernel'
    assert bool((bufs[1] == CANARY).all())
    for p in (0, 2):
        assert bool((bufs[p][n_out:] == CANARY).all())
        ref = torch.empty(n_out, dtype=torch.int16, device=gpu)
        assert lib.vittf_gemm(vt._lib.ptr(a), vt._lib.ptr(w[p * d:]), vt._lib.ptr(bias[p * d:]), vt._lib.ptr(ref), rows, d,
                              d, vt._lib.EPI_KFEAT, tokens, vt._lib.FP16, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(bufs[p][:n_out], ref), p
        del ref


@pytest.mark.parametrize('d,k,tokens,batch,kernel', [(128, 128, 17, 9, 'gemm_kernel'), (256, 768, 131, 5, 'gemm_pp_kernel')])
def test_gemm_kfeat_bit_equal_to_bias_epilogue(gpu, d, k, tokens, batch, kernel):
    """The K-feature output of both kernels, through vittf_gemm_kfeat_parts_reg and through vittf_gemm(EPI_KFEAT), against an
    oracle that shares no epilogue code with it: vittf_gemm(EPI_BIAS) of the same kernel family over the whole [3 d][k]
    projection, the rows tok <= n_reg of every slice dropped on the host, cut into thirds.  With fp16 operands both epilogues
    round the same fp32 sums to fp16: bit-equal.  (The last row tile is partial and a row tile holds several slices.)"""
    lib = vt._lib.load()
    g = torch.Generator().manual_seed(d + tokens)
    rows = tokens * batch
    a = torch.randn((rows, k), generator=g).to(gpu, torch.float16)
    w = (torch.randn((3 * d, k), generator=g) * k ** -0.5).to(gpu, torch.float16)
    bias = torch.randn(3 * d, generator=g).to(gpu)
    st = vt._lib.stream_ptr()
    full = torch.empty((rows, 3 * d), dtype=torch.int16, device=gpu)
    assert lib.vittf_gemm(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), vt._lib.ptr(full), rows, 3 * d, k,
                          vt._lib.EPI_BIAS, 0, vt._lib.FP16, st) == 0
    torch.cuda.synchronize()
    tok = torch.arange(rows, device=gpu) % tokens
    tail = 4 * d                                       # guard rows behind every output
    for n_reg in (0, 4):
        kept = full[tok > n_reg]
        want = [kept[:, p * d:(p + 1) * d].reshape(-1) for p in range(3)]
        n_out = (rows - batch * (1 + n_reg)) * d
        assert want[0].numel() == n_out
        for mask in (2, 5, 7):
            bufs = [_canary_buf(n_out, tail, gpu) for _ in range(3)]
            assert lib.vittf_gemm_kfeat_parts_reg(vt._lib.ptr(a), vt._lib.ptr(w), vt._lib.ptr(bias), rows, d, k, tokens, n_reg,
                                                  mask, *(vt._lib.ptr(b) for b in bufs), vt._lib.FP16, st) == 0
            torch.cuda.synchronize()
            assert vt._lib.kernel_name('gemm') == kernel
            for p in range(3):
                if (mask >> p) & 1:
                    assert torch.equal(bufs[p][:n_out], want[p]), (n_reg, mask, p)
                    assert bool((bufs[p][n_out:] == CANARY).all()), (n_reg, mask, p, 'guard rows')
                else:
                    assert bool((bufs[p] == CANARY).all()), (n_reg, mask, p, 'output of an unset bit')
        if n_reg == 0:
            for p in range(3):
                o = _canary_buf(n_out, tail, gpu)
                assert lib.vittf_gemm(vt._lib.ptr(a), vt._lib.ptr(w[p * d:]), vt._lib.ptr(bias[p * d:]), vt._lib.ptr(o), rows,
                                      d, k, vt._lib.EPI_KFEAT, tokens, vt._lib.FP16, st) == 0
                torch.cuda.synchronize()
                assert torch.equal(o[:n_out], want[p]), ('single third', p)
                assert bool((o[n_out:] == CANARY).all()), ('single third', p, 'guard rows')


def _engine_case(gpu, arch, seed, dt='fp16', **kw):
    sd = vt.synthetic_state_dict(arch, seed)
    model = vt.HipViT(sd, arch, dt, device=gpu, **kw)
    vol = (torch.rand((6, 16, 5), generator=torch.Generator().manual_seed(seed)) * 2 - 1).half().float()
    dvol = vt.DeviceVolume(vol, gpu)
    im_sz = (64, 128, 40)                              # z slices: 64 x 128 images, N = 129 tokens at patch 8
    singles = [vt.k_slices(model, dvol, 'z', im_sz, 0, 5, engine_batch=3, part=p) for p in range(3)]
    for parts in ([0, 1, 2], [0, 2], [1, 2], [1]):
        multi = vt.extract.qkv_slices(model, dvol, 'z', im_sz, 0, 5, engine_batch=3, parts=parts)
        for p, t in zip(parts, multi):
            assert torch.equal(t, singles[p]), (arch, parts, p)
        # the K projection is the forward's last launch of its class: the name is the kernel that ran it
        assert vt._lib.kernel_name('gemm') == ('gemm_pp_kernel' if model.embed_dim == 768 else 'gemm_kernel')
    assert torch.isfinite(singles[0].float()).all()
    return model


def test_vit_qkv_features_tiny(gpu):
    _engine_case(gpu, TINY_ARCH, 3)
    _engine_case(gpu, TINY_ARCH, 3, 'bf16')


def test_vit_qkv_features_vits8_packed(gpu):
    model = _engine_case(gpu, 'vits8', 4)
    assert model.weights.tail_packed and model.weights.qkv_packed      # the block-tail / gemm_as path


def test_vit_qkv_features_vitb8_persistent_gemm(gpu):
    _engine_case(gpu, 'vitb8', 5)
    assert vt._lib.kernel_name('gemm') == 'gemm_pp_kernel'


def test_vit_qkv_features_fp8_attention(gpu):
    _engine_case(gpu, 'vitb8', 6, attention='fp8')


def test_compute_qkv_runs_the_vit_once(gpu, golden_dir):
    import infer
    g = load_golden(golden_dir, 'featvol_even.npz')
    vol = torch.from_numpy(g['vol'])
    model = vt.HipViT(vt.synthetic_state_dict(TINY_ARCH, int(g['seed'])), TINY_ARCH, 'fp16')
    im_sz = tuple(int(x) for x in g['im_sz'])
    counts = {}
    for keys in ('k', ['q', 'k', 'v']):
        vt._lib.profiler_enable(True)
        try:
            infer.compute_qkv(vol, model, 8, im_sz, slice_along='x', return_keys=keys)
            torch.cuda.synchronize()
            rec = vt._lib.profiler_collect()
        finally:
            vt._lib.profiler_enable(False)
        counts[str(keys)] = (rec['patch_embed'][1], rec['gemm'][1])
    assert counts['k'][0] > 0 and counts['k'][1] > 0
    assert counts[str(['q', 'k', 'v'])] == counts['k'], counts


def _pool_ref(kbuf_cpu, axis, size):
    """F.adaptive_avg_pool3d (CPU, fp16) of token-major features [S, f0, f1, D] in compute_qkv's (D, x, y, z) view."""
    return F.adaptive_avg_pool3d(kbuf_cpu.permute(0, 3, 1, 2).permute(*PERMUTE_OUT[axis]), size)


@pytest.mark.parametrize('axis', ['z', 'y', 'x'])
def test_pool_slices3d_bit_equal_to_torch(gpu, axis):
    lib = vt._lib.load()
    sl, (a, b) = vt.AXIS_DIMS[axis]
    s, f0, f1, d = 11, 6, 9, 128
    k = (torch.randn((s, f0, f1, d), generator=torch.Generator().manual_seed(sl)) * 3).half()
    kd = k.to(gpu)
    st = vt._lib.stream_ptr()
    # in-plane outputs smaller, equal, larger, non-dividing and 1
    # (1, 1, 1): torch's input.mean() (fp32 accumulation), not the pooling rule
    for n_out, o0, o1 in ((4, 3, 9), (11, 6, 9), (5, 13, 20), (3, 4, 7), (2, 1, 1), (7, 1, 5), (1, 1, 1)):
        size = [0, 0, 0]
        size[sl], size[a], size[b] = n_out, o0, o1
        shape, strides = vt.extract._slab_shape_strides(axis, d, size, n_out)
        dst = torch.full(shape, float('nan'), dtype=torch.float16, device=gpu)
        rc = lib.vittf_pool_slices3d(vt._lib.ptr(kd), 0, s, s, n_out, 0, n_out, f0, f1, d, vt._lib.ptr(dst), *strides,
                                     o0, o1, sl, st)
        assert rc == 0
        ref = _pool_ref(k, axis, size)
        got = dst.cpu()
        assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16)), (axis, n_out, o0, o1)
        if (o0, o1) == (f0, f1):
            plain = torch.full(shape, float('nan'), dtype=torch.float16, device=gpu)
            assert lib.vittf_pool_slices(vt._lib.ptr(kd), 0, s, s, n_out, 0, n_out, f0, f1, d, vt._lib.ptr(plain),
                                         *strides, st) == 0
            assert torch.equal(plain.cpu().view(torch.int16), got.view(torch.int16))
        # windows 1 .. n_out - 2 from only the slices they touch, into a strided slab of chunk n_out windows (the rank
        # layout of extract.axis_features)
        if n_out >= 3:
            win0, nwin = 1, n_out - 2
            lo = vt.extract.window_bounds(win0, s, n_out)[0]
            hi = vt.extract.window_bounds(win0 + nwin - 1, s, n_out)[1]
            part = kd[lo:hi].clone()
            slab = torch.full(shape, float('nan'), dtype=torch.float16, device=gpu)
            rc = lib.vittf_pool_slices3d(vt._lib.ptr(part), lo, hi - lo, s, n_out, win0, nwin, f0, f1, d,
                                         vt._lib.ptr(slab), *strides, o0, o1, sl, st)
            assert rc == 0
            got_s = slab.cpu().narrow(1 + sl, 0, nwin)
            ref_s = ref.narrow(1 + sl, win0, nwin)
            assert torch.equal(got_s.contiguous().view(torch.int16), ref_s.contiguous().view(torch.int16))
            assert torch.isnan(slab.cpu().narrow(1 + sl, nwin, n_out - nwin).float()).all()    # nothing beyond
    # refused: bad slice_dim / sizes
    assert lib.vittf_pool_slices3d(vt._lib.ptr(kd), 0, s, s, 2, 0, 2, f0, f1, d, vt._lib.ptr(kd), 1, 1, 1, 1, 2, 2, 3, st) \
        == INVALID
    assert lib.vittf_pool_slices3d(vt._lib.ptr(kd), 0, s, s, 2, 0, 2, f0, f1, d, vt._lib.ptr(kd), 1, 1, 1, 1, 0, 2, 0, st) \
        == INVALID


@pytest.mark.parametrize('axis', ['z', 'y', 'x'])
def test_compute_qkv_in_plane_pooling(gpu, golden_dir, axis):
    import infer
    g = load_golden(golden_dir, 'featvol_even.npz')
    vol = torch.from_numpy(g['vol'])
    model = vt.HipViT(vt.synthetic_state_dict(TINY_ARCH, int(g['seed'])), TINY_ARCH, 'fp16')
    im_sz = tuple(int(x) for x in g['im_sz'])
    keys = ['q', 'k', 'v']
    noop = infer.compute_qkv(vol, model, 8, im_sz, slice_along=axis, return_keys=keys)
    assert list(noop) == keys
    for key in keys:
        one = infer.compute_qkv(vol, model, 8, im_sz, slice_along=axis, return_keys=key)
        assert torch.equal(noop[key], one[key]), key
    un_shape = noop['k'].shape[1:]
    # non-grid in-plane sizes, one None (= keep that dim) and one larger than its input
    # AdaptiveAvgPool3d(1) is torch's mean over each whole third (fp32 accumulation)
    for size in ((2, None, 7), (5, 3, 2), (None, 1, 3), 1):
        pooled = infer.compute_qkv(vol, model, 8, im_sz, pool_fn=torch.nn.AdaptiveAvgPool3d(size), slice_along=axis,
                                   return_keys=keys, batch_size=3)
        full = (1, 1, 1) if size == 1 else tuple(un_shape[i] if s is None else s for i, s in enumerate(size))
        for key in keys:
            ref = F.adaptive_avg_pool3d(noop[key], size)
            assert pooled[key].shape == ref.shape == (128, *full), (key, size)
            assert torch.equal(pooled[key].view(torch.int16), ref.view(torch.int16)), (axis, key, size)
