"""CPU: compute_qkv's multi-part, in-plane pooled extraction without a GPU.

1. The rounding rule vittf_pool_slices3d implements -- a running fp16 sum in volume-dimension order, then three fp16
   divisions by the window extents along volume dims 0, 1, 2 -- emulated in numpy, against the installed torch's CPU
   F.adaptive_avg_pool3d on fp16, contiguous and in the three permute_out layouts of compute_qkv (infer.py:201-203).
2. The sharding logic of vit_tf_amd.extract for several qkv thirds and an in-plane output size that differs from the
   token grid, over gloo with 2 and 4 ranks: the same bits as one rank and as F.adaptive_avg_pool3d of the un-pooled
   features, with ONE slab exchange per axis call whatever the number of thirds.  The device kernels are replaced by a
   CPU stand-in (tests only; the product has no such path)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# axis -> permute_out of compute_qkv: (S, F, rows, cols) -> (F, x, y, z)
PERMUTE_OUT = {'z': (1, 2, 3, 0), 'y': (1, 2, 0, 3), 'x': (1, 0, 2, 3)}


def _bounds(i, n_in, n_out):
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def emulate_pool3d(x, out_size):
    """The kernel's rule on a (C, n0, n1, n2) float16 array."""
    c, n0, n1, n2 = x.shape
    res = np.empty((c, *out_size), np.float16)
    for i in range(out_size[0]):
        l0, h0 = _bounds(i, n0, out_size[0])
        for j in range(out_size[1]):
            l1, h1 = _bounds(j, n1, out_size[1])
            for k in range(out_size[2]):
                l2, h2 = _bounds(k, n2, out_size[2])
                acc = np.zeros(c, np.float16)
                for a in range(l0, h0):
                    for b in range(l1, h1):
                        for e in range(l2, h2):
                            acc = (acc.astype(np.float32) + x[:, a, b, e].astype(np.float32)).astype(np.float16)
                v = acc
                for cnt in (h0 - l0, h1 - l1, h2 - l2):
                    v = (v.astype(np.float32) / np.float32(cnt)).astype(np.float16)
                res[:, i, j, k] = v
    return res


@pytest.mark.parametrize('layout', ['contiguous', 'z', 'y', 'x'])
@pytest.mark.parametrize('out_size', [(3, 4, 2), (1, 1, 2), (2, 1, 1), (9, 5, 7), (4, 6, 5)])
def test_pool_rounding_rule_matches_torch_fp16(layout, out_size):
    g = torch.Generator().manual_seed(11)
    s, c, f0, f1 = 6, 4, 5, 7
    un = (torch.randn((s, c, f0, f1), generator=g) * 4).half()          # (slices, F, rows, cols)
    if layout == 'contiguous':
        x = un.permute(1, 0, 2, 3).contiguous()
    else:
        x = un.permute(*PERMUTE_OUT[layout])                              # compute_qkv's view: not contiguous
    ref = F.adaptive_avg_pool3d(x, out_size)
    got = emulate_pool3d(x.contiguous().numpy(), out_size)
    assert np.array_equal(got.view(np.uint16), ref.contiguous().numpy().view(np.uint16))


def test_pool_rounding_rule_alternatives_disagree():
    """The rule is not an arbitrary one: one fp32 accumulation, or one division by the voxel count, gives other bits."""
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((4, 6, 5, 7), generator=g) * 4).half()
    out_size = (4, 3, 3)
    ref = F.adaptive_avg_pool3d(x, out_size).numpy()
    one_div = np.empty_like(ref)
    for i in range(4):
        l0, h0 = _bounds(i, 6, 4)
        for j in range(3):
            l1, h1 = _bounds(j, 5, 3)
            for k in range(3):
                l2, h2 = _bounds(k, 7, 3)
                w = x[:, l0:h0, l1:h1, l2:h2].float().reshape(4, -1).numpy()
                acc = np.zeros(4, np.float16)
                for e in range(w.shape[1]):
                    acc = (acc.astype(np.float32) + w[:, e]).astype(np.float16)
                one_div[:, i, j, k] = (acc.astype(np.float32) / np.float32(w.shape[1])).astype(np.float16)
    assert not np.array_equal(one_div, ref)
    assert np.array_equal(emulate_pool3d(x.numpy(), out_size), ref)


def emulate_global_mean(x):
    """vittf_pool_slices3d's rule for an output of exactly (1, 1, 1): fp64 sum, fp32, fp32 division, fp16."""
    flat = x.reshape(x.shape[0], -1)
    s = flat.astype(np.float64).sum(1).astype(np.float32)
    return (s / np.float32(flat.shape[1])).astype(np.float16)


@pytest.mark.parametrize('shape', [(4, 40, 40, 40), (3, 7, 5, 9), (2, 512, 64, 64)])
def test_global_pool_is_torch_mean(shape):
    """AdaptiveAvgPool3d(1) is not the pooling rule above: torch returns input.mean() (fp32 accumulation).  Over a whole
    axis the running fp16 sum stalls; the fp32 mean does not."""
    g = torch.Generator().manual_seed(shape[1])
    x = (torch.rand(shape, generator=g) * 0.6).half()
    ref = F.adaptive_avg_pool3d(x, 1).reshape(shape[0]).numpy()
    assert np.array_equal(emulate_global_mean(x.numpy()).view(np.uint16), ref.view(np.uint16))
    if shape[1] == 40:
        stalled = emulate_pool3d(x.numpy(), (1, 1, 1)).reshape(shape[0])
        assert np.abs(stalled.astype(np.float32) - ref.astype(np.float32)).max() > 0.1


# ---------------------------------------------------------------------------- sharded multi-part extraction
class QkvStandInOps:
    """CPU stand-ins with the semantics of the libvittf calls the multi-part / in-plane path makes: per-part fp16 token
    features of a slice (a cheap deterministic function of the slice, not a ViT), slice-window + in-plane pooling with
    F.adaptive_avg_pool3d on those fp16 features, the fp16 axis sum."""

    def volume(self, vol, model):
        class V:
            pass
        v = V(); v.data = torch.as_tensor(vol).float().squeeze(); v.shape = tuple(v.data.shape)
        return v

    def zeros(self, shape, model):
        return torch.zeros(shape, dtype=torch.float16)

    @staticmethod
    def _features(dvol, axis, im_sizes, s0, s1, part, d, patch):
        from vit_tf_amd.extract import AXIS_DIMS
        sl, (a, b) = AXIS_DIMS[axis]
        f0, f1 = im_sizes[a] // patch, im_sizes[b] // patch
        sl_data = dvol.data.movedim(sl, 0)[s0:s1].unsqueeze(1)                 # (n, 1, rows, cols)
        grid = F.adaptive_avg_pool2d(sl_data, (f0, f1)).reshape(s1 - s0, f0 * f1, 1)
        ch = torch.arange(d, dtype=torch.float32)
        w = torch.sin(ch * (0.37 + part)) * 3
        bias = torch.cos(ch * (1.3 + 0.5 * part))
        idx = torch.arange(s0, s1, dtype=torch.float32).view(-1, 1, 1) * 0.01
        return (torch.tanh(grid * w + bias + idx) * (2.0 + part)).half().contiguous()

    def k_slices(self, model, dvol, axis, im_sizes, s0, s1, engine_batch, part):
        return self._features(dvol, axis, im_sizes, s0, s1, part, model.embed_dim, model.patch_size)

    def qkv_slices(self, model, dvol, axis, im_sizes, s0, s1, engine_batch, parts):
        return [self._features(dvol, axis, im_sizes, s0, s1, p, model.embed_dim, model.patch_size) for p in parts]

    def _pool(self, kbuf, k_s0, n_total, n_out, win0, nwin, f0, f1, d, dst, strides, o0, o1, slice_dim):
        from vit_tf_amd.extract import window_bounds
        sd, sw, sr, sc = strides
        flat = dst.view(-1)
        k = kbuf.view(kbuf.shape[0], f0, f1, d)
        others = [i for i in range(3) if i != slice_dim]
        for i in range(nwin):
            lo, hi = window_bounds(win0 + i, n_total, n_out)
            win = k[lo - k_s0:hi - k_s0].permute(3, 0, 1, 2)                   # (d, slices, rows, cols)
            x = win.movedim(1, 1 + slice_dim)                                  # slices at their volume dim
            size = [0, 0, 0]
            size[slice_dim], size[others[0]], size[others[1]] = 1, o0, o1
            mean = F.adaptive_avg_pool3d(x, size).movedim(1 + slice_dim, 1)[:, 0]   # (d, o0, o1)
            idx = (torch.arange(d).view(d, 1, 1) * sd + i * sw + torch.arange(o0).view(1, o0, 1) * sr
                   + torch.arange(o1).view(1, 1, o1) * sc)
            flat[idx.reshape(-1)] = mean.reshape(-1)

    def pool(self, model, kbuf, k_s0, n_total, n_out, win0, nwin, f0, f1, d, dst, strides):
        # a one-slice-thick column of the 3-D pool: the in-plane windows are one token wide (slice_dim is then irrelevant)
        self._pool(kbuf, k_s0, n_total, n_out, win0, nwin, f0, f1, d, dst, strides, f0, f1, 2)

    def pool3d(self, model, kbuf, k_s0, n_total, n_out, win0, nwin, f0, f1, d, dst, strides, o0, o1, slice_dim):
        self._pool(kbuf, k_s0, n_total, n_out, win0, nwin, f0, f1, d, dst, strides, o0, o1, slice_dim)


class FakeModel:
    embed_dim, patch_size, device = 16, 8, torch.device('cpu')


SHAPE = (24, 16, 32)
IM_SIZES = (48, 32, 64)                 # token grids: z (6, 4), y (6, 8), x (4, 8)
# (axis, out_size): non-grid in-plane sizes, smaller / larger / non-dividing, a None entry, a slice axis larger than its input
CASES = [('z', (4, 3, 5)), ('y', (None, 3, 11)), ('x', (30, 2, 9)), ('z', (6, 4, 32)), ('x', (1, 1, 1))]
PARTS = [0, 1, 2]


def _volume():
    return (torch.rand(SHAPE, generator=torch.Generator().manual_seed(1)) * 2 - 1).half().float()


def _run_cases(group=None):
    import vit_tf_amd as vt
    ops = QkvStandInOps()
    vol = _volume()
    res = []
    for axis, size in CASES:
        pooled = vt.pooled_axis(vol, FakeModel(), axis, IM_SIZES, size, parts=PARTS, group=group, ops=ops)
        res.append({p: t.numpy() for p, t in pooled.items()})
    # the un-pooled thirds (compute_qkv with _noop) of one axis
    sl = vt.AXIS_DIMS['y'][0]
    g, _ = vt.extract.axis_features(FakeModel(), ops.volume(vol, None), 'y', IM_SIZES, SHAPE[sl], group=group, ops=ops,
                                    parts=PARTS)
    full = vt.extract.assemble_axis(g, 'y', SHAPE[sl])
    res.append({p: full[i * 16:(i + 1) * 16].numpy() for i, p in enumerate(PARTS)})
    return res


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        import vit_tf_amd as vt
        res = _run_cases()
        assert vt.extract.EXCHANGES.get('gloo', 0) == len(CASES) + 1, vt.extract.EXCHANGES    # one per axis call
        if rank == 0:
            q.put(res)
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _reference():
    """F.adaptive_avg_pool3d (CPU, fp16) of the stand-in's un-pooled (F, x, y, z) features of every third."""
    from vit_tf_amd.extract import AXIS_DIMS
    vol = QkvStandInOps().volume(_volume(), None)
    out = []
    for axis, size in CASES + [('y', (None, None, None))]:
        sl, _ = AXIS_DIMS[axis]
        per = {}
        for p in PARTS:
            k = QkvStandInOps._features(vol, axis, IM_SIZES, 0, SHAPE[sl], p, 16, 8)
            f0, f1 = IM_SIZES[AXIS_DIMS[axis][1][0]] // 8, IM_SIZES[AXIS_DIMS[axis][1][1]] // 8
            un = k.view(SHAPE[sl], f0, f1, 16).permute(0, 3, 1, 2).permute(*PERMUTE_OUT[axis])
            per[p] = F.adaptive_avg_pool3d(un, size).numpy()
        out.append(per)
    return out


def test_single_process_multi_part_matches_torch_pool():
    ref = _reference()
    got = _run_cases()
    for case, (r, g) in enumerate(zip(ref, got)):
        for p in PARTS:
            assert g[p].shape == r[p].shape, (case, p)
            assert np.array_equal(g[p].view(np.uint16), r[p].view(np.uint16)), (case, p)


@pytest.mark.parametrize('world', [2, 4])
def test_sharded_multi_part_in_plane_pooling_matches_one_rank(world):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    one = _run_cases()
    assert len(got) == len(one)
    for case, (g, o) in enumerate(zip(got, one)):
        for p in PARTS:
            assert g[p].shape == o[p].shape and np.array_equal(g[p].view(np.uint16), o[p].view(np.uint16)), (case, p)
