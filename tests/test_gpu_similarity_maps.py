"""GPU: the fp32 class maps of every similarity kernel form, entry by entry, against the fp64 reference and the derived
bound of tests/sim_data.py (Numerics) -- the tests of tests/test_gpu_kernels.py see these maps only after the
quantisation to uint8.  All calls go through vittf_similarity_maps_f32 (mode 0, fp16 volume: the routing of
vittf_similarity); the kernel form is chosen with the switches the library reads per call and asserted by name.

tests/test_sim_data_cpu.py shows on float32 emulations that a lost lo half, a dropped annotation and a counted padding row
break the bound used here."""
import ctypes as C

import numpy as np
import pytest
import torch

from vit_tf_amd import _lib
import sim_data as sd

pytestmark = pytest.mark.gpu

IDS = [sd.case_id(c) for c in sd.GPU_CASES]
GUARD = 7.0
_results = {}                 # (case id, data kind, normalized) -> what the call left: one GPU run per case and data set


def _call(lib, gpu, case, d, monkeypatch, feat=None):
    """One vittf_similarity_maps_f32 call under the case's switches: (kernel name, maps [classes][nvox], the guard float
    behind them, the per-class maxima at the head of the workspace), on the host."""
    for k in sd.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    classes, a = len(d.counts), int(sum(d.counts))
    n0, n1, n2 = d.grid
    nvox = n0 * n1 * n2
    feat = d.X.to(gpu) if feat is None else feat
    qf = d.q.to(gpu)
    vnorm = None if d.vnorm is None else d.vnorm.to(gpu)
    starts = sd.starts_of(d.counts)
    ws_bytes = lib.vittf_similarity_workspace_bytes(classes, 0, a)
    ws = torch.full((ws_bytes,), 0xff, dtype=torch.uint8, device=gpu)
    out = torch.full((classes * nvox + 1,), GUARD, device=gpu)
    _lib.check(lib.vittf_similarity_maps_f32(_lib.ptr(feat), 1, d.f, n0, n1, n2, _lib.ptr(qf), starts.ctypes.data_as(C.POINTER(C.c_int32)),
                                             classes, 0, 0.0, _lib.ptr(vnorm), _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    host = out.cpu()
    return _lib.kernel_name('similarity'), host[:-1].view(classes, nvox), float(host[-1]), ws[:4 * classes].cpu().view(torch.float32)


def _run(gpu, case, kind, normalized, monkeypatch):
    key = (sd.case_id(case), kind, normalized)
    if key not in _results:
        d = sd.case_data(case, kind, normalized)
        _results[key] = (d,) + _call(_lib.load(), gpu, case, d, monkeypatch)
    d, name, maps, guard, maxima = _results[key]
    assert name == case.kernel, f'routing: {name} ran, the case is written for {case.kernel}'
    assert guard == GUARD, 'wrote past the last map'
    return d, maps, maxima


def _assert_within_bound(maps, d, what):
    ratio, c, v = sd.worst(maps, d.ref, d.bound)
    off_edge = sd.worst(torch.where(d.edge, d.ref.float(), maps), d.ref, d.bound)[0]      # (figures of DESIGN.md 4.5)
    print(f'{what}: worst error / bound {ratio:.4f} (class {c}, voxel {v}: {sd.where_in_kernel(v)}); off the threshold {off_edge:.4f}')
    assert bool(torch.isfinite(maps).all())
    assert ratio <= 1.0, (f'{what}: class {c} ({d.counts[c]} annotations), voxel {v} ({sd.where_in_kernel(v)}): got {float(maps[c, v])!r}, '
                          f'fp64 {float(d.ref[c, v])!r}, bound {float(d.bound[c, v]):.3e}, error / bound {ratio:.2f}; '
                          f'{int(((maps.double() - d.ref).abs() > d.bound).sum())} of {maps.numel()} entries outside')
    return ratio


@pytest.mark.parametrize('normalized', [True, False], ids=['unit', 'cosine'])
@pytest.mark.parametrize('case', sd.GPU_CASES, ids=IDS)
def test_maps_within_fp64_bound(gpu, monkeypatch, case, normalized):
    """Every entry of every class map within the derived bound of its fp64 value, none skipped; on unit-norm volumes and on
    the cosine path (volume left at its norms, vnorm passed)."""
    d, maps, _ = _run(gpu, case, 'correlated', normalized, monkeypatch)
    sd.check_edge_share(d)
    assert float(maps.max()) > 0.01
    _assert_within_bound(maps, d, f'{sd.case_id(case)} {"unit" if normalized else "cosine"}')


@pytest.mark.parametrize('case', [c for c in sd.GPU_CASES if sd.has_tails(c)], ids=[i for c, i in zip(sd.GPU_CASES, IDS) if sd.has_tails(c)])
def test_lo_half_reaches_the_result(gpu, monkeypatch, case):
    """Queries h (1 + 2^-12) whose fp16 rounding is the volume column h itself: the same bound, at the targeted voxels --
    where a lost lo half is 5.7 to 9.5 times the bound (test_sim_data_cpu.py) -- and everywhere else."""
    d, maps, _ = _run(gpu, case, 'tails', True, monkeypatch)
    sd.check_edge_share(d)
    st = sd.starts_of(d.counts)
    for c in range(len(d.counts)):
        t = d.targets[st[c]:st[c + 1]]
        r = ((maps[c, t].double() - d.ref[c, t]).abs() / d.bound[c, t])
        assert float(r.max()) <= 1.0, (c, int(t[int(r.argmax())]), float(r.max()))
        assert float(d.ref[c, t].min()) > 0.9 / d.counts[c]                 # the target's own annotation counts there: s = 1
    _assert_within_bound(maps, d, f'{sd.case_id(case)} tails')


@pytest.mark.parametrize('case', sd.GPU_CASES, ids=IDS)
def test_lattice_maps_exact(gpu, monkeypatch, case):
    """0 / 1 features and one-hot queries of weight 1, 0.25, 0.125, -1, 4: every dot product, activation and class sum is
    exact in fp32, so the map is the exact sum divided by n_c -- within one fp32 ulp of the quotient (no more is assumed
    of the division than IEEE rounding), bit-equal where n_c is a power of two.  A dropped, doubled or misplaced
    annotation, a column read from elsewhere or > for >= moves the sum by at least 2^-5."""
    d, maps, maxima = _run(gpu, case, 'lattice', True, monkeypatch)
    n = torch.tensor(d.counts, dtype=torch.float64)[:, None]
    want = d.sums / n
    ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
    off = (maps.double() - want).abs()
    i = int((off / ulp).argmax())
    c, v = divmod(i, maps.shape[1])
    assert bool((off <= ulp).all()), (f'class {c} ({d.counts[c]} annotations), voxel {v} ({sd.where_in_kernel(v)}): got * n_c = '
                                      f'{float(maps[c, v]) * d.counts[c]!r}, exact sum {float(d.sums[c, v])!r}; {int((off > ulp).sum())} entries off')
    pow2 = torch.tensor([k & (k - 1) == 0 for k in d.counts])
    assert torch.equal(maps[pow2].double(), want[pow2])
    assert torch.equal(maxima.view(torch.int32), maps.amax(dim=1).view(torch.int32))
    assert float(d.sums.max()) >= 1.0


@pytest.mark.parametrize('normalized', [True, False], ids=['unit', 'cosine'])
@pytest.mark.parametrize('case', sd.GPU_CASES, ids=IDS)
def test_class_maxima(gpu, monkeypatch, case, normalized):
    """The head of the workspace (filled with 0xff before the call) holds max_v map[c][v] as float bits: the value the
    0.99-max scaling of the uint8 maps uses."""
    _, maps, maxima = _run(gpu, case, 'correlated', normalized, monkeypatch)
    assert torch.equal(maxima.view(torch.int32), maps.amax(dim=1).view(torch.int32)), (maxima.tolist(), maps.amax(dim=1).tolist())
    assert float(maxima.min()) > 0.0


def _misaligned(t, gpu, rem):
    """A copy of t on the GPU whose address is rem mod 16."""
    nbytes = t.numel() * t.element_size()
    buf = torch.zeros(nbytes + 32, dtype=torch.uint8, device=gpu)
    off = (rem - buf.data_ptr()) % 16
    view = buf[off:off + nbytes]
    view.copy_(t.contiguous().view(-1).view(torch.uint8).to(gpu))
    assert view.data_ptr() % 16 == rem
    return view                                           # (keeps buf alive)


def test_forms_agree(gpu, monkeypatch):
    """Every voxel goes through the same MFMA sequence whichever form stages it: one voxel block per wave, two, and the
    strided loads write the same bits; the few-query kernel joins on a one-class case.  The strided form runs on a copy of
    the volume whose rows are not 16-byte aligned (4 mod 16: the entry takes 4-byte aligned volumes, 2 mod 16 is refused
    before anything is launched).  The VALU kernels sum in another order and are held to the bound only
    (test_maps_within_fp64_bound, same data)."""
    lib = _lib.load()
    one, two = sd.GPU_CASES[0], sd.GPU_CASES[7]
    assert (one.env, two.env, one.grid, one.counts) == (sd.ONE_BLOCK, sd.TWO_BLOCKS, two.grid, two.counts)
    d, a, _ = _run(gpu, one, 'correlated', True, monkeypatch)
    _, b, _ = _run(gpu, two, 'correlated', True, monkeypatch)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    view = _misaligned(d.X, gpu, 4)
    name, s, guard, maxima = _call(lib, gpu, one, d, monkeypatch, feat=view)
    assert name == 'sim_mfma_kernel' and guard == GUARD
    assert torch.equal(a.view(torch.int32), s.view(torch.int32))
    assert torch.equal(maxima.view(torch.int32), a.amax(dim=1).view(torch.int32))
    with pytest.raises(_lib.VittfError):
        _call(lib, gpu, one, d, monkeypatch, feat=_misaligned(d.X, gpu, 2))
    # one class of 16: the persistent kernel against the strided form of the chunked kernel
    few = sd.Case(kernel='sim_mfma_few_kernel', env=sd.FEW, grid=sd.G, counts=(16,))
    d, a, _ = _run(gpu, few, 'correlated', True, monkeypatch)
    _assert_within_bound(a, d, 'sim_mfma_few_kernel 16')
    view = _misaligned(d.X, gpu, 4)
    name, s, guard, _ = _call(lib, gpu, few, d, monkeypatch, feat=view)
    assert name == 'sim_mfma_kernel' and guard == GUARD
    assert torch.equal(a.view(torch.int32), s.view(torch.int32))
