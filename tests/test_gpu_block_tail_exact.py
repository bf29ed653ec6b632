"""GPU: the fused block tail (vittf_block_tail, csrc/tail_fx.hip) and the three launches it replaces -- vittf_gemm_residual_ln
(gemm_rows.hip's epilogue LayerNorm, 384 and 768 columns), vittf_gemm with EPI_BIAS_GELU, vittf_layernorm -- on inputs for
which the residual stream x, norm2's output and the hidden activation are known bit for bit (tests/tail_data.py, DESIGN.md
5.1): x is compared equal to the fp64 integer result on every route, so all routes give the same bytes; the LayerNorm on the
way out, whose gamma and beta are real-valued, is held to the one-rounding bound against fp64 LayerNorm of the exact x.
tests/test_tail_data_cpu.py shows that the data has its properties and that subtly wrong kernels would fail.
Guard rows of 7.0 lie behind every output."""
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import tail_data as td

pytestmark = pytest.mark.gpu

GUARD, GUARD_ROWS = 7.0, 32          # 32: a partial tile's stores carry row offsets of up to 24 rows (test_gpu_kernels.GUARD_ROWS)
D = td.D


def _dev(c, gpu, dt):
    t16 = {n: getattr(c, n).to(td.TDT[dt]).to(gpu) for n in ('a', 'wp', 'w1', 'w2')}
    f32 = {n: getattr(c, n).float().to(gpu) for n in ('bp', 'b1', 'b2', 'g2', 'e2', 'g1', 'e1')}
    return {**t16, **f32}


def _guarded(x, dtype, gpu, guard_rows=GUARD_ROWS):
    """x (rows, n) followed by guard rows of 7.0, on the device."""
    g = torch.full((guard_rows, x.shape[1]), GUARD, dtype=torch.float64)
    return torch.cat([x, g]).to(dtype).to(gpu)


def _first_difference(got, want, what):
    bad = (got != want) | torch.isnan(got)
    if not bool(bad.any()):
        return None
    r, col = (int(v) for v in bad.nonzero()[0])
    return (f'{what}: {int(bad.sum())} of {bad.numel()} elements in {int(bad.any(dim=1).sum())} rows differ, first at row {r} '
            f'(row tile {r // 128}, row {r % 128} of it) column {col}: got {float(got[r, col])!r}, want {float(want[r, col])!r}')


def _check_guards(buf, rows, what):
    assert bool((buf[rows:].double() == GUARD).all()), f'wrote past the last row of {what}'


def _block_tail(lib, gpu, c, dv, dt, ln_out):
    rows = c.rows
    wpk = vt.weights.pack_block_tail_weights(dv['wp'][None], dv['w1'][None], dv['w2'][None])[0].contiguous()
    x = _guarded(c.x0, torch.float32, gpu)
    h = torch.full((rows + GUARD_ROWS, D), GUARD, dtype=td.TDT[dt], device=gpu)
    ctr = torch.full((1,), 12345, dtype=torch.int32, device=gpu)
    _lib.check(lib.vittf_block_tail(_lib.ptr(dv['a']), _lib.ptr(wpk), _lib.ptr(dv['bp']), _lib.ptr(dv['g2']), _lib.ptr(dv['e2']),
                                    _lib.ptr(dv['b1']), _lib.ptr(dv['b2']), _lib.ptr(x), rows, D, _lib.DTYPES[dt],
                                    _lib.ptr(dv['g1']) if ln_out else None, _lib.ptr(dv['e1']) if ln_out else None, td.LN_EPS,
                                    _lib.ptr(h) if ln_out else None, _lib.ptr(ctr), _lib.stream_ptr()), 'vittf_block_tail')
    torch.cuda.synchronize()
    return x, h


def _h_ratio(h, want, dt):
    return float(((h.double() - want).abs() / td.h_bound(want, dt)).max())


@pytest.mark.parametrize('ln_out', [True, False], ids=['ln', 'no_ln'])
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('rows', td.ROWS)
def test_block_tail_exact(gpu, rows, dt, ln_out):
    lib = _lib.load()
    c = td.tail_case(rows)
    dv = _dev(c, gpu, dt)
    x, h = _block_tail(lib, gpu, c, dv, dt, ln_out)
    xc, hc = x.cpu(), h.float().cpu()
    _check_guards(xc, rows, 'x')
    _check_guards(hc, rows, 'h_out')
    diff = _first_difference(xc[:rows].double(), c.x, 'x')
    assert diff is None, diff
    if ln_out:
        ratio = _h_ratio(hc[:rows], td.layernorm64(c.x, c.g1, c.e1), dt)
        print(f'block tail {rows} rows {dt}: h_out worst error / bound {ratio:.3f}')
        assert ratio <= 1.0
    else:
        assert bool((hc == GUARD).all()), 'h_out written without a LayerNorm on the way out'


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('rows', td.ROWS)
def test_the_three_launches_exact_and_the_same_bytes(gpu, rows, dt):
    """proj + residual + norm2 (vittf_gemm_residual_ln), fc1 + GELU (vittf_gemm), fc2 + residual + the next norm1
    (vittf_gemm_residual_ln, k = 1536), and vittf_layernorm alone on both residual streams: x', norm2's output, the hidden
    activation and x are all exact; the block tail's x has the same bytes."""
    lib = _lib.load()
    c = td.tail_case(rows)
    dv = _dev(c, gpu, dt)
    t, code, st = td.TDT[dt], _lib.DTYPES[dt], _lib.stream_ptr()
    guards = 2
    x = _guarded(c.x0, torch.float32, gpu, guards)
    new_h = lambda n=D: torch.full((rows + guards, n), GUARD, dtype=t, device=gpu)
    h2, hl, gbuf, h3, h4 = new_h(), new_h(), new_h(4 * D), new_h(), new_h()
    _lib.check(lib.vittf_gemm_residual_ln(_lib.ptr(dv['a']), _lib.ptr(dv['wp']), _lib.ptr(dv['bp']), _lib.ptr(x), rows, D, D, code,
                                          _lib.ptr(dv['g2']), _lib.ptr(dv['e2']), td.LN_EPS, _lib.ptr(h2), st), 'proj')
    x1 = x.clone()
    _lib.check(lib.vittf_layernorm(_lib.ptr(x1), _lib.ptr(dv['g2']), _lib.ptr(dv['e2']), _lib.ptr(hl), rows, D, td.LN_EPS, code, st), 'norm2')
    _lib.check(lib.vittf_gemm(_lib.ptr(h2), _lib.ptr(dv['w1']), _lib.ptr(dv['b1']), _lib.ptr(gbuf), rows, 4 * D, D, _lib.EPI_BIAS_GELU, 0,
                              code, st), 'fc1')
    _lib.check(lib.vittf_gemm_residual_ln(_lib.ptr(gbuf), _lib.ptr(dv['w2']), _lib.ptr(dv['b2']), _lib.ptr(x), rows, D, 4 * D, code,
                                          _lib.ptr(dv['g1']), _lib.ptr(dv['e1']), td.LN_EPS, _lib.ptr(h3), st), 'fc2')
    _lib.check(lib.vittf_layernorm(_lib.ptr(x), _lib.ptr(dv['g1']), _lib.ptr(dv['e1']), _lib.ptr(h4), rows, D, td.LN_EPS, code, st), 'norm1')
    torch.cuda.synchronize()
    for buf, what in ((x1, "x'"), (x, 'x'), (h2, 'norm2 (epilogue)'), (hl, 'norm2 (vittf_layernorm)'), (gbuf, 'hidden'), (h3, 'h'), (h4, 'h')):
        _check_guards(buf.float().cpu(), rows, what)
    for got, want, what in ((x1, c.xp, "x' of vittf_gemm_residual_ln"), (h2, c.hn, 'norm2 in the epilogue of vittf_gemm_residual_ln'),
                            (hl, c.hn, 'norm2 by vittf_layernorm'), (gbuf, c.u, 'hidden activation of vittf_gemm'),
                            (x, c.x, 'x of vittf_gemm_residual_ln')):
        diff = _first_difference(got[:rows].float().cpu().double(), want, what)
        assert diff is None, diff
    want_h = td.layernorm64(c.x, c.g1, c.e1)
    r3, r4 = _h_ratio(h3[:rows].float().cpu(), want_h, dt), _h_ratio(h4[:rows].float().cpu(), want_h, dt)
    print(f'three launches {rows} rows {dt}: h worst error / bound {r3:.3f} (epilogue) {r4:.3f} (vittf_layernorm)')
    assert r3 <= 1.0 and r4 <= 1.0
    xt, _ = _block_tail(lib, gpu, c, dv, dt, False)
    assert torch.equal(xt[:rows], x[:rows]), 'the block tail and the three launches differ in x'


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
def test_gemm_residual_ln_768_columns_exact(gpu, dt):
    """gemm_rows.hip's 768-column form (257 rows: full row tiles and a remainder of one row) with balanced patterns of its own: x and h exact,
    vittf_layernorm gives the same h."""
    lib = _lib.load()
    w = td.wide_case()
    t, code, st = td.TDT[dt], _lib.DTYPES[dt], _lib.stream_ptr()
    ad, wd = w.a.to(t).to(gpu), w.w.to(t).to(gpu)
    bd, gd, ed = (v.float().to(gpu) for v in (w.bias, w.g, w.e))
    x = _guarded(w.x0, torch.float32, gpu, 2)
    h = torch.full((w.rows + 2, w.n), GUARD, dtype=t, device=gpu)
    hl = torch.full((w.rows + 2, w.n), GUARD, dtype=t, device=gpu)
    _lib.check(lib.vittf_gemm_residual_ln(_lib.ptr(ad), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(x), w.rows, w.n, w.k, code,
                                          _lib.ptr(gd), _lib.ptr(ed), td.LN_EPS, _lib.ptr(h), st), 'vittf_gemm_residual_ln')
    _lib.check(lib.vittf_layernorm(_lib.ptr(x), _lib.ptr(gd), _lib.ptr(ed), _lib.ptr(hl), w.rows, w.n, td.LN_EPS, code, st), 'vittf_layernorm')
    torch.cuda.synchronize()
    for buf, want, what in ((x, w.x, 'x'), (h, w.h, 'h of the epilogue'), (hl, w.h, 'h of vittf_layernorm')):
        got = buf.float().cpu().double()
        _check_guards(got, w.rows, what)
        diff = _first_difference(got[:w.rows], want, what)
        assert diff is None, diff
