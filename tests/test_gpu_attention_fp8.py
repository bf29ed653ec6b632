"""GPU: the fp8 (e4m3, block-scaled MFMA) attention path -- vittf_attention_fp8 (one scale per (slice, head)),
vittf_gemm_qkv_fp8 + vittf_attention_fp8_rows (q and k with one scale per row and 32-wide block) -- per element and per
32-row block, where test_gpu_kernels.py::test_attention_fp8 / test_qkv_fp8_rows_path have global norms only.

Exact cases (tests/fp8_data.py::exact_case, its properties checked on the CPU by tests/test_fp8_data_cpu.py): integer
operands on the e4m3 grid and integer scores in exp2 units make every quantisation of the path exact and every P an exact
power of two whatever running maximum the kernel holds; what is left is the output's one rounding to the 16-bit type.
Every (slice, head, third) has its own power-of-two magnitude, so an exponent taken from the wrong head, slice, third, row
or key tile shows.  Every output buffer carries guard rows of 7.0."""
import functools

import pytest
import torch

from vit_tf_amd import _lib
import fp8_data as fd

pytestmark = pytest.mark.gpu

TDT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
EPS = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}      # half-ulp relative rounding error of the 16-bit type
GUARD = 3
R_BLOCK = 1.5                                      # criterion (E): margin over the full model's own per-block error


def _attn(gpu, entry, qkv_dev, batch, tokens, heads, dt, ws):
    """One call of vittf_attention_fp8 / vittf_attention_fp8_rows -> the 16-bit output rows (on the device), guards checked."""
    lib = _lib.load()
    rows, d = batch * tokens, heads * 64
    out = torch.full((rows + GUARD, d), 7.0, dtype=TDT[dt], device=gpu)
    _lib.check(getattr(lib, entry)(_lib.ptr(qkv_dev), _lib.ptr(out), batch, tokens, heads, _lib.DTYPES[dt], _lib.ptr(ws),
                                   ws.numel(), _lib.stream_ptr()), entry)
    torch.cuda.synchronize()
    assert (out[rows:].float() == 7.0).all(), 'wrote past the last row'
    return out[:rows].clone()


def _ws(gpu, batch, tokens, heads, fill=0xff):
    lay = fd.Layout(batch, tokens, heads)
    assert lay.total == _lib.load().vittf_attention_fp8_workspace_bytes(batch, tokens, heads)
    return torch.full((lay.total,), fill, dtype=torch.uint8, device=gpu)


def _gemm(gpu, a, w, bias, batch, tokens, heads, dt, ws, prefill=7.0, guard=GUARD):
    """vittf_gemm_qkv_fp8 into `ws` -> the qkv buffer (rows + guard rows; only the v third of the rows is written)."""
    lib = _lib.load()
    rows, n, k = batch * tokens, 3 * heads * 64, a.shape[1]
    qkv = torch.full((rows + guard, n), prefill, dtype=TDT[dt], device=gpu)
    _lib.check(lib.vittf_gemm_qkv_fp8(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(qkv), rows, n, k, tokens, heads,
                                      _lib.DTYPES[dt], _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), 'vittf_gemm_qkv_fp8')
    torch.cuda.synchronize()
    return qkv


@functools.lru_cache(maxsize=None)
def _exact_want(batch, tokens, heads, jump):
    """The exact case and its fp64 attention: computed once, shared by both 16-bit types and both entry points."""
    c = fd.exact_case(batch, tokens, heads, fd.case_seed(batch, tokens, heads), jump)
    return c, fd.exact(c.qkv, batch, tokens, heads)


def _assert_exact(got16, c, want, dt, what):
    """|got - want| <= 1.01 EPS |want| + tokens 2^-23 max|v|: one rounding of the output, plus the fp32 accumulation of
    P V and of the row sum (zero whenever the partial sums fit 24 bits).  Derived, not measured."""
    got = got16.float().cpu().double()
    assert torch.isfinite(got).all(), what
    vmax = float(c.qkv[:, 2 * c.heads * 64:].abs().max())
    excess = (got - want).abs() - (1.01 * EPS[dt] * want.abs() + c.tokens * 2.0 ** -23 * vmax)
    worst = int(excess.argmax())
    row, col = divmod(worst, want.shape[1])
    assert float(excess.max()) <= 0, (f'{what}: {int((excess > 0).sum())} of {excess.numel()} values outside the bound; worst at slice '
                                      f'{row // c.tokens} token {row % c.tokens} head {col // 64} dim {col % 64}: got '
                                      f'{float(got[row, col])!r}, want {float(want[row, col])!r}')


def _host_rows_ws(c, seed):
    """The exact case as vittf_gemm_qkv_fp8 would have left it: q8 / k8 rows = the integer operand times 2^x, x drawn per
    (row, 32-block) from 0..3 independently for q and k, scale byte = 127 - x + the (slice, head) exponent; the amax slot
    of v = max|v| of the (slice, head); rows tokens..np-1 zero; v8t and the unused slots 0xff."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = fd.split(c.qkv, c.batch, c.tokens, c.heads)
    xq = torch.randint(0, 4, (c.batch, c.heads, c.tokens, 2), generator=g)
    xk = torch.randint(0, 4, (c.batch, c.heads, c.tokens, 2), generator=g)
    a = c.a[:, :, None, None]
    lay = fd.Layout(c.batch, c.tokens, c.heads)
    ws = fd.rows_workspace(lay, q, k, a - xq, -a - xk, v.abs().amax(dim=(2, 3)))
    # (what was packed is the integer operand times 2^x, exactly)
    assert torch.equal(fd.unpack_rows(lay.rows(ws, 'q8')[:, :, :c.tokens], lay.scales(ws, 'qs')[:, :, :c.tokens]), q)
    assert torch.equal(fd.unpack_rows(lay.rows(ws, 'k8')[:, :, :c.tokens], lay.scales(ws, 'ks')[:, :, :c.tokens]), k)
    return ws


def _v_only(qkv16, heads, other=float('nan')):
    """The qkv buffer vittf_attention_fp8_rows gets: the v third; the q and k thirds hold what the GEMM never wrote."""
    out = qkv16.clone()
    out[:, :2 * heads * 64] = other
    return out


# ---------------------------------------------------------------------------------------------- (A) exact, head scales
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads', fd.HEAD_CASES)
def test_exact_head_scales(gpu, dt, batch, tokens, heads):
    """vittf_attention_fp8 on exact operands with uneven (slice, head) scales, workspace pre-filled with 0xff: every output
    value within one rounding of the fp64 softmax; a second call gives the same bytes."""
    c, want = _exact_want(batch, tokens, heads, None)
    qd = c.qkv.to(TDT[dt]).to(gpu)
    ws = _ws(gpu, batch, tokens, heads)
    got = _attn(gpu, 'vittf_attention_fp8', qd, batch, tokens, heads, dt, ws)
    _assert_exact(got, c, want, dt, 'head scales')
    again = _attn(gpu, 'vittf_attention_fp8', qd, batch, tokens, heads, dt, ws)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), 'a second call on the used workspace differs'


# ---------------------------------------------------------------------------------------------- (B) exact, late maximum
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('entry', ['vittf_attention_fp8', 'vittf_attention_fp8_rows'])
@pytest.mark.parametrize('batch,tokens,heads', fd.JUMP_CASES)
def test_exact_late_maximum(gpu, dt, entry, batch, tokens, heads):
    """Keys 12 exp2 units above everything in the tiles before them, for some query rows, in the first and the second
    32-key half of a middle tile and in the ragged last tile: the lane-half sum against the maximum of tile 0 is above 256
    (asserted by the generator), so the overflow branch (ps > 256: move M, rescale O and l) must be taken -- and the keys
    in front of the jump keep the weight they were rounded with.  Same bound as the plain exact cases, finite output."""
    c, want = _exact_want(batch, tokens, heads, True)
    q16 = c.qkv.to(TDT[dt])
    if entry == 'vittf_attention_fp8':
        got = _attn(gpu, entry, q16.to(gpu), batch, tokens, heads, dt, _ws(gpu, batch, tokens, heads))
    else:
        got = _attn(gpu, entry, _v_only(q16, heads).to(gpu), batch, tokens, heads, dt, _host_rows_ws(c, tokens).to(gpu))
    _assert_exact(got, c, want, dt, entry)


# ---------------------------------------------------------------------------------------------- (C) exact, row scales
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads', fd.ROWS_CASES)
def test_exact_row_scales_host_made_operands(gpu, dt, batch, tokens, heads):
    """vittf_attention_fp8_rows called alone, on a workspace the test fills as vittf_gemm_qkv_fp8 would have: every
    (row, 32-block) of q and of k has its own scale byte, every (slice, head) its own magnitude.  A scale operand that is
    stale (the previous key tile's), another row's, another block's or another head's moves the scores by whole binades.
    From 65 tokens up: several key tiles.  (The hazard attention_fp8.hip::scale_operand guards against was found by an
    earlier, throw-away form of this test.)"""
    c, want = _exact_want(batch, tokens, heads, None)
    ws = _host_rows_ws(c, 7 * tokens + heads).to(gpu)
    qd = _v_only(c.qkv.to(TDT[dt]), heads).to(gpu)
    got = _attn(gpu, 'vittf_attention_fp8_rows', qd, batch, tokens, heads, dt, ws)
    _assert_exact(got, c, want, dt, 'row scales')
    again = _attn(gpu, 'vittf_attention_fp8_rows', qd, batch, tokens, heads, dt, ws)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), 'a second call on the used workspace differs'


# ---------------------------------------------------------------------------------------------- (D) exact producer
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads,k', [(3, 65, 12, 768), (2, 200, 12, 768), (2, 257, 4, 832), (5, 17, 4, 832),
                                                  (1, 300, 16, 1024), (2, 256, 16, 1024), (3, 300, 4, 832)])
def test_exact_producer(gpu, dt, batch, tokens, heads, k):
    """vittf_gemm_qkv_fp8 on integer operands (every accumulator a small integer, exact in fp32), slices and heads of
    different magnitude; slice boundaries inside 256-row tiles (65, 200, 257, 300 tokens), on a tile edge (256) and more
    than two slices per tile (17 tokens: the b = m / tokens branch).  Bit for bit against the host emulation of the
    epilogue: k third = block maximum -> scale_exp -> e4m3(value * 2^-e); q third the same on float32(acc + bias) *
    float32(log2(e) / 8), one multiply; padded rows zero; v third = vittf_gemm(EPI_BIAS_QKV)'s bits; and the amax slot
    [bh * 3 + 2], as float bits, = max|acc + bias| of that (slice, head) exactly."""
    lib = _lib.load()
    a, w, bias = fd.exact_gemm_case(batch, tokens, heads, k, batch * 100 + tokens)
    rows, d = batch * tokens, heads * 64
    a16, w16 = a.to(TDT[dt]), w.to(TDT[dt])
    assert torch.equal(a16.double(), a) and torch.equal(w16.double(), w)
    ad, wd, bd = a16.to(gpu), w16.to(gpu), bias.float().to(gpu)
    ws = _ws(gpu, batch, tokens, heads)
    qkv = _gemm(gpu, ad, wd, bd, batch, tokens, heads, dt, ws)
    acc = a @ w.t() + bias                                                      # integers (times powers of two): exact
    assert float(acc.abs().max()) < 2.0 ** 24 and torch.equal(acc.float().double(), acc)
    plain = torch.empty(rows, 3 * d, dtype=TDT[dt], device=gpu)
    _lib.check(lib.vittf_gemm(_lib.ptr(ad), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(plain), rows, 3 * d, k, _lib.EPI_BIAS_QKV, 0,
                              _lib.DTYPES[dt], _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(qkv[:rows, 2 * d:], plain[:, 2 * d:]), 'v third'
    assert (qkv[rows:].float() == 7.0).all() and (qkv[:rows, :2 * d].float() == 7.0).all(), 'wrote outside the v third'
    assert torch.equal(plain[:, 2 * d:].cpu().double(), acc[:, 2 * d:].to(TDT[dt]).double()), 'v values'
    lay = fd.Layout(batch, tokens, heads)
    wsc = ws.cpu()
    q32 = (acc[:, :d].float().numpy() * fd.QSCALE32)                            # one float32 multiply, as the epilogue does
    thirds = {'q': torch.from_numpy(q32).double(), 'k': acc[:, d:2 * d], 'v': acc[:, 2 * d:]}
    per_head = lambda x: x.view(batch, tokens, heads, 64).transpose(1, 2)       # (batch, heads, tokens, 64)
    for name, p8, ps in (('q', 'q8', 'qs'), ('k', 'k8', 'ks')):
        val = per_head(thirds[name])
        e = fd.scale_exp(val.reshape(batch, heads, tokens, 2, 32).abs().amax(dim=-1))
        want_b, want_s = fd.pack_rows(val, e)
        got_b, got_s = lay.rows(wsc, p8), lay.scales(wsc, ps)
        assert torch.equal(got_s[:, :, :tokens], want_s), f'{name}: {int((got_s[:, :, :tokens] != want_s).sum())} scale bytes differ'
        assert torch.equal(got_b[:, :, :tokens], want_b), f'{name}: {int((got_b[:, :, :tokens] != want_b).sum())} bytes differ'
        assert (got_b[:, :, tokens:] == 0).all() and (got_s[:, :, tokens:] == 0).all(), f'{name}: padded rows'
    vmax = per_head(thirds['v']).abs().amax(dim=(2, 3)).float()
    got_amax = lay.amax(wsc)[:, :, 2]
    assert len(set(vmax.flatten().tolist())) >= min(batch * heads, 4), 'the (slice, head) maxima should differ'
    assert torch.equal(got_amax, vmax.view(torch.int32)), \
        f'amax of v: got {got_amax.view(torch.float32).flatten().tolist()}, want {vmax.flatten().tolist()}'


# ---------------------------------------------------------------------------------------------- (E) real-valued, per block
def _assert_blocks(got16, exact, full, batch, tokens, heads, dt, what):
    """For every (slice, head, 32-row block) B: err(got, exact; B) <= R_BLOCK * err(full model, exact; B) + EPS.
    -> the largest err(got) / err(full model) over the blocks."""
    got = got16.float().cpu().double()
    assert torch.isfinite(got).all(), what
    e_got = fd.block_errors(got, exact, batch, tokens, heads)
    e_ref = fd.block_errors(full, exact, batch, tokens, heads)
    ratio = float((e_got / e_ref).max())
    print(f'{what} {batch}x{tokens}x{heads} {dt}: per-block error {float(e_got.min()):.3e} .. {float(e_got.max()):.3e}, '
          f'largest ratio to the full model {ratio:.3f}')
    bad = e_got > R_BLOCK * e_ref + EPS[dt]
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} blocks outside the criterion, (slice, head, block) '
                                 f'{bad.nonzero()[:8].tolist()}: {e_got[bad][:8].tolist()} against {e_ref[bad][:8].tolist()}')
    return got


def _rel_fro(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads', [(2, 65, 2), (1, 200, 12), (2, 577, 2)])
def test_blocks_head_scales(gpu, dt, batch, tokens, heads):
    """vittf_attention_fp8 on the random input of test_attention_fp8 with uneven (slice, head) magnitudes: the two global
    bounds of that test (6e-2 against exact, 2e-2 against the operand model), and per (slice, head, 32-row block) the
    error against exact within 1.5 x the full model's own (fp8_data.full_model: e4m3 operands and P rounded against the
    row's global maximum) + EPS.  The kernel differs from that model only in the maximum P is rounded against and in the
    output's rounding; a host emulation of its lazy-maximum policy (fp8_data.lazy_model, asserted on these inputs by
    test_fp8_data_cpu.py) gives largest ratios of 1.01 (65 tokens), 1.19 (200) and 1.30 (577).
    Largest per-block ratio measured on an MI355X (fp16 / bf16): 2x65x2 1.011 / 1.007, 1x200x12 1.146 / 1.196,
    2x577x2 1.295 / 1.138 -- the emulation's figures."""
    qkv16 = fd.prescale16(fd.real_case(batch, tokens, heads, tokens + heads), heads, TDT[dt])
    ref = qkv16.double()
    exact, full = fd.exact(ref, batch, tokens, heads), fd.full_model(ref, batch, tokens, heads)
    got16 = _attn(gpu, 'vittf_attention_fp8', qkv16.to(gpu), batch, tokens, heads, dt, _ws(gpu, batch, tokens, heads))
    got = _assert_blocks(got16, exact, full, batch, tokens, heads, dt, 'head scales')
    e_exact, e_model = _rel_fro(got, exact), _rel_fro(got, fd.operand_model(ref, batch, tokens, heads))
    print(f'  rel fro {e_exact:.3e} vs exact, {e_model:.3e} vs the operand model')
    assert e_exact <= 6e-2 and e_model <= 2e-2


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads,k', [(3, 65, 12, 768), (2, 200, 12, 768), (1, 577, 12, 768),
                                                  (3, 65, 16, 1024), (2, 200, 16, 1024), (1, 577, 16, 1024)])
def test_blocks_rows_path(gpu, dt, batch, tokens, heads, k):
    """vittf_gemm_qkv_fp8 + vittf_attention_fp8_rows, ViT-B (12 heads, K = 768) and ViT-L (16 heads, K = 1024) widths, heads
    and slices of different magnitude (fp8_data.real_gemm_case): the two global bounds of test_qkv_fp8_rows_path and the
    per-block criterion of test_blocks_head_scales, exact = the fp64 attention of the fp64 projection, the models with q
    and k rounded per (row, 32-block) and v from its 16-bit values.
    Largest per-block ratio measured on an MI355X (fp16 / bf16):
      3x65x12 1.014 / 1.016    2x200x12 1.298 / 1.383    1x577x12 1.426 / 1.383
      3x65x16 1.122 / 1.041    2x200x16 1.238 / 1.311    1x577x16 1.486 / 1.468
    The ratio has a tail that grows with the number of blocks (304 at 1x577x16).  The host emulation of the lazy-maximum
    policy on the fp64 projection of the same operands gives 1.487 / 1.453 at 1x577x16 and 1.425 / 1.376 at 1x577x12: the
    figures are the policy's on these inputs, not an error of the kernel's own."""
    a, w, bias = fd.real_gemm_case(batch, tokens, heads, k, tokens * 7 + batch + heads)
    rows, d = batch * tokens, heads * 64
    ad, wd, bd = a.to(TDT[dt]).to(gpu), w.to(TDT[dt]).to(gpu), bias.to(gpu)
    ws = _ws(gpu, batch, tokens, heads)
    qkv = _gemm(gpu, ad, wd, bd, batch, tokens, heads, dt, ws)
    got16 = _attn(gpu, 'vittf_attention_fp8_rows', qkv, batch, tokens, heads, dt, ws)
    proj = (ad.double() @ wd.double().t() + bd.double()).cpu()
    proj[:, :d] *= 0.125 * 1.4426950408889634
    v16 = qkv[:rows, 2 * d:].cpu().double()
    assert _rel_fro(v16, proj[:, 2 * d:]) <= EPS[dt]
    exact, full = fd.exact(proj, batch, tokens, heads), fd.full_model(proj, batch, tokens, heads, rows=True, v16=v16)
    got = _assert_blocks(got16, exact, full, batch, tokens, heads, dt, 'rows path')
    e_exact, e_model = _rel_fro(got, exact), _rel_fro(got, fd.operand_model(proj, batch, tokens, heads, rows=True, v16=v16))
    print(f'  rel fro {e_exact:.3e} vs exact, {e_model:.3e} vs the MX-operand model')
    assert e_exact <= 6e-2 and e_model <= 2e-2


# ---------------------------------------------------------------------------------------------- (F) peaked softmax
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
def test_peaked_softmax(gpu, dt):
    """The input of test_attention_rescale_branch (333 tokens; single keys matching single query rows with gains 12 and 60,
    in the first tile, both halves of middle tiles and the ragged last tile: scores of several hundred exp2 units, the
    overflow branch on real values), on both entry points (the row-scale operands made on the host).  Asserted: finite
    output and the per-block criterion of test_blocks_head_scales.  NOT the path's 6e-2 against exact: a 2^-4 relative error
    of an operand on a score of several hundred exp2 units is large, and the CPU models themselves are at 5.6e-2 .. 7.1e-2
    globally and up to 0.15 per block here -- the stated error of the path is that of a diffuse softmax (include/vittf.h).
    Largest per-block ratio measured on an MI355X, the same on both entry points: gain 12 1.306 (fp16) / 1.203 (bf16),
    gain 60 1.016 / 1.007 -- the emulation's figures (1.307 / 1.203, 1.016 / 1.007)."""
    for gain, batch, tokens, heads, qkv in fd.peaked_case():
        qkv16 = fd.prescale16(qkv, heads, TDT[dt])
        ref = qkv16.double()
        exact = fd.exact(ref, batch, tokens, heads)
        got16 = _attn(gpu, 'vittf_attention_fp8', qkv16.to(gpu), batch, tokens, heads, dt, _ws(gpu, batch, tokens, heads))
        _assert_blocks(got16, exact, fd.full_model(ref, batch, tokens, heads), batch, tokens, heads, dt, f'peaked, gain {gain}: head scales')
        q, k, v = fd.split(ref, batch, tokens, heads)
        blockexp = lambda x: fd.scale_exp(x.reshape(batch, heads, tokens, 2, 32).abs().amax(dim=-1))
        ws = fd.rows_workspace(fd.Layout(batch, tokens, heads), q, k, blockexp(q), blockexp(k), v.abs().amax(dim=(2, 3)))
        got16 = _attn(gpu, 'vittf_attention_fp8_rows', _v_only(qkv16, heads).to(gpu), batch, tokens, heads, dt, ws.to(gpu))
        _assert_blocks(got16, exact, fd.full_model(ref, batch, tokens, heads, rows=True), batch, tokens, heads, dt,
                       f'peaked, gain {gain}: row scales')


# ---------------------------------------------------------------------------------------------- (G) poisoned surroundings
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('tokens', [65, 577])
def test_poisoned_surroundings(gpu, dt, tokens):
    """80 rows of NaN bit patterns behind the qkv buffer and a workspace of 0xff bytes (NaN as e4m3, NaN as an E8M0 scale),
    against zero rows and a zeroed workspace: finite and the same bits, on both entry points.  The ragged last key tile
    and the clamped query rows of the last workgroup reach past the last token; P = 0 times a NaN would poison the row.
    For vittf_attention_fp8_rows the GEMM runs first, on the pre-filled workspace and into the pre-filled qkv buffer (whose
    q and k thirds it never writes)."""
    batch, heads, k, pad = 2, 12, 768, 80
    d, rows = heads * 64, batch * tokens
    qkv16 = fd.prescale16(fd.real_case(batch, tokens, heads, tokens), heads, TDT[dt])
    a, w, bias = fd.real_gemm_case(batch, tokens, heads, k, tokens)
    ad, wd, bd = a.to(TDT[dt]).to(gpu), w.to(TDT[dt]).to(gpu), bias.to(gpu)
    outs = {}
    for name, behind, fill in (('poisoned', float('nan'), 0xff), ('clean', 0.0, 0x00)):
        buf = torch.cat([qkv16, torch.full((pad, 3 * d), behind).to(TDT[dt])]).to(gpu)
        assert name == 'clean' or bool(torch.isnan(buf[rows:].float()).all())
        head = _attn(gpu, 'vittf_attention_fp8', buf, batch, tokens, heads, dt, _ws(gpu, batch, tokens, heads, fill))
        ws = _ws(gpu, batch, tokens, heads, fill)
        qkv = _gemm(gpu, ad, wd, bd, batch, tokens, heads, dt, ws, prefill=behind, guard=pad)
        assert bool(torch.isnan(qkv[rows:].float()).all() if name == 'poisoned' else (qkv[rows:] == 0).all())
        outs[name] = (head, _attn(gpu, 'vittf_attention_fp8_rows', qkv, batch, tokens, heads, dt, ws))
    for i, entry in enumerate(('vittf_attention_fp8', 'vittf_attention_fp8_rows')):
        assert torch.isfinite(outs['poisoned'][i].float()).all(), entry
        assert torch.equal(outs['poisoned'][i].view(torch.int16), outs['clean'][i].view(torch.int16)), entry
    exact = fd.exact(qkv16.double(), batch, tokens, heads)
    assert _rel_fro(outs['clean'][0].float().cpu().double(), exact) <= 6e-2


# ---------------------------------------------------------------------------------------------- (H) refusals
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
def test_refusals(gpu, dt):
    """A workspace misaligned by 128 bytes and tokens = 0: VITTF_ERR_INVALID_ARG (-1) on all three entry points, and
    nothing written."""
    lib = _lib.load()
    batch, tokens, heads, k = 1, 65, 12, 768
    d, rows = heads * 64, batch * tokens
    qkv = torch.zeros(rows, 3 * d, dtype=TDT[dt], device=gpu)
    out = torch.full((rows, d), 7.0, dtype=TDT[dt], device=gpu)
    a = torch.zeros(rows, k, dtype=TDT[dt], device=gpu)
    w = torch.zeros(3 * d, k, dtype=TDT[dt], device=gpu)
    bias = torch.zeros(3 * d, device=gpu)
    total = fd.Layout(batch, tokens, heads).total
    ws = torch.full((total + 256,), 0xff, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    st, dtv = _lib.stream_ptr(), _lib.DTYPES[dt]
    for wsp, tok in ((ws.data_ptr() + 128, tokens), (ws.data_ptr(), 0)):
        assert lib.vittf_attention_fp8(_lib.ptr(qkv), _lib.ptr(out), batch, tok, heads, dtv, wsp, total, st) == -1
        assert lib.vittf_attention_fp8_rows(_lib.ptr(qkv), _lib.ptr(out), batch, tok, heads, dtv, wsp, total, st) == -1
        assert lib.vittf_gemm_qkv_fp8(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(qkv), rows, 3 * d, k, tok, heads, dtv,
                                      wsp, total, st) == -1
    torch.cuda.synchronize()
    assert (ws == 0xff).all() and (out.float() == 7.0).all() and (qkv.float() == 0).all()
