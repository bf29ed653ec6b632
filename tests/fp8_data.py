"""Host-only data and references for the fp8 (e4m3, block-scaled MFMA) attention tests: numpy / torch on the CPU, no GPU,
no library call.  The number-format rules and the workspace layout of csrc/fp8_rows.h are mirrored here ONCE, so that the
tests can make the operands themselves (and read back what the producer left) instead of trusting the code under test.

Conventions: a `qkv` is a (batch * tokens, 3 * heads * 64) tensor as the kernels take it -- q pre-scaled, so that the
scores q . k are in exp2 units; q / k / v operands are (batch, heads, tokens, 64) float64 tensors."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

KT = 64                                   # keys per tile (fp8_rows.h::FP8_KT): rows of a (slice, head) are padded to np
QSCALE32 = np.float32(0.125 * 1.44269504088896340736)      # what the qkv epilogue multiplies the q third by, in float32


# ---------------------------------------------------------------------------------------------- number formats
def e4m3(x):
    """Round to OCP e4m3 (torch.float8_e4m3fn, round-to-nearest-even) through fp32, and back to fp64."""
    return torch.as_tensor(x).to(torch.float32).to(torch.float8_e4m3fn).to(torch.float64)


def e4m3_bytes(x):
    return torch.as_tensor(x).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


def scale_exp(amax):
    """fp8_rows.h::scale_exp in float32: the exponent e of frexp(amax / 448) -- amax * 2^-e lies in [224, 448) -- clamped
    below at -20, 0 for amax == 0.  Takes a scalar, an array or a tensor; returns an int64 tensor of the same shape."""
    a = torch.as_tensor(amax).detach().to(torch.float32).numpy()
    with np.errstate(under='ignore'):
        _, ex = np.frexp(a * np.float32(1.0 / 448.0))
    ex = np.where(a > 0, np.maximum(ex, -20), 0)
    return torch.from_numpy(np.asarray(ex, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- workspace layout
class Layout:
    """Mirror of fp8_rows.h::fp8_ws: amax | q8 | k8 | v8t | qs | ks, every piece 256-byte aligned.
    amax: float bits [slice][head][q | k | v]; q8 / k8: [slice][head][np][64] bytes, row index bh * np + tok;
    v8t: [slice][head][64 dims][np]; qs / ks: [slice][head][np][2] E8M0 bytes."""

    def __init__(self, batch, tokens, heads):
        self.batch, self.tokens, self.heads = batch, tokens, heads
        self.np = (tokens + KT - 1) // KT * KT
        self.per = batch * heads * self.np * 64
        self.amax_bytes = batch * heads * 3 * 4
        self.sc_bytes = batch * heads * self.np * 2
        up = lambda n: (n + 255) // 256 * 256
        self.off = {'amax': 0, 'q8': up(self.amax_bytes)}
        self.off['k8'] = self.off['q8'] + self.per
        self.off['v8t'] = self.off['k8'] + self.per
        self.off['qs'] = self.off['v8t'] + self.per
        self.off['ks'] = self.off['qs'] + up(self.sc_bytes)
        self.total = self.off['ks'] + up(self.sc_bytes)

    def row_index(self, bh, tok):
        return bh * self.np + tok

    def rows(self, ws, piece):
        """q8 / k8 of a workspace (uint8 tensor) as a (batch, heads, np, 64) view."""
        o = self.off[piece]
        return ws[o:o + self.per].view(self.batch, self.heads, self.np, 64)

    def scales(self, ws, piece):
        """qs / ks as a (batch, heads, np, 2) view."""
        o = self.off[piece]
        return ws[o:o + self.sc_bytes].view(self.batch, self.heads, self.np, 2)

    def amax(self, ws):
        """The absolute maxima as int32 float bits, (batch, heads, 3)."""
        return ws[:self.amax_bytes].view(torch.int32).view(self.batch, self.heads, 3)


def _to_stored(x):
    """natural dims (..., 64) -> stored order [d 0-15 | d 32-47 | d 16-31 | d 48-63] (fp8_rows.h::fp8_row_pos)."""
    return x.reshape(*x.shape[:-1], 2, 2, 16).transpose(-3, -2).reshape(*x.shape[:-1], 64)


def pack_rows(values, block_exponents):
    """Rows with block scales as the matrix instruction reads them: values (..., 64) in natural dim order, one exponent e
    per 32-wide block (..., 2).  -> (bytes (..., 64): e4m3(value * 2^-e) in stored order, scale bytes (..., 2): 127 + e,
    scale byte index dim >> 5)."""
    v = torch.as_tensor(values, dtype=torch.float64)
    e = torch.as_tensor(block_exponents, dtype=torch.int64)
    scaled = v.reshape(*v.shape[:-1], 2, 32) * (2.0 ** (-e.double()))[..., None]
    b = e4m3_bytes(scaled.reshape(v.shape))
    return _to_stored(b).contiguous(), (127 + e).to(torch.uint8)


def unpack_rows(row_bytes, scale_bytes):
    """Inverse of pack_rows: the de-quantised values (..., 64) in natural dim order, float64."""
    nat = _to_stored(row_bytes)                                       # the permutation is its own inverse
    v = nat.contiguous().view(torch.float8_e4m3fn).to(torch.float64)
    s = 2.0 ** (scale_bytes.to(torch.float64) - 127.0)
    return (v.reshape(*v.shape[:-1], 2, 32) * s[..., None]).reshape(v.shape)


def rows_workspace(lay, q, k, eq, ek, vmax, fill=0xff):
    """The workspace as vittf_gemm_qkv_fp8 leaves it for vittf_attention_fp8_rows, made on the host: q8 / k8 rows
    0..tokens-1 = pack_rows(q, eq) / pack_rows(k, ek), rows tokens..np-1 zero bytes and zero scale bytes, the amax slot
    [bh * 3 + 2] the float bits of vmax (batch, heads); v8t and everything unused = `fill`."""
    ws = torch.full((lay.total,), fill, dtype=torch.uint8)
    for x, e, p8, ps in ((q, eq, 'q8', 'qs'), (k, ek, 'k8', 'ks')):
        by, sc = pack_rows(x, e)
        r, s = lay.rows(ws, p8), lay.scales(ws, ps)
        r[:, :, :lay.tokens], r[:, :, lay.tokens:] = by, 0
        s[:, :, :lay.tokens], s[:, :, lay.tokens:] = sc, 0
    lay.amax(ws)[:, :, 2] = torch.as_tensor(vmax).to(torch.float32).view(torch.int32)
    return ws


# ---------------------------------------------------------------------------------------------- references
def split(qkv, batch, tokens, heads):
    """qkv (batch * tokens, 3 * heads * 64) -> q, k, v as (batch, heads, tokens, 64) float64."""
    x = torch.as_tensor(qkv).double().view(batch, tokens, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def merge(o):
    """(batch, heads, tokens, 64) -> (batch * tokens, heads * 64)."""
    b, h, t, _ = o.shape
    return o.transpose(1, 2).reshape(b * t, h * 64)


def quant_head(x):
    """e4m3 with ONE power-of-two scale per (slice, head): the head-scale path, and v on both paths."""
    e = scale_exp(x.abs().amax(dim=(2, 3), keepdim=True)).double()
    return e4m3(x * 2.0 ** -e) * 2.0 ** e


def quant_rows(x):
    """e4m3 with one power-of-two scale per (row, 32-wide block): q and k on the row-scale path."""
    t = x.reshape(*x.shape[:-1], 2, 32)
    e = scale_exp(t.abs().amax(dim=-1, keepdim=True)).double()
    return (e4m3(t * 2.0 ** -e) * 2.0 ** e).reshape(x.shape)


def _softmax_v(q, k, v, round_p):
    s = q @ k.transpose(-2, -1)
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    pr = e4m3(2.0 * p) / 2.0 if round_p else p
    return merge((pr @ v) / p.sum(dim=-1, keepdim=True))


def _operands(qkv, batch, tokens, heads, rows, v16):
    q, k, v = split(qkv, batch, tokens, heads)
    if v16 is not None:
        v = split(v16, batch, tokens, heads)[2] if v16.shape[-1] == 3 * heads * 64 else \
            torch.as_tensor(v16).double().view(batch, tokens, heads, 64).transpose(1, 2)
    qq = quant_rows if rows else quant_head
    return qq(q), qq(k), quant_head(v)


def exact(qkv, batch, tokens, heads):
    """fp64 softmax attention of the inputs as they are."""
    return _softmax_v(*split(qkv, batch, tokens, heads), round_p=False)


def operand_model(qkv, batch, tokens, heads, rows=False, v16=None):
    """q, k, v rounded to e4m3 with the path's scales (rows: q and k per (row, 32-block)), the rest in fp64.  v16: the v
    third (or a whole qkv) that replaces qkv's -- the 16-bit values the row-scale path quantises v from."""
    return _softmax_v(*_operands(qkv, batch, tokens, heads, rows, v16), round_p=False)


def full_model(qkv, batch, tokens, heads, rows=False, v16=None):
    """operand_model plus P = e4m3(2 * 2^(s - rowmax)) / 2 with the row's global maximum; the row sum over the unrounded
    p; the output left in fp64."""
    return _softmax_v(*_operands(qkv, batch, tokens, heads, rows, v16), round_p=True)


def lazy_model(qkv, batch, tokens, heads, rows=False, v16=None):
    """full_model with the kernel's lazy maximum in place of the row's global one (a host emulation of the policy, fp64
    arithmetic): M is set by tile 0 so that the tile's maximum p is 2, and moved again -- to this tile's maximum, never
    down -- only in a tile where one of the 32 query rows of the wave has a lane-half sum of p above 256.  What was
    accumulated under an earlier M is rescaled, not re-rounded: keys far below a LATER maximum keep the precision they
    were rounded with, where full_model flushes them to zero."""
    q, k, v = _operands(qkv, batch, tokens, heads, rows, v16)
    nt = (tokens + KT - 1) // KT
    nb = (tokens + 31) // 32
    s = q @ k.transpose(-2, -1)
    s = torch.cat([s, s.new_full((batch, heads, tokens, nt * KT - tokens), -float('inf'))], dim=-1)
    vp = torch.cat([v, v.new_zeros(batch, heads, nt * KT - tokens, 64)], dim=2)
    half = torch.tensor([lane_half(kin) for kin in range(KT)])
    m = s.new_zeros(batch, heads, tokens, 1)
    acc = s.new_zeros(batch, heads, tokens, 64)
    l = s.new_zeros(batch, heads, tokens, 1)
    for t in range(nt):
        st = s[..., t * KT:(t + 1) * KT]
        p = torch.exp2(st - m)
        over = torch.maximum(p[..., half == 0].sum(-1), p[..., half == 1].sum(-1)) > 256.0            # (batch, heads, tokens)
        over = torch.cat([over, over.new_zeros(batch, heads, nb * 32 - tokens)], dim=-1)
        wave = over.view(batch, heads, nb, 32).any(dim=-1).repeat_interleave(32, dim=-1)[..., :tokens, None]
        target = st.amax(dim=-1, keepdim=True) - 1.0
        m_new = target if t == 0 else torch.where(wave, torch.maximum(target, m), m)
        alpha = torch.exp2(m - m_new)
        acc, l, m = acc * alpha, l * alpha, m_new
        p = torch.exp2(st - m)
        acc = acc + e4m3(p) @ vp[:, :, t * KT:(t + 1) * KT]
        l = l + p.sum(dim=-1, keepdim=True)
    return merge(acc / l)


def block_errors(got, ref, batch, tokens, heads):
    """Relative Frobenius error per (slice, head, 32-query-row block): (batch, heads, ceil(tokens / 32))."""
    nb = (tokens + 31) // 32

    def blocks(x):
        x = torch.as_tensor(x).double().view(batch, tokens, heads, 64)
        x = torch.cat([x, x.new_zeros(batch, nb * 32 - tokens, heads, 64)], dim=1)
        return x.view(batch, nb, 32, heads, 64).permute(0, 3, 1, 2, 4).reshape(batch, heads, nb, 32 * 64)
    g, r = blocks(got), blocks(ref)
    return (g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-30)


def uneven_exponents(batch, heads):
    """The (slice, head) exponents of the uneven-scale cases: q * 2^a, k * 2^-a, v * 2^c -- the scores do not change, every
    (slice, head, third) gets its own scale, neighbouring heads and neighbouring slices differ."""
    b = torch.arange(batch).view(batch, 1)
    h = torch.arange(heads).view(1, heads)
    return (3 * b + 5 * h) % 9 - 4, (2 * b + 3 * h) % 7 - 3


def apply_uneven(q, k, v):
    a, c = uneven_exponents(q.shape[0], q.shape[1])
    f = lambda e: (2.0 ** e.double())[..., None, None]
    return q * f(a), k * f(-a), v * f(c)


def to_qkv(q, k, v):
    """q, k, v (batch, heads, tokens, 64) -> (batch * tokens, 3 * heads * 64)."""
    return torch.cat([merge(q), merge(k), merge(v)], dim=1)


# ---------------------------------------------------------------------------------------------- exact cases
def lane_half(kin):
    """Lane half that holds key kin (0..63) of a tile: keys (r & 3) + 8 (r >> 2) + 4 h of each 32-key block."""
    return ((kin & 31) >> 2) & 1


# A jump key's entry on its jump dim; the entry of every other key from the start of the jump key's tile on.  (The keys of
# the jump's own tile are lifted too: the kernel meets a tile as a whole, and an unlifted key next to the jump would be
# more than 8 below the maximum that tile sets.  The jump is 9 or more above everything in the tiles before it.)
JUMP, LIFT = 12, 8


def jump_keys(tokens):
    """(i) first 32-key half of a middle tile, (ii) second half of a middle tile, (iii) the ragged last tile."""
    nt = (tokens + KT - 1) // KT
    assert nt >= 3 and tokens % KT != 0, 'a jump case needs a middle tile and a ragged last tile'
    last0 = KT * (nt - 1)
    return KT * 1 + 5, KT * (nt - 2) + 40, last0 + (tokens - last0 - 1) // 2


def running_max_ok(s):
    """The condition under which P is an exact power of two on the e4m3 grid whatever maximum the kernel keeps: for every
    row and every key j of 64-key tile t, s_ij >= max(s_i over tiles 0..t) - 8.  (The kernel's M is always some tile maximum
    seen so far minus 1, and it never lets p exceed 256: p = 2^(s - M) lies in [2^-7, 2^8].)"""
    t = s.shape[-1]
    nt = (t + KT - 1) // KT
    pad = torch.cat([s, s.new_full((*s.shape[:-1], nt * KT - t), -float('inf'))], dim=-1)
    run = pad.view(*s.shape[:-1], nt, KT).amax(dim=-1).cummax(dim=-1).values           # max over tiles 0..t
    return bool((s >= run.repeat_interleave(KT, dim=-1)[..., :t] - 8).all())


def overflow_sums(s):
    """Per (..., row, tile >= 1, lane half): the sum over the half's 32 keys of 2^(s - (tile-0 maximum - 1)) -- what the
    kernel's overflow check sees as long as M has not moved since tile 0."""
    t = s.shape[-1]
    nt = (t + KT - 1) // KT
    pad = torch.cat([s, s.new_full((*s.shape[:-1], nt * KT - t), -float('inf'))], dim=-1).view(*s.shape[:-1], nt, KT)
    m0 = pad[..., 0, :].amax(dim=-1)
    p = torch.exp2(pad - (m0[..., None, None] - 1.0))
    half = torch.tensor([lane_half(kin) for kin in range(KT)])
    return torch.stack([p[..., half == 0].sum(-1), p[..., half == 1].sum(-1)], dim=-1)[..., 1:, :]


@functools.lru_cache(maxsize=None)
def exact_case(batch, tokens, heads, seed, jump=None):
    """Integer operands for which the whole fp8 path is exact up to the output's one rounding.
    Key rows are 0 / 1 with a few ones, query rows have three ones (scores: integers 0..3), v is uniform in -7..7; slice b
    / head h then carry q * 2^a, k * 2^-a, v * 2^c (uneven_exponents).  jump: dims 61..63 are set aside; query rows i with
    i % 5 == 1 + g carry a one on dim 61 + g (i % 5 == 4: on all three), key jump_keys(tokens)[g] carries JUMP there and
    every other key from the start of its tile on LIFT, so that the running-maximum condition still holds.
    -> .q .k .v integer-valued (batch, heads, tokens, 64) before the scales, .a .c the exponents (batch, heads),
       .qkv the scaled (batch * tokens, 3 * heads * 64) float64 input, .scores (batch, heads, tokens, tokens)."""
    g = torch.Generator().manual_seed(seed)
    base = 61 if jump else 64
    perm = torch.stack([torch.randperm(base, generator=g) for _ in range(batch * heads)]).view(batch, heads, base)
    i = torch.arange(tokens)
    q = torch.zeros(batch, heads, tokens, 64, dtype=torch.float64)
    k = torch.zeros_like(q)
    for j in range(3):                                                   # three ones per query row, walking through all dims
        q.scatter_(3, perm[:, :, (3 * i + j) % base].unsqueeze(-1), 1.0)
    k[..., :base] = (torch.rand(batch, heads, tokens, base, generator=g) < 0.3).double()
    k.scatter_(3, perm.flip(-1)[:, :, i % base].unsqueeze(-1), 1.0)      # and every dim in some key row
    v = torch.randint(-7, 8, (batch, heads, tokens, 64), generator=g).double()
    if jump:
        for grp, key in enumerate(jump_keys(tokens)):
            q[:, :, (i % 5 == 1 + grp) | (i % 5 == 4), 61 + grp] = 1.0
            k[:, :, key // KT * KT:, 61 + grp] = LIFT
            k[:, :, key, 61 + grp] = JUMP
    for x in (q, k, v):
        assert float(x.abs().max()) <= 15 and bool((x == x.round()).all())
    s = q @ k.transpose(-2, -1)
    assert running_max_ok(s), 'running-maximum condition'
    if jump:
        assert float(overflow_sums(s).max()) > 256.0, 'no lane-half sum above 256: the overflow branch need not be taken'
    a, c = uneven_exponents(batch, heads)
    return SimpleNamespace(q=q, k=k, v=v, a=a, c=c, scores=s, qkv=to_qkv(*apply_uneven(q, k, v)),
                           batch=batch, tokens=tokens, heads=heads, jump=jump)


# The cases of tests/test_gpu_attention_fp8.py, checked on the CPU by tests/test_fp8_data_cpu.py
TOKENS = (1, 31, 33, 63, 64, 65, 127, 128, 129, 192, 193, 257, 320, 577)
HEAD_CASES = [(b, t, h) for (b, h) in ((1, 1), (2, 3), (1, 12)) for t in TOKENS]           # (A)
ROWS_CASES = [(b, t, h) for (b, h) in ((2, 4), (1, 12)) for t in TOKENS if t >= 65]         # (C)
JUMP_CASES = [(2, 333, 2), (1, 129, 3)]                                                   # (B)


def case_seed(batch, tokens, heads):
    return 1000 * batch + 10 * tokens + heads


# ---------------------------------------------------------------------------------------------- real-valued cases
def prescale16(qkv, heads, dtype):
    """The q third multiplied by log2(e) / 8 in fp32, everything rounded once to the 16-bit type: what the engine's qkv
    epilogue hands to the attention kernels."""
    out = qkv.float().clone()
    out[:, :heads * 64] *= float(QSCALE32)
    return out.to(dtype)


def real_case(batch, tokens, heads, seed):
    """The random input of test_gpu_kernels.py::test_attention_fp8 (q, k of std 1.3, v of std 2 around 0.5) with the uneven
    (slice, head) factors 2^a / 2^-a / 2^c on top: fp32, q not yet pre-scaled."""
    g = torch.Generator().manual_seed(seed)
    d = heads * 64
    qkv = torch.randn(batch * tokens, 3 * d, generator=g)
    qkv[:, :2 * d] *= 1.3
    qkv[:, 2 * d:] = qkv[:, 2 * d:] * 2.0 + 0.5
    return to_qkv(*apply_uneven(*split(qkv, batch, tokens, heads))).float()


def peaked_case():
    """The input of test_gpu_kernels.py::test_attention_rescale_branch, both gains: (gain, batch, tokens, heads, qkv fp32)."""
    batch, tokens, heads = 1, 333, 2
    for gain in (12.0, 60.0):
        qkv = torch.randn(batch * tokens, 3 * heads * 64, generator=torch.Generator().manual_seed(4)) * 0.5
        q = qkv[:, :128].view(tokens, 2, 64)
        k = qkv[:, 128:256].view(tokens, 2, 64)
        for key_row in (5, 100, 200, 332):
            k[key_row, 0] = q[7 + key_row % 50, 0] * gain
        k[40, 1] = q[3, 1] * -gain
        yield gain, batch, tokens, heads, qkv


def real_gemm_case(batch, tokens, heads, k, seed):
    """Operands of the qkv projection, random as in test_gpu_kernels.py::test_qkv_fp8_rows_path, with uneven magnitudes: the
    q / k / v rows of head h of w (and of the bias) carry 2^a / 2^-a / 2^c of slice 0.  q and k are projected from the
    first 3 k / 4 columns, v from the last k / 4 alone, where slice b's rows of `a` carry 2^(b % 3); the last column of `a`
    is that factor itself and holds v's offset of 0.5 -- so v of slice b is 2^(b % 3) times what it would be in slice 0,
    q and k do not change.  -> a (rows, k), w (3 d, k), bias (3 d), fp32."""
    g = torch.Generator().manual_seed(seed)
    d, rows, tail = heads * 64, batch * tokens, k // 4
    a = torch.randn(rows, k, generator=g)
    w = torch.randn(3 * d, k, generator=g)
    w[:2 * d, :k - tail] *= 1.3 / (k - tail) ** 0.5
    w[2 * d:, k - tail:] *= 2.0 / (tail - 1) ** 0.5
    w[:2 * d, k - tail:] = 0.0
    w[2 * d:, :k - tail] = 0.0
    w[2 * d:, k - 1] = 0.5
    bias = 0.2 * torch.randn(3 * d, generator=g)
    ea, ec = uneven_exponents(batch, heads)
    f = torch.cat([2.0 ** ea[0].double(), 2.0 ** -ea[0].double(), 2.0 ** ec[0].double()]).repeat_interleave(64).float()
    w, bias = w * f[:, None], bias * f
    av = a.view(batch, tokens, k)
    av[:, :, k - 1] = 1.0
    av[:, :, k - tail:] *= (2.0 ** (torch.arange(batch) % 3)).view(batch, 1, 1)
    return a, w, bias


def exact_gemm_case(batch, tokens, heads, k, seed):
    """Integer operands of the qkv projection: |a| <= 3, sparse |w| <= 2, integer bias -- every accumulator is a small
    integer, exact in fp32 in any order.  Slice b's rows of `a` carry 2^(b % 3), head h's rows of w 2^(h % 4 - 1), so that
    slices and heads differ in magnitude.  -> a (rows, k), w (3 d, k), bias (3 d), float64, all exact in fp16 and bf16."""
    g = torch.Generator().manual_seed(seed)
    d, rows = heads * 64, batch * tokens
    a = torch.randint(-3, 4, (rows, k), generator=g).double()
    w = torch.randint(-2, 3, (3 * d, k), generator=g).double() * (torch.rand(3 * d, k, generator=g) < 24.0 / k)
    bias = torch.randint(-4, 5, (3 * d,), generator=g).double()
    a.view(batch, tokens, k).mul_((2.0 ** (torch.arange(batch) % 3).double()).view(batch, 1, 1))
    w.view(3, heads, 64, k).mul_((2.0 ** (torch.arange(heads) % 4 - 1).double()).view(1, heads, 1, 1))
    return a, w, bias
