"""Host-only data, references and stated conditions for the exact tests of the 16-bit attention kernels (attention.hip's
attn_kernel, attention_pp64.hip's attn_pp64_kernel): torch / numpy on the CPU, no GPU, no library call.

Conventions are tests/fp8_data.py's: a `qkv` is a (batch * tokens, 3 * heads * 64) tensor as vittf_attention takes it;
q / k / v operands are (batch, heads, tokens, 64) float64 tensors.  Both kernels work in 32-key half steps of 64-key tiles
and give a wave 32-query-row blocks; a lane holds one query row and the 16 keys of its lane half (fp8_data.lane_half).

(A1) selector_case: scores are 0 ("on") or a multiple of -4096, every weight is exactly 1 or 0, every row sum a power of two:
     the output is the mean of the on keys' v rows, rounded ONCE -- compared equal, for both kernels.
(A2) graded_case: integer scores in exp2 units, for attn_pp64_kernel.  pp64_model restates the kernel's lazy-maximum policy
     and checks, step by step, the condition under which every P, every row sum and every P.V sum is exact (graded_ok);
     expected = RN16(RN32(o * RN32(1 / l))), independent of the maximum the kernel keeps.
(A3) real_bound: a per-element bound for real-valued inputs, derived below."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import fp8_data as fd

KT, HS = 64, 32                                           # keys per tile, keys per half step
TDT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
EPS = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}             # half-ulp relative rounding error of the 16-bit type
U32 = 2.0 ** -24                                          # the same of float32
P_LIMIT = {'fp16': 8192.0, 'bf16': 2.0 ** 30}             # attention_pp64.hip::p_limit: a lane's sum of 16 P above it -> overflow branch
OFF = -4096.0                                             # an "off" entry of a selector key row
QSCALE32 = fd.QSCALE32                                    # log2(e) / 8 in float32: attn_kernel's c, the qkv epilogue's q factor


def rn16(x, dt):
    """Round once to the 16-bit type (through float32, which holds every value the callers pass exactly), back to fp64."""
    return torch.as_tensor(x).to(torch.float32).to(TDT[dt]).to(torch.float64)


def first_difference(got, want, batch, tokens, heads):
    """None if got == want as values, else a message naming the first differing (slice, token, head, dim).
    got / want: (batch * tokens, heads * 64)."""
    bad = (got != want) | torch.isnan(got)
    if not bool(bad.any()):
        return None
    row, col = (int(x) for x in bad.nonzero()[0])
    return (f'{int(bad.sum())} of {bad.numel()} elements differ, first at slice {row // tokens} token {row % tokens} '
            f'head {col // 64} dim {col % 64}: got {float(got[row, col])!r}, want {float(want[row, col])!r}')


# ---------------------------------------------------------------------------------------------- (A1) selector cases
def _pow2_floor(n):
    return 1 << (int(n).bit_length() - 1)


def selector_groups(tokens):
    """The on sets, placed where the kernels' paths change: [(name, sorted key list)], every size a power of two in 1..64."""
    n, nt = tokens, (tokens + KT - 1) // KT
    last0 = KT * (nt - 1)
    g = [('key 0 only', [0]), ('last key only', [n - 1])]
    for a in (32, 64):                                   # pairs across a half-step and a tile boundary
        if n > a:
            g.append((f'pair {a - 1}|{a}', [a - 1, a]))
    if nt >= 2 and last0 > 64:
        g.append(('last full tile | ragged tile', [last0 - 1, last0]))
    c = min(_pow2_floor(n - last0), 64)
    g.append(('all in the ragged last tile', list(range(n - c, n))))        # ends on the key next to the padding
    for a, c in ((32, 1), (64, 2), (128, 4)):            # the late maximum: the first on key after a all-off keys
        if n > a:
            c = min(c, _pow2_floor(n - a))
            g.append((f'first on key after {a} off keys', list(range(a, a + c))))
    if nt >= 2:                                          # one or more on keys in every tile
        c = 1
        while c < nt and c < 64:
            c *= 2
        for first in ((0,) if c >= nt else (0, nt - c)):             # more than 64 tiles: two sets that overlap
            span = min(nt - first, c)
            keys = set()
            for m in range(c):
                tile = first + m * span // c
                keys.add(KT * tile + (37 * m + 5) % min(KT, n - KT * tile))
            spare = (x for x in range(KT * first, n) if x not in keys)
            while len(keys) < c:                                     # two picks fell on one key of a short tile
                keys.add(next(spare))
            g.append((f'spread over tiles {first}..{first + span - 1}', sorted(keys)))
    rng = np.random.RandomState(tokens)
    for c in (8, 16, 32, 64):                            # scattered sets of every larger size
        if n >= 2 * c:
            g.append((f'{c} scattered keys', sorted(rng.choice(n, c, replace=False).tolist())))
    for name, keys in g:
        assert len(keys) == len(set(keys)) and len(keys) & (len(keys) - 1) == 0 and 1 <= len(keys) <= 64, name
        assert 0 <= min(keys) and max(keys) < n, name
    return g


@functools.lru_cache(maxsize=None)
def selector_case(batch, tokens, heads):
    """Group g owns the dims D_g (one dim for even g, three for odd g; a per-(slice, head) permutation of the 64 dims) and
    the on set K_g.  Query row i belongs to group (i + 5 bh) % G and carries ones on D_g; key row j carries 0 on D_g for
    every g with j in K_g, and -4096 elsewhere -- except that a key outside a three-dim group's on set still carries 0 on
    the first (j + g) % 3 of its dims (scores of -4096 and -8192 beside -12288: off at three levels), and that the dims no
    group owns, where every q is 0, carry 0 for (j + d) % 3 == 0.  v = n / 16 with integer 64 <= |n| <= 128, random per
    (slice, head, key, dim) with one sign per (slice, head, dim) -- the sum over a set of 32 or more has more than 11 bits,
    so the mean is not a 16-bit number -- times 2^c (fp8_data.uneven_exponents).
    -> .qkv float64 (batch * tokens, 3 * heads * 64), exact in fp16 and bf16; .want float64 (batch * tokens, heads * 64):
       the mean of the on set's v rows, not yet rounded; .q .k .v; .groups; .group_of (batch, heads, tokens);
       .on (batch, heads, G, tokens) bool."""
    groups = selector_groups(tokens)
    G = len(groups)
    width = [1 if g % 2 == 0 else 3 for g in range(G)]
    start = np.concatenate([[0], np.cumsum(width)])
    assert start[-1] <= 64
    gen = torch.Generator().manual_seed(7919 * batch + 31 * tokens + heads)
    j = torch.arange(tokens)
    q = torch.zeros(batch, heads, tokens, 64, dtype=torch.float64)
    k = torch.full((batch, heads, tokens, 64), OFF, dtype=torch.float64)
    n = torch.randint(64, 129, (batch, heads, tokens, 64), generator=gen).double()
    n = n * (2.0 * torch.randint(0, 2, (batch, heads, 1, 64), generator=gen).double() - 1.0)     # one sign per dim: sums grow
    _, c = fd.uneven_exponents(batch, heads)
    v = n / 16.0 * (2.0 ** c.double())[..., None, None]
    on = torch.zeros(batch, heads, G, tokens, dtype=torch.bool)
    for g, (_, keys) in enumerate(groups):
        on[:, :, g, keys] = True
    group_of = torch.zeros(batch, heads, tokens, dtype=torch.int64)
    want = torch.zeros_like(q)
    for b in range(batch):
        for h in range(heads):
            bh = b * heads + h
            perm = torch.randperm(64, generator=gen)
            free = perm[int(start[-1]):]
            k[b, h][:, free] = torch.where((j[:, None] + free[None, :]) % 3 == 0, 0.0, OFF).double()
            grp = (j + 5 * bh) % G
            group_of[b, h] = grp
            means = torch.zeros(G, 64, dtype=torch.float64)
            for g in range(G):
                dims = perm[int(start[g]):int(start[g + 1])]
                for m, d in enumerate(dims.tolist()):
                    decoy = (m < (j + g) % 3) if width[g] == 3 else torch.zeros(tokens, dtype=torch.bool)
                    k[b, h, :, d] = torch.where(on[b, h, g] | decoy, 0.0, OFF).double()
                    q[b, h, grp == g, d] = 1.0
                means[g] = v[b, h, on[b, h, g]].mean(dim=0)                  # O(tokens * 64) per head: no N x N matrix
            want[b, h] = means[grp]
    return SimpleNamespace(batch=batch, tokens=tokens, heads=heads, q=q, k=k, v=v, on=on, group_of=group_of, groups=groups,
                           qkv=fd.to_qkv(q, k, v), want=fd.merge(want))


def selector_weights(case):
    """The 0 / 1 weights (batch, heads, tokens, tokens) from the scores themselves: 1 where q . k == 0.  (Small cases only.)"""
    s = case.q @ case.k.transpose(-2, -1)
    return (s == 0).double(), s


def selector_model(case, variant=None):
    """fp64 model of attention on a selector case with one deliberate error -> (batch * tokens, heads * 64), unrounded.
    None: the correct result from the score matrix (must equal case.want).
    'padding_key': one zero-filled key behind the last token is let through the ragged-tile mask (score 0, v 0).
    'boundary_key_dropped': key 64 (32, then 0, for fewer tokens), the first of a tile or half step, contributes nothing.
    'last_key_not_in_row_sum': the row sum misses the last key, the numerator keeps it.
    'rescale_skipped': the lazy maximum M of a row is the maximum of its first 32 keys; when its first on key arrives the
        accumulated weights -- 1 for every earlier key at M -- are kept (alpha = 1) instead of multiplied by exp2(-4096) = 0.
    'v_rows_swapped': the v rows of the last two keys change places."""
    w, s = selector_weights(case)
    v, n = case.v, case.tokens
    num_w, den_w = w.clone(), w.clone()
    if variant == 'padding_key':
        den_w = torch.cat([den_w, torch.ones_like(den_w[..., :1])], dim=-1)
    elif variant == 'boundary_key_dropped':
        key = 64 if n > 64 else 32 if n > 32 else 0
        num_w[..., key] = 0
        den_w[..., key] = 0
    elif variant == 'last_key_not_in_row_sum':
        den_w[..., n - 1] = 0
    elif variant == 'rescale_skipped':
        m = s[..., :HS].amax(dim=-1, keepdim=True)
        first_on = (w > 0).double().argmax(dim=-1, keepdim=True)
        early = torch.arange(n) < (first_on // HS) * HS                        # keys of the half steps before the first on key's
        stale = ((s == m) & early & (m < 0)).double()
        num_w, den_w = num_w + stale, den_w + stale
    elif variant == 'v_rows_swapped':
        v = v.clone()
        v[:, :, [n - 2, n - 1]] = v[:, :, [n - 1, n - 2]]
    else:
        assert variant is None
    return fd.merge((num_w @ v) / den_w.sum(dim=-1, keepdim=True))


SELECTOR_VARIANTS = ('padding_key', 'boundary_key_dropped', 'last_key_not_in_row_sum', 'rescale_skipped', 'v_rows_swapped')

TOKENS = (1, 31, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 320, 577, 1025)
_BH = ((1, 2), (2, 3), (1, 6))
# every token count with one (batch, heads), in turn; 65 and 257 with all three; one 4097-token case
SELECTOR_CASES = sorted({(*_BH[i % 3], t) for i, t in enumerate(TOKENS)} | {(b, h, t) for (b, h) in _BH for t in (65, 257)}
                        | {(1, 2, 4097)}, key=lambda x: (x[2], x[0], x[1]))


# ---------------------------------------------------------------------------------------------- (A2) graded cases
JUMP, LIFT = 192.0, 188.0            # exact in both 16-bit types; 2^(JUMP - 3 - 3) is past float32: every lane sum it enters is inf
GRADED_CASES = [(1, 129, 3), (2, 333, 2), (1, 577, 2)]          # (batch, tokens, heads): a middle tile and a ragged last tile


@functools.lru_cache(maxsize=None)
def graded_case(batch, tokens, heads):
    """fp8_data.exact_case with a jump that takes the 16-bit overflow branch.  Key rows are 0 / 1 on dims 0..60, query rows
    have three ones there (scores 0..3), v is an integer in -7..7; slice b / head h then carry q * 2^a, k * 2^-a, v * 2^c.
    Dims 61..63 are set aside: query rows i with i % 5 == 1 + g carry a one on dim 61 + g (i % 5 == 4: on all three), key
    fp8_data.jump_keys(tokens)[g] carries JUMP there and every other key from the start of its tile on LIFT.  For such a
    row the first lifted key is 2^185 or more above its M: the lane's sum is inf, the overflow branch runs with
    alpha = exp2(-185 or less) = 0 exactly; the rows that share its 32-row block but carry no one on that dim go through
    the same branch with alpha = 2^-(0..3)."""
    gen = torch.Generator().manual_seed(1000 * batch + 10 * tokens + heads)
    base = 61
    perm = torch.stack([torch.randperm(base, generator=gen) for _ in range(batch * heads)]).view(batch, heads, base)
    i = torch.arange(tokens)
    q = torch.zeros(batch, heads, tokens, 64, dtype=torch.float64)
    k = torch.zeros_like(q)
    for j in range(3):
        q.scatter_(3, perm[:, :, (3 * i + j) % base].unsqueeze(-1), 1.0)
    k[..., :base] = (torch.rand(batch, heads, tokens, base, generator=gen) < 0.3).double()
    k.scatter_(3, perm.flip(-1)[:, :, i % base].unsqueeze(-1), 1.0)
    v = torch.randint(-7, 8, (batch, heads, tokens, 64), generator=gen).double()
    for grp, key in enumerate(fd.jump_keys(tokens)):
        q[:, :, (i % 5 == 1 + grp) | (i % 5 == 4), 61 + grp] = 1.0
        k[:, :, key // KT * KT:, 61 + grp] = LIFT
        k[:, :, key, 61 + grp] = JUMP
    qs, ks, vs = fd.apply_uneven(q, k, v)
    a, c = fd.uneven_exponents(batch, heads)
    return SimpleNamespace(batch=batch, tokens=tokens, heads=heads, q=q, k=k, v=v, a=a, c=c, qkv=fd.to_qkv(qs, ks, vs),
                           scores=q @ k.transpose(-2, -1))


def pp64_model(case, dt, skip_rescale=False, row_sum_skips_last_key=False):
    """attn_pp64_kernel's lazy-maximum policy on integer scores, restated in fp64 (exact here: every quantity is a dyadic
    number of few bits).  Query rows are padded with copies of the last row to a multiple of 64, as the kernel's clamped
    loads do for an active wave.  Per 32-key half step hs and 32-row block:
      hs == 0: M = the row's maximum over the (valid) keys; p = 2^(s - M).
      later:   p = 2^(s - M); if for ANY row of the block a lane half's sum of p (16 keys) exceeds P_LIMIT[dt]: every row
               of the block takes delta = max(max_j s_j - M, 0), M += delta, o and l *= alpha = exp2(-delta) evaluated in
               float32 (0 for delta > 149), p = 2^(s - M).
      o += p . v, l += sum p.
    The exactness condition, checked at every step and returned as .ok (.why names the first violation):
      (P)     every p that is accumulated is 2^e with -14 <= e <= 13: a normal fp16 number, and a bf16 number;
      (alpha) every delta is at most 126 (alpha a normal float32 power of two) or above 173 (alpha = 0, and not a
              denormal whose treatment depends on the mode);
      (sums)  with e_min the smallest exponent among the terms a row still holds, l < 2^(24 + e_min) and, with |v| in
              place of v, every o < 2^(24 + e_min): all partial sums, in any order, are integers below 2^24 in units of
              2^e_min -- exact in float32.  (v here is the integer v: its factor 2^c shifts nothing.)
    -> .o (batch, heads, tokens, 64) with the factor 2^c, .l (batch, heads, tokens), .rescales: executions of the overflow
       branch (block, half step), .ok, .why."""
    s, v, T = case.scores, case.v, case.tokens
    B, H = case.batch, case.heads
    R = (T + 63) // 64 * 64
    rows = torch.arange(R).clamp(max=T - 1)
    s = s[:, :, rows]
    half = torch.tensor([fd.lane_half(kin) for kin in range(HS)])
    o = s.new_zeros(B, H, R, 64)
    oa = s.new_zeros(B, H, R, 64)
    l = s.new_zeros(B, H, R)
    emin = s.new_full((B, H, R), float('inf'))
    M = None
    ok, why, rescales = True, '', 0
    nhs = (T + HS - 1) // HS
    for hs in range(nhs):
        lo, hi = HS * hs, min(HS * hs + HS, T)
        st = torch.cat([s[..., lo:hi], s.new_full((B, H, R, HS - (hi - lo)), -float('inf'))], dim=-1)
        vt = torch.cat([v[:, :, lo:hi], v.new_zeros(B, H, HS - (hi - lo), 64)], dim=2)
        tmax = st.amax(dim=-1)
        if hs == 0:
            M = tmax.clone()
        else:
            p = torch.exp2(st - M[..., None])
            over = torch.maximum(p[..., half == 0].sum(-1), p[..., half == 1].sum(-1)) > P_LIMIT[dt]
            trig = over.view(B, H, R // 32, 32).any(dim=-1)
            rescales += int(trig.sum())
            trig = trig.repeat_interleave(32, dim=-1)
            delta = torch.where(trig, (tmax - M).clamp(min=0), torch.zeros_like(M))
            if bool(((delta > 126) & (delta <= 173)).any()):
                ok, why = False, why or f'half step {hs}: an alpha that is a float32 denormal'
            alpha = torch.where(delta > 149, torch.zeros_like(delta), torch.exp2(-delta))
            M = M + delta
            if not skip_rescale:
                o, oa, l = o * alpha[..., None], oa * alpha[..., None], l * alpha
                emin = torch.where(alpha == 0, torch.full_like(emin, float('inf')), emin - delta)
        e = st - M[..., None]
        p = torch.exp2(e)
        valid = torch.isfinite(e)
        if bool(((e < -14) | (e > 13))[valid].any()):
            ok, why = False, why or f'half step {hs}: a P outside 2^-14 .. 2^13'
        o = o + p @ vt
        oa = oa + p @ vt.abs()
        skip = row_sum_skips_last_key and hi == T
        l = l + (p[..., :hi - lo - 1].sum(-1) if skip else p.sum(-1))
        emin = torch.minimum(emin, torch.where(valid, e, torch.full_like(e, float('inf'))).amin(dim=-1))
        if bool((torch.maximum(oa.amax(dim=-1), l) >= torch.exp2(24 + emin)).any()):
            ok, why = False, why or f'half step {hs}: a sum that needs more than 24 bits'
    o = o * (2.0 ** case.c.double())[..., None, None]
    return SimpleNamespace(o=o[:, :, :T], l=l[:, :, :T], rescales=rescales, ok=ok, why=why)


def graded_ok(case, dt):
    """The data condition of (A2) -- see pp64_model."""
    m = pp64_model(case, dt)
    return m.ok, m.why


def graded_expected(model, dt):
    """-> (RN16(RN32(o * RN32(1 / l))) computed in float32 on the CPU, o / l in fp64), both (batch * tokens, heads * 64).
    o and l are exact float32 numbers; numpy's float32 division and product are correctly rounded.  The result does not
    depend on which M the kernel ended with: another M scales o and l by the same power of two."""
    o32, l32 = model.o.numpy().astype(np.float32), model.l.numpy().astype(np.float32)
    assert (o32.astype(np.float64) == model.o.numpy()).all() and (l32.astype(np.float64) == model.l.numpy()).all()
    inv = np.float32(1.0) / l32
    out32 = o32 * inv[..., None]
    assert out32.dtype == np.float32
    want = rn16(torch.from_numpy(out32), dt)
    return fd.merge(want), fd.merge(model.o / model.l[..., None])


def graded_bound(want64, dt):
    """|got - o / l| <= 1.01 EPS |o / l|: RN32(1 / l) and the float32 product are each within 2^-24, the rounding to 16 bits
    within EPS -- (1 + 2^-24)^2 (1 + EPS) - 1 < 1.01 EPS.  Below fp16's smallest normal number, 2^-14, the rounding error is
    not relative any more: half a subnormal step, 2^-25."""
    b = 1.01 * EPS[dt] * want64.abs()
    return torch.where(want64.abs() < 2.0 ** -14, b.clamp(min=2.0 ** -25), b) if dt == 'fp16' else b


def sums_three_ways(w, v):
    """sum_j w_j v_j and sum_j w_j -- in fp64, and in float32 with the keys taken first to last and last to first, one
    addition at a time.  w (..., rows, keys), v (..., keys, 64).  -> [(o, l)] * 3 as fp64 tensors."""
    out = [(w @ v, w.sum(-1))]
    w32, v32 = w.float(), v.float()
    assert torch.equal(w32.double(), w) and torch.equal(v32.double(), v)
    for order in (range(w.shape[-1]), reversed(range(w.shape[-1]))):
        o = torch.zeros(*w.shape[:-1], 64, dtype=torch.float32)
        l = torch.zeros(w.shape[:-1], dtype=torch.float32)
        for j in order:
            o = o + w32[..., j, None] * v32[..., j, :].unsqueeze(-2)
            l = l + w32[..., j]
        out.append((o.double(), l.double()))
    return out


# ---------------------------------------------------------------------------------------------- (A3) real-valued inputs
def real_input(batch, tokens, heads, dt, pre):
    """test_gpu_kernels.py::test_attention_small's input: the 16-bit qkv the kernel is given."""
    g = torch.Generator().manual_seed(batch * 1000 + tokens)
    qkv = torch.randn(batch * tokens, 3 * heads * 64, generator=g)
    qkv[:, :2 * heads * 64] *= 1.6
    return fd.prescale16(qkv, heads, TDT[dt]) if pre else qkv.to(TDT[dt])


REAL_CASES = [(1, 1, 2), (2, 17, 2), (1, 33, 2), (1, 64, 2), (3, 65, 2), (1, 128, 6), (2, 129, 2),
              (1, 192, 2), (1, 200, 6), (2, 257, 2), (1, 320, 2), (2, 577, 2), (1, 1025, 2)]          # test_attention_small's


def real_bound(qkv, batch, tokens, heads, dt, pre):
    """-> (ref, bound), both (batch * tokens, heads * 64) fp64: softmax attention of the 16-bit inputs in fp64, and a bound
    on |kernel output - ref| per element.  With kappa = 1 for pre-scaled q (scores in exp2 units) and log2(e) / 8
    otherwise, p_j the exact weights scaled so that their maximum is 1, l = sum_j p_j, ref = sum_j p_j v_j / l,
    A = sum_j p_j |v_j| / l, T_j = sum_d |q_d k_jd|, N = tokens, u = 2^-24:

      bound = 1.01 [ EPS |ref|                                    the output's rounding to 16 bits
                   + EPS A                                        P rounded to 16 bits before P . V (the row sum takes the unrounded p)
                   + sum_j p_j eta_j (|v_j| + |ref|) / l          the weights' own error, eta_j below
                   + u ((3 N / 32 + 16) A + (N / 32 + 13) |ref|)  float32 sums, 1 / l and o * (1 / l)
                   + (fp16) 2^-25 (1 + sum_{j: p_j < 2^-14} |v_j| / l) ]      fp16's subnormal range

    * weights: the kernel evaluates exp2(arg_j) with arg_j = kappa (s_j - M) up to rounding.  s_j is a float32 sum of 64
      exact products (each within 64 u T_j whatever the order; pp64 starts the sum at -M: 65 u (T_j + |M|)); kappa s_j - RN(kappa M)
      in one FMA, alpha = exp2(kappa (M_old - M_new)) and pp64's -M - delta add at most 3 u kappa |M| between keys met
      under different maxima; kappa itself is a float32 constant: u kappa |s_j - M|; |M| <= T_max = max_j T_j.
      So |d arg_j| <= u kappa (66 T_j + 6 T_max), and with v_exp_f32's
      1 ulp: eta_j = ln 2 |d arg_j| + 2 u.  A weight error eta_j moves sum p v / sum p by at most p_j eta_j |v_j - ref| / l.
    * sums: a term of the row sum passes through at most 8 (its chain in the half step) + 1 + N / 32 (the running sum, one
      addition per half step) + 1 (the two lane halves) additions, and at most N / 32 rescale products: relative error
      u (2 N / 32 + 10) <= u (N / 32 + 10) + u N / 32.  A term of o passes through at most 16 + N / 16 additions (one MFMA
      adds 16 products to the accumulator; taken as 16 roundings) and N / 32 rescale products.  1 / l: within 2 u (the
      compiled division), the product with o: u.  The row-sum terms multiply |ref|, the o terms A.
    * fp16: a P below 2^-14 in the kernel's scale is rounded on the subnormal grid, error at most 2^-25 in that scale;
      the kernel's maximum is never above the true one, so its scale is at least the one of p_j (maximum 1) and
      only keys with p_j < 2^-14 can be subnormal.  An output below 2^-14: again 2^-25.
    * 1.01 covers the products of two of these terms: (1 + 2^-8)^2 < 1.01."""
    q, k, v = fd.split(qkv, batch, tokens, heads)
    kappa = 1.0 if pre else float(QSCALE32)
    # the reference takes the softmax scale exactly: 1 / 8 in natural units, ln 2 per exp2 unit for pre-scaled q
    s_ref = (q @ k.transpose(-2, -1)) * (np.log(2.0) if pre else 0.125)
    p = torch.exp(s_ref - s_ref.amax(dim=-1, keepdim=True))
    l = p.sum(dim=-1, keepdim=True)
    ref = (p @ v) / l
    A = (p @ v.abs()) / l
    T = q.abs() @ k.abs().transpose(-2, -1)
    eta = np.log(2.0) * U32 * kappa * (66.0 * T + 6.0 * T.amax(dim=-1, keepdim=True)) + 2 * U32
    pe = p * eta
    weights = (pe @ v.abs() + pe.sum(dim=-1, keepdim=True) * ref.abs()) / l
    n = tokens
    bound = EPS[dt] * ref.abs() + EPS[dt] * A + weights + U32 * ((3 * n / 32 + 16) * A + (n / 32 + 13) * ref.abs())
    if dt == 'fp16':
        bound = bound + 2.0 ** -25 * (1 + ((p < 2.0 ** -14).double() @ v.abs()) / l)
    return fd.merge(ref), fd.merge(1.01 * bound)


# ---------------------------------------------------------------------------------------------- the old bounds, for the record
def old_bounds_pass(got, ref, v, dt):
    """test_attention_small's global bounds: rel_fro <= 3 EPS and max_abs <= 6 EPS max|v|."""
    rel = float((got - ref).norm() / ref.norm())
    return rel <= 3 * EPS[dt] and float((got - ref).abs().max()) <= 6 * EPS[dt] * float(v.abs().max())
