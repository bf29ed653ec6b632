"""Host-only data, references and stated conditions for the exact tests of the fused block tail (vittf_block_tail,
csrc/tail_fx.hip) and of the three launches it replaces (vittf_gemm_residual_ln with gemm_rows.hip's epilogue LayerNorm,
vittf_gemm with EPI_BIAS_GELU, vittf_layernorm): torch on the CPU, no GPU, no library call.  The references are products of
small integers in fp64, exact in any order (the largest case, 38477 rows, takes a second or two).

The block tail computes
    x' = x0 + a . Wp^T + bp ;  hn = RN16(LayerNorm(x'; g2, e2)) ;  hid = RN16(gelu(hn . W1^T + b1)) ;  x = x' + hid . W2^T + b2
and h_out = RN16(LayerNorm(x; g1, e1)).  tail_case makes inputs for which every rounding on the way to x is decided with a
wide margin, so x is known bit for bit:

  * a in -2..2, Wp sparse in -2..2, bp in -4..4: P = a . Wp^T + bp is a small integer, exact in any order.
  * x0 = mu_r + sigma_r z_r - P with z_r a balanced +-1 pattern (192 of each; another one per row), sigma_r an integer in
    1..8 and mu_r = an integer in -20..20 plus, on odd rows, k / 32 with 1 <= |k| <= 15: x' = mu_r + sigma_r z_r.  The row
    sum is 384 mu_r, the centred squares sum to 384 sigma_r^2: mean and variance are exact in float32 in any order (all
    partial sums are integers below 2^24 in units of 1 / 32).  The fraction makes x' a number that bf16 cannot hold
    (fp16 still can: 5 + 5 bits), so a residual stream rounded to bf16 on the way shows.
  * norm2 then gives z (1 - delta) g2 + e2 with 0 <= delta < 2e-6 (the 1e-6 under the root and float32 rounding).  (g2, e2)
    per column is (1, 3) or (2, 4): z g2 + e2 is 2, 4 or 6 -- never 0, which would come out as a tiny non-zero number, and
    2^-8 or more away from the nearest point where a 16-bit rounding changes: hn = z g2 + e2 exactly.
  * W1 in {0, 4}, about 8 per row and at least one; b1 in {0, 8, 16}: the pre-activation u is a multiple of 8, at least 8
    and far below 2048: exact in bf16, and gelu_poly(u) = u in float32 (u times 0.5 erfc(u / sqrt 2) < 5e-15 for u >= 8):
    hid = u.
  * W2 dense in -2..2, b2 in -4..4: x = x' + u . W2^T + b2, every partial sum a multiple of 1 / 32 below 2^24 / 32.
  * g1, e1 are real-valued: h_out is held to the one-rounding bound (h_bound) against fp64 LayerNorm of the exact x."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TDT = {'bf16': torch.bfloat16, 'fp16': torch.float16}
EPS = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
D, HID = 384, 1536
LN_EPS = 1e-6
ROWS = (1, 33, 127, 128, 129, 130, 4097, 128 * 300 + 77)     # the last: more row tiles than persistent workgroups
CPU_ROWS = tuple(r for r in ROWS if r <= 4097)


def balanced(rows, d, gen):
    """(rows, d) of +-1, d / 2 of each per row, another pattern per row."""
    z = torch.rand(rows, d, generator=gen).argsort(dim=1) < d // 2
    return z.double() * 2.0 - 1.0


def _row_stats(rows, gen):
    mu = torch.randint(-20, 21, (rows, 1), generator=gen).double()
    k = torch.randint(1, 16, (rows, 1), generator=gen).double() * (2.0 * torch.randint(0, 2, (rows, 1), generator=gen).double() - 1.0)
    mu = mu + torch.where(torch.arange(rows).view(rows, 1) % 2 == 1, k / 32.0, torch.zeros_like(k))
    sg = torch.randint(1, 9, (rows, 1), generator=gen).double()
    return mu, sg


def _norm_pairs(d, gen):
    sel = torch.randint(0, 2, (d,), generator=gen)
    return torch.where(sel == 1, 2.0, 1.0).double(), torch.where(sel == 1, 4.0, 3.0).double()


@functools.lru_cache(maxsize=4)
def tail_case(rows):
    """-> float64 tensors on the CPU: .a (rows, 384), .wp (384, 384), .bp, .x0 (rows, 384), .g2 .e2, .w1 (1536, 384), .b1,
    .w2 (384, 1536), .b2, .g1 .e1, and the exact intermediate and final values .xp (x'), .hn, .u (= hid), .x;
    .z .mu .sg the row patterns and statistics."""
    gen = torch.Generator().manual_seed(4000 + rows)
    d = D
    a = torch.randint(-2, 3, (rows, d), generator=gen).double()
    wp = torch.randint(-2, 3, (d, d), generator=gen).double() * (torch.rand(d, d, generator=gen) < 0.1)
    bp = torch.randint(-4, 5, (d,), generator=gen).double()
    mu, sg = _row_stats(rows, gen)
    z = balanced(rows, d, gen)
    g2, e2 = _norm_pairs(d, gen)
    w1 = 4.0 * (torch.rand(HID, d, generator=gen) < 8.0 / d).double()
    w1[torch.arange(HID), torch.arange(HID) % d] = 4.0
    b1 = 8.0 * torch.randint(0, 3, (HID,), generator=gen).double()
    w2 = torch.randint(-2, 3, (d, HID), generator=gen).double()
    b2 = torch.randint(-4, 5, (d,), generator=gen).double()
    g1 = (1.0 + 0.2 * torch.randn(d, generator=gen)).float().double()
    e1 = (0.1 * torch.randn(d, generator=gen)).float().double()
    mm = lambda p, q: p @ q.t()
    xp = mu + sg * z
    x0 = xp - (mm(a, wp) + bp)
    hn = z * g2 + e2
    u = mm(hn, w1) + b1
    x = xp + mm(u, w2) + b2
    worst = float((mm(u.abs(), w2.abs()) + xp.abs() + b2.abs()).max())
    assert worst * 32 < 2 ** 24, f'partial sums of x may need more than 24 bits: {worst}'
    return SimpleNamespace(rows=rows, a=a, wp=wp, bp=bp, x0=x0, g2=g2, e2=e2, w1=w1, b1=b1, w2=w2, b2=b2, g1=g1, e1=e1,
                           xp=xp, hn=hn, u=u, x=x, z=z, mu=mu, sg=sg)


@functools.lru_cache(maxsize=None)
def wide_case(rows=257, n=768, k=768):
    """x += a . w^T + bias and h = LayerNorm(x) for gemm_rows.hip's 768-column form, with balanced patterns of its own:
    x0 = mu_r + sigma_r z_r - P -> .x (the exact sum) and .h = z g + e (exact, 2, 4 or 6)."""
    gen = torch.Generator().manual_seed(7680 + rows)
    a = torch.randint(-2, 3, (rows, k), generator=gen).double()
    w = torch.randint(-2, 3, (n, k), generator=gen).double() * (torch.rand(n, k, generator=gen) < 0.05)
    bias = torch.randint(-4, 5, (n,), generator=gen).double()
    mu, sg = _row_stats(rows, gen)
    z = balanced(rows, n, gen)
    g, e = _norm_pairs(n, gen)
    x = mu + sg * z
    return SimpleNamespace(rows=rows, n=n, k=k, a=a, w=w, bias=bias, x0=x - (a @ w.t() + bias), g=g, e=e, x=x, h=z * g + e,
                           z=z, mu=mu, sg=sg)


def layernorm64(x, g, e):
    return F.layer_norm(x, (x.shape[-1],), g, e, LN_EPS)


def h_bound(want, dt):
    """The LayerNorm kernels' existing bound (test_layernorm, _residual_ln_case): float32 statistics and ONE rounding to the
    16-bit type -- 1.01 EPS |want|, the 1.01 for the float32 part, + 2e-5 absolute for the statistics' error where |want| is
    small.  Per element."""
    return EPS[dt] * want.abs() * 1.01 + 2e-5


def exact16(x):
    x = torch.as_tensor(x)
    return all(torch.equal(x.float().to(t).double(), x.double()) for t in TDT.values())


# ---------------------------------------------------------------------------------------------- models
def norm2_f32(xp, g2, e2, dt):
    """norm2 as the kernels evaluate it, in float32 on the CPU: mean, centred variance, 1 / sqrt(var + eps), one rounding."""
    x = xp.float()
    d = x.shape[1]
    mean = x.sum(1, keepdim=True) / d
    dv = x - mean
    var = (dv * dv).sum(1, keepdim=True) / d
    rstd = 1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))
    return (dv * rstd * g2.float() + e2.float()).to(TDT[dt]).float(), mean, var


def gelu_poly_f32(u):
    """vittf_common.h::gelu_poly in float32."""
    u = u.float()
    ax = u.abs()
    p = torch.tensor(-0.000524238159) * ax + 0.00741911121
    p = p * ax - 0.0526018888
    p = p * ax - 0.459225923
    p = p * ax - 1.15109742
    return torch.clamp(u, min=0) - ax * torch.exp2(p * ax - 1.0)


def chain_f32(c, dt):
    """The whole chain in float32 with the 16-bit roundings of the kernel -> x (float32)."""
    x1 = c.x0.float() + (c.a.float() @ c.wp.float().t() + c.bp.float())
    hn, _, _ = norm2_f32(x1.double(), c.g2, c.e2, dt)
    hid = gelu_poly_f32(hn @ c.w1.float().t() + c.b1.float()).to(TDT[dt]).float()
    return x1 + hid @ c.w2.float().t() + c.b2.float(), x1, hn, hid


def tail_model(inp, dt, variant=None):
    """fp64 model of the block tail on any inputs (an object with a, wp, bp, x0, g2, e2, w1, b1, w2, b2 in float64; exact
    erf GELU), with one deliberate error -> x.
    'rows_exchanged': rows 5 and 6 of norm2's output change places at the hand-over to fc1.
    'k_step_dropped': output columns 32..63 miss the hidden units 16..31 (one k step of fc2 for one column tile).
    'b2_wrong_block': b2 is applied 32 columns further on.
    'x_prime_rounded': x' is rounded to the 16-bit type before fc2 accumulates on top of it."""
    x1 = inp.x0 + inp.a @ inp.wp.t() + inp.bp
    hn = layernorm64(x1, inp.g2, inp.e2).to(torch.float32).to(TDT[dt]).double()
    if variant == 'rows_exchanged':
        hn[[5, 6]] = hn[[6, 5]]
    hid = F.gelu(hn @ inp.w1.t() + inp.b1).to(torch.float32).to(TDT[dt]).double()
    b2 = inp.b2.roll(32) if variant == 'b2_wrong_block' else inp.b2
    base = x1.to(torch.float32).to(TDT[dt]).double() if variant == 'x_prime_rounded' else x1
    x = base + hid @ inp.w2.t() + b2
    if variant == 'k_step_dropped':
        x[:, 32:64] -= hid[:, 16:32] @ inp.w2[32:64, 16:32].t()
    assert variant in (None, 'rows_exchanged', 'k_step_dropped', 'b2_wrong_block', 'x_prime_rounded')
    return x


TAIL_VARIANTS = ('rows_exchanged', 'k_step_dropped', 'b2_wrong_block', 'x_prime_rounded')


def gaussian_inputs(rows, dt):
    """test_gpu_kernels.py::test_block_tail's inputs (16-bit a and weights, fp32 vectors and residual), as float64."""
    d = D
    g = torch.Generator().manual_seed(rows + 5)
    t = TDT[dt]
    a = torch.randn(rows, d, generator=g).to(t)
    wp = (torch.randn(d, d, generator=g) / d ** 0.5).to(t)
    bp = 0.3 * torch.randn(d, generator=g)
    w1 = (torch.randn(4 * d, d, generator=g) / d ** 0.5).to(t)
    b1 = 0.3 * torch.randn(4 * d, generator=g)
    w2 = (torch.randn(d, 4 * d, generator=g) / (4 * d) ** 0.5).to(t)
    b2 = 0.3 * torch.randn(d, generator=g)
    g2, e2 = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    _g1, _e1 = 1.0 + 0.2 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    x0 = (torch.randn(rows + 32, d, generator=g) * 3)[:rows]
    f = lambda v: v.double()
    return SimpleNamespace(a=f(a), wp=f(wp), bp=f(bp), x0=f(x0), g2=f(g2), e2=f(e2), w1=f(w1), b1=f(b1), w2=f(w2), b2=f(b2))


def old_per_element_passes(got, ref, dt):
    """test_block_tail's per-element allowance."""
    return bool(((got - ref).abs() <= 6 * EPS[dt] + 1e-4).all())
