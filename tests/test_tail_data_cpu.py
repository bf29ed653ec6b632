"""CPU: the data of tests/test_gpu_block_tail_exact.py (tests/tail_data.py) has the properties its exactness argument needs,
a float32 restatement of the whole chain reproduces the fp64 integers, and block-tail models with one deliberate error each
fail the equality check.

What the fp64 model says about test_block_tail's per-element allowance of 6 EPS + 1e-4 (0.023 in bf16, about twenty times the
arithmetic's own error) is recorded here too, as measured: on that test's Gaussian inputs the four errors of
tail_data.TAIL_VARIANTS all exceed it somewhere among 130 x 384 elements (the rounded residual stream by a factor of 1.3
only); what it lets through are errors of up to twenty roundings per element, and on the exact data there is no such thing
as a small error -- any wrong term moves an x by 1 / 32 or more."""
import pytest
import torch

import tail_data as td

DTS = ('fp16', 'bf16')


@pytest.mark.parametrize('rows', td.CPU_ROWS)
def test_tail_case_properties(rows):
    c = td.tail_case(rows)
    d = td.D
    for name in ('a', 'wp', 'w1', 'w2'):
        assert td.exact16(getattr(c, name)), name
    for name in ('bp', 'b1', 'b2', 'g2', 'e2', 'g1', 'e1', 'x0'):
        v = getattr(c, name)
        assert torch.equal(v.float().double(), v), name
    # small integers, sparse where stated
    assert float(c.a.abs().max()) <= 2 and float(c.wp.abs().max()) <= 2 and float(c.bp.abs().max()) <= 4
    assert 0.05 < float((c.wp != 0).double().mean()) < 0.12
    assert set(c.w1.unique().tolist()) == {0.0, 4.0} and set(c.b1.unique().tolist()) <= {0.0, 8.0, 16.0}
    nz = (c.w1 != 0).sum(1)
    assert int(nz.min()) >= 1 and 6 < float(nz.double().mean()) < 11
    assert float(c.w2.abs().max()) <= 2 and float((c.w2 != 0).double().mean()) > 0.7
    # row statistics: balance, integer sigma, mu an integer (even rows) or an integer + k / 32 (odd rows)
    assert bool((c.z.abs() == 1).all()) and bool((c.z.sum(1) == 0).all())
    if rows >= 33:
        assert len({tuple(r.tolist()) for r in c.z[:33]}) == 33, 'another pattern per row'
        assert len(c.mu.unique()) > 8 and set(c.sg.flatten().tolist()) == set(range(1, 9))
    assert bool((c.sg == c.sg.round()).all()) and 1 <= float(c.sg.min()) and float(c.sg.max()) <= 8
    assert bool((c.mu[0::2] == c.mu[0::2].round()).all()) and float(c.mu.abs().max()) < 21
    if rows > 1:
        assert bool((c.mu[1::2] != c.mu[1::2].round()).all()) and bool((c.mu * 32 == (c.mu * 32).round()).all())
        xp_bf16 = c.xp.float().to(torch.bfloat16).double()
        lost = (xp_bf16[1::2] != c.xp[1::2]).any(dim=1).double().mean()          # (|x'| < 8 still fits: 3 + 5 bits)
        assert float(lost) > (0.2 if rows >= 33 else -1), "bf16 cannot hold x' of a good part of the odd rows"
    assert torch.equal(c.xp.float().to(torch.float16).double(), c.xp), "fp16 can"
    assert torch.equal(c.x0 + c.a @ c.wp.t() + c.bp, c.xp)
    # mean and centred variance: exact sums, below 2^24 in units of 1 / 32 in any order
    assert torch.equal(c.xp.sum(1, keepdim=True), d * c.mu) and torch.equal(((c.xp - c.mu) ** 2).sum(1, keepdim=True), d * c.sg ** 2)
    assert float(c.xp.abs().sum(1).max()) * 32 < 2 ** 24 and float(d * c.sg.max() ** 2) < 2 ** 24
    assert float((c.a.abs() @ c.wp.abs().t() + c.bp.abs() + c.x0.abs()).max()) * 32 < 2 ** 24
    # norm2 in fp64 with the real eps: never zero, 2, 4 or 6 up to delta < 2e-6, far from any 16-bit rounding boundary
    hn64 = td.layernorm64(c.xp, c.g2, c.e2)
    assert set(c.hn.unique().tolist()) <= {2.0, 4.0, 6.0} and bool((c.hn != 0).all())
    assert float((hn64 - c.hn).abs().max()) < 2 * 2e-6
    # (the nearest point where a bf16 rounding changes is half a step below 2: 2^-8 away -- 900 times that distance from 2)
    assert 2.0 ** -8 > 900 * 4e-6
    # fc1: multiples of 8, at least 8, exact in bf16; the activation leaves them alone in float32
    assert bool((c.u % 8 == 0).all()) and float(c.u.min()) >= 8 and float(c.u.max()) < 2048 and td.exact16(c.u)
    assert torch.equal(td.gelu_poly_f32(c.u).double(), c.u)
    # fc2: partial sums below 2^24 in units of 1 / 32 whatever the order
    worst = float((c.u.abs() @ c.w2.abs().t() + c.xp.abs() + c.b2.abs()).max())
    assert worst * 32 < 2 ** 24, worst
    assert bool((c.x * 32 == (c.x * 32).round()).all()) and torch.equal(c.x.float().double(), c.x)
    assert torch.equal(c.x, c.xp + c.u @ c.w2.t() + c.b2)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('rows', [r for r in td.CPU_ROWS if r <= 130])
def test_float32_restatement_is_exact(rows, dt):
    c = td.tail_case(rows)
    x, x1, hn, hid = td.chain_f32(c, dt)
    assert torch.equal(x1.double(), c.xp) and torch.equal(hn.double(), c.hn) and torch.equal(hid.double(), c.u)
    assert torch.equal(x.double(), c.x)
    _, mean, var = td.norm2_f32(c.xp, c.g2, c.e2, dt)
    assert torch.equal(mean.double(), c.mu) and torch.equal(var.double(), c.sg ** 2)
    assert torch.equal(td.tail_model(c, dt), c.x), 'the fp64 model with the exact erf GELU agrees'


def test_wide_case_properties():
    w = td.wide_case()
    assert (w.n, w.k) == (768, 768) and w.rows % 128 not in (0,) and w.rows > 256
    assert td.exact16(w.a) and td.exact16(w.w) and torch.equal(w.x0.float().double(), w.x0)
    assert bool((w.z.sum(1) == 0).all()) and torch.equal(w.x0 + w.a @ w.w.t() + w.bias, w.x)
    assert set(w.h.unique().tolist()) <= {2.0, 4.0, 6.0}
    assert float((td.layernorm64(w.x, w.g, w.e) - w.h).abs().max()) < 4e-6
    for dt in DTS:
        hn, mean, var = td.norm2_f32(w.x, w.g, w.e, dt)
        assert torch.equal(hn.double(), w.h) and torch.equal(mean.double(), w.mu) and torch.equal(var.double(), w.sg ** 2)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('variant', td.TAIL_VARIANTS)
def test_wrong_variants_fail_the_equality_check(variant, dt):
    c = td.tail_case(130)
    bad = td.tail_model(c, dt, variant)
    seen = not torch.equal(bad, c.x)
    # x' of this data is a 10-bit number: fp16 holds it, so a residual stream rounded to fp16 is the one error that the
    # exact data cannot show in that type (bf16 shows it)
    assert seen == (not (variant == 'x_prime_rounded' and dt == 'fp16'))
    if seen:
        assert float((bad - c.x).abs().max()) >= 1.0 / 32
    # the old allowance on the old inputs, as the model measures it (see the module docstring)
    gi = td.gaussian_inputs(130, dt)
    ref, gbad = td.tail_model(gi, dt), td.tail_model(gi, dt, variant)
    ratio = float((gbad - ref).abs().max()) / (6 * td.EPS[dt] + 1e-4)
    print(f'{variant} {dt}: worst error on Gaussian inputs / (6 EPS + 1e-4) = {ratio:.2f}')
    assert td.old_per_element_passes(ref, ref, dt) and not td.old_per_element_passes(gbad, ref, dt)
    assert ratio < 1.5 if variant == 'x_prime_rounded' else ratio > 10
