"""CPU: the data of tests/test_gpu_attention_exact.py (tests/attn_data.py) has the properties its exactness arguments need,
and attention models with one deliberate error each fail the new checks -- while the most likely of them, a padding key
let through the ragged-tile mask, passes test_attention_small's global bounds on test_attention_small's data."""
import numpy as np
import pytest
import torch

import attn_data as ad
import fp8_data as fd

DTS = ('fp16', 'bf16')


def _exact16(x):
    x = torch.as_tensor(x)
    return all(torch.equal(x.float().to(ad.TDT[dt]).double(), x.double()) for dt in DTS)


# ---------------------------------------------------------------------------------------------- (A1)
def test_selector_cases_cover_the_token_counts_and_shapes():
    tokens = {t for _, _, t in ad.SELECTOR_CASES}
    assert tokens == set(ad.TOKENS) | {4097}
    assert {(b, h) for b, h, _ in ad.SELECTOR_CASES} == {(1, 2), (2, 3), (1, 6)}
    assert sum(t == 4097 for _, _, t in ad.SELECTOR_CASES) == 1


@pytest.mark.parametrize('tokens', ad.TOKENS + (4097,))
def test_selector_groups_are_placed_where_the_paths_change(tokens):
    groups = dict(ad.selector_groups(tokens))
    nt = (tokens + 63) // 64
    last0 = 64 * (nt - 1)
    sizes = {len(k) for k in groups.values()}
    assert all(s & (s - 1) == 0 and 1 <= s <= 64 for s in sizes)
    assert groups['key 0 only'] == [0] and groups['last key only'] == [tokens - 1]
    if tokens > 32:
        assert groups['pair 31|32'] == [31, 32] and groups['first on key after 32 off keys'][0] == 32
    if tokens > 64:
        assert groups['pair 63|64'] == [63, 64] and groups['first on key after 64 off keys'][0] == 64
    if tokens > 128:
        assert groups['first on key after 128 off keys'][0] == 128
        assert groups['last full tile | ragged tile'] == [last0 - 1, last0]
    ragged = groups['all in the ragged last tile']
    assert min(ragged) >= last0 and max(ragged) == tokens - 1
    if nt >= 2:
        spread = [k for name, k in groups.items() if name.startswith('spread')]
        assert {key // 64 for keys in spread for key in keys} == set(range(nt)), 'an on key in every tile'
    if tokens >= 128:
        assert {8, 16, 32, 64} <= sizes
    if tokens >= 577:
        assert sizes == {1, 2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize('batch,heads,tokens', ad.SELECTOR_CASES)
def test_selector_case_properties(batch, heads, tokens):
    c = ad.selector_case(batch, tokens, heads)
    assert _exact16(c.qkv), 'operands exact in fp16 and bf16'
    G = len(c.groups)
    # query rows: one or three ones; every group met in every full 32-row block
    ones = (c.q == 1).sum(-1)
    assert bool(((c.q == 0) | (c.q == 1)).all()) and set(ones.unique().tolist()) <= {1, 3}
    if tokens >= 32:
        assert all(len(c.group_of[0, 0, r:r + 32].unique()) == G for r in range(0, tokens - 31, 32)) or G > 32
    assert bool(((c.k == 0) | (c.k == ad.OFF)).all())
    # scores, one group's query at a time (no N x N matrix): 0 exactly on the on set, a multiple of -4096 elsewhere
    levels = set()
    for b in range(batch):
        for h in range(heads):
            qg = torch.stack([c.q[b, h, int((c.group_of[b, h] == g).nonzero()[0])] if bool((c.group_of[b, h] == g).any())
                              else torch.full((64,), float('nan'), dtype=torch.float64) for g in range(G)])
            present = ~torch.isnan(qg[:, 0])
            s = qg[present] @ c.k[b, h].t()
            assert torch.equal(s == 0, c.on[b, h][present]), 'the on sets are the zero scores'
            assert bool((s % ad.OFF == 0).all()) and float(s.min()) >= 3 * ad.OFF
            levels |= set(s.unique().tolist())
            assert bool(c.on[b, h][present].any(dim=-1).all()), 'every query has an on key'
    if tokens >= 65:
        assert levels == {0.0, ad.OFF, 2 * ad.OFF, 3 * ad.OFF}, 'off at three levels'
    # -4096 c is far below float32's exp2 range, in attn_kernel's units too
    assert float(ad.QSCALE32) * ad.OFF < -160 and ad.OFF < -160
    # v: multiples of 1/16 up to 8 before the (slice, head) factor, neighbouring keys differ on every dim's row, sums < 2^24
    _, cexp = fd.uneven_exponents(batch, heads)
    n = c.v * 16.0 / (2.0 ** cexp.double())[..., None, None]
    assert bool((n == n.round()).all()) and float(n.abs().max()) <= 128
    if tokens > 1:
        assert bool((c.v[:, :, 1:] != c.v[:, :, :-1]).any(dim=-1).all()), 'neighbouring v rows differ'
    assert 64 * 128 < 2 ** 24
    assert len({tuple(x.tolist()) for x in cexp.flatten().view(-1, 1)}) > 1 or batch * heads == 1
    # the expected output needs more bits than the 16-bit types have: the final rounding is exercised
    # (a set of 8 keys for bf16, of 32 for fp16: 16 and 64 tokens at the least)
    for dt, least in (('bf16', 16), ('fp16', 64)):
        assert bool((ad.rn16(c.want, dt) != c.want).any()) or tokens < least
    # per-(slice, head) dim permutations differ
    qrows = c.q[:, :, 0].reshape(batch * heads, 64)
    assert len({tuple(r.tolist()) for r in qrows}) > 1


@pytest.mark.parametrize('batch,heads,tokens', [x for x in ad.SELECTOR_CASES if x[2] <= 1025])
def test_selector_reference_and_wrong_variants(batch, heads, tokens):
    """The O(N * 64) reference is the score-matrix model; float32 sums in two orders are the fp64 sums; each wrong variant
    changes at least one rounded output element, in both types."""
    c = ad.selector_case(batch, tokens, heads)
    assert torch.equal(ad.selector_model(c), c.want)
    w, _ = ad.selector_weights(c)
    if tokens <= 257:
        (o64, l64), fwd, bwd = ad.sums_three_ways(w, c.v)
        assert torch.equal(fwd[0], o64) and torch.equal(bwd[0], o64) and torch.equal(fwd[1], l64) and torch.equal(bwd[1], l64)
        l32 = l64.float()
        assert bool((torch.log2(l64) % 1 == 0).all()), 'row sums are powers of two'
        assert torch.equal(((o64.float() * (1.0 / l32)[..., None]).double()), o64 / l64[..., None]), 'o * (1 / l) is exact in float32'
        assert torch.equal((o64.float() / l32[..., None]).double(), o64 / l64[..., None]), 'and so is o / l'
    for var in ad.SELECTOR_VARIANTS:
        applies = {'rescale_skipped': tokens > 32, 'v_rows_swapped': tokens >= 2}.get(var, True)
        bad = ad.selector_model(c, var)
        for dt in DTS:
            seen = ad.first_difference(ad.rn16(bad, dt), ad.rn16(c.want, dt), batch, tokens, heads) is not None
            assert seen == applies, (var, dt)


# ---------------------------------------------------------------------------------------------- (A2)
@pytest.mark.parametrize('batch,tokens,heads', ad.GRADED_CASES)
def test_graded_case_condition_and_wrong_variants(batch, tokens, heads):
    c = ad.graded_case(batch, tokens, heads)
    assert {t for _, t, _ in ad.GRADED_CASES} <= set(ad.TOKENS) | {333}
    assert _exact16(c.qkv)
    assert bool((c.scores == c.scores.round()).all()), 'integer scores in exp2 units'
    assert float(c.scores[..., :32].amax(-1).max()) <= 3, 'M of the first 32 keys is an ordinary score'
    for dt in DTS:
        ok, why = ad.graded_ok(c, dt)
        assert ok, why
        m = ad.pp64_model(c, dt)
        assert m.rescales > 0, 'the overflow branch is taken'
        # the jump rows' lane sums are past the limit by construction, not by a hair
        assert 2.0 ** (ad.LIFT - 3 - 3) > 1e30 * ad.P_LIMIT[dt]
        want, want64 = ad.graded_expected(m, dt)
        assert bool(((want - want64).abs() <= ad.graded_bound(want64, dt)).all()), 'the float32 restatement is within the fp64 bound'
        assert bool((want != want64).any()), 'the output rounding is exercised'
        for kw in ({'skip_rescale': True}, {'row_sum_skips_last_key': True}):
            mb = ad.pp64_model(c, dt, **kw)
            bad = ad.rn16(fd.merge(mb.o / mb.l[..., None]), dt)
            assert ad.first_difference(bad, want, batch, tokens, heads) is not None, kw
            assert not bool(((bad - want64).abs() <= ad.graded_bound(want64, dt)).all()), kw
    # graded rescales: some rows go through the branch with alpha = 1/2, 1/4 or 1/8 (they share a block with a jump row)
    # -- seen as a model without the rescale differing on rows that carry no one on a jump dim
    plain = (c.q[..., 61:].sum(-1) == 0)
    mb, m = ad.pp64_model(c, 'fp16', skip_rescale=True), ad.pp64_model(c, 'fp16')
    assert bool(((mb.l != m.l) & plain).any())


def test_graded_sums_do_not_depend_on_the_order():
    """o and l of the (A2) model, in the final M's units, against float32 sums first-to-last and last-to-first."""
    c = ad.graded_case(1, 129, 3)
    m = ad.pp64_model(c, 'fp16')
    # weights under the model's final M: l is their sum; rebuilt from the scores with what survived (o / l is M-free)
    s = c.scores
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    w = torch.where(w < 2.0 ** -100, torch.zeros_like(w), w)          # what alpha = 0 removed
    (o64, l64), fwd, bwd = ad.sums_three_ways(w, c.v)
    for o, l in (fwd, bwd):
        assert torch.equal(o, o64) and torch.equal(l, l64)
    ratio = m.l / l64
    assert bool((torch.log2(ratio) % 1 == 0).all()), 'the model holds the same sums at another power-of-two scale'
    assert torch.equal(m.o / (2.0 ** c.c.double())[..., None, None] / m.l[..., None], o64 / l64[..., None])


def test_pp64_model_pads_rows_like_the_kernel():
    """129 tokens: rows 129..191 of wave 2 are copies of row 128 -- block b of that wave is a block of its own."""
    c = ad.graded_case(1, 129, 3)
    m = ad.pp64_model(c, 'bf16')
    assert m.o.shape == (1, 3, 129, 64) and m.l.shape == (1, 3, 129)


# ---------------------------------------------------------------------------------------------- (A3) and the documented gap
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('batch,tokens,heads', [(3, 65, 2), (2, 257, 2), (1, 1025, 2)])
def test_padding_key_passes_the_old_bounds_and_real_bound_is_sane(dt, batch, tokens, heads):
    """A zero-filled key let through the mask (score 0, v 0) on test_attention_small's data: inside 3 EPS / 6 EPS max|v|.
    The per-element bound holds for the correctly rounded fp64 result with room to spare, and is a small multiple of the
    output's own rounding -- not a global allowance."""
    for pre in (0, 1):
        qkv = ad.real_input(batch, tokens, heads, dt, pre)
        q, k, v = fd.split(qkv, batch, tokens, heads)
        s = (q @ k.transpose(-2, -1)) * (np.log(2.0) if pre else 0.125)
        ref = fd.merge(s.softmax(-1) @ v)
        s2 = torch.cat([s, s.new_zeros(*s.shape[:-1], 1)], dim=-1)
        v2 = torch.cat([v, v.new_zeros(batch, heads, 1, 64)], dim=2)
        bad = ad.rn16(fd.merge(s2.softmax(-1) @ v2), dt)
        assert ad.old_bounds_pass(bad, ref, v, dt), 'the gap: the old bounds let a padding key through'
        ref2, bound = ad.real_bound(qkv, batch, tokens, heads, dt, pre)
        assert torch.allclose(ref2, ref, rtol=1e-12, atol=1e-14)
        good = ad.rn16(ref, dt)
        assert float(((good - ref).abs() / bound).max()) <= 0.55
        assert float((bound / (ad.EPS[dt] * ref.abs() + 1e-30)).median()) < 8
