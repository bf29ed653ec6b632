"""GPU: the two 16-bit attention kernels behind vittf_attention -- attn_kernel (q_prescaled = 0, attention.hip) and
attn_pp64_kernel (q_prescaled = 1, attention_pp64.hip), the one the engine runs -- on inputs whose result is known bit for bit.

(A1) selector cases, both kernels: every weight is exactly 0 or 1, the output is the mean of a known set of v rows rounded
     once; compared equal.
(A2) graded cases, attn_pp64_kernel: integer scores, the overflow branch taken (vittf_attention_rescale_count), o and l
     exact; compared equal to RN16(RN32(o * RN32(1 / l))) and held to 1.01 EPS of fp64.
(A3) test_attention_small's real-valued inputs, both kernels: a derived bound per element.

Data, references, conditions and the bound's derivation: tests/attn_data.py; tests/test_attn_data_cpu.py
shows that the data has the properties named there and that subtly wrong kernels would fail.  Every output carries guard
rows of 7.0 behind it."""
import pytest
import torch

from vit_tf_amd import _lib
import attn_data as ad

pytestmark = pytest.mark.gpu

GUARD, GUARD_ROWS = 7.0, 2
KERNELS = {'plain': 0, 'pingpong': 1}                     # -> the q_prescaled flag of vittf_attention, which selects the kernel


def _attention(gpu, qkv16, batch, tokens, heads, dt, pre):
    """vittf_attention on a 16-bit qkv (host) -> the output as float64 values (batch * tokens, heads * 64)."""
    lib = _lib.load()
    qd = qkv16.to(gpu)
    out = torch.full((batch * tokens + GUARD_ROWS, heads * 64), GUARD, dtype=ad.TDT[dt], device=gpu)
    _lib.check(lib.vittf_attention(_lib.ptr(qd), _lib.ptr(out), batch, tokens, heads, _lib.DTYPES[dt], pre, _lib.stream_ptr()),
               'vittf_attention')
    torch.cuda.synchronize()
    got = out.float().cpu().double()
    assert bool((got[batch * tokens:] == GUARD).all()), 'wrote past the last row'
    return got[:batch * tokens]


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,heads,tokens', ad.SELECTOR_CASES)
def test_attention_selector_cases_bit_exact(gpu, batch, heads, tokens, dt, kernel):
    c = ad.selector_case(batch, tokens, heads)
    got = _attention(gpu, c.qkv.to(ad.TDT[dt]), batch, tokens, heads, dt, KERNELS[kernel])
    want = ad.rn16(c.want, dt)
    diff = ad.first_difference(got, want, batch, tokens, heads)
    if diff is not None:                                   # name the on set of the first wrong row
        row, col = (int(x) for x in ((got != want) | torch.isnan(got)).nonzero()[0])
        name, keys = c.groups[int(c.group_of[row // tokens, col // 64, row % tokens])]
        diff += f' (on set "{name}": keys {keys[:4]}{"..." if len(keys) > 4 else ""})'
    assert diff is None, diff


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads', ad.GRADED_CASES)
def test_attention_graded_cases_bit_exact(gpu, batch, tokens, heads, dt):
    lib = _lib.load()
    c = ad.graded_case(batch, tokens, heads)
    model = ad.pp64_model(c, dt)
    assert model.ok, model.why
    want, want64 = ad.graded_expected(model, dt)
    lib.vittf_attention_rescale_count(1)
    got = _attention(gpu, c.qkv.to(ad.TDT[dt]), batch, tokens, heads, dt, 1)
    count = int(lib.vittf_attention_rescale_count(1))
    print(f'graded {batch} x {tokens} x {heads} {dt}: overflow branch ran {count} times, the model says {model.rescales}')
    assert count > 0, 'the overflow branch did not run'
    assert count == model.rescales, 'the overflow branch ran another number of times than the stated policy says'
    ratio = (got - want64).abs() / ad.graded_bound(want64, dt).clamp(min=1e-300)
    diff = ad.first_difference(got, want, batch, tokens, heads)
    print(f'    worst error / (1.01 EPS |fp64|) {float(ratio.max()):.3f}; against the float32 restatement: {diff or "equal"}')
    assert float(ratio.max()) <= 1.0, 'beyond 1.01 EPS of fp64'
    assert diff is None, diff


@pytest.mark.parametrize('kernel', list(KERNELS))
@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
@pytest.mark.parametrize('batch,tokens,heads', ad.REAL_CASES)
def test_attention_real_inputs_per_element(gpu, batch, tokens, heads, dt, kernel):
    """test_attention_small's inputs against attn_data.real_bound (its docstring derives it)."""
    pre = KERNELS[kernel]
    qkv = ad.real_input(batch, tokens, heads, dt, pre)
    ref, bound = ad.real_bound(qkv, batch, tokens, heads, dt, pre)
    got = _attention(gpu, qkv, batch, tokens, heads, dt, pre)
    ratio = (got - ref).abs() / bound
    worst = int(ratio.argmax())
    row, col = worst // ratio.shape[1], worst % ratio.shape[1]
    print(f'attention {kernel} {dt} {batch} x {tokens} x {heads}: worst error / bound {float(ratio.max()):.3f} at slice {row // tokens} '
          f'token {row % tokens} head {col // 64} dim {col % 64}')
    assert bool(torch.isfinite(got).all())
    assert float(ratio.max()) <= 1.0
