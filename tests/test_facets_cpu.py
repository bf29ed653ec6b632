"""CPU: the token facet and the hooked-layer selection -- the C-ABI surface, the host package, the CLI, and what the GPU
tests' reference expression means.

* include/vittf.h declares vittf_vit_features / vittf_token_features and the library exports them; the new entry refuses
  part_mask 0 and 16 and the token bit without an output or a final norm (no launch: there is no GPU here); the ABI stays 6.
* PARTS['t'] == 3; resolve_layer: -1, 0, depth - 1, out of range.
* infer.py: --facet / --layer parse, handle_output_path keeps today's name for the defaults and suffixes the others,
  save_features round-trips a {'t': ...} dict; predict_ntf.pick_features takes a one-entry dict and still prefers 'k'.
* The reference expression of tests/test_gpu_facets.py, ``model.norm(model.tokens_before_block(x, l + 1))[:, 1 + R:]``, is
  transformers' ``last_hidden_state`` / ``layernorm(hidden_states[l + 1])`` for Dinov2Model and DINOv3ViTModel on the same
  synthetic weights (the state-dict mappings are the existing CPU tests'), at their fp32-vs-fp32 tolerance 2e-5.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
from vit_tf_amd import _lib
import dinov3_ref as r3
from dinov2_ref import build_dinov2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ---------------------------------------------------------------------------- 1. ABI surface
def _dummy_call(lib, mask, norm_g=1, norm_b=1, q=1, k=1, v=1, t=1, cfg=None):
    """vittf_vit_features with well-formed host structs and placeholder device addresses: only calls the argument checks
    refuse are made with it (nothing is launched, nothing is dereferenced on the device)."""
    addr = 0x1000                                            # never read: every call below returns from the checks
    cfg = cfg or _lib.VitConfig(384, 12, 6, 8, _lib.FP16, 1e-6, 0, 0)
    w = _lib.VitWeights(**{n: addr for n, _ in _lib.VitWeights._fields_})
    pos = _lib.PosEmbed(addr, addr)
    view = _lib.SliceView(addr, 64 * 64, 64, 1, 64, 64, 64, 64, addr)
    p = lambda on: C.c_void_p(addr) if on else None          # noqa: E731
    return lib.vittf_vit_features(C.byref(cfg), C.byref(w), C.byref(pos), C.byref(view), 0, 1, mask, None, 0, None, p(norm_g),
                                  p(norm_b), p(q), p(k), p(v), p(t), C.c_void_p(addr), 0, None)


def test_features_entry_is_declared_exported_and_validates():
    header = open(os.path.join(ROOT, 'include', 'vittf.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('vittf_vit_features', 'vittf_token_features'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), f'{name} is not declared in include/vittf.h'
        assert name in _lib.SIGNATURES
    assert '#define VITTF_ABI_VERSION 6' in header
    lib = _lib.load()
    assert hasattr(lib, 'vittf_vit_features') and hasattr(lib, 'vittf_token_features')
    assert lib.vittf_abi_version() == _lib.ABI_VERSION == 6
    # the older entries are still there: symbols were added only
    for name in ('vittf_vit_qkv_features_rope', 'vittf_vit_qkv_features_reg', 'vittf_vit_qkv_features', 'vittf_vit_k_features'):
        assert hasattr(lib, name)
    for mask in (0, 16, -1, 31):
        assert _dummy_call(lib, mask) == INVALID, mask
    for missing in ('t', 'norm_g', 'norm_b'):
        for mask in (8, 15):
            assert _dummy_call(lib, mask, **{missing: 0}) == INVALID, (mask, missing)
    for missing, bit in (('q', 1), ('k', 2), ('v', 4)):
        assert _dummy_call(lib, bit | 8, **{missing: 0}) == INVALID, missing
    # a call the checks above let through gets as far as the workspace check (0 bytes were passed): the masks 1 .. 15 are valid,
    # and a mask without bit 3 needs neither t_out nor the final norm
    WORKSPACE = -2
    for mask in range(1, 16):
        assert _dummy_call(lib, mask) == WORKSPACE, mask
    assert _dummy_call(lib, 7, norm_g=0, norm_b=0, t=0) == WORKSPACE
    # the older entry refuses the token bit (its masks stay 1 .. 7)
    cfg = _lib.VitConfig(384, 12, 6, 8, _lib.FP16, 1e-6, 0, 0)
    assert lib.vittf_vit_qkv_features_rope(C.byref(cfg), None, None, None, 0, 1, 8, None, 0, None, None, None, None, None, 0,
                                           None) == INVALID
    # the output kernel's own checks
    a = C.c_void_p(0x1000)
    assert lib.vittf_token_features(None, a, a, a, 1, 10, 1, 384, 1e-6, None) == INVALID
    assert lib.vittf_token_features(a, a, a, None, 1, 10, 1, 384, 1e-6, None) == INVALID
    assert lib.vittf_token_features(a, a, a, a, 1, 5, 5, 384, 1e-6, None) == INVALID        # no patch token behind the prefix
    assert lib.vittf_token_features(a, a, a, a, 1, 10, 0, 384, 1e-6, None) == INVALID       # prefix counts CLS
    assert lib.vittf_token_features(a, a, a, a, 1, 10, 1, 1028, 1e-6, None) == INVALID      # wider than a wave holds
    assert lib.vittf_token_features(a, a, a, a, 0, 10, 1, 384, 1e-6, None) == INVALID


# ---------------------------------------------------------------------------- 2. host package
def test_parts_and_layer_resolution():
    assert vt.extract.PARTS == {'q': 0, 'k': 1, 'v': 2, 't': 3}
    from vit_tf_amd.engine import resolve_layer
    for depth in (1, 3, 12, 24):
        assert resolve_layer(None, depth) == depth - 1
        assert resolve_layer(-1, depth) == depth - 1
        assert resolve_layer(0, depth) == 0
        assert resolve_layer(depth - 1, depth) == depth - 1
        assert resolve_layer(-depth, depth) == 0
        for bad in (depth, depth + 5, -depth - 1):
            with pytest.raises(ValueError):
                resolve_layer(bad, depth)
    assert resolve_layer(5, 12) == 5 and resolve_layer(-3, 12) == 9
    import inspect
    sig = inspect.signature(vt.HipViT.__init__)
    assert sig.parameters['layer'].default is None


# ---------------------------------------------------------------------------- 3. CLI
class _Args:
    cache_path = None
    slice_along = 'all'
    feature_output_size = 64
    overwrite = False


def _name(tmp_path, model, **kw):
    import infer
    a = _Args()
    a.data_path = str(tmp_path / 'vol.npy')
    a.model = model
    for k, v in kw.items():
        setattr(a, k, v)
    return infer.handle_output_path(a).name


def test_output_name_keeps_the_default_and_suffixes_the_rest(tmp_path):
    assert _name(tmp_path, 'vits8') == 'vol_vits8_all_features64.npy'                       # no facet / layer attribute at all
    assert _name(tmp_path, 'vits8', facet='key', layer=-1) == 'vol_vits8_all_features64.npy'
    assert _name(tmp_path, 'vits14_reg', facet='key', layer=-1) == 'vol_vits14_reg_all_features64.npy'
    assert _name(tmp_path, 'vits14_reg', facet='token', layer=-1) == 'vol_vits14_reg_all_features64_token.npy'
    assert _name(tmp_path, 'dinov3_vitl16', facet='token', layer=-1) == 'vol_dinov3_vitl16_all_features64_token.npy'
    assert _name(tmp_path, 'vits8', facet='query', layer=-1) == 'vol_vits8_all_features64_query.npy'
    assert _name(tmp_path, 'vits8', facet='key', layer=3) == 'vol_vits8_all_features64_L3.npy'
    assert _name(tmp_path, 'vits8', facet='key', layer=-2) == 'vol_vits8_all_features64_L10.npy'      # the resolved index
    assert _name(tmp_path, 'vitl14', facet='value', layer=-24) == 'vol_vitl14_all_features64_value_L0.npy'
    assert _name(tmp_path, 'vits8', facet='token', layer=5) == 'vol_vits8_all_features64_token_L5.npy'
    assert _name(tmp_path, 'vits8', facet='key', layer=11) == 'vol_vits8_all_features64.npy'          # the last block by its index
    with pytest.raises(ValueError):
        _name(tmp_path, 'vits8', facet='key', layer=12)
    # an explicit --cache-path is taken as it is
    assert _name(tmp_path, 'vits8', facet='token', layer=2, cache_path=str(tmp_path / 'mine.npy')) == 'mine.npy'


def test_cli_parses_facet_and_layer(tmp_path, monkeypatch, capsys):
    """main() up to the model constructor: the flags reach the output name and HipViT's `layer`; bad values exit."""
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((8, 8, 8), dtype=np.float16))
    seen = {}

    class Stop(Exception):
        pass

    def fake_hipvit(sd, name, **kw):
        seen.update(kw, name=name)
        raise Stop

    monkeypatch.setattr(vt, 'HipViT', fake_hipvit)
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.setattr(vt.extract, 'DIST_FORCE', False)
    base = ['--data-path', str(tmp_path / 'vol.npy'), '--synthetic-weights', '0', '--feature-output-size', '4']
    for extra, layer in ((['--dino2-model', 'vits14_reg', '--facet', 'token'], -1),
                         (['--dino3-model', 'vits16', '--facet', 'token', '--layer', '-3'], -3),
                         (['--facet', 'value', '--layer', '4'], 4), ([], -1)):
        seen.clear()
        with pytest.raises(Stop):
            infer.main(base + extra)
        assert seen['layer'] == layer, extra
    for bad in (['--facet', 'cls'], ['--layer', 'x'], ['--layer', '12'], ['--layer', '-13']):
        with pytest.raises(SystemExit) as e:
            infer.main(base + bad)
        assert e.value.code in (1, 2), bad
    assert 'Invalid argument for --layer' in capsys.readouterr().out
    assert infer.FACETS == {'key': 'k', 'query': 'q', 'value': 'v', 'token': 't'}
    # fp8 attention stays refused for DINOv3 whatever the facet, by the model itself (engine.HipViT): nothing to parse here


def test_save_features_and_predict_loader_take_the_token_key(tmp_path):
    import infer
    import predict_ntf
    t = torch.rand(6, 2, 3, 4).half()
    infer.save_features({'t': t}, tmp_path / 'f_features.npy')
    back = np.load(tmp_path / 'f_features.npy', allow_pickle=True)[()]
    assert list(back) == ['t'] and back['t'].dtype == np.float16 and np.array_equal(back['t'], t.numpy())
    infer.save_features({'t': t}, tmp_path / 'f_features.pt')
    assert torch.equal(torch.load(tmp_path / 'f_features.pt', weights_only=False)['t'], t)
    assert torch.equal(predict_ntf.pick_features(back), t)
    k = torch.rand(6, 2, 3, 4).half()
    assert torch.equal(predict_ntf.pick_features({'t': t.numpy(), 'k': k.numpy()}), k)            # 'k' is still preferred
    assert torch.equal(predict_ntf.pick_features({'k': k.numpy()}), k)
    assert torch.equal(predict_ntf.pick_features(k.numpy()), k)                                  # a bare array, as before
    with pytest.raises(ValueError):
        predict_ntf.pick_features({'q': k.numpy(), 't': t.numpy()})
    with pytest.raises(ValueError):
        predict_ntf.pick_features({})


# ---------------------------------------------------------------------------- 4. what the reference expression means
TOL = 2e-5          # the fp32-vs-fp32 tolerance of test_dinov2_ref_matches_transformers_dinov2 / test_dinov3_ref_matches_transformers


def _token_facet(model, x, layer, registers):
    return model.norm(model.tokens_before_block(x, layer + 1))[:, 1 + registers:]


def test_token_facet_expression_is_transformers_dinov2():
    from test_dinov2_cpu import _hf_from_dinov2, _perturbed_dinov2
    arch, grid = (128, 3, 2, 14), 4
    dim, depth, heads, patch = arch
    sd = _perturbed_dinov2(arch, 5, grid)
    ours = build_dinov2(arch, sd)
    hf = _hf_from_dinov2(sd, dim, depth, heads, patch, grid)
    x = torch.randn(2, 3, grid * patch, grid * patch, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        out = hf(pixel_values=x, output_hidden_states=True)
        want_last = out.last_hidden_state[:, 1:]
        got_last = _token_facet(ours, x, depth - 1, 0)
        assert float((got_last - want_last).abs().max()) <= TOL * float(want_last.abs().max())
        for layer in range(depth):
            want = hf.layernorm(out.hidden_states[layer + 1])[:, 1:]
            got = _token_facet(ours, x, layer, 0)
            assert got.shape == want.shape == (2, grid * grid, dim)
            assert float((got - want).abs().max()) <= TOL * float(want.abs().max()), layer
        # the final norm is live in the expression: without it the tokens are something else
        assert float((ours.tokens_before_block(x, depth)[:, 1:] - want_last).abs().max()) > 1e-2 * float(want_last.abs().max())


def test_token_facet_expression_is_transformers_dinov3():
    from test_dinov3_cpu import _hf_model, _hf_prefix, _perturbed_v3, _to_hf
    arch, size = (128, 3, 2, 16), (3, 5)
    dim, depth, heads, patch = arch
    meta = _perturbed_v3(arch, 5)
    ours = r3.build_dinov3(arch, meta)
    hf = _hf_model(arch)
    hf.load_state_dict(_to_hf(vt.weights.dinov3_canonical(meta), depth, _hf_prefix(hf)), strict=True)
    x = torch.randn(2, 3, size[0] * patch, size[1] * patch, generator=torch.Generator().manual_seed(9))
    layers = hf.model.layer if hasattr(hf, 'model') else hf.layer
    seen = {}
    hooks = [blk.register_forward_hook(lambda m, a, out, i=i: seen.__setitem__(i, out[0] if isinstance(out, tuple) else out))
             for i, blk in enumerate(layers)]
    with torch.no_grad():
        out = hf(pixel_values=x)
        for h in hooks:
            h.remove()
        want_last = out.last_hidden_state[:, 5:]
        got_last = _token_facet(ours, x, depth - 1, 4)
        assert got_last.shape == want_last.shape == (2, size[0] * size[1], dim)
        assert float((got_last - want_last).abs().max()) <= TOL * float(want_last.abs().max())
        for layer in range(depth):
            want = hf.norm(seen[layer])[:, 5:]
            got = _token_facet(ours, x, layer, 4)
            assert float((got - want).abs().max()) <= TOL * float(want.abs().max()), layer
