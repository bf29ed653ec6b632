"""CPU: DINOv3 ViT-S/16, B/16, L/16 -- the test model, the rotary table, the loaders, the CLI surface, the fixtures.

* tests/dinov3_ref.py against transformers.DINOv3ViTModel (an independent implementation, built from a config
  object: no download), through vt.weights.dinov3_from_hf: the residual stream behind the last block (before the final norm)
  and the hooked q / k / v of the last block (before the rotation), at square and non-square inputs.
* vt.weights.rope_table equals the transformers class's table (first 32 columns), bit for bit.
* Loading: the Hugging Face layout and Meta's layout of the same weights give the same engine tensors; the k bias is zeroed;
  checkpoints of the wrong family are refused; a .pth and a .safetensors file in the Hugging Face layout load.
* infer.py's --dino3-model path; the plus / 7B models exit 1 naming the reason; two model flags exit 1.
* tests/golden/dinov3_*.npz are what tests/golden/make_golden_dinov3.py makes.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import dinov3_ref as r3
from helpers import load_golden, rel_fro

V3_NAMES = ('dinov3_vits16', 'dinov3_vitb16', 'dinov3_vitl16')


def _perturbed_v3(arch, seed):
    """Synthetic DINOv3 weights (Meta's layout) with random biases and gammas, so that every term of the block counts."""
    sd = vt.synthetic_state_dict(arch, seed, dinov3=True)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('.bias'):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith('.gamma'):
            sd[k] = 0.05 + torch.rand(sd[k].shape, generator=g)
    return sd


def _to_hf(sd, depth, prefix='model.'):
    """The canonical layout (zero k bias) as the transformers class names it: dinov3_from_hf inverted."""
    dim = sd['cls_token'].shape[-1]
    hf = {'embeddings.cls_token': sd['cls_token'], 'embeddings.mask_token': torch.zeros(1, 1, dim),
          'embeddings.register_tokens': sd['register_tokens'],
          'embeddings.patch_embeddings.weight': sd['patch_embed.proj.weight'],
          'embeddings.patch_embeddings.bias': sd['patch_embed.proj.bias'],
          'norm.weight': sd['norm.weight'], 'norm.bias': sd['norm.bias']}
    for i in range(depth):
        a, b = f'{prefix}layer.{i}.', f'blocks.{i}.'
        w, bias = sd[b + 'attn.qkv.weight'], sd[b + 'attn.qkv.bias']
        for j, name in enumerate(('q_proj', 'k_proj', 'v_proj')):
            hf[a + f'attention.{name}.weight'] = w[j * dim:(j + 1) * dim]
            if name != 'k_proj':
                hf[a + f'attention.{name}.bias'] = bias[j * dim:(j + 1) * dim]
        for theirs, ours in (('attention.o_proj', 'attn.proj'), ('norm1', 'norm1'), ('norm2', 'norm2'),
                             ('mlp.up_proj', 'mlp.fc1'), ('mlp.down_proj', 'mlp.fc2')):
            for p in ('weight', 'bias'):
                hf[a + f'{theirs}.{p}'] = sd[b + f'{ours}.{p}']
        hf[a + 'layer_scale1.lambda1'] = sd[b + 'ls1.gamma']
        hf[a + 'layer_scale2.lambda1'] = sd[b + 'ls2.gamma']
    return hf


def _hf_model(arch, registers=4):
    transformers = pytest.importorskip('transformers')
    dim, depth, heads, patch = arch
    cfg = transformers.DINOv3ViTConfig(
        hidden_size=dim, intermediate_size=4 * dim, num_hidden_layers=depth, num_attention_heads=heads, hidden_act='gelu',
        layer_norm_eps=1e-5, rope_theta=100.0, image_size=224, patch_size=patch, num_channels=3, query_bias=True,
        key_bias=False, value_bias=True, proj_bias=True, mlp_bias=True, layerscale_value=1.0, use_gated_mlp=False,
        num_register_tokens=registers, attention_dropout=0.0, drop_path_rate=0.0)
    return transformers.DINOv3ViTModel(cfg).eval()


def _hf_prefix(model):
    return 'model.' if any(k.startswith('model.layer.') for k in model.state_dict()) else ''


# ---------------------------------------------------------------------------- 1. the helper against transformers
@pytest.mark.parametrize('size', [(4, 4), (6, 5), (3, 7)])                   # a square and two non-square token grids
@pytest.mark.parametrize('arch', [(128, 3, 2, 16), (384, 2, 6, 16)])
def test_dinov3_ref_matches_transformers(arch, size):
    dim, depth, heads, patch = arch
    meta = _perturbed_v3(arch, 5)
    ours = r3.build_dinov3(arch, meta)
    hf = _hf_model(arch)
    hf.load_state_dict(_to_hf(vt.weights.dinov3_canonical(meta), depth, _hf_prefix(hf)), strict=True)
    # and back: the class's own state dict through dinov3_from_hf is the canonical dict
    back = vt.weights.dinov3_from_hf(hf.state_dict())
    canon = vt.weights.dinov3_canonical(meta)
    assert sorted(back) == sorted(canon)
    for k in canon:
        assert torch.equal(back[k], canon[k]), k
    x = torch.randn(2, 3, size[0] * patch, size[1] * patch, generator=torch.Generator().manual_seed(9))
    seen = {}
    last = (hf.model.layer if hasattr(hf, 'model') else hf.layer)[-1]
    hooks = [hf.norm.register_forward_pre_hook(lambda m, a: seen.__setitem__('stream', a[0]))]
    for name in ('q_proj', 'k_proj', 'v_proj'):
        hooks.append(getattr(last.attention, name).register_forward_hook(
            lambda m, a, out, name=name: seen.__setitem__(name, out)))
    with torch.no_grad():
        hf(pixel_values=x)
        stream = ours.tokens_before_block(x, depth)
        qkv = ours.last_block_qkv(x)
    for h in hooks:
        h.remove()
    assert stream.shape == seen['stream'].shape == (2, 5 + size[0] * size[1], dim)
    e_stream = float((seen['stream'] - stream).abs().max()) / float(stream.abs().max())
    hf_qkv = torch.cat([seen['q_proj'], seen['k_proj'], seen['v_proj']], dim=-1)
    e_qkv = float((hf_qkv - qkv).abs().max()) / float(qkv.abs().max())
    print(f'{arch} {size}: stream {e_stream:.2e}, hooked qkv {e_qkv:.2e}')
    assert e_stream <= 2e-5 and e_qkv <= 2e-5


@pytest.mark.parametrize('arch', [(128, 3, 2, 16), (384, 2, 6, 16)])
def test_rotation_and_key_bias_mask_are_live(arch):
    """A skipped rotation (cos = 1, sin = 0) and a forgotten bias mask each move the patch tokens' K by more than 1e-2."""
    meta = _perturbed_v3(arch, 5)
    model = r3.build_dinov3(arch, meta)
    x = torch.randn(2, 3, 6 * 16, 5 * 16, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        k = model.last_block_qkv(x)[:, 5:, arch[0]:2 * arch[0]]
        model.identity_rope = True
        k_id = model.last_block_qkv(x)[:, 5:, arch[0]:2 * arch[0]]
        model.identity_rope = False
        unmasked = {kk: v for kk, v in meta.items()}
        unmasked['register_tokens'] = unmasked.pop('storage_tokens')
        plain = r3.VisionTransformer(4, arch[3], arch[0], arch[1], arch[2])
        plain.load_state_dict({kk: v for kk, v in unmasked.items() if kk != 'mask_token' and not kk.startswith('rope_embed.')
                               and not kk.endswith('.bias_mask')}, strict=True)
        k_unmasked = plain.eval().last_block_qkv(x)[:, 5:, arch[0]:2 * arch[0]]
    assert rel_fro(k_id, k) > 1e-2 and rel_fro(k_unmasked, k) > 1e-2


# ---------------------------------------------------------------------------- 2. the rotary table
@pytest.mark.parametrize('grid', [(4, 4), (64, 64), (14, 14), (1, 3), (6, 5), (3, 7), (64, 1), (37, 20)])
def test_rope_table_is_the_transformers_table(grid):
    hf = _hf_model((128, 1, 2, 16))
    x = torch.zeros(1, 3, grid[0] * 16, grid[1] * 16)
    with torch.no_grad():
        cos_hf, sin_hf = hf.rope_embeddings(x)
    cos, sin = vt.weights.rope_table(*grid)
    assert cos.shape == sin.shape == (grid[0] * grid[1], 32) and cos.dtype == torch.float32
    assert cos_hf.shape == (grid[0] * grid[1], 64)
    for got, want in ((cos, cos_hf), (sin, sin_hf)):
        assert torch.equal(got.view(torch.int32), want[:, :32].contiguous().view(torch.int32))
        assert torch.equal(want[:, 32:], want[:, :32])              # only 32 distinct angles per token
    ref_cos, ref_sin = r3.rope_cos_sin(*grid)                       # the test model's own restatement
    assert torch.equal(ref_cos, cos_hf) and torch.equal(ref_sin, sin_hf)


# ---------------------------------------------------------------------------- 3. tables and loading
def test_arch_tables_v3():
    w = vt.weights
    assert w.DINOV3_ARCHS == V3_NAMES and w.DINOV3_REGISTER_TOKENS == 4
    assert vt.ARCHS['dinov3_vits16'] == (384, 12, 6, 16) and vt.ARCHS['dinov3_vitb16'] == (768, 12, 12, 16)
    assert vt.ARCHS['dinov3_vitl16'] == (1024, 24, 16, 16)
    assert all(len(v) == 4 for v in vt.ARCHS.values())
    assert vt.ARCHS['vits16'] == (384, 12, 6, 16)                    # DINO's own vits16 keeps its name
    for name in V3_NAMES:
        assert name not in w.HUB_FILES and vt.find_local_checkpoint(name) in (None, os.environ.get('VITTF_WEIGHTS'))
    for bad in ('dinov3_vits16plus', 'dinov3_vith16plus', 'dinov3_vit7b16'):
        assert bad not in vt.ARCHS


@pytest.mark.parametrize('seed', [0, 3])
def test_synthetic_v3_recipe(seed):
    w = vt.weights
    sd = vt.synthetic_state_dict('dinov3_vits16', seed)
    dino = vt.synthetic_state_dict('vits16', seed)
    v2 = vt.synthetic_state_dict('vits14_reg', seed)
    assert 'pos_embed' not in sd and 'register_tokens' not in sd and sd['storage_tokens'].shape == (1, 4, 384)
    for k in dino:                                                   # the DINO tensors of the seed, without pos_embed
        if k != 'pos_embed':
            assert torch.equal(sd[k], dino[k]), k
    assert torch.equal(sd['blocks.3.ls1.gamma'], v2['blocks.3.ls1.gamma'])
    assert torch.equal(sd['storage_tokens'], v2['register_tokens'])
    d = 384
    for i in range(12):
        assert float(sd[f'blocks.{i}.attn.qkv.bias'][d:2 * d].abs().min()) > 0          # NOT zero in the file
        assert torch.equal(sd[f'blocks.{i}.attn.qkv.bias_mask'], torch.cat([torch.ones(d), torch.zeros(d), torch.ones(d)]))
    canon = w.dinov3_canonical(sd)
    assert 'storage_tokens' not in canon and torch.equal(canon['register_tokens'], sd['storage_tokens'])
    assert not any(k == 'mask_token' or k.startswith('rope_embed.') or k.endswith('.bias_mask') for k in canon)
    for i in range(12):
        b, b0 = canon[f'blocks.{i}.attn.qkv.bias'], sd[f'blocks.{i}.attn.qkv.bias']
        assert bool((b[d:2 * d] == 0).all()) and torch.equal(b[:d], b0[:d]) and torch.equal(b[2 * d:], b0[2 * d:])
    assert float(sd['blocks.0.attn.qkv.bias'][d:2 * d].abs().min()) > 0                 # the input was not modified
    assert w.dinov3_canonical(canon).keys() == canon.keys()                              # idempotent
    # a tuple arch takes the flag; without it the old recipe is untouched
    assert 'pos_embed' in vt.synthetic_state_dict((128, 2, 2, 16), seed)
    assert 'pos_embed' not in vt.synthetic_state_dict((128, 2, 2, 16), seed, dinov3=True)


def test_wrong_family_is_refused():
    w = vt.weights
    v3 = vt.synthetic_state_dict('dinov3_vits16', 1)
    v2 = vt.synthetic_state_dict('vits14_reg', 1)
    dino = vt.synthetic_state_dict('vits16', 1)
    assert w.is_dinov3('dinov3_vits16', v3) is True and w.is_dinov3('vits14_reg', v2) is False
    assert w.is_dinov3('vits16', dino) is False
    assert w.is_dinov3((384, 12, 6, 16), v3) is True and w.is_dinov3((384, 12, 6, 16), dino) is False
    with pytest.raises(ValueError):
        w.is_dinov3('dinov3_vits16', v2)                             # a DINOv2 dict under a v3 name
    with pytest.raises(ValueError):
        w.is_dinov3('dinov3_vits16', dino)
    with pytest.raises(ValueError):
        w.is_dinov3('vits14_reg', v3)                                # a v3 dict under a v2 name
    with pytest.raises(ValueError):
        w.is_dinov3('vits16', v3)
    canon = w.dinov3_canonical(v3)
    assert w.register_tokens_of('dinov3_vits16', canon) == 4
    with pytest.raises(ValueError):                                  # a v3 dict without its registers
        w.register_tokens_of('dinov3_vits16', {k: v for k, v in canon.items() if k != 'register_tokens'})


def test_hf_and_meta_layout_give_the_same_engine_tensors(tmp_path):
    arch = (128, 2, 2, 16)
    meta = _perturbed_v3(arch, 6)
    canon = vt.weights.dinov3_canonical(meta)
    files = {}
    torch.save({'teacher': {'backbone.' + k: v for k, v in meta.items()}}, tmp_path / 'meta.pth')
    files['meta'] = vt.load_state_dict_file(str(tmp_path / 'meta.pth'))
    assert sorted(files['meta']) == sorted(meta)                     # Meta's layout passes the file loader as it is
    for prefix in ('model.', ''):
        torch.save(_to_hf(canon, arch[1], prefix), tmp_path / f'hf{len(prefix)}.pth')
        files['hf' + prefix] = vt.load_state_dict_file(str(tmp_path / f'hf{len(prefix)}.pth'))
    st = pytest.importorskip('safetensors.torch')
    st.save_file({k: v.contiguous() for k, v in _to_hf(canon, arch[1]).items()}, str(tmp_path / 'hf.safetensors'))
    files['safetensors'] = vt.load_state_dict_file(str(tmp_path / 'hf.safetensors'))
    want = vt.fold_layer_scale(canon)
    for name, sd in files.items():
        assert vt.weights.is_dinov3(arch, sd), name
        got = vt.fold_layer_scale(vt.weights.dinov3_canonical(sd))
        assert sorted(got) == sorted(want), name
        for k in want:
            assert torch.equal(got[k], want[k]), (name, k)
        r3.build_dinov3(arch, sd)                                    # strict
    with pytest.raises(ValueError):
        vt.weights.dinov3_from_hf(dict(_to_hf(canon, arch[1]), **{'model.layer.0.mlp.gate_proj.weight': torch.zeros(1)}))


# ---------------------------------------------------------------------------- 4. CLI surface
class _Args:
    dino_model = None
    dino2_model = None
    dino3_model = None


@pytest.mark.parametrize('name', ['vits16', 'vitb16', 'vitl16'])
def test_load_model_v3(name, tmp_path):
    import infer
    a = _Args(); a.dino3_model = name
    assert infer.load_model(a) == (f'dinov3_{name}', infer.get_dinov3_model, 16)
    assert a.model == f'dinov3_{name}'
    a.data_path = str(tmp_path / 'vol.npy'); a.cache_path = None; a.slice_along = 'all'; a.feature_output_size = 64
    a.overwrite = False
    assert infer.handle_output_path(a) == tmp_path / f'vol_dinov3_{name}_all_features64.npy'
    # DINO's vits16 keeps its own file name
    b = _Args(); b.dino_model = 'vits16'
    assert infer.load_model(b)[0] == 'vits16'


@pytest.mark.parametrize('name,word', [('vits16plus', 'SwiGLU'), ('vith16plus', '1280'), ('vit7b16', '4096')])
def test_cli_refuses_unsupported_v3(name, word, tmp_path, capsys):
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((4, 4, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        infer.get_dinov3_model(name)
    assert e.value.code == 1
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), '--dino3-model', name, '--synthetic-weights', '0'])
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert word in out and f'dinov3_{name}' in out


@pytest.mark.parametrize('flags', [('--dino-model', 'vits16', '--dino3-model', 'vits16'),
                                   ('--dino2-model', 'vits14', '--dino3-model', 'vitb16'),
                                   ('--dino-model', 'vits8', '--dino2-model', 'vits14', '--dino3-model', 'vitl16')])
def test_cli_two_model_flags_exit_1(flags, tmp_path, capsys):
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((4, 4, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), *flags, '--synthetic-weights', '0'])
    assert e.value.code == 1
    assert 'Please only set one of them' in capsys.readouterr().out


def test_cli_reaches_the_model_with_the_v3_layout(tmp_path, monkeypatch):
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((4, 4, 4), np.float32))
    seen = {}

    class Reached(Exception):
        pass

    class FakeHipViT:
        def __init__(self, state_dict, arch, **kw):
            seen['sd'], seen['arch'] = state_dict, arch
            raise Reached
    monkeypatch.setattr(infer.vt, 'HipViT', FakeHipViT)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    with pytest.raises(Reached):
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), '--dino3-model', 'vitb16', '--synthetic-weights', '0'])
    assert seen['arch'] == 'dinov3_vitb16' and seen['sd']['storage_tokens'].shape == (1, 4, 768)
    assert 'pos_embed' not in seen['sd']
    # a Hugging Face file through --weights
    arch = (128, 2, 2, 16)
    canon = vt.weights.dinov3_canonical(vt.synthetic_state_dict(arch, 2, dinov3=True))
    torch.save(_to_hf(canon, 2), tmp_path / 'hf.pth')
    monkeypatch.setitem(infer._MODEL_OPTS, 'weights', str(tmp_path / 'hf.pth'))
    with pytest.raises(Reached):
        infer.get_dinov3_model('vits16')
    assert seen['arch'] == 'dinov3_vits16' and torch.equal(seen['sd']['register_tokens'], canon['register_tokens'])


# ---------------------------------------------------------------------------- 5. fixtures
def _load_maker():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    try:
        import make_golden_dinov3 as maker
    finally:
        sys.path.pop(0)
    return maker


@pytest.mark.parametrize('name', ['dinov3_d128', 'dinov3_d384'])
def test_v3_fixtures_regenerate(golden_dir, name):
    maker = _load_maker()
    path = os.path.join(golden_dir, name + '.npz')
    assert os.path.getsize(path) <= 347170                       # tests/golden/dinov2_d384.npz
    rec = load_golden(golden_dir, name + '.npz')
    arch, seed, shape, fos, vol_seed = maker.CASES[name]
    assert tuple(int(v) for v in rec['arch']) == arch and int(rec['registers']) == 4 and int(rec['seed']) == seed
    sd = r3.synthetic_v3(arch, seed)
    assert math.isclose(vt.weights.state_dict_checksum(sd), float(rec['weights_checksum']), rel_tol=1e-12), 'generator drift'
    new = maker.case(arch, seed, shape, fos, vol_seed)
    assert sorted(new) == sorted(rec)
    assert np.array_equal(new['vol'], rec['vol']) and np.array_equal(new['im_sz'], rec['im_sz'])
    rows = 0
    for ax in 'zyx':
        for key in 'qkv':
            got, ref = torch.from_numpy(new[f'{key}_{ax}']), torch.from_numpy(rec[f'{key}_{ax}'])
            assert got.shape == ref.shape and got.dtype == torch.float16
            # fp32 on another CPU may round a value to the neighbouring fp16: the bound the other DINOv2 fixtures use
            assert float((got.float() - ref.float()).abs().max()) <= 2e-3 * float(ref.float().abs().max()), (ax, key)
            assert rel_fro(got, ref) < 1e-3, (ax, key)
        rows = max(rows, rec[f'k_{ax}'].shape[0] * (rec[f'k_{ax}'].shape[1] + 5))
    assert rows > 128                                            # one axis is more than one 128-row tile in a single call
