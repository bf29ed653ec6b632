"""CPU: the DINOv2 register models (vits14_reg / vitb14_reg / vitl14_reg) -- the test model, the position-embedding resize,
the weight tables and loaders, the CLI surface, the engine batch, the fixtures.

* tests/dinov2_reg_ref.py against transformers.Dinov2WithRegistersModel (an independent implementation in the image, built
  from a config object: no download) at the stored grid, a larger square and two non-square inputs; the registers are live.
* vt.interpolate_pos_embed's antialias form is the helper's, bit for bit, and is not the scale-factor form.
* ARCHS / REGISTER_TOKENS / HUB_FILES, the hub-cache lookup, strict loading of a checkpoint-layout state dict, refusal of a
  wrong register count; the synthetic recipe leaves every shared tensor of a seed alone.
* infer.py's --dino2-model path for the new names; vitg14_reg exits 1.
* ViT-L/14-reg at N = 4101: the engine batch stays within what the engine accepts.
* tests/golden/dinov2_reg_*.npz are what tests/golden/make_golden_dinov2_reg.py makes.
"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

import vit_tf_amd as vt
import dinov2_reg_ref as rr
from helpers import load_golden, rel_fro

REG_NAMES = ('vits14_reg', 'vitb14_reg', 'vitl14_reg')


def _perturbed_reg(arch, seed, grid, registers):
    """Synthetic register-model weights with random biases and gammas (every term of the block counts), registers of std 0.5."""
    sd = vt.synthetic_state_dict(arch, seed, stored_grid=grid, layer_scale=True)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('.bias'):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith('.gamma'):
            sd[k] = 0.05 + torch.rand(sd[k].shape, generator=g)
    sd['register_tokens'] = 0.5 * torch.randn(1, registers, arch[0], generator=g)
    return sd


def _hf_with_registers(sd, dim, depth, heads, patch, grid, registers):
    transformers = pytest.importorskip('transformers')
    cfg = transformers.Dinov2WithRegistersConfig(
        hidden_size=dim, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4, hidden_act='gelu',
        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=1e-6, image_size=grid * patch,
        patch_size=patch, num_channels=3, qkv_bias=True, layerscale_value=1.0, use_swiglu_ffn=False,
        num_register_tokens=registers)
    model = transformers.Dinov2WithRegistersModel(cfg).eval()
    hf = {'embeddings.cls_token': sd['cls_token'], 'embeddings.mask_token': sd['mask_token'],
          'embeddings.register_tokens': sd['register_tokens'], 'embeddings.position_embeddings': sd['pos_embed'],
          'embeddings.patch_embeddings.projection.weight': sd['patch_embed.proj.weight'],
          'embeddings.patch_embeddings.projection.bias': sd['patch_embed.proj.bias'],
          'layernorm.weight': sd['norm.weight'], 'layernorm.bias': sd['norm.bias']}
    for i in range(depth):
        pre = f'encoder.layer.{i}.'
        w, b = sd[f'blocks.{i}.attn.qkv.weight'], sd[f'blocks.{i}.attn.qkv.bias']
        for j, name in enumerate(('query', 'key', 'value')):
            hf[pre + f'attention.attention.{name}.weight'] = w[j * dim:(j + 1) * dim]
            hf[pre + f'attention.attention.{name}.bias'] = b[j * dim:(j + 1) * dim]
        for theirs, ours in (('attention.output.dense', 'attn.proj'), ('norm1', 'norm1'), ('norm2', 'norm2'),
                             ('mlp.fc1', 'mlp.fc1'), ('mlp.fc2', 'mlp.fc2')):
            for p in ('weight', 'bias'):
                hf[pre + f'{theirs}.{p}'] = sd[f'blocks.{i}.{ours}.{p}']
        hf[pre + 'layer_scale1.lambda1'] = sd[f'blocks.{i}.ls1.gamma']
        hf[pre + 'layer_scale2.lambda1'] = sd[f'blocks.{i}.ls2.gamma']
    model.load_state_dict(hf, strict=True)
    return model


# ---------------------------------------------------------------------------- 1. the helper against transformers
@pytest.mark.parametrize('size', [(4, 4), (7, 7), (6, 5), (3, 7)])         # the stored grid, a larger square, two non-square
@pytest.mark.parametrize('registers', [4, 1])
@pytest.mark.parametrize('arch', [(128, 3, 2, 14), (384, 2, 6, 14)])
def test_reg_ref_matches_transformers(arch, registers, size):
    dim, depth, heads, patch = arch
    grid = 4
    sd = _perturbed_reg(arch, 5, grid, registers)
    ours = rr.build_dinov2_reg(arch, sd)
    hf = _hf_with_registers(sd, dim, depth, heads, patch, grid, registers)
    x = torch.randn(2, 3, size[0] * patch, size[1] * patch, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        out = hf(pixel_values=x, output_hidden_states=True)
        stream = ours.tokens_before_block(x, depth - 1)
        k_ref = ours.last_block_k(x)
        last = hf.encoder.layer[-1]
        k_hf = last.attention.attention.key(last.norm1(out.hidden_states[depth - 1]))
    assert stream.shape == (2, 1 + registers + size[0] * size[1], dim)
    e_stream = float((out.hidden_states[depth - 1] - stream).abs().max()) / float(stream.abs().max())
    e_k = float((k_hf - k_ref).abs().max()) / float(k_ref.abs().max())
    print(f'{arch} R={registers} {size}: stream {e_stream:.2e}, k {e_k:.2e}')
    assert e_stream <= 2e-5 and e_k <= 2e-5
    # the K third of the hooked tensor is what last_block_k gives (a 3 D wide and a D wide fp32 product: not the same bits)
    with torch.no_grad():
        third = ours.last_block_qkv(x)[..., dim:2 * dim]
    assert float((third - k_ref).abs().max()) <= 1e-5 * float(k_ref.abs().max())


@pytest.mark.parametrize('registers', [4, 1])
@pytest.mark.parametrize('arch', [(128, 3, 2, 14), (384, 2, 6, 14)])
def test_registers_are_live(arch, registers):
    """Zeroing register_tokens moves the patch tokens' K by more than 1e-2 relative Frobenius."""
    sd = _perturbed_reg(arch, 5, 4, registers)
    model = rr.build_dinov2_reg(arch, sd)
    x = torch.randn(2, 3, 6 * 14, 5 * 14, generator=torch.Generator().manual_seed(9))
    zeroed = copy.deepcopy(model)
    zeroed.register_tokens.data.zero_()
    with torch.no_grad():
        k = model.last_block_k(x)[:, 1 + registers:]
        k0 = zeroed.last_block_k(x)[:, 1 + registers:]
    moved = rel_fro(k0, k)
    print(f'{arch} R={registers}: zeroed registers move K by {moved:.3e}')
    assert moved > 1e-2


# ---------------------------------------------------------------------------- 2. the position-embedding resize
@pytest.mark.parametrize('rows,cols', [(37 * 14, 37 * 14), (64 * 14, 64 * 14), (20 * 14, 20 * 14), (4 * 14, 4 * 14),
                                       (14, 42), (56, 28), (896, 14)])
def test_interpolate_pos_embed_register_form(rows, cols):
    pos = torch.randn(1, 1 + 37 * 37, 64, generator=torch.Generator().manual_seed(rows + cols))
    got = vt.interpolate_pos_embed(pos, rows, cols, 14, antialias=True)
    want = rr.interpolate_pos_embed_reg(pos, rows, cols, 14)
    assert got.shape == (1, 1 + (rows // 14) * (cols // 14), 64)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    plain = vt.interpolate_pos_embed(pos, rows, cols, 14)
    assert torch.equal(plain, vt.interpolate_pos_embed(pos, rows, cols, 14, antialias=False))
    if (rows, cols) == (37 * 14, 37 * 14):
        assert got is pos and plain is pos                   # the stored square grid at a square image: the identity
    else:
        # the two forms are far apart on a unit-variance embedding: no tolerance used anywhere hides a wrong one
        assert float((got - plain).abs().max()) > 0.1


def test_resize_form_follows_the_model():
    w = vt.weights
    plain = vt.synthetic_state_dict('vits14', 0)
    reg = vt.synthetic_state_dict('vits14_reg', 0)
    assert w.pos_embed_antialias_of('vits14', plain) is False and w.pos_embed_antialias_of('vits14_reg', reg) is True
    assert w.pos_embed_antialias_of((384, 12, 6, 14), reg) is True and w.pos_embed_antialias_of((384, 12, 6, 14), plain) is False
    assert w.pos_embed_antialias_of('vits8', vt.synthetic_state_dict('vits8', 0)) is False


# ---------------------------------------------------------------------------- 3. tables, hub cache, loading
def test_arch_tables():
    for name in REG_NAMES:
        assert vt.ARCHS[name] == vt.ARCHS[name[:-4]] and len(vt.ARCHS[name]) == 4
        assert vt.weights.REGISTER_TOKENS[name] == 4 and name in vt.weights.DINOV2_ARCHS
        assert vt.weights.HUB_FILES[name] == f'dinov2_{name[:-4]}_reg4_pretrain.pth'
    assert all(len(v) == 4 for v in vt.ARCHS.values())
    assert set(vt.weights.REGISTER_TOKENS) == set(REG_NAMES)
    assert 'vitg14' not in vt.ARCHS and 'vitg14_reg' not in vt.ARCHS


def test_find_local_checkpoint_reg(tmp_path, monkeypatch):
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    ck = tmp_path / 'hub' / 'checkpoints'
    ck.mkdir(parents=True)
    (ck / 'dinov2_vitb14_pretrain.pth').write_bytes(b'')
    assert vt.find_local_checkpoint('vitb14_reg') is None        # the plain checkpoint is not the register one
    (ck / 'dinov2_vitb14_reg4_pretrain.pth').write_bytes(b'')
    assert vt.find_local_checkpoint('vitb14_reg') == str(ck / 'dinov2_vitb14_reg4_pretrain.pth')
    assert vt.find_local_checkpoint('vitl14_reg') is None


def test_reg_checkpoint_layout_loads_strictly(tmp_path, monkeypatch):
    import infer
    arch = (128, 2, 2, 14)
    sd = rr.synthetic_reg(arch, 6)
    path = tmp_path / 'dinov2_reg.pth'
    torch.save({'teacher': {'backbone.' + k: v for k, v in sd.items()}}, path)
    loaded = vt.load_state_dict_file(str(path))
    assert sorted(loaded) == sorted(sd) and loaded['register_tokens'].shape == (1, 4, 128)
    rr.build_dinov2_reg(arch, loaded)                            # strict: the register models' key layout
    assert vt.weights.register_tokens_of(arch, loaded) == 4
    assert vt.weights.register_tokens_of(arch, {k: v for k, v in loaded.items() if k != 'register_tokens'}) == 0
    seen = {}

    class FakeHipViT:
        def __init__(self, state_dict, arch, **kw):
            seen['sd'], seen['arch'] = state_dict, arch
    monkeypatch.setattr(infer.vt, 'HipViT', FakeHipViT)
    monkeypatch.setitem(infer._MODEL_OPTS, 'weights', str(path))
    infer.get_dinov2_model('vits14_reg')
    assert seen['arch'] == 'vits14_reg' and torch.equal(seen['sd']['register_tokens'], sd['register_tokens'])


def test_wrong_register_count_is_refused():
    w = vt.weights
    reg = vt.synthetic_state_dict('vits14_reg', 1)
    plain = vt.synthetic_state_dict('vits14', 1)
    assert w.register_tokens_of('vits14_reg', reg) == 4 and w.register_tokens_of('vits14', plain) == 0
    with pytest.raises(ValueError):
        w.register_tokens_of('vits14_reg', plain)                # a plain checkpoint under a register name
    with pytest.raises(ValueError):
        w.register_tokens_of('vits14', reg)                      # and the other way round
    with pytest.raises(ValueError):
        w.register_tokens_of('vits14_reg', dict(reg, register_tokens=reg['register_tokens'][:, :3]))
    with pytest.raises(ValueError):
        w.register_tokens_of('vits14_reg', dict(reg, register_tokens=reg['register_tokens'][..., :128]))
    with pytest.raises(ValueError):                              # more than the engine's entry points take
        w.register_tokens_of((384, 12, 6, 14), dict(reg, register_tokens=torch.zeros(1, 9, 384)))


# ---------------------------------------------------------------------------- 4. the synthetic recipe
@pytest.mark.parametrize('seed', [0, 3])
def test_synthetic_reg_shares_every_plain_tensor(seed):
    plain = vt.synthetic_state_dict('vits14', seed)
    reg = vt.synthetic_state_dict('vits14_reg', seed)
    assert sorted(reg) == sorted(list(plain) + ['register_tokens'])
    for k in plain:
        assert torch.equal(plain[k].view(torch.int32), reg[k].view(torch.int32)), k
    assert reg['register_tokens'].shape == (1, 4, 384)
    assert 0.3 < float(reg['register_tokens'].std()) < 0.7
    assert not torch.equal(reg['register_tokens'], vt.synthetic_state_dict('vits14_reg', seed + 1)['register_tokens'])
    assert vt.synthetic_state_dict('vitl14_reg', seed)['register_tokens'].shape == (1, 4, 1024)
    assert 'register_tokens' not in vt.synthetic_state_dict((384, 2, 6, 14), seed, layer_scale=True)


# ---------------------------------------------------------------------------- 5. CLI surface
class _Args:
    dino_model = None
    dino2_model = None


@pytest.mark.parametrize('name', REG_NAMES)
def test_load_model_reg(name, tmp_path):
    import infer
    a = _Args(); a.dino2_model = name
    assert infer.load_model(a) == (name, infer.get_dinov2_model, 14)
    assert a.model == name
    a.data_path = str(tmp_path / 'vol.npy'); a.cache_path = None; a.slice_along = 'all'; a.feature_output_size = 64
    a.overwrite = False
    assert infer.handle_output_path(a) == tmp_path / f'vol_{name}_all_features64.npy'


def test_cli_accepts_reg_names_and_refuses_vitg14_reg(tmp_path, capsys, monkeypatch):
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((4, 4, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        infer.get_dinov2_model('vitg14_reg')
    assert e.value.code == 1
    with pytest.raises(SystemExit) as e:
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), '--dino2-model', 'vitg14_reg', '--synthetic-weights', '0'])
    assert e.value.code == 1
    assert 'SwiGLU' in capsys.readouterr().out
    # a register name passes the parser and reaches the model constructor with the register layout
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
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), '--dino2-model', 'vitb14_reg', '--synthetic-weights', '0'])
    assert seen['arch'] == 'vitb14_reg' and seen['sd']['register_tokens'].shape == (1, 4, 768)


# ---------------------------------------------------------------------------- 6. engine batch
def test_engine_batch_vitl14_reg(monkeypatch):
    monkeypatch.delenv('VITTF_ENGINE_BATCH', raising=False)
    ex = vt.extract
    tokens, d = 64 * 64 + 1 + 4, 1024

    class Model:
        num_register_tokens = 4
    assert ex._slice_tokens(Model, 64, 64) == tokens and ex._slice_tokens(object(), 64, 64) == 4097
    limit = ex.wide_batch_limit(tokens, d)
    for req in (None, ex.AtLeast(1024), ex.AtLeast(2)):
        b = ex.engine_batch_for(tokens, d, req, n_reg=4)
        assert 1 <= b <= limit, req
        assert b * tokens * 4 * d <= 0xffffffff                  # what vittf_vit_qkv_features_reg refuses beyond
        assert b * (tokens - 5) * d * 2 < 2 ** 31                # each K-feature output
    assert ex.engine_batch_for(tokens, d, n_reg=4) == limit == 255
    # D <= 768: the register rows do not shrink the default call (1536 slices stay three calls of 512), the limits count them
    assert ex.engine_batch_for(tokens, 384, n_reg=4) == 512 and ex.engine_batch_for(tokens, 768, n_reg=4) == 256
    assert 256 * tokens * 4 * 768 <= 0xffffffff and 512 * tokens * 3 * 384 <= 0xffffffff
    assert ex.engine_batch_for(tokens, 384) == 511                # the same row count without registers: the old rule
    for t in (4097, 16385, 1025, 10):
        for dd in (384, 768, 1024):
            assert ex.engine_batch_for(t, dd, n_reg=0) == ex.engine_batch_for(t, dd)


# ---------------------------------------------------------------------------- 7. fixtures
def _load_maker():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    try:
        import make_golden_dinov2_reg as maker
    finally:
        sys.path.pop(0)
    return maker


@pytest.mark.parametrize('name', ['dinov2_reg_d128', 'dinov2_reg_d384'])
def test_reg_fixtures_regenerate(golden_dir, name):
    maker = _load_maker()
    path = os.path.join(golden_dir, name + '.npz')
    assert os.path.getsize(path) < 347170                        # tests/golden/dinov2_d384.npz
    rec = load_golden(golden_dir, name + '.npz')
    arch, seed, shape, fos, vol_seed = maker.CASES[name]
    assert tuple(int(v) for v in rec['arch']) == arch and int(rec['registers']) == 4 and int(rec['seed']) == seed
    sd = rr.synthetic_reg(arch, seed, 4)
    assert math.isclose(vt.weights.state_dict_checksum(sd), float(rec['weights_checksum']), rel_tol=1e-12), 'generator drift'
    new = maker.case(arch, seed, shape, fos, vol_seed)
    assert sorted(new) == sorted(rec)
    assert np.array_equal(new['vol'], rec['vol']) and np.array_equal(new['im_sz'], rec['im_sz'])
    rows = 0
    for ax in 'zyx':
        for key in 'qkv':
            got, ref = torch.from_numpy(new[f'{key}_{ax}']), torch.from_numpy(rec[f'{key}_{ax}'])
            assert got.shape == ref.shape and got.dtype == torch.float16
            # fp32 on another CPU may round a value to the neighbouring fp16: the bound the reference-made DINOv2 fixtures use
            assert float((got.float() - ref.float()).abs().max()) <= 2e-3 * float(ref.float().abs().max()), (ax, key)
            assert rel_fro(got, ref) < 1e-3, (ax, key)
        rows = max(rows, rec[f'k_{ax}'].shape[0] * (rec[f'k_{ax}'].shape[1] + 5))
    assert rows > 128                                            # one axis is more than one 128-row tile in a single call
