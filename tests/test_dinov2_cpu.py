"""CPU: DINOv2 (patch 14, LayerScale) -- the test model, the fixtures, LayerScale folding, the CLI surface, batch limits.

* tests/dinov2_ref.py against transformers.Dinov2Model (an independent DINOv2 implementation in the image, built from a config
  object: no download) at a grid-equal square input, where both resize nothing.
* tests/dinov2_ref.py reproduces the fixtures made with the reference's compute_qkv (tests/golden/make_golden_dinov2.py).
* fold_layer_scale: with the folded weights rounded to fp16 (what the engine uploads) the K features stay within 1e-3 of the
  unfolded fp32 model for gammas down to 1e-6; gammas of exactly 1.0 change no byte of the prepared weights.
* infer.py's --dino2-model path, the hub cache lookup, the DINOv2 checkpoint layout, and the ViT-L/14 engine batch.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_tf_amd as vt
from dinov2_ref import build_dinov2
from helpers import load_golden, rel_fro
from oracle import dino_vit, feature_volume as ofv

FIXTURES = {'dinov2_d128.npz': (128, 3, 2, 14), 'dinov2_d384.npz': (384, 2, 6, 14)}


def _perturbed_dinov2(arch, seed, grid):
    """Synthetic DINOv2 weights with random biases, LayerNorm affines and gammas (every term of the block counts)."""
    sd = vt.synthetic_state_dict(arch, seed, stored_grid=grid, layer_scale=True)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if k.endswith('.bias'):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif 'norm' in k and k.endswith('.weight'):
            sd[k] = 1.0 + 0.2 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith('.gamma'):
            sd[k] = 0.05 + torch.rand(sd[k].shape, generator=g)
    return sd


def _hf_from_dinov2(sd, dim, depth, heads, patch, grid):
    transformers = pytest.importorskip('transformers')
    cfg = transformers.Dinov2Config(hidden_size=dim, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=4,
                                    hidden_act='gelu', hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                    layer_norm_eps=1e-6, image_size=grid * patch, patch_size=patch, num_channels=3,
                                    qkv_bias=True, layerscale_value=1.0, use_swiglu_ffn=False)
    model = transformers.Dinov2Model(cfg).eval()
    hf = {'embeddings.cls_token': sd['cls_token'], 'embeddings.mask_token': sd['mask_token'],
          'embeddings.position_embeddings': sd['pos_embed'],
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


@pytest.mark.parametrize('arch', [(128, 3, 2, 14), (384, 2, 6, 14)])
def test_dinov2_ref_matches_transformers_dinov2(arch):
    dim, depth, heads, patch = arch
    grid = 4
    sd = _perturbed_dinov2(arch, 5, grid)
    ours = build_dinov2(arch, sd)
    hf = _hf_from_dinov2(sd, dim, depth, heads, patch, grid)
    x = torch.randn(2, 3, grid * patch, grid * patch, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        out = hf(pixel_values=x, output_hidden_states=True)
        stream = ours.tokens_before_block(x, depth - 1)
        k_ref = ours.last_block_k(x)
        last = hf.encoder.layer[-1]
        k_hf = last.attention.attention.key(last.norm1(out.hidden_states[depth - 1]))
        cls = ours(x)
    assert float((out.hidden_states[depth - 1] - stream).abs().max()) <= 2e-5 * float(stream.abs().max())
    assert float((k_hf - k_ref).abs().max()) <= 2e-5 * float(k_ref.abs().max())
    assert float((out.last_hidden_state[:, 0] - cls).abs().max()) <= 2e-5 * float(cls.abs().max())
    # the LayerScale is live: the same weights with unit gammas give a different stream
    sd1 = dict(sd, **{k: torch.ones_like(v) for k, v in sd.items() if k.endswith('.gamma')})
    with torch.no_grad():
        assert rel_fro(build_dinov2(arch, sd1).last_block_k(x), k_ref) > 1e-2


def _qkv_third(model, imgs, rows, cols, part):
    """fp16 third `part` of blocks[-1].attn.qkv for the patch tokens of every image -> (S, f0 * f1, D)."""
    d = model.embed_dim
    blk = model.blocks[-1]
    out = []
    with torch.no_grad():
        for i in range(imgs.shape[0]):
            x = F.interpolate(imgs[i:i + 1], size=(rows, cols), mode='nearest')
            t = model.tokens_before_block(x, len(model.blocks) - 1)
            out.append(F.linear(blk.norm1(t), blk.attn.qkv.weight[part * d:(part + 1) * d],
                                blk.attn.qkv.bias[part * d:(part + 1) * d]).half()[0, 1:])
    return torch.stack(out)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_dinov2_ref_reproduces_reference_fixtures(golden_dir, name):
    rec = load_golden(golden_dir, name)
    arch = tuple(int(v) for v in rec['arch'])
    assert arch == FIXTURES[name]
    sd = vt.synthetic_state_dict(arch, int(rec['seed']), stored_grid=vt.weights.DINOV2_STORED_GRID, layer_scale=True)
    assert math.isclose(vt.weights.state_dict_checksum(sd), float(rec['weights_checksum']), rel_tol=1e-12), 'generator drift'
    model = build_dinov2(arch, sd)
    vol = torch.from_numpy(rec['vol'])
    im_sz = tuple(int(v) for v in rec['im_sz'])
    for ax in 'zyx':
        got = ofv.k_features_axis(vol, model, 14, im_sz, ax, batch_size=4)
        ref = torch.from_numpy(rec[f'k_{ax}'])
        assert got.shape == ref.shape
        assert float((got.float() - ref.float()).abs().max()) <= 2e-3 * float(ref.float().abs().max()), ax
    got = ofv.feature_volume(vol, model, 14, int(rec['fos']), 'all', batch_size=2)
    ref = torch.from_numpy(rec['k_all'])
    assert got.shape == ref.shape and rel_fro(got, ref) < 1e-3
    # q and v of the z axis (reference layout: (D, W', H', S))
    imgs = ofv.normalized_slices(vol, 'z')
    rows, cols = ofv.axis_image_size(im_sz, 'z')
    f0, f1 = rows // 14, cols // 14
    for part, key in ((0, 'q_z'), (2, 'v_z')):
        t = _qkv_third(model, imgs, rows, cols, part)
        got = t.view(t.shape[0], f0, f1, -1).permute(3, 1, 2, 0)
        ref = torch.from_numpy(rec[key])
        assert got.shape == ref.shape and rel_fro(got, ref) < 1e-3, key


def _round_linears_fp16(sd):
    return {k: (v.half().float() if any(f'.{n}.weight' in k for n in ('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')) else v)
            for k, v in sd.items()}


def test_layer_scale_folding_within_fp16_bound():
    """The engine's preparation simulated on the CPU: fold in fp32, round the linears to fp16, run the plain DINO block.
    Gammas log-uniform over [1e-6, 1] (so |gamma w| crosses fp16's subnormal floor): K features within 1e-3 relative
    Frobenius of the unfolded fp32 DINOv2 model."""
    arch = (384, 3, 6, 14)
    sd = vt.synthetic_state_dict(arch, 11, stored_grid=4, layer_scale=True)
    g = torch.Generator().manual_seed(12)
    for k in sd:
        if k.endswith('.gamma'):
            sd[k] = 10.0 ** (torch.rand(sd[k].shape, generator=g) * -6.0)
    assert min(float(v.min()) for k, v in sd.items() if k.endswith('.gamma')) < 1e-5
    ref_model = build_dinov2(arch, sd)
    folded = vt.fold_layer_scale(sd)
    assert not any(k.endswith('.gamma') for k in folded)
    folded.pop('mask_token')
    plain = dino_vit.build_vit(arch, _round_linears_fp16(folded), stored_img_size=4 * 14)
    x = torch.rand(3, 1, 56, 70, generator=g)
    x = (x.expand(-1, 3, -1, -1) - torch.tensor(ofv.IN_MEAN).view(1, 3, 1, 1)) / torch.tensor(ofv.IN_STD).view(1, 3, 1, 1)
    with torch.no_grad():
        want = ref_model.last_block_k(x)
        got = plain.last_block_k(x)
        # folding alone (fp32, no rounding) is exact up to fp32 reassociation
        exact = dino_vit.build_vit(arch, folded, stored_img_size=4 * 14).last_block_k(x)
    assert rel_fro(exact, want) < 1e-5
    err = rel_fro(got, want)
    assert err < 1e-3, err


def test_unit_gammas_prepare_identical_weights():
    """A DINO v1 state dict plus ls gammas of exactly 1.0 prepares byte-identical weights to the same dict without them."""
    arch = (384, 2, 6, 8)
    sd = vt.synthetic_state_dict(arch, 3)
    assert vt.fold_layer_scale(sd) is sd            # no ls keys: the v1 path is untouched
    with_ls = dict(sd)
    for i in range(2):
        with_ls[f'blocks.{i}.ls1.gamma'] = torch.ones(384)
        with_ls[f'blocks.{i}.ls2.gamma'] = torch.ones(384)
    folded = vt.fold_layer_scale(with_ls)
    assert sorted(folded) == sorted(sd)
    for k in sd:
        assert torch.equal(folded[k].view(torch.int32), sd[k].view(torch.int32)), k
        assert torch.equal(folded[k].half().view(torch.int16), sd[k].half().view(torch.int16)), k

    def stack(d, name):
        return torch.stack([d[f'blocks.{i}.{name}.weight'] for i in range(2)]).half()
    packed = [vt.weights.pack_block_tail_weights(stack(d, 'attn.proj'), stack(d, 'mlp.fc1'), stack(d, 'mlp.fc2'))
              for d in (sd, folded)]
    assert torch.equal(packed[0].view(torch.int16), packed[1].view(torch.int16))


def test_synthetic_dinov2_keys_and_v1_unchanged():
    sd = vt.synthetic_state_dict('vits14', 0)
    assert sd['pos_embed'].shape == (1, 1 + 37 * 37, 384) and sd['mask_token'].shape == (1, 384)
    assert sd['patch_embed.proj.weight'].shape == (384, 3, 14, 14)
    gam = torch.cat([v for k, v in sd.items() if k.endswith('.gamma')])
    assert gam.numel() == 2 * 12 * 384 and float(gam.min()) >= 1e-5 and float(gam.max()) <= 1.0 and float(gam.min()) < 1e-4
    # tuple archs get the DINOv2 keys only on request; the DINO tensors of a seed do not depend on the request
    a = vt.synthetic_state_dict((128, 2, 2, 14), 4)
    b = vt.synthetic_state_dict((128, 2, 2, 14), 4, layer_scale=True)
    assert not any(k.endswith('.gamma') or k == 'mask_token' for k in a)
    assert all(torch.equal(a[k], b[k]) for k in a) and len(b) == len(a) + 1 + 4
    assert vt.ARCHS['vits14'] == (384, 12, 6, 14) and vt.ARCHS['vitb14'] == (768, 12, 12, 14)
    assert vt.ARCHS['vitl14'] == (1024, 24, 16, 14) and all(len(v) == 4 for v in vt.ARCHS.values())


# ---------------------------------------------------------------------------- CLI surface
class _Args:
    dino_model = None
    dino2_model = None


def test_load_model_dinov2():
    import infer
    a = _Args(); a.dino2_model = 'vits14'
    assert infer.load_model(a) == ('vits14', infer.get_dinov2_model, 14)
    assert a.model == 'vits14'
    with pytest.raises(SystemExit) as e:
        infer.get_dinov2_model('vitg14')
    assert e.value.code == 1


def test_vitg14_cli_exits_1(tmp_path, capsys):
    import infer
    np.save(tmp_path / 'vol.npy', np.zeros((4, 4, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        infer.main(['--data-path', str(tmp_path / 'vol.npy'), '--dino2-model', 'vitg14', '--synthetic-weights', '0'])
    assert e.value.code == 1
    assert 'SwiGLU' in capsys.readouterr().out


def test_dinov2_output_name(tmp_path):
    import infer
    a = _Args(); a.dino2_model = 'vits14'
    infer.load_model(a)
    a.data_path = str(tmp_path / 'vol.npy'); a.cache_path = None; a.slice_along = 'z'; a.feature_output_size = 32
    a.overwrite = False
    assert infer.handle_output_path(a) == tmp_path / 'vol_vits14_z_features32.npy'


def test_find_local_checkpoint_dinov2(tmp_path, monkeypatch):
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    assert vt.find_local_checkpoint('vitb14') is None
    ck = tmp_path / 'hub' / 'checkpoints'
    ck.mkdir(parents=True)
    (ck / 'dinov2_vitb14_pretrain.pth').write_bytes(b'')
    assert vt.find_local_checkpoint('vitb14') == str(ck / 'dinov2_vitb14_pretrain.pth')
    assert vt.find_local_checkpoint('vitl14') is None


def test_dinov2_checkpoint_layout_loads(tmp_path, monkeypatch):
    """A DINOv2-layout checkpoint (gammas, mask_token) goes through load_state_dict_file and get_dinov2_model; mask_token is
    carried but unused, the gammas reach the engine's folding."""
    import infer
    arch = (128, 2, 2, 14)
    sd = vt.synthetic_state_dict(arch, 6, stored_grid=37, layer_scale=True)
    path = tmp_path / 'dinov2.pth'
    torch.save({'teacher': {'backbone.' + k: v for k, v in sd.items()}}, path)
    loaded = vt.load_state_dict_file(str(path))
    assert sorted(loaded) == sorted(sd) and 'mask_token' in loaded
    build_dinov2(arch, loaded)                     # strict: the DINOv2 key layout
    seen = {}

    class FakeHipViT:
        def __init__(self, state_dict, arch, **kw):
            seen['sd'], seen['arch'] = state_dict, arch
    monkeypatch.setattr(infer.vt, 'HipViT', FakeHipViT)
    monkeypatch.setitem(infer._MODEL_OPTS, 'weights', str(path))
    infer.get_dinov2_model('vits14')
    assert seen['arch'] == 'vits14' and 'blocks.1.ls2.gamma' in seen['sd']
    folded = vt.fold_layer_scale(seen['sd'])
    assert torch.equal(folded['blocks.1.mlp.fc2.bias'], sd['blocks.1.mlp.fc2.bias'] * sd['blocks.1.ls2.gamma'])
    # synthetic weights for a DINOv2 name: the DINOv2 layout
    monkeypatch.setitem(infer._MODEL_OPTS, 'weights', None)
    monkeypatch.setitem(infer._MODEL_OPTS, 'synthetic_seed', 1)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    monkeypatch.delenv('VITTF_WEIGHTS', raising=False)
    infer.get_dinov2_model('vitb14')
    assert seen['sd']['pos_embed'].shape == (1, 1 + 37 * 37, 768) and 'blocks.11.ls1.gamma' in seen['sd']


# ---------------------------------------------------------------------------- ViT-L/14 engine batch
def test_engine_batch_vitl14_offsets(monkeypatch):
    monkeypatch.delenv('VITTF_ENGINE_BATCH', raising=False)
    eb = vt.extract.engine_batch_for
    for tokens in (4097, 16385, 1025, 10):
        for req in (None, vt.extract.AtLeast(5000), vt.extract.AtLeast(2), 3):
            b = eb(tokens, 1024, req)
            assert b * tokens * 4 * 1024 < 2 ** 32, (tokens, req)
            assert b * (tokens - 1) * 1024 * 2 < 2 ** 31, (tokens, req)
    assert eb(4097, 1024) == 255 and eb(4097, 1024, vt.extract.AtLeast(5000)) == 255
    assert eb(4097, 1024, 3) == 3 and eb(4097, 1024, vt.extract.AtLeast(3)) == 255
    # D <= 768 unchanged
    assert eb(4097, 384) == 512 and eb(4097, 768) == 256 and eb(16385, 384) == 128 and eb(16385, 768) == 64
    assert eb(4097, 384, vt.extract.AtLeast(5000)) == 1024 and eb(4097, 768, vt.extract.AtLeast(5000)) == 1024
