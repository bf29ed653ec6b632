"""CPU fp32 restatement of the DINOv2 register models for the tests (test infrastructure, like tests/dinov2_ref.py).

Hub entries ``dinov2_vit{s,b,l}14_reg`` are the plain DINOv2 entries (tests/dinov2_ref.py) with three differences, restated
from the published code (nothing vendored):

* ``num_register_tokens = 4``: the state dict gains ``register_tokens`` (1, R, D);
* the token order is ``[CLS, reg_0 .. reg_{R-1}, patch_0 ..]``: the position embedding is added to CLS and the patches
  first, the registers are inserted afterwards and get none;
* ``interpolate_offset = 0.0`` and ``interpolate_antialias = True``: the stored grid is resized with
  ``F.interpolate(size=(r0, c0), mode='bicubic', antialias=True)`` (identity for the stored square grid at a square image).

The registers take part in the attention of every block; they leave together with CLS when the hooked q / k / v thirds are
cut to the patch tokens (``qkv_axis`` below; the reference's ``k[:, 1:]`` cannot do that, so neither the reference nor
oracle.feature_volume drives this model).  tests/test_dinov2_reg_cpu.py checks this file against
``transformers.Dinov2WithRegistersModel``.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import dinov2_ref
from oracle import feature_volume as ofv

PARTS = ('q', 'k', 'v')


def interpolate_pos_embed_reg(pos_embed, rows, cols, patch):
    """(1, 1 + r0 * c0, D): the stored (1, 1 + G * G, D) embedding resized by size with antialiased bicubic interpolation."""
    n = pos_embed.shape[1] - 1
    g = math.isqrt(n)
    d = pos_embed.shape[-1]
    r0, c0 = rows // patch, cols // patch
    if r0 * c0 == n and rows == cols:
        return pos_embed
    grid = F.interpolate(pos_embed[:, 1:].reshape(1, g, g, d).permute(0, 3, 1, 2), size=(r0, c0), mode='bicubic',
                         antialias=True)
    return torch.cat((pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, d)), dim=1)


class VisionTransformer(dinov2_ref.VisionTransformer):
    def __init__(self, num_register_tokens=4, patch_size=14, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4.0,
                 stored_img_size=518):
        super().__init__(patch_size, embed_dim, depth, num_heads, mlp_ratio, stored_img_size)
        self.num_register_tokens = num_register_tokens
        self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim))

    def prepare_tokens(self, x):
        b, _, rows, cols = x.shape
        tok = self.patch_embed(x)
        tok = torch.cat((self.cls_token.expand(b, -1, -1), tok), dim=1)
        tok = tok + interpolate_pos_embed_reg(self.pos_embed, rows, cols, self.patch_embed.patch_size)
        return torch.cat((tok[:, :1], self.register_tokens.expand(b, -1, -1), tok[:, 1:]), dim=1)

    def last_block_qkv(self, x):
        """The hooked tensor, blocks[-1].attn.qkv of every token: (B, 1 + R + n, 3 D) fp32."""
        t = self.tokens_before_block(x, len(self.blocks) - 1)
        blk = self.blocks[-1]
        return blk.attn.qkv(blk.norm1(t))


def build_dinov2_reg(arch, state_dict):
    """arch: a register-model name ('vits14_reg', ...) or (D, depth, heads, patch); R and the stored grid are read off the
    state dict, which is loaded strictly (the plain DINOv2 keys + ``register_tokens``)."""
    import vit_tf_amd as vt
    dim, depth, heads, patch = vt.weights.arch_of(arch)
    grid = math.isqrt(state_dict['pos_embed'].shape[1] - 1)
    model = VisionTransformer(int(state_dict['register_tokens'].shape[1]), patch, dim, depth, heads,
                              stored_img_size=grid * patch)
    model.load_state_dict(state_dict, strict=True)
    return model.eval()


def patch_qkv(model, x):
    """{'q' | 'k' | 'v': (B, n, D) fp16}: the hooked thirds rounded as the hook rounds them (fp32 -> fp16), CLS and the
    registers dropped."""
    d = model.embed_dim
    with torch.no_grad():
        t = model.last_block_qkv(x).half()[:, 1 + model.num_register_tokens:]
    return {key: t[..., i * d:(i + 1) * d].contiguous() for i, key in enumerate(PARTS)}


def qkv_axis(vol, model, im_sizes, axis, batch_size=4):
    """Un-pooled fp16 q, k, v of every slice of one axis, token-major: {'q' | 'k' | 'v': (S, f0 * f1, D)} -- the volume
    normalised and nearest-resized exactly as oracle.feature_volume does it (infer.py:137, 154-155, 177)."""
    imgs = ofv.normalized_slices(vol, axis)
    rows, cols = ofv.axis_image_size(im_sizes, axis)
    out = {key: [] for key in PARTS}
    for idx in torch.arange(imgs.shape[0]).split(batch_size):
        res = patch_qkv(model, F.interpolate(imgs[idx], size=(rows, cols), mode='nearest'))
        for key in PARTS:
            out[key].append(res[key])
    return {key: torch.cat(v) for key, v in out.items()}


def synthetic_reg(arch, seed, num_register_tokens=4, stored_grid=37):
    """Seeded weights in the register models' layout for a tuple arch: the synthetic DINOv2 recipe + ``register_tokens`` of
    std 0.5 from a generator of their own."""
    import vit_tf_amd as vt
    sd = vt.synthetic_state_dict(arch, seed, stored_grid=stored_grid, layer_scale=True)
    g = torch.Generator().manual_seed(0x7265 + seed)
    sd['register_tokens'] = 0.5 * torch.randn(1, num_register_tokens, vt.weights.arch_of(arch)[0], generator=g)
    return sd
