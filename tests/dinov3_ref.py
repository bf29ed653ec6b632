"""CPU fp32 restatement of DINOv3 ViT-S/16, B/16 and L/16 for the tests (test infrastructure, like tests/dinov2_reg_ref.py).

Restated from the published model (nothing vendored); tests/test_dinov3_cpu.py checks this file against
``transformers.DINOv3ViTModel``.  Against the DINOv2 register models (tests/dinov2_reg_ref.py):

* patch 16; tokens ``[CLS, reg_0 .. reg_3, patch_0 ..]``; NO additive position embedding: the embedding is the patch conv
  plus ``cls_token`` / the register rows;
* LayerNorm eps 1e-5; q and v have biases, k has none (the k third of the fused ``attn.qkv.bias`` is zero: the canonical
  layout of vit_tf_amd.weights.dinov3_canonical / dinov3_from_hf);
* rotary position embedding in every block: per head of 64, with ``rot(v) = cat(-v[32:64], v[0:32])``,
  ``q' = q cos + rot(q) sin`` and the same for k, for the patch tokens only, the same table for every head.  The table is
  restated here on its own (``rope_cos_sin``: 64 columns, like upstream), not taken from the package.

The attention keeps a fused ``attn.qkv`` Linear, so the hooked tensor (``blocks[-1].attn.qkv``'s output, BEFORE the rotation)
sits where the reference's hook sits.  LayerScale stays explicit and unfolded.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import dinov2_ref
from oracle import dino_vit, feature_volume as ofv

PARTS = ('q', 'k', 'v')
LN_EPS = 1e-5
ROPE_THETA = 100.0


def rope_cos_sin(f0, f1, head_dim=64):
    """(cos, sin), each fp32 (f0 * f1, head_dim): angle[0:d/4] = 2 pi cy inv_freq, angle[d/4:d/2] = 2 pi cx inv_freq, tiled
    twice; cy, cx the patch centres in [-1, 1]; inv_freq = 1 / theta ** arange(0, 1, 4 / d)."""
    inv_freq = 1 / ROPE_THETA ** torch.arange(0, 1, 4 / head_dim, dtype=torch.float32)
    cy = 2.0 * (torch.arange(0.5, f0, dtype=torch.float32) / f0) - 1.0
    cx = 2.0 * (torch.arange(0.5, f1, dtype=torch.float32) / f1) - 1.0
    coords = torch.stack(torch.meshgrid(cy, cx, indexing='ij'), dim=-1).flatten(0, 1)
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2).tile(2)
    return torch.cos(angles), torch.sin(angles)


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


class Attention(dino_vit.Attention):
    def forward(self, x, cos, sin):
        b, n, c = x.shape
        qkv = self.qkv(x).reshape(b, n, 3, self.num_heads, c // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]                         # (B, heads, N, 64)
        prefix = n - cos.shape[0]                                # CLS + registers: not rotated
        q = torch.cat((q[..., :prefix, :], q[..., prefix:, :] * cos + rotate_half(q[..., prefix:, :]) * sin), dim=-2)
        k = torch.cat((k[..., :prefix, :], k[..., prefix:, :] * cos + rotate_half(k[..., prefix:, :]) * sin), dim=-2)
        att = ((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return self.proj((att @ v).transpose(1, 2).reshape(b, n, c))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim, num_heads)
        self.ls1 = dinov2_ref.LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = dino_vit.Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = dinov2_ref.LayerScale(dim)

    def forward(self, x, cos, sin):
        x = x + self.ls1(self.attn(self.norm1(x), cos, sin))
        return x + self.ls2(self.mlp(self.norm2(x)))


class VisionTransformer(nn.Module):
    def __init__(self, num_register_tokens=4, patch_size=16, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4.0):
        super().__init__()
        self.embed_dim, self.num_register_tokens = embed_dim, num_register_tokens
        self.patch_embed = dino_vit.PatchEmbed(patch_size, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=LN_EPS)
        self.identity_rope = False        # tests: cos = 1, sin = 0 (a rotation that is silently skipped)

    def prepare_tokens(self, x):
        b = x.shape[0]
        return torch.cat((self.cls_token.expand(b, -1, -1), self.register_tokens.expand(b, -1, -1), self.patch_embed(x)), dim=1)

    def rope(self, x):
        p = self.patch_embed.patch_size
        cos, sin = rope_cos_sin(x.shape[-2] // p, x.shape[-1] // p)
        return (torch.ones_like(cos), torch.zeros_like(sin)) if self.identity_rope else (cos, sin)

    def tokens_before_block(self, x, idx):
        """Residual stream entering block ``idx`` (0-based; idx = depth: behind the last block, before the final norm)."""
        cos, sin = self.rope(x)
        t = self.prepare_tokens(x)
        for blk in self.blocks[:idx]:
            t = blk(t, cos, sin)
        return t

    def forward(self, x):
        return self.norm(self.tokens_before_block(x, len(self.blocks)))[:, 0]

    def last_block_qkv(self, x):
        """The hooked tensor, blocks[-1].attn.qkv of every token, before the rotation: (B, 1 + R + n, 3 D) fp32."""
        blk = self.blocks[-1]
        return blk.attn.qkv(blk.norm1(self.tokens_before_block(x, len(self.blocks) - 1)))


def build_dinov3(arch, state_dict):
    """arch: a DINOv3 name ('dinov3_vits16', ...) or (D, depth, heads, patch); state_dict in Meta's layout or the canonical one
    (vit_tf_amd.weights.dinov3_canonical is applied: registers under ``register_tokens``, k bias zeroed, buffers dropped),
    then loaded strictly."""
    import vit_tf_amd as vt
    dim, depth, heads, patch = vt.weights.arch_of(arch)
    sd = vt.weights.dinov3_canonical(state_dict)
    model = VisionTransformer(int(sd['register_tokens'].shape[1]), patch, dim, depth, heads)
    model.load_state_dict(sd, strict=True)
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


def synthetic_v3(arch, seed):
    """Seeded weights in Meta's DINOv3 layout for a tuple arch (the package's recipe: non-zero k bias + bias_mask)."""
    import vit_tf_amd as vt
    return vt.synthetic_state_dict(arch, seed, dinov3=True)
