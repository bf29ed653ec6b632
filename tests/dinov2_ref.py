"""CPU fp32 DINOv2 restatement for the tests (test infrastructure, like oracle/).

Upstream facebookresearch/dinov2 is not vendored and cannot be fetched; its block is restated from the published code
(hub entries ``dinov2_vit{s,b,l}14``: ``patch_size=14, img_size=518, init_values=1.0, ffn_layer="mlp"``, no register
tokens, ``interpolate_offset=0.1``):

    x = x + ls1(attn(norm1(x)));  x = x + ls2(mlp(norm2(x)));  ls(y) = y * gamma

Everything else -- PatchEmbed, CLS + bicubic scale-factor position embedding, LayerNorm eps 1e-6, the attention, the erf
GELU MLP, the hooked ``blocks[-1].attn.qkv`` -- is DINO v1's, so the model subclasses oracle.dino_vit and keeps its test
helpers (``tokens_before_block``, ``last_block_k``): oracle.feature_volume drives it unchanged, and so does the reference's
own ``compute_qkv`` (tests/golden/make_golden_dinov2.py).  LayerScale stays explicit and unfolded here; the engine folds it
into the weights (vit_tf_amd.weights.fold_layer_scale).
"""
import math

import torch
import torch.nn as nn

from oracle import dino_vit


class LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Block(dino_vit.Block):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, eps=1e-6):
        super().__init__(dim, num_heads, mlp_ratio, eps)
        self.ls1 = LayerScale(dim)
        self.ls2 = LayerScale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        x = x + self.ls2(self.mlp(self.norm2(x)))
        return x


class VisionTransformer(dino_vit.VisionTransformer):
    def __init__(self, patch_size=14, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4.0, stored_img_size=518):
        super().__init__(patch_size, embed_dim, depth, num_heads, mlp_ratio, stored_img_size)
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio) for _ in range(depth)])
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))       # unused at inference (upstream: masked training)


def build_dinov2(arch, state_dict):
    """arch: a DINOv2 name ('vits14', ...) or (D, depth, heads, patch); the stored position grid is read off
    ``pos_embed`` (37 x 37 for the hub models).  The state dict is loaded strictly: the DINOv2 key layout, gammas and
    mask_token included."""
    import vit_tf_amd as vt
    dim, depth, heads, patch = vt.weights.arch_of(arch)
    grid = int(math.isqrt(state_dict['pos_embed'].shape[1] - 1))
    model = VisionTransformer(patch, dim, depth, heads, stored_img_size=grid * patch)
    model.load_state_dict(state_dict, strict=True)
    return model.eval()
