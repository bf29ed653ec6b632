"""HipViT: the DINO ViT as an HBM-resident weight set driven through libvittf's C ABI.

Stands where ``torch.hub.load('facebookresearch/dino:main', 'dino_vits8').to(dev).eval()`` stands in
the reference (infer.py:323): an object the extraction loop hands slices to.  It exposes what the
reference reads off the upstream module (``num_heads`` via ``blocks[-1].attn.num_heads`` infer.py:180,
the patch size, the embedding width) but runs nothing in PyTorch: torch only owns the device buffers.
"""
import ctypes as C

import torch

from . import _lib
from .weights import (DINOV3_LN_EPS, arch_of, dinov3_canonical, fold_layer_scale, fold_patch_embed, interpolate_pos_embed,
                      is_dinov3, pack_block_tail_weights, pack_row_images, pos_embed_antialias_of, register_tokens_of,
                      rope_table)

_TORCH_DT = {_lib.BF16: torch.bfloat16, _lib.FP16: torch.float16}


def resolve_layer(layer, depth):
    """Index of the hooked block: 0-based, negatives count from the end, None = the last block.  ValueError when out of range."""
    if layer is None:
        return int(depth) - 1
    idx = int(layer)
    if idx < 0:
        idx += int(depth)
    if not 0 <= idx < int(depth):
        raise ValueError(f'layer {layer} is out of range for a model of {depth} blocks (valid: {-int(depth)} .. {int(depth) - 1})')
    return idx


class _Attn:
    def __init__(self, heads):
        self.num_heads = heads


class _Block:
    def __init__(self, heads):
        self.attn = _Attn(heads)


class HipViT:
    """Weights + workspace of one ViT on one GPU.

    state_dict: DINO-layout tensors (fp32, CPU or GPU; DINOv2's LayerScale gammas are folded in).  arch: DINO / DINOv2 / DINOv3
    name ('vits8', 'vits14', 'vits14_reg', 'dinov3_vits16', ...) or
    (embed_dim, depth, heads, patch).  A ``register_tokens`` key (1, R, D) makes it a register model (the DINOv2 ``_reg`` names
    require it, a tuple arch follows the key): ``num_register_tokens`` = R rows behind CLS in every slice, kept on the device,
    and the size-based antialiased position-embedding resize.  dtype of the MFMA operands: 'fp16' (default: the reference's own GPU autocast
    type, infer.py:309; meets the 1e-3 parity bound against the fp32 CPU path) or 'bf16' (opt-in: 8-bit mantissa,
    2.4e-3 .. 3.9e-3 against the CPU path).  attention: '16bit' (default) or 'fp8' -- BASELINE configs[3]'s fp8 MFMA
    attention path (e4m3 operands on the block-scaled matrix instruction; ~3e-2 on the features: opt-in).
    A DINOv3 model ('dinov3_vits16', ...; a tuple arch with a state dict without ``pos_embed``): LayerNorm eps 1e-5, the key
    bias zeroed, no additive position embedding, and the rotary table of the image size (``rope_for``) handed to the engine,
    which rotates q and k of the patch tokens in every block; attention='fp8' is refused for it (ValueError): that path
    quantises q and k inside the qkv GEMM, before the rotation.
    fused_tail=False: ViT-S without the packed weight streams (the block tail and the activation-stationary qkv GEMM): the GEMM
    launches every other width uses; flags: _lib.CFG_* bits (vittf_vit_config.flags), the slower alternatives the tests also run.
    layer: the hooked block (resolve_layer: 0-based, negatives from the end, default the last): q, k and v are the thirds of
    ``blocks[layer].attn.qkv``, the token facet (part 3) is the model's final ``norm`` of the patch tokens behind ``blocks[layer]``
    (``get_intermediate_layers(norm=True)``).  The engine is told a model of ``layer + 1`` blocks; the weight stacks stay whole.
    """

    def __init__(self, state_dict, arch='vits8', dtype='fp16', device=None, attention='16bit', fused_tail=True, flags=0,
                 layer=None):
        self.lib = _lib.require_device()
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        dim, depth, heads, patch = arch_of(arch)
        if heads * 64 != dim:
            raise ValueError('HipViT supports head dim 64 only (all DINO ViTs)')
        self.embed_dim, self.depth, self.num_heads, self.patch_size = dim, depth, heads, patch
        self.layer = resolve_layer(layer, depth)
        self.dtype_id = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        self.dtype_name = 'bf16' if self.dtype_id == _lib.BF16 else 'fp16'
        self.blocks = [_Block(heads) for _ in range(depth)]    # duck-typing of model.blocks[-1].attn.num_heads
        if attention not in ('16bit', 'fp8'):
            raise ValueError(f"attention must be '16bit' or 'fp8', got {attention!r}")
        self.attention = attention
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        self.rope = is_dinov3(arch, sd)
        if self.rope:
            if attention == 'fp8':
                raise ValueError('attention=\'fp8\' is not available for DINOv3: q and k are quantised inside the qkv GEMM, before '
                                 'the rotary embedding could be applied')
            sd = dinov3_canonical(sd)
        self.cfg = _lib.VitConfig(dim, self.layer + 1, heads, patch, self.dtype_id, DINOV3_LN_EPS if self.rope else 1e-6,
                                  1 if attention == 'fp8' else 0, int(flags))
        self.num_register_tokens = register_tokens_of(arch, sd)
        self._pos_antialias = pos_embed_antialias_of(arch, sd)
        # DINOv2 LayerScale (blocks.{i}.ls1 / ls2.gamma present, whatever the arch name): folded into attn.proj / mlp.fc2 in
        # fp32 before the one conversion to 16 bits -- the kernels see ordinary weights
        sd = fold_layer_scale(sd)
        h16 = _TORCH_DT[self.dtype_id]
        dev = self.device

        def stack(fmt, dt):
            return torch.stack([sd[fmt.format(i)] for i in range(depth)]).to(dev, dt).contiguous()

        pe_w_t, pe_b = fold_patch_embed(sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'])
        self._t = {
            'pe_w_t': pe_w_t.to(dev).contiguous(), 'pe_b': pe_b.to(dev).contiguous(),
            'qkv_w': stack('blocks.{}.attn.qkv.weight', h16), 'qkv_b': stack('blocks.{}.attn.qkv.bias', torch.float32),
            'proj_w': stack('blocks.{}.attn.proj.weight', h16), 'proj_b': stack('blocks.{}.attn.proj.bias', torch.float32),
            'fc1_w': stack('blocks.{}.mlp.fc1.weight', h16), 'fc1_b': stack('blocks.{}.mlp.fc1.bias', torch.float32),
            'fc2_w': stack('blocks.{}.mlp.fc2.weight', h16), 'fc2_b': stack('blocks.{}.mlp.fc2.bias', torch.float32),
            'ln1_g': stack('blocks.{}.norm1.weight', torch.float32), 'ln1_b': stack('blocks.{}.norm1.bias', torch.float32),
            'ln2_g': stack('blocks.{}.norm2.weight', torch.float32), 'ln2_b': stack('blocks.{}.norm2.bias', torch.float32),
        }
        ptrs = {k: v.data_ptr() for k, v in self._t.items()}
        ptrs['tail_packed'] = ptrs['qkv_packed'] = None
        if fused_tail and dim == 384:          # the kernels' register budgets are sized for ViT-S
            self._t['tail_packed'] = pack_block_tail_weights(self._t['proj_w'], self._t['fc1_w'], self._t['fc2_w'])
            self._t['qkv_packed'] = pack_row_images(self._t['qkv_w'])
            ptrs['tail_packed'] = self._t['tail_packed'].data_ptr()
            ptrs['qkv_packed'] = self._t['qkv_packed'].data_ptr()
        self.weights = _lib.VitWeights(**ptrs)
        # the model's final LayerNorm (fp32): only the token facet runs it, so only that facet needs it in the state dict
        has_norm = 'norm.weight' in sd and 'norm.bias' in sd
        self._norm_g = sd['norm.weight'].to(dev, torch.float32).contiguous() if has_norm else None
        self._norm_b = sd['norm.bias'].to(dev, torch.float32).contiguous() if has_norm else None
        # [R][D] fp32 rows the embedding kernels copy behind CLS (no position embedding)
        self._reg = sd['register_tokens'].reshape(-1, dim).to(dev).contiguous() if self.num_register_tokens else None
        self._cls = sd['cls_token'].reshape(1, 1, dim)
        self._pos = None if self.rope else sd['pos_embed']
        self._pos_cache = {}
        self._rope_cache = {}
        self._ws = None

    # -- reference-shaped conveniences --------------------------------------------------------------
    def to(self, *_a, **_k):
        return self

    def eval(self):
        return self

    # -- device-side pieces ---------------------------------------------------------------------------
    def pos_for(self, rows, cols):
        """Device position embedding for a rows x cols image: (PosEmbed struct, keep-alive tensors)."""
        key = (rows, cols)
        if key not in self._pos_cache and self.rope:
            # DINOv3: nothing is added to the patches (x + 0 keeps the bits) and CLS is the bare cls_token
            cls0 = self._cls[0, 0].to(self.device).contiguous()
            patch = torch.zeros((rows // self.patch_size) * (cols // self.patch_size), self.embed_dim, device=self.device)
            self._pos_cache[key] = (_lib.PosEmbed(cls0.data_ptr(), patch.data_ptr()), cls0, patch)
        if key not in self._pos_cache:
            pos = interpolate_pos_embed(self._pos, rows, cols, self.patch_size, antialias=self._pos_antialias)[0]      # (1 + n, D)
            cls0 = (self._cls[0, 0] + pos[0]).to(self.device).contiguous()
            patch = pos[1:].to(self.device).contiguous()
            self._pos_cache[key] = (_lib.PosEmbed(cls0.data_ptr(), patch.data_ptr()), cls0, patch)
        return self._pos_cache[key]

    def rope_for(self, rows, cols):
        """DINOv3: the device rotary table for a rows x cols image, (RopeTable struct, keep-alive tensors), computed once per
        image size in fp32 on the host (weights.rope_table); None for a model without rotary embedding."""
        if not self.rope:
            return None
        key = (rows, cols)
        if key not in self._rope_cache:
            cos, sin = (t.to(self.device).contiguous() for t in rope_table(rows // self.patch_size, cols // self.patch_size))
            self._rope_cache[key] = (_lib.RopeTable(cos.data_ptr(), sin.data_ptr(), cos.shape[0]), cos, sin)
        return self._rope_cache[key]

    def workspace(self, batch, tokens):
        """The engine's workspace for `batch` slices of `tokens` tokens (registers included; grown on demand, kept)."""
        need = self.lib.vittf_vit_workspace_bytes(C.byref(self.cfg), batch, tokens)
        if need == 0:
            raise _lib.VittfError('unsupported ViT configuration for the HIP engine')
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def tokens_for(self, view):
        """Token rows of one slice of `view`: CLS + the register tokens + the f0 x f1 patches."""
        p = self.patch_size
        return (view.out_rows // p) * (view.out_cols // p) + 1 + self.num_register_tokens

    def k_features(self, view, slice0, batch, out, part=1):
        """Run slices [slice0, slice0+batch) of `view` (a _lib.SliceView) through the ViT and write one facet of the patch
        tokens as fp16 into `out` (tensor of >= batch * f0*f1 * D halves).  `part`: 0 q, 1 k, 2 v -- that third of the hooked
        qkv tensor of block `self.layer` --, 3 t -- the final-norm patch tokens behind that block."""
        self.qkv_features(view, slice0, batch, {int(part): out})

    def qkv_features(self, view, slice0, batch, outs):
        """One forward of slices [slice0, slice0+batch) for several facets: `outs` maps a part (0 q, 1 k, 2 v, 3 t) to its
        output tensor, each written as k_features(part) writes it (same bits)."""
        tokens = self.tokens_for(view)
        npatch = tokens - 1 - self.num_register_tokens
        pos, _, _ = self.pos_for(view.out_rows, view.out_cols)
        ws = self.workspace(batch, tokens)
        ptrs = [None, None, None, None]
        for part, out in outs.items():
            if int(part) not in (0, 1, 2, 3):
                raise ValueError(f'part must be 0 (q), 1 (k), 2 (v) or 3 (t), got {part!r}')
            assert out.dtype == torch.float16 and out.is_contiguous() and \
                out.numel() >= batch * npatch * self.embed_dim
            ptrs[int(part)] = _lib.ptr(out)
        mask = sum(1 << int(part) for part in outs)
        if mask & 8 and self._norm_g is None:
            raise ValueError('the token facet needs the final LayerNorm: the state dict has no norm.weight / norm.bias')
        rope = self.rope_for(view.out_rows, view.out_cols)
        rc = self.lib.vittf_vit_features(C.byref(self.cfg), C.byref(self.weights), C.byref(pos), C.byref(view), slice0, batch,
                                         mask, _lib.ptr(self._reg), self.num_register_tokens,
                                         C.byref(rope[0]) if rope else None, _lib.ptr(self._norm_g), _lib.ptr(self._norm_b),
                                         *ptrs, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, 'vittf_vit_features')

    def __call__(self, *_a, **_k):
        raise _lib.VittfError('HipViT is driven through compute_qkv / FeatureExtractor, not called on image tensors')
