"""Weights of the DINO / DINOv2 ViT in the upstream state-dict layout: local loading, a seeded synthetic
recipe, and the host-side preprocessing the HIP engine needs (channel folding, LayerScale folding, position embedding).

The reference fetches the model over the network (``torch.hub.load('facebookresearch/dino:main',
'dino_vits8')``, infer.py:42-43).  Here weights come from a LOCAL state-dict file (same key names as the
DINO checkpoints: ``cls_token``, ``pos_embed``, ``patch_embed.proj.*``, ``blocks.{i}.norm1|attn.qkv|
attn.proj|norm2|mlp.fc1|mlp.fc2.*``, ``norm.*``) or from the seeded synthetic recipe below when no
checkpoint is available (benchmarks, tests).

DINOv2 (facebookresearch/dinov2, hub entries ``dinov2_vit{s,b,l,g}14``; upstream code is not vendored, these facts are
restated from it like SURVEY.md 8a row a5 restates DINO's): ``img_size=518, patch_size=14, init_values=1.0``,
``ffn_layer="mlp"`` (g14: ``"swiglufused"``), no register tokens, ``interpolate_offset=0.1`` with the same bicubic
scale-factor resize as DINO (stored grid 37 x 37).  Its block is ``x + ls1(attn(norm1(x)))``, ``x + ls2(mlp(norm2(x)))``
with ``ls(y) = y * gamma`` (one gamma per channel): the checkpoint holds the DINO keys plus ``blocks.{i}.ls1.gamma``,
``blocks.{i}.ls2.gamma`` and ``mask_token`` (unused at inference).

DINOv2 with registers (hub entries ``dinov2_vit{s,b,l}14_reg``, checkpoints ``dinov2_vit{s,b,l}14_reg4_pretrain.pth``; here
``vits14_reg``, ``vitb14_reg``, ``vitl14_reg``): the plain entries with ``num_register_tokens=4``, ``interpolate_offset=0.0``
and ``interpolate_antialias=True``.  The state dict gains ``register_tokens`` (1, 4, D); the token order is
``[CLS, reg_0 .. reg_3, patch_0 ..]``: the position embedding is added to CLS and the patches, the registers are inserted
afterwards and get none.  The stored grid is resized to the token grid by SIZE with antialiased bicubic interpolation
(``F.interpolate(size=(r0, c0), mode='bicubic', antialias=True)``), not by the scale factor with the 0.1 offset.  The
registers take part in the attention of every block and are dropped, with CLS, from the hooked q / k / v.  No ``_reg``
checkpoint has been run through this code yet (none was available): the tests use synthetic weights in that layout.
ViT-g/14 (with or without registers) is not built.

DINOv3 (``dinov3_vits16``, ``dinov3_vitb16``, ``dinov3_vitl16``; restated, nothing vendored; checked against
``transformers.models.dinov3_vit`` by tests/test_dinov3_cpu.py): patch 16, 4 register tokens behind CLS, LayerScale blocks
like DINOv2, LayerNorm eps 1e-5, q and v biases but NO key bias, and no additive position embedding -- the state dict has no
``pos_embed``.  Instead the q and k vectors of the patch tokens are rotated in every block (rotary position embedding, RoPE;
``rope_table`` below, csrc/rope.hip); CLS and the registers are not.  Two key layouts are read:

* the Hugging Face one (``embeddings.*``, ``layer.{i}.attention.{q,k,v,o}_proj``, ``mlp.up_proj / down_proj``,
  ``layer_scale{1,2}.lambda1``), converted by ``dinov3_from_hf``; checked against the real class;
* Meta's own ``.pth`` layout, UNCHECKED (no such file has been available; written from memory): the DINOv2 names with the
  registers as ``storage_tokens`` (1, 4, D), a full-width ``attn.qkv.bias`` whose k third is masked to zero at run time by the
  buffer ``blocks.{i}.attn.qkv.bias_mask``, the buffer ``rope_embed.periods``, and no ``pos_embed``.  The loader takes
  ``storage_tokens`` or ``register_tokens``, zeroes the k third of the bias whatever the file holds, and ignores
  ``mask_token``, ``rope_embed.*`` and ``*.bias_mask``.  The file names of those checkpoints carry hashes that could not be
  checked either, so HUB_FILES has no entry for them: weights come from ``--weights``, ``$VITTF_WEIGHTS`` or the synthetic recipe.

``vits16plus`` / ``vith16plus`` (gated SwiGLU MLP, D = 1280 for the latter) and ``vit7b16`` (D = 4096, head dim 128) are not built.
"""
import math
import os

import torch
import torch.nn.functional as F

# name: (embed_dim, depth, heads, patch)   -- hub entries dino_<name>
ARCHS = {
    'vits8': (384, 12, 6, 8),
    'vits16': (384, 12, 6, 16),
    'vitb8': (768, 12, 12, 8),
    'vitb16': (768, 12, 12, 16),
    # hub entries dinov2_<name> (LayerScale blocks; see the module docstring).  vitg14 (SwiGLU FFN, D = 1536) is not built.
    'vits14': (384, 12, 6, 14),
    'vitb14': (768, 12, 12, 14),
    'vitl14': (1024, 24, 16, 14),
    # hub entries dinov2_<name>: the same with register tokens (REGISTER_TOKENS) and the size-based antialiased position resize
    'vits14_reg': (384, 12, 6, 14),
    'vitb14_reg': (768, 12, 12, 14),
    'vitl14_reg': (1024, 24, 16, 14),
    # dinov3_<name>: patch 16, DINOV3_REGISTER_TOKENS registers, rotary position embedding, no pos_embed (module docstring).
    # The prefix keeps them apart from DINO's vits16 / vitb16.
    'dinov3_vits16': (384, 12, 6, 16),
    'dinov3_vitb16': (768, 12, 12, 16),
    'dinov3_vitl16': (1024, 24, 16, 16),
}
DINOV2_ARCHS = ('vits14', 'vitb14', 'vitl14', 'vits14_reg', 'vitb14_reg', 'vitl14_reg')
# name: register tokens behind CLS (the state dict's ``register_tokens`` is (1, R, D)); every other name has none
REGISTER_TOKENS = {'vits14_reg': 4, 'vitb14_reg': 4, 'vitl14_reg': 4}
DINOV3_ARCHS = ('dinov3_vits16', 'dinov3_vitb16', 'dinov3_vitl16')
DINOV3_REGISTER_TOKENS = 4              # every DINOv3 name
DINOV3_LN_EPS = 1e-5                    # DINO and DINOv2: 1e-6
ROPE_THETA = 100.0
MAX_REGISTER_TOKENS = 8                 # what the engine's *_reg entry points take (VITTF_MAX_REGISTER_TOKENS)
DINOV2_STORED_GRID = 37                 # 518 / 14
# file names torch.hub would have cached for these entries
HUB_FILES = {
    'vits8': 'dino_deitsmall8_pretrain.pth',
    'vits16': 'dino_deitsmall16_pretrain.pth',
    'vitb8': 'dino_vitbase8_pretrain.pth',
    'vitb16': 'dino_vitbase16_pretrain.pth',
    'vits14': 'dinov2_vits14_pretrain.pth',
    'vitb14': 'dinov2_vitb14_pretrain.pth',
    'vitl14': 'dinov2_vitl14_pretrain.pth',
    'vits14_reg': 'dinov2_vits14_reg4_pretrain.pth',
    'vitb14_reg': 'dinov2_vitb14_reg4_pretrain.pth',
    'vitl14_reg': 'dinov2_vitl14_reg4_pretrain.pth',
}
IN_MEAN = (0.485, 0.456, 0.406)   # infer.py:39
IN_STD = (0.229, 0.224, 0.225)    # infer.py:40


def arch_of(arch):
    if isinstance(arch, str):
        if arch not in ARCHS:
            raise ValueError(f'unknown DINO arch {arch!r}; known: {sorted(ARCHS)}')
        return ARCHS[arch]
    dim, depth, heads, patch = arch
    return int(dim), int(depth), int(heads), int(patch)


def register_tokens_of(arch, state_dict):
    """Number of register tokens R of a model: for a name, REGISTER_TOKENS (0 for the plain names), checked against the state
    dict's ``register_tokens`` key -- a checkpoint of the other family, or with another count, is refused; for an arch given
    as a (D, depth, heads, patch) tuple, read off that key (no key: 0)."""
    reg = state_dict.get('register_tokens')
    have = 0
    if reg is not None:
        if reg.ndim != 3 or reg.shape[0] != 1 or reg.shape[2] != arch_of(arch)[0]:
            raise ValueError(f'register_tokens has shape {tuple(reg.shape)}, expected (1, R, {arch_of(arch)[0]})')
        have = int(reg.shape[1])
    if isinstance(arch, str):
        want = DINOV3_REGISTER_TOKENS if arch in DINOV3_ARCHS else REGISTER_TOKENS.get(arch, 0)
        if have != want:
            raise ValueError(f'{arch} has {want} register tokens, the state dict has {have}'
                             + (' (no register_tokens key)' if reg is None else ''))
    if have > MAX_REGISTER_TOKENS:
        raise ValueError(f'{have} register tokens: the engine takes at most {MAX_REGISTER_TOKENS}')
    return have


def pos_embed_antialias_of(arch, state_dict):
    """Which position-embedding resize a model uses: True = the register models' size-based antialiased form
    (interpolate_offset 0.0, interpolate_antialias True), False = the scale-factor form with the 0.1 offset (DINO, plain
    DINOv2).  Upstream ties it to the hub entry; a tuple arch follows the presence of ``register_tokens``."""
    return register_tokens_of(arch, state_dict) > 0


def is_dinov3(arch, state_dict):
    """True for a DINOv3 model (rotary position embedding, eps 1e-5, no key bias): a DINOV3_ARCHS name, whose state dict must
    then have no ``pos_embed``; any other name must have one (a checkpoint of the other family is refused); an arch given as
    a tuple follows the absence of ``pos_embed``."""
    has_pos = 'pos_embed' in state_dict
    if isinstance(arch, str):
        v3 = arch in DINOV3_ARCHS
        if v3 and has_pos:
            raise ValueError(f'{arch} has no additive position embedding, the state dict has a pos_embed: not a DINOv3 checkpoint')
        if not v3 and not has_pos:
            raise ValueError(f'{arch} needs a pos_embed, the state dict has none (a DINOv3 checkpoint?)')
        return v3
    return not has_pos


def dinov3_canonical(sd):
    """A DINOv3 state dict (Meta-style or already canonical; Hugging Face files go through dinov3_from_hf first) as the engine
    reads it: the registers under ``register_tokens`` (from ``storage_tokens``), the k third of every ``attn.qkv.bias`` zeroed
    whatever the file holds (upstream masks it at run time), and without ``mask_token``, ``rope_embed.*`` and ``*.bias_mask``.
    Returns a new dict; the input tensors are not modified."""
    out = {}
    for k, v in sd.items():
        if k == 'mask_token' or k.startswith('rope_embed.') or k.endswith('.bias_mask'):
            continue
        if k == 'storage_tokens':
            k = 'register_tokens'
        if k.endswith('.attn.qkv.bias'):
            d = v.shape[0] // 3
            v = v.clone()
            v[d:2 * d] = 0
        out[k] = v
    return out


_HF_BLOCK = (('norm1.', 'norm1.'), ('norm2.', 'norm2.'), ('attention.o_proj.', 'attn.proj.'), ('mlp.up_proj.', 'mlp.fc1.'),
             ('mlp.down_proj.', 'mlp.fc2.'))


def is_dinov3_hf_layout(sd):
    return 'embeddings.patch_embeddings.weight' in sd and any(k.endswith('attention.q_proj.weight') for k in sd)


def dinov3_from_hf(sd):
    """The Hugging Face DINOv3ViTModel state dict in this project's canonical DINOv3 layout: ``q_proj / k_proj / v_proj``
    concatenated into ``blocks.{i}.attn.qkv`` with a zero k bias (the class has none), ``o_proj -> attn.proj``,
    ``up_proj / down_proj -> mlp.fc1 / fc2``, ``layer_scale{1,2}.lambda1 -> ls{1,2}.gamma``, ``embeddings.* -> cls_token /
    register_tokens / patch_embed.proj.*``, ``layer.{i} -> blocks.{i}`` (with or without the ``model.`` prefix the class puts
    in front of its encoder).  A gated MLP (``gate_proj``: the ``plus`` models) is refused."""
    sd = {(k[len('model.'):] if k.startswith('model.layer.') else k): v for k, v in sd.items()}
    if any('.mlp.gate_proj.' in k for k in sd):
        raise ValueError('gated (SwiGLU) MLP: the DINOv3 "plus" and 7B models are not supported')
    out = {'cls_token': sd['embeddings.cls_token'], 'register_tokens': sd['embeddings.register_tokens'],
           'patch_embed.proj.weight': sd['embeddings.patch_embeddings.weight'],
           'patch_embed.proj.bias': sd['embeddings.patch_embeddings.bias'],
           'norm.weight': sd['norm.weight'], 'norm.bias': sd['norm.bias']}
    i = 0
    while f'layer.{i}.attention.q_proj.weight' in sd:
        a, b = f'layer.{i}.', f'blocks.{i}.'
        wq = sd[a + 'attention.q_proj.weight']
        out[b + 'attn.qkv.weight'] = torch.cat([wq, sd[a + 'attention.k_proj.weight'], sd[a + 'attention.v_proj.weight']])
        zero = torch.zeros(wq.shape[0], dtype=wq.dtype)
        out[b + 'attn.qkv.bias'] = torch.cat([sd.get(a + 'attention.q_proj.bias', zero), zero,
                                              sd.get(a + 'attention.v_proj.bias', zero)])
        for theirs, ours in _HF_BLOCK:
            for p in ('weight', 'bias'):
                out[b + ours + p] = sd[a + theirs + p]
        out[b + 'ls1.gamma'] = sd[a + 'layer_scale1.lambda1']
        out[b + 'ls2.gamma'] = sd[a + 'layer_scale2.lambda1']
        i += 1
    if i == 0:
        raise ValueError('no layer.{i}.attention.q_proj.weight key: not a Hugging Face DINOv3 state dict')
    return out


def rope_table(f0, f1):
    """(cos, sin), each fp32 [f0 * f1][32]: DINOv3's rotary table for an f0 x f1 patch grid, head dim 64 -- the 32 distinct
    angles of a patch (columns j and j + 32 of a head share angle j).  fp32 and this order of operations throughout: the table
    is then bit-equal to transformers' DINOv3ViTRopePositionEmbedding (first 32 columns; tests/test_dinov3_cpu.py), while
    ``theta ** -(i / 16)`` for inv_freq is already 1 ulp off.  Depends on the grid only: computed once per image size."""
    inv_freq = 1 / ROPE_THETA ** torch.arange(0, 1, 1 / 16, dtype=torch.float32)                 # 16 values
    cy = 2.0 * (torch.arange(0.5, f0, dtype=torch.float32) / f0) - 1.0
    cx = 2.0 * (torch.arange(0.5, f1, dtype=torch.float32) / f1) - 1.0
    coords = torch.stack(torch.meshgrid(cy, cx, indexing='ij'), dim=-1).flatten(0, 1)           # (f0 f1, 2): (y, x)
    angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2)        # (f0 f1, 32)
    return torch.cos(angles).contiguous(), torch.sin(angles).contiguous()


# "massive activation" channels of the outlier variant below (trained ViTs carry a handful of residual-stream channels two
# orders of magnitude above the rest; Gaussian unit-gain weights have none)
OUTLIER_CHANNELS = (7, 100, 191, 250, 333, 380)


def synthetic_state_dict(arch='vits8', seed=0, stored_grid=None, outliers=False, layer_scale=None, dinov3=None):
    """Seeded random weights with the DINO key layout.

    stored_grid: side of the stored position-embedding grid (default 28, 37 for the DINOv2 names).
    layer_scale: add the DINOv2 keys -- ``blocks.{i}.ls1.gamma`` / ``ls2.gamma``, log-uniform over [1e-5, 1] so that tiny
    gammas are exercised, and ``mask_token`` (default: True for the DINOv2 names only).  They are drawn from a generator of
    their own, after every DINO tensor, so the DINO tensors of a seed do not depend on this flag.  The ``_reg`` names add
    ``register_tokens`` (1, R, D), std 0.5, from a third generator after all of those: ``vits14_reg`` and ``vits14`` of one
    seed agree on every shared key.

    dinov3 (default: True for the DINOV3_ARCHS names only; pass True with a tuple arch): Meta's DINOv3 key layout as far as it
    is known (module docstring) -- the DINO tensors of the seed without ``pos_embed``, the LayerScale keys, the registers as
    ``storage_tokens`` (1, 4, D) from the register generator, ``rope_embed.periods``, and per block a ``attn.qkv.bias_mask``
    (1 / 0 / 1 over the thirds) beside a bias whose k third is NOT zero: a loader that forgets the mask gives other features.

    outliers=True: the same weights with six massive channels planted -- x50 rows in two blocks' mlp.fc2 and one block's
    attn.proj (the residual stream then carries them to the end), x50 entries in several norm weights (16-bit LayerNorm
    output in the hundreds), and in one block a q / k pair of one head that both read the same massive direction, so that
    its attention logits spread over more than +-60: what the parity tests on benign weights never drive through the 16-bit
    operand path (LN -> h, GELU -> hidden, the lazy-maximum attention kernel's overflow branch).

    Not an initialisation for training: the scales are chosen so that a forward pass looks like a trained
    ViT numerically (unit-gain linears, attention logits with a std of a few units so the softmax is
    peaked, non-trivial biases and LayerNorm affine terms) -- this keeps parity tests sensitive to
    ordering / bias / masking mistakes and gives realistic data for benchmarking.
    """
    dim, depth, heads, patch = arch_of(arch)
    dinov2 = isinstance(arch, str) and arch in DINOV2_ARCHS
    if dinov3 is None:
        dinov3 = isinstance(arch, str) and arch in DINOV3_ARCHS
    if layer_scale is None and dinov3:
        layer_scale = True
    if stored_grid is None:
        stored_grid = DINOV2_STORED_GRID if dinov2 else 28
    if layer_scale is None:
        layer_scale = dinov2
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    sd = {
        'cls_token': rnd(1, 1, dim, std=0.5),
        'pos_embed': rnd(1, stored_grid * stored_grid + 1, dim, std=0.5),
        'patch_embed.proj.weight': rnd(dim, 3, patch, patch, std=1.0 / math.sqrt(3 * patch * patch) * 3.0),
        'patch_embed.proj.bias': rnd(dim, std=0.1),
        'norm.weight': 1.0 + rnd(dim, std=0.1),
        'norm.bias': rnd(dim, std=0.1),
    }
    for i in range(depth):
        p = f'blocks.{i}.'
        sd[p + 'norm1.weight'] = 1.0 + rnd(dim, std=0.1)
        sd[p + 'norm1.bias'] = rnd(dim, std=0.1)
        sd[p + 'attn.qkv.weight'] = rnd(3 * dim, dim, std=1.3 / math.sqrt(dim))
        sd[p + 'attn.qkv.bias'] = rnd(3 * dim, std=0.1)
        sd[p + 'attn.proj.weight'] = rnd(dim, dim, std=1.0 / math.sqrt(dim))
        sd[p + 'attn.proj.bias'] = rnd(dim, std=0.1)
        sd[p + 'norm2.weight'] = 1.0 + rnd(dim, std=0.1)
        sd[p + 'norm2.bias'] = rnd(dim, std=0.1)
        sd[p + 'mlp.fc1.weight'] = rnd(4 * dim, dim, std=1.0 / math.sqrt(dim))
        sd[p + 'mlp.fc1.bias'] = rnd(4 * dim, std=0.1)
        sd[p + 'mlp.fc2.weight'] = rnd(dim, 4 * dim, std=1.0 / math.sqrt(4 * dim))
        sd[p + 'mlp.fc2.bias'] = rnd(dim, std=0.1)
    if outliers:
        c = [ch % dim for ch in OUTLIER_CHANNELS]
        for blk in (1, depth // 2):
            sd[f'blocks.{blk}.mlp.fc2.weight'][c[0]] *= 50.0
            sd[f'blocks.{blk}.mlp.fc2.weight'][c[1]] *= 50.0
        sd[f'blocks.{2 % depth}.attn.proj.weight'][c[2]] *= 50.0
        for blk in range(depth):
            sd[f'blocks.{blk}.norm1.weight'][c[3]] *= 50.0 if blk % 3 == 0 else 1.0
            sd[f'blocks.{blk}.norm2.weight'][c[4]] *= 50.0 if blk % 3 == 1 else 1.0
        # one head whose q and k both follow the (massive) channel c[0] of the normalised input: logits = 64 a^2 h_q h_k / 8
        # (all of one sign there: logits up to ~140 but a spread of only ~10 inside a row), and one head that follows a
        # channel whose sign changes with the token's position (its position embedding is x 20): logits of both signs (+-60)
        # inside one row, i.e. keys far above the first key tile's maximum late in the sequence
        sd['pos_embed'][0, :, c[5]] *= 20.0
        blk = min(depth - 2, 6)
        wq = sd[f'blocks.{blk}.attn.qkv.weight']
        for head, ch, a in ((1 % heads, c[0], 0.5), (2 % heads, c[5], 0.5)):
            wq[head * 64:(head + 1) * 64, ch] += a
            wq[dim + head * 64:dim + (head + 1) * 64, ch] += a
    if layer_scale:
        g2 = torch.Generator().manual_seed(0x15ca1e + seed)
        sd['mask_token'] = torch.randn(1, dim, generator=g2) * 0.5
        for i in range(depth):
            for ls in ('ls1', 'ls2'):
                sd[f'blocks.{i}.{ls}.gamma'] = 10.0 ** (torch.rand(dim, generator=g2) * -5.0)
    n_reg = REGISTER_TOKENS.get(arch, 0) if isinstance(arch, str) else 0
    if dinov3:
        n_reg = DINOV3_REGISTER_TOKENS
    if n_reg:
        g3 = torch.Generator().manual_seed(0x4e6157 + seed)
        sd['storage_tokens' if dinov3 else 'register_tokens'] = torch.randn(1, n_reg, dim, generator=g3) * 0.5
    if dinov3:
        del sd['pos_embed']
        sd['rope_embed.periods'] = ROPE_THETA ** torch.arange(0, 1, 1 / 16, dtype=torch.float32)
        mask = torch.ones(3 * dim)
        mask[dim:2 * dim] = 0
        for i in range(depth):
            sd[f'blocks.{i}.attn.qkv.bias_mask'] = mask.clone()
    return sd


def fold_layer_scale(sd):
    """DINOv2 LayerScale folded into the linear in front of it: ``ls1(proj(y)) = (diag(g) W) y + g * b`` for attn.proj,
    the same with ls2 for mlp.fc2.  fp32, on the host, before the engine's one conversion of the weights to 16 bits (exact
    in real arithmetic; DESIGN.md section 5 bounds what the fp16 weights lose).  Returns a new dict without the ``ls*``
    keys; a dict without them is returned unchanged (the same tensors)."""
    if not any(k.endswith(('.ls1.gamma', '.ls2.gamma')) for k in sd):
        return sd
    out = {k: v for k, v in sd.items() if not k.endswith(('.ls1.gamma', '.ls2.gamma'))}
    i = 0
    while f'blocks.{i}.attn.proj.weight' in sd:
        for ls, lin in (('ls1', 'attn.proj'), ('ls2', 'mlp.fc2')):
            key = f'blocks.{i}.{ls}.gamma'
            if key in sd:
                gamma = sd[key].float()
                out[f'blocks.{i}.{lin}.weight'] = sd[f'blocks.{i}.{lin}.weight'].float() * gamma[:, None]
                out[f'blocks.{i}.{lin}.bias'] = sd[f'blocks.{i}.{lin}.bias'].float() * gamma
        i += 1
    return out


def load_state_dict_file(path):
    """Load a DINO / DINOv2 / DINOv3 checkpoint from a local file; accepts bare backbones and teacher/student wrappers.  A
    ``.safetensors`` file is read with the ``safetensors`` module (absent: a message and exit code 1).  The Hugging Face DINOv3
    layout is recognised by its keys and converted (dinov3_from_hf)."""
    if str(path).endswith('.safetensors'):
        try:
            from safetensors.torch import load_file
        except ImportError:
            print(f'{path}: reading .safetensors needs the safetensors module, which is not installed. '
                  'Convert the file to a torch state dict (.pth) or install safetensors.')
            raise SystemExit(1)
        sd = load_file(str(path), device='cpu')
    else:
        sd = torch.load(path, map_location='cpu', weights_only=True)
    for key in ('teacher', 'student', 'state_dict', 'model'):
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
            sd = sd[key]
            break
    out = {}
    for k, v in sd.items():
        for prefix in ('module.', 'backbone.'):
            if k.startswith(prefix):
                k = k[len(prefix):]
        if k.startswith('head.'):
            continue
        out[k] = v.float()
    if is_dinov3_hf_layout(out):
        out = dinov3_from_hf(out)
    return out


def find_local_checkpoint(name):
    """Where a previously downloaded hub checkpoint would be; None if absent.  Never touches the network."""
    env = os.environ.get('VITTF_WEIGHTS')
    if env:
        return env if os.path.exists(env) else None
    hub = os.environ.get('TORCH_HOME', os.path.join(os.path.expanduser('~'), '.cache', 'torch'))
    cand = os.path.join(hub, 'hub', 'checkpoints', HUB_FILES.get(name, ''))
    return cand if os.path.isfile(cand) else None


def state_dict_checksum(sd):
    """Order-independent float64 checksum used by golden fixtures to detect generator drift."""
    tot = 0.0
    for k in sorted(sd):
        t = sd[k].double()
        tot += float((t * torch.arange(1, t.numel() + 1, dtype=torch.float64).reshape(t.shape).remainder(7.0)).sum())
    return tot


def fold_patch_embed(weight, bias):
    """Fold the 3-channel conv applied to a grey image replicated over 3 ImageNet-normalised channels
    into a single-channel conv acting on the [0, 1] grey value:

        sum_c W[d,c,i,j] * (x - mean_c) / std_c + b[d]
      = sum_ij (sum_c W[d,c,i,j] / std_c) * x_ij + (b[d] - sum_c mean_c / std_c * sum_ij W[d,c,i,j])

    (infer.py:39-40, 154-155 + upstream PatchEmbed).  Returns (w_t [P*P][D], b [D]) fp32, folded in fp64.  DINOv2's
    PatchEmbed is the same conv with P = 14.
    """
    w = weight.double()
    mean = torch.tensor(IN_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(IN_STD, dtype=torch.float64).view(1, 3, 1, 1)
    w1 = (w / std).sum(1)                                  # (D, P, P)
    b1 = bias.double() - (w * mean / std).sum((1, 2, 3))
    d = w.shape[0]
    return w1.reshape(d, -1).t().contiguous().float(), b1.float()


def interpolate_pos_embed(pos_embed, rows, cols, patch, antialias=False):
    """Position embedding for a rows x cols pixel image, upstream form: bicubic,
    ``scale_factor=((r0 + 0.1) / sqrt(N), (c0 + 0.1) / sqrt(N))``; identity for the stored square grid.
    antialias=True: the DINOv2 register models' form instead (interpolate_offset 0.0, interpolate_antialias True) --
    ``size=(r0, c0)``, bicubic with antialias; the caller chooses by the model (pos_embed_antialias_of).
    Runs once per image size on the host (it depends on the weights only).  Returns (1, 1 + r0*c0, D)."""
    n_stored = pos_embed.shape[1] - 1
    r0, c0 = rows // patch, cols // patch
    if r0 * c0 == n_stored and rows == cols:
        return pos_embed
    dim = pos_embed.shape[-1]
    g = int(math.sqrt(n_stored))
    grid = pos_embed[:, 1:].reshape(1, g, g, dim).permute(0, 3, 1, 2)
    if antialias:
        grid = F.interpolate(grid.float(), size=(r0, c0), mode='bicubic', antialias=True)
    else:
        grid = F.interpolate(grid.float(), scale_factor=((r0 + 0.1) / math.sqrt(n_stored), (c0 + 0.1) / math.sqrt(n_stored)),
                             mode='bicubic')
    if grid.shape[-2] != r0 or grid.shape[-1] != c0:
        raise ValueError(f'position-embedding grid {tuple(grid.shape[-2:])} != token grid {(r0, c0)}')
    grid = grid.permute(0, 2, 3, 1).reshape(1, -1, dim)
    return torch.cat((pos_embed[:, :1].float(), grid), dim=1)


FC2_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def _tile_pos_tables():
    """(row, chunk) held by each of the 256 16-byte positions of a [32 rows][64 x 16-bit] sub-image in the kernels' tile_off
    layout (vittf_common.h: tile_pos)."""
    q = torch.arange(256)
    p = q >> 4
    slot = (q & 15) ^ (p & 15)
    return (p << 1) | (slot >> 3), slot & 7


def _pack_row_images(w):
    """[L, 32 U, 384] -> [L, U, 12288]: image u = rows 32 u .. + 31 over the 384 inputs as 6 sub-images [32 rows][64 k] in LDS
    layout: element (s6, q, e) = w[32 u + r[q], 64 s6 + 8 c[q] + e]."""
    L, n, d = w.shape
    assert d == 384 and n % 32 == 0
    units, dev = n // 32, w.device
    r, c = (t.to(dev) for t in _tile_pos_tables())
    e = torch.arange(8, device=dev)
    s6 = torch.arange(6, device=dev)
    rows = torch.arange(units, device=dev).view(-1, 1, 1, 1) * 32 + r.view(1, 1, -1, 1)                # [U, 1, 256, 1]
    cols = (64 * s6.view(1, -1, 1, 1) + 8 * c.view(1, 1, -1, 1) + e.view(1, 1, 1, -1))                  # [1, 6, 256, 8]
    return w[:, rows.expand(units, 6, 256, 8), cols.expand(units, 6, 256, 8)].reshape(L, units, -1)


def pack_row_images(w):
    """A K = 384 weight [L, N, 384] (N a multiple of 32) as the stream of 24 KB LDS images of vittf_gemm_as (csrc/gemm_as.hip):
    image u = rows 32 u .. + 31, natural k order -> [L, N / 32, 12288]."""
    return _pack_row_images(w).contiguous()


def norm2_register_order():
    """Column of x held at fc1 input position 16 s + 8 h + e when norm2 is computed in the block-tail kernel's accumulator
    registers (csrc/tail_fx.hip): 32 (s >> 1) + 16 (s & 1) + 8 (e >> 2) + 4 h + (e & 3)."""
    p = torch.arange(384)
    s_, h, e = p >> 4, (p >> 3) & 1, p & 7
    return 32 * (s_ >> 1) + 16 * (s_ & 1) + 8 * (e >> 2) + 4 * h + (e & 3)


def _mlp_images(w1, w2):
    """fc1 / fc2 weights of L blocks as 24 KB LDS images, one per hidden unit of 32: (img1, img2), each [L, 48, 12288].
      W1(u): rows = hidden units 32 u .. + 31, k = the 384 inputs: 6 sub-images [32 rows][64 k] (tile_off layout).
      W2(u): rows = outputs; sub-image s6 holds output tiles 2 s6 and 2 s6 + 1, 32 k each = hidden units 32 u .. + 31 in the
             order the second MFMA finds them in the first one's accumulator registers (permute_fc2_hidden)."""
    L, hid, d = w1.shape
    assert d == 384 and hid == 4 * d and tuple(w2.shape) == (L, d, hid)
    units = hid // 32
    dev = w1.device
    r, c = (t.to(dev) for t in _tile_pos_tables())                      # [256]
    e = torch.arange(8, device=dev)
    s6 = torch.arange(6, device=dev)
    img1 = _pack_row_images(w1)
    # W2(u): element (s6, q, e) = w2p[32 (2 s6 + (c >> 2)) + r, 32 u + 16 ((c >> 1) & 1) + 8 (c & 1) + e]
    w2p = permute_fc2_hidden(w2)
    rows2 = (32 * (2 * s6.view(1, -1, 1, 1) + (c.view(1, 1, -1, 1) >> 2)) + r.view(1, 1, -1, 1))       # [1, 6, 256, 1]
    cols2 = (32 * torch.arange(units, device=dev).view(-1, 1, 1, 1) + 16 * ((c.view(1, 1, -1, 1) >> 1) & 1)
             + 8 * (c.view(1, 1, -1, 1) & 1) + e.view(1, 1, 1, -1))                                     # [U, 1, 256, 8]
    img2 = w2p[:, rows2.expand(units, 6, 256, 8), cols2.expand(units, 6, 256, 8)].reshape(L, units, -1)
    return img1, img2


TAIL_FX_PSTEPS, TAIL_FX_MSTEPS, TAIL_FX_LAG = 12, 100, 4


def _pack_proj_kmajor(wp):
    """[L, 384, 384] -> [L, 12, 12288]: projection step p = k steps 2 p, 2 p + 1 of all 12 output tiles: fragment f (0 .. 23; the
    kernel reads it at sub-image f >> 2, chunk pair f & 3) = Wp[32 (f % 12) + r][16 (2 p + f // 12) + 8 h + e]."""
    L, n, d = wp.shape
    assert n == 384 and d == 384
    dev = wp.device
    r, c = (t.to(dev) for t in _tile_pos_tables())
    e = torch.arange(8, device=dev).view(1, 1, 1, -1)
    s6 = torch.arange(6, device=dev).view(1, -1, 1, 1)
    p = torch.arange(12, device=dev).view(-1, 1, 1, 1)
    f = 4 * s6 + (c.view(1, 1, -1, 1) >> 1)                                 # [1, 6, 256, 1]
    rows = 32 * (f % 12) + r.view(1, 1, -1, 1)
    cols = 16 * (2 * p + f // 12) + 8 * (c.view(1, 1, -1, 1) & 1) + e        # [12, 6, 256, 8]
    return wp[:, rows.expand(12, 6, 256, 8), cols.expand(12, 6, 256, 8)].reshape(L, 12, -1)


def pack_block_tail_weights(wp, w1, w2):
    """proj / fc1 / fc2 weights of L blocks -> the stream of the block-tail kernel (vittf_block_tail, csrc/tail_fx.hip): per block
    12 projection steps of 24 KB (k steps 2 p, 2 p + 1 of all output tiles, K-major: _pack_proj_kmajor), then 100 main steps =
    [ W1(m >> 1) k half m & 1 | W2((m - 4) >> 1) output-tile half (m - 4) & 1 ] (zeros where a role has no work: the first four
    W2 halves, the last four W1 halves); fc1's input dim in the order norm2 leaves its values in the registers.
    -> [L, 112, 12288]."""
    L, d, d2 = wp.shape
    assert d == 384 and d2 == 384
    order = norm2_register_order().to(w1.device)
    img1, img2 = _mlp_images(w1[:, :, order], w2)
    half = img1.shape[-1] // 2
    zero = torch.zeros_like(img1[:, 0, :half])
    steps = []
    for m in range(TAIL_FX_MSTEPS):
        a = img1[:, m >> 1, (m & 1) * half:(m & 1) * half + half] if m < 96 else zero
        m2 = m - TAIL_FX_LAG
        b = img2[:, m2 >> 1, (m2 & 1) * half:(m2 & 1) * half + half] if m2 >= 0 else zero
        steps.append(torch.cat([a, b], dim=-1))
    return torch.cat([_pack_proj_kmajor(wp), torch.stack(steps, dim=1)], dim=1).contiguous()


def permute_fc2_hidden(w2):
    """fc2 weight [..., D, 4D] with its hidden (input) dim re-ordered inside every block of 16: the k order in which
    the fused MLP kernel's second MFMA consumes the first one's accumulator registers (include/vittf.h, fc2_w_perm)."""
    hid = w2.shape[-1]
    idx = (torch.arange(hid).view(-1, 16)[:, list(FC2_PERM16)]).reshape(-1)
    return w2[..., idx].contiguous()
