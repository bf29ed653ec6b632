/* vittf.h -- C ABI of the MI355X-native vit-tf hot path (libvittf.so, gfx950 only).
 *
 * The reference (xeTaiz/vit-tf) has no FFI: its hot path is Python calling stock PyTorch ops.
 * This header is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): every
 * entry point names the reference lines whose arithmetic it replaces.  Conventions:
 *
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host]
 *   - the caller owns all memory; nothing is allocated inside (workspace passed in, size from the
 *     matching *_workspace_bytes query); no host synchronisation inside any call
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work of a call is
 *     enqueued on it in order, so calls compose without further synchronisation
 *   - return value: 0 (VITTF_OK) or a negative vittf_status; no exceptions cross the ABI
 *   - "h16" = the 16-bit arithmetic type selected by vittf_dtype (bf16 or fp16); feature volumes
 *     and K features are always IEEE fp16 like the reference's files (infer.py:134, 337-340)
 *   - thread-compatible: no global mutable state
 */
#ifndef VITTF_H
#define VITTF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITTF_ABI_VERSION 6

typedef enum vittf_status {
  VITTF_OK = 0,
  VITTF_ERR_INVALID_ARG = -1,   /* bad shape / null pointer / unsupported configuration */
  VITTF_ERR_WORKSPACE = -2,     /* workspace too small */
  VITTF_ERR_LAUNCH = -3,        /* HIP launch error (hipGetLastError != hipSuccess) */
  VITTF_ERR_NO_DEVICE = -4      /* no gfx950 device visible */
} vittf_status;

typedef enum vittf_dtype { VITTF_BF16 = 0, VITTF_FP16 = 1 } vittf_dtype;

/* slice axis, naming of infer.py:138-152 ('z' slices along the last volume dim) */
typedef enum vittf_axis { VITTF_AXIS_X = 0, VITTF_AXIS_Y = 1, VITTF_AXIS_Z = 2 } vittf_axis;

typedef enum vittf_sample_mode { VITTF_SAMPLE_NEAREST = 0, VITTF_SAMPLE_TRILINEAR = 1 } vittf_sample_mode;

int vittf_abi_version(void);
const char* vittf_status_string(int status);
/* number of visible gfx950 devices (<= 0: none).  Does not create a context on failure. */
int vittf_device_count(void);

/* ------------------------------------------------------------------------------------------
 * ViT description.  Replaces the module tree of the upstream DINO VisionTransformer that the
 * reference fetches with torch.hub (infer.py:42-43, 323).  Head dim must be 64 (all DINO ViTs),
 * embed_dim a multiple of 128, patch 8, 14 or 16.
 * ---------------------------------------------------------------------------------------- */
typedef struct vittf_vit_config {
  int32_t embed_dim;   /* D: 384 (ViT-S) / 768 (ViT-B) */
  int32_t depth;       /* L: 12 */
  int32_t heads;       /* D / 64 */
  int32_t patch;       /* P: 8, 14 (DINOv2) or 16 */
  int32_t dtype;       /* vittf_dtype of the MFMA operands */
  float   ln_eps;      /* 1e-6 (DINO, DINOv2), 1e-5 (DINOv3) */
  int32_t attention_fp8; /* 0: 16-bit attention (default).  1: the fp8 (e4m3) block-scaled MFMA attention path of BASELINE
                            configs[3] (vittf_attention_fp8): 3-mantissa-bit operands, ~3e-2 on the features -- opt-in */
  int32_t flags;       /* 0 = the measured path.  Bits select the slower alternatives the parity tests also run (ABI 6: they
                            were environment variables latched inside the library before -- the library reads no environment
                            on this path any more): */
} vittf_vit_config;
enum {
  VITTF_CFG_SEPARATE_LN = 1,       /* every LayerNorm as its own launch instead of riding on the kernel in front of it */
  VITTF_CFG_UNSCALED_Q = 2,        /* q as the model produces it + the online-maximum attention kernel (vittf_attention(.., 0)) */
  VITTF_CFG_FP8_HEAD_SCALES = 4    /* fp8 attention with one scale per (slice, head) (absmax + quantise launches) instead of row scales */
};
#define VITTF_MAX_REGISTER_TOKENS 8 /* most register tokens (DINOv2 _reg models carry 4) the *_reg entry points take */
#define VITTF_TAIL_STEPS 112       /* 24 KB steps of one block in vittf_vit_weights.tail_packed */

/* All weights live in HBM for the lifetime of the engine (about 43 MB for ViT-S).  Per-layer tensors
 * are stacked along a leading L dimension.  "h16" matrices are row-major [out][in] exactly like the
 * nn.Linear weights of the DINO state dict, converted once to the engine dtype. */
typedef struct vittf_vit_weights {
  const float* pe_w_t;   /* [P*P][D]  patch-embed conv folded to ONE input channel, transposed (k-major);
                            folding of the 3 identical grey channels + ImageNet mean/std: infer.py:39-40,154-155 */
  const float* pe_b;     /* [D]       folded bias */
  const void*  qkv_w;    /* h16 [L][3D][D]   blocks.i.attn.qkv.weight */
  const float* qkv_b;    /* [L][3D] */
  const void*  proj_w;   /* h16 [L][D][D]    blocks.i.attn.proj.weight */
  const float* proj_b;   /* [L][D] */
  const void*  fc1_w;    /* h16 [L][4D][D]   blocks.i.mlp.fc1.weight */
  const float* fc1_b;    /* [L][4D] */
  const void*  fc2_w;    /* h16 [L][D][4D]   blocks.i.mlp.fc2.weight */
  const float* fc2_b;    /* [L][D] */
  const void*  tail_packed; /* h16 [L][112][12288] or NULL: proj_w, fc1_w and fc2_w of every block as the weight stream of the
                            block-tail kernel (vittf_block_tail; packing: vit-tf_amd/weights.py pack_block_tail_weights); when
                            non-NULL and D == 384 the engine runs everything behind the attention of a block -- proj, residual,
                            norm2, MLP, residual, the next block's norm1 -- as one launch */
  const void*  qkv_packed; /* h16 [L][3D/32][12288] or NULL: qkv_w as the 24 KB LDS images of vittf_gemm_as (weights.py
                            pack_row_images); when non-NULL and D == 384 the qkv projection runs on the activation-stationary kernel */
  const float* ln1_g;    /* [L][D] */
  const float* ln1_b;    /* [L][D] */
  const float* ln2_g;    /* [L][D] */
  const float* ln2_b;    /* [L][D] */
} vittf_vit_weights;

/* Position embedding for ONE image size, already interpolated on the host in the upstream
 * scale-factor/bicubic form: row 0 = cls_token + pos[0], rows 1.. = patch part. */
typedef struct vittf_pos_embed {
  const float* cls_plus_pos0;  /* [D] */
  const float* patch_pos;      /* [f0*f1][D] */
} vittf_pos_embed;

/* Where the slices of one axis sit inside the resident fp32 volume (W, H, D), C-contiguous.
 * Replaces make_4d(vol).permute(permute_in) (infer.py:138-142, 154) without materialising it. */
typedef struct vittf_slice_view {
  const float* vol;        /* fp32 volume in HBM */
  int64_t stride_slice;    /* element strides of the (slice, row, col) view */
  int64_t stride_row;
  int64_t stride_col;
  int32_t in_rows;         /* slice size in volume voxels */
  int32_t in_cols;
  int32_t out_rows;        /* network input size (im_sz of the axis, multiple of P), nearest-resized: */
  int32_t out_cols;        /*   src = min(floor(dst * in/out), in-1), F.interpolate 'nearest' infer.py:177 */
  const float* minmax;     /* [2] device: global min, max of the volume (norm_minmax infer.py:32-34) */
} vittf_slice_view;

/* min / max of n floats -> out[2] (device).  ws: >= vittf_minmax_workspace_bytes() bytes.
 * Replaces t.min(), t.max() of norm_minmax (infer.py:33). */
size_t vittf_minmax_workspace_bytes(void);
int vittf_volume_minmax(const float* vol, int64_t n, float* out_minmax, void* ws, size_t ws_bytes, void* stream);

/* Bytes of workspace for a forward over `batch` slices of `tokens` = f0*f1 + 1 tokens (+ n_reg for vittf_vit_qkv_features_reg). */
size_t vittf_vit_workspace_bytes(const vittf_vit_config* cfg, int32_t batch, int32_t tokens);

/* The ViT leg of compute_qkv (infer.py:173-177 + the hooked K third, infer.py:133-135, 189-203):
 * for slices [slice0, slice0 + batch) of `view`: normalise, nearest-resize, patch-embed, (L-1) full
 * blocks, then ONLY LayerNorm1 + the K projection of block L; the K features of the patch tokens
 * (CLS dropped, infer.py:202) are rounded to fp16 (infer.py:134) and written token-major:
 *     k_out[(s - slice0) * f0*f1 + token][D]      token = row-major over the (rows/P, cols/P) grid
 * qkv_part selects the third of the hooked qkv tensor: 0 = q, 1 = k (what infer.py's __main__ asks for,
 * infer.py:326,331), 2 = v  (compute_qkv's return_keys, infer.py:195-209).
 * [host] cfg, w, pos, view are host structs holding device pointers. */
int vittf_vit_k_features(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                         const vittf_slice_view* view, int32_t slice0, int32_t batch, int32_t qkv_part,
                         uint16_t* k_out, void* ws, size_t ws_bytes, void* stream);

/* Several thirds of the hooked qkv tensor from ONE forward (compute_qkv's return_keys=['q','k','v'], infer.py:133-135,
 * 189-209): the forward of vittf_vit_k_features, then one projection launch for every third whose bit is set in part_mask
 * (bit 0 = q, 1 = k, 2 = v).  Each output has vittf_vit_k_features' layout, bits, argument checks, workspace and batch
 * limit; vittf_vit_k_features(part) is this call with part_mask = 1 << part.  The pointer of an unset bit is ignored (may
 * be NULL); a NULL pointer for a set bit, part_mask 0 or above 7: VITTF_ERR_INVALID_ARG.
 * [host] cfg, w, pos, view are host structs holding device pointers. */
int vittf_vit_qkv_features(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                           const vittf_slice_view* view, int32_t slice0, int32_t batch, int32_t part_mask,
                           uint16_t* q_out, uint16_t* k_out, uint16_t* v_out, void* ws, size_t ws_bytes, void* stream);

/* vittf_vit_qkv_features for a model with n_reg register tokens (DINOv2 dinov2_vit{s,b,l}14_reg: 4; 0 .. VITTF_MAX_REGISTER_TOKENS):
 * the token rows of a slice are [CLS, reg_0 .. reg_{n_reg-1}, patch_0 ..], tokens = f0*f1 + 1 + n_reg (the workspace query
 * takes that number).  reg_rows: fp32 [n_reg][D], the checkpoint's register_tokens; they get no position embedding, take part
 * in the attention of every block and are dropped together with CLS: the outputs keep vittf_vit_k_features' layout, f0*f1 rows
 * per slice.  The 32-bit offset limit applies to batch * tokens.  n_reg = 0 (reg_rows ignored) is vittf_vit_qkv_features, bit
 * for bit.  [host] cfg, w, pos, view are host structs holding device pointers. */
int vittf_vit_qkv_features_reg(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                               const vittf_slice_view* view, int32_t slice0, int32_t batch, int32_t part_mask,
                               const float* reg_rows, int32_t n_reg, uint16_t* q_out, uint16_t* k_out, uint16_t* v_out,
                               void* ws, size_t ws_bytes, void* stream);

/* Rotary position embedding of DINOv3 for ONE image size: cos and sin of the 32 distinct angles of every patch token, fp32
 * [patches = f0*f1][32], row-major over the patch grid.  Built on the host (vit-tf_amd/weights.py rope_table): with
 * inv_freq[i] = 1 / 100^(i/16), cy = 2 (r + 0.5) / f0 - 1, cx = 2 (c + 0.5) / f1 - 1: angle[0:16] = 2 pi cy inv_freq,
 * angle[16:32] = 2 pi cx inv_freq; columns j and j + 32 of a head of 64 share angle[j]. */
typedef struct vittf_rope_table {
  const float* cos;      /* [patches][32] */
  const float* sin;      /* [patches][32] */
  int32_t patches;       /* f0*f1 */
} vittf_rope_table;

/* vittf_vit_qkv_features_reg for a model with rotary position embedding (DINOv3 dinov3_vit{s,b,l}16): with a table, the q and
 * k thirds of the patch tokens are rotated (vittf_rope_qk, prefix = 1 + n_reg) behind the qkv projection of every full block,
 * on every qkv path and with VITTF_CFG_UNSCALED_Q; the hooked tensor of the last block is taken BEFORE the rotation, as the
 * hook on blocks[-1].attn.qkv sees it.  The rotated q and k are rounded to h16 a second time (the projection's epilogue has
 * rounded them once).  table->patches must be f0*f1.  cfg->attention_fp8 together with a table: VITTF_ERR_INVALID_ARG -- that
 * path quantises q and k to fp8 inside the GEMM epilogue, before a rotation could happen.  Such a model has no additive
 * position embedding: pass a zero pos->patch_pos and pos->cls_plus_pos0 = cls_token.  table == NULL is
 * vittf_vit_qkv_features_reg, bit for bit.  [host] cfg, w, pos, view, table are host structs holding device pointers. */
int vittf_vit_qkv_features_rope(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                                const vittf_slice_view* view, int32_t slice0, int32_t batch, int32_t part_mask,
                                const float* reg_rows, int32_t n_reg, const vittf_rope_table* table, uint16_t* q_out,
                                uint16_t* k_out, uint16_t* v_out, void* ws, size_t ws_bytes, void* stream);

/* The whole feature call: vittf_vit_qkv_features_rope plus the TOKEN facet, the final-norm patch tokens the DINOv2 / DINOv3
 * families publish as their dense feature (x_norm_patchtokens, get_intermediate_layers(norm=True); last_hidden_state[:, 1 + R:]
 * in transformers).  part_mask bits 0..2 = q, k, v of the hooked projection of block cfg->depth - 1, as before; bit 3 (8) = the
 * token facet: block cfg->depth - 1 is run in full, then the model's final LayerNorm norm_g / norm_b (fp32 [D], cfg->ln_eps)
 * over the patch-token rows of the fp32 residual stream (vittf_token_features); CLS and the n_reg register rows are dropped.
 * t_out: fp16 [batch][f0*f1][D], the layout of the other three outputs; fp16 whatever cfg->dtype, rounded once.  All four facets
 * come from ONE forward: with bit 3 and any of bits 0..2, the hooked thirds leave first (before the rotation, without the q
 * pre-scale: the bits of a call without bit 3), then the block goes on.  A hooked block in the middle of the model: set
 * cfg->depth to its index + 1 and pass the whole weight stacks; the final norm is then applied to that block's output.  Without
 * bit 3 this is vittf_vit_qkv_features_rope, bit for bit and launch for launch (norm_g, norm_b, t_out ignored, may be NULL).
 * part_mask outside 1..15, a NULL output of a set bit, bit 3 with a NULL norm_g / norm_b: VITTF_ERR_INVALID_ARG.  Workspace,
 * batch limit and every other check as vittf_vit_qkv_features_rope.  cfg->attention_fp8 without a table is allowed.
 * [host] cfg, w, pos, view, table are host structs holding device pointers. */
int vittf_vit_features(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                       const vittf_slice_view* view, int32_t slice0, int32_t batch, int32_t part_mask, const float* reg_rows,
                       int32_t n_reg, const vittf_rope_table* table, const float* norm_g, const float* norm_b, uint16_t* q_out,
                       uint16_t* k_out, uint16_t* v_out, uint16_t* t_out, void* ws, size_t ws_bytes, void* stream);

/* Optional timing of the launches inside vittf_vit_features (and the entry points that forward to it) and vittf_similarity, by kernel class, with HIP events recorded on
 * the caller's stream (what bench.py's roofline leg reads).  Process-global, off by default, not thread-safe:
 * the one exception to "no global mutable state".  enable(mask) clears earlier records and starts recording the
 * classes whose bit (1 << vittf_kernel_class) is set (-1: all; two event records per launch cost ~2-3 % of the
 * throughput when every launch is bracketed, so bench.py times with the dominant class only), enable(0) stops; collect() waits for the recorded events and returns, per class, the summed launch
 * durations in ms and the launch counts (arrays of VITTF_KERNEL_CLASSES entries, [host]). */
typedef enum vittf_kernel_class {
  VITTF_KERNEL_PATCH_EMBED = 0, VITTF_KERNEL_LAYERNORM = 1,
  VITTF_KERNEL_GEMM = 2,        /* linears without a class of their own: the K-feature projection */
  VITTF_KERNEL_ATTENTION = 3, VITTF_KERNEL_MLP = 4,
  VITTF_KERNEL_GEMM_QKV = 5,    /* attn.qkv (+ q pre-scale; + the DINOv3 rotation of q and k, vittf_rope_qk) */
  VITTF_KERNEL_GEMM_PROJ = 6,   /* attn.proj + residual (+ norm2) */
  VITTF_KERNEL_GEMM_FC1 = 7,    /* mlp.fc1 + GELU */
  VITTF_KERNEL_GEMM_FC2 = 8,    /* mlp.fc2 + residual (+ the next norm1) */
  VITTF_KERNEL_SIMILARITY = 9,  /* the voxel x query accumulation kernel(s) inside vittf_similarity / _maps_f32 */
  VITTF_KERNEL_CLASSES = 10
} vittf_kernel_class;
int vittf_profiler_enable(int32_t class_mask);
int vittf_profiler_collect(double* ms_per_class, int64_t* launches_per_class);
/* Name of the kernel the library's dispatcher launched LAST for a class that has several candidates (attention, similarity):
 * "" if none was launched yet.  Static storage; never NULL. */
const char* vittf_profiler_kernel_name(int32_t kernel_class);

/* ------------------------------------------------------------------------------------------
 * Individual kernels, exported so that each one is parity-tested on its own (tests/).
 * Row counts: activations are [rows][cols] row-major; `rows` need not be tile aligned.
 * ---------------------------------------------------------------------------------------- */

/* tokens[b][0] = cls+pos0 ; tokens[b][1+p] = patch_embed(slice slice0+b)[p] + pos[p]   -> fp32 [batch][tokens][D] */
int vittf_patch_embed(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                      const vittf_slice_view* view, int32_t slice0, int32_t batch, float* tokens_out, void* stream);

/* vittf_patch_embed with n_reg register rows behind CLS: tokens[b][0] = cls+pos0 ; tokens[b][1+r] = reg_rows[r] (bit for bit) ;
 * tokens[b][1+n_reg+p] = patch_embed(slice slice0+b)[p] + pos[p]   -> fp32 [batch][f0*f1 + 1 + n_reg][D].  A row's bits do not
 * depend on n_reg or on the batching. */
int vittf_patch_embed_reg(const vittf_vit_config* cfg, const vittf_vit_weights* w, const vittf_pos_embed* pos,
                          const vittf_slice_view* view, int32_t slice0, int32_t batch, const float* reg_rows, int32_t n_reg,
                          float* tokens_out, void* stream);

/* y = LayerNorm(x) * g + b, x fp32 [rows][D] -> y h16 [rows][D]  (nn.LayerNorm, biased variance) */
int vittf_layernorm(const float* x, const float* g, const float* b, void* y, int64_t rows, int32_t d,
                    float eps, int32_t dtype, void* stream);

/* The token facet's output kernel: t_out[b * (tokens - prefix) + t][d] (fp16) = LayerNorm(x[b * tokens + prefix + t]; norm_g,
 * norm_b, eps) for b < batch, t < tokens - prefix; x fp32 [batch * tokens][d], 16-byte aligned like norm_g and norm_b; t_out
 * 8-byte aligned.  The first `prefix` (>= 1: CLS + register tokens) rows of every slice are skipped, not read.  Statistics and
 * the affine map in fp32, biased variance as nn.LayerNorm, one rounding to fp16.  d a multiple of 4, at most 1024.  A row's bits
 * do not depend on batch or on where the slice sits in x. */
int vittf_token_features(const float* x, const float* norm_g, const float* norm_b, uint16_t* t_out, int32_t batch,
                         int32_t tokens, int32_t prefix, int32_t d, float eps, void* stream);

typedef enum vittf_epilogue {
  VITTF_EPI_BIAS = 0,        /* out h16 [rows][n] = a.w^T + bias */
  VITTF_EPI_BIAS_GELU = 1,   /* out h16 [rows][n] = gelu_erf(a.w^T + bias)        (Mlp.fc1 + nn.GELU) */
  VITTF_EPI_BIAS_RESIDUAL = 2,/* out fp32 [rows][n] += a.w^T + bias                (x = x + proj/fc2(...)) */
  VITTF_EPI_KFEAT = 3,       /* out fp16: rows whose (row % tokens) == 0 (CLS) are dropped, the others are
                                written densely: out[(row/tokens)*(tokens-1) + row%tokens - 1][n] */
  VITTF_EPI_BIAS_QKV = 4     /* as VITTF_EPI_BIAS, but columns [0, n/3) (the q third of Attention.qkv) are multiplied by
                                log2(e)/8 before the single rounding to h16: the softmax scale and the exp -> exp2 base
                                change folded into q, for vittf_attention(..., q_prescaled = 1) */
} vittf_epilogue;

/* out = epilogue(a[rows][k] . w[n][k]^T + bias[n]);  a, w: h16; k % 64 == 0, n % 128 == 0.
 * `tokens` is only used by VITTF_EPI_KFEAT. */
int vittf_gemm(const void* a, const void* w, const float* bias, void* out, int64_t rows, int32_t n, int32_t k,
               int32_t epilogue, int32_t tokens, int32_t dtype, void* stream);

/* The VITTF_EPI_KFEAT projection for several thirds of Attention.qkv in one launch: w is the whole qkv.weight [3 d][k],
 * bias the whole qkv.bias [3 d]; for every third p whose bit is set in part_mask (bit 0 = q, 1 = k, 2 = v) the K-feature
 * rows of a . w[p d .. p d + d - 1]^T + bias[p d ..] go to {q,k,v}_out ([rows - CLS rows][d] fp16, the VITTF_EPI_KFEAT
 * layout).  The grid covers the requested thirds' column tiles only, and each third is bit-equal to
 * vittf_gemm(EPI_KFEAT) on that third's weights and bias (the same kernel, the same accumulation order).  The pointer of an
 * unset bit is ignored (may be NULL); a NULL pointer for a set bit, part_mask 0 or above 7: VITTF_ERR_INVALID_ARG. */
int vittf_gemm_kfeat_parts(const void* a, const void* w, const float* bias, int64_t rows, int32_t d, int32_t k,
                           int32_t tokens, int32_t part_mask, void* q_out, void* k_out, void* v_out, int32_t dtype,
                           void* stream);

/* vittf_gemm_kfeat_parts with n_reg register rows behind CLS: rows whose (row % tokens) <= n_reg are dropped, the others go to
 * out[(row/tokens)*(tokens-1-n_reg) + row%tokens - 1 - n_reg][d].  tokens >= 2 + n_reg.  A kept row has the bits
 * vittf_gemm_kfeat_parts gives it when the register rows are taken out of `a`. */
int vittf_gemm_kfeat_parts_reg(const void* a, const void* w, const float* bias, int64_t rows, int32_t d, int32_t k,
                               int32_t tokens, int32_t n_reg, int32_t part_mask, void* q_out, void* k_out, void* v_out,
                               int32_t dtype, void* stream);

/* Residual linear + the LayerNorm that follows it:  x[rows][n] (fp32) += a[rows][k] . w[n][k]^T + bias;
 * h[rows][n] (h16) = LayerNorm(x; ln_g, ln_b, ln_eps).  Replaces attn.proj + residual + norm2 and mlp.fc2 + residual +
 * the next block's norm1.  For n = 384 (ViT-S) the LayerNorm is computed in the epilogue of a whole-row GEMM; other
 * shapes run vittf_gemm(BIAS_RESIDUAL) + vittf_layernorm. */
int vittf_gemm_residual_ln(const void* a, const void* w, const float* bias, float* x, int64_t rows, int32_t n, int32_t k,
                           int32_t dtype, const float* ln_g, const float* ln_b, float ln_eps, void* h, void* stream);

/* The K = 384 linears with a wide 16-bit output (Attention.qkv of ViT-S) with the ACTIVATIONS stationary: a wave keeps its 32 rows
 * as 24 MFMA operands and the weights stream through LDS, so every activation byte is read once.  out = epilogue(a . w^T + bias),
 * epilogue VITTF_EPI_BIAS or VITTF_EPI_BIAS_QKV; k == 384; n a multiple of 64, at most 1536 (a multiple of 96 for _QKV).
 * w_packed: h16 [n / 32][12288], the 24 KB images of weights.py pack_row_images (image u = rows 32 u .. + 31 of w in the LDS
 * tile layout).  Same bits as vittf_gemm on the same operands.  tile_counter: vittf_gemm_as_workspace_bytes() bytes of
 * caller-owned device memory, 4-byte aligned, private to this call until it has finished on `stream` (256-row tiles are handed
 * out through it; the call zeroes it on `stream` itself); concurrent calls need one each. */
size_t vittf_gemm_as_workspace_bytes(void);
int vittf_gemm_as(const void* a, const void* w_packed, const float* bias, void* out, int64_t rows, int32_t n, int32_t k,
                  int32_t epilogue, int32_t dtype, void* tile_counter, void* stream);

/* Everything behind the attention of one block for D == 384, in one launch:
 *   x' = x + attn_out . Wp^T + proj_b ;  x_new = x' + fc2(gelu_erf(fc1(LayerNorm(x'; ln2)) + b1)) + b2 ;  x := x_new ;
 *   h_out = LayerNorm(x_new; ln_g, ln_b)  (the next block's norm1; optional: ln_g, ln_b, h_out all NULL leaves it out).
 * Replaces Attention.proj + the two residual adds + norm2 + Mlp.forward of the upstream DINO block (reached through
 * model(...), infer.py:177).  attn_out: h16 [rows][D] (vittf_attention's output); w_packed: h16 [VITTF_TAIL_STEPS][12288], one
 * block of vittf_vit_weights.tail_packed.  The fp32 residual rows are read once and written once, and neither x' nor norm2's
 * output nor the hidden activation reaches HBM.  Same result as vittf_gemm_residual_ln (proj) + vittf_gemm(BIAS_GELU) +
 * vittf_gemm_residual_ln (fc2) up to fp32 summation order.  attn_out, w_packed, x and h_out must be 16-byte aligned
 * (VITTF_ERR_INVALID_ARG otherwise); D != 384: VITTF_ERR_INVALID_ARG (use the GEMM entries).  tile_counter:
 * vittf_block_tail_workspace_bytes() bytes of caller-owned device memory, 4-byte aligned, private to this call until it has
 * finished on `stream` (the persistent workgroups hand out 128-row tiles through it; the call zeroes it on `stream` itself;
 * concurrent calls -- two streams -- need one each; inside vittf_vit_k_features it lives in the engine workspace). */
size_t vittf_block_tail_workspace_bytes(void);
int vittf_block_tail(const void* attn_out, const void* w_packed, const float* proj_b, const float* ln2_g, const float* ln2_b,
                     const float* b1, const float* b2, float* x, int64_t rows, int32_t d, int32_t dtype, const float* ln_g,
                     const float* ln_b, float ln_eps, void* h_out, void* tile_counter, void* stream);

/* DINOv3's rotary position embedding applied in place to the q and k thirds of qkv h16 [rows][3 * 64 * heads] (columns
 * [q | k | v], heads of 64; 16-byte aligned): for every row with row % tokens >= prefix (a patch token; prefix = 1 + register
 * tokens: CLS and the registers are left untouched), every head of q and of k and j < 32, with t = row % tokens - prefix:
 *     x[j]'      = x[j] cos[t][j] - x[j + 32] sin[t][j]
 *     x[j + 32]' = x[j + 32] cos[t][j] + x[j] sin[t][j]
 * in fp32, rounded once to h16.  The v third is neither read nor written.  table->patches == tokens - prefix.  Works on q as
 * VITTF_EPI_BIAS_QKV leaves it (a rotation commutes with the scale). */
int vittf_rope_qk(void* qkv, int64_t rows, int32_t tokens, int32_t prefix, int32_t heads, const vittf_rope_table* table,
                  int32_t dtype, void* stream);

/* Multi-head self-attention over `batch` independent sequences of `tokens` rows.
 * qkv h16 [batch*tokens][3D] with columns [q | k | v], heads of 64 concatenated inside each third
 * (layout of Attention.qkv's output); out h16 [batch*tokens][D] = softmax(q k^T / 8) v per head.
 * q_prescaled = 0: q as the model produces it.  q_prescaled = 1: q already multiplied by log2(e)/8
 * (VITTF_EPI_BIAS_QKV) -- same result, computed by the faster kernel the engine uses (two 32-row query blocks per wave taking
 * turns, lazy running maximum). */
int vittf_attention(const void* qkv, void* out, int32_t batch, int32_t tokens, int32_t heads, int32_t dtype,
                    int32_t q_prescaled, void* stream);

/* Statistics: how many times (per 32-row query block and 32-key half step) the pre-scaled kernel's lazy running maximum
 * took its overflow branch (a row sum said the 16-bit P would overflow: true maximum, everything accumulated rescaled)
 * since the counter was last reset.  Rare on trained weights; the tests use it to prove that a case drives the branch.
 * Synchronises the device.  reset != 0 zeroes the counter after reading it. */
int64_t vittf_attention_rescale_count(int32_t reset);

/* fp8 attention (BASELINE configs[3]: "ViT-B/8 features, fp8 MFMA attention path").  Same contract as vittf_attention with
 * q_prescaled = 1, computed with OCP e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4: per (slice, head) power-of-two
 * scales for q, k and v (absmax / 448, applied by the instruction's scale operands), fp32 softmax statistics and
 * accumulators, P as fp8.  Error of the attention output ~3e-2 relative (3-bit mantissas):
 * an opt-in, never the default.  That figure is for a diffuse softmax; it grows with the magnitude of the logits (a 2^-4
 * relative operand error on a score of several hundred exp2 units moves the weights of a peaked row).  ws: vittf_attention_fp8_workspace_bytes(batch, tokens, heads) bytes, 256-byte aligned. */
size_t vittf_attention_fp8_workspace_bytes(int32_t batch, int32_t tokens, int32_t heads);
int vittf_attention_fp8(const void* qkv, void* out, int32_t batch, int32_t tokens, int32_t heads, int32_t dtype, void* ws,
                        size_t ws_bytes, void* stream);

/* The same path with q and k quantised where they are produced (round 4; what the engine runs for embed_dim >= 768):
 *   vittf_gemm_qkv_fp8: Attention.qkv (+ the q scale of VITTF_EPI_BIAS_QKV) for rows = batch * tokens rows, n = 3 * heads * 64,
 *     n / 3 a multiple of 256, k >= 768 and a multiple of 64.  q and k leave as e4m3 bytes [slice][head][token][64] with one
 *     power-of-two scale (E8M0 byte) per row and 32-wide block -- the MX block format: the matrix instruction's scale operand
 *     is per lane, i.e. per row and block -- into `ws`; v is written as h16 into the v third of qkv_out [rows][n] (the q and k
 *     thirds of qkv_out are NOT written) and its per-(slice, head) absolute maximum is collected into `ws`.
 *   vittf_attention_fp8_rows: quantises + re-lays the v third (per-(slice, head) scale), then the attention kernel with the
 *     row scales.  Same output contract and error class as vittf_attention_fp8 (finer scales for q and k).
 * ws: the same vittf_attention_fp8_workspace_bytes(batch, tokens, heads) workspace, passed to both calls. */
int vittf_gemm_qkv_fp8(const void* a, const void* w, const float* bias, void* qkv_out, int64_t rows, int32_t n, int32_t k,
                       int32_t tokens, int32_t heads, int32_t dtype, void* ws, size_t ws_bytes, void* stream);
int vittf_attention_fp8_rows(const void* qkv, void* out, int32_t batch, int32_t tokens, int32_t heads, int32_t dtype, void* ws,
                             size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature-volume epilogue (infer.py:201-203 permute_out, :329 AdaptiveAvgPool3d, :330-332 axis sum).
 * ---------------------------------------------------------------------------------------- */

/* Average-pool the slice axis of the token-major K features of ONE axis and scatter them, feature-major,
 * into a pooled slab:  for window i in [win0, win0 + nwin):
 *     slices [floor(i*S/n_out), ceil((i+1)*S/n_out))  (adaptive rule); running sum in slice order kept in
 *     fp16 (one rounding per add, as the CPU AdaptiveAvgPool3d does for half tensors), then fp16(sum / count);  written to dst[d*dst_stride_d + (i - win0)*dst_stride_win + r*dst_stride_row + c*dst_stride_col]
 * k_slices holds slices [k_slice0, k_slice0 + k_nslices) of the axis as [slice][f0][f1][D] fp16; every
 * slice a requested window touches must be inside that range.  n_out == S gives the un-pooled layout. */
int vittf_pool_slices(const uint16_t* k_slices, int32_t k_slice0, int32_t k_nslices, int32_t total_slices,
                      int32_t n_out, int32_t win0, int32_t nwin, int32_t f0, int32_t f1, int32_t d,
                      uint16_t* dst, int64_t dst_stride_d, int64_t dst_stride_win, int64_t dst_stride_row,
                      int64_t dst_stride_col, void* stream);

/* vittf_pool_slices with in-plane adaptive pooling too (AdaptiveAvgPool3d of any output size, infer.py:203): output
 * voxel (i, r, c), i in [win0, win0 + nwin), r < o0 (image rows), c < o1 (image cols), is the mean over slice window i and
 * in-plane windows r of f0 and c of f1 (adaptive rule; o0 > f0 / o1 > f1 allowed), written to
 * dst[d*dst_stride_d + (i - win0)*dst_stride_win + r*dst_stride_row + c*dst_stride_col].  slice_dim (0, 1, 2) = the volume
 * dimension the slices run along (x, y, z); the image rows / cols are the other two, in order.  Rounding of the CPU
 * AdaptiveAvgPool3d on fp16: a running fp16 sum over the window in volume-dimension order (dim 0 outermost, dim 2
 * innermost), then fp16(sum / n0), fp16(. / n1), fp16(. / n2) with the window extents along volume dims 0, 1, 2.
 * Exception, as in torch: an output of exactly (1, 1, 1) (n_out == o0 == o1 == 1) is input.mean(), i.e. the sum over every
 * slice accumulated in fp32 or wider, divided in fp32, rounded once to fp16 (the bits of torch's CPU mean up to its fp32
 * summation order).
 * Otherwise, o0 == f0 and o1 == f1 is vittf_pool_slices (the same kernel; the same bits for any slice_dim). */
int vittf_pool_slices3d(const uint16_t* k_slices, int32_t k_slice0, int32_t k_nslices, int32_t total_slices,
                        int32_t n_out, int32_t win0, int32_t nwin, int32_t f0, int32_t f1, int32_t d,
                        uint16_t* dst, int64_t dst_stride_d, int64_t dst_stride_win, int64_t dst_stride_row,
                        int64_t dst_stride_col, int32_t o0, int32_t o1, int32_t slice_dim, void* stream);

/* out = fp16(fp16(z + y) + x) element-wise: the reference's running fp16 sum in z, y, x order
 * (infer.py:330-332).  Inputs are the per-axis pooled volumes as gathered from `nranks` ranks:
 * axis a is stored [nranks][D][...] where each rank block holds `chunk[a]` windows of the axis' slice
 * dimension (slab layout written by vittf_pool_slices); out is (D, n0, n1, n2) fp16, C-contiguous. */
int vittf_assemble_sum(const uint16_t* gz, const uint16_t* gy, const uint16_t* gx, int32_t nranks,
                       const int32_t chunk[3], int32_t d, int32_t n0, int32_t n1, int32_t n2, uint16_t* out,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Similarity query (predict_ntf.py:52-72, 95-100) and label assignment (predict_ntf.py:203-215).
 * ---------------------------------------------------------------------------------------- */

/* F.grid_sample of the feature volume (infer.py:48-72): feat fp16 or fp32 (F, n0, n1, n2); rel fp32 [A][3]
 * relative coordinates in [-1, 1] in VOLUME dim order (the flip to grid_sample's x,y,z order of infer.py:67
 * happens inside); align_corners=False, zero padding; mode nearest or trilinear ('bilinear').  out fp32 [A][F]. */
int vittf_sample_features(const void* feat, int32_t feat_is_fp16, int32_t f, int32_t n0, int32_t n1, int32_t n2,
                          const float* rel, int32_t a, int32_t mode, const float* voxel_norm, float* out, void* stream);

/* Per-voxel L2 norm of the F-major fp16 feature volume, clamped like F.normalize's denominator:
 * out[v] = max(|feat[:, v]|_2, 1e-12), fp32 [nvox].  Passing it as `voxel_norm` to vittf_sample_features /
 * vittf_similarity makes them operate on F.normalize(feat, dim=0) -- the cosine similarity of
 * compare_feat_sampling.py:45 / tests/test_vishum.py:12 -- without materialising a normalised copy. */
int vittf_voxel_norm(const uint16_t* feat, int32_t f, int64_t nvox, float* out, void* stream);

size_t vittf_similarity_workspace_bytes(int32_t classes, int64_t nvox, int32_t annotations);

/* Fused similarity: for every voxel v and class c with annotations [class_start[c], class_start[c+1]):
 *     dot[a] = sum_f feat[f][v] * qf[a][f]                       (einsum predict_ntf.py:65)
 *     sim_c  = mean_a( dot[a] >= 0.25 ? dot[a]^2.5 : 0 )         (predict_ntf.py:71-72)
 *     (big_a_mean != 0: the single-class A > 1024 variant, mean of raw dots first, predict_ntf.py:62-63)
 *     u8     = trunc(255 / (0.99 * max_v sim_c) * sim_c) mod 256 (predict_ntf.py:98-99, x86 wrap-around)
 * then nearest-resized to (o0, o1, o2) (predict_ntf.py:100).  feat fp16 (F, n0, n1, n2) F-major;
 * qf fp32 [A][F]; class_start int32 [classes + 1] on the HOST; out uint8 [classes][o0][o1][o2].
 * voxel_norm: NULL (predict_ntf.py semantics: raw dot products) or the vittf_voxel_norm array (every dot divided by
 * the voxel's norm: cosine similarity against queries sampled with the same array). */
int vittf_similarity(const uint16_t* feat, int32_t f, int32_t n0, int32_t n1, int32_t n2, const float* qf,
                     const int32_t* class_start_host, int32_t classes, int32_t big_a_mean, const float* voxel_norm,
                     int32_t o0, int32_t o1, int32_t o2, uint8_t* out, void* ws, size_t ws_bytes, void* stream);

/* The interactive query in ONE call (predict_ntf.py:56-72, 95-100): samples the annotations' features (trilinear, as
 * vittf_sample_features) at rel_host -- fp32 [A][3] relative coordinates in HOST memory, formed as predict_ntf.py:56 does; they
 * travel as a kernel argument, so A = class_start_host[classes] is at most VITTF_QUERY_MAX_A --, accumulates the class maps and
 * quantises + resizes them: the same bytes as vittf_sample_features + vittf_similarity, with three launches and no copy or
 * memset between the call and the first kernel.  ws: vittf_similarity_query_workspace_bytes(classes, nvox, A, f) bytes: the
 * vittf_similarity_workspace_bytes(classes, nvox, A) bytes of vittf_similarity's workspace, then the sampled queries, fp32
 * [A][F] (what vittf_sample_features would have written). */
#define VITTF_QUERY_MAX_A 64
size_t vittf_similarity_query_workspace_bytes(int32_t classes, int64_t nvox, int32_t annotations, int32_t f);
int vittf_similarity_query(const uint16_t* feat, int32_t f, int32_t n0, int32_t n1, int32_t n2, const float* rel_host,
                           const int32_t* class_start_host, int32_t classes, int32_t big_a_mean, const float* voxel_norm,
                           int32_t o0, int32_t o1, int32_t o2, uint8_t* out, void* ws, size_t ws_bytes, void* stream);

/* fp32 per-group maps without quantisation or resizing: maps_out fp32 [classes][n0*n1*n2].
 *   mode 0: predict_ntf.py:65-72 (the input of the bilateral-solver branch :73-96); mode 1: its A > 1024 variant (:62-63);
 *   mode 2: the second similarity of resample_topk (infer.py:104-106): clamp(dot, 0, 1) ** exponent, mean over each group
 *           of queries; feat may then be fp32 (feat_is_fp16 = 0), e.g. an already normalised volume.
 * ws: vittf_similarity_workspace_bytes(classes, 0, annotations) bytes (no fp32 map region needed). */
int vittf_similarity_maps_f32(const void* feat, int32_t feat_is_fp16, int32_t f, int32_t n0, int32_t n1, int32_t n2,
                              const float* qf, const int32_t* class_start_host, int32_t classes, int32_t mode,
                              float exponent, const float* voxel_norm, float* maps_out, void* ws, size_t ws_bytes,
                              void* stream);

/* Per map (nmaps maps of nvox fp32 values): the first k voxel indices, in index order, whose value is >= the k-th largest
 * value of the map -- torch.topk(s.flatten(), K).values[-1]; (s >= that).nonzero()[:K]  (infer.py:95-96).
 * idx_out int32 [nmaps][k] (device).  1 <= k <= nvox and nmaps >= 1, else VITTF_ERR_INVALID_ARG.
 * Zeros: -0.0 and +0.0 compare equal, as under the expression's >=: on a map whose k-th largest value is a zero, voxels of
 * either sign of zero are kept, in index order (a thresholded map is mostly zeros).  +-inf order like any value.
 * NaN is outside the contract: with a NaN in the map the expression itself returns fewer than K indices (NaN sorts above
 * +inf in topk and compares false under >=); the kernel then still writes k indices, and which ones is unspecified. */
int vittf_topk_voxels(const float* maps, int32_t nmaps, int64_t nvox, int32_t k, int32_t* idx_out, void* stream);

/* take_most_dissimilar's distance (infer.py:118-121): dist[i] = 1 - mean_j cos(x_i, x_j) (measure 0, F.cosine_similarity
 * with eps 1e-8) or mean_j |x_i - x_j|_2 (measure 1, torch.cdist); x fp32 [n][f], dist fp32 [n]. */
int vittf_mean_pairwise_distance(const float* x, int32_t n, int32_t f, int32_t measure, float* dist, void* stream);

/* ------------------------------------------------------------------------------------------
 * PCA reduction of a feature volume (vit-tf_amd/pca.py, reduce_features.py, infer.py --pca): the first principal
 * components of the dense features, as the DINOv2 / DINOv3 papers show them, as a colour volume or a compact volume the
 * similarity entries above take unchanged.  feat: fp16 [f][nvox], the F-major file layout, 2-byte aligned; f a multiple of
 * 32 in 32..1024; nvox >= 1, any value (rows that are not 16-byte aligned take a slower load path).
 * ---------------------------------------------------------------------------------------- */
#define VITTF_GRAM_RUN 2048   /* most voxels one fp32 accumulator of the Gram kernel covers before it is added into fp64 */
#define VITTF_PCA_MAX_K 64    /* most components of one projection call */

/* gram[i][j] = sum_v x_iv x_jv (fp64 [f][f], both triangles, exactly symmetric) and sums[i] = sum_v x_iv (fp64 [f]).
 * fp16 MFMAs with fp32 accumulation (every product is exact) over runs of at most VITTF_GRAM_RUN voxels; the runs are summed
 * in fp64 in a fixed order and there are no floating-point atomics: the same call gives the same bits.  The eigenproblem
 * of the f x f covariance is host work (pca.py basis_from_gram).  gram, sums, ws: 8-byte aligned; ws: >=
 * vittf_feature_gram_workspace_bytes(f, nvox) bytes (0 for an f or nvox the call refuses). */
size_t vittf_feature_gram_workspace_bytes(int32_t f, int64_t nvox);
int vittf_feature_gram(const uint16_t* feat, int32_t f, int64_t nvox, double* gram, double* sums, void* ws, size_t ws_bytes,
                       void* stream);

/* out[c][v] = fp16(sum_f comp[c][f] x_fv - offset[c]): fp16 [k][nvox], F-major like the input, rounded once.  comp fp32
 * [k][f], taken as fp16 hi + lo halves (to 2^-22 relative) with fp32 accumulation; offset fp32 [k] or NULL (zeros);
 * 1 <= k <= VITTF_PCA_MAX_K.  The volume is read once. */
int vittf_feature_project(const uint16_t* feat, int32_t f, int64_t nvox, const float* comp, const float* offset, int32_t k,
                          uint16_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * k-means clustering of a feature volume (vit-tf_amd/kmeans.py, cluster_features.py): the two passes over the volume of
 * one Lloyd iteration.  feat, f, nvox: as for the PCA entries above (fp16 [f][nvox], 2-byte aligned, f a multiple of 32 in
 * 32..1024, nvox >= 1; rows that are not 16-byte aligned take a slower load path).  2 <= c <= VITTF_KMEANS_MAX_C.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_KMEANS_MAX_C 64   /* most clusters of one call */

/* labels[v] = argmax_c (sum_f cent[c][f] x_fv - half_sq[c]); the lowest index wins among equal fp32 scores.  With half_sq[c]
 * = 0.5 |m_c|^2 that is the nearest centroid in squared Euclidean distance.  cent fp32 [c][f], taken as fp16 hi + lo halves
 * (to 2^-22 relative) with fp32 accumulation; half_sq fp32 [c] or NULL (zeros); labels uint8 [nvox]; best fp32 [nvox] or NULL:
 * the winning score.  The volume is read once. */
int vittf_kmeans_assign(const uint16_t* feat, int32_t f, int64_t nvox, const float* cent, const float* half_sq, int32_t c,
                        uint8_t* labels, float* best, void* stream);

/* sums[k][i] = sum over {v: labels[v] == k} of x_iv (fp64 [c][f]) and counts[k] = the number of such voxels (int64 [c]).  A
 * voxel whose label is >= c contributes nowhere (255 masks a voxel out).  fp16 MFMAs against a 0/1 operand (every product
 * is exact) with fp32 accumulation over runs of at most VITTF_GRAM_RUN voxels; the runs are summed in fp64 in a fixed order
 * and there are no floating-point atomics: the same call gives the same bits.  The volume is cut into at most 128 spans of
 * whole runs; ws: >= vittf_kmeans_sums_workspace_bytes(f, nvox, c) = spans x ((f / 32) ceil(c / 32) x 1024 + 64) x 8 bytes
 * (at most 67 MB; 0 for a shape the call refuses).  sums, counts, ws: 8-byte aligned. */
size_t vittf_kmeans_sums_workspace_bytes(int32_t f, int64_t nvox, int32_t c);
int vittf_kmeans_sums(const uint16_t* feat, int32_t f, int64_t nvox, const uint8_t* labels, int32_t c, double* sums,
                      int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Support-vector classification of a feature volume (vit-tf_amd/svm.py, classify_features.py): the decision pass of a
 * one-vs-one C-SVC as libsvm and scikit-learn define it.  classes = C in 2..VITTF_SVM_MAX_CLASSES; the P = C (C - 1) / 2
 * pairs are ordered (0,1), (0,2), ..., (C-2,C-1); for pair p = (i, j) a decision dec_p > 0 votes for i, anything else
 * (exactly 0 included) for j; the label is the class with the most votes, the lowest index among equal counts.
 * feat, nvox: as for the PCA entries above (fp16 [f][nvox], 2-byte aligned, nvox >= 1; rows that are not 16-byte aligned take
 * a slower load path).  voxel_norm: NULL or the vittf_voxel_norm array: the voxel is then x / norm, as in vittf_similarity.
 * labels uint8 [nvox] (0..C-1, any alignment); decision NULL or fp32 [P][nvox].  The labels are the vote over exactly the
 * fp32 values the call writes to `decision`, and the same bytes whether it is NULL or not; fixed summation order and no
 * floating-point atomics: the same call gives the same bytes.  The volume is read once.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_SVM_MAX_CLASSES 8   /* most classes of one model: 28 pairs, the decisions of a voxel fill one 32-row MFMA tile */
#define VITTF_SVM_MAX_SV 65536    /* most support vectors of one model */

/* RBF kernel: dec_p(x) = sum_s pair_coef[p][s] exp(-gamma |x - sv_s|^2) + intercept[p].  sv fp16 [n_sv][f] (the fit rounds
 * its samples to fp16 first, so these are the model's vectors exactly), pair_coef fp32 [P][n_sv], dense, zero where the
 * support vector's class is not in the pair; intercept fp32 [P]; 1 <= n_sv <= VITTF_SVM_MAX_SV; gamma >= 0, finite.
 * f a multiple of 32 in 32..768 (padded inside with zero features to 32, 128, 384 or 768; reduce a wider volume first).
 * sv . x: fp16 MFMAs with fp32 accumulation; the exponential is one v_exp_f32; the second contraction runs on the matrix
 * cores with the kernel values and the (power-of-two scaled) coefficients as fp16 hi + lo halves (2^-22 relative).
 * Three launches (coefficient scale, support-vector images, decision).  ws: 16-byte aligned, >=
 * vittf_svm_rbf_workspace_bytes(f, n_sv, classes) = 256 + ceil(n_sv / 32) x (64 FP + 5760) bytes (0 for a shape the call
 * refuses); too small: VITTF_ERR_WORKSPACE. */
size_t vittf_svm_rbf_workspace_bytes(int32_t f, int32_t n_sv, int32_t classes);
int vittf_svm_rbf_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint16_t* sv, const float* pair_coef,
                         const float* intercept, int32_t n_sv, int32_t classes, float gamma, const float* voxel_norm,
                         uint8_t* labels, float* decision, void* ws, size_t ws_bytes, void* stream);

/* Linear kernel: dec_p(x) = w[p] . x + intercept[p], w fp32 [P][f] = sum_s pair_coef[p][s] sv_s folded on the host, taken as
 * fp16 hi + lo halves (to 2^-22 relative) with fp32 accumulation: vittf_kmeans_assign's score loop with the vote behind it
 * instead of the arg-max.  f a multiple of 32 in 32..1024. */
int vittf_svm_linear_decide(const uint16_t* feat, int32_t f, int64_t nvox, const float* w, const float* intercept,
                            int32_t classes, const float* voxel_norm, uint8_t* labels, float* decision, void* stream);

/* ------------------------------------------------------------------------------------------
 * Random-forest classification of a feature volume (vit-tf_amd/forest.py, classify_features.py --classifier forest): the
 * pass of a fitted forest of binary decision trees over every voxel, scikit-learn's soft vote in integers.
 * feat, nvox: as above (fp16 [f][nvox], finite, 2-byte aligned, nvox >= 1, f a multiple of 32 in 32..1024; rows that are
 * not 16-byte aligned take scalar loads).  The packed forest (forest.py's pack() writes it from a validated model):
 *   tree_offset  uint32 [trees + 1]: tree t owns nodes[tree_offset[t] .. tree_offset[t + 1]), node 0 of it is its root;
 *                at most VITTF_FOREST_MAX_NODES nodes a tree
 *   nodes        two uint32 per node (8 bytes, 8-byte aligned).
 *                inner node: word 0 = feature | threshold << 16 (feature < f; threshold: the bits of an fp16, not NaN),
 *                            word 1 = left | right << 16, indices inside the tree, BOTH LARGER than the node's own;
 *                leaf:       word 0 = 0xFFFF, word 1 = the row of the leaf in leaf_values
 *   leaf_values  uint16 [leaves][8] (16-byte aligned): floor(p_c 65535 + 0.5) of the leaf's class shares p_c, zeros behind
 *                the last class
 * A voxel goes LEFT at an inner node when feat[feature][voxel] <= threshold, the two compared as fp16 numbers (-0 == +0;
 * a threshold of +inf sends everything left, -inf everything right).  For fp16 x and any real t, x <= t exactly when
 * x <= the largest fp16 <= t: a forest fitted in fp32 or fp64 converts without changing a decision.  votes[c][v] is the
 * uint32 sum over the trees of leaf_values[leaf][c] (trees <= 4096: at most 4096 x 65535 < 2^32); labels[v] the class with
 * the largest vote, the lowest index among equal votes.  max_depth, 0..VITTF_FOREST_MAX_DEPTH, is the depth of the deepest
 * tree (a single leaf has depth 0): a walk takes at most max_depth steps whatever the nodes say, and one that has not
 * reached a leaf by then casts no vote for its tree.  votes may be NULL; the labels are the same.  Integer arithmetic
 * only, no atomics: the same call gives the same bytes.  One launch, no workspace; the volume is read once.
 * Workgroups of 1024 threads own 1024, 512, 256, 128 or 64 voxels (f <= 64, 128, 256, 512, 1024), staged in a 128 KiB LDS tile.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_FOREST_MAX_CLASSES 8       /* most classes of one forest: a leaf row is one 16-byte load */
#define VITTF_FOREST_MAX_TREES 4096      /* most trees: the uint32 votes cannot overflow */
#define VITTF_FOREST_MAX_NODES 65535     /* most nodes of one tree: child indices are 16 bits */
#define VITTF_FOREST_MAX_DEPTH 64        /* largest max_depth */
int vittf_forest_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint32_t* nodes, const uint16_t* leaf_values,
                        const uint32_t* tree_offset, int32_t trees, int32_t classes, int32_t max_depth, uint8_t* labels,
                        uint32_t* votes, void* stream);

/* ------------------------------------------------------------------------------------------
 * MLP head over a feature volume (vit-tf_amd/mlp.py, classify_features.py --classifier mlp): the decision pass of the
 * reference's old/compare_feat_sampling_mlp.py head, Linear (-> ReLU -> Linear) x layers, over every voxel.
 * feat, nvox, voxel_norm: as for the SVM entries above (fp16 [f][nvox], f a multiple of 32 in 32..1024; with voxel_norm the
 * voxel is x / norm, applied to the first contraction before its bias).  widths [host]: the `layers` hidden widths
 * (layers in 0..VITTF_MLP_MAX_LAYERS, may be NULL for 0), each a multiple of 32 in 32..VITTF_MLP_MAX_WIDTH; classes in
 * 2..VITTF_MLP_MAX_CLASSES.  weights: the layers + 1 matrices fp32 [out][in] one behind the other (in = f, then the widths;
 * the last out = classes), biases: their fp32 [out] vectors one behind the other; all values finite.
 * labels uint8 [nvox]: the arg-max of the fp32 logits, the lowest index among equal logits.  logits NULL or fp32
 * [classes][nvox]; probs NULL or uint8 [classes][nvox] = floor(255 softmax_c + 0.5), the maximum subtracted first, from the
 * same registers.  The labels are the same bytes whatever else is asked for.
 * Arithmetic: every matrix is scaled by a power of two (largest entry into [2^10, 2^11)) and split into fp16 hi + lo
 * (2^-22 relative, 2^-35 of the largest entry absolute); the voxels' fp16 features are exact MFMA operands; fp32
 * accumulation in a fixed order, no atomics: the same call gives the same bytes.  After bias and ReLU the accumulator tile
 * of a wave is the B operand of the next contraction as it lies (hi + lo; hi hi + hi lo + lo hi), scaled PER VOXEL by a
 * power of two that brings the voxel's largest activation into [2^10, 2^11): the hand-over cannot leave the fp16 range
 * whatever the activations are.  Hidden activations never leave the chip; the volume is read once.
 * Three launches (scales, weight images, decision).  ws: 16-byte aligned, >= vittf_mlp_workspace_bytes(f, widths, layers,
 * classes) = 256 + sum over the matrices of (in / 32) x ceil(out / 32) x 5120 bytes (0 for a head the call refuses); too
 * small: VITTF_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_MLP_MAX_CLASSES 8   /* most classes of one head: the logits of a voxel are 8 rows of one MFMA tile */
#define VITTF_MLP_MAX_LAYERS 2    /* most hidden layers */
#define VITTF_MLP_MAX_WIDTH 256   /* widest hidden layer: 8 accumulator tiles a wave */
size_t vittf_mlp_workspace_bytes(int32_t f, const int32_t* widths, int32_t layers, int32_t classes);
int vittf_mlp_decide(const uint16_t* feat, int32_t f, int64_t nvox, const float* weights, const float* biases,
                     const int32_t* widths, int32_t layers, int32_t classes, const float* voxel_norm, uint8_t* labels,
                     float* logits, uint8_t* probs, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weighted k-nearest-neighbour classification of a feature volume (vit-tf_amd/knn.py, classify_features.py --classifier
 * knn): the k-NN of the DINO evaluation protocol.  There is no fit: the model is the bank of labelled samples itself.
 * feat, nvox, voxel_norm: as for the SVM entries above (fp16 [f][nvox]; f a multiple of 32 in 32..768, padded inside with
 * zero features to 32, 128, 384 or 768).  bank fp16 [n_bank][f], bank_class uint8 [n_bank] with values in 0..classes-1 (the
 * caller checks them; the call trusts them), 1 <= n_bank <= VITTF_KNN_MAX_BANK, classes in 2..VITTF_KNN_MAX_CLASSES,
 * 1 <= k <= min(VITTF_KNN_MAX_K, n_bank).
 * Per voxel v: sim_s = bank_s . x_v (fp16 MFMAs, fp32 accumulation), times 1 / voxel_norm[v] in fp32 when voxel_norm is not
 * NULL.  The neighbours are the k samples that come first under "larger sim first, then lower sample index", an IEEE
 * comparison of exactly these fp32 values; rank 1 is the nearest.  Weights: w_j = 1 for inv_temperature = 0 (uniform);
 * otherwise (inv_temperature = 1 / T > 0, finite) w_j = exp2((sim_j - sim_1) c) with c = fl32(log2(e) inv_temperature),
 * formed on the host in double: w_1 = 1, nothing overflows.  scores[c][v] = the sum of w_j over the ranks j = 1..k whose
 * sample has class c, added in fp32 in rank order; labels[v] = the arg-max of these fp32 scores, the lowest class among
 * equal ones.  scores NULL or fp32 [classes][nvox]; nn_index (int32) and nn_sim (fp32) each NULL or [k][nvox], rank-major.
 * Fixed order and no floating-point atomics: the same call gives the same bytes, and leaving any optional output NULL gives
 * the same bytes in the others.  Two launches (bank images, decision); the volume is read once.
 * ws: 16-byte aligned, >= vittf_knn_workspace_bytes(f, n_bank) = ceil(n_bank / 32) x (64 FP + 640) bytes (0 for a shape the
 * call refuses); too small: VITTF_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_KNN_MAX_K 32        /* most neighbours: the sorted list of a lane lives in registers */
#define VITTF_KNN_MAX_CLASSES 8   /* most classes of one bank */
#define VITTF_KNN_MAX_BANK 65536  /* most samples of one bank: index and class share one 32-bit word */
size_t vittf_knn_workspace_bytes(int32_t f, int32_t n_bank);
int vittf_knn_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint16_t* bank, const uint8_t* bank_class,
                     int32_t n_bank, int32_t classes, int32_t k, float inv_temperature, const float* voxel_norm,
                     uint8_t* labels, float* scores, int32_t* nn_index, float* nn_sim, void* ws, size_t ws_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Hand-crafted voxel features (vit-tf_amd/voxel_features.py, classify_features.py --features handcrafted | intensity): the
 * 11-channel per-voxel vector of the reference's classical baseline (predict_svm_rf.py:25-65) at the volume's own
 * resolution, as rows of the fp16 [f][nvox] matrix the two decision passes above take.
 * vol: fp32 (n0, n1, n2), C-contiguous, 4-byte aligned; every dimension in 2..2048 and n0 n1 n2 < 2^31; vmax its maximum
 * (vittf_volume_minmax), finite and > 0.  With I = vol / vmax and v = (i0 n1 + i1) n2 + i2 the raw channels are
 *   0      I
 *   1      sqrt(gx^2 + gy^2 + gz^2), g = 0.5 (I[+1] - I[-1]) along each axis; a neighbour outside the volume counts as 0
 *   2..7   I at (i0+1), (i1+1), (i2+1), (i0-1), (i1-1), (i2-1); a neighbour outside the volume is the border voxel itself
 *   8..10  i0 / n0 - 0.5, i1 / n1 - 0.5, i2 / n2 - 0.5
 * and each is standardised over the whole volume, (x - mean_c) / std_c, std_c the unbiased one (divisor nvox - 1).
 *
 * vittf_voxel_feature_stats: stats (device fp64 [2][11], 8-byte aligned) = the means, then the stds of the raw channels,
 * accumulated in fp64 over workgroups of 16384 consecutive voxels whose partial sums (ws: 8-byte aligned, at least
 * vittf_voxel_feature_stats_workspace_bytes(n0, n1, n2) = 128 bytes per workgroup; 0 for a shape the call refuses; too small:
 * VITTF_ERR_WORKSPACE) are added in a fixed order by a second launch: no floating-point atomics, the same call gives the same
 * bytes.  The coordinate channels take their closed forms.
 *
 * vittf_voxel_features: out[c out_stride + i] (fp16 bits, 2-byte aligned, out_stride >= n) = the standardised channel
 * c < channels of voxel voxel_index[i] (device int64 [n], 8-byte aligned, every entry in 0..nvox-1: the CALLER checks them;
 * the kernel writes NaN for one that is not) or, with voxel_index NULL, of voxel v0 + i (0 <= v0, v0 + n <= nvox), for
 * i < n, n >= 1.  channels is 11 or 1 (the intensity alone); rows from `channels` up are neither read nor written -- the
 * caller embeds the rows in a zeroed 32-row matrix for the decision passes.  A voxel's bits do not depend on the addressing
 * mode, on v0, n or out_stride.  16-byte stores where out + c out_stride + i is 16-byte aligned (every row when out_stride
 * is a multiple of 8), 2-byte stores elsewhere.  The call reads `stats` back (it waits for the stream) and returns
 * VITTF_ERR_INVALID_ARG without a launch when a mean is not finite or a std of a channel < channels is 0 or not finite.
 * fp32 arithmetic from coefficients folded in fp64: I = vol (1 / vmax), then one fma per channel.
 * ---------------------------------------------------------------------------------------- */
#define VITTF_VOXFEAT_CHANNELS 11
size_t vittf_voxel_feature_stats_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int vittf_voxel_feature_stats(const float* vol, int32_t n0, int32_t n1, int32_t n2, float vmax, double* stats, void* ws,
                              size_t ws_bytes, void* stream);
int vittf_voxel_features(const float* vol, int32_t n0, int32_t n1, int32_t n2, float vmax, const double* stats, int32_t channels,
                         const int64_t* voxel_index, int64_t v0, int64_t n, uint16_t* out, int64_t out_stride, void* stream);

/* ---- label-volume helpers: sampler candidate masks and scores --------------------------- */
/* dst = binary_erosion(set, generate_binary_structure(3, connectivity)) with scipy.ndimage's defaults (one iteration,
 * border_value 0): set = {src == class_id} (class_id 0..255) or {src != 0} (class_id < 0); uint8 volumes (n0, n1, n2),
 * dst 0/1, src != dst.  connectivity 1 = 6 face neighbours, 2 = 18, >= 3 = the full 3x3x3 cube. */
int vittf_erode_mask(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t class_id, int32_t connectivity,
                     uint8_t* dst, void* stream);

/* sample_surface's candidate set (compare_feat_sampling.py:19-24): outer = erosion of {labels == class_id} by
 * generate_binary_structure(3, connectivity = dist_from_surface), shell = outer XOR erosion of outer by the 6-neighbour
 * element; shell uint8 0/1 (n0, n1, n2); ws: vittf_surface_shell_workspace_bytes(n0, n1, n2). */
size_t vittf_surface_shell_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int vittf_surface_shell(const uint8_t* labels, int32_t n0, int32_t n1, int32_t n2, int32_t class_id, int32_t connectivity,
                        uint8_t* shell, void* ws, size_t ws_bytes, void* stream);

/* counts[t * classes + p] = number of voxels with target t and prediction p (sklearn confusion_matrix with labels
 * 0..classes-1; predict_ntf.py:228-246, evaluate_similarities.py:63-68); counts[classes * classes] = voxels holding a
 * value >= classes in either volume.  counts: int64 [classes * classes + 1] (device, overwritten); classes <= 16. */
int vittf_confusion_matrix(const uint8_t* target, const uint8_t* pred, int64_t n, int32_t classes, int64_t* counts,
                           void* stream);

/* ---- connected components of a uint8 volume (vit-tf_amd/components.py, label_islands.py, predict_ntf.py --largest-island) --
 * Foreground and link rule: select 0..255: the set {src == select} (as vittf_erode_mask defines it); -1: {src != 0}; -2 ("each
 * value"): every voxel whose value is not 255 is foreground and two neighbours are linked only if they hold the same value
 * (one call labels every cluster of a k-means volume: there 0 is a cluster and 255 the mask value of vittf_kmeans_sums).
 * connectivity 1 = 6 face neighbours (scipy.ndimage.label's default), 2 = 18, 3 = 26: generate_binary_structure(3,
 * connectivity), the numbering of vittf_erode_mask; anything else: VITTF_ERR_INVALID_ARG.
 * labels int32 (n0, n1, n2), 4-byte aligned: 0 for background, else 1 + the smallest linear index (i0 * n1 + i1) * n2 + i2
 * among the voxels of the component -- independent of any execution order: the same input gives the same bytes.
 * n0 * n1 * n2 <= 2^31 - 2.  src may sit at any byte alignment.  ws: 4-byte aligned, >= vittf_components_workspace_bytes(n0, n1,
 * n2) = 4 bytes per voxel rounded up to 256 (0 for a shape the call refuses); too small: VITTF_ERR_WORKSPACE.
 * Three launches: union-find in LDS per 4 x 8 x 64 tile (n2 the fast axis), union-find over the tile seams on the global parent
 * array (agent-scope atomics), flatten. */
#define VITTF_CC_TILE0 4
#define VITTF_CC_TILE1 8
#define VITTF_CC_TILE2 64
size_t vittf_components_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int vittf_label_components(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t select, int32_t connectivity,
                           int32_t* labels, void* ws, size_t ws_bytes, void* stream);

/* sizes[l - 1] = the number of voxels with label l, for a label volume of vittf_label_components (labels 0..nvox); sizes int32
 * [nvox], zeroed by the call on `stream`.  Integer adds: exact and order-independent.  1 <= nvox <= 2^31 - 2; 4-byte aligned. */
int vittf_component_sizes(const int32_t* labels, int64_t nvox, int32_t* sizes, void* stream);

/* dst[v] = src[v] where labels[v] != 0 and the component is kept, else fill (0..255).  keep_label > 0: the component with that
 * label is kept (sizes may be NULL); keep_label == 0: every component with sizes[labels[v] - 1] >= min_size.  One pass; dst may
 * equal src.  labels, sizes: 4-byte aligned. */
int vittf_filter_components(const uint8_t* src, const int32_t* labels, const int32_t* sizes, int64_t nvox, int32_t min_size,
                            int32_t keep_label, int32_t fill, uint8_t* dst, void* stream);

/* ---- exact Euclidean distance transform of a uint8 volume (vit-tf_amd/distance.py, score_labels.py) ----------------------
 * A SITE is a voxel of the set that `value` selects -- 0..255: {src == value}; -1: {src != 0}, the select of
 * vittf_label_components without its -2 -- with mode 0, or of its complement with mode 1 ({src != value}; {src == 0} for -1).
 * d2_out (n0, n1, n2): for every voxel the squared Euclidean distance to the nearest site, 0 on a site
 * (scipy.ndimage.distance_transform_edt(~sites) ** 2).  site_out, unless NULL: int32 (n0, n1, n2), the linear index
 * (i0 * n1 + i1) * n2 + i2 of a site at that distance (the feature transform); among several nearest sites the one the fixed
 * walk meets, not necessarily scipy's.  A volume without a site: VITTF_EDT_NO_SITE on every voxel (+inf in the fp32 output), -1
 * in site_out, and the call returns VITTF_OK.  No atomics, every output is stored once: the same input gives the same bytes.
 *
 * vittf_edt_sq: unit spacing.  d2_out int32, exact (int32 arithmetic, at most 3 x 2047^2).
 * vittf_edt_sq_weighted: d2 = sum_a w2_host[a] (x_a - s_a)^2, w2_host = the three squared voxel spacings (host doubles, finite
 * and > 0).  fp64 arithmetic, rounded once to fp32: |d2_out - exact| <= 2^-24 exact + 2^-40 sum_a w2[a] (n_a - 1)^2.  With
 * weights (1, 1, 1) it equals vittf_edt_sq converted to fp32.
 *
 * Every dimension in 1..VITTF_EDT_MAX_DIM and n0 n1 n2 < 2^31; value in -1..255; mode 0 or 1; src, d2_out, ws not NULL; d2_out
 * and site_out 4-byte aligned, ws 8-byte aligned; anything else: VITTF_ERR_INVALID_ARG without a launch.  ws >=
 * vittf_edt_workspace_bytes(n0, n1, n2) = 8 + 4 bytes per voxel, each part rounded up to 256 (0 for a shape the call refuses), the
 * same for both entries; too small: VITTF_ERR_WORKSPACE.  src may sit at any byte alignment.
 * Three launches: axis 2 by wave ballots and scans, then axis 1 and axis 0 as lower envelopes of parabolas (Meijster et al.
 * 2000) on tiles of adjacent lines in LDS, as many lines as 80 KiB hold at n (4 or 8 + 4) bytes each. */
#define VITTF_EDT_MAX_DIM 2048
#define VITTF_EDT_NO_SITE 2147483647
size_t vittf_edt_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int vittf_edt_sq(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t value, int32_t mode, int32_t* d2_out,
                 int32_t* site_out, void* ws, size_t ws_bytes, void* stream);
int vittf_edt_sq_weighted(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t value, int32_t mode,
                          const double* w2_host, float* d2_out, int32_t* site_out, void* ws, size_t ws_bytes, void* stream);

/* ---- direct volume rendering of an intensity volume with class maps as opacity (vit-tf_amd/render.py, render_volume.py) ----
 * The model (tests/render_data.py restates it in fp64):
 * Coordinates.  World box [0, n_a s_a] along volume axis a, the centre of voxel i at (i + 0.5) s_a: index coordinate x_a =
 *   p_a / s_a - 0.5.  The class maps live on their own grid (m0, m1, m2) over the same box: x_a = p_a / (n_a s_a) m_a - 0.5.
 * Intensity.  q = rint(65535 clamp((V - vmin) / (vmax - vmin), 0, 1)) as uint16, computed in fp64 (vittf_render_prepare).  A
 *   sample's intensity is the border-clamped trilinear value of q, clamped to the range of its eight corners (what exact
 *   arithmetic gives anyway).
 * Transfer function.  table: 256 entries of fp32 (r, g, b, sigma) on the device, linear between entries, read at q / 257
 *   (65535 = 255 x 257); sigma is extinction per world unit, finite and >= 0.
 * Classes.  0..VITTF_RENDER_MAX_CLASSES uint8 maps (C, m0, m1, m2).  value = border-clamped trilinear map value in levels
 *   0..255 (clamped to its corners' range), omega_c = clamp((value - lo_c) / (hi_c - lo_c), 0, 1) with integers 0 <= lo_c <
 *   hi_c <= 255, sigma_c = strength_c omega_c with colour rgb_c; class_rgbs_host holds (r, g, b, strength) per class.
 * Coverage.  Every sigma of a sample is multiplied by the sum of the trilinear weights of its in-bounds corners of the
 *   intensity grid: 1 inside the hull of voxel centres, 0 from half a voxel outside the box on.
 * Rays.  Pixel (x, y) of width x height: u = 2 (x + 0.5) / width - 1, v = 1 - 2 (y + 0.5) / height, origin eye + u ox + v oy,
 *   direction normalize(fwd + u dx + v dy); camera_host = {eye, ox, oy, fwd, dx, dy}, 18 floats in world units.  The ray
 *   interval is the slab intersection with the box grown by half a voxel, clipped to t >= 0; samples sit on the global lattice
 *   t_i = (i + 0.5) dt.  A ray that misses stores 0, 0, 0, 0; a zero direction component is handled without a division.
 * Compositing, front to back with sigma = sum_k sigma_k over the table and the classes: a = 1 - exp(-sigma dt), rgb += T a
 *   shade (sum_k sigma_k rgb_k) / max(sigma, 1e-30), A += T a, T *= 1 - a, the ray ends when T < 2^-10.  A sample with sigma
 *   == 0 changes nothing.  rgba_out: premultiplied fp32 (height, width, 4), every pixel stored.
 * Shading.  shade_host = {ka, kd, eps}: shade = ka + kd |g . d| / (|g| + eps), g_a = (I(x + e_a) - I(x - e_a)) / (2 s_a) from
 *   the border-clamped trilinear intensity (in levels of q) one voxel either way with the centre sample's fractions (24 more
 *   voxels); kd == 0 fetches none of them.  ka, kd >= 0, eps > 0.
 * Occupancy (vittf_render_occupancy).  One byte per 8^3 brick of the intensity grid, (ceil(n0 / 8), ceil(n1 / 8), ceil(n2 /
 *   8)), 0 = empty.  A sample belongs to the brick of clamp(floor(x_a), 0, n_a - 1) div 8.  A brick is empty when (1) every
 *   table entry from qmin div 257 to min(255, qmax div 257 + 1) has sigma == 0, qmin and qmax over voxels 8 b_a .. min(8 b_a +
 *   8, n_a - 1), and (2) every class has its map maximum <= lo_c over the map voxels max(0, ((8 b_a - 1) m_a) div n_a - 1)
 *   .. min(m_a - 1, ((8 b_a + 10) m_a) div n_a + 1) per axis: a sample of the brick has p_a / s_a in [8 b_a, 8 b_a + 9); the
 *   rule widens that by one voxel either way, far more than the rounding of the fp32 map coordinate, and takes the floor of
 *   the map coordinate at the lower end and its upper corner at the upper end.  vittf_render with occ jumps over runs of
 *   samples it has proved to lie in empty bricks and gives the same bytes as with occ == NULL.
 *
 * Every dimension of the volume and of the map grid in 2..VITTF_RENDER_MAX_DIM, fewer than 2^31 voxels each; width and height
 * in 1..VITTF_RENDER_MAX_IMAGE; spacing finite and > 0; dt finite and > 0 and fewer than 2^22 lattice samples between a ray
 * origin and the far side of the box; camera finite with fwd != 0; table 16-byte aligned, rgba_out 16-byte aligned, the
 * volume of vittf_render_prepare 16-byte and q there 8-byte aligned; anything else: VITTF_ERR_INVALID_ARG without a launch.
 * maps, lo_host, hi_host, class_rgbs_host may be NULL with classes == 0.  vittf_render_occupancy_bytes: the bricks of a
 * volume, 0 for a shape the calls refuse.  No atomics, every output stored once: the same call gives the same bytes. */
#define VITTF_RENDER_MAX_DIM 2048
#define VITTF_RENDER_MAX_IMAGE 8192
#define VITTF_RENDER_MAX_CLASSES 8
int vittf_render_prepare(const float* volume, int64_t nvox, double vmin, double vmax, uint16_t* q, void* stream);
size_t vittf_render_occupancy_bytes(int32_t n0, int32_t n1, int32_t n2);
int vittf_render_occupancy(const uint16_t* q, int32_t n0, int32_t n1, int32_t n2, const float* table, const uint8_t* maps,
                           int32_t classes, int32_t m0, int32_t m1, int32_t m2, const int32_t* lo_host, uint8_t* occ,
                           void* stream);
int vittf_render(const uint16_t* q, int32_t n0, int32_t n1, int32_t n2, const float* spacing_host, const float* table,
                 const uint8_t* maps, int32_t classes, int32_t m0, int32_t m1, int32_t m2, const int32_t* lo_host,
                 const int32_t* hi_host, const float* class_rgbs_host, const uint8_t* occ, const float* camera_host,
                 int32_t width, int32_t height, float dt, const float* shade_host, float* rgba_out, void* stream);

/* F.interpolate(mode='nearest') of a uint8 volume (n0, n1, n2) -> (o0, o1, o2): src index = min(floor(dst * (float)in /
 * out), in - 1) per dim.  equals < 0: plain resize -- the label up-sample of predict_ntf.py:217-218; equals = c in 0..255:
 * the resized class mask (src == c) as 0/1 -- evaluate_similarities.py:63 without materialising the full-size mask. */
int vittf_resize_nearest_u8(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, uint8_t* dst, int32_t o0, int32_t o1,
                            int32_t o2, int32_t equals, void* stream);

/* dst fp32 [n] = src fp16 [n] (exact): volumes are stored as fp16 (create_synthetic_volumes.py:44-46) and uploaded as
 * such; the vol.float() of infer.py:137 / the astype(np.float32) of infer.py:230-232 happens in HBM.  16-byte aligned. */
int vittf_widen_f16(const uint16_t* src, int64_t n, float* dst, void* stream);

/* ---- 3-D bilateral solver post-process (bilateral_solver3d.py, predict_ntf.py:73-96) ---------- */
typedef struct vittf_bilateral_params {
  double sigma_spatial;        /* grid_params['sigma_spatial'] (predict_ntf.py:75-79: 7) */
  double lam;                  /* bs_params_default (bilateral_solver3d.py:162-167): 256 */
  double a_diag_min;           /* 1e-5 */
  double cg_tol;               /* 1e-5, relative to |b| (scipy cg rtol) */
  int32_t cg_maxiter;          /* 25 */
  int32_t bistochastize_iters; /* 10 (bilateral_solver3d.py:107) */
  int32_t pad;                 /* crop_pad(..., pad=2) (predict_ntf.py:90) */
  float crop_threshold;        /* crop_pad(..., thresh=0.1) */
} vittf_bilateral_params;

/* luma_bins = 1 + the largest luma bin; 0 = unsupported size. */
size_t vittf_bilateral_workspace_bytes(int32_t o0, int32_t o1, int32_t o2, double sigma_spatial, int32_t luma_bins);

/* One class of predict_ntf.py:80-94: volume (v0, v1, v2) fp32 and the class map sim_in (n0, n1, n2) fp32 are resized
 * (trilinear) to (o0, o1, o2); the volume becomes the uint8 grey reference (min-max); the box where sim > crop_threshold
 * (+ pad) is refined by the bilateral solver with the Sobel confidence and written back.  sim_out: fp32 (o0, o1, o2).
 * [host] luma_bin_host[256]: bilateral-space luma bin of each grey level, (rgb2yuv(v, v, v)[0] / sigma_luma).astype(int)
 * (bilateral_solver3d.py:19-20, 47); the chroma bins are constant for a grey reference and drop out.
 * [host] info_host (nullable): {vertices, voxels in the crop box}; {0, 0} when nothing exceeds the threshold (the map is
 * then returned unrefined; the reference raises in that case).  Synchronises the stream twice (box, vertex count). */
int vittf_bilateral_refine(const float* sim_in, int32_t n0, int32_t n1, int32_t n2, const float* volume, int32_t v0,
                           int32_t v1, int32_t v2, int32_t o0, int32_t o1, int32_t o2, const int32_t* luma_bin_host,
                           int32_t luma_bins, const vittf_bilateral_params* prm, float* sim_out, int32_t* info_host,
                           void* ws, size_t ws_bytes, void* stream);

/* (255 / (0.99 * max(sim)) * sim).to(uint8) with the x86 wrap-around (predict_ntf.py:95-96).  max_scratch: 4 device bytes. */
int vittf_quantize_wrap_u8(const float* sim, int64_t n, uint8_t* out, float* max_scratch, void* stream);

/* pred = 0; best = 0; for i: mask = sims[i] > thr[i] && sims[i] > best; pred[mask] = i+1; best[mask] = sims[i]
 * sims uint8 [classes][n]; thr int32 [classes] on the HOST (= int(t*255), predict_ntf.py:212); labels uint8 [n]. */
int vittf_assign_labels(const uint8_t* sims, int32_t classes, int64_t n, const int32_t* thr_host, uint8_t* labels,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITTF_H */
