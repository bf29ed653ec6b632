// MLP head over every voxel of an F-major fp16 feature volume [f][nvox] (vit-tf_amd/mlp.py fits the head on the host;
// classify_features.py --classifier mlp is the command line): Linear (-> ReLU -> Linear){0..2}, the arg-max of the logits
// and, when asked for, the logits and the uint8 softmax.  The head has M = layers + 1 matrices W_0 .. W_layers, fp32
// [out][in], in_0 = f, out_last = classes, the hidden widths multiples of 32 in 32..256.
//
// Layout.  A workgroup of 4 waves owns 128 voxels, a wave 32 of them; every matrix is the A operand of
// v_mfma_f32_32x32x16_f16 in blocks of 32 output rows, the voxels are the columns, so a lane's accumulator registers hold
// 16 rows (acc_row(r, h)) of its OWN voxel.  The prep kernel writes every matrix into the workspace as "parts" of 32
// contraction indices: [32 blk rows][32 k] fp16 hi, then the same lo, 80-byte rows -- the LDS image the workgroups copy as
// it lies.  The rows behind `out` are zeros.
//
// Arithmetic, as built:
//   scale    per matrix a power of two 2^e with max |W| 2^-e in [2^10, 2^11) (1 for a zero matrix): W' = W 2^-e, exact
//   split    W' = hi + lo, hi = fp16(W'), lo = fp16(W' - hi): |W' - hi - lo| <= 2^-22 |W'| + 2^-25 (the second term is the
//            fp16 subnormal spacing: 2^-35 of the largest entry)
//   layer 0  acc = sum_k hi x + sum_k lo x, the voxels' fp16 features exact operands (feat_rows.h's transposing pickup), fp32
//            accumulation, k ascending in steps of 16, hi before lo inside a step
//   epilogue z = fmaf(acc * colmul, 2^e, bias): colmul = 1 / voxel_norm[v] (layer 0 with norms), 1 (without) or the
//            hand-over's 2^s (later layers)
//   hand-over (range-safe) a = max(z, 0); per VOXEL m = max_j a_j and s = max(floor(log2 m) - 10, -116), a' = a 2^-s (exact;
//            m 2^-s in [2^10, 2^11)), a' = ahi + alo split as the weights.  The accumulator registers ARE the B operand of the
//            next contraction: its k index runs in accumulator-row order, which the prep kernel bakes into the images
//            (k = 32 part + acc_row(8 ks + j, h) at position 16 ks + 8 h + j), as svm.hip does for its coefficients.
//   layer>0  acc = sum hi ahi + hi alo + lo ahi (lo alo, <= 2^-22 relative, is left out), parts ascending, fp32; the next
//            weight image is register-prefetched while the matrix cores work on the current one
//   labels   arg-max of the fp32 logits, strict > from class 0 up: the lowest index among equals
//   probs    t_c = (z_c - max z) * log2(e) (fp32), e_c = v_exp_f32(t_c), S = e_0 + e_1 + ... in class order, p = e_c / S,
//            probs = (uint8) fmaf(255, p, 0.5)
// Hidden activations live in registers only.  Fixed order, no atomics: the same call gives the same bytes.  Three launches
// (scales, images, decision).
#include "vittf_common.h"
#include "feat_rows.h"

namespace {

constexpr int ML_THREADS = 256, ML_WAVES = 4;
constexpr int ML_VOX = 32 * ML_WAVES;          // voxels per workgroup
constexpr int ML_VROW = 2 * ML_VOX + 64;       // LDS bytes per staged feature row of the pickup
constexpr int ML_CROW = 2 * 32 + 16;           // LDS bytes per weight row of a part (hi or lo)
constexpr int ML_BLOCK = 2 * 32 * ML_CROW;     // image bytes of a part per block of 32 output rows (hi + lo)
constexpr int ML_HEADER = 256;                 // workspace bytes in front of the images: {2^e, 2^-e} per matrix
constexpr int ML_MAX_MATS = VITTF_MLP_MAX_LAYERS + 1;

struct MlpDesc {
  int n;                                       // matrices
  int in[ML_MAX_MATS], out[ML_MAX_MATS], blk[ML_MAX_MATS];       // blk = ceil(out / 32)
  int w_off[ML_MAX_MATS], b_off[ML_MAX_MATS];  // in floats
  int part0[ML_MAX_MATS + 1];                  // first part of the matrix among all parts
  int64_t img_off[ML_MAX_MATS + 1];            // bytes behind the header
};

static bool mlp_classes_ok(int32_t c) { return c >= 2 && c <= VITTF_MLP_MAX_CLASSES; }
static bool mlp_width_ok(int32_t w) { return w >= 32 && w <= VITTF_MLP_MAX_WIDTH && w % 32 == 0; }

static bool mlp_describe(int32_t f, const int32_t* widths, int32_t layers, int32_t classes, MlpDesc& d) {
  if (!feat_f_ok(f) || layers < 0 || layers > VITTF_MLP_MAX_LAYERS || !mlp_classes_ok(classes) || (layers > 0 && !widths)) return false;
  for (int l = 0; l < layers; ++l)
    if (!mlp_width_ok(widths[l])) return false;
  d.n = layers + 1;
  int w = 0, b = 0, p = 0;
  int64_t img = 0;
  for (int l = 0; l < ML_MAX_MATS; ++l) {
    if (l < d.n) {
      d.in[l] = l ? widths[l - 1] : f;
      d.out[l] = l < layers ? widths[l] : classes;
    } else {
      d.in[l] = 0;
      d.out[l] = 0;
    }
    d.blk[l] = (d.out[l] + 31) / 32;
    d.w_off[l] = w;
    d.b_off[l] = b;
    d.part0[l] = p;
    d.img_off[l] = img;
    w += d.in[l] * d.out[l];
    b += d.out[l];
    p += d.in[l] / 32;
    img += (int64_t)(d.in[l] / 32) * d.blk[l] * ML_BLOCK;
  }
  d.part0[ML_MAX_MATS] = p;
  d.img_off[ML_MAX_MATS] = img;
  return true;
}

// ------------------------------------------------------------------------------------------------ scales and images
// grid: matrices.  hdr[2 l] = 2^e with max |W_l| 2^-e in [2^10, 2^11) (1 for a zero matrix), hdr[2 l + 1] = 2^-e.
__global__ __launch_bounds__(1024) void mlp_scale_kernel(const float* __restrict__ weights, MlpDesc d, float* __restrict__ hdr) {
  __shared__ float part[1024];
  const int l = blockIdx.x;
  const float* w = weights + d.w_off[l];
  const int n = d.in[l] * d.out[l];
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(w[i]));
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmaxf(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int e = 11;
    if (part[0] > 0.f && part[0] < __builtin_inff()) frexpf(part[0], &e);
    e -= 11;
    e = e < -120 ? -120 : e > 120 ? 120 : e;
    hdr[2 * l] = ldexpf(1.f, e);
    hdr[2 * l + 1] = ldexpf(1.f, -e);
  }
}

// grid: all parts of all matrices.  Position q of a row <-> contraction index 32 part + q (matrix 0: the pickup's order) or
// 32 part + acc_row(8 ks + j, h), q = 16 ks + 8 h + j (later matrices: the accumulator's row order).
__global__ __launch_bounds__(ML_THREADS) void mlp_prep_kernel(const float* __restrict__ weights, MlpDesc d, char* __restrict__ ws) {
  const int tid = threadIdx.x;
  int l = 0;
  while (l + 1 < d.n && (int)blockIdx.x >= d.part0[l + 1]) ++l;
  const int part = blockIdx.x - d.part0[l];
  const int rows = 32 * d.blk[l];
  char* img = ws + ML_HEADER + d.img_off[l] + (int64_t)part * d.blk[l] * ML_BLOCK;
  const float inv_scale = reinterpret_cast<const float*>(ws)[2 * l + 1];
  const float* w = weights + d.w_off[l];
  for (int i = tid; i < rows * 32; i += ML_THREADS) {
    const int p = i >> 5, q = i & 31;
    const int ks = q >> 4, h = (q >> 3) & 1, j = q & 7;
    const int k = 32 * part + (l ? acc_row(8 * ks + j, h) : q);
    const float c = p < d.out[l] ? w[p * d.in[l] + k] * inv_scale : 0.f;
    const unsigned short hi = f32_to_f16bits(c);
    const unsigned short lo = f32_to_f16bits(c - f16bits_to_f32(hi));
    *reinterpret_cast<unsigned short*>(img + p * ML_CROW + 2 * q) = hi;
    *reinterpret_cast<unsigned short*>(img + (rows + p) * ML_CROW + 2 * q) = lo;
  }
  for (int i = tid; i < 2 * rows; i += ML_THREADS)     // the 16 bytes behind every row
    *reinterpret_cast<uint4*>(img + i * ML_CROW + 64) = make_uint4(0u, 0u, 0u, 0u);
}

// ------------------------------------------------------------------------------------------------ the contractions
// matrix 0: acc[b][r] = sum_k W'[32 b + acc_row(r, h)][k] x[k][v] over the f / 32 parts of the image sequence `img`; the
// feature rows and the next image are register-prefetched one part ahead
template <int RB>
__device__ __forceinline__ void first_contract(const unsigned short* __restrict__ feat, int f, int64_t nvox, bool aligned, int64_t v0,
                                               const char* __restrict__ img, int nb, char* vbuf, char* cbuf, f32x16_t (&acc)[RB]) {
  constexpr int PRE = (RB * (ML_BLOCK / 16) + ML_THREADS - 1) / ML_THREADS;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int parts = f / 32;
  const int pieces = nb * (ML_BLOCK / 16);
  const int lo_off = 32 * nb * ML_CROW;
  i32x4_t pre[2], cpre[PRE];                         // (native vectors: hipcc keeps an array of HIP uint4 structs in scratch)
  auto prefetch = [&](int part) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + ML_THREADS * j;
      const unsigned short* row = feat + (int64_t)(part * 32 + (i >> 4)) * nvox;
      const uint4 c = aligned ? feat_load8<true>(row, v0 + 8 * (i & 15), nvox) : feat_load8<false>(row, v0 + 8 * (i & 15), nvox);
      pre[j] = i32x4_t{(int)c.x, (int)c.y, (int)c.z, (int)c.w};
    }
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
      const int i = tid + ML_THREADS * j;              // spare lanes of the last round load a piece twice
      cpre[j] = reinterpret_cast<const i32x4_t*>(img + (int64_t)part * pieces * 16)[i < pieces ? i : pieces - 1];
    }
  };
  const int tr_off = tr_lane_offset<ML_VROW>(lane, wave);
  const int a_off = l31 * ML_CROW + 16 * h;
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  prefetch(0);
  for (int part = 0; part < parts; ++part) {
    __syncthreads();                                   // the previous part's fragments have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + ML_THREADS * j;
      *reinterpret_cast<i32x4_t*>(vbuf + (i >> 4) * ML_VROW + 16 * (i & 15)) = pre[j];
    }
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
      const int i = tid + ML_THREADS * j;
      if (i < pieces) reinterpret_cast<i32x4_t*>(cbuf)[i] = cpre[j];
    }
    __syncthreads();
    if (part + 1 < parts) prefetch(part + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const s16x8_t x = tr_fragment<ML_VROW>(vbuf + tr_off + (16 * s) * ML_VROW);
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        if (b < nb) {
          const char* cb = cbuf + (32 * b) * ML_CROW + a_off + 32 * s;
          const s16x8_t ch = *reinterpret_cast<const s16x8_t*>(cb);
          const s16x8_t cl = *reinterpret_cast<const s16x8_t*>(cb + lo_off);
          acc[b] = mfma32<VITTF_FP16>(ch, x, acc[b]);
          acc[b] = mfma32<VITTF_FP16>(cl, x, acc[b]);
        }
      }
    }
  }
}

// epilogue + ReLU + the per-voxel power-of-two scale of the hand-over: acc becomes a 2^-s, the return value is 2^s
template <int RB>
__device__ __forceinline__ float activate(f32x16_t (&acc)[RB], int nb, float colmul, float scale, const float* __restrict__ bias, int h) {
  float m = 0.f;
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    if (b < nb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a = fmaxf(fmaf(acc[b][r] * colmul, scale, bias[32 * b + acc_row(r, h)]), 0.f);
        acc[b][r] = a;
        m = fmaxf(m, a);
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32));                      // the other 16 rows of every block of this voxel
  int s = (int)((__float_as_uint(m) >> 23) & 0xffu) - 127 - 10;
  s = s < -116 ? -116 : s;
  const float dn = __uint_as_float((unsigned)(127 - s) << 23);
#pragma unroll
  for (int b = 0; b < RB; ++b)
    if (b < nb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] *= dn;
    }
  return __uint_as_float((unsigned)(127 + s) << 23);
}

// a later matrix: out[ob][r] = sum_k W'[32 ob + acc_row(r, h)][k] a'[k][v], the activations taken from the accumulator
// tiles `in` as they lie (block b of them is part b of the image sequence `img`)
template <int RBI, int RBO>
__device__ __forceinline__ void hidden_contract(const f32x16_t (&in)[RBI], int nbi, f32x16_t (&out)[RBO], int nbo,
                                                const char* __restrict__ img, char* cbuf) {
  constexpr int PRE = (RBO * (ML_BLOCK / 16) + ML_THREADS - 1) / ML_THREADS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int h = lane >> 5, l31 = lane & 31;
  const int pieces = nbo * (ML_BLOCK / 16);
  const int lo_off = 32 * nbo * ML_CROW;
  const int a_off = l31 * ML_CROW + 16 * h;
  i32x4_t cpre[PRE];                                   // the next image, register-prefetched one part ahead
  auto prefetch = [&](int part) {
#pragma unroll
    for (int j = 0; j < PRE; ++j) {
      const int i = tid + ML_THREADS * j;              // spare lanes of the last round load a piece twice
      cpre[j] = reinterpret_cast<const i32x4_t*>(img + (int64_t)part * pieces * 16)[i < pieces ? i : pieces - 1];
    }
  };
#pragma unroll
  for (int b = 0; b < RBO; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[b][r] = 0.f;
  prefetch(0);
#pragma unroll
  for (int b = 0; b < RBI; ++b) {
    if (b < nbi) {
      __syncthreads();                                 // the previous image has been read
#pragma unroll
      for (int j = 0; j < PRE; ++j) {
        const int i = tid + ML_THREADS * j;
        if (i < pieces) reinterpret_cast<i32x4_t*>(cbuf)[i] = cpre[j];
      }
      __syncthreads();
      if (b + 1 < nbi) prefetch(b + 1);
      s16x8_t kh[2], kl[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a = in[b][r];
        const unsigned short hi = f32_to_f16bits(a);
        kh[r >> 3][r & 7] = (short)hi;
        kl[r >> 3][r & 7] = (short)f32_to_f16bits(a - f16bits_to_f32(hi));
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int ob = 0; ob < RBO; ++ob) {
          if (ob < nbo) {
            const char* cb = cbuf + (32 * ob) * ML_CROW + a_off + 32 * s;
            const s16x8_t ch = *reinterpret_cast<const s16x8_t*>(cb);
            const s16x8_t cl = *reinterpret_cast<const s16x8_t*>(cb + lo_off);
            out[ob] = mfma32<VITTF_FP16>(ch, kh[s], out[ob]);
            out[ob] = mfma32<VITTF_FP16>(ch, kl[s], out[ob]);
            out[ob] = mfma32<VITTF_FP16>(cl, kh[s], out[ob]);
          }
        }
      }
    }
  }
}

// the logits of the lane's voxel from the last accumulator tile (rows 4 h .. 4 h + 3 of the first 8 are the lane's own, the
// other four come from lane ^ 32), the arg-max, and the softmax from the same registers
__device__ __forceinline__ void finish(f32x16_t acc, float colmul, float scale, const float* __restrict__ bias, int classes,
                                       unsigned char* lab, int64_t v0, int64_t nvox, unsigned char* __restrict__ labels,
                                       float* __restrict__ logits, unsigned char* __restrict__ probs) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v = v0 + wave * 32 + l31;
  float own[4], z[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 4 * h + i;
    own[i] = c < classes ? fmaf(acc[i] * colmul, scale, bias[c]) : -__builtin_inff();
    if (logits && c < classes && v < nvox) logits[(int64_t)c * nvox + v] = own[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float other = __shfl_xor(own[i], 32);
    z[i] = h ? other : own[i];
    z[4 + i] = h ? own[i] : other;
  }
  float best = z[0];
  int bi = 0;
#pragma unroll
  for (int c = 1; c < 8; ++c)
    if (z[c] > best) { best = z[c]; bi = c; }            // strict: the lowest index wins a tie
  if (probs) {
    float e[8], sum = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      e[c] = c < classes ? __builtin_amdgcn_exp2f((z[c] - best) * 1.44269504088896340736f) : 0.f;
      sum += e[c];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 4 * h + i;
      const float p = __builtin_amdgcn_exp2f((own[i] - best) * 1.44269504088896340736f) / sum;      // = e[c], the same bits
      if (c < classes && v < nvox) probs[(int64_t)c * nvox + v] = (unsigned char)(int)fmaf(255.f, p, 0.5f);
    }
  }
  if (h == 0) lab[wave * 32 + l31] = (unsigned char)bi;
  __syncthreads();
  if (tid < ML_VOX / 4) {
    const int64_t vq = v0 + 4 * tid;
    if ((((uintptr_t)labels) & 3) == 0 && vq + 3 < nvox) {
      *reinterpret_cast<unsigned*>(labels + vq) = *reinterpret_cast<const unsigned*>(lab + 4 * tid);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (vq + j < nvox) labels[vq + j] = lab[4 * tid + j];
    }
  }
}

// RB: row blocks of the widest hidden layer, rounded up to 1, 2, 4 or 8 (1 for LAYERS = 0)
template <int LAYERS, int RB>
__global__ __launch_bounds__(ML_THREADS) void mlp_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox, int aligned,
                                                         const char* __restrict__ ws, MlpDesc d, const float* __restrict__ biases,
                                                         int classes, const float* __restrict__ voxel_norm,
                                                         unsigned char* __restrict__ labels, float* __restrict__ logits,
                                                         unsigned char* __restrict__ probs) {
  __shared__ __attribute__((aligned(16))) char vbuf[32 * ML_VROW];
  __shared__ __attribute__((aligned(16))) char cbuf[RB * ML_BLOCK];
  __shared__ __attribute__((aligned(4))) unsigned char lab[ML_VOX];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5;
  const int64_t v0 = (int64_t)blockIdx.x * ML_VOX;
  const int64_t v = v0 + wave * 32 + (lane & 31);
  const float* hdr = reinterpret_cast<const float*>(ws);
  const char* images = ws + ML_HEADER;
  const float inv = (voxel_norm && v < nvox) ? 1.f / voxel_norm[v] : 1.f;
  f32x16_t a0[RB];
  first_contract<RB>(feat, f, nvox, aligned != 0, v0, images, d.blk[0], vbuf, cbuf, a0);
  if constexpr (LAYERS == 0) {
    finish(a0[0], inv, hdr[0], biases, classes, lab, v0, nvox, labels, logits, probs);
  } else {
    const float up0 = activate<RB>(a0, d.blk[0], inv, hdr[0], biases + d.b_off[0], h);
    if constexpr (LAYERS == 1) {
      f32x16_t z[1];
      hidden_contract<RB, 1>(a0, d.blk[0], z, 1, images + d.img_off[1], cbuf);
      finish(z[0], up0, hdr[2], biases + d.b_off[1], classes, lab, v0, nvox, labels, logits, probs);
    } else {
      f32x16_t a1[RB];
      hidden_contract<RB, RB>(a0, d.blk[0], a1, d.blk[1], images + d.img_off[1], cbuf);
      const float up1 = activate<RB>(a1, d.blk[1], up0, hdr[2], biases + d.b_off[1], h);
      f32x16_t z[1];
      hidden_contract<RB, 1>(a1, d.blk[1], z, 1, images + d.img_off[2], cbuf);
      finish(z[0], up1, hdr[4], biases + d.b_off[2], classes, lab, v0, nvox, labels, logits, probs);
    }
  }
}

}  // namespace

size_t vittf_mlp_workspace_bytes(int32_t f, const int32_t* widths, int32_t layers, int32_t classes) {
  MlpDesc d;
  if (!mlp_describe(f, widths, layers, classes, d)) return 0;
  return ML_HEADER + (size_t)d.img_off[ML_MAX_MATS];
}

int vittf_mlp_decide(const uint16_t* feat, int32_t f, int64_t nvox, const float* weights, const float* biases,
                     const int32_t* widths, int32_t layers, int32_t classes, const float* voxel_norm, uint8_t* labels,
                     float* logits, uint8_t* probs, void* ws, size_t ws_bytes, void* stream) {
  if (!feat || !weights || !biases || !labels || !ws || nvox < 1) return VITTF_ERR_INVALID_ARG;
  MlpDesc d;
  if (!mlp_describe(f, widths, layers, classes, d)) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)weights & 3) || ((uintptr_t)biases & 3) || ((uintptr_t)voxel_norm & 3) ||
      ((uintptr_t)logits & 3) || ((uintptr_t)ws & 15))
    return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + ML_VOX - 1) / ML_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < ML_HEADER + (size_t)d.img_off[ML_MAX_MATS]) return VITTF_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mlp_scale_kernel, dim3((unsigned)d.n), dim3(1024), 0, st, weights, d, (float*)ws);
  hipLaunchKernelGGL(mlp_prep_kernel, dim3((unsigned)d.part0[ML_MAX_MATS]), dim3(ML_THREADS), 0, st, weights, d, (char*)ws);
  const int al = rows_aligned(feat, nvox) ? 1 : 0;
  int widest = 1;
  for (int l = 0; l < layers; ++l) widest = d.blk[l] > widest ? d.blk[l] : widest;
#define ML_LAUNCH(LY, RBV) \
  hipLaunchKernelGGL((mlp_kernel<LY, RBV>), dim3((unsigned)wgs), dim3(ML_THREADS), 0, st, feat, f, nvox, al, (const char*)ws, d, biases, \
                     classes, voxel_norm, labels, logits, probs)
#define ML_PICK(LY) do { if (widest <= 1) ML_LAUNCH(LY, 1); else if (widest <= 2) ML_LAUNCH(LY, 2); else if (widest <= 4) ML_LAUNCH(LY, 4); \
                         else ML_LAUNCH(LY, 8); } while (0)
  if (layers == 0) ML_LAUNCH(0, 1); else if (layers == 1) ML_PICK(1); else ML_PICK(2);
#undef ML_PICK
#undef ML_LAUNCH
  return vittf_check_launch();
}
