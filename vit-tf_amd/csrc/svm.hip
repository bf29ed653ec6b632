// One-vs-one C-SVC decision of every voxel of an F-major fp16 feature volume [f][nvox] (vit-tf_amd/svm.py fits the model
// on the host; classify_features.py is the command line).  classes = C in 2..8, pairs p = (i, j) in the order (0,1), (0,2),
// ..., (C-2,C-1); dec_p > 0 votes for i, anything else for j; the class with the most votes wins, the lowest index among
// equal counts.
//
// vittf_svm_rbf_decide: dec_p(x) = sum_s coef[p][s] exp(-gamma |x - sv_s|^2) + b_p on the frame of bank_frame.h: the voxels
// stay where they are as MFMA B operands, the support vectors stream past in chunks of 32 through the ring of LDS images.  An
// image holds [32 sv][FP] fp16 rows (the support vectors ARE fp16: no split), the chunk's coefficients as fp16 hi + lo A
// fragments, and |sv|^2 in fp32.  Per chunk and wave:
//   1. acc[sv][voxel] = sv . x                                     chunk_dots
//   2. d2 = max(|x|^2 + |sv|^2 - 2 sv . x, 0);  K = exp2(-gamma log2(e) d2)         (|x|^2 from the wave's own registers)
//   3. the accumulator tile holds 16 support-vector rows of the lane's OWN voxel: K (as fp16 hi + lo, 2^-22) is a B operand
//      as it lies, with the k index of the second contraction permuted to the accumulator's row order -- the prep kernel
//      writes the coefficients in that order (attention_pp64.hip feeds P into its second MFMA the same way)
//   4. dec[pair][voxel] += coef_hi K_hi + coef_hi K_lo + coef_lo K_hi                6 MFMAs
// The coefficients are scaled by a power of two (the scale kernel: 2^e > max |coef|) so that their halves cannot leave the
// fp16 range; the scale is multiplied back, exactly, when the intercept is added.  n_sv is padded to the chunk with ZERO
// COEFFICIENTS (a zero support vector still has K = exp(-gamma |x|^2), not 0).  Fixed summation order, no atomics: the same
// call gives the same bytes.
//
// vittf_svm_linear_decide: dec_p(x) = w_p . x + b_p, the score loop project_scores<.., 1> of feat_rows.h (w as fp16 hi + lo).
//
// Both end in vote_epilogue: a lane holds the decisions of 16 of the 32 pair rows of its voxel (rows acc_row(r, h)), lanes l
// and l + 32 the two halves; eight 4-bit vote counters share one 32-bit word, one __shfl_xor(.., 32) and one add combine the
// halves.  The decisions are written (when asked for) from the very registers the vote reads.
#include "vittf_common.h"
#include "bank_frame.h"

namespace {

constexpr int SVM_MAX_PAIRS = VITTF_SVM_MAX_CLASSES * (VITTF_SVM_MAX_CLASSES - 1) / 2;    // 28 <= 32: one accumulator tile
constexpr int SV_CROW = 2 * BK_CHUNK + 16;     // LDS bytes per coefficient row (hi or lo) of a chunk
constexpr int SV_HEADER = 256;                 // workspace bytes in front of the images: {scale, 1 / scale}
static_assert(SVM_MAX_PAIRS <= 32, "the decisions of a voxel fill one 32-row tile");

// image of a chunk: [32 sv rows of 2 FP + 16 bytes][32 coefficient rows hi][32 lo][32 x |sv|^2 fp32]
__host__ __device__ constexpr int sv_image_bytes(int fp) { return BK_CHUNK * bank_row_bytes(fp) + 2 * 32 * SV_CROW + 4 * BK_CHUNK; }

static bool svm_classes_ok(int32_t c) { return c >= 2 && c <= VITTF_SVM_MAX_CLASSES; }
static bool svm_nsv_ok(int32_t n) { return n >= 1 && n <= VITTF_SVM_MAX_SV; }

// ------------------------------------------------------------------------------------------------ the vote
// tab[p] = (i << 4) | j of pair p, 0xff for the rows behind the last pair; threads 0..31 of the workgroup
__device__ __forceinline__ void pair_table(unsigned char* tab, int classes) {
  const int tid = threadIdx.x;
  if (tid < 32) {
    int p = tid, i = 0;
    while (i < classes - 1 && p >= classes - 1 - i) { p -= classes - 1 - i; ++i; }
    tab[tid] = i < classes - 1 ? (unsigned char)((i << 4) | (i + 1 + p)) : (unsigned char)0xff;
  }
}

// dec: the accumulator tile [pair][voxel] of the wave WITHOUT scale and intercept: dec_p = dec[r] * mul + b_p is formed here,
// written to decision (when not NULL) and voted on.  lab: VOX bytes of LDS; all threads of the workgroup call this.
template <int VOX>
__device__ __forceinline__ void vote_epilogue(f32x16_t dec, float mul, const float* __restrict__ intercept, int classes,
                                              const unsigned char* tab, unsigned char* lab, int64_t v0, int64_t nvox,
                                              unsigned char* __restrict__ labels, float* __restrict__ decision) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v = v0 + wave * 32 + l31;
  unsigned votes = 0u;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int p = acc_row(r, h);
    const unsigned code = tab[p];
    if (code != 0xffu) {
      const float d = fmaf(dec[r], mul, intercept[p]);
      if (decision && v < nvox) decision[(int64_t)p * nvox + v] = d;
      votes += 1u << (4 * (d > 0.f ? (code >> 4) : (code & 15u)));
    }
  }
  votes += __shfl_xor(votes, 32);                     // the other 16 pair rows of this voxel
  unsigned bn = votes & 15u;
  int bi = 0;
  for (int c = 1; c < classes; ++c) {
    const unsigned n = (votes >> (4 * c)) & 15u;
    if (n > bn) { bn = n; bi = c; }                   // strict: the lowest index wins a tie
  }
  if (h == 0) lab[wave * 32 + l31] = (unsigned char)bi;
  __syncthreads();
  if (tid < VOX / 4) {
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

// ------------------------------------------------------------------------------------------------ linear
template <bool ALIGNED>
__global__ __launch_bounds__(PJ_THREADS) void svm_linear_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                                const float* __restrict__ w, const float* __restrict__ intercept,
                                                                int classes, int pairs, const float* __restrict__ voxel_norm,
                                                                unsigned char* __restrict__ labels, float* __restrict__ decision) {
  __shared__ __attribute__((aligned(16))) char vbuf[PJ_ROWS * PJ_VROW];
  __shared__ __attribute__((aligned(16))) char cbuf[2 * 32 * PJ_CROW];
  __shared__ __attribute__((aligned(4))) unsigned char lab[PJ_VOX];
  __shared__ unsigned char tab[32];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t v0 = (int64_t)blockIdx.x * PJ_VOX;
  pair_table(tab, classes);                           // (visible behind the score loop's barriers)
  f32x16_t acc[1];
  project_scores<ALIGNED, 1>(feat, f, nvox, w, pairs, v0, vbuf, cbuf, acc);
  const int64_t v = v0 + wave * 32 + (lane & 31);
  const float inv = (voxel_norm && v < nvox) ? 1.f / voxel_norm[v] : 1.f;
  vote_epilogue<PJ_VOX>(acc[0], inv, intercept, classes, tab, lab, v0, nvox, labels, decision);
}

// ------------------------------------------------------------------------------------------------ RBF: scale and images
// hdr[0] = 2^e > max |coef| (1 for an all-zero model), hdr[1] = 2^-e.  One workgroup.
__global__ __launch_bounds__(1024) void svm_scale_kernel(const float* __restrict__ coef, int64_t n, float* __restrict__ hdr) {
  __shared__ float part[1024];
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(coef[i]));
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmaxf(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int e = 0;
    if (part[0] > 0.f && part[0] < __builtin_inff()) frexpf(part[0], &e);
    e = e < -100 ? -100 : e > 100 ? 100 : e;
    hdr[0] = ldexpf(1.f, e);
    hdr[1] = ldexpf(1.f, -e);
  }
}

// grid: chunks.  One image per chunk (see sv_image_bytes); rows behind n_sv and features behind f are zeros.
__global__ __launch_bounds__(BK_THREADS) void svm_prep_kernel(const unsigned short* __restrict__ sv, int f, int fp, int n_sv,
                                                              const float* __restrict__ coef, int pairs, char* __restrict__ ws) {
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x;
  char* img = ws + SV_HEADER + (int64_t)chunk * sv_image_bytes(fp);
  const float inv_scale = reinterpret_cast<const float*>(ws)[1];
  float sq = bank_write_rows<true>(tid, sv, f, fp, n_sv, chunk, img);     // |sv|^2: the strided partial sums, then a tree
  sq += __shfl_xor(sq, 1);
  sq += __shfl_xor(sq, 2);
  sq += __shfl_xor(sq, 4);
  char* cimg = img + BK_CHUNK * bank_row_bytes(fp);
  if ((tid & 7) == 0) reinterpret_cast<float*>(cimg + 2 * 32 * SV_CROW)[tid >> 3] = sq;
  // coefficients: pair row p, k-step ks, lane half h, element j <-> support vector acc_row(8 ks + j, h) of the chunk
  for (int i = tid; i < 32 * 32; i += BK_THREADS) {
    const int p = i >> 5, q = i & 31;
    const int ks = q >> 4, h = (q >> 3) & 1, j = q & 7;
    const int sidx = chunk * BK_CHUNK + acc_row(8 * ks + j, h);
    const float c = (p < pairs && sidx < n_sv) ? coef[(int64_t)p * n_sv + sidx] * inv_scale : 0.f;
    const unsigned short hi = f32_to_f16bits(c);
    const unsigned short lo = f32_to_f16bits(c - f16bits_to_f32(hi));
    *reinterpret_cast<unsigned short*>(cimg + p * SV_CROW + 2 * q) = hi;
    *reinterpret_cast<unsigned short*>(cimg + 32 * SV_CROW + p * SV_CROW + 2 * q) = lo;
  }
  for (int i = tid; i < 2 * 32; i += BK_THREADS)      // the 16 bytes behind every coefficient row
    *reinterpret_cast<uint4*>(cimg + i * SV_CROW + 2 * BK_CHUNK) = make_uint4(0u, 0u, 0u, 0u);
}

// ------------------------------------------------------------------------------------------------ RBF: the decision
template <bool ALIGNED, int FP>
__global__ __launch_bounds__(BK_THREADS) void svm_rbf_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                             const char* __restrict__ ws, int chunks,
                                                             const float* __restrict__ intercept, int classes, float neg_g2,
                                                             const float* __restrict__ voxel_norm,
                                                             unsigned char* __restrict__ labels, float* __restrict__ decision) {
  constexpr int IMG = sv_image_bytes(FP);
  __shared__ __attribute__((aligned(16))) char ring[2 * IMG];
  __shared__ __attribute__((aligned(16))) char vbuf[32 * BK_VROW];
  __shared__ __attribute__((aligned(4))) unsigned char lab[BK_VOX];
  __shared__ unsigned char tab[32];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v0 = (int64_t)blockIdx.x * BK_VOX;
  const int64_t v = v0 + wave * 32 + l31;
  pair_table(tab, classes);

  const char* images = ws + SV_HEADER;
  i32x4_t pre[ring_regs(IMG)];
  ring_prefetch<IMG>(tid, images, 0, pre);
  s16x8_t x[FP / 16];
  pickup_fragments<ALIGNED, FP>(tid, feat, f, nvox, v0, vbuf, x);
  // |x|^2 of the lane's voxel: its half of the features in register order, then the other half's sum
  float x2 = 0.f;
#pragma unroll
  for (int k = 0; k < FP / 16; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float e = f16bits_to_f32((unsigned short)x[k][j]);
      x2 = fmaf(e, e, x2);
    }
  x2 += __shfl_xor(x2, 32);
  const float inv = (voxel_norm && v < nvox) ? 1.f / voxel_norm[v] : 1.f;      // the voxel is x / norm
  x2 = x2 * inv * inv;
  const float m2inv = -2.f * inv;
  const float scale = reinterpret_cast<const float*>(ws)[0];

  f32x16_t dec;
#pragma unroll
  for (int r = 0; r < 16; ++r) dec[r] = 0.f;
  ring_commit<IMG>(tid, ring, 0, pre);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) ring_prefetch<IMG>(tid, images, c + 1, pre);
    const char* slot = ring + (c & 1) * IMG;
    const char* cimg = slot + BK_CHUNK * bank_row_bytes(FP);
    const f32x16_t acc = chunk_dots<FP>(l31, h, slot, x);
    // K of the lane's voxel against its 16 support-vector rows, as B fragments in accumulator order
    s16x8_t kh[2], kl[2];
    const float* s2 = reinterpret_cast<const float*>(cimg + 2 * 32 * SV_CROW);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4_t sq = *reinterpret_cast<const f32x4_t*>(s2 + 8 * q + 4 * h);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * q + i;
        const float d2 = fmaxf(fmaf(m2inv, acc[r], x2 + sq[i]), 0.f);
        const float kv = __builtin_amdgcn_exp2f(neg_g2 * d2);
        const unsigned short hi = f32_to_f16bits(kv);
        kh[r >> 3][r & 7] = (short)hi;
        kl[r >> 3][r & 7] = (short)f32_to_f16bits(kv - f16bits_to_f32(hi));
      }
    }
    const char* cb = cimg + l31 * SV_CROW + 16 * h;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const s16x8_t ch = *reinterpret_cast<const s16x8_t*>(cb + 32 * s);
      const s16x8_t cl = *reinterpret_cast<const s16x8_t*>(cb + 32 * SV_CROW + 32 * s);
      dec = mfma32<VITTF_FP16>(ch, kh[s], dec);
      dec = mfma32<VITTF_FP16>(ch, kl[s], dec);
      dec = mfma32<VITTF_FP16>(cl, kh[s], dec);
    }
    if (c + 1 < chunks) ring_commit<IMG>(tid, ring, c + 1, pre);      // slot (c + 1) & 1 was last read before the previous barrier
    __syncthreads();
  }
  vote_epilogue<BK_VOX>(dec, scale, intercept, classes, tab, lab, v0, nvox, labels, decision);
}

}  // namespace

size_t vittf_svm_rbf_workspace_bytes(int32_t f, int32_t n_sv, int32_t classes) {
  if (!bank_f_ok(f) || !svm_nsv_ok(n_sv) || !svm_classes_ok(classes)) return 0;
  const size_t chunks = ((size_t)n_sv + BK_CHUNK - 1) / BK_CHUNK;
  return SV_HEADER + chunks * (size_t)sv_image_bytes(bank_padded_f(f));
}

int vittf_svm_rbf_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint16_t* sv, const float* pair_coef,
                         const float* intercept, int32_t n_sv, int32_t classes, float gamma, const float* voxel_norm,
                         uint8_t* labels, float* decision, void* ws, size_t ws_bytes, void* stream) {
  if (!feat || !sv || !pair_coef || !intercept || !labels || !ws) return VITTF_ERR_INVALID_ARG;
  if (!bank_f_ok(f) || nvox < 1 || !svm_nsv_ok(n_sv) || !svm_classes_ok(classes) || !(gamma >= 0.f) || !(gamma < __builtin_inff()))
    return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)sv & 1) || ((uintptr_t)pair_coef & 3) || ((uintptr_t)intercept & 3) ||
      ((uintptr_t)voxel_norm & 3) || ((uintptr_t)decision & 3) || ((uintptr_t)ws & 15))
    return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + BK_VOX - 1) / BK_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_svm_rbf_workspace_bytes(f, n_sv, classes)) return VITTF_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int pairs = classes * (classes - 1) / 2;
  const int chunks = (n_sv + BK_CHUNK - 1) / BK_CHUNK;
  const int fp = bank_padded_f(f);
  const float neg_g2 = (float)(-(double)gamma * 1.4426950408889634074);     // exp(-gamma d2) = exp2(neg_g2 d2)
  hipLaunchKernelGGL(svm_scale_kernel, dim3(1), dim3(1024), 0, st, pair_coef, (int64_t)pairs * n_sv, (float*)ws);
  hipLaunchKernelGGL(svm_prep_kernel, dim3((unsigned)chunks), dim3(BK_THREADS), 0, st, sv, f, fp, n_sv, pair_coef, pairs, (char*)ws);
  const bool al = rows_aligned(feat, nvox);
#define SV_LAUNCH(AL, FPV) \
  hipLaunchKernelGGL((svm_rbf_kernel<AL, FPV>), dim3((unsigned)wgs), dim3(BK_THREADS), 0, st, feat, f, nvox, (const char*)ws, chunks, \
                     intercept, classes, neg_g2, voxel_norm, labels, decision)
#define SV_PICK(FPV) do { if (al) SV_LAUNCH(true, FPV); else SV_LAUNCH(false, FPV); } while (0)
  if (fp == 32) SV_PICK(32); else if (fp == 128) SV_PICK(128); else if (fp == 384) SV_PICK(384); else SV_PICK(768);
#undef SV_PICK
#undef SV_LAUNCH
  return vittf_check_launch();
}

int vittf_svm_linear_decide(const uint16_t* feat, int32_t f, int64_t nvox, const float* w, const float* intercept,
                            int32_t classes, const float* voxel_norm, uint8_t* labels, float* decision, void* stream) {
  if (!feat || !w || !intercept || !labels || !feat_f_ok(f) || nvox < 1 || !svm_classes_ok(classes)) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)w & 3) || ((uintptr_t)intercept & 3) || ((uintptr_t)voxel_norm & 3) ||
      ((uintptr_t)decision & 3))
    return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + PJ_VOX - 1) / PJ_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int pairs = classes * (classes - 1) / 2;
#define SL_LAUNCH(AL) \
  hipLaunchKernelGGL((svm_linear_kernel<AL>), dim3((unsigned)wgs), dim3(PJ_THREADS), 0, st, feat, f, nvox, w, intercept, classes, pairs, \
                     voxel_norm, labels, decision)
  if (rows_aligned(feat, nvox)) SL_LAUNCH(true); else SL_LAUNCH(false);
#undef SL_LAUNCH
  return vittf_check_launch();
}
