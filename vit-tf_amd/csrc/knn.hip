// Weighted k-nearest-neighbour classification of every voxel of an F-major fp16 feature volume [f][nvox] against a bank of
// labelled fp16 samples (vit-tf_amd/knn.py; classify_features.py --classifier knn): the k-NN of the DINO evaluation protocol.
//
// sim[s][v] = bank_s . x_v (fp16 MFMA, fp32 accumulation), times 1 / voxel_norm[v] when a norm array is given.  The
// neighbours of a voxel are the k samples that come first under "larger sim first, then lower sample index" (an IEEE
// comparison of exactly these fp32 values), rank 1 the nearest; w_j = 1 (uniform) or exp2((sim_j - sim_1) c), c = log2(e) / T;
// scores[c] = sum of w_j over the ranks j = 1..k of class c, added in fp32 in rank order; label = arg-max, lowest class first.
//
// The frame is bank_frame.h's, shared with svm_rbf_kernel: the voxels stay where they are as MFMA B operands, the bank streams
// past in chunks of 32 rows through the ring of LDS images.  An image holds [32 rows][FP] fp16 and one 32-bit word per row,
// (index << 3) | class, 0xffffffff for a row behind the bank.  After chunk_dots a lane holds 16 similarities of its OWN voxel
// (rows acc_row(r, h)); lanes l and l + 32 hold the two halves of the chunk.
//
// Selection.  Every lane keeps a sorted list of LEN >= k entries (sim, word) of the rows IT has seen, in registers under
// compile-time indices (LEN = 1, 4, 8, 16, 20, 24 or 32 is a template parameter: k = 1 or 5 does not pay for 32).  A lane meets
// its rows in ascending index order, so inserting a candidate strictly behind every entry that is not smaller keeps equal
// similarities in index order.  Per chunk the 16 values are first filtered into a bit mask against a threshold t that LEN
// EARLIER rows of the voxel are known to reach -- the lane's own LEN-th value, the other half's, or the smaller of the two
// LEN / 2-th values (two __shfl_xor(.., 32) a chunk): a row that is not above t has LEN earlier rows before it in the order
// and cannot be a neighbour, a row above t is inserted.  The 16 values and their words go to a per-lane column of LDS (a
// register array under a runtime index would be scratch), for FP = 384 those of two chunks before anything is inserted; the
// wave then runs as many insertion rounds as its busiest lane has candidates (a few instead of 16 a chunk), each lane
// fetching the row of its lowest set bit; a lane with nothing left inserts -inf, which changes nothing.  One insertion is a
// fully unrolled chain: a compare, a v_med3_f32 and two selects per slot.  LEN = 1 is a running maximum without rounds.
// At the end the two lanes of a voxel exchange their lists with __shfl_xor(.., 32) and merge them with a bitonic network over
// CAP slots, LEN rounded up to a power of two (half-cleaner of own[i] against other[CAP - 1 - i], then log2(CAP) stages)
// under the total order (sim, index): both lanes compute the same entries, of which the first k are the neighbours.
// Fixed order, no atomics: the same call gives the same bytes, whatever optional outputs are asked for.
#include "vittf_common.h"
#include "bank_frame.h"

namespace {

constexpr unsigned KN_NONE = 0xffffffffu;      // the word of a row behind the bank / an empty list slot

// image of a chunk: [32 bank rows of 2 FP + 16 bytes][32 words (index << 3) | class]
__host__ __device__ constexpr int kn_image_bytes(int fp) { return BK_CHUNK * bank_row_bytes(fp) + 4 * BK_CHUNK; }

static bool knn_bank_ok(int32_t n) { return n >= 1 && n <= VITTF_KNN_MAX_BANK; }

// grid: chunks.  One image per chunk; rows behind n_bank and features behind f are zeros.
__global__ __launch_bounds__(BK_THREADS) void knn_prep_kernel(const unsigned short* __restrict__ bank,
                                                              const unsigned char* __restrict__ bank_class, int f, int fp,
                                                              int n_bank, char* __restrict__ ws) {
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x;
  char* img = ws + (int64_t)chunk * kn_image_bytes(fp);
  bank_write_rows<false>(tid, bank, f, fp, n_bank, chunk, img);
  if (tid < BK_CHUNK) {
    const int sm = chunk * BK_CHUNK + tid;
    reinterpret_cast<unsigned*>(img + BK_CHUNK * bank_row_bytes(fp))[tid] =
        sm < n_bank ? ((unsigned)sm << 3) | (unsigned)(bank_class[sm] & 7) : KN_NONE;
  }
}

// (sa, ma) comes before (sb, mb): larger similarity first, then the lower index (the index is the high part of the word)
__device__ __forceinline__ bool kn_before(float sa, unsigned ma, float sb, unsigned mb) {
  return sa > sb || (sa == sb && ma < mb);
}

// LEN sorted entries in the first slots of CAP (a power of two, for the merge network; the slots behind LEN stay empty)
template <int CAP, int LEN>
struct KnnList {
  float s[CAP];
  unsigned m[CAP];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < CAP; ++j) { s[j] = -__builtin_inff(); m[j] = KN_NONE; }
  }
  // the candidate goes behind every entry that is not smaller; cs = -inf changes nothing
  __device__ __forceinline__ void insert(float cs, unsigned cm) {
    bool g[LEN];
#pragma unroll
    for (int j = 0; j < LEN; ++j) g[j] = cs > s[j];
#pragma unroll
    for (int j = LEN - 1; j > 0; --j) {
      m[j] = g[j - 1] ? m[j - 1] : (g[j] ? cm : m[j]);
      s[j] = __builtin_amdgcn_fmed3f(s[j - 1], cs, s[j]);       // s[j - 1] >= s[j]: the median is the new s[j]
    }
    m[0] = g[0] ? cm : m[0];
    s[0] = g[0] ? cs : s[0];
  }
  __device__ __forceinline__ void exchange(int i, int j) {       // the entry that comes first goes to i
    const bool sw = kn_before(s[j], m[j], s[i], m[i]);
    const float ts = s[i];
    const unsigned tm = m[i];
    s[i] = sw ? s[j] : ts;  m[i] = sw ? m[j] : tm;
    s[j] = sw ? ts : s[j];  m[j] = sw ? tm : m[j];
  }
  // the CAP first entries of this list and the one of lane ^ 32 together, sorted; both lanes end with the same list
  __device__ __forceinline__ void merge_halves() {
    float os[CAP];
    unsigned om[CAP];
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      os[j] = __shfl_xor(s[j], 32);
      om[j] = (unsigned)__shfl_xor((int)m[j], 32);
    }
#pragma unroll
    for (int j = 0; j < CAP; ++j) {                              // half-cleaner: own (descending) against the other, reversed
      const bool o = kn_before(os[CAP - 1 - j], om[CAP - 1 - j], s[j], m[j]);
      s[j] = o ? os[CAP - 1 - j] : s[j];
      m[j] = o ? om[CAP - 1 - j] : m[j];
    }
#pragma unroll
    for (int stride = CAP / 2; stride > 0; stride >>= 1)         // the CAP entries are bitonic: log2(CAP) stages sort them
#pragma unroll
      for (int j = 0; j < CAP; ++j)
        if ((j & stride) == 0) exchange(j, j + stride);
  }
};

// FP = 32 does not take pickup_fragments, tr_fragment and chunk_dots from the shared headers: there the kernel is all
// selection (two MFMAs a chunk), and its time follows the order hipcc gives the unrolled insertion chains -- with the
// helpers, and even with tr_fragment alone, the same instructions came out in another order and k = 4 .. 24 measured 1 to
// 3 % slower at 64^3 x 32 (k = 20: 0.2972 against 0.2936 ms).  With these lines written out the FP = 32 kernels are within
// 0.3 % of the code before the frame was shared; the ring helpers cost nothing there and stay.
template <bool ALIGNED, int FP, int LEN>
__global__ __launch_bounds__(BK_THREADS) void knn_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                         const char* __restrict__ images, int chunks, int n_bank, int classes,
                                                         int k, float exp_scale, const float* __restrict__ voxel_norm,
                                                         unsigned char* __restrict__ labels, float* __restrict__ scores,
                                                         int* __restrict__ nn_index, float* __restrict__ nn_sim) {
  constexpr int CAP = LEN <= 1 ? 1 : LEN <= 4 ? 4 : LEN <= 8 ? 8 : LEN <= 16 ? 16 : 32;
  constexpr int IMG = kn_image_bytes(FP);
  __shared__ __attribute__((aligned(16))) char ring[2 * IMG];
  __shared__ __attribute__((aligned(16))) char vbuf[32 * BK_VROW];
  __shared__ __attribute__((aligned(4))) unsigned char lab[BK_VOX];
  // the candidates of BATCH chunks, [row][thread]: a lane reads back only what it wrote itself (any row: no bank conflict)
  constexpr int BATCH = (LEN > 1 && FP == 384) ? 2 : 1;      // (registers leave one workgroup a CU there anyway; 768 lacks the LDS)
  __shared__ float cand_s[LEN > 1 ? 16 * BATCH * BK_THREADS : 1];
  __shared__ unsigned cand_m[LEN > 1 ? 16 * BATCH * BK_THREADS : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v0 = (int64_t)blockIdx.x * BK_VOX;
  const int64_t v = v0 + wave * 32 + l31;

  i32x4_t pre[ring_regs(IMG)];
  ring_prefetch<IMG>(tid, images, 0, pre);
  s16x8_t x[FP / 16];
  if constexpr (FP == 32) {
    // FP = 32 keeps the one-part pickup and the two MFMAs of a chunk written out (see the note above the kernel)
    const int grp = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    const int tr_off = (8 * (grp >> 1) + qq) * BK_VROW + 2 * (wave * 32 + 16 * (grp & 1) + 4 * pp);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + BK_THREADS * j;
      const int row = i >> 4;
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      if (row < f) c = feat_load8<ALIGNED>(feat + (int64_t)row * nvox, v0 + 8 * (i & 15), nvox);
      *reinterpret_cast<uint4*>(vbuf + (i >> 4) * BK_VROW + 16 * (i & 15)) = c;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const char* buf = vbuf + tr_off + (16 * s) * BK_VROW;
      const s16x4_t x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(buf));
      const s16x4_t x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(buf + 4 * BK_VROW));
      s16x8_t t;
      t[0] = x0[0]; t[1] = x0[1]; t[2] = x0[2]; t[3] = x0[3]; t[4] = x1[0]; t[5] = x1[1]; t[6] = x1[2]; t[7] = x1[3];
      x[s] = t;
    }
  } else {
    pickup_fragments<ALIGNED, FP>(tid, feat, f, nvox, v0, vbuf, x);
  }
  const float inv = (voxel_norm && v < nvox) ? 1.f / voxel_norm[v] : 1.f;      // the voxel is x / norm

  KnnList<CAP, LEN> best;
  best.clear();
  [[maybe_unused]] unsigned pending = 0u;                                 // bit 16 b + r: row r of the b-th chunk of the batch is a candidate
  ring_commit<IMG>(tid, ring, 0, pre);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) ring_prefetch<IMG>(tid, images, c + 1, pre);
    const char* slot = ring + (c & 1) * IMG;
    const unsigned* word = reinterpret_cast<const unsigned*>(slot + BK_CHUNK * bank_row_bytes(FP));
    f32x16_t acc;
    if constexpr (FP == 32) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const char* ab = slot + l31 * bank_row_bytes(FP) + 16 * h;
#pragma unroll
      for (int kk = 0; kk < FP / 16; ++kk) acc = mfma32<VITTF_FP16>(*reinterpret_cast<const s16x8_t*>(ab + 32 * kk), x[kk], acc);
    } else {
      acc = chunk_dots<FP>(l31, h, slot, x);
    }
    float sim[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sim[r] = acc[r] * inv;
    if (c == chunks - 1) {                                // rows behind the bank are never neighbours
      const int left = n_bank - BK_CHUNK * c;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc_row(r, h) >= left) sim[r] = -__builtin_inff();
    }
    if constexpr (CAP == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i32x4_t w4 = *reinterpret_cast<const i32x4_t*>(word + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool gt = sim[4 * q + i] > best.s[0];     // strict: the earlier row keeps an equal similarity
          best.s[0] = gt ? sim[4 * q + i] : best.s[0];
          best.m[0] = gt ? (unsigned)w4[i] : best.m[0];
        }
      }
    } else {
      // a candidate can only be a neighbour if fewer than LEN >= k earlier rows are at least as large: the lane's own
      // LEN-th value, the other half's, or the smaller of the two LEN / 2-th values (LEN / 2 rows of each half) say so
      const float other_last = __shfl_xor(best.s[LEN - 1], 32), other_mid = __shfl_xor(best.s[LEN / 2 - 1], 32);
      const float kth = fmaxf(fmaxf(best.s[LEN - 1], other_last), fminf(best.s[LEN / 2 - 1], other_mid));
      // all 16 rows go to LDS with their words (a runtime-indexed register would be scratch); the bits say which to fetch
      const int base = BATCH == 2 ? 16 * (c & 1) : 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const i32x4_t w4 = *reinterpret_cast<const i32x4_t*>(word + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * q + i;
          cand_s[(base + r) * BK_THREADS + tid] = sim[r];
          cand_m[(base + r) * BK_THREADS + tid] = (unsigned)w4[i];
          pending |= sim[r] > kth ? 1u << (base + r) : 0u;
        }
      }
      // the wave runs as many rounds as its busiest lane has candidates; over a batch of two chunks that maximum is
      // nearer the mean.  The threshold of a chunk stays valid while earlier candidates wait: it only grows.
      if (BATCH == 1 || (c & 1) || c == chunks - 1) {
        while (__any(pending != 0u)) {
          const int pick = pending ? __builtin_ctz(pending) : 0;             // ascending index order
          const float cs = pending ? cand_s[pick * BK_THREADS + tid] : -__builtin_inff();
          const unsigned cm = cand_m[pick * BK_THREADS + tid];
          pending &= pending - 1u;
          best.insert(cs, cm);
        }
      }
    }
    if (c + 1 < chunks) ring_commit<IMG>(tid, ring, c + 1, pre);      // slot (c + 1) & 1 was last read before the previous barrier
    __syncthreads();
  }

  // both lanes of a voxel: the merged list, the weights and the per-class sums in rank order
  if constexpr (CAP == 1) {
    const float os = __shfl_xor(best.s[0], 32);
    const unsigned om = (unsigned)__shfl_xor((int)best.m[0], 32);
    const bool o = kn_before(os, om, best.s[0], best.m[0]);
    best.s[0] = o ? os : best.s[0];
    best.m[0] = o ? om : best.m[0];
  } else {
    best.merge_halves();
  }
  float sc[VITTF_KNN_MAX_CLASSES];
#pragma unroll
  for (int q = 0; q < VITTF_KNN_MAX_CLASSES; ++q) sc[q] = 0.f;
  const float top = best.s[0];
#pragma unroll
  for (int j = 0; j < LEN; ++j) {
    if (j < k) {
      const float w = exp_scale == 0.f ? 1.f : __builtin_amdgcn_exp2f((best.s[j] - top) * exp_scale);
      const unsigned cls = best.m[j] & 7u;
#pragma unroll
      for (int q = 0; q < VITTF_KNN_MAX_CLASSES; ++q) sc[q] += cls == (unsigned)q ? w : 0.f;
      if (v < nvox) {
        if (nn_index && h == 0) nn_index[(int64_t)j * nvox + v] = (int)(best.m[j] >> 3);
        if (nn_sim && h == 1) nn_sim[(int64_t)j * nvox + v] = best.s[j];
      }
    }
  }
  float bs = sc[0];
  int bi = 0;
#pragma unroll
  for (int q = 1; q < VITTF_KNN_MAX_CLASSES; ++q)
    if (q < classes && sc[q] > bs) { bs = sc[q]; bi = q; }     // strict: the lowest class wins a tie
  if (scores && h == 0 && v < nvox) {
#pragma unroll
    for (int q = 0; q < VITTF_KNN_MAX_CLASSES; ++q)
      if (q < classes) scores[(int64_t)q * nvox + v] = sc[q];
  }
  if (h == 0) lab[wave * 32 + l31] = (unsigned char)bi;
  __syncthreads();
  if (tid < BK_VOX / 4) {
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

}  // namespace

size_t vittf_knn_workspace_bytes(int32_t f, int32_t n_bank) {
  if (!bank_f_ok(f) || !knn_bank_ok(n_bank)) return 0;
  const size_t chunks = ((size_t)n_bank + BK_CHUNK - 1) / BK_CHUNK;
  return chunks * (size_t)kn_image_bytes(bank_padded_f(f));
}

int vittf_knn_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint16_t* bank, const uint8_t* bank_class,
                     int32_t n_bank, int32_t classes, int32_t k, float inv_temperature, const float* voxel_norm,
                     uint8_t* labels, float* scores, int32_t* nn_index, float* nn_sim, void* ws, size_t ws_bytes,
                     void* stream) {
  if (!feat || !bank || !bank_class || !labels || !ws) return VITTF_ERR_INVALID_ARG;
  if (!bank_f_ok(f) || nvox < 1 || !knn_bank_ok(n_bank) || classes < 2 || classes > VITTF_KNN_MAX_CLASSES || k < 1 ||
      k > VITTF_KNN_MAX_K || k > n_bank || !(inv_temperature >= 0.f) || !(inv_temperature < __builtin_inff()))
    return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)bank & 1) || ((uintptr_t)voxel_norm & 3) || ((uintptr_t)scores & 3) ||
      ((uintptr_t)nn_index & 3) || ((uintptr_t)nn_sim & 3) || ((uintptr_t)ws & 15))
    return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + BK_VOX - 1) / BK_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_knn_workspace_bytes(f, n_bank)) return VITTF_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (n_bank + BK_CHUNK - 1) / BK_CHUNK;
  const int fp = bank_padded_f(f);
  const float exp_scale = (float)((double)inv_temperature * 1.4426950408889634074);     // exp(d / T) = exp2(d exp_scale)
  if (inv_temperature > 0.f && !(exp_scale > 0.f && exp_scale < __builtin_inff())) return VITTF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(knn_prep_kernel, dim3((unsigned)chunks), dim3(BK_THREADS), 0, st, bank, bank_class, f, fp, n_bank, (char*)ws);
  const bool al = rows_aligned(feat, nvox);
#define KN_LAUNCH(AL, FPV, CAPV) \
  hipLaunchKernelGGL((knn_kernel<AL, FPV, CAPV>), dim3((unsigned)wgs), dim3(BK_THREADS), 0, st, feat, f, nvox, (const char*)ws, chunks, \
                     n_bank, classes, k, exp_scale, voxel_norm, labels, scores, nn_index, nn_sim)
#define KN_CAP(AL, FPV) do { if (k == 1) KN_LAUNCH(AL, FPV, 1); else if (k <= 4) KN_LAUNCH(AL, FPV, 4); else if (k <= 8) KN_LAUNCH(AL, FPV, 8); \
                             else if (k <= 16) KN_LAUNCH(AL, FPV, 16); else if (k <= 20) KN_LAUNCH(AL, FPV, 20); \
                             else if (k <= 24) KN_LAUNCH(AL, FPV, 24); else KN_LAUNCH(AL, FPV, 32); } while (0)
#define KN_PICK(FPV) do { if (al) KN_CAP(true, FPV); else KN_CAP(false, FPV); } while (0)
  if (fp == 32) KN_PICK(32); else if (fp == 128) KN_PICK(128); else if (fp == 384) KN_PICK(384); else KN_PICK(768);
#undef KN_PICK
#undef KN_CAP
#undef KN_LAUNCH
  return vittf_check_launch();
}
