// Row access to an F-major fp16 feature volume [f][nvox], the transposing pickup of its voxels as MFMA B fragments and the
// score loop over it, shared by the kernels that walk one: pca.hip, kmeans.hip and the linear machine of svm.hip through
// project_scores, mlp.hip's first contraction and the bank frame of svm.hip and knn.hip (bank_frame.h) through the pickup.
// (The reduction along the voxels that the Gram and the cluster sums share is span_rows.h.)
#pragma once
#include "vittf_common.h"

namespace {

// 8 consecutive voxels v .. v + 7 of a row as one 16-byte chunk; voxels past the end are zeros
template <bool ALIGNED>
__device__ __forceinline__ uint4 feat_load8(const unsigned short* __restrict__ row, int64_t v, int64_t nvox) {
  uint4 c = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (ALIGNED) {
    if (v < nvox) c = *reinterpret_cast<const uint4*>(row + v);       // nvox % 8 == 0: the chunk is inside the row
  } else {
    unsigned e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = v + j < nvox ? (unsigned)row[v + j] : 0u;
    c = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
  return c;
}

// ---- the transposing pickup (sim_mfma.hip's): feature rows are staged in LDS, ROW bytes apart, 32 voxels of a row per wave.
// 16-lane group g covers voxels 16 (g & 1) .. + 15 of the wave's 32 and feature group g >> 1; lane 4 q + p of the group
// addresses row q, voxels 4 p .. 4 p + 3; it receives 4 features of ITS voxel.  tr_lane_offset: the lane's byte offset into
// the staged rows.  tr_fragment: the B fragment of one MFMA k-step (16 staged rows from `buf` on) of the lane's voxel, two
// ds_read_b64_tr_b16 four rows apart.  No divergence around it: the transposing read needs all 64 lanes.
template <int ROW>
__device__ __forceinline__ int tr_lane_offset(int lane, int wave) {
  const int grp = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
  return (8 * (grp >> 1) + qq) * ROW + 2 * (wave * 32 + 16 * (grp & 1) + 4 * pp);
}

template <int ROW>
__device__ __forceinline__ s16x8_t tr_fragment(const char* buf) {
  const s16x4_t x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(buf));
  const s16x4_t x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(buf + 4 * ROW));
  s16x8_t x;
  x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
  return x;
}

constexpr int FEAT_MAXF = 1024;
static bool rows_aligned(const void* feat, int64_t nvox) { return nvox % 8 == 0 && ((uintptr_t)feat & 15) == 0; }
static bool feat_f_ok(int32_t f) { return f >= 32 && f <= FEAT_MAXF && f % 32 == 0; }

// ---- scores of the rows of a small fp32 matrix against 256 voxels: the main loop of the projection and of the k-means
// assignment.  acc[b][r] = sum_f mat[32 b + acc_row(r, h)][f] x[f][v] for voxel v = v0 + 32 wave + lane % 32 (fp32, an
// accumulator tile per 32-row block; rows >= k are zeros).  The reduction runs over f, so the volume is the operand that
// needs transposed fragments: the workgroup (512 threads) stages [32 feature rows][256 voxels] parts in LDS and every wave
// picks the 8 features of its 32 voxels up with tr_fragment.  The matrix is split into fp16 hi + lo halves (mat = hi + lo to
// 2^-22, sim_mfma_prep's arithmetic) by the workgroup itself, part by part; both stagings are register-prefetched one part
// ahead.  No divergence in here.
constexpr int PJ_THREADS = 512;
constexpr int PJ_VOX = 256;                  // voxels per workgroup: 32 per wave
constexpr int PJ_ROWS = 32;                  // feature rows per staged part: two MFMA k-steps
constexpr int PJ_VROW = 2 * PJ_VOX + 64;     // LDS bytes per staged feature row: the four rows of a transposing read on four bank quarters
constexpr int PJ_CROW = 2 * PJ_ROWS + 16;    // LDS bytes per matrix row of a part (hi or lo)

// vbuf: PJ_ROWS * PJ_VROW bytes, cbuf: 2 * 32 RB * PJ_CROW bytes (hi rows, then lo rows), both 16-byte aligned LDS
template <bool ALIGNED, int RB>
__device__ __forceinline__ void project_scores(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                               const float* __restrict__ mat, int k, int64_t v0, char* vbuf, char* cbuf,
                                               f32x16_t (&acc)[RB]) {
  constexpr int KP = 32 * RB;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int parts = f / PJ_ROWS;

  // staging of a part: the volume's [32][256] as 1024 chunks of 8 voxels, two per thread; the matrix's [KP][32] as
  // KP x 8 groups of four, one per thread
  uint4 pre[2];
  float cpre[4];
  const int crow = tid >> 3, cq = tid & 7;
  auto prefetch = [&](int part) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + PJ_THREADS * j;
      pre[j] = feat_load8<ALIGNED>(feat + (int64_t)(part * PJ_ROWS + (i >> 5)) * nvox, v0 + 8 * (i & 31), nvox);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cpre[j] = (crow < k) ? mat[(int64_t)crow * f + part * PJ_ROWS + 4 * cq + j] : 0.f;
  };
  const int tr_off = tr_lane_offset<PJ_VROW>(lane, wave);
  const int a_off = l31 * PJ_CROW + 16 * h;

#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  prefetch(0);
  for (int part = 0; part < parts; ++part) {
    __syncthreads();                                   // the previous part's fragments have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + PJ_THREADS * j;
      *reinterpret_cast<uint4*>(vbuf + (i >> 5) * PJ_VROW + 16 * (i & 31)) = pre[j];
    }
    if (crow < KP) {
      unsigned short hi[4], lo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi[j] = f32_to_f16bits(cpre[j]);
        lo[j] = f32_to_f16bits(cpre[j] - f16bits_to_f32(hi[j]));
      }
      char* dst = cbuf + crow * PJ_CROW + 8 * cq;
      *reinterpret_cast<uint2*>(dst) = make_uint2((unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16));
      *reinterpret_cast<uint2*>(dst + KP * PJ_CROW) = make_uint2((unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16));
    }
    __syncthreads();
    if (part + 1 < parts) prefetch(part + 1);
#pragma unroll
    for (int s = 0; s < PJ_ROWS / 16; ++s) {
      const s16x8_t x = tr_fragment<PJ_VROW>(vbuf + tr_off + (16 * s) * PJ_VROW);
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        const char* cb = cbuf + (32 * b) * PJ_CROW + a_off + 32 * s;
        const s16x8_t ch = *reinterpret_cast<const s16x8_t*>(cb);
        const s16x8_t cl = *reinterpret_cast<const s16x8_t*>(cb + KP * PJ_CROW);
        acc[b] = mfma32<VITTF_FP16>(ch, x, acc[b]);
        acc[b] = mfma32<VITTF_FP16>(cl, x, acc[b]);
      }
    }
  }
}

}  // namespace
