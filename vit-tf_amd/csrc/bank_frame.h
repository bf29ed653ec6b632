// The frame of the kernels that stream a bank of fp16 rows past the voxels of an F-major fp16 feature volume [f][nvox]:
// svm.hip (the bank is the support vectors) and knn.hip (the annotated samples).  A workgroup of 4 waves owns 128 voxels;
// every wave picks all features of its 32 voxels up once (pickup_fragments) and keeps them as the B operands of
// v_mfma_f32_32x32x16_f16, f padded with zero features to FP = 32, 128, 384 or 768.  The bank streams past in chunks of 32
// rows: a prep kernel writes one LDS image per chunk into the workspace -- [32 rows of 2 FP + 16 bytes] (bank_write_rows)
// and behind them whatever the kernel needs per chunk -- and the workgroups copy the images through a ring of two LDS slots,
// chunk c in slot c & 1, register-prefetched one chunk ahead (ring_prefetch, ring_commit).  chunk_dots is the contraction of
// a chunk: a lane ends with the 16 dot products of its OWN voxel with the rows acc_row(r, h) of the chunk.
#pragma once
#include "vittf_common.h"
#include "feat_rows.h"

namespace {

constexpr int BK_THREADS = 256, BK_WAVES = 4;
constexpr int BK_VOX = 32 * BK_WAVES;          // voxels per workgroup
constexpr int BK_CHUNK = 32;                   // bank rows per chunk
constexpr int BK_VROW = 2 * BK_VOX + 64;       // LDS bytes per staged feature row of the pickup

__host__ __device__ constexpr int bank_row_bytes(int fp) { return 2 * fp + 16; }
static int bank_padded_f(int32_t f) { return f <= 32 ? 32 : f <= 128 ? 128 : f <= 384 ? 384 : 768; }
static bool bank_f_ok(int32_t f) { return f >= 32 && f <= 768 && f % 32 == 0; }

// prep kernels (BK_THREADS threads, one chunk): the chunk's 32 rows of the image `img`, 8 threads per row, 8 features a step;
// rows behind n_rows and features behind f are zeros.  With SQ the return value is the thread's part of |row|^2 in a fixed
// order (strided over the row's 8 threads: tid >> 3 is the row, a tree over tid & 7 finishes it); without, nothing is summed.
template <bool SQ>
__device__ __forceinline__ float bank_write_rows(int tid, const unsigned short* bank, int f, int fp, int n_rows, int chunk,
                                                 char* img) {
  const int rowb = bank_row_bytes(fp);
  const int row = tid >> 3, sub = tid & 7;
  const int s = chunk * BK_CHUNK + row;
  float sq = 0.f;
  for (int k8 = sub; k8 < rowb / 16; k8 += 8) {
    unsigned e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = 8 * k8 + j;
      e[j] = (s < n_rows && i < f) ? (unsigned)bank[(int64_t)s * f + i] : 0u;
      if constexpr (SQ) {
        const float x = f16bits_to_f32((unsigned short)e[j]);
        sq = fmaf(x, x, sq);
      }
    }
    *reinterpret_cast<uint4*>(img + row * rowb + 16 * k8) =
        make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
  return sq;
}

// the wave's 32 voxels v0 + 32 wave .. + 31: all FP features as B fragments, 32 feature rows of 128 voxels staged at a time
// in vbuf (32 * BK_VROW bytes of 16-byte aligned LDS); rows from f on are zeros.  All threads of the workgroup call this.
template <bool ALIGNED, int FP>
__device__ __forceinline__ void pickup_fragments(int tid, const unsigned short* feat, int f, int64_t nvox, int64_t v0,
                                                 char* vbuf, s16x8_t (&x)[FP / 16]) {
  const int tr_off = tr_lane_offset<BK_VROW>(tid & 63, __builtin_amdgcn_readfirstlane(tid >> 6));
#pragma unroll
  for (int part = 0; part < FP / 32; ++part) {
    if (part) __syncthreads();                      // the previous part's fragments have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int i = tid + BK_THREADS * j;
      const int row = part * 32 + (i >> 4);
      uint4 c = make_uint4(0u, 0u, 0u, 0u);
      if (row < f) c = feat_load8<ALIGNED>(feat + (int64_t)row * nvox, v0 + 8 * (i & 15), nvox);
      *reinterpret_cast<uint4*>(vbuf + (i >> 4) * BK_VROW + 16 * (i & 15)) = c;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) x[2 * part + s] = tr_fragment<BK_VROW>(vbuf + tr_off + (16 * s) * BK_VROW);
  }
}

// the ring of two slots of IMG bytes (a multiple of 16): the 16-byte pieces of an image, ring_regs(IMG) per thread.  The
// registers are native vectors: hipcc keeps an array of HIP uint4 structs in scratch here.  tid is threadIdx.x of a
// workgroup of BK_THREADS: saying so lets hipcc keep the piece index tid | 256 j, its offset an immediate of the load, as it
// does where the loop stands in the kernel itself (without it: one 64-bit add per piece and chunk).
__host__ __device__ constexpr int ring_regs(int img) { return (img / 16 + BK_THREADS - 1) / BK_THREADS; }

template <int IMG>
__device__ __forceinline__ void ring_prefetch(int tid, const char* images, int c, i32x4_t (&pre)[ring_regs(IMG)]) {
  static_assert(IMG % 16 == 0, "images are copied in 16-byte pieces");
  constexpr int PIECES = IMG / 16;
  __builtin_assume((unsigned)tid < (unsigned)BK_THREADS);
#pragma unroll
  for (int j = 0; j < ring_regs(IMG); ++j) {
    const int i = tid + BK_THREADS * j;             // the last round is part-filled: its spare lanes load a piece twice
    pre[j] = reinterpret_cast<const i32x4_t*>(images + (int64_t)c * IMG)[i < PIECES ? i : PIECES - 1];
  }
}

template <int IMG>
__device__ __forceinline__ void ring_commit(int tid, char* ring, int c, const i32x4_t (&pre)[ring_regs(IMG)]) {
  constexpr int PIECES = IMG / 16;
  __builtin_assume((unsigned)tid < (unsigned)BK_THREADS);
#pragma unroll
  for (int j = 0; j < ring_regs(IMG); ++j) {
    const int i = tid + BK_THREADS * j;
    if (i < PIECES) reinterpret_cast<i32x4_t*>(ring + (c & 1) * IMG)[i] = pre[j];
  }
}

// acc[r] = row acc_row(r, h) of the chunk in `slot` . the voxel of lane l31 + 32 h: FP / 16 MFMAs, fp32 accumulation of exact
// products
template <int FP>
__device__ __forceinline__ f32x16_t chunk_dots(int l31, int h, const char* slot, const s16x8_t (&x)[FP / 16]) {
  const char* ab = slot + l31 * bank_row_bytes(FP) + 16 * h;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int k = 0; k < FP / 16; ++k) acc = mfma32<VITTF_FP16>(*reinterpret_cast<const s16x8_t*>(ab + 32 * k), x[k], acc);
  return acc;
}

}  // namespace
