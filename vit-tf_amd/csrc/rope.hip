// Rotary position embedding of DINOv3: the q and k thirds of the engine's QKV buffer rotated in place.
//
// DINOv3 has no additive position embedding; in every block the q and k vectors of the PATCH tokens are rotated, per head of
// 64, by angles that depend on the patch's (row, column) only (the same table for every head and every block); CLS and the
// register tokens are left as they are.  With rot(v) = cat(-v[32:64], v[0:32]):  q' = q cos + rot(q) sin, i.e. column j < 32
// of a head pairs with column j + 32:
//     lo' = lo cos_j - hi sin_j        hi' = hi cos_j + lo sin_j
// The table ([patches][32] cos and sin, fp32) is built on the host (weights.py rope_table) and stays L2-resident (1 MB for
// 64 x 64 patches).  HBM-bound: a lane owns 8 columns of the low half of a head and the same 8 of the high half -- two 16-byte
// loads, fp32 arithmetic, one rounding to the 16-bit type, two 16-byte stores -- so every byte of the q and k thirds is read
// once and written once and the v third is never touched.  The q and k thirds are contiguous, so head slot s (0 .. 2 heads - 1;
// q heads, then k heads) starts at column 64 s of the row.  A rotation commutes with the log2(e) / 8 the qkv epilogue
// (VITTF_EPI_BIAS_QKV) has already multiplied q by.
#include "vittf_common.h"

namespace {

template <int DT>
__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = h16_to_f32<DT>((unsigned short)(w[i] & 0xffffu));
    f[2 * i + 1] = h16_to_f32<DT>((unsigned short)(w[i] >> 16));
  }
}

// lanes_per_row = 8 heads: (head slot, 8-column chunk c of 4); consecutive lanes cover consecutive chunks, so the four lanes
// of a head slot read its low 64 bytes with the first load and its high 64 bytes with the second
template <int DT>
__global__ __launch_bounds__(256) void rope_qk_kernel(unsigned short* __restrict__ qkv, const float* __restrict__ cos_t,
                                                      const float* __restrict__ sin_t, int64_t rows, int tokens, int prefix,
                                                      int lanes_per_row, int row_stride) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / lanes_per_row;
  if (row >= rows) return;
  const int rem = (int)(gid - row * lanes_per_row);
  const int tok = (int)(row % tokens);
  if (tok < prefix) return;                       // CLS and the register tokens are not rotated
  const int c = rem & 3;
  unsigned short* lo_p = qkv + row * row_stride + (rem >> 2) * 64 + c * 8;
  const float4* cp = reinterpret_cast<const float4*>(cos_t + (int64_t)(tok - prefix) * 32 + c * 8);
  const float4* sp = reinterpret_cast<const float4*>(sin_t + (int64_t)(tok - prefix) * 32 + c * 8);
  const uint4 lo_v = *reinterpret_cast<const uint4*>(lo_p);
  const uint4 hi_v = *reinterpret_cast<const uint4*>(lo_p + 32);
  const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
  const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float lo[8], hi[8], nlo[8], nhi[8];
  unpack8<DT>(lo_v, lo);
  unpack8<DT>(hi_v, hi);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    nlo[i] = lo[i] * cs[i] - hi[i] * sn[i];
    nhi[i] = hi[i] * cs[i] + lo[i] * sn[i];
  }
  uint4 lo_o, hi_o;
  lo_o.x = pack2_h16<DT>(nlo[0], nlo[1]); lo_o.y = pack2_h16<DT>(nlo[2], nlo[3]);
  lo_o.z = pack2_h16<DT>(nlo[4], nlo[5]); lo_o.w = pack2_h16<DT>(nlo[6], nlo[7]);
  hi_o.x = pack2_h16<DT>(nhi[0], nhi[1]); hi_o.y = pack2_h16<DT>(nhi[2], nhi[3]);
  hi_o.z = pack2_h16<DT>(nhi[4], nhi[5]); hi_o.w = pack2_h16<DT>(nhi[6], nhi[7]);
  *reinterpret_cast<uint4*>(lo_p) = lo_o;
  *reinterpret_cast<uint4*>(lo_p + 32) = hi_o;
}

}  // namespace

extern "C" int vittf_rope_qk(void* qkv, int64_t rows, int32_t tokens, int32_t prefix, int32_t heads,
                             const vittf_rope_table* table, int32_t dtype, void* stream) {
  if (!qkv || !table || !table->cos || !table->sin || rows <= 0 || heads <= 0 || heads > 64 || prefix < 0 || tokens <= prefix)
    return VITTF_ERR_INVALID_ARG;
  if (table->patches != tokens - prefix) return VITTF_ERR_INVALID_ARG;      // one table row per patch token of a slice
  if ((((uintptr_t)qkv | (uintptr_t)table->cos | (uintptr_t)table->sin) & 15) != 0) return VITTF_ERR_INVALID_ARG;
  const int lanes_per_row = 8 * heads;                                      // 2 heads slots (q, k) x 4 chunks
  const int64_t blocks = (rows * lanes_per_row + 255) / 256;
  if (blocks > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int row_stride = 3 * 64 * heads;
  if (dtype == VITTF_BF16)
    hipLaunchKernelGGL((rope_qk_kernel<VITTF_BF16>), dim3((unsigned)blocks), dim3(256), 0, st, (unsigned short*)qkv, table->cos,
                       table->sin, rows, tokens, prefix, lanes_per_row, row_stride);
  else if (dtype == VITTF_FP16)
    hipLaunchKernelGGL((rope_qk_kernel<VITTF_FP16>), dim3((unsigned)blocks), dim3(256), 0, st, (unsigned short*)qkv, table->cos,
                       table->sin, rows, tokens, prefix, lanes_per_row, row_stride);
  else
    return VITTF_ERR_INVALID_ARG;
  return vittf_check_launch();
}
