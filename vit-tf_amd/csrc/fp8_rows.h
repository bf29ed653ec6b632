// The fp8 (OCP e4m3) hand-over between the qkv projection that writes q and k rows with MX block scales (gemm_pp.hip,
// vittf_gemm_qkv_fp8) and the attention kernels that read them (attention_fp8.hip): the scale rule, the byte order of a row,
// the row index, the slot order of V^T and the workspace layout -- each written once, for the producer and the consumer.
#pragma once
#include "vittf_common.h"

constexpr int FP8_KT = 64;      // keys per tile: the rows of a (slice, head) are padded to a multiple (np)

// power-of-two scale exponent for values with absolute maximum amax: amax * 2^-e <= 448 (e4m3 maximum), e >= -20.
// The E8M0 scale byte is 127 + e.
__device__ __forceinline__ int scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int ex;
  (void)frexpf(amax * (1.0f / 448.0f), &ex);        // amax / 448 = m 2^ex, m in [0.5, 1)
  return ex < -20 ? -20 : ex;
}

__device__ __forceinline__ unsigned pack4_fp8(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}

// q8 / k8 are [slice][head][np tokens][64] bytes, qs / ks [slice][head][np tokens][2] E8M0 bytes (one per 32-wide block
// of the row): the row of token tok of (slice b, head hd), bh = b * heads + hd
__device__ __forceinline__ int64_t fp8_row_index(int64_t bh, int np, int tok) { return bh * np + tok; }
// Position of dim (a multiple of 16) inside a stored 64-byte row, when the row carries block scales.  The matrix
// instruction's MX block b of a row is bytes 16 b .. 16 b + 15 of BOTH lane halves (k = 32 (byte >> 4) + 16 (lane >> 5) +
// (byte & 15): tools/micro/mfma_f8_scale_probe2), and the attention kernel's lane half hh reads bytes 32 hh .. 32 hh + 31
// with the scale byte hh of the row: a row is stored as [d 0-15 | d 32-47 | d 16-31 | d 48-63], scale byte dim >> 5.
__device__ __forceinline__ int fp8_row_pos(int dim) { return ((dim >> 4) & 1) * 32 + (dim >> 5) * 16; }

// V8T is [slice][head][64 dims][np keys] with the keys of a tile in the order the P operand has them.  Slot of key `kin`
// (0..63) inside its tile: inverse of key = 32 b + (r & 3) + 8 (r >> 2) + 4 h, slot = 32 h + 16 b + r
__device__ __forceinline__ int vt_slot(int kin) {
  const int b = kin >> 5, w = kin & 31;
  const int h = (w >> 2) & 1, r = (w & 3) + 4 * (w >> 3);
  return 32 * h + 16 * b + r;
}

// The workspace of vittf_attention_fp8 / vittf_gemm_qkv_fp8 + vittf_attention_fp8_rows (256-byte aligned pieces):
// absolute maxima as float bits [slice][head][q | k | v], then q8, k8, v8t, qs, ks
struct Fp8Ws {
  unsigned* amax;
  unsigned char *q8, *k8, *v8t, *qs, *ks;
  size_t total;
  int np;
};
static inline Fp8Ws fp8_ws(void* ws, int batch, int tokens, int heads) {
  Fp8Ws w;
  w.np = (tokens + FP8_KT - 1) / FP8_KT * FP8_KT;
  const size_t per = (size_t)batch * heads * w.np * 64;
  const size_t sc = ((size_t)batch * heads * w.np * 2 + 255) & ~(size_t)255;     // row scales (vittf_gemm_qkv_fp8)
  const size_t q8 = ((size_t)batch * heads * 3 * 4 + 255) & ~(size_t)255;
  unsigned char* base = (unsigned char*)ws;
  w.amax = (unsigned*)ws;
  w.q8 = base + q8;
  w.k8 = w.q8 + per;
  w.v8t = w.k8 + per;
  w.qs = w.v8t + per;
  w.ks = w.qs + sc;
  w.total = q8 + 3 * per + 2 * sc;
  return w;
}
