// The frame the 16-bit attention kernels share (attention.hip, attention_pp64.hip): work-item decode, Q fragments, K / V
// tile staging, LDS images and their fragment reads, row maximum, ragged-tile mask, row-sum inverse, output rows.  What a
// kernel keeps to itself is its schedule: ring depth, phase order, waits.  attention_fp8.hip has images and staging of its
// own (byte operands) and takes the decode, the mask, the row-sum inverse and the output rows from here.
#pragma once
#include "vittf_common.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

constexpr int ATT_KT = 64;                       // keys per LDS tile
constexpr int ATT_KV_TILE_BYTES = ATT_KT * 64 * 2;   // 8 KB
constexpr int ATT_BUF_BYTES = 2 * ATT_KV_TILE_BYTES; // K | V

// V image: [8 key groups][2 column halves] subtiles of 8 keys x 32 columns (512 B), chunk XOR by (key>>2)&3;
// read with ds_read_b64_tr_b16, conflict free
__device__ __forceinline__ int v_off(int key, int ch) {
  return 1024 * (key >> 3) + 512 * (ch >> 2) + 64 * (key & 7) + 16 * ((ch & 3) ^ ((key >> 2) & 3));
}
// inverse of v_off for the LDS-DMA source side: linear 16-byte position q -> (key, chunk)
__device__ __forceinline__ void v_pos(int q, int& key, int& ch) {
  const int kg = q >> 6, half = (q >> 5) & 1, k7 = (q >> 2) & 7, x = q & 3;
  key = 8 * kg + k7;
  ch = 4 * half + (x ^ ((key >> 2) & 3));
}

// max of three scores.  Plain fmaxf: attention.hip is built with -fno-honor-nans (Makefile), which drops the
// canonicalising v_max hipcc otherwise inserts per operand and lets it form v_max3_f32 itself.  (An inline-asm
// v_max3 is NOT an option: asm consumers of an MFMA result get none of the MFMA -> VALU wait states the compiler
// inserts for its own instructions, and read the accumulator before the matrix pipe has written it.)
__device__ __forceinline__ float max3_f32(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// Output rows of the transposed product O^T = V^T P^T: a lane holds, of ITS query row, the columns
// 32 dvt + 8 g + 4 h + {0..3} (h = lane >> 5) in o0 (dvt = 0) / o1 (dvt = 1).  Written as they lie that is 16 8-byte
// stores per row; the end of a workgroup is bound by store ISSUE, so the column groups (g, g + 1) are paired across the
// lane halves first (v_permlane32_swap: the lower half ends up with [own g | upper's g] = columns 8 g .. 8 g + 7, the
// upper half with [lower's g + 1 | own g + 1]) and a row goes out as 8 16-byte stores.  `row` points at column 0 of
// this head.  +1.0 % on the 16-bit kernel (profiles/r04j_attn_wide_store.txt).
template <int DT, typename ACC>
__device__ __forceinline__ void store_o_row(unsigned short* row, int h, const ACC& o0, const ACC& o1, float inv) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  unsigned short* p = row + 8 * h;
#pragma unroll
  for (int dv = 0; dv < 2; ++dv) {
    const ACC& o = dv ? o1 : o0;
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const unsigned ax = pack2_h16<DT>(o[4 * g + 0] * inv, o[4 * g + 1] * inv);
      const unsigned ay = pack2_h16<DT>(o[4 * g + 2] * inv, o[4 * g + 3] * inv);
      const unsigned bx = pack2_h16<DT>(o[4 * g + 4] * inv, o[4 * g + 5] * inv);
      const unsigned by = pack2_h16<DT>(o[4 * g + 6] * inv, o[4 * g + 7] * inv);
      const auto sx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
      const auto sy = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
      u32x4_t pk;
      pk.x = sx[0]; pk.y = sy[0]; pk.z = sx[1]; pk.w = sy[1];
      *reinterpret_cast<u32x4_t*>(p + 32 * dv + 8 * g) = pk;
    }
  }
}

// ---- work item: q-tile qt of head hd of slice b (bh = b * heads + hd); the q-tiles of one (slice, head) are neighbours, so
//      they share an XCD's L2 for the K / V re-reads ----
struct AttnItem { int qt, bh, hd, b; };
__device__ __forceinline__ AttnItem attn_item(int q_tiles, int heads, int total) {
  const int item = xcd_remap(blockIdx.x, total);
  AttnItem w;
  w.qt = item % q_tiles;
  w.bh = item / q_tiles;
  w.hd = w.bh % heads;
  w.b = w.bh / heads;
  return w;
}
// the item's slice of a [slice][token][q | k | v][head][64] buffer: its first row, and a buffer descriptor over its rows --
// loads past the last token return 0 (no clamping VALU)
struct QkvSlice { const unsigned short* base; i32x4_t rsrc; };
__device__ __forceinline__ QkvSlice qkv_slice(const unsigned short* qkv, int b, int tokens, int ld) {
  QkvSlice s;
  s.base = qkv + (int64_t)b * tokens * ld;
  s.rsrc = lds_dma_rsrc(s.base, (unsigned)((int64_t)tokens * ld * 2));
  return s;
}

// ---- Q fragments (B operand of S^T = K Q^T), resident: the lane holds Q[qrow][16 i + 8 h .. + 7]; rows past the end are
//      clamped on load (their stores are guarded) ----
struct QFrag { s16x8_t q[4]; };
__device__ __forceinline__ QFrag load_q(const unsigned short* base, int qrow, int tokens, int ld, int hd, int h) {
  const unsigned short* qp = base + (int64_t)(qrow < tokens ? qrow : tokens - 1) * ld + hd * 64 + 8 * h;
  QFrag f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.q[i] = *reinterpret_cast<const s16x8_t*>(qp + 16 * i);
  return f;
}

// ---- staging by LDS-DMA: an operand image is 512 16-byte chunks, piece i of a workgroup's two fills linear positions
//      [256 i + tid, ...); the destination is lane-linear, so the swizzles of tile_off / v_off are applied by choosing which
//      (row, chunk) a lane FETCHES.  Position + 256 is the same chunk 32 rows further on (tile_pos, v_pos), so one voffset
//      per operand serves both pieces and the 32-row step is a constant. ----
struct KvStage { int voff_k, voff_v, tile_stride, half_stride; };
__device__ __forceinline__ KvStage kv_stage(int tid, int ld, int dmodel, int hd) {
  int r, cc, key, ch;
  tile_pos(tid, r, cc);
  v_pos(tid, key, ch);
  KvStage s;
  s.voff_k = (r * ld + dmodel + hd * 64 + cc * 8) * 2;
  s.voff_v = (key * ld + 2 * dmodel + hd * 64 + ch * 8) * 2;
  s.tile_stride = ATT_KT * ld * 2;
  s.half_stride = 32 * ld * 2;
  return s;
}
// Tile t of nt into the K | V buffer at LDS byte address dst (wave-uniform; the hardware adds lane * 16).  The LAST tile --
// the only one that can reach past the slice's rows -- carries its offset in the per-lane voffset: that is the operand the
// descriptor's range check is documented to cover, so rows >= tokens arrive as zeros whatever lies behind the slice (the
// next slice's rows, or uninitialised workspace whose NaN / Inf bit patterns would turn P = 0 times V into NaN).  Every
// other tile keeps the offset in the scalar operand: no VALU on the hot path.
__device__ __forceinline__ void stage_tile(i32x4_t rsrc, const KvStage& s, unsigned dst, int t, int nt) {
  const int so = t * s.tile_stride;
  if (t == nt - 1) {
    int vk = s.voff_k, vv = s.voff_v;   // opaque copies: the sums below are formed here, not kept alive through the loop
    asm volatile("" : "+v"(vk), "+v"(vv));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      lds_dma16(rsrc, dst + i * 4096, vk + so + i * s.half_stride, 0);
      lds_dma16(rsrc, dst + ATT_KV_TILE_BYTES + i * 4096, vv + so + i * s.half_stride, 0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      lds_dma16(rsrc, dst + i * 4096, s.voff_k, so + i * s.half_stride);
      lds_dma16(rsrc, dst + ATT_KV_TILE_BYTES + i * 4096, s.voff_v, so + i * s.half_stride);
    }
  }
}

// ---- per-lane LDS read bases (tile_off / v_off): the buffer, key half, key step s2, d half dvt and jj terms of a fragment's
//      address are immediates on one of these six registers ----
struct LdsBases { const char *ka0, *ka1, *ka2, *ka3, *va0, *va1; };
__device__ __forceinline__ LdsBases lds_bases(const char* smem, int lane) {
  const int h = lane >> 5, l31 = lane & 31;
  const int p_l = l31 >> 1;
  const int bslot = (((l31 & 1) << 3) | h) ^ (p_l & 15);
  LdsBases b;
  b.ka0 = smem + (p_l << 8) + ((bslot ^ 0) << 4);
  b.ka1 = smem + (p_l << 8) + ((bslot ^ 2) << 4);
  b.ka2 = smem + (p_l << 8) + ((bslot ^ 4) << 4);
  b.ka3 = smem + (p_l << 8) + ((bslot ^ 6) << 4);
  const int g16 = lane >> 4;                 // 16-lane group 0..3
  const int tr_q = (lane & 15) >> 2;         // row inside the 4-row block
  const int tr_p = lane & 3;
  const int tr_ch = 2 * (g16 & 1) + (tr_p >> 1);
  const int vl0 = 64 * (4 * h + tr_q) + 16 * (tr_ch ^ h) + 8 * (tr_p & 1);
  b.va0 = smem + vl0;          // jj = 0
  b.va1 = smem + (vl0 ^ 32);   // jj = 1: (key >> 2) & 3 gains 2 -> chunk index ^ 2
  return b;
}
// K rows (A operand of S^T = K Q^T) of 16-wide d chunk i; off = buffer + 4096 x key half
__device__ __forceinline__ s16x8_t ld_k(const LdsBases& b, int i, int off) {
  const char* base = i == 0 ? b.ka0 : i == 1 ? b.ka1 : i == 2 ? b.ka2 : b.ka3;
  return *reinterpret_cast<const s16x8_t*>(base + off);
}
// V^T (A operand of O^T = V^T P^T) of key step j >> 1 and d half j & 1, by transposing reads; off = V image + 4096 x key half
__device__ __forceinline__ s16x8_t ld_v(const LdsBases& b, int j, int off) {
  const int imm = off + 2048 * (j >> 1) + 512 * (j & 1);
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(b.va0 + imm));
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(b.va1 + imm + 1024));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- a 32 x 32 score tile S^T: the lane owns one query column and 16 of the 32 keys, its other lane half the rest ----
// maximum of m and the column's 32 scores; both lane halves agree (m = -INFINITY: of the column alone)
__device__ __forceinline__ float tile_max(const f32x16_t& s, float m) {
  float tmax = max3_f32(s[0], s[1], s[2]);
#pragma unroll
  for (int r = 3; r < 15; r += 2) tmax = max3_f32(tmax, s[r], s[r + 1]);
  tmax = fmaxf(tmax, s[15]);
  const unsigned tb = __float_as_uint(tmax);
  const auto sw = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);   // one of the two is tmax, the other the other half's
  return max3_f32(m, __uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
// ragged last tile: keys >= tokens contribute nothing (key0 = the tile's first key)
__device__ __forceinline__ void mask_keys(f32x16_t& s, int key0, int tokens, int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (key0 + acc_row(r, h) >= tokens) s[r] = -INFINITY;
}
// num / (row sum): l_run holds the sum over this lane half's keys
__device__ __forceinline__ float row_sum_inv(float l_run, float num = 1.0f) {
  const unsigned lb = __float_as_uint(l_run);
  const auto sw = __builtin_amdgcn_permlane32_swap(lb, lb, false, false);
  return num / (__uint_as_float(sw[0]) + __uint_as_float(sw[1]));
}
