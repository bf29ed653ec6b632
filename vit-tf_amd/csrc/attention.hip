// Flash-style multi-head self-attention forward, head dim 64, for the DINO ViT blocks.
//
// Replaces Attention.forward of the upstream model the reference calls (infer.py:177):
//   softmax(q k^T / sqrt(64)) v  per head, without materialising the N x N score matrix.
//
// Machine mapping (gfx950, wave64):
//   * one 256-thread workgroup = 4 waves = 128 query rows of one (slice, head); each wave owns 32 query rows
//   * K/V tiles of 64 keys are register-staged (buffer_load_dwordx4 issued before the tile's MFMAs, ds_write
//     after them) into two LDS buffers, one barrier per tile; the buffer descriptor's range check zero-fills rows
//     past the end of the slice, the tile offset rides in the scalar offset, so the prefetch costs no VALU
//   * scores are computed TRANSPOSED, S^T = K Q^T with v_mfma_f32_32x32x16 (K rows as the A operand, Q rows as
//     the B operand, Q fragments live in registers for the whole kernel), so a lane owns one query column:
//     the row maximum / row sum of the online softmax are in-lane reductions plus ONE v_permlane32_swap
//   * the S^T accumulator registers, converted pairwise to 16 bit (v_cvt_pk), are directly the B operand of the
//     second product O^T = V^T P^T (k order 16s + 8(j>>2) + 4h + (j&3)); the matching V^T A-fragments come from
//     ds_read_b64_tr_b16 transposed reads of a row-major V image (8-row x 32-col subtiles, conflict free)
//   * the K image uses the tile_off() swizzle shared with the GEMM and is read with ds_read_b128
//   * every LDS address is a per-lane base computed once + an immediate (the two buffers are two instantiations
//     of the tile body): the kernel is VALU-bound at head dim 64 (PMC: VALU 75 % busy vs MFMA 38 %), so address
//     arithmetic inside the loop is what was removed first
//   * exp2 with the softmax scale folded into one FMA: p = exp2(s*c - m*c), c = log2(e)/8
//   * token count need not be tile aligned (N = f0*f1 + 1): the last key tile is masked to -inf, query rows
//     past the end are clamped on load and their stores are guarded
//   * workgroups are remapped so that the q-tiles of one (slice, head) share an XCD's L2 (K/V re-reads)
#include "attn_common.h"
#include "vittf_internal.h"

#include <stdlib.h>

namespace {

constexpr int QT = 128;   // query rows per workgroup

// One 64-key tile for this wave's 32 query rows.  BUF selects the LDS buffer at compile time so that every
// ds_read offset is an immediate on one of six per-lane base registers.  LAST masks keys >= tokens.
template <int DT, int BUF, bool LAST>
__device__ __forceinline__ void attn_tile(const LdsBases& lb, const QFrag& q, f32x16_t& o0, f32x16_t& o1, float& m_run,
                                          float& l_run, int t, int tokens, int h, float c) {
  // Two 32-key halves, each carried from S^T to O^T: the score registers (16) and the P fragments (8) of one half are
  // (nearly) all that is live.  The halves are NOT fenced off from each other any more: within the register budget of
  // the launch bounds hipcc sinks the O^T MFMAs of one half into the exp2 stream of the next (an `s_nop 10` behind the
  // S^T chain otherwise idles the wave): -1.5 % per launch in the pipeline, no spills (168 / 128 VGPRs).
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    constexpr int kb = BUF * ATT_BUF_BYTES;
    f32x16_t sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) sacc = mfma32<DT>(ld_k(lb, i, kb + 4096 * kt), q.q[i], sacc);
    if constexpr (LAST) mask_keys(sacc, t * ATT_KT + 32 * kt, tokens, h);

    float p[16];
    // ---- online softmax (lane = one query column; 16 of the half's 32 keys are in this lane) ----
    const float m_new = tile_max(sacc, m_run);
    const float mc = m_new * c;
    if (!__all(m_new == m_run)) {   // rare after the first tiles: rescale what was accumulated at the old maximum
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
      l_run *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
      m_run = m_new;
    }
    float psum0 = 0.f, psum1 = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      p[r] = __builtin_amdgcn_exp2f(fmaf(sacc[r], c, -mc));
      p[r + 1] = __builtin_amdgcn_exp2f(fmaf(sacc[r + 1], c, -mc));
      psum0 += p[r];
      psum1 += p[r + 1];
    }
    l_run += psum0 + psum1;
    s16x8_t pf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4_t u;
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = pack2_h16<DT>(p[8 * s2 + 2 * j], p[8 * s2 + 2 * j + 1]);
      pf[s2] = __builtin_bit_cast(s16x8_t, u);
    }

    // ---- O^T += V^T P^T for these 32 keys ----
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const s16x8_t vf = ld_v(lb, j, kb + ATT_KV_TILE_BYTES + 4096 * kt);
      if (j & 1) o1 = mfma32<DT>(vf, pf[j >> 1], o1);
      else       o0 = mfma32<DT>(vf, pf[j >> 1], o0);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256, 4) void attn_kernel(const unsigned short* __restrict__ qkv,
                                                      unsigned short* __restrict__ out, int tokens, int heads,
                                                      int q_tiles, int total, float c) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ATT_BUF_BYTES];  // [buffer][K | V]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;

  const AttnItem w = attn_item(q_tiles, heads, total);
  const int dmodel = heads * 64;
  const int ld = 3 * dmodel;                                   // elements per token row of qkv
  const QkvSlice sl = qkv_slice(qkv, w.b, tokens, ld);

  const int qrow = w.qt * QT + wave * 32 + l31;
  QFrag q = load_q(sl.base, qrow, tokens, ld, w.hd, h);

  // ---- staging: LDS-DMA (buffer_load_dwordx4 ... lds), no staging registers and no ds_write ----
  const KvStage stg = kv_stage(tid, ld, dmodel, w.hd);
  const int nt = (tokens + ATT_KT - 1) / ATT_KT;
  // wave-uniform LDS byte address; the hardware adds lane * 16.  (asm pieces, see lds_dma16: with the builtin hipcc
  // put s_waitcnt vmcnt(0) in front of the V reads in the middle of every tile.)
  const unsigned dma_dst = (unsigned)(size_t)LDS_PTR(smem) + (__builtin_amdgcn_readfirstlane(tid & ~63) << 4);
  auto stage = [&](int t, int buf) { stage_tile(sl.rsrc, stg, dma_dst + buf * ATT_BUF_BYTES, t, nt); };

  const LdsBases lb = lds_bases(smem, lane);

  f32x16_t o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // Retire the Q loads here: otherwise hipcc's waitcnt pass re-waits for the Q registers inside the loop.
  asm volatile("" : "+v"(q.q[0]), "+v"(q.q[1]), "+v"(q.q[2]), "+v"(q.q[3]));

  // N = f0*f1 + 1 leaves the last q-tile with a single valid row: waves whose 32 rows are all past the end keep
  // staging and synchronising but skip the arithmetic (3 of 4 waves in 1 of 33 workgroups at N = 4097)
  const bool active = __builtin_amdgcn_readfirstlane(w.qt * QT + wave * 32) < tokens;
  int t = 0;
  if (!active) {   // a separate loop: with `if (active)` around the tile body hipcc keeps the 32 output accumulators in
                   // two register sets and copies them at every loop head (32 v_mov per tile on the hot path)
    for (; t + 1 < nt; ++t) {
      stage(t + 1, (t + 1) & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    return;
  }
  // every tile but the last: the DMA of tile t + 1 flies under the MFMAs of t.  Two tiles per trip, straight-line (an
  // `if (t & 1)` diamond makes hipcc give the two ring-buffer variants different accumulator registers + copies)
#define ATTN_STEP(BUFC, BUFN)                                                                                          \
  {                                                                                                                    \
    stage(t + 1, BUFN);                                                                                                \
    attn_tile<DT, BUFC, false>(lb, q, o0, o1, m_run, l_run, t, tokens, h, c);                                          \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* this wave's DMA pieces have landed ... */                    \
    __syncthreads();                                    /* ... and everybody's have, and everybody is done reading */  \
    ++t;                                                                                                               \
  }
  while (t + 2 < nt) {
    ATTN_STEP(0, 1)
    ATTN_STEP(1, 0)
  }
  if (t + 1 < nt) ATTN_STEP(0, 1)
#undef ATTN_STEP
  if (t & 1) attn_tile<DT, 1, true>(lb, q, o0, o1, m_run, l_run, t, tokens, h, c);
  else       attn_tile<DT, 0, true>(lb, q, o0, o1, m_run, l_run, t, tokens, h, c);

  // ---- normalise and store: lane owns query row `qrow` (store_o_row pairs its columns into 16-byte runs) ----
  const float inv = row_sum_inv(l_run);
  if (qrow < tokens) store_o_row<DT>(out + ((int64_t)w.b * tokens + qrow) * dmodel + w.hd * 64, h, o0, o1, inv);
}

}  // namespace

extern "C" int vittf_attention(const void* qkv, void* out, int32_t batch, int32_t tokens, int32_t heads,
                               int32_t dtype, int32_t q_prescaled, void* stream) {
  if (!qkv || !out || batch <= 0 || tokens <= 0 || heads <= 0) return VITTF_ERR_INVALID_ARG;
  // 32-bit byte offsets inside one slice's qkv rows (buffer addressing)
  if ((int64_t)(tokens + ATT_KT) * heads * 64 * 3 * 2 > 0x7fffffffLL) return VITTF_ERR_INVALID_ARG;
  const int q_tiles = (tokens + QT - 1) / QT;
  const int64_t total64 = (int64_t)batch * heads * q_tiles;
  if (total64 > (1 << 30)) return VITTF_ERR_INVALID_ARG;
  const int total = (int)total64;
  hipStream_t st = (hipStream_t)stream;
  if (q_prescaled) {
    // pre-scaled q (what the engine runs): attention_pp64.hip, two 32-row query blocks per wave taking turns, two waves per SIMD
    if (dtype != VITTF_BF16 && dtype != VITTF_FP16) return VITTF_ERR_INVALID_ARG;
    vittf_note_kernel(VITTF_KERNEL_ATTENTION, "attn_pp64_kernel");
    return vittf_attention_pp64(qkv, out, batch, tokens, heads, dtype, st);
  }
  // q as the model produces it: the online-maximum kernel of this file
#define VITTF_ATTN_LAUNCH(DTV)                                                                              \
  hipLaunchKernelGGL((attn_kernel<DTV>), dim3(total), dim3(256), 0, st, (const unsigned short*)qkv,  \
                     (unsigned short*)out, tokens, heads, q_tiles, total, VITTF_Q_PRESCALE)
  vittf_note_kernel(VITTF_KERNEL_ATTENTION, "attn_kernel<online maximum>");
  if (dtype == VITTF_BF16) VITTF_ATTN_LAUNCH(VITTF_BF16);
  else if (dtype == VITTF_FP16) VITTF_ATTN_LAUNCH(VITTF_FP16);
  else return VITTF_ERR_INVALID_ARG;
#undef VITTF_ATTN_LAUNCH
  return vittf_check_launch();
}
