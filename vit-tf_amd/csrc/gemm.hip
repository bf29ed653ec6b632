// MFMA GEMM for the ViT linears:  out = epilogue(A[rows][K] . W[N][K]^T + bias[N])
//
// Replaces nn.Linear (attn.qkv, attn.proj, mlp.fc1 + GELU, mlp.fc2) of the upstream DINO blocks that the
// reference runs through torch (infer.py:177 -> model(...)); the fused epilogues replace the separate
// bias / GELU / residual-add passes.
//
// Shape of the machine mapping (gfx950):
//   * 128 x 128 output tile per 256-thread workgroup, 4 waves as 2 (m) x 2 (n), each wave 64 x 64
//   * K step 64; A and W tiles are [128][64 x 16 bit] images (16 KB each) filled by global_load_lds_dwordx4
//     (no VGPR staging); the XOR swizzle of tile_off() is applied on the per-lane SOURCE address because the
//     LDS destination of an LDS-DMA is lane-linear; one stage + 4 workgroups per CU (the K = 384 shapes have
//     only six K steps, so latency is hidden across workgroups, not inside one)
//   * v_mfma_f32_32x32x16 with W as the A operand and the activations as the B operand, i.e. the wave
//     computes C^T: a lane then owns ONE activation row and 4 consecutive output columns per register quad,
//     so bias loads are float4 and stores are 8 B (16-bit out) or 16 B (fp32 residual) per lane
//   * workgroups are remapped so that consecutive tiles (which share the A panel) run on one XCD's L2
//
// This file also holds the dispatch of every linear (vittf_gemm, vittf_gemm_residual_ln, vittf_gemm_kfeat_parts): which of
// the three GEMM kernels takes a shape is asked of the coverage predicates beside the other two (vittf_internal.h); the tiles
// here take the rest.  One K-feature epilogue (EPI_KFEAT_PARTS): vittf_gemm(VITTF_EPI_KFEAT) is its one-slot launch.
#include "vittf_internal.h"

#include <stdlib.h>

namespace {

// LDS-only synchronisation for the epilogue: __syncthreads() also drains vmcnt(0), i.e. the residual read-modify-write
// of the first half tile would be waited for before the second half is even staged
#define GEMM_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KB

// issue the LDS-DMA of one [128][64] operand tile: 1024 16-byte chunks, 4 per thread (asm pieces, see lds_dma16:
// with the builtin, hipcc drains vmcnt(0) before the fragment reads of the tile being multiplied, which is what
// made the two-stage pipeline slower than the single stage)
template <typename T>
__device__ __forceinline__ void stage_tile(const T* __restrict__ src, int64_t ld, int64_t row0, int64_t row_max,
                                           int k0, unsigned lds_tile, int tid, const int (&voff)[4]) {
  // descriptor over the tile's rows [row0, min(row0 + 127, row_max)]: rows past the end read as zeros (never stored)
  const int64_t nrows = row_max - row0 + 1 < 128 ? row_max - row0 + 1 : 128;
  const i32x4_t rsrc = lds_dma_rsrc(src + row0 * ld, (unsigned)(nrows * ld * 2));
#pragma unroll
  for (int i = 0; i < 4; ++i) lds_dma16(rsrc, lds_tile + i * 4096, voff[i], k0 * 2);
}

// The K-feature epilogue (the hooked tensor: fp16 values, the leading rows of every slice dropped), for several thirds of
// attn.qkv in one launch (vittf_gemm_kfeat_parts): W / bias are the whole [n = 3 d][k] / [3 d] of the projection and the
// grid covers only the column tiles of the requested thirds, slot s of them = third part[s]; each third leaves into its own
// [rows - dropped rows][d] output.  vittf_gemm(VITTF_EPI_KFEAT) is the same launch with one slot: its [n][k] weights as
// third 0 of width d = n, drop = 1.  A tile's bits depend on its weight rows, bias and activations, not on the slot.
constexpr int EPI_KFEAT_PARTS = 100;      // (internal epilogue id)
struct KfeatParts {
  unsigned short* out[3];   // by third (q, k, v)
  int part[3];              // slot -> third
  int d;
  int drop;                 // leading rows of a slice that are dropped: CLS + the register tokens
};

template <int DT, int EPI>
__global__ __launch_bounds__(256, 4) void gemm_kernel(const unsigned short* __restrict__ A,
                                                      const unsigned short* __restrict__ W,
                                                      const float* __restrict__ bias, void* __restrict__ out,
                                                      int64_t rows, int n, int k, int tokens, int n_tiles,
                                                      int total_tiles, KfeatParts kp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [A tile | W tile], then the epilogue's C tile
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, l31 = lane & 31;

  const int tile = xcd_remap(blockIdx.x, total_tiles);
  const int mt = tile / n_tiles, nt = tile - mt * n_tiles;
  const int64_t m0 = (int64_t)mt * BM;
  int n0 = nt * BN;
  [[maybe_unused]] unsigned short* part_out = nullptr;   // (EPI_KFEAT_PARTS) this tile's third: output, first column
  [[maybe_unused]] int part_col0 = 0;
  if constexpr (EPI == EPI_KFEAT_PARTS) {
    const int slot = n0 / kp.d;
    part_col0 = n0 - slot * kp.d;
    n0 = kp.part[slot] * kp.d + part_col0;
    part_out = kp.out[kp.part[slot]];
  }

  f32x16_t acc[2][2];  // [ni][mi]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = k / BK;
  int voff[4];   // LDS-DMA source offsets: chunk q = i * 256 + tid of a tile image <- (row, 16-byte chunk) = tile_pos(q)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int r, c;
    tile_pos(i * 256 + tid, r, c);
    voff[i] = (r * k + c * 8) * 2;
  }
  const unsigned lds_wave = (unsigned)(size_t)LDS_PTR(smem) + (__builtin_amdgcn_readfirstlane(tid & ~63) << 4);
  auto compute_tile = [&](const char* a_t, const char* w_t) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = 2 * s + h;
      s16x8_t af[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const s16x8_t*>(a_t + tile_off(wm * 64 + i * 32 + l31, c));
        wf[i] = *reinterpret_cast<const s16x8_t*>(w_t + tile_off(wn * 64 + i * 32 + l31, c));
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) acc[ni][mi] = mfma32<DT>(wf[ni], af[mi], acc[ni][mi]);
    }
  };
  // one 32 KB stage, four workgroups per CU: the other workgroups' MFMAs cover this one's load latency
  for (int t = 0; t < nk; ++t) {
    stage_tile(A, k, m0, rows - 1, t * BK, lds_wave, tid, voff);
    stage_tile(W, k, n0, n - 1, t * BK, lds_wave + TILE_BYTES, tid, voff);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    compute_tile(smem, smem + TILE_BYTES);
    __syncthreads();
  }

  // ---- epilogue ----
  // The accumulators hold C^T: a lane owns activation row m (per mi) and columns nb + 8g + 4h + {0..3}.
  if constexpr (EPI == VITTF_EPI_BIAS_RESIDUAL) {
    // fp32 read-modify-write of the residual stream, also re-tiled through LDS so that every global access is a
    // whole 256-byte row segment: two passes of 64 columns (the 128 x 64 fp32 half tile is 32 KB + padding)
    constexpr int CSF = 64 * 4 + 16;
    float* xo = reinterpret_cast<float*>(out);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half) GEMM_LDS_BARRIER();
      if (wn == half) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          const int ml = wm * 64 + mi * 32 + l31;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int nl = ni * 32 + 8 * g + 4 * h;          // column inside this 64-wide half
              const float4 bv = *reinterpret_cast<const float4*>(bias + n0 + half * 64 + nl);
              float4 v;
              v.x = acc[ni][mi][4 * g + 0] + bv.x; v.y = acc[ni][mi][4 * g + 1] + bv.y;
              v.z = acc[ni][mi][4 * g + 2] + bv.z; v.w = acc[ni][mi][4 * g + 3] + bv.w;
              *reinterpret_cast<float4*>(smem + ml * CSF + nl * 4) = v;
            }
          }
        }
      }
      GEMM_LDS_BARRIER();
#pragma unroll
      for (int pass = 0; pass < 8; ++pass) {
        const int rl = pass * 16 + (tid >> 4);
        const int64_t m = m0 + rl;
        if (m >= rows) continue;
        const float4 d = *reinterpret_cast<const float4*>(smem + rl * CSF + (tid & 15) * 16);
        float4* p = reinterpret_cast<float4*>(xo + m * n + n0 + half * 64 + (tid & 15) * 4);
        float4 x = *p;
        x.x += d.x; x.y += d.y; x.z += d.z; x.w += d.w;
        *p = x;
      }
    }
  } else {
    // 16-bit outputs go through LDS so that global stores are whole 256-byte rows (16 lanes x 16 B): storing the
    // register fragments directly puts 16-byte pieces on 32 different rows per instruction and halves the GEMM's
    // speed (measured: 0.23 -> 0.12 ms for the qkv shape with the stores removed).
    // The K loop ended on a barrier, so the operand tiles are dead; C tile rows are padded to 272 B.
    constexpr int CS = BN * 2 + 16;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int ml = wm * 64 + mi * 32 + l31;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int nl = wn * 64 + ni * 32 + 8 * g + 4 * h;
          const float4 bv = *reinterpret_cast<const float4*>(bias + n0 + nl);
          float v0 = acc[ni][mi][4 * g + 0] + bv.x;
          float v1 = acc[ni][mi][4 * g + 1] + bv.y;
          float v2 = acc[ni][mi][4 * g + 2] + bv.z;
          float v3 = acc[ni][mi][4 * g + 3] + bv.w;
          if constexpr (EPI == VITTF_EPI_BIAS_GELU) {
            v0 = gelu_poly(v0); v1 = gelu_poly(v1); v2 = gelu_poly(v2); v3 = gelu_poly(v3);
          }
          if constexpr (EPI == VITTF_EPI_BIAS_QKV) {
            // the q third carries the softmax scale and the exp -> exp2 base change: one rounding, like plain q
            const float sc = (n0 + nl) < n / 3 ? VITTF_Q_PRESCALE : 1.0f;
            v0 *= sc; v1 *= sc; v2 *= sc; v3 *= sc;
          }
          uint2 pk;
          if constexpr (EPI == EPI_KFEAT_PARTS) {
            pk.x = pack2_h16<VITTF_FP16>(v0, v1);
            pk.y = pack2_h16<VITTF_FP16>(v2, v3);
          } else {
            pk.x = pack2_h16<DT>(v0, v1);
            pk.y = pack2_h16<DT>(v2, v3);
          }
          *reinterpret_cast<uint2*>(smem + ml * CS + nl * 2) = pk;
        }
      }
    }
    GEMM_LDS_BARRIER();
    unsigned short* o16 = reinterpret_cast<unsigned short*>(out);
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
      const int rl = pass * 16 + (tid >> 4);
      const int64_t m = m0 + rl;
      if (m >= rows) continue;
      int64_t orow = m;
      if constexpr (EPI == EPI_KFEAT_PARTS) {
        const int64_t b = m / tokens;
        const int tok = (int)(m - b * tokens);
        // CLS row dropped (infer.py:202 k[:, 1:]), and the register rows behind it
        if (tok < kp.drop) continue;
        orow = b * (tokens - kp.drop) + tok - kp.drop;
      }
      const uint4 v = *reinterpret_cast<const uint4*>(smem + rl * CS + (tid & 15) * 16);
      if constexpr (EPI == EPI_KFEAT_PARTS)
        *reinterpret_cast<uint4*>(part_out + orow * kp.d + part_col0 + (tid & 15) * 8) = v;
      else
        *reinterpret_cast<uint4*>(o16 + orow * n + n0 + (tid & 15) * 8) = v;
    }
  }
}

// kp: the K-feature launch (n = the weight rows W holds, part_tiles = the column tiles of its slots), else epi's epilogue
template <int DT>
int launch_gemm(const void* a, const void* w, const float* bias, void* out, int64_t rows, int n, int k, int epi,
                int tokens, hipStream_t st, const KfeatParts* kp = nullptr, int part_tiles = 0) {
  const int64_t m_tiles = (rows + BM - 1) / BM;
  const int n_tiles = kp ? part_tiles : n / BN;
  if (m_tiles * n_tiles > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  const int total = (int)(m_tiles * n_tiles);
  // one stage, not two: +16 % on the K = 384 shapes, whose six K steps are too short for a double buffer to pay
  const size_t lds = (size_t)BM * (BN * 2 + 16);   // 32 KB stage / padded C tile (16-bit: 128 x 272 B; fp32 half tile: 128 x 272 B)
  const unsigned short* A = (const unsigned short*)a;
  const unsigned short* Wp = (const unsigned short*)w;
#define VITTF_GEMM_CASE(E)                                                                                   \
  case E:                                                                                                    \
    hipLaunchKernelGGL((gemm_kernel<DT, E>), dim3(total), dim3(256), lds, st, A, Wp, bias, out, rows, n, k,  \
                       tokens, n_tiles, total, kp ? *kp : KfeatParts{});                                     \
    break;
  switch (kp ? EPI_KFEAT_PARTS : epi) {
    VITTF_GEMM_CASE(VITTF_EPI_BIAS)
    VITTF_GEMM_CASE(VITTF_EPI_BIAS_GELU)
    VITTF_GEMM_CASE(VITTF_EPI_BIAS_RESIDUAL)
    VITTF_GEMM_CASE(VITTF_EPI_BIAS_QKV)
    VITTF_GEMM_CASE(EPI_KFEAT_PARTS)
    default: return VITTF_ERR_INVALID_ARG;
  }
#undef VITTF_GEMM_CASE
  return vittf_check_launch();
}

// the K-feature launch of the thirds in `mask` (third p of w [.. ][k] -> outs[p], `drop` leading rows of a slice dropped)
int launch_gemm_kfeat(const void* a, const void* w, const float* bias, int64_t rows, int d, int k, int tokens, int drop,
                      int mask, int w_rows, void* const outs[3], int dtype, hipStream_t st) {
  KfeatParts kp{};
  int slots = 0;
  for (int p = 0; p < 3; ++p) {
    kp.out[p] = (unsigned short*)outs[p];
    if ((mask >> p) & 1) kp.part[slots++] = p;
  }
  kp.d = d;
  kp.drop = drop;
  const int part_tiles = slots * (d / BN);
  if (dtype == VITTF_BF16) return launch_gemm<VITTF_BF16>(a, w, bias, nullptr, rows, w_rows, k, 0, tokens, st, &kp, part_tiles);
  if (dtype == VITTF_FP16) return launch_gemm<VITTF_FP16>(a, w, bias, nullptr, rows, w_rows, k, 0, tokens, st, &kp, part_tiles);
  return VITTF_ERR_INVALID_ARG;
}

// Residual linears with 384 / 768 output columns (ViT-S / ViT-B proj and fc2) ask the whole-row kernel of gemm_rows.hip
// first -- except 768 columns from K = 3072 on (ViT-B fc2), which ask the persistent kernel first: the LayerNorm behind
// it then runs as its own launch instead of in the whole-row kernel's epilogue, 1.56 against 1.87 ms per 64 slices.
bool rows_first(int n, int k) { return n == 384 || (n == 768 && k < 3072); }

}  // namespace

// Dispatch of a linear, in this order: the whole-row kernel (residual epilogue, rows_first, vittf_gemm_rows_covers), the
// persistent 256 x 256 kernel (vittf_gemm_pp_covers + vittf_gemm_pp_covers_out: K >= 768 with N % 256 == 0, the ViT-B
// linears), the 128 x 128 tiles of this file.  The predicates are the only place a kernel's coverage is written down.
extern "C" int vittf_gemm(const void* a, const void* w, const float* bias, void* out, int64_t rows, int32_t n,
                          int32_t k, int32_t epilogue, int32_t tokens, int32_t dtype, void* stream) {
  if (!a || !w || !bias || !out || rows <= 0 || n <= 0 || k <= 0) return VITTF_ERR_INVALID_ARG;
  if (n % BN != 0 || k % BK != 0) return VITTF_ERR_INVALID_ARG;
  if (epilogue < VITTF_EPI_BIAS || epilogue > VITTF_EPI_BIAS_QKV) return VITTF_ERR_INVALID_ARG;
  if (epilogue == VITTF_EPI_KFEAT && tokens < 2) return VITTF_ERR_INVALID_ARG;
  if (rows / BM + 1 > (1 << 20)) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (epilogue == VITTF_EPI_BIAS_RESIDUAL && rows_first(n, k) && vittf_gemm_rows_covers(n, k, rows))
    return vittf_gemm_rows(a, w, bias, (float*)out, rows, n, k, dtype, nullptr, nullptr, 0.f, nullptr, st);
  const int64_t kfeat_bytes = epilogue == VITTF_EPI_KFEAT ? vittf_kfeat_out_bytes(rows, n, tokens, 1) : 0;
  if (vittf_gemm_pp_covers(k, n, a, w) && vittf_gemm_pp_covers_out(out, kfeat_bytes))
    return vittf_gemm_pp(a, w, bias, out, rows, n, k, epilogue, tokens, dtype, st);
  if (epilogue == VITTF_EPI_KFEAT) {   // one slot: the [n][k] weights as third 0 of width n, the CLS row dropped
    void* const outs[3] = {out, nullptr, nullptr};
    return launch_gemm_kfeat(a, w, bias, rows, n, k, tokens, 1, 1, n, outs, dtype, st);
  }
  if (dtype == VITTF_BF16) return launch_gemm<VITTF_BF16>(a, w, bias, out, rows, n, k, epilogue, tokens, st);
  if (dtype == VITTF_FP16) return launch_gemm<VITTF_FP16>(a, w, bias, out, rows, n, k, epilogue, tokens, st);
  return VITTF_ERR_INVALID_ARG;
}

// The thirds of attn.qkv selected by part_mask (bit 0 q, 1 k, 2 v) in one launch per kernel, each with the K-feature epilogue
// into its own output.  Every third runs on the kernel its own vittf_gemm(EPI_KFEAT) call would take -- the persistent
// 256 x 256 kernel where it covers the shape, alignment and output size, else the 128 x 128 tiles --, so its bits are that
// call's.  n_reg register tokens behind CLS (DINOv2 _reg models) are dropped with it: rows tok <= n_reg of a slice go, the
// others move up by 1 + n_reg; the arithmetic of a kept row does not depend on n_reg.
extern "C" int vittf_gemm_kfeat_parts_reg(const void* a, const void* w, const float* bias, int64_t rows, int32_t d, int32_t k,
                                          int32_t tokens, int32_t n_reg, int32_t part_mask, void* q_out, void* k_out,
                                          void* v_out, int32_t dtype, void* stream) {
  void* const outs[3] = {q_out, k_out, v_out};
  if (!a || !w || !bias || rows <= 0 || d <= 0 || k <= 0) return VITTF_ERR_INVALID_ARG;
  if (n_reg < 0 || n_reg > VITTF_MAX_REGISTER_TOKENS || tokens < 2 + n_reg) return VITTF_ERR_INVALID_ARG;
  if (part_mask <= 0 || part_mask > 7) return VITTF_ERR_INVALID_ARG;
  for (int p = 0; p < 3; ++p)
    if (((part_mask >> p) & 1) && !outs[p]) return VITTF_ERR_INVALID_ARG;
  if (d % BN != 0 || k % BK != 0) return VITTF_ERR_INVALID_ARG;
  if (rows / BM + 1 > (1 << 20)) return VITTF_ERR_INVALID_ARG;
  if (dtype != VITTF_BF16 && dtype != VITTF_FP16) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  int32_t taken = 0;
  const int rc = vittf_gemm_pp_kfeat_parts(a, w, bias, rows, d, k, tokens, n_reg, part_mask, outs, dtype, st, &taken);
  if (rc != VITTF_OK) return rc;
  const int rest = part_mask & ~taken;
  if (!rest) return VITTF_OK;
  vittf_note_kernel(VITTF_KERNEL_GEMM, "gemm_kernel");   // (the projection is the engine's last launch: its class name tells which ran)
  return launch_gemm_kfeat(a, w, bias, rows, d, k, tokens, 1 + n_reg, rest, 3 * d, outs, dtype, st);
}

extern "C" int vittf_gemm_kfeat_parts(const void* a, const void* w, const float* bias, int64_t rows, int32_t d, int32_t k,
                                      int32_t tokens, int32_t part_mask, void* q_out, void* k_out, void* v_out, int32_t dtype,
                                      void* stream) {
  return vittf_gemm_kfeat_parts_reg(a, w, bias, rows, d, k, tokens, 0, part_mask, q_out, k_out, v_out, dtype, stream);
}

// x += a . w^T + bias (fp32 residual stream, n = 384), then h = LayerNorm(x; g, b) as the 16-bit operand of the next
// GEMM: whole-row kernel with the LayerNorm in its epilogue; shapes it does not cover take the two separate kernels.
extern "C" int vittf_gemm_residual_ln(const void* a, const void* w, const float* bias, float* x, int64_t rows, int32_t n,
                                      int32_t k, int32_t dtype, const float* ln_g, const float* ln_b, float ln_eps, void* h,
                                      void* stream) {
  if (!a || !w || !bias || !x || !ln_g || !ln_b || !h || rows <= 0 || n <= 0 || k <= 0) return VITTF_ERR_INVALID_ARG;
  if (dtype != VITTF_BF16 && dtype != VITTF_FP16) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (rows_first(n, k) && vittf_gemm_rows_covers(n, k, rows))
    return vittf_gemm_rows(a, w, bias, x, rows, n, k, dtype, ln_g, ln_b, ln_eps, h, st);
  const int rc = vittf_gemm(a, w, bias, x, rows, n, k, VITTF_EPI_BIAS_RESIDUAL, 0, dtype, stream);
  if (rc != VITTF_OK) return rc;
  return vittf_layernorm(x, ln_g, ln_b, h, rows, n, ln_eps, dtype, stream);
}
