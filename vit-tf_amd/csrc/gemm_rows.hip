// Whole-row MFMA GEMM for the residual linears (attn.proj, mlp.fc2) of ViT-S (D = 384) and ViT-B (D = 768):
//     x[rows][D] (fp32) += A[rows][K] . W[D][K]^T + bias          (K = D or 4 D)
// and, optionally in the same pass, the next LayerNorm:  h[rows][D] (16 bit) = LayerNorm(x_new; g, b).
// (The text below describes D = 384; D = 768 is the same kernel with 8 waves side by side on 128 rows: RowsCfg.)
//
// Why next to gemm.hip: a 128 x 128 tile moves 32 KB of operands from L2 into LDS per 64-wide K step, 2.36 GB per fc2
// launch, and its run time follows L2->LDS bytes / ~17 TB/s + HBM bytes / ~5 TB/s.  Here a workgroup owns whole rows:
// 8 KB (activations) + 24 KB (all 384 weight rows) per 32-wide K step for 128 x 384 outputs = 1.57 GB per launch
// (0.98 GB with 256-row workgroups), and because the rows are whole the LayerNorm that follows every residual add can
// be computed on the way out instead of by a separate kernel that re-reads the 201 MB stream.
//
//   * a wave owns 128 x 96 outputs = 12 accumulator tiles (192 VGPRs; 2 waves per SIMD), computed transposed (weights =
//     MFMA A operand, activations = B operand) like the other GEMMs; per 16-wide K slice 4 + 3 fragment reads feed 12
//     MFMAs.  Default (VITTF_ROWS_WM=1): workgroup = 4 waves side by side = 128 rows x 384 columns, 2-deep ring of
//     32 KB stages, two workgroups per CU (each covers the other's DMA latency; finer tiles at the launch's tail);
//     VITTF_ROWS_WM=2: 8 waves as 2 (rows) x 4 (columns) = 256 rows, 3-deep ring of 40 KB stages, one workgroup per
//     CU (half the weight re-reads; same speed in isolation, 1 % slower in the pipeline).
//   * operands arrive by LDS-DMA (asm pieces), one bare barrier per 32-wide K step; a [R][32] operand image is stored
//     as R / 2 "double rows" of 128 B in the tile_off() layout (rows 2 j and 2 j + 1 side by side), which keeps the
//     16-byte fragment reads conflict-free.
//   * epilogue in four rounds of 32 rows per row half through a padded fp32 LDS tile (it reuses the ring), each round
//     in two passes: 16 lanes per row do the read-modify-write as 256-byte runs with the x of the next pass
//     already in flight, and -- with the whole row in those 16 lanes' registers -- the LayerNorm statistics,
//     affine transform and 16-bit store.
//   * a partial last tile reads zeros for its missing rows and drops their outputs, so a row's bits do not depend on
//     where it sits in a launch (1 rank and N ranks batch the slices differently and must write the same file).
//   * where the time goes, measured with timing-only builds: fc2 + LayerNorm 0.235 ms without MFMAs, 0.19 ms without the
//     epilogue, 0.30 ms complete.
#include "vittf_internal.h"

#include <stdlib.h>

namespace {

constexpr int RBK = 32;

// RN = output columns = the embedding width: 384 (ViT-S) or 768 (ViT-B); a wave owns 96 of them, so NW = 4 or 8 waves
// side by side.
// WM = row halves per workgroup: 2 -> 256 rows, 8 waves, 3-deep ring, one workgroup per CU (RN = 384 only);
//                                1 -> 128 rows, NW waves, 2-deep ring; RN = 384: two workgroups per CU (the epilogue of
//                                     one overlaps the K loop of the other; the weight image is staged twice as often),
//                                     RN = 768: 8 waves, 56 KB stages, one workgroup per CU
template <int WM, int RN>
struct RowsCfg {
  static constexpr int NW = RN / 96;
  static constexpr int BM = 128 * WM, THREADS = 64 * WM * NW;
  static constexpr int A_BYTES = BM * RBK * 2;                // 16 / 8 KB
  static constexpr int RW_BYTES = RN * RBK * 2;               // 24 / 48 KB
  static constexpr int STAGE = A_BYTES + RW_BYTES;            // 40 / 32 / 56 KB
  static constexpr int STAGES = WM == 2 ? 3 : 2;
  static constexpr int LDS = STAGES * STAGE;                  // 122,880 / 65,536 / 114,688 B
  static constexpr int RCS = RN * 4 + 16;                     // fp32 staging row stride
  static constexpr int BIAS_OFF = 32 * WM * RCS;              // bias / gamma / beta behind the staging tile
  static constexpr int A_PIECES = A_BYTES / (THREADS * 16);   // 2 / 2 / 1 LDS-DMA pieces per thread and stage
  static constexpr int W_PIECES = RW_BYTES / (THREADS * 16);  // 6 / 3 / 6
  static constexpr int LPR = RN / 24;                         // epilogue: lanes per row (24 values each): 16 / 32
  static_assert(RN == 384 || (RN == 768 && WM == 1), "shapes: 384 columns (128 / 256 rows) or 768 columns (128 rows)");
  static_assert(A_PIECES * THREADS * 16 == A_BYTES && W_PIECES * THREADS * 16 == RW_BYTES && (W_PIECES == 3 || W_PIECES == 6), "pieces");
  static_assert(BIAS_OFF + 3 * RN * 4 <= LDS, "staging tile + bias / gamma / beta must fit in the ring");
  static_assert(32 * WM * LPR == 2 * THREADS, "two epilogue passes per 32-row round");
};

#define ROWS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// byte offset of 16-byte k-chunk kc (0..3) of row r inside a [R][32] operand image
__device__ __forceinline__ int img_off(int r, int kc) { return tile_off(r >> 1, ((r & 1) << 2) | kc); }

template <int DT, bool LN, int WM, int RN>
__global__ __launch_bounds__((RowsCfg<WM, RN>::THREADS)) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_rows_kernel(
    const unsigned short* __restrict__ A, const unsigned short* __restrict__ W, const float* __restrict__ bias,
    float* __restrict__ X, int64_t rows, int k, const float* __restrict__ ln_g, const float* __restrict__ ln_b, float ln_eps,
    unsigned short* __restrict__ H) {
  using C = RowsCfg<WM, RN>;
  constexpr int RBM = C::BM, RTHREADS = C::THREADS, RA_BYTES = C::A_BYTES, RSTAGE = C::STAGE, RSTAGES = C::STAGES;
  constexpr int RBIAS_OFF = C::BIAS_OFF, RCS = C::RCS, NW = C::NW, A_PIECES = C::A_PIECES, W_PIECES = C::W_PIECES, LPR = C::LPR;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int wm = WM == 2 ? wave / NW : 0, wn = wave % NW;
  const int64_t m0 = (int64_t)blockIdx.x * RBM;

  // ---- LDS-DMA pieces per thread and stage: 2 / 1 of the activation image (voff[0..1]), 3 / 6 of the weight image
  //      (voff[2..4]; pieces 3..5 are pieces 0..2 shifted by 3 THREADS / 4 weight rows: same lane offset, the shift in the
  //      scalar offset)
  int voff[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int q = (i < 2 ? i : i - 2) * RTHREADS + tid;
    int dr, c;
    tile_pos(q, dr, c);
    voff[i] = (2 * dr + (c >> 2)) * k * 2 + (c & 3) * 16;
  }
  // the last tile may be partial: its missing activation rows read as zeros (descriptor bounds), their outputs are
  // computed and dropped -- every row takes the same arithmetic wherever it sits in the launch
  const int rows_here = (int)(rows - m0 < RBM ? rows - m0 : RBM);
  const i32x4_t rsrc_a = lds_dma_rsrc(A + m0 * k, (unsigned)(rows_here * k * 2));
  const i32x4_t rsrc_w = lds_dma_rsrc(W, (unsigned)(RN * k * 2));
  const unsigned ring_lds = (unsigned)(size_t)LDS_PTR(smem);
  const unsigned dma_wave = ring_lds + wave * 1024;
  constexpr int PIECE = RTHREADS * 16;             // LDS bytes one piece of all threads covers (8 / 4 KB)
  const int w_half = (3 * RTHREADS / 4) * k * 2;
#define ROWS_STAGE(T, BUF)                                                                      \
  {                                                                                             \
    const unsigned dst_ = dma_wave + (BUF) * RSTAGE;                                            \
    const int so_ = (T) * (RBK * 2);                                                            \
    lds_dma16(rsrc_a, dst_, voff[0], so_);                                                      \
    if (A_PIECES == 2) lds_dma16(rsrc_a, dst_ + PIECE, voff[1], so_);                           \
    lds_dma16(rsrc_w, dst_ + RA_BYTES, voff[2], so_);                                           \
    lds_dma16(rsrc_w, dst_ + RA_BYTES + PIECE, voff[3], so_);                                   \
    lds_dma16(rsrc_w, dst_ + RA_BYTES + 2 * PIECE, voff[4], so_);                               \
    if (W_PIECES == 6) {                                                                        \
      lds_dma16(rsrc_w, dst_ + RA_BYTES + 3 * PIECE, voff[2], so_ + w_half);                    \
      lds_dma16(rsrc_w, dst_ + RA_BYTES + 4 * PIECE, voff[3], so_ + w_half);                    \
      lds_dma16(rsrc_w, dst_ + RA_BYTES + 5 * PIECE, voff[4], so_ + w_half);                    \
    }                                                                                           \
  }

  // ---- fragment addresses: block b (32 rows further) = + 2048 B and the swizzle bit flips when b is odd ----
  int aoff[2], woff[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    aoff[s2] = img_off(128 * wm + l31, 2 * s2 + h);
    woff[s2] = RA_BYTES + img_off(96 * wn + l31, 2 * s2 + h);
  }

  f32x16_t acc[3][4];   // [column block nb][row block mb]
#pragma unroll
  for (int nb = 0; nb < 3; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][mb][r] = 0.f;

  const int nk = k / RBK;
  ROWS_STAGE(0, 0)
  if (RSTAGES == 3 && nk > 1) ROWS_STAGE(1, 1)
  for (int t = 0; t < nk; ++t) {
    // this wave's pieces of stage t have landed (3-deep ring: the 5 youngest may belong to stage t + 1)
    if (RSTAGES == 3 && t + 1 < nk) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ROWS_BARRIER();   // everybody's pieces have; and everybody is done with stage t - 1, whose buffer is refilled now
    if (t + RSTAGES - 1 < nk) ROWS_STAGE(t + RSTAGES - 1, (t + RSTAGES - 1) % RSTAGES)
    const char* buf = smem + (t % RSTAGES) * RSTAGE;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      s16x8_t af[4], wf[3];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        af[mb] = *reinterpret_cast<const s16x8_t*>(buf + (aoff[s2] ^ ((mb & 1) << 7)) + mb * 2048);
#pragma unroll
      for (int nb = 0; nb < 3; ++nb)
        wf[nb] = *reinterpret_cast<const s16x8_t*>(buf + (woff[s2] ^ ((nb & 1) << 7)) + nb * 2048);
#pragma unroll
      for (int nb = 0; nb < 3; ++nb)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[nb][mb] = mfma32<DT>(wf[nb], af[mb], acc[nb][mb]);
    }
  }
#undef ROWS_STAGE

  // ---- epilogue: four rounds of 64 rows (row block mb of both row halves) through a padded fp32 LDS tile ----
  ROWS_BARRIER();                                  // the last stage has been read by everybody: the ring is free
  float* const sbias = reinterpret_cast<float*>(smem + RBIAS_OFF);
  for (int i = tid; i < (LN ? 3 : 1) * RN; i += RTHREADS)
    sbias[i] = i < RN ? bias[i] : (i < 2 * RN ? ln_g[i - RN] : ln_b[i - 2 * RN]);
  // read-modify-write in two passes per round (32 / 16 rows each): 16 lanes per row, 16-byte chunks seg + 16 j.
  // The x loads of the NEXT pass are issued before the stores of this one: the memory counter retires in issue order,
  // so a load waited for behind earlier stores would also wait for those stores.
  int tid_e = tid;
  asm volatile("" : "+v"(tid_e));   // opaque: keeps the epilogue's lane-derived addresses out of the main loop's registers
  const int row_p = tid_e / LPR, seg = tid_e % LPR;
  float4 xn[6];
#define ROWS_LOADX(MB, P)                                                                       \
  {                                                                                             \
    const int sr_ = (P) * (RTHREADS / LPR) + row_p;                                              \
    const int rl_ = (sr_ >> 5) * 128 + 32 * (MB) + (sr_ & 31);                                  \
    const float* xr_ = X + (m0 + (rl_ < rows_here ? rl_ : rows_here - 1)) * RN + seg * 4;       \
    _Pragma("unroll") for (int j = 0; j < 6; ++j) xn[j] = *reinterpret_cast<const float4*>(xr_ + 4 * LPR * j); \
  }
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    ROWS_BARRIER();                                // bias visible (first round) / previous round's readers are done
    // the lane owns row 128 wm + 32 mb + l31 and columns 96 wn + 32 nb + 8 g + 4 h + {0..3}
#pragma unroll
    for (int nb = 0; nb < 3; ++nb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = 96 * wn + 32 * nb + 8 * g + 4 * h;
        const float4 bv = *reinterpret_cast<const float4*>(sbias + n);
        float4 v;
        v.x = acc[nb][mb][4 * g + 0] + bv.x; v.y = acc[nb][mb][4 * g + 1] + bv.y;
        v.z = acc[nb][mb][4 * g + 2] + bv.z; v.w = acc[nb][mb][4 * g + 3] + bv.w;
        *reinterpret_cast<float4*>(smem + (32 * wm + l31) * RCS + n * 4) = v;
      }
    if (mb == 0) {   // (not earlier: all 192 accumulator registers are live until the first round has been staged)
      __builtin_amdgcn_sched_barrier(0);
      ROWS_LOADX(0, 0)
    }
    ROWS_BARRIER();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int srow = p * (RTHREADS / LPR) + row_p;                 // row of the staging tile
      const int rl = (srow >> 5) * 128 + 32 * mb + (srow & 31);     // row of the workgroup's tile
      const int64_t gm = m0 + rl;
      const bool live = rl < rows_here;
      const char* sr = smem + srow * RCS + seg * 16;
      float4 x[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) x[j] = xn[j];
      if (p == 0) ROWS_LOADX(mb, 1)
      else if (mb < 3) ROWS_LOADX(mb + 1, 0)
      __builtin_amdgcn_sched_barrier(0);
      float* xw = X + gm * RN + seg * 4;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float4 d = *reinterpret_cast<const float4*>(sr + 16 * LPR * j);
        x[j].x += d.x; x[j].y += d.y; x[j].z += d.z; x[j].w += d.w;
        if (live) *reinterpret_cast<float4*>(xw + 4 * LPR * j) = x[j];
        s += (x[j].x + x[j].y) + (x[j].z + x[j].w);
      }
      __builtin_amdgcn_sched_barrier(0);   // (keeps the LayerNorm's LDS reads from being hoisted into the loop above: spills)
      if constexpr (LN) {
        // the row's 384 new values sit in these 16 lanes (24 each): statistics by 4 shuffles, arithmetic of layernorm.hip
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        if (LPR == 32) s += __shfl_xor(s, 16);
        const float mean = s / (float)RN;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          x[j].x -= mean; x[j].y -= mean; x[j].z -= mean; x[j].w -= mean;
          q += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
        }
        q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4); q += __shfl_xor(q, 8);
        if (LPR == 32) q += __shfl_xor(q, 16);
        const float rstd = 1.0f / sqrtf(q / (float)RN + ln_eps);
        unsigned short* hr = H + gm * RN + seg * 4;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float4 gg = *reinterpret_cast<const float4*>(sbias + RN + seg * 4 + 4 * LPR * j);
          const float4 bb = *reinterpret_cast<const float4*>(sbias + 2 * RN + seg * 4 + 4 * LPR * j);
          uint2 pk;
          pk.x = pack2_h16<DT>(x[j].x * rstd * gg.x + bb.x, x[j].y * rstd * gg.y + bb.y);
          pk.y = pack2_h16<DT>(x[j].z * rstd * gg.z + bb.z, x[j].w * rstd * gg.w + bb.w);
          if (live) *reinterpret_cast<uint2*>(hr + 4 * LPR * j) = pk;
        }
      }
    }
  }
#undef ROWS_LOADX
}

}  // namespace

// the shapes this kernel covers (whether it is asked first: the dispatch's rows_first, gemm.hip)
bool vittf_gemm_rows_covers(int32_t n, int32_t k, int64_t rows) {
  if ((n != 384 && n != 768) || k % RBK != 0 || k < 2 * RBK || rows <= 0) return false;
  return (int64_t)256 * k * 2 <= 0x7fffffff && rows / 128 + 1 <= 0x7fffffff;      // 32-bit per-lane offsets, grid
}

int vittf_gemm_rows(const void* a, const void* w, const float* bias, float* x, int64_t rows, int32_t n, int32_t k,
                    int32_t dtype, const float* ln_g, const float* ln_b, float ln_eps, void* h, hipStream_t st) {
  if (!vittf_gemm_rows_covers(n, k, rows)) return VITTF_ERR_INVALID_ARG;
  if (dtype != VITTF_BF16 && dtype != VITTF_FP16) return VITTF_ERR_INVALID_ARG;
  // Workgroup shape by K (never by the row count: results must not depend on how the rows are batched): the 256-row
  // shape for the long-K linear (fc2: 239 against 254 ms per 3072 slices), the 128-row one for proj (123 against 127).
  const int wm = n == 768 ? 1 : (k >= 1024 ? 2 : 1);
  const unsigned short* A = (const unsigned short*)a;
  const unsigned short* Wp = (const unsigned short*)w;
  const bool ln = ln_g && ln_b && h;
  const int bm = 128 * wm;
  const dim3 grid((unsigned)((rows + bm - 1) / bm)), block(n == 768 ? 512 : 256 * wm);
#define ROWS_LAUNCH(DT, LN, WM, RNV)                                                                                     \
  hipLaunchKernelGGL((gemm_rows_kernel<DT, LN, WM, RNV>), grid, block, 0, st, A, Wp, bias, x, rows, k, ln_g, ln_b, ln_eps, \
                     (unsigned short*)h)
#define ROWS_LAUNCH_WM(DT, LN) \
  { if (n == 768) ROWS_LAUNCH(DT, LN, 1, 768); else if (wm == 2) ROWS_LAUNCH(DT, LN, 2, 384); else ROWS_LAUNCH(DT, LN, 1, 384); }
  if (dtype == VITTF_BF16) {
    if (ln) ROWS_LAUNCH_WM(VITTF_BF16, true) else ROWS_LAUNCH_WM(VITTF_BF16, false)
  } else {
    if (ln) ROWS_LAUNCH_WM(VITTF_FP16, true) else ROWS_LAUNCH_WM(VITTF_FP16, false)
  }
#undef ROWS_LAUNCH_WM
#undef ROWS_LAUNCH
  return vittf_check_launch();
}
