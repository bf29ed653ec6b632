// Lloyd's k-means over an F-major fp16 feature volume [f][nvox] (the file layout of infer.py): the two passes over the
// volume of one iteration (vit-tf_amd/kmeans.py does the rest on the host).
//
// vittf_kmeans_assign: labels[v] = argmax_c (sum_f cent[c][f] x_fv - half_sq[c]) -- the nearest centroid in squared
// Euclidean distance when half_sq[c] = 0.5 |m_c|^2.  The scores are vittf_feature_project's (pca.hip): a workgroup stages
// [32 feature rows][256 voxels] parts in LDS, every wave picks the 8 features of its 32 voxels up with ds_read_b64_tr_b16,
// the centroids are split into fp16 hi + lo halves by the workgroup itself (c padded with zero rows to 32 or 64), fp32
// accumulation, the volume is read once.  Behind the accumulators a lane holds ONE voxel's scores for 16 of every 32
// clusters (rows acc_row(r, h) of each block, ascending in r): it scans them in ascending cluster order with a strict
// compare (rows >= c skipped), then lanes l and l + 32 exchange (score, index) and keep the larger score, the lower index
// among equal ones -- so the lowest index wins among equal fp32 scores, across lane halves and across the two row blocks.
// The 256 one-byte labels of a workgroup are collected in LDS and stored four to a lane.
//
// vittf_kmeans_sums: sums[c][f] = sum over {v: labels[v] == c} of x_fv (fp64) = X onehot(labels)^T, and the cluster sizes,
// by the span reduction of span_rows.h: the A fragment is a staged feature row, the B fragment is 0.0 / 1.0 fp16 built in
// registers from the step's 8 label bytes (label == the lane's cluster column), so every product is exact.  Accumulator
// tiles: (f / 32) x ceil(c / 32), row block b on wave b % 8.  The counts are integers: an LDS histogram per workgroup
// (integer LDS atomics, order-independent), one int64 partial per span, added by the second kernel.
//   * spans: the volume is cut into at most KS_SPANS = 128 spans of whole runs (one workgroup each; a volume of more than
//     128 runs gives a workgroup several runs); workspace = spans x ((f / 32) ceil(c / 32) x 1024 + 64) x 8 bytes,
//     at most 128 x 65600 x 8 = 67 MB (f = 1024, c > 32), 25 MB at f = 384, c > 32;
//   * a label >= c (255 = masked out) matches no column that is kept and is not counted; voxels past the end read as label
//     255 and zero features.
#include "vittf_common.h"
#include "span_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------ assignment
// RB = 32-row blocks of the padded centroids (c <= 32 RB)
template <bool ALIGNED, int RB>
__global__ __launch_bounds__(PJ_THREADS) void assign_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                            const float* __restrict__ cent, const float* __restrict__ half_sq,
                                                            int c, unsigned char* __restrict__ labels, float* __restrict__ best) {
  __shared__ __attribute__((aligned(16))) char vbuf[PJ_ROWS * PJ_VROW];
  __shared__ __attribute__((aligned(16))) char cbuf[2 * 32 * RB * PJ_CROW];  // hi rows, then lo rows
  __shared__ float hs[VITTF_KMEANS_MAX_C];
  __shared__ __attribute__((aligned(4))) unsigned char lab[PJ_VOX];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v0 = (int64_t)blockIdx.x * PJ_VOX;
  if (tid < VITTF_KMEANS_MAX_C) hs[tid] = (half_sq && tid < c) ? half_sq[tid] : 0.f;     // (visible behind the score loop's barriers)
  f32x16_t acc[RB];
  project_scores<ALIGNED, RB>(feat, f, nvox, cent, c, v0, vbuf, cbuf, acc);
  // the lane's 16 RB clusters in ascending order; a strict compare keeps the lowest index of equal scores
  float bs = -__builtin_inff();
  int bi = 0;
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cc = 32 * b + acc_row(r, h);
      const float s = acc[b][r] - hs[cc];
      if (cc < c && s > bs) { bs = s; bi = cc; }
    }
  // the other half of the clusters of this voxel is on lane l ^ 32
  const float os = __shfl_xor(bs, 32);
  const int oi = __shfl_xor(bi, 32);
  if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
  const int64_t v = v0 + wave * 32 + l31;
  if (h == 0) {
    lab[wave * 32 + l31] = (unsigned char)bi;
    if (best && v < nvox) best[v] = bs;
  }
  __syncthreads();
  if (tid < PJ_VOX / 4) {
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

// ------------------------------------------------------------------------------------------------ cluster sums
constexpr int KS_RBW_NARROW = SPAN_NARROW / 32 / SPAN_WAVES + 1, KS_RBW_WIDE = FEAT_MAXF / 32 / SPAN_WAVES;      // row blocks per wave
constexpr int KS_SPANS = 128;                       // most voxel spans: bounds the workspace
static_assert(KS_RBW_NARROW * SPAN_WAVES * 32 >= SPAN_NARROW && KS_RBW_WIDE * SPAN_WAVES * 32 >= FEAT_MAXF, "every row block has a wave");

struct SumsPlan { int nb, cbn, tiles; SpanPlan span; };

static SumsPlan sums_plan(int f, int64_t nvox, int c) {
  SumsPlan p;
  p.nb = f / 32;
  p.cbn = (c + 31) / 32;
  p.tiles = p.nb * p.cbn;
  p.span = span_plan(nvox, KS_SPANS);
  return p;
}

// grid: units.  part: fp64 [units][tiles][1024] (tile = row block x CB + column block, in accumulator order),
// pcounts: int64 [units][64].
// RBW: row blocks per wave, PRE: 16-byte chunks a thread stages per step, CB: 32-cluster column blocks
template <bool ALIGNED, int RBW, int PRE, int CB>
__global__ __launch_bounds__(SPAN_THREADS) void sums_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                            const unsigned char* __restrict__ labels, int c, int nb,
                                                            int64_t runs_per_unit, double* __restrict__ part,
                                                            unsigned long long* __restrict__ pcounts) {
  __shared__ __attribute__((aligned(16))) char slab[span_slab_bytes(PRE)];   // 30 KB (f <= 384) or 80 KB
  __shared__ __attribute__((aligned(8))) unsigned char lab[SPAN_STEP];
  __shared__ unsigned long long hist[VITTF_KMEANS_MAX_C];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int unit = blockIdx.x;
  const Span span(unit, runs_per_unit, nvox);
  // the wave's row blocks: wave, wave + 8, ...
  const int nrb = nb > wave ? (nb - wave + SPAN_WAVES - 1) / SPAN_WAVES : 0;

  f32x16_t acc[RBW][CB];
#pragma unroll
  for (int t = 0; t < RBW; ++t)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][cb][r] = 0.f;
  if (tid < VITTF_KMEANS_MAX_C) hist[tid] = 0ull;     // wave 0, which alone adds to it

  // beside the rows the step's 32 labels are staged, one per thread of wave 0
  RowStager<ALIGNED, PRE> rows(feat, f, nvox, span.vbeg);
  unsigned plab = 255u;
  auto prefetch = [&](int64_t step) {
    rows.prefetch(step);
    if (tid < SPAN_STEP) {
      const int64_t vl = span.vbeg + step * SPAN_STEP + tid;
      plab = vl < nvox ? (unsigned)labels[vl] : 255u;
    }
  };
  const int frag_off = span_frag_off(lane);
  bool first = true;
  prefetch(0);
  for (int64_t step = 0; step < span.nsteps; ++step) {
    __syncthreads();                                  // the previous step's fragments have been read
    rows.commit(slab);
    if (tid < SPAN_STEP) {
      lab[tid] = (unsigned char)plab;
      if (plab < (unsigned)c) atomicAdd(&hist[plab], 1ull);
    }
    __syncthreads();
    if (step + 1 < span.nsteps) prefetch(step + 1);
    // B fragments: element j of k-step s is 1.0 where voxel 16 s + 8 h + j carries the lane's cluster 32 cb + l31
    s16x8_t bf[2][CB];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint2 lb = *reinterpret_cast<const uint2*>(lab + 16 * s + 8 * h);
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned byte = ((j < 4 ? lb.x : lb.y) >> (8 * (j & 3))) & 0xffu;
          bf[s][cb][j] = byte == (unsigned)(32 * cb + l31) ? (short)0x3c00 : (short)0;
        }
    }
#pragma unroll
    for (int t = 0; t < RBW; ++t) {
      if (t < nrb) {                                  // (wave-uniform)
        const char* ab = slab + (wave + SPAN_WAVES * t) * 32 * SPAN_ROW + frag_off;
        const s16x8_t a0 = *reinterpret_cast<const s16x8_t*>(ab);
        const s16x8_t a1 = *reinterpret_cast<const s16x8_t*>(ab + 32);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          acc[t][cb] = mfma32<VITTF_FP16>(a0, bf[0][cb], acc[t][cb]);
          acc[t][cb] = mfma32<VITTF_FP16>(a1, bf[1][cb], acc[t][cb]);
        }
      }
    }
    if (span.run_ends(step)) {
#pragma unroll
      for (int t = 0; t < RBW; ++t)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          if (t < nrb) flush_tile(part + ((int64_t)unit * nb * CB + (wave + SPAN_WAVES * t) * CB + cb) * 1024, acc[t][cb], first);
      first = false;
    }
  }
  if (tid < VITTF_KMEANS_MAX_C) pcounts[(int64_t)unit * VITTF_KMEANS_MAX_C + tid] = hist[tid];     // wave 0's own atomics: in order
}

// sums[c][i] = sum over the spans, in span order, of the tile partials; counts likewise
__global__ __launch_bounds__(256) void sums_reduce_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ pcounts,
                                                          int f, int c, int cbn, int tiles, int units, double* __restrict__ sums,
                                                          int64_t* __restrict__ counts) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t items = (int64_t)tiles * 1024;
  if (gid < items) {
    const int tile = (int)(gid >> 10);
    const int rb = tile / cbn, cb = tile % cbn;
    int row, col;
    acc_elem((int)(gid & 1023), row, col);
    const int cl = 32 * cb + col;
    if (cl < c) sums[(int64_t)cl * f + 32 * rb + row] = sum_over_spans(part, units, items, gid);
  } else if (gid - items < c) {
    counts[gid - items] = (int64_t)sum_over_spans(pcounts, units, VITTF_KMEANS_MAX_C, gid - items);
  }
}

static bool kmeans_c_ok(int32_t c) { return c >= 2 && c <= VITTF_KMEANS_MAX_C; }

}  // namespace

int vittf_kmeans_assign(const uint16_t* feat, int32_t f, int64_t nvox, const float* cent, const float* half_sq, int32_t c,
                        uint8_t* labels, float* best, void* stream) {
  if (!feat || !cent || !labels || !feat_f_ok(f) || nvox < 1 || !kmeans_c_ok(c)) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)cent & 3) || ((uintptr_t)half_sq & 3) || ((uintptr_t)best & 3)) return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + PJ_VOX - 1) / PJ_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool al = rows_aligned(feat, nvox);
#define KA_LAUNCH(AL, RBV) \
  hipLaunchKernelGGL((assign_kernel<AL, RBV>), dim3((unsigned)wgs), dim3(PJ_THREADS), 0, st, feat, f, nvox, cent, half_sq, c, labels, best)
  if (c <= 32) { if (al) KA_LAUNCH(true, 1); else KA_LAUNCH(false, 1); }
  else { if (al) KA_LAUNCH(true, 2); else KA_LAUNCH(false, 2); }
#undef KA_LAUNCH
  return vittf_check_launch();
}

size_t vittf_kmeans_sums_workspace_bytes(int32_t f, int64_t nvox, int32_t c) {
  if (!feat_f_ok(f) || nvox < 1 || !kmeans_c_ok(c)) return 0;
  const SumsPlan p = sums_plan(f, nvox, c);
  return ((size_t)p.span.units * p.tiles * 1024 + (size_t)p.span.units * VITTF_KMEANS_MAX_C) * sizeof(double);
}

int vittf_kmeans_sums(const uint16_t* feat, int32_t f, int64_t nvox, const uint8_t* labels, int32_t c, double* sums,
                      int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!feat || !labels || !sums || !counts || !ws || !feat_f_ok(f) || nvox < 1 || !kmeans_c_ok(c)) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)ws & 7)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_kmeans_sums_workspace_bytes(f, nvox, c)) return VITTF_ERR_WORKSPACE;
  const SumsPlan p = sums_plan(f, nvox, c);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  unsigned long long* pcounts = (unsigned long long*)(part + (size_t)p.span.units * p.tiles * 1024);
  const dim3 grid((unsigned)p.span.units);
  const bool al = rows_aligned(feat, nvox);
#define KS_LAUNCH(AL, RBW, PRE, CB) \
  hipLaunchKernelGGL((sums_kernel<AL, RBW, PRE, CB>), grid, dim3(SPAN_THREADS), 0, st, feat, f, nvox, labels, c, p.nb, p.span.runs_per_unit, part, pcounts)
#define KS_PICK(RBW, PRE) \
  do { if (p.cbn == 1) { if (al) KS_LAUNCH(true, RBW, PRE, 1); else KS_LAUNCH(false, RBW, PRE, 1); } \
       else { if (al) KS_LAUNCH(true, RBW, PRE, 2); else KS_LAUNCH(false, RBW, PRE, 2); } } while (0)
  if (f <= SPAN_NARROW) KS_PICK(KS_RBW_NARROW, SPAN_PRE_NARROW); else KS_PICK(KS_RBW_WIDE, SPAN_PRE_WIDE);
#undef KS_PICK
#undef KS_LAUNCH
  const int64_t items = (int64_t)p.tiles * 1024 + c;
  hipLaunchKernelGGL(sums_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, part, pcounts, f, c, p.cbn, p.tiles,
                     p.span.units, sums, counts);
  return vittf_check_launch();
}
