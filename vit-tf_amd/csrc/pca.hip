// PCA reduction of an F-major fp16 feature volume [f][nvox] (the file layout of infer.py): the Gram matrix + row sums the
// host turns into a basis (vit-tf_amd/pca.py basis_from_gram), and the projection onto that basis.
//
// vittf_feature_gram: gram = X X^T and sums = X 1 in fp64, by the span reduction of span_rows.h with both MFMA operands
// rows of the same staged matrix.  Only the nb (nb + 1) / 2 upper 32 x 32 tiles (nb = f / 32) are computed.  For f <= 384 a
// workgroup of 8 waves owns up to 80 of them (10 accumulator tiles per wave: f = 384 has 78, one workgroup group, the volume
// is read once); wider f stages more rows per thread, keeps 6 tiles per wave and splits the tile list over several groups,
// each of which reads the volume again.
//   * products of two fp16 values are exact in fp32, so an entry carries only the rounding of its fp32 runs;
//   * the row sums are taken from the staged chunks as they are committed (group 0 only), flushed with the tiles;
//   * the second kernel writes both triangles (a diagonal tile is mirrored from its own upper half, so gram is exactly
//     symmetric);
//   * rows that are not 16-byte aligned (nvox % 8, or an odd base address) take 2-byte loads; voxels past the end are zeros.
//
// vittf_feature_project: out[k][v] = fp16(sum_f comp[k][f] x[f][v] - offset[k]).  The reduction runs over f, so the volume
// is the operand that needs transposed fragments: a workgroup stages [32 feature rows][256 voxels] parts in LDS and every
// wave picks the 8 features of its 32 voxels up with ds_read_b64_tr_b16 (sim_mfma.hip's pickup).  The components are split
// into fp16 hi + lo halves (comp = hi + lo to 2^-22, sim_mfma_prep's arithmetic) by the workgroup itself, part by part,
// k padded with zero rows to 32 or 64; fp32 accumulation, one rounding to fp16; the volume is read once.  That loop is
// project_scores in feat_rows.h, which the k-means assignment (kmeans.hip) shares.
#include "vittf_common.h"
#include "span_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------ Gram
constexpr int GR_SLOTS_NARROW = 10, GR_SLOTS_WIDE = 6;   // accumulator tiles per wave (f <= SPAN_NARROW, wider); x SPAN_WAVES = tiles per workgroup
constexpr int GR_UNITS = 128;                       // most voxel spans (over all tile groups): bounds the workspace

struct GramPlan { int nb, pairs, groups; SpanPlan span; };

static GramPlan gram_plan(int f, int64_t nvox) {
  GramPlan p;
  p.nb = f / 32;
  p.pairs = p.nb * (p.nb + 1) / 2;
  const int per_group = SPAN_WAVES * (f <= SPAN_NARROW ? GR_SLOTS_NARROW : GR_SLOTS_WIDE);
  p.groups = (p.pairs + per_group - 1) / per_group;
  p.span = span_plan(nvox, GR_UNITS / p.groups > 0 ? GR_UNITS / p.groups : 1);
  return p;
}

// tile p of the row-major list of upper tiles -> (row block, column block)
__device__ __forceinline__ void gram_pair(int p, int nb, int& bi, int& bj) {
  int rem = p;
  bi = 0;
  while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
  bj = bi + rem;
}

__device__ __forceinline__ float sum8_f16(uint4 c) {
  const unsigned w[4] = {c.x, c.y, c.z, c.w};
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += f16bits_to_f32((unsigned short)(w[j] & 0xffffu)) + f16bits_to_f32((unsigned short)(w[j] >> 16));
  return s;
}

// grid: units x groups.  part: fp64 [units][pairs][1024] (tiles in accumulator order), psums: fp64 [units][f].
// GR_PRE: 16-byte chunks a thread stages per step = rows the slab holds / 128
template <bool ALIGNED, int GR_SLOTS, int GR_PRE>
__global__ __launch_bounds__(SPAN_THREADS) void gram_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox, int nb,
                                                            int pairs, int units, int64_t runs_per_unit,
                                                            double* __restrict__ part, double* __restrict__ psums) {
  __shared__ __attribute__((aligned(16))) char slab[span_slab_bytes(GR_PRE)];   // 30 KB (f <= 384) or 80 KB
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int unit = blockIdx.x % units, group = blockIdx.x / units;
  const Span span(unit, runs_per_unit, nvox);

  // the wave's tiles: GR_SLOTS consecutive entries of the tile list, so that neighbours share their row block
  const int p0 = (group * SPAN_WAVES + wave) * GR_SLOTS;
  const int nslots = pairs - p0 < 0 ? 0 : (pairs - p0 < GR_SLOTS ? pairs - p0 : GR_SLOTS);
  int abase[GR_SLOTS], bbase[GR_SLOTS];
#pragma unroll
  for (int t = 0; t < GR_SLOTS; ++t) {
    int bi = 0, bj = 0;
    if (t < nslots) gram_pair(p0 + t, nb, bi, bj);
    abase[t] = __builtin_amdgcn_readfirstlane(bi * 32 * SPAN_ROW);
    bbase[t] = __builtin_amdgcn_readfirstlane(bj * 32 * SPAN_ROW);
  }
  f32x16_t acc[GR_SLOTS];
#pragma unroll
  for (int t = 0; t < GR_SLOTS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  RowStager<ALIGNED, GR_PRE> rows(feat, f, nvox, span.vbeg);
  float rowsum[GR_PRE];                               // of the thread's chunks, since the last flush
#pragma unroll
  for (int k = 0; k < GR_PRE; ++k) rowsum[k] = 0.f;
  const int frag_off = span_frag_off(lane);
  bool first = true;
  rows.prefetch(0);
  for (int64_t step = 0; step < span.nsteps; ++step) {
    __syncthreads();                                  // the previous step's fragments have been read
    rows.commit(slab);
#pragma unroll
    for (int k = 0; k < GR_PRE; ++k)
      if (rows.mine(k)) rowsum[k] += sum8_f16(rows.pre[k]);
    __syncthreads();
    if (step + 1 < span.nsteps) rows.prefetch(step + 1);
    s16x8_t a0 = {}, a1 = {};
#pragma unroll
    for (int t = 0; t < GR_SLOTS; ++t) {            // (a slot past the wave's last tile computes tile (0, 0) and is never flushed)
      if (t == 0 || abase[t] != abase[t > 0 ? t - 1 : 0]) {
        a0 = *reinterpret_cast<const s16x8_t*>(slab + abase[t] + frag_off);
        a1 = *reinterpret_cast<const s16x8_t*>(slab + abase[t] + frag_off + 32);
      }
      const s16x8_t b0 = *reinterpret_cast<const s16x8_t*>(slab + bbase[t] + frag_off);
      const s16x8_t b1 = *reinterpret_cast<const s16x8_t*>(slab + bbase[t] + frag_off + 32);
      acc[t] = mfma32<VITTF_FP16>(a0, b0, acc[t]);
      acc[t] = mfma32<VITTF_FP16>(a1, b1, acc[t]);
    }
    if (span.run_ends(step)) {
#pragma unroll
      for (int t = 0; t < GR_SLOTS; ++t)
        if (t < nslots) flush_tile(part + ((int64_t)unit * pairs + p0 + t) * 1024, acc[t], first);
      if (group == 0) {
#pragma unroll
        for (int k = 0; k < GR_PRE; ++k) {
          float s = rowsum[k];
          s += __shfl_xor(s, 1);
          s += __shfl_xor(s, 2);
          if (rows.mine(k) && rows.chunk() == 0) {
            double* dst = psums + (int64_t)unit * f + rows.row(k);
            *dst = first ? (double)s : *dst + (double)s;
          }
          rowsum[k] = 0.f;
        }
      }
      first = false;
    }
  }
}

// gram[i][j] = sum over the spans, in span order, of the tile partials; both triangles.  sums likewise.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ part, const double* __restrict__ psums, int f,
                                                          int nb, int pairs, int units, double* __restrict__ gram,
                                                          double* __restrict__ sums) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tiles = (int64_t)pairs * 1024;
  if (gid < tiles) {
    int bi, bj, row, col;
    gram_pair((int)(gid >> 10), nb, bi, bj);
    acc_elem((int)(gid & 1023), row, col);
    const double s = sum_over_spans(part, units, tiles, gid);
    if (bi != bj || row <= col) {
      const int i = 32 * bi + row, j = 32 * bj + col;
      gram[(int64_t)i * f + j] = s;
      gram[(int64_t)j * f + i] = s;
    }
  } else if (gid - tiles < f) {
    sums[gid - tiles] = sum_over_spans(psums, units, f, gid - tiles);
  }
}

// ------------------------------------------------------------------------------------------------ projection
// RB = 32-row blocks of the padded components (k <= 32 RB)
template <bool ALIGNED, int RB>
__global__ __launch_bounds__(PJ_THREADS) void project_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                             const float* __restrict__ comp, const float* __restrict__ offset,
                                                             int k, unsigned short* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char vbuf[PJ_ROWS * PJ_VROW];
  __shared__ __attribute__((aligned(16))) char cbuf[2 * 32 * RB * PJ_CROW];  // hi rows, then lo rows
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int64_t v0 = (int64_t)blockIdx.x * PJ_VOX;
  f32x16_t acc[RB];
  project_scores<ALIGNED, RB>(feat, f, nvox, comp, k, v0, vbuf, cbuf, acc);
  const int64_t v = v0 + wave * 32 + l31;
  if (v < nvox) {
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * b + acc_row(r, h);
        if (kk < k) out[(int64_t)kk * nvox + v] = f32_to_f16bits(acc[b][r] - (offset ? offset[kk] : 0.f));
      }
  }
}

}  // namespace

size_t vittf_feature_gram_workspace_bytes(int32_t f, int64_t nvox) {
  if (!feat_f_ok(f) || nvox < 1) return 0;
  const GramPlan p = gram_plan(f, nvox);
  return ((size_t)p.span.units * p.pairs * 1024 + (size_t)p.span.units * f) * sizeof(double);
}

int vittf_feature_gram(const uint16_t* feat, int32_t f, int64_t nvox, double* gram, double* sums, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!feat || !gram || !sums || !ws || !feat_f_ok(f) || nvox < 1) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)gram & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)ws & 7)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_feature_gram_workspace_bytes(f, nvox)) return VITTF_ERR_WORKSPACE;
  const GramPlan p = gram_plan(f, nvox);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  double* psums = part + (size_t)p.span.units * p.pairs * 1024;
  const dim3 grid((unsigned)(p.span.units * p.groups));
  const bool al = rows_aligned(feat, nvox);
#define GR_LAUNCH(AL, SLOTS, PRE) \
  hipLaunchKernelGGL((gram_kernel<AL, SLOTS, PRE>), grid, dim3(SPAN_THREADS), 0, st, feat, f, nvox, p.nb, p.pairs, p.span.units, p.span.runs_per_unit, part, psums)
  if (f <= SPAN_NARROW) { if (al) GR_LAUNCH(true, GR_SLOTS_NARROW, SPAN_PRE_NARROW); else GR_LAUNCH(false, GR_SLOTS_NARROW, SPAN_PRE_NARROW); }
  else { if (al) GR_LAUNCH(true, GR_SLOTS_WIDE, SPAN_PRE_WIDE); else GR_LAUNCH(false, GR_SLOTS_WIDE, SPAN_PRE_WIDE); }
#undef GR_LAUNCH
  const int64_t items = (int64_t)p.pairs * 1024 + f;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, part, psums, f, p.nb, p.pairs,
                     p.span.units, gram, sums);
  return vittf_check_launch();
}

int vittf_feature_project(const uint16_t* feat, int32_t f, int64_t nvox, const float* comp, const float* offset, int32_t k,
                          uint16_t* out, void* stream) {
  if (!feat || !comp || !out || !feat_f_ok(f) || nvox < 1 || k < 1 || k > VITTF_PCA_MAX_K) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)out & 1) || ((uintptr_t)comp & 3) || ((uintptr_t)offset & 3)) return VITTF_ERR_INVALID_ARG;
  const int64_t wgs = (nvox + PJ_VOX - 1) / PJ_VOX;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool al = rows_aligned(feat, nvox);
#define PJ_LAUNCH(AL, RBV) \
  hipLaunchKernelGGL((project_kernel<AL, RBV>), dim3((unsigned)wgs), dim3(PJ_THREADS), 0, st, feat, f, nvox, comp, offset, k, out)
  if (k <= 32) { if (al) PJ_LAUNCH(true, 1); else PJ_LAUNCH(false, 1); }
  else { if (al) PJ_LAUNCH(true, 2); else PJ_LAUNCH(false, 2); }
#undef PJ_LAUNCH
  return vittf_check_launch();
}
