// PCA reduction of an F-major fp16 feature volume [f][nvox] (the file layout of infer.py): the Gram matrix + row sums the
// host turns into a basis (vit-tf_amd/pca.py basis_from_gram), and the projection onto that basis.
//
// vittf_feature_gram: gram = X X^T and sums = X 1 in fp64.  Both MFMA operands are rows of the same matrix and the reduction
// runs along the rows, so a lane's 8 consecutive voxels of a row ARE an operand fragment of v_mfma_f32_32x32x16_f16: no
// transpose.  Only the nb (nb + 1) / 2 upper 32 x 32 tiles (nb = f / 32) are computed.  For f <= 384 a workgroup of 8 waves
// owns up to 80 of them (10 accumulator tiles per wave: f = 384 has 78, one workgroup group, the volume is read once); wider
// f stages more rows per thread, keeps 6 tiles per wave and splits the tile list over several groups, each of which reads
// the volume again.  A workgroup walks a span of voxels in steps of 32: all f rows of a step are staged
// in LDS (through registers, one step ahead of the MFMAs), every wave reads its tiles' row blocks from there.
//   * products of two fp16 values are exact in fp32; an fp32 accumulator covers at most VITTF_GRAM_RUN voxels, then it is
//     added into the workgroup's private fp64 partial in the workspace (the first run writes, later runs read-add-write);
//   * a second kernel sums the partials of the voxel spans in fp64 in span order and writes both triangles (a diagonal
//     tile is mirrored from its own upper half, so gram is exactly symmetric); no floating-point atomics anywhere;
//   * rows that are not 16-byte aligned (nvox % 8, or an odd base address) take 2-byte loads; voxels past the end are zeros.
//
// vittf_feature_project: out[k][v] = fp16(sum_f comp[k][f] x[f][v] - offset[k]).  The reduction runs over f, so the volume
// is the operand that needs transposed fragments: a workgroup stages [32 feature rows][256 voxels] parts in LDS and every
// wave picks the 8 features of its 32 voxels up with ds_read_b64_tr_b16 (sim_mfma.hip's pickup).  The components are split
// into fp16 hi + lo halves (comp = hi + lo to 2^-22, sim_mfma_prep's arithmetic) by the workgroup itself, part by part,
// k padded with zero rows to 32 or 64; fp32 accumulation, one rounding to fp16; the volume is read once.  That loop is
// project_scores in feat_rows.h, which the k-means assignment (kmeans.hip) shares.
#include "vittf_common.h"
#include "feat_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------ Gram
constexpr int GR_THREADS = 512, GR_WAVES = 8;
constexpr int GR_STEP = 32;                         // voxels per staged step: two MFMA k-steps
constexpr int GR_ROW = 2 * GR_STEP + 16;            // LDS bytes per staged row (16 bytes of padding: odd number of 16-byte slots)
constexpr int GR_MAXF = FEAT_MAXF;
constexpr int GR_NARROW = 384;                      // f up to here: 10 accumulator tiles per wave, 3 staged chunks per thread
constexpr int GR_SLOTS_NARROW = 10, GR_SLOTS_WIDE = 6;   // accumulator tiles per wave; x GR_WAVES = tiles per workgroup
constexpr int GR_UNITS = 128;                       // most voxel spans (over all tile groups): bounds the workspace
constexpr int GR_PRE_NARROW = GR_NARROW * (GR_STEP / 8) / GR_THREADS;   // 16-byte chunks a thread stages per step, at most
constexpr int GR_PRE_WIDE = GR_MAXF * (GR_STEP / 8) / GR_THREADS;
static_assert(VITTF_GRAM_RUN % GR_STEP == 0 && VITTF_GRAM_RUN <= 4096, "an fp32 accumulator covers whole steps");
static_assert(GR_THREADS % (GR_STEP / 8) == 0, "a thread's chunk column is the same for all its rows");

struct GramPlan { int nb, pairs, groups, units; int64_t runs_per_unit; };

static GramPlan gram_plan(int f, int64_t nvox) {
  GramPlan p;
  p.nb = f / 32;
  p.pairs = p.nb * (p.nb + 1) / 2;
  const int per_group = GR_WAVES * (f <= GR_NARROW ? GR_SLOTS_NARROW : GR_SLOTS_WIDE);
  p.groups = (p.pairs + per_group - 1) / per_group;
  const int max_units = GR_UNITS / p.groups > 0 ? GR_UNITS / p.groups : 1;
  const int64_t runs = (nvox + VITTF_GRAM_RUN - 1) / VITTF_GRAM_RUN;
  p.runs_per_unit = (runs + max_units - 1) / max_units;
  p.units = (int)((runs + p.runs_per_unit - 1) / p.runs_per_unit);
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

// grid: units x groups.  part: fp64 [units][pairs][1024] (a tile in accumulator order: register r of lane l at 16 l + r),
// psums: fp64 [units][f].
// GR_PRE: 16-byte chunks a thread stages per step = rows the slab holds / 128
template <bool ALIGNED, int GR_SLOTS, int GR_PRE>
__global__ __launch_bounds__(GR_THREADS) void gram_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox, int nb,
                                                          int pairs, int units, int64_t runs_per_unit,
                                                          double* __restrict__ part, double* __restrict__ psums) {
  __shared__ __attribute__((aligned(16))) char slab[GR_PRE * GR_THREADS / (GR_STEP / 8) * GR_ROW];   // 30 KB (f <= 384) or 80 KB
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int unit = blockIdx.x % units, group = blockIdx.x / units;
  const int64_t vbeg = (int64_t)unit * runs_per_unit * VITTF_GRAM_RUN;
  const int64_t vend = vbeg + runs_per_unit * VITTF_GRAM_RUN < nvox ? vbeg + runs_per_unit * VITTF_GRAM_RUN : nvox;
  const int64_t nsteps = (vend - vbeg + GR_STEP - 1) / GR_STEP;

  // the wave's tiles: GR_SLOTS consecutive entries of the tile list, so that neighbours share their row block
  const int p0 = (group * GR_WAVES + wave) * GR_SLOTS;
  const int nslots = pairs - p0 < 0 ? 0 : (pairs - p0 < GR_SLOTS ? pairs - p0 : GR_SLOTS);
  int abase[GR_SLOTS], bbase[GR_SLOTS];
#pragma unroll
  for (int t = 0; t < GR_SLOTS; ++t) {
    int bi = 0, bj = 0;
    if (t < nslots) gram_pair(p0 + t, nb, bi, bj);
    abase[t] = __builtin_amdgcn_readfirstlane(bi * 32 * GR_ROW);
    bbase[t] = __builtin_amdgcn_readfirstlane(bj * 32 * GR_ROW);
  }
  f32x16_t acc[GR_SLOTS];
#pragma unroll
  for (int t = 0; t < GR_SLOTS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // staging: 16-byte chunk (i & 3) of row (i >> 2), i = tid + GR_THREADS k
  const int nchunks = f * (GR_STEP / 8);
  const int my_chunk = tid & (GR_STEP / 8 - 1);
  uint4 pre[GR_PRE];
  float rowsum[GR_PRE];
#pragma unroll
  for (int k = 0; k < GR_PRE; ++k) rowsum[k] = 0.f;
  auto prefetch = [&](int64_t step) {
    const int64_t v = vbeg + step * GR_STEP + 8 * my_chunk;
#pragma unroll
    for (int k = 0; k < GR_PRE; ++k) {
      const int i = tid + GR_THREADS * k;
      if (i < nchunks) pre[k] = gram_load8<ALIGNED>(feat + (int64_t)(i >> 2) * nvox, v, nvox);
    }
  };
  const int frag_off = l31 * GR_ROW + h * 16;
  bool first = true;
  prefetch(0);
  for (int64_t step = 0; step < nsteps; ++step) {
    __syncthreads();                                  // the previous step's fragments have been read
#pragma unroll
    for (int k = 0; k < GR_PRE; ++k) {
      const int i = tid + GR_THREADS * k;
      if (i < nchunks) {
        *reinterpret_cast<uint4*>(slab + (i >> 2) * GR_ROW + 16 * my_chunk) = pre[k];
        rowsum[k] += sum8_f16(pre[k]);
      }
    }
    __syncthreads();
    if (step + 1 < nsteps) prefetch(step + 1);
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
    // the end of a run of VITTF_GRAM_RUN voxels (or of the span): fp32 -> the workgroup's fp64 partial
    if ((step + 1) % (VITTF_GRAM_RUN / GR_STEP) == 0 || step + 1 == nsteps) {
#pragma unroll
      for (int t = 0; t < GR_SLOTS; ++t) {
        if (t < nslots) {
          unsigned loff = 16 * lane;                      // 128 bytes per lane
          asm volatile("" : "+v"(loff));                  // (keeps the 160 store addresses from being formed, and spilled, ahead of the loop)
          double* dst = part + ((int64_t)unit * pairs + p0 + t) * 1024 + loff;
          if (first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = (double)acc[t][r];
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] += (double)acc[t][r];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);              // one tile's 16 fp64 values in registers at a time
      }
      if (group == 0) {
#pragma unroll
        for (int k = 0; k < GR_PRE; ++k) {
          float s = rowsum[k];
          s += __shfl_xor(s, 1);
          s += __shfl_xor(s, 2);
          const int i = tid + GR_THREADS * k;
          if (i < nchunks && my_chunk == 0) {
            double* dst = psums + (int64_t)unit * f + (i >> 2);
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
    const int p = (int)(gid >> 10), e = (int)(gid & 1023);
    int bi, bj;
    gram_pair(p, nb, bi, bj);
    const int row = acc_row(e & 15, e >> 9), col = (e >> 4) & 31;      // e = 16 lane + register
    double s = 0.0;
    for (int u = 0; u < units; ++u) s += part[((int64_t)u * pairs + p) * 1024 + e];
    if (bi != bj || row <= col) {
      const int i = 32 * bi + row, j = 32 * bj + col;
      gram[(int64_t)i * f + j] = s;
      gram[(int64_t)j * f + i] = s;
    }
  } else if (gid - tiles < f) {
    const int i = (int)(gid - tiles);
    double s = 0.0;
    for (int u = 0; u < units; ++u) s += psums[(int64_t)u * f + i];
    sums[i] = s;
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
  if (!gram_f_ok(f) || nvox < 1) return 0;
  const GramPlan p = gram_plan(f, nvox);
  return ((size_t)p.units * p.pairs * 1024 + (size_t)p.units * f) * sizeof(double);
}

int vittf_feature_gram(const uint16_t* feat, int32_t f, int64_t nvox, double* gram, double* sums, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!feat || !gram || !sums || !ws || !gram_f_ok(f) || nvox < 1) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)gram & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)ws & 7)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_feature_gram_workspace_bytes(f, nvox)) return VITTF_ERR_WORKSPACE;
  const GramPlan p = gram_plan(f, nvox);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  double* psums = part + (size_t)p.units * p.pairs * 1024;
  const dim3 grid((unsigned)(p.units * p.groups));
  const bool al = rows_aligned(feat, nvox);
#define GR_LAUNCH(AL, SLOTS, PRE) \
  hipLaunchKernelGGL((gram_kernel<AL, SLOTS, PRE>), grid, dim3(GR_THREADS), 0, st, feat, f, nvox, p.nb, p.pairs, p.units, p.runs_per_unit, part, psums)
  if (f <= GR_NARROW) { if (al) GR_LAUNCH(true, GR_SLOTS_NARROW, GR_PRE_NARROW); else GR_LAUNCH(false, GR_SLOTS_NARROW, GR_PRE_NARROW); }
  else { if (al) GR_LAUNCH(true, GR_SLOTS_WIDE, GR_PRE_WIDE); else GR_LAUNCH(false, GR_SLOTS_WIDE, GR_PRE_WIDE); }
#undef GR_LAUNCH
  const int64_t items = (int64_t)p.pairs * 1024 + f;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, part, psums, f, p.nb, p.pairs,
                     p.units, gram, sums);
  return vittf_check_launch();
}

int vittf_feature_project(const uint16_t* feat, int32_t f, int64_t nvox, const float* comp, const float* offset, int32_t k,
                          uint16_t* out, void* stream) {
  if (!feat || !comp || !out || !gram_f_ok(f) || nvox < 1 || k < 1 || k > VITTF_PCA_MAX_K) return VITTF_ERR_INVALID_ARG;
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
