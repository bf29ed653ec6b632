// The reduction along the voxels of an F-major fp16 feature volume [f][nvox] that gram_kernel (pca.hip: X X^T) and
// sums_kernel (kmeans.hip: X onehot(labels)^T) share.  The volume is cut into spans of whole runs of VITTF_GRAM_RUN voxels
// (span_plan); a workgroup of 8 waves walks one span (Span) in steps of 32 voxels.  All f rows of a step are staged in LDS
// through registers, one step ahead of the MFMAs, with two barriers per step (RowStager); a lane's 8 consecutive voxels of
// a staged row ARE an operand fragment of v_mfma_f32_32x32x16_f16 (span_frag_off): no transpose.  An fp32 accumulator tile
// covers at most one run, then flush_tile adds it into the workgroup's private fp64 partial in the workspace (the first run
// writes, later runs read-add-write).  A second kernel adds the partials in span order (sum_over_spans, acc_elem): no
// floating-point atomics anywhere, the same call gives the same bits.  Each kernel keeps its own step loop.
#pragma once
#include "feat_rows.h"

namespace {

constexpr int SPAN_THREADS = 512, SPAN_WAVES = 8;
constexpr int SPAN_STEP = 32;                           // voxels per staged step: two MFMA k-steps
constexpr int SPAN_ROW = 2 * SPAN_STEP + 16;            // LDS bytes per staged row (16 bytes of padding: odd number of 16-byte slots)
constexpr int SPAN_NARROW = 384;                        // f up to here: 3 staged chunks per thread, a 30 KB slab; wider: 8, 80 KB
constexpr int SPAN_PRE_NARROW = SPAN_NARROW * (SPAN_STEP / 8) / SPAN_THREADS;   // 16-byte chunks a thread stages per step, at most
constexpr int SPAN_PRE_WIDE = FEAT_MAXF * (SPAN_STEP / 8) / SPAN_THREADS;
constexpr int SPAN_RUN_STEPS = VITTF_GRAM_RUN / SPAN_STEP;
static_assert(VITTF_GRAM_RUN % SPAN_STEP == 0 && VITTF_GRAM_RUN <= 4096, "an fp32 accumulator covers whole steps");
static_assert(SPAN_THREADS % (SPAN_STEP / 8) == 0, "a thread's chunk column is the same for all its rows");

// LDS bytes of the staged step of a kernel whose threads stage PRE chunks: PRE * 128 rows
constexpr int span_slab_bytes(int pre) { return pre * SPAN_THREADS / (SPAN_STEP / 8) * SPAN_ROW; }

// at most max_units spans of whole runs; beyond max_units runs a span holds several
struct SpanPlan { int units; int64_t runs_per_unit; };

static SpanPlan span_plan(int64_t nvox, int max_units) {
  const int64_t runs = (nvox + VITTF_GRAM_RUN - 1) / VITTF_GRAM_RUN;
  const int64_t runs_per_unit = (runs + max_units - 1) / max_units;
  return {(int)((runs + runs_per_unit - 1) / runs_per_unit), runs_per_unit};
}

// span `unit`: nsteps steps from voxel vbeg on (the last one may reach past nvox)
struct Span {
  int64_t vbeg, nsteps;
  __device__ __forceinline__ Span(int unit, int64_t runs_per_unit, int64_t nvox) {
    vbeg = (int64_t)unit * runs_per_unit * VITTF_GRAM_RUN;
    const int64_t vend = vbeg + runs_per_unit * VITTF_GRAM_RUN < nvox ? vbeg + runs_per_unit * VITTF_GRAM_RUN : nvox;
    nsteps = (vend - vbeg + SPAN_STEP - 1) / SPAN_STEP;
  }
  // the accumulators are flushed behind this step: a run of VITTF_GRAM_RUN voxels ends, or the span
  __device__ __forceinline__ bool run_ends(int64_t step) const { return (step + 1) % SPAN_RUN_STEPS == 0 || step + 1 == nsteps; }
};

// Staging of a step's [f][32] voxels: thread tid holds 16-byte chunk (i & 3) of row (i >> 2), i = tid + SPAN_THREADS k, for
// k < PRE, in registers from prefetch(step) until commit(slab) writes it to the row's place in LDS.
template <bool ALIGNED, int PRE>
struct RowStager {
  const unsigned short* __restrict__ feat;
  int64_t nvox, vbeg;
  int nchunks, tid;
  uint4 pre[PRE];
  __device__ __forceinline__ RowStager(const unsigned short* __restrict__ feat_, int f, int64_t nvox_, int64_t vbeg_)
      : feat(feat_), nvox(nvox_), vbeg(vbeg_), nchunks(f * (SPAN_STEP / 8)), tid(threadIdx.x) {}
  __device__ __forceinline__ bool mine(int k) const { return tid + SPAN_THREADS * k < nchunks; }   // chunk k exists (f < 128 PRE)
  __device__ __forceinline__ int row(int k) const { return (tid + SPAN_THREADS * k) >> 2; }
  __device__ __forceinline__ int chunk() const { return tid & (SPAN_STEP / 8 - 1); }              // the same for every k
  __device__ __forceinline__ void prefetch(int64_t step) {
    const int64_t v = vbeg + step * SPAN_STEP + 8 * chunk();
#pragma unroll
    for (int k = 0; k < PRE; ++k)
      if (mine(k)) pre[k] = feat_load8<ALIGNED>(feat + (int64_t)row(k) * nvox, v, nvox);
  }
  __device__ __forceinline__ void commit(char* slab) const {
#pragma unroll
    for (int k = 0; k < PRE; ++k)
      if (mine(k)) *reinterpret_cast<uint4*>(slab + row(k) * SPAN_ROW + 16 * chunk()) = pre[k];
  }
};

// byte offset of the lane's fragment inside a 32-row block of the slab: row lane % 32, k-step 0 (k-step 1 at + 32)
__device__ __forceinline__ int span_frag_off(int lane) { return (lane & 31) * SPAN_ROW + (lane >> 5) * 16; }

// acc -> the wave's 1024-double tile of the workgroup's partial, then cleared
__device__ __forceinline__ void flush_tile(double* tile, f32x16_t& acc, bool first) {
  unsigned loff = 16 * (threadIdx.x & 63);            // 128 bytes per lane
  asm volatile("" : "+v"(loff));                      // (keeps the store addresses of all the tiles from being formed, and spilled, ahead of the step loop)
  double* dst = tile + loff;
  if (first) {
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[r] = (double)acc[r];
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[r] += (double)acc[r];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  __builtin_amdgcn_sched_barrier(0);                  // one tile's 16 fp64 values in registers at a time
}

// the sum over the spans, in span order, of entry `index` of their partials (`stride` entries per span)
template <typename T>
__device__ __forceinline__ T sum_over_spans(const T* __restrict__ part, int units, int64_t stride, int64_t index) {
  T s = 0;
  for (int u = 0; u < units; ++u) s += part[(int64_t)u * stride + index];
  return s;
}

// entry e = 16 lane + register of a tile in accumulator order -> (row, column) of the 32 x 32 tile
__device__ __forceinline__ void acc_elem(int e, int& row, int& col) { row = acc_row(e & 15, e >> 9), col = (e >> 4) & 31; }

}  // namespace
