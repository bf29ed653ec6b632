// Hand-crafted per-voxel features of a scalar volume at its own resolution: the 11-channel vector of the reference's
// classical baseline (predict_svm_rf.py:25-65) for the SVM and forest passes (vit-tf_amd/voxel_features.py,
// classify_features.py --features handcrafted | intensity).
//
// V is fp32 (n0, n1, n2), C-contiguous, I = V / vmax, v = (i0 n1 + i1) n2 + i2.  Raw channels:
//   0      I
//   1      sqrt(gx^2 + gy^2 + gz^2), g = 0.5 (I[+1] - I[-1]) per axis, a neighbour outside the volume counting as 0 (ZERO padding)
//   2..7   I at (i0+1), (i1+1), (i2+1), (i0-1), (i1-1), (i2-1); outside the volume the border voxel itself (REPLICATE padding)
//   8..10  i0 / n0 - 0.5, i1 / n1 - 0.5, i2 / n2 - 0.5
// and every channel standardised over the whole volume, (x - mean_c) / std_c with the unbiased std, rounded once to fp16.
//
// vittf_voxel_feature_stats: means and stds in fp64.  Every channel but the coordinates is vmax^-1 times a function of V alone
// (the gradient magnitude too), so the sums run over V itself -- sum and sum of squares of the centre, of the zero-padded
// gradient magnitude (fp64 differences, squares and square root) and of the six replicated neighbours -- and vmax divides the
// results once.  stats_kernel: workgroup u owns the VS_UNIT consecutive voxels from u VS_UNIT, thread t the voxels t, t + 256,
// ... of them in ascending order; the 256 threads' sums meet in a fixed tree (xor-shuffles over the wave, then the four waves
// in order) and land in ws[u][16].  stats_finish_kernel (one workgroup) adds the units in a fixed order as well: thread t the
// units t, t + 256, ..., then the same tree.  No atomics: the same call gives the same bytes.  The coordinate channels have
// closed forms: mean -1 / (2 n), population variance (n^2 - 1) / (12 n^2).
//
// vittf_voxel_features: compose_kernel.  A workgroup owns VC_TILE consecutive OUTPUT positions i (voxel voxel_index[i] or
// v0 + i); thread t computes the positions t, t + 256, ... (the seven loads of a wave are then seven runs of 256 contiguous
// bytes in dense mode) in fp32 from coefficients the host folded in fp64 (I = V * (1 / vmax), x * (1 / std) - mean / std as
// one fma), and parks the fp16 results in an LDS tile [channel][position].  Behind a barrier the tile leaves row by row in
// 16-byte pieces, a wave-instruction covering 1024 contiguous bytes of one channel row.  The tiles start at -phase, phase the
// distance of out from a 16-byte boundary in elements, so with out_stride a multiple of 8 every full piece of every row is
// aligned; a piece that is not aligned (another stride) or not full (the ragged ends) goes out in 2-byte stores.  A voxel's
// values are computed by one function of the voxel index alone: its bits depend on neither the mode nor v0, n or out_stride.
#include "vittf_common.h"

namespace {

constexpr int VF_C = VITTF_VOXFEAT_CHANNELS;
constexpr int VF_MIN_DIM = 2, VF_MAX_DIM = 2048;

constexpr int VS_THREADS = 256;
constexpr int VS_UNIT = 16384;               // voxels per workgroup of the statistics: 64 per thread
constexpr int VS_SUMS = 16;                  // sum and sum of squares of the channels 0..7

constexpr int VC_THREADS = 256;
constexpr int VC_PER_THREAD = 4;
constexpr int VC_TILE = VC_THREADS * VC_PER_THREAD;      // output positions per workgroup

static bool vf_shape_ok(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < VF_MIN_DIM || n1 < VF_MIN_DIM || n2 < VF_MIN_DIM || n0 > VF_MAX_DIM || n1 > VF_MAX_DIM || n2 > VF_MAX_DIM) return false;
  return (int64_t)n0 * n1 * n2 < ((int64_t)1 << 31);
}
static bool vf_vmax_ok(float vmax) { return vmax > 0.f && vmax <= 3.402823466e38f; }      // (NaN fails both)
static int64_t vs_units(int64_t nvox) { return (nvox + VS_UNIT - 1) / VS_UNIT; }

struct Shape { int n0, n1, n2; };

// the centre and its six neighbours as the volume holds them; `in` tells which neighbours exist (bit k: the order of the
// channels 2..7); a missing one is returned as the centre (replicate padding) -- by loading the centre's address again, so
// that all seven loads are unconditional and in flight together
__device__ __forceinline__ unsigned load7(const float* __restrict__ vol, Shape s, unsigned v, float& c, float (&nb)[6], unsigned (&idx)[3]) {
  const unsigned i2 = v % (unsigned)s.n2, r = v / (unsigned)s.n2;
  const unsigned i1 = r % (unsigned)s.n1, i0 = r / (unsigned)s.n1;
  idx[0] = i0; idx[1] = i1; idx[2] = i2;
  const unsigned st0 = (unsigned)s.n1 * (unsigned)s.n2, st1 = (unsigned)s.n2;
  unsigned in = 0u;
  in |= (i0 + 1 < (unsigned)s.n0) ? 1u : 0u;
  in |= (i1 + 1 < (unsigned)s.n1) ? 2u : 0u;
  in |= (i2 + 1 < (unsigned)s.n2) ? 4u : 0u;
  in |= (i0 > 0) ? 8u : 0u;
  in |= (i1 > 0) ? 16u : 0u;
  in |= (i2 > 0) ? 32u : 0u;
  c = vol[v];
  nb[0] = vol[(in & 1u) ? v + st0 : v];
  nb[1] = vol[(in & 2u) ? v + st1 : v];
  nb[2] = vol[(in & 4u) ? v + 1 : v];
  nb[3] = vol[(in & 8u) ? v - st0 : v];
  nb[4] = vol[(in & 16u) ? v - st1 : v];
  nb[5] = vol[(in & 32u) ? v - 1 : v];
  return in;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// the 256 threads' acc[VS_SUMS] added in a fixed tree; thread k < VS_SUMS returns the k-th total (the others garbage)
__device__ __forceinline__ double block_sums(double (&acc)[VS_SUMS], double (*lds)[VS_SUMS]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < VS_SUMS; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < VS_SUMS; ++k) lds[wave][k] = acc[k];
  }
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < VS_SUMS) t = ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
  return t;
}

__global__ __launch_bounds__(VS_THREADS) void stats_kernel(const float* __restrict__ vol, Shape s, unsigned nvox, double* __restrict__ part) {
  __shared__ double lds[VS_THREADS / 64][VS_SUMS];
  double acc[VS_SUMS];
#pragma unroll
  for (int k = 0; k < VS_SUMS; ++k) acc[k] = 0.0;
  const int64_t base = (int64_t)blockIdx.x * VS_UNIT;
  for (int j = 0; j < VS_UNIT / VS_THREADS; ++j) {
    const int64_t v = base + threadIdx.x + (int64_t)VS_THREADS * j;
    if (v >= (int64_t)nvox) break;
    float c, nb[6];
    unsigned idx[3];
    const unsigned in = load7(vol, s, (unsigned)v, c, nb, idx);
    const double dc = (double)c;
    acc[0] += dc;
    acc[1] += dc * dc;
    double g2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double up = (in >> a) & 1u ? (double)nb[a] : 0.0, dn = (in >> (a + 3)) & 1u ? (double)nb[a + 3] : 0.0;
      const double g = 0.5 * (up - dn);
      g2 += g * g;
    }
    acc[2] += sqrt(g2);
    acc[3] += g2;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double d = (double)nb[k];
      acc[4 + 2 * k] += d;
      acc[5 + 2 * k] += d * d;
    }
  }
  const double t = block_sums(acc, lds);
  if (threadIdx.x < VS_SUMS) part[(int64_t)blockIdx.x * VS_SUMS + threadIdx.x] = t;
}

__global__ __launch_bounds__(VS_THREADS) void stats_finish_kernel(const double* __restrict__ part, int64_t units, Shape s, double nvox,
                                                                   double vmax, double* __restrict__ stats) {
  __shared__ double lds[VS_THREADS / 64][VS_SUMS];
  double acc[VS_SUMS];
#pragma unroll
  for (int k = 0; k < VS_SUMS; ++k) acc[k] = 0.0;
  for (int64_t u = threadIdx.x; u < units; u += VS_THREADS) {
#pragma unroll
    for (int k = 0; k < VS_SUMS; ++k) acc[k] += part[u * VS_SUMS + k];
  }
  const double t = block_sums(acc, lds);
  __syncthreads();
  if (threadIdx.x < VS_SUMS) lds[0][threadIdx.x] = t;
  __syncthreads();
  const int c = threadIdx.x;
  if (c < 8) {
    const double sum = lds[0][2 * c], sq = lds[0][2 * c + 1];
    const double mean = sum / nvox;
    const double var = (sq - sum * mean) / (nvox - 1.0);
    stats[c] = mean / vmax;
    stats[VF_C + c] = sqrt(var > 0.0 ? var : 0.0) / vmax;
  } else if (c < VF_C) {
    const double n = (double)(c == 8 ? s.n0 : c == 9 ? s.n1 : s.n2);
    stats[c] = -0.5 / n;
    stats[VF_C + c] = sqrt((n * n - 1.0) / (12.0 * n * n) * (nvox / (nvox - 1.0)));
  }
}

// what the host folds once per call: I = V * rmax; channel c leaves as fma(x, scale[c], shift[c])
struct Coef { float rmax, rn[3], scale[VF_C], shift[VF_C]; };

// what voxel v brings from memory: the centre, the six neighbours, which of them exist, its coordinates
struct Taps { float c, nb[6]; unsigned in, idx[3]; bool ok; };

template <int CH>
__device__ __forceinline__ void load_taps(const float* __restrict__ vol, Shape s, unsigned v, Taps& t) {
  if constexpr (CH == 1) t.c = vol[v];
  else t.in = load7(vol, s, v, t.c, t.nb, t.idx);
}

// the standardised channels of a voxel from its taps, the one function both addressing modes call
template <int CH>
__device__ __forceinline__ void voxel_channels(const Taps& t, const Coef& k, unsigned short (&out)[CH]) {
  if constexpr (CH == 1) {
    out[0] = f32_to_f16bits(__builtin_fmaf(t.c * k.rmax, k.scale[0], k.shift[0]));
  } else {
    float x[VF_C];
    x[0] = t.c * k.rmax;
#pragma unroll
    for (int j = 0; j < 6; ++j) x[2 + j] = t.nb[j] * k.rmax;
    float g2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float up = (t.in >> a) & 1u ? x[2 + a] : 0.f, dn = (t.in >> (a + 3)) & 1u ? x[5 + a] : 0.f;
      const float g = 0.5f * (up - dn);
      g2 = __builtin_fmaf(g, g, g2);
    }
    x[1] = __builtin_sqrtf(g2);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[8 + a] = __builtin_fmaf((float)t.idx[a], k.rn[a], -0.5f);
#pragma unroll
    for (int j = 0; j < VF_C; ++j) out[j] = f32_to_f16bits(__builtin_fmaf(x[j], k.scale[j], k.shift[j]));
  }
}

template <int CH>
__global__ __launch_bounds__(VC_THREADS) void compose_kernel(const float* __restrict__ vol, Shape s, unsigned nvox, Coef k,
                                                             const int64_t* __restrict__ voxel_index, int64_t v0, int64_t n,
                                                             unsigned short* __restrict__ out, int64_t out_stride, int phase) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[CH][VC_TILE];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * VC_TILE - phase;          // the tile's first output position (may be < 0)
  // every load of the thread's positions is issued before the first value is used: 7 VC_PER_THREAD loads in flight a lane
  Taps taps[VC_PER_THREAD];
  int64_t vox[VC_PER_THREAD];
#pragma unroll
  for (int j = 0; j < VC_PER_THREAD; ++j) {
    const int64_t i = i0 + tid + VC_THREADS * j;
    const int64_t ic = i < 0 ? 0 : i < n ? i : n - 1;                // (a position outside the call loads position 0 or n - 1
    vox[j] = voxel_index ? voxel_index[ic] : v0 + ic;                // and a voxel outside the volume voxel 0: no branches)
    taps[j].ok = i == ic;
  }
#pragma unroll
  for (int j = 0; j < VC_PER_THREAD; ++j) {
    taps[j].ok = taps[j].ok && vox[j] >= 0 && vox[j] < (int64_t)nvox;
    load_taps<CH>(vol, s, taps[j].ok ? (unsigned)vox[j] : 0u, taps[j]);
  }
#pragma unroll
  for (int j = 0; j < VC_PER_THREAD; ++j) {
    const int p = tid + VC_THREADS * j;
    unsigned short h[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) h[c] = 0x7e00u;                     // NaN: what an index outside the volume would leave
    if (taps[j].ok) voxel_channels<CH>(taps[j], k, h);
#pragma unroll
    for (int c = 0; c < CH; ++c) tile[c][p] = h[c];
  }
  __syncthreads();
  constexpr int PIECES = VC_TILE / 8;
  for (int q = tid; q < CH * PIECES; q += VC_THREADS) {
    const int c = q / PIECES, p = 8 * (q % PIECES);
    const int64_t i = i0 + p;
    if (i + 8 <= 0 || i >= n) continue;
    unsigned short* dst = out + (int64_t)c * out_stride + i;
    if (i >= 0 && i + 8 <= n && ((uintptr_t)dst & 15) == 0) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&tile[c][p]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (i + e >= 0 && i + e < n) dst[e] = tile[c][p + e];
    }
  }
}

}  // namespace

size_t vittf_voxel_feature_stats_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!vf_shape_ok(n0, n1, n2)) return 0;
  return (size_t)vs_units((int64_t)n0 * n1 * n2) * VS_SUMS * sizeof(double);
}

int vittf_voxel_feature_stats(const float* vol, int32_t n0, int32_t n1, int32_t n2, float vmax, double* stats, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!vol || !stats || !ws || !vf_shape_ok(n0, n1, n2) || !vf_vmax_ok(vmax)) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)vol & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)ws & 7)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_voxel_feature_stats_workspace_bytes(n0, n1, n2)) return VITTF_ERR_WORKSPACE;
  const int64_t nvox = (int64_t)n0 * n1 * n2, units = vs_units(nvox);
  const Shape s = {n0, n1, n2};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stats_kernel, dim3((unsigned)units), dim3(VS_THREADS), 0, st, vol, s, (unsigned)nvox, (double*)ws);
  hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(VS_THREADS), 0, st, (const double*)ws, units, s, (double)nvox, (double)vmax, stats);
  return vittf_check_launch();
}

int vittf_voxel_features(const float* vol, int32_t n0, int32_t n1, int32_t n2, float vmax, const double* stats, int32_t channels,
                         const int64_t* voxel_index, int64_t v0, int64_t n, uint16_t* out, int64_t out_stride, void* stream) {
  if (!vol || !stats || !out || !vf_shape_ok(n0, n1, n2) || !vf_vmax_ok(vmax)) return VITTF_ERR_INVALID_ARG;
  if (channels != VF_C && channels != 1) return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)vol & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)voxel_index & 7) || ((uintptr_t)out & 1)) return VITTF_ERR_INVALID_ARG;
  const int64_t nvox = (int64_t)n0 * n1 * n2;
  if (n < 1 || n >= ((int64_t)1 << 31) || out_stride < n) return VITTF_ERR_INVALID_ARG;
  if (!voxel_index && (v0 < 0 || v0 >= nvox || n > nvox - v0)) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  double host[2 * VF_C];
  if (hipMemcpyAsync(host, stats, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipGetLastError();
    return VITTF_ERR_LAUNCH;
  }
  Coef k;
  k.rmax = (float)(1.0 / (double)vmax);
  k.rn[0] = (float)(1.0 / n0); k.rn[1] = (float)(1.0 / n1); k.rn[2] = (float)(1.0 / n2);
  for (int c = 0; c < VF_C; ++c) {
    const double mean = host[c], sd = host[VF_C + c];
    if (c < channels && !(sd > 0.0 && sd <= 1.7976931348623157e308 && mean >= -1.7976931348623157e308 && mean <= 1.7976931348623157e308))
      return VITTF_ERR_INVALID_ARG;
    k.scale[c] = c < channels ? (float)(1.0 / sd) : 0.f;
    k.shift[c] = c < channels ? (float)(-mean / sd) : 0.f;
    if (!(k.scale[c] <= 3.402823466e38f && k.shift[c] >= -3.402823466e38f && k.shift[c] <= 3.402823466e38f)) return VITTF_ERR_INVALID_ARG;
  }
  const int phase = (int)(((uintptr_t)out >> 1) & 7);
  const int64_t wgs = (n + phase + VC_TILE - 1) / VC_TILE;
  const Shape s = {n0, n1, n2};
#define VC_LAUNCH(CH) \
  hipLaunchKernelGGL((compose_kernel<CH>), dim3((unsigned)wgs), dim3(VC_THREADS), 0, st, vol, s, (unsigned)nvox, k, voxel_index, v0, n, \
                     (unsigned short*)out, out_stride, phase)
  if (channels == VF_C) VC_LAUNCH(VF_C); else VC_LAUNCH(1);
#undef VC_LAUNCH
  return vittf_check_launch();
}
