// Exact Euclidean distance transform of a uint8 volume: for every voxel the squared distance to the nearest SITE (a voxel that
// meets a predicate), and optionally the linear index of such a site (the feature transform).  The primitive under the
// surface-distance scores (Hausdorff, HD95, ASSD, surface Dice: vit-tf_amd/distance.py) and signed distance fields;
// scipy.ndimage.distance_transform_edt on the host.
//
// The transform is separable: min over sites of sum_a w_a (x_a - s_a)^2 is a min along axis 2, then along 1, then along 0.
//   row   (axis 2, contiguous)  one wave per line.  64 voxels per step with coalesced byte loads; the ballot of the predicate is
//         the step's site mask, lane c keeps the mask of step c.  The last site before and the first site after every step
//         follow from a prefix max / suffix min over the lanes (shuffles); then each voxel finds its nearest site to the left
//         (clz of the mask below it, else the carried one) and to the right (ctz, else the carried one).  A tie goes left.
//   line  (axis 1, then axis 0; strided)  the lower envelope of the parabolas g(i) + w (x - i)^2 (Meijster, Roerdink and
//         Hesselink 2000).  A workgroup takes `width` lines that are adjacent in memory, loads them as n rows of `width`
//         consecutive values (coalesced) into LDS, and lane c walks line c: a forward scan that builds the envelope on two
//         stacks in LDS (s: the parabola's position, t: the first position it wins), a backward scan that evaluates it and
//         stores row after row (the lanes of a wave store consecutive addresses).  The LDS images are [position][lane], so the
//         lanes of one access sit on consecutive banks.  Along axis 0 the "adjacent lines" are the whole (n1, n2) plane.
//         width follows from the LDS budget (edt_tile_width): n (sizeof(value) + 4) bytes a line.
// A position whose value is "no site" (a line of the previous pass without one) is no parabola: the forward scan skips it, so
// the sentinel never enters the arithmetic.  A line without any parabola stores the sentinel.
//
// Integer path: int32 throughout, exact.  Every value is at most 3 x 2047^2 < 2^31, and so is every term of Meijster's
// separator (u^2 - i^2 + g(u) - g(i)) div (2 (u - i)), whose numerator is >= 2 t (u - i) >= 0 after the pops, so the
// truncating division is the floor.  d2_out itself carries the values between the passes (a workgroup reads its lines into LDS
// before it stores them).
// Weighted path: the same walk in fp64 on g = w2 d^2 (fp64 volume in the workspace), the last pass rounds once to fp32.
// Each pass adds two roundings of 2^-53 to a value <= D2 = sum_a w_a (n_a - 1)^2; a comparison or a separator that rounding
// decides the other way exchanges two parabolas whose values at that position differ by no more than those roundings.  The
// separator is forced past the previous one, which exact arithmetic guarantees, so the backward scan cannot lose a parabola.
// With weights (1, 1, 1) every fp64 operation is exact (integers < 2^53; a quotient that is no integer is at least 2^-13 away
// from one) and the result is the integer result converted to fp32.
//
// Feature transform: the row pass stores the site's linear index, a line pass gathers site_in[line position of the winning
// parabola] (the lanes read consecutive addresses); the two buffers alternate, since a line cannot be gathered in place.
// No atomics, every output is stored once by one lane, and ties are decided by the fixed walk: the same input gives the same
// bytes.
#include <math.h>
#include "vittf_internal.h"
#include "components_uf.h"
#include "distance_env.h"

namespace {

constexpr int64_t EDT_MAX_VOX = 0x7fffffffLL;          // fewer than 2^31 voxels: a linear index fits an int32
// LDS of one workgroup of the line pass: half of the CU's 160 KiB, so that one workgroup loads while the other walks
constexpr size_t EDT_LDS_BUDGET = 80 * 1024;
constexpr int EDT_THREADS = 256;

// ---- axis 2 ----
template <typename T, bool SITE>
__global__ __launch_bounds__(EDT_THREADS) void edt_row_kernel(const unsigned char* __restrict__ src, int64_t lines, int n2, int value,
                                                              int mode, T w, T* __restrict__ out, int* __restrict__ site) {
  const int lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * (EDT_THREADS / 64) + (threadIdx.x >> 6);
  if (line >= lines) return;                                            // the whole wave
  const unsigned char* row = src + line * n2;
  const int steps = (n2 + 63) >> 6;                                     // <= 32
  unsigned long long mine = 0;
  for (int c = 0; c < steps; ++c) {
    const int i = c * 64 + lane;
    const bool is = i < n2 && ((cc_key(row[i], value) != CC_BG) != (mode != 0));
    const unsigned long long m = __ballot(is);
    if (lane == c) mine = m;
  }
  // lane c: the last site of the steps before c (-1: none) and the first site of the steps after c (n2: none)
  int last = mine ? lane * 64 + 63 - __builtin_clzll(mine) : -1;
  int first = mine ? lane * 64 + __builtin_ctzll(mine) : n2;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int a = __shfl_up(last, d), b = __shfl_down(first, d);
    if (lane >= d && a > last) last = a;
    if (lane + d < 64 && b < first) first = b;
  }
  int before = __shfl_up(last, 1), after = __shfl_down(first, 1);
  if (lane == 0) before = -1;
  if (lane == 63) after = n2;
  const unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
  for (int c = 0; c < steps; ++c) {
    const unsigned long long m = ((unsigned long long)(unsigned)__shfl((int)hi, c) << 32) | (unsigned)__shfl((int)lo, c);
    const int i = c * 64 + lane;
    const unsigned long long below = m & (~0ull >> (63 - lane)), above = m & (~0ull << lane);
    const int carried_l = __shfl(before, c), carried_r = __shfl(after, c);           // by every lane, before any branch
    const int l = below ? c * 64 + 63 - __builtin_clzll(below) : carried_l;
    const int r = above ? c * 64 + __builtin_ctzll(above) : carried_r;
    if (i >= n2) continue;
    int s = -1;
    if (l >= 0) s = l;
    if (r < n2 && (s < 0 || r - i < i - s)) s = r;
    const int64_t v = line * n2 + i;
    out[v] = s < 0 ? Edt<T>::none() : Edt<T>::sq(w, i - s);
    if (SITE) site[v] = s < 0 ? -1 : (int)(line * n2 + s);
  }
}

// ---- axes 1 and 0 ----
// Line c of tile b of slab y: positions in + y slab + (b width + c) + u stride, u < n.  `lines` lines in a slab.
template <typename T, typename Out, bool SITE>
__global__ __launch_bounds__(EDT_THREADS) void edt_line_kernel(const T* in, Out* out, const int* site_in, int* site_out, int n,
                                                               int64_t stride, int64_t lines, int64_t slab, int width, T w) {
  extern __shared__ __align__(16) unsigned char edt_lds[];
  T* g = reinterpret_cast<T*>(edt_lds);                                 // [n][width]
  unsigned short* s = reinterpret_cast<unsigned short*>(g + (size_t)n * width);      // [n][width] position of parabola q
  unsigned short* t = s + (size_t)n * width;                            // [n][width] first position parabola q wins
  const int64_t first = (int64_t)blockIdx.x * width;
  const int live = lines - first < width ? (int)(lines - first) : width;
  const int64_t base = (int64_t)blockIdx.y * slab + first;
  for (int e = threadIdx.x; e < n * width; e += EDT_THREADS) {
    const int u = e / width, c = e - u * width;
    if (c < live) g[e] = in[base + u * stride + c];
  }
  __syncthreads();
  const int c = threadIdx.x;
  if (c >= live) return;
  const int64_t line = base + c;
  edt_walk_line<T, Out, SITE>(g, s, t, width, c, n, w, out + line, SITE ? site_in + line : nullptr,
                              SITE ? site_out + line : nullptr, stride);
}

int64_t edt_voxels(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > EDT_MAX_DIM || n1 > EDT_MAX_DIM || n2 > EDT_MAX_DIM) return 0;
  const int64_t nvox = (int64_t)n0 * n1 * n2;                           // <= 2^33
  return nvox < EDT_MAX_VOX + 1 ? nvox : 0;
}

template <typename T, typename Out, bool SITE>
int edt_line_pass(const T* in, Out* out, const int* site_in, int* site_out, int n, int64_t stride, int64_t lines, int slabs,
                  int64_t slab, T w, hipStream_t st) {
  const int width = edt_tile_width<T>(n, lines, EDT_LDS_BUDGET, EDT_THREADS);   // n = 2048: 5 (int32), 3 (fp64)
  const size_t lds = (size_t)n * width * (sizeof(T) + 4);
  auto kernel = edt_line_kernel<T, Out, SITE>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)EDT_LDS_BUDGET) !=
      hipSuccess)
    return VITTF_ERR_LAUNCH;
  const dim3 grid((unsigned)((lines + width - 1) / width), (unsigned)slabs);
  hipLaunchKernelGGL(kernel, grid, dim3(EDT_THREADS), lds, st, in, out, site_in, site_out, n, stride, lines, slab, width, w);
  return VITTF_OK;
}

// mid: the values between the passes (d2_out itself on the integer path); site_mid: the second site buffer
template <typename T, typename Out, bool SITE>
int edt_passes(const uint8_t* src, int n0, int n1, int n2, int value, int mode, const T* w, T* mid, Out* d2_out, int* site_mid,
               int* site_out, hipStream_t st) {
  const int64_t plane = (int64_t)n1 * n2, rows = (int64_t)n0 * n1;
  hipLaunchKernelGGL((edt_row_kernel<T, SITE>), dim3((unsigned)((rows + EDT_THREADS / 64 - 1) / (EDT_THREADS / 64))),
                     dim3(EDT_THREADS), 0, st, src, rows, n2, value, mode, w[2], mid, site_out);
  int rc = edt_line_pass<T, T, SITE>(mid, mid, site_out, site_mid, n1, n2, n2, n0, plane, w[1], st);
  if (rc != VITTF_OK) return rc;
  rc = edt_line_pass<T, Out, SITE>(mid, d2_out, site_mid, site_out, n0, plane, plane, 1, 0, w[0], st);
  return rc != VITTF_OK ? rc : vittf_check_launch();
}

bool edt_args_ok(const void* src, const void* d2_out, const void* site_out, const void* ws, int64_t nvox, int32_t value,
                 int32_t mode) {
  if (!src || !d2_out || !ws || nvox == 0 || value < -1 || value > 255 || (mode != 0 && mode != 1)) return false;
  return ((((uintptr_t)d2_out) | ((uintptr_t)site_out)) & 3) == 0 && (((uintptr_t)ws) & 7) == 0;
}

}  // namespace

extern "C" size_t vittf_edt_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  const int64_t nvox = edt_voxels(n0, n1, n2);
  return nvox ? align256((size_t)nvox * 8) + align256((size_t)nvox * 4) : 0;
}

extern "C" int vittf_edt_sq(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t value, int32_t mode, int32_t* d2_out,
                            int32_t* site_out, void* ws, size_t ws_bytes, void* stream) {
  const int64_t nvox = edt_voxels(n0, n1, n2);
  if (!edt_args_ok(src, d2_out, site_out, ws, nvox, value, mode)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_edt_workspace_bytes(n0, n1, n2)) return VITTF_ERR_WORKSPACE;
  const int w[3] = {1, 1, 1};
  int* site_mid = reinterpret_cast<int*>((char*)ws + align256((size_t)nvox * 8));
  hipStream_t st = (hipStream_t)stream;
  return site_out ? edt_passes<int, int, true>(src, n0, n1, n2, value, mode, w, d2_out, d2_out, site_mid, site_out, st)
                  : edt_passes<int, int, false>(src, n0, n1, n2, value, mode, w, d2_out, d2_out, nullptr, nullptr, st);
}

extern "C" int vittf_edt_sq_weighted(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t value, int32_t mode,
                                     const double* w2_host, float* d2_out, int32_t* site_out, void* ws, size_t ws_bytes,
                                     void* stream) {
  const int64_t nvox = edt_voxels(n0, n1, n2);
  if (!edt_args_ok(src, d2_out, site_out, ws, nvox, value, mode) || !w2_host) return VITTF_ERR_INVALID_ARG;
  for (int a = 0; a < 3; ++a)
    if (!(w2_host[a] > 0.0) || !(w2_host[a] < HUGE_VAL)) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_edt_workspace_bytes(n0, n1, n2)) return VITTF_ERR_WORKSPACE;
  double* mid = reinterpret_cast<double*>(ws);
  int* site_mid = reinterpret_cast<int*>((char*)ws + align256((size_t)nvox * 8));
  hipStream_t st = (hipStream_t)stream;
  return site_out ? edt_passes<double, float, true>(src, n0, n1, n2, value, mode, w2_host, mid, d2_out, site_mid, site_out, st)
                  : edt_passes<double, float, false>(src, n0, n1, n2, value, mode, w2_host, mid, d2_out, nullptr, nullptr, st);
}
