// Connected-component labelling of uint8 label / mask volumes: "voxels of a class" -> "objects".
//
// Replaces cc_torch.connected_components_labeling of the reference's tests/test_connected_components.py (threshold a
// similarity map, keep its largest island) and the scipy.ndimage.label of bilateral_solver.py:199-200.
// A voxel's label is 1 + the smallest linear index of its component (0: background): a definition that does not depend on
// the order in which anything runs, so the same input gives the same bytes.
//
// Three launches (phase boundaries are kernel boundaries; no grid-wide barrier, no persistent kernel):
//   tile     one workgroup per 4 x 8 x 64 tile (CC_T0 x CC_T1 x CC_T2, components_uf.h): the runs along a row from a wave ballot,
//            union-find in LDS over the in-tile links between rows (LDS atomicMin, one union per pair of runs), a local
//            flatten, ONE plain store per voxel: parent[v] = global index of the tile-local root, -1 for background.
//            Nearly all links of a volume are met here and cost no global atomic.
//   seam     the 725 low-face voxels of every tile against their neighbours in other tiles: union-find on the global
//            parent array, again one union per pair of runs.  The per-XCD L2s are not coherent for plain loads inside a
//            kernel, so every load of a find is a relaxed agent-scope atomic load and every link an agent-scope atomicMin
//            whose RETURN value decides the step.
//   flatten  labels[v] = 1 + root(parent[v]) into `labels`; the parent array is only read (other threads follow its chains).
// The union / find loops, their termination and race argument: components_uf.h.
// HBM bytes per voxel: tile 1 + 4, seam ~0.35 x (1 + a few neighbour bytes and parents, mostly cache hits), flatten 4 + 4:
// about 14, plus the chain reads of the flatten (tile root -> component root, shared by a whole tile).
//
// vittf_component_sizes: equal labels are added up in the thread (runs of its 16 voxels), then in a 256-slot LDS table of the
// workgroup, which walks many chunks; one global add per distinct label and workgroup (a label that finds no slot adds
// directly).  A volume that is one component costs <= 2048 same-address atomics, not one per voxel.
#include "vittf_internal.h"
#include "components_uf.h"

namespace {

struct LdsMem {
  int* p;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int fetch_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

struct GlobalMem {
  int* p;
  __device__ __forceinline__ int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int fetch_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// the flatten pass runs after the seam kernel has ended: plain loads, nothing is written to the array
struct ReadMem {
  const int* p;
  __device__ __forceinline__ int load(int i) { return p[i]; }
};

struct TileGrid { int t1, t2; };      // tiles along n1 and n2; blockIdx.x = (b0 * t1 + b1) * t2 + b2

__device__ __forceinline__ void tile_of_block(const TileGrid g, int& b0, int& b1, int& b2) {
  const int bid = blockIdx.x;
  b2 = bid % g.t2;
  b1 = (bid / g.t2) % g.t1;
  b0 = bid / (g.t2 * g.t1);
}

__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* __restrict__ src, int n0, int n1, int n2, int select,
                                                      int connectivity, TileGrid g, int* __restrict__ parent) {
  __shared__ int par[CC_TILE];
  __shared__ unsigned char key[CC_TILE];
  const int tid = threadIdx.x;
  int b0, b1, b2;
  tile_of_block(g, b0, b1, b2);
  const int t2 = tid & (CC_T2 - 1), i2 = b2 * CC_T2 + t2;
#pragma unroll
  for (int r = 0; r < CC_TILE / 256; ++r) {
    const int l = r * 256 + tid;                       // t2 = l % 64: a wave is one row of the tile
    const int i1 = b1 * CC_T1 + ((l / CC_T2) % CC_T1), i0 = b0 * CC_T0 + l / (CC_T2 * CC_T1);
    const bool in = i0 < n0 && i1 < n1 && i2 < n2;
    const int k = in ? cc_key(src[((int64_t)i0 * n1 + i1) * n2 + i2], select) : CC_BG;
    key[l] = (unsigned char)k;
    // rows without atomics: the first voxel of the lane's run of equal keys (cc_row_start) from a ballot of the run starts
    const int before = __shfl_up(k, 1);
    const unsigned long long starts = __ballot(t2 == 0 || k == CC_BG || before != k);      // bit 0 is always set
    par[l] = l - t2 + (63 - __builtin_clzll(starts & (~0ull >> (63 - t2))));
  }
  __syncthreads();
  LdsMem m{par};
#pragma unroll 1
  for (int k = 0; k < CC_TILE / 256; ++k) cc_tile_links(m, key, k * 256 + tid, connectivity);
  __syncthreads();
  // local flatten: reads only (nobody writes par any more), then one plain store per voxel of the volume
#pragma unroll 1
  for (int k = 0; k < CC_TILE / 256; ++k) {
    const int l = k * 256 + tid;
    const int i1 = b1 * CC_T1 + ((l / CC_T2) % CC_T1), i0 = b0 * CC_T0 + l / (CC_T2 * CC_T1);
    if (i0 >= n0 || i1 >= n1 || i2 >= n2) continue;
    const int64_t v = ((int64_t)i0 * n1 + i1) * n2 + i2;
    parent[v] = key[l] == CC_BG ? -1 : cc_global_index(cc_find(m, l), b0, b1, b2, n1, n2);
  }
}

__global__ __launch_bounds__(256) void cc_seam_kernel(const unsigned char* __restrict__ src, int n0, int n1, int n2, int select,
                                                      int connectivity, TileGrid g, int* parent) {
  int b0, b1, b2;
  tile_of_block(g, b0, b1, b2);
  GlobalMem m{parent};
  for (int s = threadIdx.x; s < CC_SEAM; s += 256) cc_seam_links(m, src, n0, n1, n2, select, connectivity, b0, b1, b2, s);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int nvox, int* __restrict__ labels) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvox) return;
  ReadMem m{parent};
  labels[v] = cc_label(m, parent[v]);
}

// ---- sizes ----
constexpr int SZ_SLOTS = 256, SZ_PROBES = 8, SZ_PER_THREAD = 16, SZ_CHUNK = 256 * SZ_PER_THREAD;

__device__ __forceinline__ void sizes_add(int* tkey, int* tcnt, int* sizes, int nvox, int lab, int cnt) {
  if (lab < 1 || lab > nvox) return;                   // background (and anything that is not a label of this volume)
  unsigned slot = ((unsigned)lab * 2654435761u) >> 24;
  for (int probe = 0; probe < SZ_PROBES; ++probe, slot = (slot + 1) & (SZ_SLOTS - 1)) {
    const int seen = atomicCAS(&tkey[slot], 0, lab);
    if (seen == 0 || seen == lab) { atomicAdd(&tcnt[slot], cnt); return; }
  }
  atomicAdd(&sizes[lab - 1], cnt);                     // no free slot near: add directly
}

__global__ __launch_bounds__(256) void cc_sizes_kernel(const int* __restrict__ labels, int nvox, int* sizes) {
  __shared__ int tkey[SZ_SLOTS], tcnt[SZ_SLOTS];
  const int tid = threadIdx.x;
  tkey[tid] = 0; tcnt[tid] = 0;                        // SZ_SLOTS == 256 threads
  __syncthreads();
  const int64_t chunks = ((int64_t)nvox + SZ_CHUNK - 1) / SZ_CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t first = c * SZ_CHUNK + (int64_t)tid * SZ_PER_THREAD;
    int run = 0, cnt = 0;
    for (int j = 0; j < SZ_PER_THREAD; ++j) {
      if (first + j >= nvox) break;
      const int lab = labels[first + j];
      if (lab == run) { ++cnt; continue; }
      if (cnt) sizes_add(tkey, tcnt, sizes, nvox, run, cnt);
      run = lab; cnt = 1;
    }
    if (cnt) sizes_add(tkey, tcnt, sizes, nvox, run, cnt);
  }
  __syncthreads();
  if (tkey[tid] != 0 && tcnt[tid] != 0) atomicAdd(&sizes[tkey[tid] - 1], tcnt[tid]);
}

// ---- filter ----
__device__ __forceinline__ bool cc_kept(int lab, const int* __restrict__ sizes, int nvox, int min_size, int keep_label) {
  if (lab < 1 || lab > nvox) return false;
  return keep_label > 0 ? lab == keep_label : sizes[lab - 1] >= min_size;
}

// VEC: 4 voxels per thread (16-byte label loads, 4-byte src loads and dst stores); else one voxel per thread
template <bool VEC>
__global__ __launch_bounds__(256) void cc_filter_kernel(const unsigned char* src, const int* __restrict__ labels,
                                                        const int* __restrict__ sizes, int nvox, int min_size, int keep_label,
                                                        unsigned fill, unsigned char* dst) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const int64_t v = 4 * e;
    if (v + 3 < nvox) {
      const int4 l4 = *reinterpret_cast<const int4*>(labels + v);
      const unsigned s = *reinterpret_cast<const unsigned*>(src + v);
      const int l[4] = {l4.x, l4.y, l4.z, l4.w};
      unsigned out = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out |= (cc_kept(l[j], sizes, nvox, min_size, keep_label) ? (s >> (8 * j)) & 255u : fill) << (8 * j);
      *reinterpret_cast<unsigned*>(dst + v) = out;
    } else {
      for (int64_t w = v; w < nvox; ++w) {
        const unsigned char x = src[w];
        dst[w] = cc_kept(labels[w], sizes, nvox, min_size, keep_label) ? x : (unsigned char)fill;
      }
    }
  } else if (e < nvox) {
    const unsigned char x = src[e];
    dst[e] = cc_kept(labels[e], sizes, nvox, min_size, keep_label) ? x : (unsigned char)fill;
  }
}

constexpr int64_t CC_MAX_VOX = 0x7fffffffLL - 1;       // a label is 1 + a linear index and must fit an int32

int64_t checked_voxels(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
  const int64_t plane = (int64_t)n1 * n2;
  if (plane > CC_MAX_VOX || n0 > CC_MAX_VOX / plane) return 0;
  return plane * n0;
}

}  // namespace

extern "C" size_t vittf_components_workspace_bytes(int32_t n0, int32_t n1, int32_t n2) {
  const int64_t nvox = checked_voxels(n0, n1, n2);
  return nvox ? align256((size_t)nvox * 4) : 0;
}

extern "C" int vittf_label_components(const uint8_t* src, int32_t n0, int32_t n1, int32_t n2, int32_t select,
                                      int32_t connectivity, int32_t* labels, void* ws, size_t ws_bytes, void* stream) {
  const int64_t nvox = checked_voxels(n0, n1, n2);
  if (!src || !labels || !ws || nvox == 0 || select < -2 || select > 255 || connectivity < 1 || connectivity > 3)
    return VITTF_ERR_INVALID_ARG;
  if ((((uintptr_t)labels) | ((uintptr_t)ws)) & 3) return VITTF_ERR_INVALID_ARG;
  if (ws_bytes < vittf_components_workspace_bytes(n0, n1, n2)) return VITTF_ERR_WORKSPACE;
  TileGrid g{(n1 + CC_T1 - 1) / CC_T1, (n2 + CC_T2 - 1) / CC_T2};
  const int64_t tiles = (int64_t)((n0 + CC_T0 - 1) / CC_T0) * g.t1 * g.t2;       // <= nvox < 2^31
  hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)ws;
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, st, src, n0, n1, n2, select, connectivity, g, parent);
  if (tiles > 1)
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)tiles), dim3(256), 0, st, src, n0, n1, n2, select, connectivity, g, parent);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, parent, (int)nvox, labels);
  return vittf_check_launch();
}

extern "C" int vittf_component_sizes(const int32_t* labels, int64_t nvox, int32_t* sizes, void* stream) {
  if (!labels || !sizes || nvox < 1 || nvox > CC_MAX_VOX || ((((uintptr_t)labels) | ((uintptr_t)sizes)) & 3))
    return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sizes, 0, (size_t)nvox * 4, st) != hipSuccess) return VITTF_ERR_LAUNCH;
  int64_t blocks = (nvox + SZ_CHUNK - 1) / SZ_CHUNK;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, labels, (int)nvox, sizes);
  return vittf_check_launch();
}

extern "C" int vittf_filter_components(const uint8_t* src, const int32_t* labels, const int32_t* sizes, int64_t nvox,
                                       int32_t min_size, int32_t keep_label, int32_t fill, uint8_t* dst, void* stream) {
  if (!src || !labels || !dst || nvox < 1 || nvox > CC_MAX_VOX || keep_label < 0 || fill < 0 || fill > 255)
    return VITTF_ERR_INVALID_ARG;
  if (keep_label == 0 && !sizes) return VITTF_ERR_INVALID_ARG;
  if ((((uintptr_t)labels) | ((uintptr_t)sizes)) & 3) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 3) == 0 && (((uintptr_t)labels) & 15) == 0;
  if (vec) {
    const int64_t threads = (nvox + 3) / 4;
    hipLaunchKernelGGL(cc_filter_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, labels, sizes,
                       (int)nvox, min_size, keep_label, (unsigned)fill, dst);
  } else {
    hipLaunchKernelGGL(cc_filter_kernel<false>, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0, st, src, labels, sizes,
                       (int)nvox, min_size, keep_label, (unsigned)fill, dst);
  }
  return vittf_check_launch();
}
