// Random-forest decision of every voxel of an F-major fp16 feature volume [f][nvox] (vit-tf_amd/forest.py fits or imports the
// model on the host and packs it; classify_features.py --classifier forest is the command line).
//
// The packed forest (forest.py's pack()):
//   nodes        uint2 per node, the trees one behind the other, tree t at nodes[tree_offset[t] .. tree_offset[t + 1])
//                  inner node: .x = feature | threshold fp16 bits << 16, .y = left | right << 16 (tree-local indices, both
//                              larger than the node's own: the walk only moves forward)
//                  leaf:       .x = 0xFFFF, .y = the row of the leaf in leaf_values
//   leaf_values  8 x uint16 per leaf (16 bytes, one load): floor(p_c 65535 + 0.5) of the leaf's class shares, zeros behind
//                the last class
// A voxel goes left at an inner node when feat[feature][voxel] <= threshold, compared as fp16 NUMBERS (-0 == +0, +-inf
// thresholds allowed).  Its vote for class c is the uint32 sum of leaf_values[leaf_t][c] over the trees (4096 x 65535 < 2^32);
// its label the class with the largest vote, the lowest index among equal votes.  Integers only: the same bytes every run.
//
// forest_kernel<VT>: a workgroup of 1024 threads owns VT consecutive voxels.  It stages their [f][VT] tile in LDS with
// coalesced row loads (feat_rows.h's feat_load8), then splits as (voxel, tree group): thread tid walks trees g, g + G, ...
// (g = tid / VT, G = 1024 / VT) for voxel tid % VT.  A wave is 64 voxels of ONE tree, so the lanes read the same nodes near
// the root and drift apart below; VT / 64 waves walk the same tree at the same time.  The walk is a chain of dependent
// loads (node from global memory / L2, then the feature from the tile), yet in the measurements neither
// more trees in flight nor more waves per SIMD made it faster; more voxels on the same tree at the same time did -- the
// node gathers of a CU then touch fewer different cache lines.  So the tile is as wide as LDS allows: one 128 KiB tile per CU,
// VT = 1024, 512, 256, 128 or 64 voxels for f <= 64, 128, 256, 512, 1024 -- 16 waves per CU, 4 per SIMD.  With VT = 1024
// there is one tree group and nothing to add up.
// The walk takes at most max_depth steps per tree whatever the nodes say; a walk that the bound stops on an inner node (it
// cannot with a model forest.py's validate() let through) casts no vote for that tree.  The G groups then add their votes
// into one LDS row per class (in the tile's memory, behind a barrier), group after group, and group 0 takes the arg-max;
// labels and votes leave in vector stores.
#include "vittf_common.h"
#include "feat_rows.h"

namespace {

constexpr int FR_THREADS = 1024;
constexpr int FR_CHAINS = 4;                 // trees a thread walks at once
constexpr int FR_TILE_ELEMS = 64 * 1024;     // fp16 values of a tile: 128 KiB, one workgroup per CU
constexpr int FR_MIN_VT = FR_TILE_ELEMS / FEAT_MAXF;
static_assert(FR_MIN_VT >= 64, "a wave is 64 voxels of one tree");
constexpr unsigned FR_LEAF = 0xFFFFu;
static_assert(VITTF_FOREST_MAX_CLASSES == 8, "a leaf row is 8 x uint16: one 16-byte load");

static bool forest_classes_ok(int32_t c) { return c >= 2 && c <= VITTF_FOREST_MAX_CLASSES; }
static bool forest_trees_ok(int32_t t) { return t >= 1 && t <= VITTF_FOREST_MAX_TREES; }
static bool forest_depth_ok(int32_t d) { return d >= 0 && d <= VITTF_FOREST_MAX_DEPTH; }

// voxels per workgroup: the widest tile of f rows that fits
static int forest_tile_voxels(int32_t f) {
  int vt = FR_THREADS;
  while (vt > FR_MIN_VT && f * vt > FR_TILE_ELEMS) vt >>= 1;
  return vt;
}

template <bool ALIGNED, int VT>
__global__ __launch_bounds__(FR_THREADS) void forest_kernel(const unsigned short* __restrict__ feat, int f, int64_t nvox,
                                                            const uint2* __restrict__ nodes, const uint4* __restrict__ leaf_values,
                                                            const unsigned* __restrict__ tree_offset, int trees, int classes,
                                                            int max_depth, unsigned char* __restrict__ labels,
                                                            unsigned* __restrict__ votes) {
  constexpr int G = FR_THREADS / VT;
  static_assert(FR_TILE_ELEMS * 2 >= VITTF_FOREST_MAX_CLASSES * VT * 4, "the vote rows fit the tile's memory");
  __shared__ __attribute__((aligned(16))) char lds[2 * FR_TILE_ELEMS];
  unsigned short* tile = reinterpret_cast<unsigned short*>(lds);       // [feature][voxel]
  unsigned (*sum)[VT] = reinterpret_cast<unsigned (*)[VT]>(lds);       // [class][voxel], once the walks are over
  const int tid = threadIdx.x;
  const int vl = tid % VT, g = tid / VT;
  const int64_t v0 = (int64_t)blockIdx.x * VT;
  const int64_t v = v0 + vl;

  // the tile: f rows of VT voxels, 8 voxels (16 bytes) a piece
  for (int i = tid; i < f * (VT / 8); i += FR_THREADS) {
    const int row = i / (VT / 8), piece = i % (VT / 8);
    *reinterpret_cast<uint4*>(tile + row * VT + 8 * piece) = feat_load8<ALIGNED>(feat + (int64_t)row * nvox, v0 + 8 * piece, nvox);
  }
  __syncthreads();

  unsigned mine[VITTF_FOREST_MAX_CLASSES];
#pragma unroll
  for (int c = 0; c < VITTF_FOREST_MAX_CLASSES; ++c) mine[c] = 0u;
  if (v < nvox) {
    for (int t0 = g; t0 < trees; t0 += G * FR_CHAINS) {
      const uint2* base[FR_CHAINS];
      uint2 n[FR_CHAINS];
#pragma unroll
      for (int u = 0; u < FR_CHAINS; ++u) {
        const int t = t0 + G * u;
        base[u] = nodes + tree_offset[t < trees ? t : t0];
        n[u] = base[u][0];
        if (t >= trees) n[u] = make_uint2(FR_LEAF, 0xFFFFFFFFu);       // no such tree: a leaf that is not counted
      }
      for (int d = 0; d < max_depth; ++d) {
        bool any = false;
#pragma unroll
        for (int u = 0; u < FR_CHAINS; ++u) {
          const unsigned feature = n[u].x & 0xFFFFu;
          if (feature != FR_LEAF) {
            const float x = f16bits_to_f32(tile[feature * VT + vl]);
            const float thr = f16bits_to_f32((unsigned short)(n[u].x >> 16));
            n[u] = base[u][x <= thr ? (n[u].y & 0xFFFFu) : (n[u].y >> 16)];
            any = true;
          }
        }
        if (!any) break;
      }
#pragma unroll
      for (int u = 0; u < FR_CHAINS; ++u) {
        if ((n[u].x & 0xFFFFu) == FR_LEAF && n[u].y != 0xFFFFFFFFu) {
          const uint4 p = leaf_values[n[u].y];
          mine[0] += p.x & 0xFFFFu; mine[1] += p.x >> 16;
          mine[2] += p.y & 0xFFFFu; mine[3] += p.y >> 16;
          mine[4] += p.z & 0xFFFFu; mine[5] += p.z >> 16;
          mine[6] += p.w & 0xFFFFu; mine[7] += p.w >> 16;
        }
      }
    }
  }

  // the groups' votes, group after group, where the tile was
  __syncthreads();
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < VITTF_FOREST_MAX_CLASSES; ++c) sum[c][vl] = mine[c];
  }
  __syncthreads();
  for (int r = 1; r < G; ++r) {
    if (g == r) {
#pragma unroll
      for (int c = 0; c < VITTF_FOREST_MAX_CLASSES; ++c) sum[c][vl] += mine[c];
    }
    __syncthreads();
  }
  if (g == 0 && v < nvox) {
    unsigned best = sum[0][vl];
    int bi = 0;
    for (int c = 1; c < classes; ++c) {
      const unsigned s = sum[c][vl];
      if (s > best) { best = s; bi = c; }               // strict: the lowest index wins a tie
    }
    labels[v] = (unsigned char)bi;
  }
  if (votes) {
    for (int i = tid; i < classes * VT; i += FR_THREADS) {
      const int c = i / VT, j = i % VT;
      if (v0 + j < nvox) votes[(int64_t)c * nvox + v0 + j] = sum[c][j];
    }
  }
}

}  // namespace

int vittf_forest_decide(const uint16_t* feat, int32_t f, int64_t nvox, const uint32_t* nodes, const uint16_t* leaf_values,
                        const uint32_t* tree_offset, int32_t trees, int32_t classes, int32_t max_depth, uint8_t* labels,
                        uint32_t* votes, void* stream) {
  if (!feat || !nodes || !leaf_values || !tree_offset || !labels) return VITTF_ERR_INVALID_ARG;
  if (!feat_f_ok(f) || nvox < 1 || !forest_trees_ok(trees) || !forest_classes_ok(classes) || !forest_depth_ok(max_depth))
    return VITTF_ERR_INVALID_ARG;
  if (((uintptr_t)feat & 1) || ((uintptr_t)nodes & 7) || ((uintptr_t)leaf_values & 15) || ((uintptr_t)tree_offset & 3) ||
      ((uintptr_t)votes & 3))
    return VITTF_ERR_INVALID_ARG;
  const int vt = forest_tile_voxels(f);
  const int64_t wgs = (nvox + vt - 1) / vt;
  if (wgs > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const bool al = rows_aligned(feat, nvox);
#define FR_LAUNCH(AL, VT) \
  hipLaunchKernelGGL((forest_kernel<AL, VT>), dim3((unsigned)wgs), dim3(FR_THREADS), 0, st, feat, f, nvox, (const uint2*)nodes, \
                     (const uint4*)leaf_values, tree_offset, trees, classes, max_depth, labels, votes)
#define FR_PICK(VT) do { if (al) FR_LAUNCH(true, VT); else FR_LAUNCH(false, VT); } while (0)
  if (vt == 1024) FR_PICK(1024);
  else if (vt == 512) FR_PICK(512);
  else if (vt == 256) FR_PICK(256);
  else if (vt == 128) FR_PICK(128);
  else FR_PICK(64);
#undef FR_PICK
#undef FR_LAUNCH
  return vittf_check_launch();
}
