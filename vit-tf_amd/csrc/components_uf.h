// Union-find core of the connected-component labelling (components.hip), free of any HIP call so that a host program
// (tools/micro/components_host.cpp) drives the same three phases sequentially and checks them against a flood fill.
//
// Memory is reached through a policy `Mem` with   int load(int i)   and   int fetch_min(int i, int v)   (returns the old
// value).  The kernels pass LDS (workgroup-scope atomics) for the tile pass and the global parent array (agent-scope
// atomics) for the seam pass; the host program passes a plain array.
//
// Invariant: parent[x] <= x for every foreground x, at every moment, whatever the interleaving.
//   * It holds at the start (parent[x] = x in the tile pass; parent[x] = its tile root <= x in the seam pass).
//   * The only write is fetch_min(big, small) with small < big: it can only lower parent[big], to a value < big.
// Hence
//   * cc_find ends: every step goes from x to parent[x] < x or stops at parent[x] == x; indices are bounded below by 0.
//   * no cycle can form: a cycle would need some parent[x] > x.
//   * cc_union ends: an iteration either returns or replaces the pair (big, small) by (old, small) -- followed to their
//     roots, which are no larger -- with old < big, so max(a, b) falls strictly and is bounded below by 0.
//   * cc_union is correct under races: the decision is taken from the value the atomic RETURNS.  old == big: big was a root
//     at the instant of the atomic and hangs under small now.  old != big: somebody else had hung big under old; the atomic
//     has left parent[big] = min(old, small), which keeps big connected to one of them, and the loop goes on to join old
//     and small, so nothing is lost.  No step relies on an earlier load still being true.
//   * the root of a finished component is its smallest index: roots only ever hang under smaller indices.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CC_FN __host__ __device__ __forceinline__
#else
#define CC_FN static inline
#endif

// The tile of the tile pass: CC_T0 x CC_T1 x CC_T2 voxels (n2 is the fast axis), one 256-thread workgroup, 8 voxels a thread.
// The local index l = (t0 * CC_T1 + t1) * CC_T2 + t2 orders a tile's voxels as the global linear index does.
constexpr int CC_T0 = 4, CC_T1 = 8, CC_T2 = 64;
constexpr int CC_TILE = CC_T0 * CC_T1 * CC_T2;
// voxels on a low face of their tile: t0 == 0 (T1 x T2), else t1 == 0 ((T0-1) x T2), else t2 == 0 ((T0-1) x (T1-1))
constexpr int CC_SEAM_F0 = CC_T1 * CC_T2, CC_SEAM_F1 = (CC_T0 - 1) * CC_T2, CC_SEAM_F2 = (CC_T0 - 1) * (CC_T1 - 1);
constexpr int CC_SEAM = CC_SEAM_F0 + CC_SEAM_F1 + CC_SEAM_F2;
constexpr int CC_BG = 255;          // key of a background voxel

// key of a voxel: CC_BG for background; two neighbours are linked when their keys are equal and not CC_BG.
// select 0..255: {x == select};  -1: {x != 0};  -2: every x != 255 is foreground and links only to its own value.
CC_FN int cc_key(int x, int select) {
  if (select == -2) return x;
  const bool fg = select >= 0 ? x == select : x != 0;
  return fg ? 0 : CC_BG;
}

template <class Mem> CC_FN int cc_find(Mem& m, int x) {
  for (;;) {
    const int p = m.load(x);          // p <= x
    if (p == x) return x;
    x = p;
  }
}

template <class Mem> CC_FN void cc_union(Mem& m, int a, int b) {
  for (;;) {
    a = cc_find(m, a);
    b = cc_find(m, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a = the larger root, b = the smaller
    const int old = m.fetch_min(a, b);
    if (old == a) return;                              // a was still a root: the link a -> b is made
    a = old;                                           // old < a: go on with (old, b)
  }
}

// ---- tile pass ----
// Rows first, without atomics: parent[l] starts as the first voxel of l's run of equal keys along the row (fast axis); the
// kernel finds it with a wave ballot (a wave is one row), this scan is what the host check uses.  parent[l] <= l holds.
CC_FN int cc_row_start(const unsigned char* key, int l) {
  const int k = key[l];
  if (k == CC_BG) return l;
  int t2 = l % CC_T2;
  while (t2 > 0 && key[l - 1] == k) { --l; --t2; }
  return l;
}

// Then voxel l against its in-tile neighbours in the rows above it (lower half of the neighbourhood without the row itself:
// 2, 8 or 12 offsets).  key: the tile's CC_TILE keys; m: the tile's parent array (local indices).
// Run starts only: when l - 1 and nb - 1 both carry the key too, l - 1 ~ l and nb - 1 ~ nb are row links and the pair
// (l - 1, nb - 1) is the same offset met from l - 1, so the union (l, nb) adds nothing.  In a dense volume that leaves one
// union per pair of runs instead of one per pair of voxels.
template <class Mem> CC_FN void cc_tile_links(Mem& m, const unsigned char* key, int l, int connectivity) {
  const int k = key[l];
  if (k == CC_BG) return;
  const int t2 = l % CC_T2, t1 = (l / CC_T2) % CC_T1, t0 = l / (CC_T2 * CC_T1);
  const bool left = t2 > 0 && key[l - 1] == k;
  for (int d0 = -1; d0 <= 0; ++d0)
    for (int d1 = -1; d1 <= (d0 < 0 ? 1 : -1); ++d1)
      for (int d2 = -1; d2 <= 1; ++d2) {
        if ((d0 != 0) + (d1 != 0) + (d2 != 0) > connectivity) continue;
        const int u0 = t0 + d0, u1 = t1 + d1, u2 = t2 + d2;
        if (u0 < 0 || u1 < 0 || u1 >= CC_T1 || u2 < 0 || u2 >= CC_T2) continue;
        const int nb = (u0 * CC_T1 + u1) * CC_T2 + u2;
        if (key[nb] != k) continue;
        if (left && u2 > 0 && key[nb - 1] == k) continue;
        cc_union(m, l, nb);
      }
}

// local index -> global linear index, for the tile whose first voxel is (b0, b1, b2) * (T0, T1, T2)
CC_FN int cc_global_index(int l, int b0, int b1, int b2, int n1, int n2) {
  const int t2 = l % CC_T2, t1 = (l / CC_T2) % CC_T1, t0 = l / (CC_T2 * CC_T1);
  return (int)(((int64_t)(b0 * CC_T0 + t0) * n1 + (b1 * CC_T1 + t1)) * n2 + (b2 * CC_T2 + t2));
}

// ---- seam pass: seam voxel s (0 .. CC_SEAM-1) of tile (b0, b1, b2) against every neighbour that lies in another tile ----
// Two neighbours in different tiles differ in the tile coordinate of some axis; along that axis one of them sits at local
// coordinate 0, so the pair is met from a low-face voxel when that voxel looks at its whole neighbourhood (6, 18 or 26),
// diagonals across edges, corners and high faces included.  A pair may be met twice; a union is idempotent.
// Run starts only, as in the tile pass: when v - 1 lies in v's tile, w - 1 in w's tile and both carry the key, v - 1 ~ v and
// w - 1 ~ w are row links (made in the tile pass) and v - 1 is a seam voxel that meets w - 1 through the same offset.
template <class Mem> CC_FN void cc_seam_links(Mem& m, const unsigned char* src, int n0, int n1, int n2, int select,
                                              int connectivity, int b0, int b1, int b2, int s) {
  int t0, t1, t2;
  if (s < CC_SEAM_F0) { t0 = 0; t1 = s / CC_T2; t2 = s % CC_T2; }
  else if (s < CC_SEAM_F0 + CC_SEAM_F1) { s -= CC_SEAM_F0; t1 = 0; t0 = 1 + s / CC_T2; t2 = s % CC_T2; }
  else { s -= CC_SEAM_F0 + CC_SEAM_F1; t2 = 0; t0 = 1 + s / (CC_T1 - 1); t1 = 1 + s % (CC_T1 - 1); }
  const int i0 = b0 * CC_T0 + t0, i1 = b1 * CC_T1 + t1, i2 = b2 * CC_T2 + t2;
  if (i0 >= n0 || i1 >= n1 || i2 >= n2) return;
  const int64_t v = ((int64_t)i0 * n1 + i1) * n2 + i2;
  const int k = cc_key(src[v], select);
  if (k == CC_BG) return;
  const bool left = t2 > 0 && cc_key(src[v - 1], select) == k;
  for (int d0 = -1; d0 <= 1; ++d0)
    for (int d1 = -1; d1 <= 1; ++d1)
      for (int d2 = -1; d2 <= 1; ++d2) {
        const int order = (d0 != 0) + (d1 != 0) + (d2 != 0);
        if (order == 0 || order > connectivity) continue;
        const int u0 = t0 + d0, u1 = t1 + d1, u2 = t2 + d2;
        if (u0 >= 0 && u0 < CC_T0 && u1 >= 0 && u1 < CC_T1 && u2 >= 0 && u2 < CC_T2) continue;   // same tile: done
        const int j0 = i0 + d0, j1 = i1 + d1, j2 = i2 + d2;
        if (j0 < 0 || j0 >= n0 || j1 < 0 || j1 >= n1 || j2 < 0 || j2 >= n2) continue;
        const int64_t w = ((int64_t)j0 * n1 + j1) * n2 + j2;
        if (cc_key(src[w], select) != k) continue;
        if (left && j2 % CC_T2 != 0 && cc_key(src[w - 1], select) == k) continue;
        cc_union(m, (int)v, (int)w);
      }
}

// ---- flatten pass: the label of a voxel whose tile-pass parent is p (-1: background) ----
template <class Mem> CC_FN int cc_label(Mem& m, int p) { return p < 0 ? 0 : 1 + cc_find(m, p); }
