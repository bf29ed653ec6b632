// Host check of the union / find / flatten logic of csrc/components_uf.h: the three phases of vittf_label_components driven
// sequentially over the same header (tile pass per tile with a local parent array, seam pass over the global parent array,
// flatten), in a shuffled order within every phase, against a flood fill.  No GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/micro/components_host.cpp
//       -o tools/micro/components_host && tools/micro/components_host
//
// Prints one line per case family and "OK"; exits 1 at the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../../vit-tf_amd/csrc/components_uf.h"

struct ArrayMem {
  int* p;
  int load(int i) { return p[i]; }
  int fetch_min(int i, int v) { const int old = p[i]; if (v < old) p[i] = v; return old; }
};

static std::mt19937 rng(12345);

static std::vector<int> shuffled(int n) {
  std::vector<int> o(n);
  std::iota(o.begin(), o.end(), 0);
  std::shuffle(o.begin(), o.end(), rng);
  return o;
}

static std::vector<int> label_phases(const std::vector<unsigned char>& src, int n0, int n1, int n2, int select, int conn) {
  const int64_t nvox = (int64_t)n0 * n1 * n2;
  std::vector<int> parent(nvox, -2), labels(nvox, -2);
  const int g0 = (n0 + CC_T0 - 1) / CC_T0, g1 = (n1 + CC_T1 - 1) / CC_T1, g2 = (n2 + CC_T2 - 1) / CC_T2;
  // tile pass
  for (int b0 = 0; b0 < g0; ++b0) for (int b1 = 0; b1 < g1; ++b1) for (int b2 = 0; b2 < g2; ++b2) {
    std::vector<int> par(CC_TILE);
    std::vector<unsigned char> key(CC_TILE);
    for (int l = 0; l < CC_TILE; ++l) {
      const int i2 = b2 * CC_T2 + l % CC_T2, i1 = b1 * CC_T1 + (l / CC_T2) % CC_T1, i0 = b0 * CC_T0 + l / (CC_T2 * CC_T1);
      const bool in = i0 < n0 && i1 < n1 && i2 < n2;
      key[l] = in ? (unsigned char)cc_key(src[((int64_t)i0 * n1 + i1) * n2 + i2], select) : (unsigned char)CC_BG;
    }
    for (int l = 0; l < CC_TILE; ++l) par[l] = cc_row_start(key.data(), l);
    ArrayMem m{par.data()};
    for (int l : shuffled(CC_TILE)) cc_tile_links(m, key.data(), l, conn);
    for (int l = 0; l < CC_TILE; ++l) {
      const int i2 = b2 * CC_T2 + l % CC_T2, i1 = b1 * CC_T1 + (l / CC_T2) % CC_T1, i0 = b0 * CC_T0 + l / (CC_T2 * CC_T1);
      if (i0 >= n0 || i1 >= n1 || i2 >= n2) continue;
      parent[((int64_t)i0 * n1 + i1) * n2 + i2] = key[l] == CC_BG ? -1 : cc_global_index(cc_find(m, l), b0, b1, b2, n1, n2);
    }
  }
  for (int64_t v = 0; v < nvox; ++v)
    if (parent[v] == -2 || parent[v] > v) { std::printf("tile pass: parent[%lld] = %d\n", (long long)v, parent[v]); std::exit(1); }
  // seam pass
  ArrayMem gm{parent.data()};
  const int tiles = g0 * g1 * g2;
  for (int t : shuffled(tiles)) {
    const int b2 = t % g2, b1 = (t / g2) % g1, b0 = t / (g2 * g1);
    for (int s : shuffled(CC_SEAM)) cc_seam_links(gm, src.data(), n0, n1, n2, select, conn, b0, b1, b2, s);
  }
  for (int64_t v = 0; v < nvox; ++v)
    if (parent[v] > v) { std::printf("seam pass: parent[%lld] = %d\n", (long long)v, parent[v]); std::exit(1); }
  // flatten
  for (int64_t v = 0; v < nvox; ++v) labels[v] = cc_label(gm, parent[v]);
  return labels;
}

static std::vector<int> label_flood(const std::vector<unsigned char>& src, int n0, int n1, int n2, int select, int conn) {
  const int64_t nvox = (int64_t)n0 * n1 * n2;
  std::vector<int> labels(nvox, 0);
  std::vector<int64_t> stack;
  for (int64_t seed = 0; seed < nvox; ++seed) {        // ascending: the seed is the smallest index of its component
    const int k = cc_key(src[seed], select);
    if (k == CC_BG || labels[seed]) continue;
    labels[seed] = (int)seed + 1;
    stack.push_back(seed);
    while (!stack.empty()) {
      const int64_t v = stack.back(); stack.pop_back();
      const int i2 = (int)(v % n2), i1 = (int)((v / n2) % n1), i0 = (int)(v / ((int64_t)n1 * n2));
      for (int d0 = -1; d0 <= 1; ++d0) for (int d1 = -1; d1 <= 1; ++d1) for (int d2 = -1; d2 <= 1; ++d2) {
        const int order = std::abs(d0) + std::abs(d1) + std::abs(d2);
        if (order == 0 || order > conn) continue;
        const int j0 = i0 + d0, j1 = i1 + d1, j2 = i2 + d2;
        if (j0 < 0 || j0 >= n0 || j1 < 0 || j1 >= n1 || j2 < 0 || j2 >= n2) continue;
        const int64_t w = ((int64_t)j0 * n1 + j1) * n2 + j2;
        if (labels[w] || cc_key(src[w], select) != k) continue;
        labels[w] = (int)seed + 1;
        stack.push_back(w);
      }
    }
  }
  return labels;
}

static int cases = 0;

static void check(const char* what, const std::vector<unsigned char>& src, int n0, int n1, int n2, int select, int conn) {
  const std::vector<int> got = label_phases(src, n0, n1, n2, select, conn), want = label_flood(src, n0, n1, n2, select, conn);
  ++cases;
  for (size_t v = 0; v < got.size(); ++v)
    if (got[v] != want[v]) {
      std::printf("MISMATCH %s (%d, %d, %d) select %d connectivity %d at voxel %zu: %d, flood fill %d\n", what, n0, n1, n2,
                  select, conn, v, got[v], want[v]);
      std::exit(1);
    }
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 1, CC_T2 + 1}, {3, 5, 7}, {CC_T0 - 1, CC_T1 - 1, CC_T2 - 1}, {CC_T0, CC_T1, CC_T2},
                           {CC_T0 + 1, CC_T1 + 1, CC_T2 + 1}, {2 * CC_T0 + 1, 3 * CC_T1 + 1, 2 * CC_T2 + 2}, {13, 18, 131}};
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  for (const auto& sh : shapes) {
    const int n0 = sh[0], n1 = sh[1], n2 = sh[2];
    const size_t nvox = (size_t)n0 * n1 * n2;
    std::vector<unsigned char> src(nvox);
    for (int conn = 1; conn <= 3; ++conn) {
      for (double p : {0.0, 0.10, 0.14, 0.31, 0.5, 0.9, 1.0}) {
        for (auto& x : src) x = uni(rng) < p ? 1 : 0;
        check("noise", src, n0, n1, n2, -1, conn);
        check("noise", src, n0, n1, n2, 1, conn);
      }
      for (size_t v = 0; v < nvox; ++v) src[v] = (unsigned char)(((v / ((size_t)n1 * n2)) + ((v / n2) % n1) + (v % n2)) % 2 == 0);
      check("checkerboard", src, n0, n1, n2, -1, conn);
      // serpentine: rows along n2 joined alternately at their ends, planes joined alternately at their last / first row
      std::fill(src.begin(), src.end(), 0);
      for (int i0 = 0; i0 < n0; i0 += 2)
        for (int i1 = 0; i1 < n1; ++i1)
          for (int i2 = 0; i2 < n2; ++i2) {
            const bool row = i1 % 2 == 0, joint = i1 % 2 == 1 && i2 == (((i1 / 2) % 2 == 0) ? n2 - 1 : 0);
            if (row || joint) src[((size_t)i0 * n1 + i1) * n2 + i2] = 1;
          }
      check("serpentine", src, n0, n1, n2, -1, conn);
      // values in random blocks, 255 masked out
      for (size_t v = 0; v < nvox; ++v) {
        const int i2 = (int)(v % n2), i1 = (int)((v / n2) % n1), i0 = (int)(v / ((size_t)n1 * n2));
        const unsigned h = (unsigned)((i0 / 2) * 73856093u) ^ (unsigned)((i1 / 3) * 19349663u) ^ (unsigned)((i2 / 5) * 83492791u);
        src[v] = (h >> 7) % 7 == 6 ? 255 : (unsigned char)((h >> 7) % 7);
      }
      check("values", src, n0, n1, n2, -2, conn);
      check("values", src, n0, n1, n2, -1, conn);
      check("values", src, n0, n1, n2, 0, conn);
      check("values", src, n0, n1, n2, 3, conn);
    }
    std::printf("(%d, %d, %d): ok\n", n0, n1, n2);
  }
  // two slabs that touch only across a tile corner: linked under connectivity 3 only
  {
    const int n0 = 2 * CC_T0, n1 = 2 * CC_T1, n2 = 2 * CC_T2;
    std::vector<unsigned char> src((size_t)n0 * n1 * n2, 0);
    for (int i0 = 0; i0 < n0; ++i0) for (int i1 = 0; i1 < n1; ++i1) for (int i2 = 0; i2 < n2; ++i2) {
      const bool low = i0 < CC_T0 && i1 < CC_T1 && i2 < CC_T2, high = i0 >= CC_T0 && i1 >= CC_T1 && i2 >= CC_T2;
      src[((size_t)i0 * n1 + i1) * n2 + i2] = low || high;
    }
    for (int conn = 1; conn <= 3; ++conn) check("corner", src, n0, n1, n2, -1, conn);
    std::printf("corner slabs: ok\n");
  }
  std::printf("OK: %d cases agree with the flood fill\n", cases);
  return 0;
}
