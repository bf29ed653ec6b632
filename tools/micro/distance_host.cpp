// Host check of the line walk of csrc/distance_env.h: the axis-1 and axis-0 passes of vittf_edt_sq / vittf_edt_sq_weighted
// driven sequentially over the same header, tile by tile as the kernel does it (a [position][lane] copy of the tile, the two
// 16-bit stacks, the width that edt_tile_width derives), after a plain two-scan row pass, against a brute-force minimum over
// all sites.  Integer results must be equal; weighted results within 2^-40 D2 in fp64; the returned site must lie at the
// returned distance.  No GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/micro/distance_host.cpp
//       -o tools/micro/distance_host && tools/micro/distance_host
//
// Prints one line per shape and "OK"; exits 1 at the first mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../vit-tf_amd/csrc/distance_env.h"

static std::mt19937 rng(2024);
constexpr size_t BUDGET = 80 * 1024;
constexpr int THREADS = 256;

template <typename T, typename Out>
static void line_pass(std::vector<T>& in, std::vector<Out>& out, const std::vector<int>& site_in, std::vector<int>& site_out, int n,
                      int64_t stride, int64_t lines, int slabs, int64_t slab, T w) {
  const int width = edt_tile_width<T>(n, lines, BUDGET, THREADS);
  if (width < 1 || (size_t)n * width * (sizeof(T) + 4) > BUDGET) { std::printf("tile width %d breaks the budget\n", width); std::exit(1); }
  for (int y = 0; y < slabs; ++y)
    for (int64_t first = 0; first < lines; first += width) {
      const int live = lines - first < width ? (int)(lines - first) : width;
      const int64_t base = y * slab + first;
      std::vector<T> g((size_t)n * width);
      std::vector<unsigned short> s((size_t)n * width), t((size_t)n * width);
      for (int e = 0; e < n * width; ++e) {
        const int u = e / width, c = e - u * width;
        if (c < live) g[e] = in[base + u * stride + c];
      }
      for (int c = 0; c < live; ++c)
        edt_walk_line<T, Out, true>(g.data(), s.data(), t.data(), width, c, n, w, out.data() + base + c, site_in.data() + base + c,
                                    site_out.data() + base + c, stride);
    }
}

template <typename T, typename Out>
static void transform(const std::vector<unsigned char>& site, int n0, int n1, int n2, const T* w, std::vector<Out>& d2,
                      std::vector<int>& where) {
  const int64_t nvox = (int64_t)n0 * n1 * n2, plane = (int64_t)n1 * n2;
  std::vector<T> mid(nvox);
  std::vector<int> sa(nvox), sb(nvox);
  for (int64_t line = 0; line < (int64_t)n0 * n1; ++line)
    for (int i = 0; i < n2; ++i) {
      int best = -1;
      for (int j = 0; j < n2; ++j)
        if (site[line * n2 + j] && (best < 0 || std::abs(j - i) < std::abs(best - i))) best = j;
      mid[line * n2 + i] = best < 0 ? Edt<T>::none() : Edt<T>::sq(w[2], i - best);
      sa[line * n2 + i] = best < 0 ? -1 : (int)(line * n2 + best);
    }
  line_pass<T, T>(mid, mid, sa, sb, n1, n2, n2, n0, plane, w[1]);
  d2.assign(nvox, Out());
  line_pass<T, Out>(mid, d2, sb, where, n0, plane, plane, 1, 0, w[0]);
}

static int check(int n0, int n1, int n2, double density, const double* w2) {
  const int64_t nvox = (int64_t)n0 * n1 * n2;
  std::vector<unsigned char> site(nvox);
  std::vector<int64_t> sites;
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  for (int64_t v = 0; v < nvox; ++v)
    if ((site[v] = uni(rng) < density)) sites.push_back(v);
  const int one[3] = {1, 1, 1};
  std::vector<int> di, wi(nvox), ww(nvox);
  std::vector<float> dw;
  transform<int, int>(site, n0, n1, n2, one, di, wi);
  transform<double, float>(site, n0, n1, n2, w2, dw, ww);
  const double D2 = w2[0] * (n0 - 1) * (n0 - 1) + w2[1] * (n1 - 1) * (n1 - 1) + w2[2] * (n2 - 1) * (n2 - 1);
  for (int64_t v = 0; v < nvox; ++v) {
    const int i0 = (int)(v / ((int64_t)n1 * n2)), i1 = (int)(v / n2 % n1), i2 = (int)(v % n2);
    int64_t best = -1;
    double bestw = HUGE_VAL;
    for (int64_t sv : sites) {
      const int64_t a = i0 - sv / ((int64_t)n1 * n2), b = i1 - sv / n2 % n1, c = i2 - sv % n2;
      const int64_t d = a * a + b * b + c * c;
      const double x = w2[0] * a * a + w2[1] * b * b + w2[2] * c * c;
      if (best < 0 || d < best) best = d;
      if (x < bestw) bestw = x;
    }
    auto at = [&](int64_t sv, bool weighted) {
      const int64_t a = i0 - sv / ((int64_t)n1 * n2), b = i1 - sv / n2 % n1, c = i2 - sv % n2;
      return weighted ? w2[0] * a * a + w2[1] * b * b + w2[2] * c * c : (double)(a * a + b * b + c * c);
    };
    if (sites.empty()) {
      if (di[v] != Edt<int>::none() || wi[v] != -1 || !std::isinf(dw[v]) || ww[v] != -1) return std::printf("no-site sentinel missing at %lld\n", (long long)v), 1;
      continue;
    }
    if (di[v] != best || wi[v] < 0 || !site[wi[v]] || at(wi[v], false) != (double)best)
      return std::printf("integer mismatch at %lld: %d want %lld (site %d)\n", (long long)v, di[v], (long long)best, wi[v]), 1;
    const double tol = std::ldexp(bestw, -24) + std::ldexp(D2, -40);
    if (std::fabs((double)dw[v] - bestw) > tol || ww[v] < 0 || !site[ww[v]] || std::fabs(at(ww[v], true) - bestw) > std::ldexp(D2, -40))
      return std::printf("weighted mismatch at %lld: %.9g want %.9g (site %d)\n", (long long)v, (double)dw[v], bestw, ww[v]), 1;
  }
  return 0;
}

int main() {
  const int shapes[][3] = {{5, 7, 67}, {3, 130, 9}, {1, 1, 300}, {40, 1, 33}, {2, 3, 2048}, {2, 2048, 3}, {2048, 2, 2}, {24, 24, 24}, {1, 1, 1}};
  const double spacings[][3] = {{0.7 * 0.7, 0.7 * 0.7, 2.5 * 2.5}, {9.0, 0.0625, 1.0}, {1.0, 1.0, 1.0}, {1e6, 1e-6, 3.0}};
  for (const auto& sh : shapes) {
    int cases = 0;
    for (const auto& w2 : spacings)
      for (double density : {0.0, 0.0008, 0.02, 0.5, 1.0}) {
        if (check(sh[0], sh[1], sh[2], density, w2)) return 1;
        ++cases;
      }
    std::printf("%d x %d x %d: %d cases\n", sh[0], sh[1], sh[2], cases);
  }
  std::printf("OK\n");
  return 0;
}
