// The line walk of the Euclidean distance transform (distance.hip): the lower envelope of the parabolas g(i) + w (x - i)^2
// along one line (Meijster, Roerdink and Hesselink 2000), free of any HIP call so that a host program
// (tools/micro/distance_host.cpp) drives the same code over plain arrays and checks it against a brute-force minimum.
//
// All arrays of a tile are [position][lane] images `width` lanes wide; lane c walks line c:
//   g  the values of the previous pass (Edt<T>::none(): no site in that line, such a position is no parabola and is skipped,
//      so the sentinel never enters the arithmetic);
//   s  stack, the position of parabola q;      t  stack, the first position at which parabola q is the lowest.
// Both stacks hold positions < n <= 2048 in 16 bits.  t is strictly increasing along the stack and t[0] = 0, so q <= t[q] and
// the backward scan pops exactly when it leaves a parabola's range.
//
// Edt<int>: exact.  Values are at most 3 x 2047^2 < 2^31.  At the separator, the pops have established
// g(i) + (t - i)^2 <= g(u) + (t - u)^2 for the top (i, t), that is u^2 - i^2 + g(u) - g(i) >= 2 t (u - i) >= 0: the truncating
// division is the floor, and the new entry's t exceeds the top's.
// Edt<double>: the same in fp64 on weighted values.  Rounding may decide a comparison or a separator the other way only between
// parabolas whose values there differ by the roundings themselves; the separator is forced past the top's, which exact
// arithmetic guarantees, so t stays strictly increasing whatever the rounding.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_FN __host__ __device__ __forceinline__
#else
#define EDT_FN inline
#endif

constexpr int EDT_MAX_DIM = 2048;

template <typename T> struct Edt;
template <> struct Edt<int> {
  static EDT_FN int none() { return 0x7fffffff; }
  static EDT_FN bool is_site(int g) { return g != 0x7fffffff; }
  static EDT_FN int sq(int, int d) { return d * d; }                   // the weight is 1
  // first position at which parabola u (value gu) is lower than parabola i < u (value gi, the top, winning from t_top on)
  static EDT_FN int first_win(int, int i, int gi, int u, int gu, int, int) {
    return 1 + (u * u - i * i + gu - gi) / (2 * (u - i));
  }
};
template <> struct Edt<double> {
  static EDT_FN double none() { return HUGE_VAL; }
  static EDT_FN bool is_site(double g) { return g < HUGE_VAL; }
  static EDT_FN double sq(double w, int d) { return w * (double)(d * d); }
  static EDT_FN int first_win(double w, int i, double gi, int u, double gu, int n, int t_top) {
    const double x = floor(((gu - gi) + w * (double)(u * u - i * i)) / (2.0 * w * (double)(u - i)));
    const int f = 1 + (int)fmin(fmax(x, -1.0), (double)n);
    return f > t_top ? f : t_top + 1;
  }
};

EDT_FN float edt_store(float*, double v) { return (float)v; }
EDT_FN double edt_store(double*, double v) { return v; }
EDT_FN int edt_store(int*, int v) { return v; }

// Lane c of a tile: builds the envelope of line c (g, s, t: see above), then stores out[u stride] for u = n-1 .. 0 and, with
// SITE, site_out[u stride] = site_in[i stride] of the winning parabola i (-1 in a line without a site).  out / site_in /
// site_out point at position 0 of the line.
template <typename T, typename Out, bool SITE>
EDT_FN void edt_walk_line(const T* g, unsigned short* s, unsigned short* t, int width, int c, int n, T w, Out* out,
                          const int* site_in, int* site_out, int64_t stride) {
  int q = -1;
  for (int u = 0; u < n; ++u) {
    const T gu = g[u * width + c];
    if (!Edt<T>::is_site(gu)) continue;
    int i = 0, ti = 0;
    T gi = 0;
    while (q >= 0) {
      i = s[q * width + c];
      ti = t[q * width + c];
      gi = g[i * width + c];
      if (gi + Edt<T>::sq(w, ti - i) > gu + Edt<T>::sq(w, ti - u)) --q; else break;
    }
    if (q < 0) {
      q = 0;
      s[c] = (unsigned short)u;
      t[c] = 0;
    } else {
      const int f = Edt<T>::first_win(w, i, gi, u, gu, n, ti);
      if (f < n) {
        ++q;
        s[q * width + c] = (unsigned short)u;
        t[q * width + c] = (unsigned short)f;
      }
    }
  }
  for (int u = n - 1; u >= 0; --u) {
    if (q < 0) {                                                        // a line without a site (then for every u)
      out[u * stride] = edt_store(out, Edt<T>::none());
      if (SITE) site_out[u * stride] = -1;
      continue;
    }
    const int i = s[q * width + c];
    out[u * stride] = edt_store(out, g[i * width + c] + Edt<T>::sq(w, u - i));
    if (SITE) site_out[u * stride] = site_in[i * stride];
    if (q > 0 && u == t[q * width + c]) --q;
  }
}

// Lines of length n that one workgroup takes: what `lds_budget` bytes hold at value + two 16-bit stack entries per position,
// at most one per thread and no more than there are; a multiple of 8 (whole 32-byte rows of int32) where it can be.
template <typename T> EDT_FN int edt_tile_width(int n, int64_t lines, size_t lds_budget, int threads) {
  int64_t width = (int64_t)(lds_budget / ((size_t)n * (sizeof(T) + 4)));
  if (width > threads) width = threads;
  if (width >= 8) width &= ~(int64_t)7;
  if (width > lines) width = lines;
  return (int)width;
}
