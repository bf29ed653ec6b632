// Direct volume rendering of an intensity volume with up to 8 class maps as per-class opacity (vit-tf_amd/render.py,
// render_volume.py).  gfx950 has no texture unit: every sample is a manual trilinear gather.  The model -- coordinates,
// transfer function, coverage, compositing, shading, occupancy -- is stated once in include/vittf.h; tests/render_data.py
// restates it in fp64.
//
//   prepare    q = rint(65535 clamp((V - vmin) / (vmax - vmin), 0, 1)) in fp64, stored uint16 (linear layout): half the
//              bytes of the fp32 volume under every gather.  Four voxels a lane, one 16-byte load and one 8-byte store.
//   occupancy  one wave per 8^3 brick: min / max of q over the brick's 9^3 footprint and the maximum of every class map
//              over the map voxels the footprint can touch (wave shuffles), then the two integer emptiness rules.
//   render     one ray per lane, an 8 x 8 pixel tile per wave, 16 x 16 per workgroup, so the rays of a wave stay close in
//              the volume.  Samples sit on the global lattice t_i = (i + 0.5) dt.  Each sample is classified by its OWN
//              brick; in an empty brick the lane computes where the ray leaves it and moves to the last sample before the
//              exit, but only after it has checked that this sample lies in the same brick.  t -> brick index is monotone
//              per axis in fp32 as well (fma, divide, subtract, floor are monotone), so every sample in between lies in
//              that brick too: a jump passes only samples it has proved empty, and a halved jump always terminates.
// Exact zeros: an interpolated value is clamped to the range of its eight corners (a no-op in exact arithmetic), so a
// sample of an empty brick has sigma == 0 bit for bit whether or not the grid is given, and the images with and without
// the grid are the same bytes.  No atomics; every pixel is stored once by one lane.
#include <math.h>
#include "vittf_internal.h"

namespace {

constexpr int RENDER_THREADS = 256;                 // 16 x 16 pixels; wave w is the 8 x 8 tile (w & 1, w >> 1)
constexpr int64_t RENDER_MAX_VOX = 0x7fffffffLL;
constexpr float RENDER_TINY = 1e-30f;
constexpr float RENDER_STOP = 1.0f / 1024.0f;       // the ray ends when T < 2^-10
constexpr double RENDER_MAX_STEPS = 4194304.0;      // 2^22 lattice samples between the eye and the far end of the box

struct RenderParams {
  const uint16_t* q;
  const float4* table;
  const uint8_t* maps;
  const uint8_t* occ;
  float4* out;
  int n[3], m[3], nb[3];
  int classes, width, height;
  float s[3], box[3];                               // spacing; n_a s_a
  float eye[3], ox[3], oy[3], fwd[3], dx[3], dy[3];
  float dt, ka, kd, eps;
  int lo[VITTF_RENDER_MAX_CLASSES];
  float range[VITTF_RENDER_MAX_CLASSES];            // hi - lo
  float rgbs[VITTF_RENDER_MAX_CLASSES][4];          // colour, strength
};

struct OccParams {
  const uint16_t* q;
  const float4* table;
  const uint8_t* maps;
  uint8_t* occ;
  int n[3], m[3], nb[3];
  int classes;
  int lo[VITTF_RENDER_MAX_CLASSES];
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }
__device__ __forceinline__ float min8(const float c[8]) {
  return fminf(fminf(fminf(c[0], c[1]), fminf(c[2], c[3])), fminf(fminf(c[4], c[5]), fminf(c[6], c[7])));
}
__device__ __forceinline__ float max8(const float c[8]) {
  return fmaxf(fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3])), fmaxf(fmaxf(c[4], c[5]), fmaxf(c[6], c[7])));
}
// corners c[4 j0 + 2 j1 + j2]; the result never leaves the range of the corners
__device__ __forceinline__ float trilerp(const float c[8], float f0, float f1, float f2) {
  const float a = lerpf(lerpf(c[0], c[1], f2), lerpf(c[2], c[3], f2), f1);
  const float b = lerpf(lerpf(c[4], c[5], f2), lerpf(c[6], c[7], f2), f1);
  return fminf(fmaxf(lerpf(a, b, f0), min8(c)), max8(c));
}

// index coordinate along one axis of lattice sample i: x = (o + t d) / s - 0.5, t = (i + 0.5) dt.  The ONE expression both the
// sample and the jump check evaluate, so that they cannot disagree about a brick.
__device__ __forceinline__ float ray_index(int i, float dt, float o, float d, float s) {
  return fmaf(((float)i + 0.5f) * dt, d, o) / s - 0.5f;
}
__device__ __forceinline__ int ray_brick(int i, float dt, float o, float d, float s, int n) {
  return clampi((int)floorf(ray_index(i, dt, o, d, s)), n - 1) >> 3;
}

__global__ __launch_bounds__(RENDER_THREADS) void render_kernel(const RenderParams P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (px >= P.width || py >= P.height) return;
  float4* pixel = P.out + (size_t)py * P.width + px;
  const float u = 2.0f * ((float)px + 0.5f) / (float)P.width - 1.0f;
  const float v = 1.0f - 2.0f * ((float)py + 0.5f) / (float)P.height;
  float o[3], d[3];
  float len2 = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = P.eye[a] + u * P.ox[a] + v * P.oy[a];
    d[a] = P.fwd[a] + u * P.dx[a] + v * P.dy[a];
    len2 += d[a] * d[a];
  }
  const float len = sqrtf(len2);
  float tmin = 0.f, tmax = INFINITY;
  bool hit = len > 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    d[a] = d[a] / len;
    const float lo = -0.5f * P.s[a], hi = ((float)P.n[a] + 0.5f) * P.s[a];
    if (d[a] == 0.f) {                              // parallel to the slab: inside it or never
      hit = hit && o[a] >= lo && o[a] <= hi;
    } else {
      const float t1 = (lo - o[a]) / d[a], t2 = (hi - o[a]) / d[a];
      tmin = fmaxf(tmin, fminf(t1, t2));
      tmax = fminf(tmax, fmaxf(t1, t2));
    }
  }
  if (!hit || !(tmin <= tmax)) {
    *pixel = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  // one lattice sample more at either end: a sample outside the grown box has coverage exactly 0, so rounding in tmin and
  // tmax cannot drop a sample that counts
  int i = (int)ceilf(tmin / P.dt - 0.5f) - 1;
  if (i < 0) i = 0;
  const int last = (int)floorf(tmax / P.dt - 0.5f) + 1;
  const int n0 = P.n[0], n1 = P.n[1], n2 = P.n[2];
  float T = 1.f, R = 0.f, G = 0.f, B = 0.f, A = 0.f;
  while (i <= last) {
    float x[3], f[3];
    int i0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      x[a] = ray_index(i, P.dt, o[a], d[a], P.s[a]);
      const float fl = floorf(x[a]);
      f[a] = x[a] - fl;
      i0[a] = (int)fl;
    }
    if (P.occ) {
      const int b0 = clampi(i0[0], n0 - 1) >> 3, b1 = clampi(i0[1], n1 - 1) >> 3, b2 = clampi(i0[2], n2 - 1) >> 3;
      if (!P.occ[((size_t)b0 * P.nb[1] + b1) * P.nb[2] + b2]) {
        const int b[3] = {b0, b1, b2};
        float texit = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          if (d[a] > 0.f && b[a] < P.nb[a] - 1) texit = fminf(texit, (((float)(8 * b[a] + 8) + 0.5f) * P.s[a] - o[a]) / d[a]);
          if (d[a] < 0.f && b[a] > 0) texit = fminf(texit, (((float)(8 * b[a]) + 0.5f) * P.s[a] - o[a]) / d[a]);
        }
        int j = last;
        const float jf = floorf(texit / P.dt - 0.5f);
        if (jf < (float)last) j = (int)jf;             // false for inf and NaN
        if (j < i) j = i;
        while (j > i && (ray_brick(j, P.dt, o[0], d[0], P.s[0], n0) != b0 || ray_brick(j, P.dt, o[1], d[1], P.s[1], n1) != b1 ||
                         ray_brick(j, P.dt, o[2], d[2], P.s[2], n2) != b2))
          j = i + ((j - i) >> 1);
        i = j + 1;
        continue;
      }
    }
    // coverage: the weights of the in-bounds corners, factorised per axis
    float cov = 1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int n = P.n[a];
      cov *= ((i0[a] >= 0 && i0[a] < n) ? 1.f - f[a] : 0.f) + ((i0[a] >= -1 && i0[a] < n - 1) ? f[a] : 0.f);
    }
    if (!(cov > 0.f)) {
      ++i;
      continue;
    }
    // positions -1, 0, +1, +2 around the cell along each axis, border-clamped, as element offsets
    int e0[4], e1[4], e2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e0[k] = clampi(i0[0] - 1 + k, n0 - 1) * n1 * n2;
      e1[k] = clampi(i0[1] - 1 + k, n1 - 1) * n2;
      e2[k] = clampi(i0[2] - 1 + k, n2 - 1);
    }
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = (float)P.q[e0[1 + (k >> 2)] + e1[1 + ((k >> 1) & 1)] + e2[1 + (k & 1)]];
    const float inten = trilerp(c, f[0], f[1], f[2]);
    const float tc = inten / 257.0f;
    int ti = (int)tc;
    if (ti > 254) ti = 254;
    const float tf = tc - (float)ti;
    const float4 ta = P.table[ti], tb = P.table[ti + 1];
    float sigma = lerpf(ta.w, tb.w, tf) * cov;
    float cr = sigma * lerpf(ta.x, tb.x, tf), cg = sigma * lerpf(ta.y, tb.y, tf), cb = sigma * lerpf(ta.z, tb.z, tf);
    if (P.classes > 0) {
      float g[3];
      int m0[3], m1[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float p = fmaf(((float)i + 0.5f) * P.dt, d[a], o[a]);
        const float xm = p / P.box[a] * (float)P.m[a] - 0.5f;
        const float fl = floorf(xm);
        g[a] = xm - fl;
        m0[a] = clampi((int)fl, P.m[a] - 1);
        m1[a] = clampi((int)fl + 1, P.m[a] - 1);
      }
      const int64_t mvox = (int64_t)P.m[0] * P.m[1] * P.m[2];
      const int r00 = (m0[0] * P.m[1] + m0[1]) * P.m[2], r01 = (m0[0] * P.m[1] + m1[1]) * P.m[2];
      const int r10 = (m1[0] * P.m[1] + m0[1]) * P.m[2], r11 = (m1[0] * P.m[1] + m1[1]) * P.m[2];
      for (int k = 0; k < P.classes; ++k) {
        const uint8_t* map = P.maps + k * mvox;
        const float w[8] = {(float)map[r00 + m0[2]], (float)map[r00 + m1[2]], (float)map[r01 + m0[2]], (float)map[r01 + m1[2]],
                            (float)map[r10 + m0[2]], (float)map[r10 + m1[2]], (float)map[r11 + m0[2]], (float)map[r11 + m1[2]]};
        const float val = trilerp(w, g[0], g[1], g[2]);
        const float omega = fminf(fmaxf((val - (float)P.lo[k]) / P.range[k], 0.f), 1.f);
        const float sk = P.rgbs[k][3] * omega * cov;
        sigma += sk;
        cr = fmaf(sk, P.rgbs[k][0], cr);
        cg = fmaf(sk, P.rgbs[k][1], cg);
        cb = fmaf(sk, P.rgbs[k][2], cb);
      }
    }
    if (sigma > 0.f) {
      float shade = P.ka;
      if (P.kd != 0.f) {
        // central differences of the trilinear intensity one voxel either way, with the centre's fractions: 8 more voxels
        // an axis (32 distinct ones with the centre's 8)
        float grad[3];
        {
          float dlt[4];                                  // axis 0: [j1][j2]
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int rest = e1[1 + (k >> 1)] + e2[1 + (k & 1)];
            const float lo = (float)P.q[e0[0] + rest], hi = (float)P.q[e0[3] + rest];
            dlt[k] = lerpf(c[4 + k] - lo, hi - c[k], f[0]);
          }
          grad[0] = lerpf(lerpf(dlt[0], dlt[1], f[2]), lerpf(dlt[2], dlt[3], f[2]), f[1]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {                  // axis 1: [j0][j2]
            const int rest = e0[1 + (k >> 1)] + e2[1 + (k & 1)];
            const float lo = (float)P.q[rest + e1[0]], hi = (float)P.q[rest + e1[3]];
            const int at = 4 * (k >> 1) + (k & 1);
            dlt[k] = lerpf(c[at + 2] - lo, hi - c[at], f[1]);
          }
          grad[1] = lerpf(lerpf(dlt[0], dlt[1], f[2]), lerpf(dlt[2], dlt[3], f[2]), f[0]);
#pragma unroll
          for (int k = 0; k < 4; ++k) {                  // axis 2: [j0][j1]
            const int rest = e0[1 + (k >> 1)] + e1[1 + (k & 1)];
            const float lo = (float)P.q[rest + e2[0]], hi = (float)P.q[rest + e2[3]];
            dlt[k] = lerpf(c[2 * k + 1] - lo, hi - c[2 * k], f[2]);
          }
          grad[2] = lerpf(lerpf(dlt[0], dlt[1], f[1]), lerpf(dlt[2], dlt[3], f[1]), f[0]);
        }
        float dot = 0.f, gg = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float ga = grad[a] / (2.0f * P.s[a]);
          dot = fmaf(ga, d[a], dot);
          gg = fmaf(ga, ga, gg);
        }
        shade = P.ka + P.kd * fabsf(dot) / (sqrtf(gg) + P.eps);
      }
      const float alpha = 1.0f - expf(-sigma * P.dt);
      const float wgt = T * alpha * shade / fmaxf(sigma, RENDER_TINY);
      R = fmaf(wgt, cr, R);
      G = fmaf(wgt, cg, G);
      B = fmaf(wgt, cb, B);
      A = fmaf(T, alpha, A);
      T *= 1.0f - alpha;
      if (T < RENDER_STOP) break;
    }
    ++i;
  }
  *pixel = make_float4(R, G, B, A);
}

// One wave per brick.  Footprint of brick b along an axis of n voxels: voxels 8 b .. min(8 b + 8, n - 1), the corners of every
// sample whose clamped cell index lies in the brick.  Map voxels along an axis of m: a sample of the brick has p / s in
// [8 b, 8 b + 9) (x + 0.5 with x in [8 b, 8 b + 8); the first and the last brick also take the samples outside, whose indices
// clamp into the range).  The rule takes [8 b - 1, 8 b + 10): a whole voxel either way, at least 2 / 2048 of a map voxel,
// against the few 2^-13 by which the fp32 map coordinate can be off.  Then p / (n s) m - 0.5 has floor >=
// ((8 b - 1) m) div n - 1 and floor + 1 <= ((8 b + 10) m) div n + 1, clamped to the grid.
__global__ __launch_bounds__(64) void render_occupancy_kernel(const OccParams P) {
  const int lane = threadIdx.x;
  const int64_t brick = blockIdx.x;
  const int b2 = (int)(brick % P.nb[2]), b1 = (int)(brick / P.nb[2] % P.nb[1]), b0 = (int)(brick / ((int64_t)P.nb[2] * P.nb[1]));
  const int b[3] = {b0, b1, b2};
  int lo[3], ext[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = 8 * b[a];
    const int hi = 8 * b[a] + 8 < P.n[a] - 1 ? 8 * b[a] + 8 : P.n[a] - 1;
    ext[a] = hi - lo[a] + 1;
  }
  int qmin = 65535, qmax = 0;
  for (int e = lane; e < ext[0] * ext[1] * ext[2]; e += 64) {
    const int k2 = e % ext[2], k1 = e / ext[2] % ext[1], k0 = e / (ext[2] * ext[1]);
    const int val = P.q[((size_t)(lo[0] + k0) * P.n[1] + lo[1] + k1) * P.n[2] + lo[2] + k2];
    qmin = val < qmin ? val : qmin;
    qmax = val > qmax ? val : qmax;
  }
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const int a = __shfl_xor(qmin, sft), c = __shfl_xor(qmax, sft);
    qmin = a < qmin ? a : qmin;
    qmax = c > qmax ? c : qmax;
  }
  const int ja = qmin / 257, jb = qmax / 257 + 1 < 255 ? qmax / 257 + 1 : 255;
  bool full = false;
  for (int j = ja + lane; j <= jb; j += 64) full = full || P.table[j].w != 0.f;
  bool any = __any(full);
  for (int k = 0; k < P.classes && !any; ++k) {
    int mlo[3], mext[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int l = (8 * b[a] - 1) * P.m[a] / P.n[a] - 1, h = (8 * b[a] + 10) * P.m[a] / P.n[a] + 1;
      mlo[a] = l < 0 ? 0 : l;
      mext[a] = (h > P.m[a] - 1 ? P.m[a] - 1 : h) - mlo[a] + 1;
    }
    const uint8_t* map = P.maps + k * ((int64_t)P.m[0] * P.m[1] * P.m[2]);
    int top = 0;
    const int64_t count = (int64_t)mext[0] * mext[1] * mext[2];
    for (int64_t e = lane; e < count; e += 64) {
      const int k2 = (int)(e % mext[2]), k1 = (int)(e / mext[2] % mext[1]), k0 = (int)(e / ((int64_t)mext[2] * mext[1]));
      const int val = map[((size_t)(mlo[0] + k0) * P.m[1] + mlo[1] + k1) * P.m[2] + mlo[2] + k2];
      top = val > top ? val : top;
    }
    any = __any(top > P.lo[k]);
  }
  if (lane == 0) P.occ[brick] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void render_prepare_kernel(const float* __restrict__ vol, int64_t nvox, double vmin, double range,
                                                             uint16_t* __restrict__ q) {
  const int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (at >= nvox) return;
  float v[4];
  const int live = nvox - at < 4 ? (int)(nvox - at) : 4;
  if (live == 4) {
    const float4 x = *reinterpret_cast<const float4*>(vol + at);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = k < live ? vol[at + k] : 0.f;
  }
  unsigned short r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double y = ((double)v[k] - vmin) / range;
    y = y < 0.0 ? 0.0 : (y > 1.0 ? 1.0 : y);
    r[k] = (unsigned short)rint(65535.0 * y);
  }
  if (live == 4) {
    *reinterpret_cast<uint2*>(q + at) = make_uint2(r[0] | ((unsigned)r[1] << 16), r[2] | ((unsigned)r[3] << 16));
  } else {
    for (int k = 0; k < live; ++k) q[at + k] = r[k];
  }
}

bool render_dims_ok(int32_t n0, int32_t n1, int32_t n2) {
  if (n0 < 2 || n1 < 2 || n2 < 2 || n0 > VITTF_RENDER_MAX_DIM || n1 > VITTF_RENDER_MAX_DIM || n2 > VITTF_RENDER_MAX_DIM) return false;
  return (int64_t)n0 * n1 * n2 <= RENDER_MAX_VOX;
}

bool finite_all(const float* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!isfinite(v[k])) return false;
  return true;
}

// classes, maps, map grid and lo (hi when given) of one call
bool render_classes_ok(const uint8_t* maps, int32_t classes, int32_t m0, int32_t m1, int32_t m2, const int32_t* lo, const int32_t* hi) {
  if (classes < 0 || classes > VITTF_RENDER_MAX_CLASSES) return false;
  if (classes == 0) return true;
  if (!maps || !lo || !render_dims_ok(m0, m1, m2)) return false;
  for (int k = 0; k < classes; ++k) {
    if (lo[k] < 0 || lo[k] > 255) return false;
    if (hi && (hi[k] <= lo[k] || hi[k] > 255)) return false;
  }
  return true;
}

}  // namespace

extern "C" int vittf_render_prepare(const float* volume, int64_t nvox, double vmin, double vmax, uint16_t* q, void* stream) {
  if (!volume || !q || nvox < 1 || nvox > RENDER_MAX_VOX || !isfinite(vmin) || !isfinite(vmax) || !(vmin < vmax) ||
      !isfinite(vmax - vmin))
    return VITTF_ERR_INVALID_ARG;
  if ((((uintptr_t)volume) & 15) || (((uintptr_t)q) & 7)) return VITTF_ERR_INVALID_ARG;
  const int64_t lanes = (nvox + 3) / 4;
  hipLaunchKernelGGL(render_prepare_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, volume, nvox,
                     vmin, vmax - vmin, q);
  return vittf_check_launch();
}

extern "C" size_t vittf_render_occupancy_bytes(int32_t n0, int32_t n1, int32_t n2) {
  if (!render_dims_ok(n0, n1, n2)) return 0;
  return (size_t)((n0 + 7) / 8) * ((n1 + 7) / 8) * ((n2 + 7) / 8);
}

extern "C" int vittf_render_occupancy(const uint16_t* q, int32_t n0, int32_t n1, int32_t n2, const float* table, const uint8_t* maps,
                                      int32_t classes, int32_t m0, int32_t m1, int32_t m2, const int32_t* lo_host, uint8_t* occ,
                                      void* stream) {
  if (!q || !table || !occ || !render_dims_ok(n0, n1, n2) || (((uintptr_t)q) & 1) || (((uintptr_t)table) & 15))
    return VITTF_ERR_INVALID_ARG;
  if (!render_classes_ok(maps, classes, m0, m1, m2, lo_host, nullptr)) return VITTF_ERR_INVALID_ARG;
  OccParams P = {};
  P.q = q, P.table = reinterpret_cast<const float4*>(table), P.maps = maps, P.occ = occ, P.classes = classes;
  const int n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
  for (int a = 0; a < 3; ++a) P.n[a] = n[a], P.m[a] = classes ? m[a] : 0, P.nb[a] = (n[a] + 7) / 8;
  for (int k = 0; k < classes; ++k) P.lo[k] = lo_host[k];
  const size_t bricks = vittf_render_occupancy_bytes(n0, n1, n2);
  hipLaunchKernelGGL(render_occupancy_kernel, dim3((unsigned)bricks), dim3(64), 0, (hipStream_t)stream, P);
  return vittf_check_launch();
}

extern "C" int vittf_render(const uint16_t* q, int32_t n0, int32_t n1, int32_t n2, const float* spacing_host, const float* table,
                            const uint8_t* maps, int32_t classes, int32_t m0, int32_t m1, int32_t m2, const int32_t* lo_host,
                            const int32_t* hi_host, const float* class_rgbs_host, const uint8_t* occ, const float* camera_host,
                            int32_t width, int32_t height, float dt, const float* shade_host, float* rgba_out, void* stream) {
  if (!q || !table || !spacing_host || !camera_host || !shade_host || !rgba_out || !render_dims_ok(n0, n1, n2))
    return VITTF_ERR_INVALID_ARG;
  if ((((uintptr_t)q) & 1) || (((uintptr_t)table) & 15) || (((uintptr_t)rgba_out) & 15)) return VITTF_ERR_INVALID_ARG;
  if (width < 1 || height < 1 || width > VITTF_RENDER_MAX_IMAGE || height > VITTF_RENDER_MAX_IMAGE) return VITTF_ERR_INVALID_ARG;
  if (!render_classes_ok(maps, classes, m0, m1, m2, lo_host, hi_host) || (classes > 0 && (!hi_host || !class_rgbs_host)))
    return VITTF_ERR_INVALID_ARG;
  if (!finite_all(spacing_host, 3) || !finite_all(camera_host, 18) || !finite_all(shade_host, 3) || !isfinite(dt) || !(dt > 0.f))
    return VITTF_ERR_INVALID_ARG;
  if (!(shade_host[0] >= 0.f) || !(shade_host[1] >= 0.f) || !(shade_host[2] > 0.f)) return VITTF_ERR_INVALID_ARG;
  if (classes > 0 && !finite_all(class_rgbs_host, 4 * classes)) return VITTF_ERR_INVALID_ARG;
  for (int k = 0; k < classes; ++k)
    if (!(class_rgbs_host[4 * k + 3] >= 0.f)) return VITTF_ERR_INVALID_ARG;
  const int n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
  // the farthest lattice sample: no ray origin is farther from the eye than |ox| + |oy|, no point of the grown box farther
  // from the box's near corner than its diagonal
  double reach = 0.0, fwd2 = 0.0, diag = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (!(spacing_host[a] > 0.f) || !isfinite((float)n[a] * spacing_host[a])) return VITTF_ERR_INVALID_ARG;
    const double ext = ((double)n[a] + 1.0) * spacing_host[a];
    diag += ext * ext;
    double far = 0.0;
    for (int k = 0; k < 3; ++k) far += fabs((double)camera_host[3 * k + a]);            // eye, ox, oy
    far += 0.5 * spacing_host[a];
    reach += (far + ext) * (far + ext);
    fwd2 += (double)camera_host[9 + a] * camera_host[9 + a];
  }
  if (!(fwd2 > 0.0) || !((sqrt(reach) + sqrt(diag)) / dt < RENDER_MAX_STEPS)) return VITTF_ERR_INVALID_ARG;
  RenderParams P = {};
  P.q = q, P.table = reinterpret_cast<const float4*>(table), P.maps = maps, P.occ = occ, P.out = reinterpret_cast<float4*>(rgba_out);
  P.classes = classes, P.width = width, P.height = height, P.dt = dt;
  P.ka = shade_host[0], P.kd = shade_host[1], P.eps = shade_host[2];
  for (int a = 0; a < 3; ++a) {
    P.n[a] = n[a], P.m[a] = classes ? m[a] : 0, P.nb[a] = (n[a] + 7) / 8;
    P.s[a] = spacing_host[a], P.box[a] = (float)n[a] * spacing_host[a];
    P.eye[a] = camera_host[a], P.ox[a] = camera_host[3 + a], P.oy[a] = camera_host[6 + a];
    P.fwd[a] = camera_host[9 + a], P.dx[a] = camera_host[12 + a], P.dy[a] = camera_host[15 + a];
  }
  for (int k = 0; k < classes; ++k) {
    P.lo[k] = lo_host[k], P.range[k] = (float)(hi_host[k] - lo_host[k]);
    for (int e = 0; e < 4; ++e) P.rgbs[k][e] = class_rgbs_host[4 * k + e];
  }
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(RENDER_THREADS), 0,
                     (hipStream_t)stream, P);
  return vittf_check_launch();
}
