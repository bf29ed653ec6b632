// Token facet output: the model's final LayerNorm over the patch-token rows of the fp32 residual stream, written as the
// compact fp16 [batch][f0*f1][D] tensor the K-feature epilogue writes for the hooked thirds.
//
// Replaces x_norm_patchtokens of the DINOv2 / DINOv3 forward (get_intermediate_layers(norm=True); last_hidden_state[:, 1 + R:]
// in transformers): norm(x)[:, 1 + R:].  It reads the residual stream X itself, not the 16-bit H a fused LayerNorm leaves
// behind, so a bf16 engine does not round through bf16 first and every width takes the same path; the result is rounded once,
// to fp16, whatever the MFMA operand type.  HBM-bound: one wave per output row, the row stays in registers between the two
// statistics passes (layernorm.hip's idiom: float4 loads, mean, then centred variance -- biased, as nn.LayerNorm), 8-byte
// stores.  The `prefix` = 1 + register-token rows at the head of every slice (CLS, registers) are never read.
#include "vittf_common.h"

namespace {

constexpr int TO_MAX_V4 = 4;  // float4 per lane -> D <= 1024

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__global__ __launch_bounds__(256) void token_out_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, unsigned short* __restrict__ y,
                                                        int64_t out_rows, int npatch, int prefix, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t orow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (orow >= out_rows) return;
  const int64_t slice = orow / npatch;
  const int64_t row = slice * (npatch + prefix) + prefix + (orow - slice * npatch);   // row of X: the slice's prefix skipped
  const int nv = d >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + row * d);
  float4 v[TO_MAX_V4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < TO_MAX_V4; ++i) {
    const int idx = lane + 64 * i;
    if (idx < nv) {
      v[i] = xr[idx];
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < TO_MAX_V4; ++i) {
    const int idx = lane + 64 * i;
    if (idx < nv) {
      const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
      q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  uint2* yr = reinterpret_cast<uint2*>(y + orow * d);
#pragma unroll
  for (int i = 0; i < TO_MAX_V4; ++i) {
    const int idx = lane + 64 * i;
    if (idx < nv) {
      const float4 gg = g4[idx], bb = b4[idx];
      uint2 pk;
      pk.x = pack2_h16<VITTF_FP16>((v[i].x - mean) * rstd * gg.x + bb.x, (v[i].y - mean) * rstd * gg.y + bb.y);
      pk.y = pack2_h16<VITTF_FP16>((v[i].z - mean) * rstd * gg.z + bb.z, (v[i].w - mean) * rstd * gg.w + bb.w);
      yr[idx] = pk;
    }
  }
}

}  // namespace

extern "C" int vittf_token_features(const float* x, const float* norm_g, const float* norm_b, uint16_t* t_out, int32_t batch,
                                    int32_t tokens, int32_t prefix, int32_t d, float eps, void* stream) {
  if (!x || !norm_g || !norm_b || !t_out || batch <= 0 || prefix < 1 || tokens <= prefix || d <= 0 || (d & 3) ||
      d > 256 * TO_MAX_V4 || !(eps > 0.f))
    return VITTF_ERR_INVALID_ARG;
  // float4 loads of x / norm_g / norm_b and 8-byte stores of t_out (rows are d * 4 and d * 2 bytes: multiples of 16 and 8)
  if (((uintptr_t)x & 15) || ((uintptr_t)norm_g & 15) || ((uintptr_t)norm_b & 15) || ((uintptr_t)t_out & 7))
    return VITTF_ERR_INVALID_ARG;
  const int npatch = tokens - prefix;
  const int64_t out_rows = (int64_t)batch * npatch;
  const int64_t blocks = (out_rows + 3) / 4;
  if (blocks > 0x7fffffff) return VITTF_ERR_INVALID_ARG;
  hipLaunchKernelGGL(token_out_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, norm_g, norm_b,
                     (unsigned short*)t_out, out_rows, npatch, (int)prefix, (int)d, eps);
  vittf_note_kernel(VITTF_KERNEL_LAYERNORM, "token_out_kernel");
  return vittf_check_launch();
}
