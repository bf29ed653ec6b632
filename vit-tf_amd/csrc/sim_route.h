// Which kernels a similarity call runs, decided in one place: the switches, the two route functions and the chunk walk of
// the VALU kernels.  Host only, no HIP: similarity.hip and sim_mfma.hip launch what these functions say, and
// tools/micro/sim_route_host.cpp drives them on the CPU (tests/test_sim_route_cpu.py).
#pragma once
#include <stdint.h>
#include <stdlib.h>

constexpr int ACH = 16;        // annotations per pass of the VALU kernels over the volume
constexpr int MAXC = 8;        // classes handled by one such pass (more classes: several launches)
constexpr int SM_MIN_A = 8;    // matrix-core kernels: fewer annotations go to the VALU kernels (VITTF_SIM_MFMA_MIN overrides),
constexpr int SM_F = 384;      //   features per unit (F = 384: one unit, F = 768: two),
constexpr int SM_VOX = 256;    //   voxels of a workgroup tile (two voxel blocks per wave: 512)
constexpr int SM_MAXC = 32;    //   classes of the by-value class table (more: device tables filled by copies)

struct SimChunk {
  int n_ann;          // annotations in this chunk (<= ACH)
  int cls[ACH];       // class of each annotation, relative to c0 (padding: -1)
  int c0, nc;         // classes [c0, c0 + nc) are touched by this chunk
  int first[MAXC];    // chunk holds the first annotations of that class -> overwrite instead of accumulate
  int last[MAXC];     // chunk holds the last annotations of that class  -> finalise (mean, max)
  float count[MAXC];    // annotations of that class (fp32, exact)
};

// The chunk of the annotation list that starts at a0 < class_start[classes]: up to ACH annotations of up to MAXC consecutive
// classes.  Returns its length.
inline int sim_next_chunk(const int32_t* class_start, int classes, int a0, SimChunk* ch) {
  const int total_a = class_start[classes];
  int c_first = 0;
  while (class_start[c_first + 1] <= a0) ++c_first;
  ch->c0 = c_first;
  int n = 0, c = c_first;
  while (n < ACH && a0 + n < total_a) {
    while (class_start[c + 1] <= a0 + n) ++c;
    if (c - c_first >= MAXC) break;
    ch->cls[n] = c - c_first;
    ++n;
  }
  ch->n_ann = n;
  for (int i = n; i < ACH; ++i) ch->cls[i] = -1;
  ch->nc = ch->cls[n - 1] + 1;
  for (int i = 0; i < MAXC; ++i) { ch->first[i] = ch->last[i] = 0; ch->count[i] = 1.f; }
  for (int i = 0; i < ch->nc; ++i) {
    const int cc = c_first + i;
    ch->first[i] = class_start[cc] >= a0;
    ch->last[i] = class_start[cc + 1] <= a0 + n;
    ch->count[i] = (float)(class_start[cc + 1] - class_start[cc]);
  }
  return n;
}

// The environment switches, read once per entry call and never latched: the tests and tools change them
// inside a process.
struct SimSwitches {
  int mfma = 1;             // VITTF_SIM_MFMA        0: never the matrix-core kernels
  int mfma_min = SM_MIN_A;  // VITTF_SIM_MFMA_MIN    annotations from which they are used
  int mfma_vb = 0;          // VITTF_SIM_MFMA_VB     voxel blocks per wave: 1, anything else 2; unset (0): by size
  int split = 1;            // VITTF_SIM_SPLIT       0: always the one-wave-per-voxel-pair VALU kernel
  int quant16 = 1;          // VITTF_SIM_QUANT16     0: bytewise quantise kernel, 2: the general 16-value form
};
inline SimSwitches sim_switches_from_env() {
  SimSwitches s;
  const auto read = [](const char* name, int* v) { const char* e = getenv(name); if (e) *v = atoi(e); return e != nullptr; };
  read("VITTF_SIM_MFMA", &s.mfma);
  read("VITTF_SIM_MFMA_MIN", &s.mfma_min);
  if (read("VITTF_SIM_MFMA_VB", &s.mfma_vb)) s.mfma_vb = s.mfma_vb == 1 ? 1 : 2;
  read("VITTF_SIM_SPLIT", &s.split);
  read("VITTF_SIM_QUANT16", &s.quant16);
  return s;
}

// ---- accumulation: fp32 class maps from the volume and the queries
enum SimAccum : int { SIM_MFMA_FEW, SIM_MFMA_768, SIM_MFMA_VB2, SIM_MFMA_DMA, SIM_MFMA_STRIDED, SIM_VALU_SPLIT, SIM_VALU };
struct SimRoute { SimAccum form; const char* name; };   // name: what vittf_profiler_kernel_name reports

// whole-row LDS-DMA needs 16-byte aligned feature rows
inline bool sim_rows_aligned(uintptr_t feat, int64_t nvox) { return nvox % 8 == 0 && nvox >= 8 && (feat & 15) == 0; }

// Do the matrix-core kernels take the call?  mode 0 on an fp16 volume of 384 or 768 features, enough annotations, and a
// workspace of vittf_sim_mfma_workspace_bytes (mfma_ws).  768-wide rows need the LDS-DMA: their strided-load form has no
// registers left.
inline bool sim_mfma_takes(int f, int64_t nvox, int total_a, bool half, int mode, uintptr_t feat, bool mfma_ws, const SimSwitches& sw) {
  if (!sw.mfma || mode != 0 || !half || !mfma_ws || total_a < sw.mfma_min) return false;
  return f == SM_F || (f == 2 * SM_F && sim_rows_aligned(feat, nvox));
}

// cus: compute units of the current device (only read when sim_mfma_takes)
inline SimRoute sim_route_accumulate(int f, int64_t nvox, const int32_t* class_start, int classes, bool half, int mode,
                                     uintptr_t feat, bool mfma_ws, int cus, const SimSwitches& sw) {
  if (sim_mfma_takes(f, nvox, class_start[classes], half, mode, feat, mfma_ws, sw)) {
    const bool dma = sim_rows_aligned(feat, nvox);
    // the interactive query: one class and one 32-query chunk; the kernel prepares the queries itself
    if (dma && f == SM_F && classes == 1 && class_start[1] <= 32) return {SIM_MFMA_FEW, "sim_mfma_few_kernel"};
    if (f == 2 * SM_F) return {SIM_MFMA_768, "sim_mfma_kernel<F 768>"};
    if (!dma) return {SIM_MFMA_STRIDED, "sim_mfma_kernel"};
    // two voxel blocks per wave (512-voxel workgroups) only when that still fills the chip
    const int vb = sw.mfma_vb ? sw.mfma_vb : ((nvox + 2 * SM_VOX - 1) / (2 * SM_VOX) >= cus ? 2 : 1);
    return vb == 2 ? SimRoute{SIM_MFMA_VB2, "sim_mfma_kernel<2 voxel blocks>"} : SimRoute{SIM_MFMA_DMA, "sim_mfma_kernel"};
  }
  // split-feature kernel when the shapes allow its 8- / 16-byte loads
  if (sw.split && f % 4 == 0 && nvox % 4 == 0 && (feat & 15) == 0) return {SIM_VALU_SPLIT, "sim_accumulate_split"};
  return {SIM_VALU, "sim_accumulate"};
}

// ---- quantise + nearest resize of the maps [classes][.][.][n2] to uint8 [classes][o0][o1][o2]
enum SimQuant : int { SIM_QUANT_BYTES, SIM_QUANT_16, SIM_QUANT_POW2 };
struct SimQuantRoute { SimQuant form; int shift; };   // shift: log2(o2 / n2) of the power-of-two form, else 0

inline SimQuantRoute sim_route_quantize(int classes, int n2, int o0, int o1, int o2, uintptr_t sim, uintptr_t out, const SimSwitches& sw) {
  const int64_t total_out = (int64_t)classes * o0 * o1 * o2;
  // 16 values of one output row per thread, index arithmetic in 31 bits
  if (sw.quant16 == 0 || o2 % 16 != 0 || (out & 15) != 0 || total_out / 16 >= 0x7fffffff || (int64_t)classes * o0 * o1 >= 0x7fffffff)
    return {SIM_QUANT_BYTES, 0};
  const int r2 = o2 % n2 == 0 ? o2 / n2 : 0;
  for (int sh = 0; sh <= 4; ++sh)
    if (sw.quant16 == 1 && r2 == 1 << sh && (sim & 15) == 0 && n2 % (16 / r2) == 0 && ((int64_t)n2 * 4) % 16 == 0) return {SIM_QUANT_POW2, sh};
  return {SIM_QUANT_16, 0};
}
