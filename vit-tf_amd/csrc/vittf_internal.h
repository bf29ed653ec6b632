// Host functions with C++ linkage that one .hip defines and another calls (the C ABI is include/vittf.h), and the host
// helpers more than one file needs.  Definers include it too, so a signature cannot drift from its callers.
#pragma once
#include "vittf_common.h"

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the linears: which kernel takes a shape is decided by these predicates alone (dispatch: gemm.hip) ----
// Bytes of a [rows - dropped rows][d] 16-bit K-feature output: `drop` leading rows of every whole slice of `tokens` rows go.
static inline int64_t vittf_kfeat_out_bytes(int64_t rows, int32_t d, int32_t tokens, int32_t drop) {
  return (rows - rows / tokens * drop) * (int64_t)d * 2;
}

// gemm_rows.hip: the whole-row residual kernel (x += a . w^T + bias, optionally the LayerNorm behind it)
bool vittf_gemm_rows_covers(int32_t n, int32_t k, int64_t rows);
int vittf_gemm_rows(const void* a, const void* w, const float* bias, float* x, int64_t rows, int32_t n, int32_t k,
                    int32_t dtype, const float* ln_g, const float* ln_b, float ln_eps, void* h, hipStream_t st);

// gemm_pp.hip: the persistent 256 x 256 kernel.  It covers a linear with `columns` output columns (of one third, for the
// K-feature thirds) when both predicates hold; kfeat_bytes = vittf_kfeat_out_bytes of a K-feature output, else 0.
bool vittf_gemm_pp_covers(int32_t k, int32_t columns, const void* a, const void* w);
bool vittf_gemm_pp_covers_out(const void* out, int64_t kfeat_bytes);
int vittf_gemm_pp(const void* a, const void* w, const float* bias, void* out, int64_t rows, int32_t n, int32_t k,
                  int32_t epilogue, int32_t tokens, int32_t dtype, hipStream_t st);
int vittf_gemm_pp_kfeat_parts(const void* a, const void* w, const float* bias, int64_t rows, int32_t d, int32_t k,
                              int32_t tokens, int32_t n_reg, int32_t part_mask, void* const outs[3], int32_t dtype,
                              hipStream_t st, int32_t* taken);

// attention_pp64.hip: attention on pre-scaled q (entry point: attention.hip)
int vittf_attention_pp64(const void* qkv, void* out, int32_t batch, int32_t tokens, int32_t heads, int32_t dtype,
                         hipStream_t st);

// sim_mfma.hip: the matrix-core class maps of similarity.hip, which decides the kernel form (sim_route.h)
enum SimAccum : int;
size_t vittf_sim_mfma_workspace_bytes(int32_t classes, int32_t annotations);
int vittf_sim_mfma_maps(SimAccum form, int cus, const unsigned short* feat, int32_t f, int64_t nvox, const float* qf,
                        const int32_t* class_start_host, int32_t classes, const float* voxel_norm, float* sim, unsigned* maxbits,
                        void* ws, hipStream_t st);
