// What the host says to the fp32 MFMA GEMM kernels (gemm.hip, gemm_core.h) about one
// product.  Which kernel takes it, with which grid, and the launch entries are in
// layer_plans.h.  Host C++ only (no device code), so that the per-layer dispatch
// (mlp_layers.cpp) builds for the CPU harness under tests/host as well.  Not part of the
// C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int BK = 32;

enum Epilogue { EPI_BIAS_ACT = 0, EPI_MUL_DTANH = 1, EPI_PLAIN = 2 };

// network code (ga_mlp_desc::hidden_act) -> forward code (GemmParams::act); the codes
// are listed in gemm_core.h
__host__ __device__ inline int act_forward_code(int hidden_act) {
  return hidden_act == 0 ? 1 : (hidden_act == 1 ? 2 : (hidden_act == 2 ? 0 : hidden_act));
}

inline int round4(int v) { return (v + 3) & ~3; }

struct GemmParams {
  const float* A;
  int64_t lda;           // floats between consecutive memory lines of A
  const int32_t* a_idx;  // optional gather applied to A's memory-line index
  const float* B;
  int64_t ldb;
  const int32_t* b_idx;
  float* C;
  int64_t c_rs, c_cs;    // C(m,n) at C[m * c_rs + n * c_cs]
  int M, N, K;
  int epi;
  const float* bias;     // EPI_BIAS_ACT: per-n bias (may be null)
  int act;               // 0 identity, 1 tanh
  const float* H;        // EPI_MUL_DTANH (or EPI_BIAS_ACT with H set): activation
  int64_t ldh;           // outputs H[m * ldh + n]; the result is scaled by the
  int hact;              // activation's slope there (network code, 0 = tanh)
  int accum;             // 1: add the product to what C already holds
  int k_per_split;       // multiple of BK
  int64_t c_split_stride;
  float* colsum;         // optional: sum_k of operand A (or B) -> colsum[line]
  int colsum_of_b;       // 0: columns of A tile (index m), 1: of B tile (index n)
  int64_t colsum_split_stride;
  int gx, gy, gz;        // logical grid (m blocks, n blocks, splits); 1-D launch
  // HEAD kernels (the tile spans all N columns): the next, narrow layer is applied to
  // the staged output rows in the epilogue: head_out[m, j] = head_bias[j] +
  // sum_n C(m, n) * head_W[j * head_ldw + n],  j < head_n <= 8
  const float* head_W;
  int64_t head_ldw;
  const float* head_bias;
  int head_n;
  float* head_out;
  int64_t head_ld;
  // split-operand instantiation (opt-in): the B operand as three bf16 planes in
  // fragment order (fused_train.h: ga_weight_planes), plane pl at + pl * stride,
  // bplane_nblk = round32(N) / 32 column blocks per 16-deep k group
  const uint16_t* bplanes;
  int64_t bplane_stride;
  int bplane_nblk;
};

// Two problems of the same shape in one grid (the policy's and the value function's
// weight-gradient GEMM of one optimizer step): workgroup b takes workgroup b / 2 of
// problem b % 2 (see fwd_head_loss_pair_kernel, fused_train.hip).
struct GemmPair {
  GemmParams a, b;
};
