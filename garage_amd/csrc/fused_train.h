// Entry points of the fused optimizer-step kernels and of the MLP layer ranges they
// combine with (mlp_layers.cpp), used by the epoch loop (update.cpp).  The entry points
// are host C++ (fused_train_host.cpp: argument checks, kernel choice, grids, the weight-
// plane cache); they fill the kernels' parameter structs (fused_params.h) and hand them
// to the launch seam of fused_train.hip, which holds the device code.  The shape rules
// (ga_fused_tiles, ga_fused_width_ok, ga_fused_first_layer_ok, ga_fused_pair_supported,
// ga_narrow_step_supported, ga_narrow_step_stride) are shape_rules.h's.
// Not part of the C ABI: ga_update_epoch* is what callers see.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shape_rules.h"

struct ga_fused_loss_args {
  int kind;                  // 0 Gaussian policy, 1 value NLL, 2 categorical policy
  const float* actions; int64_t lda;
  const float* old_ll; const float* adv; const float* returns;
  const int32_t* idx;        // minibatch row m is sample idx[m] (null: m)
  const float* log_std; int has_min, has_max; float min_log_std, max_log_std;
  int A;                     // head width
  int algo; float clip; float ent_coeff; int ent_flags;
  int double_softmax;
};

struct ga_fused_region {
  int64_t beg, n;            // flat parameter range [beg, beg + n)
  const float* src;          // partial 0 of element 0
  int64_t stride;            // floats between partials
  int n_part;
};

extern "C" {
// The layer under the last hidden one when that is the network's FIRST layer and
// the kernel is to produce its outputs itself (H = tanh(X W^T + b), X gathered
// through loss->idx) instead of reading them: in_w <= 32, K * round4(in_w) <=
// ga_fused_first_layer_ok's bound.  H is written too (the backward pass reads it).
typedef struct ga_fused_first_layer {
  const float* X;
  int64_t ldx;
  const float* W;  // [K][round4(in_w)]
  const float* b;  // [K]
  int in_w;
  float* H;        // [M][ldh]
  int64_t ldh;
} ga_fused_first_layer;
// The whole MLP (two hidden tanh layers of the shapes above, <= 8 linear outputs) for
// its OUTPUTS only: out[m] = MLP(X[idx ? idx[m] : m]); no activation reaches memory.
int ga_fused_eval_supported(int n_layers, const int* dims);
int ga_fused_eval_forward(const float* X, int64_t ldx, const int32_t* idx, int64_t M,
                          const int* dims, const float* W1, const float* b1,
                          const float* W2, const float* b2, const float* Wh,
                          const float* bh, float* out, int64_t ldo, hipStream_t stream);
// narrow_step.hip: forward + loss + backward of a 2 x H network (H = 32 or 64) in one
// launch; part: [tiles][ga_narrow_step_stride] floats, lpart: [tiles][2] doubles
int ga_narrow_train_step(const float* params, const int64_t* w_off, const int64_t* b_off,
                         int in_w, int H, int out_w, const float* X, int64_t ldx,
                         int64_t M, const ga_fused_loss_args* loss, float* part,
                         double* lpart, hipStream_t stream);
// ---- The four launches of a fused optimizer step.  Each takes one descriptor per
// network: n_nets = 1, or 2 for the policy's and the value function's step k in ONE
// grid (same shapes and row count for both; ga_fused_pair_supported: width 256, first
// layer in the kernel).  update.cpp (fused_step) fills the descriptors.
//
// 1. last hidden layer + head + loss + gradient seed + head weight-gradient shares;
// hpart: [tiles][8 * width + 8] floats, lpart: [tiles][2] doubles.  first != null:
// A / lda / a_idx are ignored, the operand comes from `first`
typedef struct ga_fused_fwd_net {
  const float* A; int64_t lda; const int32_t* a_idx;
  const float* W; int64_t ldw; const float* bias;
  const float* head_W; int64_t head_ldw; const float* head_bias;
  const ga_fused_loss_args* loss;
  float* dZ; int64_t lddz; float* hpart; double* lpart;
  const ga_fused_first_layer* first;
} ga_fused_fwd_net;
int ga_fused_fwd_head_loss(const ga_fused_fwd_net* nets, int n_nets, int64_t M, int width,
                           int K, hipStream_t stream);
// 2. mlp_layers.cpp: the weight-gradient GEMM of the middle layer (dW2 = dZ2^T H1, split-K
// slabs + bias column sums) of a 3-layer network: the launch ga_mlp_backward_range_f32
// makes for layer 1 with fused_first = 1.  n_nets = 2 only: one network's middle layers,
// of any depth, go through ga_mlp_backward_range_f32
typedef struct ga_wgrad_mid_net {
  const float* dz; const float* in; float* slabs_w; float* slabs_b; int64_t slab_stride;
} ga_wgrad_mid_net;
int ga_wgrad_mid(const ga_wgrad_mid_net* nets, int n_nets, int64_t M, int64_t n_splits,
                 int out_w, int in_w, hipStream_t stream);
// 3. data gradient into the first hidden layer + first-layer weight / bias gradient
// shares; wpart: [tiles][width * round4(in_w) + width] floats.
// sum_w / sum_b (src != null): split-K slabs that the launch BEFORE this one on the same
// stream wrote and that this launch sums on the side -- n elements (a multiple of 4),
// partial k of element e at src[k * stride + e]; every element's sum, in the order
// reduce_regions_adam_kernel gives a region of <= 128 partials, replaces its partial 0.
// Two ranges of one launch share stride and n_part and lie within 2^30 floats of each
// other, partials included.
typedef struct ga_slab_range {
  float* src; int64_t n; int64_t stride; int n_part;
} ga_slab_range;
typedef struct ga_fused_dgrad_net {
  const float* dZ2; int64_t lddz; const float* W2; int64_t ldw;
  const float* H1; int64_t ldh; const float* X; int64_t ldx; const int32_t* idx;
  float* wpart;
  ga_slab_range sum_w, sum_b;
} ga_fused_dgrad_net;
int ga_fused_dgrad_wgrad0(const ga_fused_dgrad_net* nets, int n_nets, int64_t M, int width,
                          int K, int in_w, hipStream_t stream);
// 1 + 3 in ONE launch, one network: every workgroup runs launch 1's body and then launch
// 3's on the same 64 rows, dZ2 staying in LDS between them (it is still written once,
// for launch 2, which now runs AFTER this one: `dgrad` carries no slab ranges).
// ga_fused_fwd_dgrad_supported: two hidden layers of the same width (width == K), first
// layer in the kernel.  `dgrad` must describe the step `fwd` describes.
int ga_fused_fwd_dgrad_supported(int width, int K, int in_w);
int ga_fused_fwd_dgrad(const ga_fused_fwd_net* fwd, const ga_fused_dgrad_net* dgrad,
                       int64_t M, int width, int K, hipStream_t stream);
// 4. partial sums -> gradient -> Adam, and the loss.  pl_rows > 0 (one network only):
// the launch also rewrites the split-operand planes of the [pl_rows][pl_cols] weight
// matrix at flat index pl_beg, when the step's forward launch used them;
// ga_planes_epoch_begin: planes written that way are trusted only until the epoch
// call that wrote them returns.
// presummed, bit k: partial 0 of region k already holds the sum of all its partials
// (ga_fused_dgrad_net::sum_w / sum_b); the launch reads nothing else of that region.
typedef struct ga_reduce_net {
  const ga_fused_region* regions; int n_regions;
  float* params; float* grads; float* exp_avg; float* exp_avg_sq;
  int64_t step; double lr, beta1, beta2, eps; float scale; int do_adam, zero_slot0;
  const double* lpart; int n_lpart; int64_t M; const ga_fused_loss_args* loss;
  float* loss_out;
  int64_t pl_beg; int pl_rows, pl_cols;
  uint32_t presummed;
} ga_reduce_net;
int ga_reduce_regions_adam(const ga_reduce_net* nets, int n_nets, hipStream_t stream);
void ga_planes_epoch_begin(void);
/* 1 while the opt-in split-operand (3 x bf16) k-loops are selected
 * (ga_set_split_bf16 / GARAGE_AMD_SPLIT_BF16=1). */
int ga_split_bf16_enabled(void); /* ... for the weight-gradient GEMM */
int ga_split_bf16_any(void);     /* ... for any kernel */
int ga_split_bf16_gemm(void);    /* ... for the per-layer forward / data-gradient GEMMs */
/* W [rows][ld] (cols valid) as the B operand of a split-operand k-loop: three bf16
 * planes in fragment order (fused_train.hip: split_planes_kernel), both dimensions
 * padded to multiples of 32; bwd = 0: B(k, n) = W[n][k], 1: B(k, n) = W[k][n].
 * Recomputed by every call, on `stream`; plane pl at + pl * round32(rows) *
 * round32(cols). */
const uint16_t* ga_weight_planes(const float* W, int64_t ld, int rows, int cols, int bwd,
                                 hipStream_t stream);
}
