// What the host says to the stand-alone loss, statistics and optimizer kernels
// (losses.hip) about one launch, and the launch seam that takes it.  Host C++ only (no
// device code), in the style of fused_params.h and rollout_params.h: the host side
// (losses_host.cpp) checks the C-ABI arguments, fills these structs and chooses the grid,
// the dynamic LDS size and one launch or two, the seam instantiates and launches -- so
// that the host side builds for the CPU harness under tests/host
// (losses_host_harness.cpp) against fakes of the seam.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "loss_args.h"
#include "shape_rules.h"

struct PpoLossParams {
  const float* mean;      // [M, ldm] policy means of the minibatch rows
  int64_t ldm;
  const float* actions;   // [*, lda] gathered through idx (or row i when null)
  int64_t lda;
  const float* old_ll;    // gathered through idx
  const float* adv;       // gathered through idx
  const int32_t* idx;
  const float* log_std;   // device scalar parameter (unclamped)
  float min_log_std;      // lower clamp, applied when has_min
  int has_min;
  float max_log_std;
  int has_max;
  int64_t M;
  int A;
  int algo;               // 0 PPO clipped surrogate, 1 VPG (ll * adv),
                          // 2 TRPO unclipped surrogate (ratio * adv)
  float clip;
  LossEnt ent;
  float* dmean;           // optional [M, ldm]: dLoss/dmean (already / M)
  float* ll_out;          // optional [M]: new log-likelihoods
  double* partials;       // [gridDim.x][2]: sum objective, sum dLoss/dlog_std * M
  // the scalars of the batch (written by the last block to finish)
  float* loss_out;        // null: a finalize launch follows
  float* grad_slab0;
  int64_t slab_stride, n_splits;
  unsigned* ticket;
};

struct PpoFinalizeParams {
  const double* partials;
  int nblocks;
  const float* log_std;
  float min_log_std, max_log_std;
  int has_min, has_max;
  int64_t M;
  int A;
  LossEnt ent;
  float* loss_out;      // scalar
  float* grad_slab0;    // optional: slot that receives dLoss/dlog_std
  int64_t slab_stride;  // the same slot of slabs 1..n_splits-1 is zeroed
  int64_t n_splits;
};

// ---- categorical policy head ---------------------------------------------------
// The reference has no torch CategoricalMLPPolicy; its torch categorical (CNN)
// policies feed softmax(net(x)) to Categorical(logits=...)
// (torch/policies/categorical_cnn_policy.py:138-139).
// double_softmax = 1 keeps that convention, 0 treats the MLP output as logits.
struct CatLossParams {
  const float* scores;   // [M, lds] MLP outputs of the minibatch rows
  int64_t lds;
  const float* actions;  // [*, lda] column 0 holds the class id (as float)
  int64_t lda;
  const float* old_ll;
  const float* adv;
  const int32_t* idx;
  int64_t M;
  int A;
  int double_softmax;
  int algo;
  float clip;
  LossEnt ent;
  float* dscores;        // optional [M, lds]: dLoss/dscores (already / M)
  float* ll_out;         // optional [M]
  float* ent_out;        // optional [M]: per-row entropy (after softplus if set)
  double* partials;      // [gridDim.x][2]: sum objective, sum entropy
  // the scalars of the batch (written by the last block to finish)
  float* loss_out;       // null: a finalize launch follows
  double* ent_sum_out;
  float* grad_slab0;
  int64_t slab_stride, n_splits;
  unsigned* ticket;
};

struct NllParams {
  const float* v;        // [M, ldv], value in column 0
  int64_t ldv;
  const float* returns;  // gathered through idx
  const int32_t* idx;
  const float* log_std;  // device scalar, no clamp (min_std=None, max_std=None)
  int64_t M;
  float* dv;             // optional [M, ldv] column 0
  double* partials;      // [gridDim.x][2]
  float* loss_out;       // written by the last block; null: a finalize launch follows
  float* grad_slab0;
  int64_t slab_stride, n_splits;
  unsigned* ticket;
};

struct AdamParams {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  GaAdam c;
};

// ---------------------------------------------------------------------------
// Optimizers other than the default Adam (make_optimizer, _functions.py:25-65,
// builds any torch.optim class): elementwise steps over the flat parameter buffer
// with torch's single-tensor arithmetic, one rounding per torch operation.  Every
// scalar torch forms in Python before it reaches a tensor -- 1 - beta1, 1 - beta2,
// 1 - alpha, 1 - dampening, 1 - lr * weight_decay, -lr / bias_correction1,
// sqrt(bias_correction2), -lr -- is formed on the host from the doubles in h and
// rounded to fp32 once, as ga_adam_coeffs does (1.f - 0.999f is 1.3e-5 away from
// float(1 - 0.999)); the kernel never subtracts two rounded constants.  addcdiv
// is x + (value * t1) / t2, as in ga_adam_update and torch's elementwise kernels.
//   kind 1  torch.optim.SGD      h = {lr, momentum, dampening, weight_decay};
//                                flag bit 0 nesterov; s1 = momentum buffer
//   kind 2  torch.optim.RMSprop  h = {lr, alpha, eps, weight_decay, momentum};
//                                flag bit 0 centered; s1 = square_avg, s2 = momentum
//                                buffer, s3 = grad_avg
//   kind 3  torch.optim.Adam / AdamW beyond the defaults
//                                h = {lr, beta1, beta2, eps, weight_decay};
//                                flag bit 0 amsgrad, bit 1 decoupled decay (AdamW);
//                                s1 = exp_avg, s2 = exp_avg_sq, s3 = max_exp_avg_sq
struct OptParams {
  float* p;
  const float* g;
  float* s1;
  float* s2;
  float* s3;
  int64_t n;
  int kind, flags, first;  // first: step == 1 (SGD initialises its buffer with g)
  float neg_lr, h1, h2, h3, h4;
  // derived in double, rounded once (ga_optimizer_step_f32)
  float w1;     // 1 - dampening (kind 1), 1 - alpha (kind 2), 1 - beta1 (kind 3)
  float w2;     // 1 - beta2 (kind 3)
  float decay;  // 1 - lr * weight_decay (AdamW)
  float neg_step_size, bc2_sqrt;  // kind 3
};

// The network's last linear layer, computed inside the loss kernel
struct HeadLayer {
  const float* H;       // [M, ldh] last hidden activations (minibatch rows)
  int64_t ldh;
  const float* W;       // [A][ldw], k contiguous
  int64_t ldw;
  const float* bias;    // [A]
  int K;                // hidden width, a multiple of 64
  float* out;           // optional [M, ldo] head outputs
  int64_t ldo;
};

// ---- losses.hip: the launch seam, one function per kernel family.  Each does nothing
// but launch on `stream` (and, where it says so, choose the instantiation from a value
// the host passes): `blocks` workgroups of the kernel's own thread count -- 256; one wave
// for a finalize, which is always one workgroup; LS_DOT_THREADS for the dot product,
// HL_THREADS for the head kernels.
void ls_launch_ppo_gaussian_loss(const PpoLossParams& p, unsigned blocks, hipStream_t stream);
void ls_launch_ppo_gaussian_finalize(const PpoFinalizeParams& f, hipStream_t stream);
void ls_launch_ppo_categorical_loss(const CatLossParams& p, unsigned blocks,
                                    hipStream_t stream);
void ls_launch_ppo_categorical_finalize(const double* partials, int nblocks, int64_t M,
                                        float* loss_out, double* ent_sum_out,
                                        float* grad_slab0, int64_t slab_stride,
                                        int64_t n_splits, hipStream_t stream);
void ls_launch_gaussian_nll(const NllParams& p, unsigned blocks, hipStream_t stream);
void ls_launch_gaussian_nll_finalize(const double* partials, int nblocks, int64_t M,
                                     float* loss_out, float* grad_slab0,
                                     int64_t slab_stride, int64_t n_splits,
                                     hipStream_t stream);
// per-block KL sums -> partials[blocks]; ls_launch_sum_partials adds them up
void ls_launch_categorical_kl(const float* sc_old, const float* sc_new, int64_t ld, int64_t M,
                              int A, int dbl, double* partials, unsigned blocks,
                              hipStream_t stream);
void ls_launch_gaussian_kl(const float* mean_old, const float* mean_new, int64_t ld,
                           int64_t M, int A, float s_old, float s_new, double* partials,
                           unsigned blocks, hipStream_t stream);
void ls_launch_sum_partials(const double* partials, int nblocks, double* out,
                            hipStream_t stream);
void ls_launch_reduce_slabs(const float* slabs, int64_t n_splits, int64_t stride, int64_t n,
                            float* out, float scale, unsigned blocks, hipStream_t stream);
void ls_launch_reduce_adam(const float* slabs, int64_t n_splits, int64_t stride,
                           int zero_slot0, const AdamParams& a, float* grads, unsigned blocks,
                           hipStream_t stream);
void ls_launch_adam(const AdamParams& a, unsigned blocks, hipStream_t stream);
void ls_launch_optimizer_step(const OptParams& a, unsigned blocks, hipStream_t stream);
// the partial launch (`blocks` workgroups) and the finalize launch of statistic `what`
// (0: sum, 1: squared deviations from the mean in stats, 2: min)
void ls_launch_stats(int what, const float* x, int64_t n, double* stats, double* partials,
                     unsigned blocks, hipStream_t stream);
void ls_launch_adv_center(float* x, int64_t n, const double* stats, float eps,
                          unsigned blocks, hipStream_t stream);
void ls_launch_sub_scalar(float* x, int64_t n, const double* scalar, unsigned blocks,
                          hipStream_t stream);
void ls_launch_dot(const float* a, const float* b, int64_t n, double* out, unsigned blocks,
                   hipStream_t stream);
void ls_launch_axpby(float alpha, const float* x, float beta, float* y, int64_t n,
                     unsigned blocks, hipStream_t stream);
void ls_launch_fisher_seed_gaussian(const float* tmean, int64_t ldt, int64_t M, int A,
                                    const float* log_std, int has_min, float min_log_std,
                                    int has_max, float max_log_std, float* dout, int64_t ldd,
                                    unsigned blocks, hipStream_t stream);
void ls_launch_fisher_seed_categorical(const float* scores, int64_t lds, const float* tscores,
                                       int64_t ldt, int64_t M, int A, int double_softmax,
                                       float* dout, int64_t ldd, unsigned blocks,
                                       hipStream_t stream);
// the head kernels: the instantiation is L.K / 64's, lds_bytes the dynamic LDS
void ls_launch_head_ppo_gaussian(const HeadLayer& L, const PpoLossParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t stream);
void ls_launch_head_gaussian_nll(const HeadLayer& L, const NllParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t stream);
