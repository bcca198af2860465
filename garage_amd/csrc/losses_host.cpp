// The host side of the stand-alone loss, statistics and optimizer kernels (losses.hip):
// every extern "C" entry point -- its argument checks, the kernels' parameter structs,
// the grid, the dynamic LDS size and the choice between one launch and partials +
// finalize.  Host C++ only: the launches go through the seam of loss_params.h, so that
// this file builds for the CPU harness under tests/host (losses_host_harness.cpp) too.
//
//   ga_ppo_gaussian_loss_f32   PPO._compute_objective + VPG._compute_loss_with_adv
//                              (torch/algos/ppo.py:96-132, vpg.py:324-347,408-454)
//                              forward AND the gradient wrt the policy mean /
//                              scalar log-std, in one pass over the minibatch
//   ga_gaussian_nll_loss_f32   GaussianMLPValueFunction.compute_loss
//                              (torch/value_functions/gaussian_mlp_value_function.py:81-98)
//   ga_gaussian_kl_f32         VPG._compute_kl_constraint (vpg.py:381-406)
//   ga_reduce_slabs_f32 / ga_adam_step_f32
//                              OptimizerWrapper.step == torch.optim.Adam.step
//                              (torch/optimizers/optimizer_wrapper.py:53-63)
//   ga_stats_* / ga_adv_center_f32 / ga_sub_scalar_f32
//                              VPG._compute_advantage centring (vpg.py:371-377)
#include "common.h"
#include "loss_params.h"
#include "shape_rules.h"

namespace {

inline int red_blocks(int64_t n) { return ga_red_blocks(n); }  // (shape_rules.h)

// the head kernels: a workgroup's 16-lane groups take HL_ROWS_MAX rows each per pass
inline int head_blocks(int64_t M) {
  int64_t b = ga_ceil_div(M, HL_GROUPS * HL_ROWS_MAX);
  if (b < 1) b = 1;
  if (b > RED_BLOCKS) b = RED_BLOCKS;
  return (int)b;
}
inline unsigned head_lds_bytes(int A, int K) {
  return (unsigned)(ga_head_lds(A, K).floats() * sizeof(float));
}

// A single block always finishes its own launch.  With several blocks the last
// ticket saves the finalize launch but pays two device-scope fences (L2 write-back
// / invalidate across the XCDs) in every block: measured +1 % per C3 iteration
// (146.5 vs 145.1 ms overlapped, 167.4 vs 166.1 ms on one stream) and +2 % at C2,
// so it is off by default.
int g_one_launch_losses = 0;

// How the batch sums of `rows` rows are reduced: nb blocks leave their partials at the
// front of the workspace; one_launch: the loss launch finishes the batch itself (the
// last block to draw the ticket behind the partials), otherwise a finalize launch does.
struct RedPlan {
  int nb;
  bool one_launch;
  unsigned* ticket;
};
RedPlan red_plan(int64_t rows, double* workspace) {
  RedPlan r;
  r.nb = red_blocks(rows);
  r.one_launch = r.nb == 1 || g_one_launch_losses != 0;
  r.ticket = reinterpret_cast<unsigned*>(workspace + 2 * RED_BLOCKS);
  return r;
}
// ... and what a loss launch under the plan is told about the scalars of the batch
template <class P>
void finish_by_plan(P& p, const RedPlan& r, float* loss_out, float* grad_slab0,
                    int64_t slab_stride, int64_t n_splits) {
  p.loss_out = r.one_launch ? loss_out : nullptr;
  p.grad_slab0 = grad_slab0; p.slab_stride = slab_stride; p.n_splits = n_splits;
  p.ticket = r.ticket;
}

// The rows of a Gaussian policy loss, for the plain and the head entry (whose `mean` is
// null: the kernel computes it); the scalars of the batch are left to a finalize launch.
PpoLossParams ppo_loss_params(const float* mean, int64_t ldm, const float* actions,
                              int64_t lda, const float* old_ll, const float* adv,
                              const int32_t* idx, const float* log_std, int has_min,
                              float min_log_std, int has_max, float max_log_std, int64_t M,
                              int A, int algo, float clip, float ent_coeff, int ent_flags,
                              float* dmean, float* ll_out, double* workspace) {
  PpoLossParams p;
  p.mean = mean; p.ldm = ldm; p.actions = actions; p.lda = lda; p.old_ll = old_ll;
  p.adv = adv; p.idx = idx; p.log_std = log_std; p.min_log_std = min_log_std;
  p.has_min = has_min; p.max_log_std = max_log_std; p.has_max = has_max; p.M = M;
  p.A = A; p.algo = algo; p.clip = clip; p.ent = lr_ent(ent_coeff, ent_flags);
  p.dmean = dmean; p.ll_out = ll_out; p.partials = workspace;
  p.loss_out = nullptr; p.grad_slab0 = nullptr; p.slab_stride = 0; p.n_splits = 0;
  p.ticket = nullptr;
  return p;
}
PpoFinalizeParams ppo_finalize_params(const PpoLossParams& p, int nblocks, float* loss_out,
                                      float* grad_slab0, int64_t slab_stride,
                                      int64_t n_splits) {
  PpoFinalizeParams f;
  f.partials = p.partials; f.nblocks = nblocks; f.log_std = p.log_std;
  f.min_log_std = p.min_log_std; f.max_log_std = p.max_log_std; f.has_min = p.has_min;
  f.has_max = p.has_max; f.M = p.M; f.A = p.A; f.ent = p.ent; f.loss_out = loss_out;
  f.grad_slab0 = grad_slab0; f.slab_stride = slab_stride; f.n_splits = n_splits;
  return f;
}
NllParams nll_params(const float* v, int64_t ldv, const float* returns, const int32_t* idx,
                     const float* log_std, int64_t M, float* dv, double* workspace) {
  NllParams p;
  p.v = v; p.ldv = ldv; p.returns = returns; p.idx = idx; p.log_std = log_std;
  p.M = M; p.dv = dv; p.partials = workspace;
  p.loss_out = nullptr; p.grad_slab0 = nullptr; p.slab_stride = 0; p.n_splits = 0;
  p.ticket = nullptr;
  return p;
}
AdamParams adam_params(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       int64_t n, int64_t step, double lr, double beta1, double beta2,
                       double eps) {
  AdamParams a;
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
  a.c = ga_adam_coeffs(lr, beta1, beta2, eps, step);
  return a;
}

}  // namespace

// [RED_BLOCKS][2] partial sums + one slot for the ticket of the single-launch
// reductions / the grid-barrier words of small_step.hip (both leave it zero) + one
// slot whose first word small_step.hip raises when a barrier gave up
extern "C" int64_t ga_reduction_workspace_doubles(void) { return 2 * RED_BLOCKS + 2; }
extern "C" int64_t ga_reduction_partials_doubles(void) { return 2 * RED_BLOCKS; }

extern "C" int ga_set_one_launch_losses(int on) {
  g_one_launch_losses = on != 0;
  return 0;
}

extern "C" int ga_ppo_gaussian_loss_f32(
    const float* mean, int64_t ldm, const float* actions, int64_t lda,
    const float* old_ll, const float* adv, const int32_t* idx, const float* log_std,
    int has_min, float min_log_std, int has_max, float max_log_std, int64_t M, int A,
    int algo, float clip, float ent_coeff, int ent_flags, float* dmean,
    float* ll_out, float* loss_out, float* grad_slab0, int64_t slab_stride,
    int64_t n_splits, double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(mean && actions && adv && log_std && loss_out && workspace,
             "ga_ppo_gaussian_loss_f32: null pointer");
  GA_REQUIRE(algo == 1 || old_ll, "ga_ppo_gaussian_loss_f32: PPO needs old_ll");
  GA_REQUIRE(M > 0 && A > 0 && ldm >= A && lda >= A,
             "ga_ppo_gaussian_loss_f32: bad sizes");
  PpoLossParams p = ppo_loss_params(mean, ldm, actions, lda, old_ll, adv, idx, log_std,
                                    has_min, min_log_std, has_max, max_log_std, M, A, algo,
                                    clip, ent_coeff, ent_flags, dmean, ll_out, workspace);
  const RedPlan r = red_plan(M, workspace);
  finish_by_plan(p, r, loss_out, grad_slab0, slab_stride, n_splits);
  ls_launch_ppo_gaussian_loss(p, (unsigned)r.nb, stream);
  GA_CHECK_LAUNCH("ppo_gaussian_loss");
  if (r.one_launch) return GA_OK;
  ls_launch_ppo_gaussian_finalize(
      ppo_finalize_params(p, r.nb, loss_out, grad_slab0, slab_stride, n_splits), stream);
  GA_CHECK_LAUNCH("ppo_gaussian_finalize");
  return GA_OK;
}

extern "C" int ga_ppo_categorical_loss_f32(
    const float* scores, int64_t lds, const float* actions, int64_t lda,
    const float* old_ll, const float* adv, const int32_t* idx, int64_t M, int A,
    int double_softmax, int algo, float clip, float ent_coeff, int ent_flags,
    float* dscores, float* ll_out, float* ent_out, float* loss_out,
    double* ent_sum_out, float* grad_slab0, int64_t slab_stride, int64_t n_splits,
    double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(scores && actions && adv && loss_out && workspace,
             "ga_ppo_categorical_loss_f32: null pointer");
  GA_REQUIRE(algo == 1 || old_ll, "ga_ppo_categorical_loss_f32: PPO needs old_ll");
  GA_REQUIRE(M > 0 && A > 0 && lds >= A && lda >= 1,
             "ga_ppo_categorical_loss_f32: bad sizes");
  CatLossParams p;
  p.scores = scores; p.lds = lds; p.actions = actions; p.lda = lda;
  p.old_ll = old_ll; p.adv = adv; p.idx = idx; p.M = M; p.A = A;
  p.double_softmax = double_softmax; p.algo = algo; p.clip = clip;
  p.ent = lr_ent(ent_coeff, ent_flags);
  p.dscores = dscores; p.ll_out = ll_out; p.ent_out = ent_out;
  p.partials = workspace; p.ent_sum_out = ent_sum_out;
  const RedPlan r = red_plan(M, workspace);
  finish_by_plan(p, r, loss_out, grad_slab0, slab_stride, n_splits);
  ls_launch_ppo_categorical_loss(p, (unsigned)r.nb, stream);
  GA_CHECK_LAUNCH("ppo_categorical_loss");
  if (r.one_launch) return GA_OK;
  ls_launch_ppo_categorical_finalize(workspace, r.nb, M, loss_out, ent_sum_out, grad_slab0,
                                     slab_stride, n_splits, stream);
  GA_CHECK_LAUNCH("ppo_categorical_finalize");
  return GA_OK;
}

extern "C" int ga_categorical_kl_f32(const float* scores_old, const float* scores_new,
                                     int64_t ld, int64_t M, int A, int double_softmax,
                                     double* kl_sum_out, double* workspace,
                                     ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(scores_old && scores_new && kl_sum_out && workspace,
             "ga_categorical_kl_f32: null pointer");
  GA_REQUIRE(M > 0 && A > 0 && ld >= A, "ga_categorical_kl_f32: bad sizes");
  const int nb = red_blocks(M);
  ls_launch_categorical_kl(scores_old, scores_new, ld, M, A, double_softmax, workspace,
                           (unsigned)nb, stream);
  GA_CHECK_LAUNCH("categorical_kl");
  ls_launch_sum_partials(workspace, nb, kl_sum_out, stream);
  GA_CHECK_LAUNCH("sum_partials");
  return GA_OK;
}

extern "C" int ga_gaussian_nll_loss_f32(const float* v, int64_t ldv,
                                        const float* returns, const int32_t* idx,
                                        const float* log_std, int64_t M, float* dv,
                                        float* loss_out, float* grad_slab0,
                                        int64_t slab_stride, int64_t n_splits,
                                        double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(v && returns && log_std && loss_out && workspace,
             "ga_gaussian_nll_loss_f32: null pointer");
  GA_REQUIRE(M > 0 && ldv >= 1, "ga_gaussian_nll_loss_f32: bad sizes");
  NllParams p = nll_params(v, ldv, returns, idx, log_std, M, dv, workspace);
  const RedPlan r = red_plan(M, workspace);
  finish_by_plan(p, r, loss_out, grad_slab0, slab_stride, n_splits);
  ls_launch_gaussian_nll(p, (unsigned)r.nb, stream);
  GA_CHECK_LAUNCH("gaussian_nll");
  if (r.one_launch) return GA_OK;
  ls_launch_gaussian_nll_finalize(workspace, r.nb, M, loss_out, grad_slab0, slab_stride,
                                  n_splits, stream);
  GA_CHECK_LAUNCH("gaussian_nll_finalize");
  return GA_OK;
}

extern "C" int ga_gaussian_kl_f32(const float* mean_old, const float* mean_new,
                                  int64_t ld, int64_t M, int A, float log_std_old,
                                  float log_std_new, double* kl_sum_out,
                                  double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(mean_old && mean_new && kl_sum_out && workspace,
             "ga_gaussian_kl_f32: null pointer");
  GA_REQUIRE(M > 0 && A > 0 && ld >= A, "ga_gaussian_kl_f32: bad sizes");
  const int nb = red_blocks(M);
  ls_launch_gaussian_kl(mean_old, mean_new, ld, M, A, log_std_old, log_std_new, workspace,
                        (unsigned)nb, stream);
  GA_CHECK_LAUNCH("gaussian_kl");
  ls_launch_sum_partials(workspace, nb, kl_sum_out, stream);
  GA_CHECK_LAUNCH("sum_partials");
  return GA_OK;
}

// ---- optimiser --------------------------------------------------------------
extern "C" int ga_reduce_slabs_f32(const float* slabs, int64_t n_splits,
                                   int64_t slab_stride, int64_t n, float scale,
                                   float* out, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(slabs && out, "ga_reduce_slabs_f32: null pointer");
  GA_REQUIRE(n > 0 && n % 4 == 0 && slab_stride % 4 == 0 && n_splits >= 1,
             "ga_reduce_slabs_f32: n and stride must be multiples of 4");
  GA_REQUIRE(ga_aligned16(slabs) && ga_aligned16(out),
             "ga_reduce_slabs_f32: 16-B alignment required");
  // 64 float4 columns per block
  ls_launch_reduce_slabs(slabs, n_splits, slab_stride, n, out, scale,
                         (unsigned)ga_ceil_div(n / 4, 64), stream);
  GA_CHECK_LAUNCH("reduce_slabs");
  return GA_OK;
}

extern "C" int ga_reduce_adam_f32(const float* slabs, int64_t n_splits,
                                  int64_t slab_stride, float* params, float* grads,
                                  float* exp_avg, float* exp_avg_sq, int64_t n,
                                  int64_t step, double lr, double beta1, double beta2,
                                  double eps, int zero_slot0, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(slabs && params && grads && exp_avg && exp_avg_sq,
             "ga_reduce_adam_f32: null pointer");
  GA_REQUIRE(n > 0 && n % 4 == 0 && slab_stride % 4 == 0 && n_splits >= 1 && step >= 1,
             "ga_reduce_adam_f32: bad sizes");
  GA_REQUIRE(ga_aligned16(slabs) && ga_aligned16(params) && ga_aligned16(grads) &&
                 ga_aligned16(exp_avg) && ga_aligned16(exp_avg_sq),
             "ga_reduce_adam_f32: 16-B alignment required");
  ls_launch_reduce_adam(
      slabs, n_splits, slab_stride, zero_slot0,
      adam_params(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps), grads,
      (unsigned)ga_ceil_div(n / 4, 64), stream);
  GA_CHECK_LAUNCH("reduce_adam");
  return GA_OK;
}

extern "C" int ga_adam_step_f32(float* params, const float* grads, float* exp_avg,
                                float* exp_avg_sq, int64_t n, int64_t step, double lr,
                                double beta1, double beta2, double eps,
                                ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(params && grads && exp_avg && exp_avg_sq, "ga_adam_step_f32: null pointer");
  GA_REQUIRE(n > 0 && step >= 1, "ga_adam_step_f32: bad n / step");
  ls_launch_adam(
      adam_params(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps),
      (unsigned)ga_ceil_div(n, 256), stream);
  GA_CHECK_LAUNCH("adam");
  return GA_OK;
}

// (the kinds, their hyper-parameters h and state buffers: OptParams, loss_params.h)
extern "C" int ga_optimizer_step_f32(int kind, float* params, const float* grads,
                                     float* s1, float* s2, float* s3, int64_t n,
                                     int64_t step, const double* h, int flags,
                                     ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(params && grads && h, "ga_optimizer_step_f32: null pointer");
  GA_REQUIRE(n > 0 && step >= 1 && kind >= 1 && kind <= 3,
             "ga_optimizer_step_f32: bad n / step / kind");
  OptParams a;
  memset(&a, 0, sizeof(a));
  a.p = params; a.g = grads; a.s1 = s1; a.s2 = s2; a.s3 = s3; a.n = n;
  a.kind = kind; a.flags = flags; a.first = step == 1;
  a.neg_lr = (float)(-h[0]); a.h1 = (float)h[1]; a.h2 = (float)h[2];
  a.h3 = (float)h[3]; a.h4 = (float)h[4];
  // complements and products of the hyper-parameters: in double, rounded once
  if (kind == 1) {
    GA_REQUIRE(h[1] == 0.0 || s1, "ga_optimizer_step_f32: SGD momentum buffer");
    a.w1 = (float)(1.0 - h[2]);
  } else if (kind == 2) {
    GA_REQUIRE(s1 && (h[4] <= 0.0 || s2) && (!(flags & 1) || s3),
               "ga_optimizer_step_f32: RMSprop state buffers");
    a.w1 = (float)(1.0 - h[1]);
  } else {
    GA_REQUIRE(s1 && s2 && (!(flags & 1) || s3),
               "ga_optimizer_step_f32: Adam state buffers");
    const GaAdam c = ga_adam_coeffs(h[0], h[1], h[2], h[3], step);
    a.w1 = c.lerp_w;
    a.w2 = c.one_minus_beta2;
    a.decay = (float)(1.0 - h[0] * h[4]);
    a.neg_step_size = c.neg_step_size;
    a.bc2_sqrt = c.bc2_sqrt;
  }
  ls_launch_optimizer_step(a, (unsigned)ga_ceil_div(n, 256), stream);
  GA_CHECK_LAUNCH("optimizer_step");
  return GA_OK;
}

// ---- advantage statistics ---------------------------------------------------
extern "C" int ga_stats_f32(const float* x, int64_t n, int what, double* stats,
                            double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(x && stats && workspace, "ga_stats_f32: null pointer");
  GA_REQUIRE(n > 0 && what >= 0 && what <= 2, "ga_stats_f32: bad arguments");
  ls_launch_stats(what, x, n, stats, workspace, (unsigned)red_blocks(n), stream);
  GA_CHECK_LAUNCH("stats");
  return GA_OK;
}

extern "C" int ga_adv_center_f32(float* x, int64_t n, const double* stats, float eps,
                                 ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(x && stats && n > 0, "ga_adv_center_f32: bad arguments");
  ls_launch_adv_center(x, n, stats, eps, (unsigned)red_blocks(n), stream);
  GA_CHECK_LAUNCH("adv_center");
  return GA_OK;
}

extern "C" int ga_sub_scalar_f32(float* x, int64_t n, const double* scalar,
                                 ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(x && scalar && n > 0, "ga_sub_scalar_f32: bad arguments");
  ls_launch_sub_scalar(x, n, scalar, (unsigned)red_blocks(n), stream);
  GA_CHECK_LAUNCH("sub_scalar");
  return GA_OK;
}

// ---- vector ops of the constrained (TRPO) policy step ------------------------------
// torch/optimizers/conjugate_gradient_optimizer.py:69-104,146-186 works on the flat
// parameter vector (~72 k floats at C3): dot products and axpy-type updates.
extern "C" int ga_dot_f32(const float* a, const float* b, int64_t n, double* out,
                          ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(a && b && out && n > 0, "ga_dot_f32: bad arguments");
  ls_launch_dot(a, b, n, out, 1, stream);  // one workgroup: a fixed order
  GA_CHECK_LAUNCH("dot");
  return GA_OK;
}

extern "C" int ga_axpby_f32(double alpha, const float* x, double beta, float* y,
                            int64_t n, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(x && y && n > 0, "ga_axpby_f32: bad arguments");
  ls_launch_axpby((float)alpha, x, (float)beta, y, n, (unsigned)ga_ceil_div(n, 256), stream);
  GA_CHECK_LAUNCH("axpby");
  return GA_OK;
}

extern "C" int ga_fisher_seed_gaussian_f32(const float* tmean, int64_t ldt, int64_t M,
                                           int A, const float* log_std, int has_min,
                                           float min_log_std, int has_max,
                                           float max_log_std, float* dout, int64_t ldd,
                                           ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(tmean && log_std && dout && M > 0 && A > 0 && ldt >= A && ldd >= A,
             "ga_fisher_seed_gaussian_f32: bad arguments");
  ls_launch_fisher_seed_gaussian(tmean, ldt, M, A, log_std, has_min, min_log_std, has_max,
                                 max_log_std, dout, ldd, (unsigned)ga_ceil_div(M, 256),
                                 stream);
  GA_CHECK_LAUNCH("fisher_seed");
  return GA_OK;
}

extern "C" int ga_fisher_seed_categorical_f32(const float* scores, int64_t lds,
                                              const float* tscores, int64_t ldt,
                                              int64_t M, int A, int double_softmax,
                                              float* dout, int64_t ldd,
                                              ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(scores && tscores && dout && M > 0 && A > 0 && A <= FS_MAX_A && lds >= A &&
                 ldt >= A && ldd >= A,
             "ga_fisher_seed_categorical_f32: bad arguments");
  ls_launch_fisher_seed_categorical(scores, lds, tscores, ldt, M, A, double_softmax, dout,
                                    ldd, (unsigned)ga_ceil_div(M, 256), stream);
  GA_CHECK_LAUNCH("fisher_seed_categorical");
  return GA_OK;
}

// ---- head layer fused into the loss ------------------------------------------------
// In a minibatch step the network's last linear layer (hidden -> action means, or
// hidden -> value) feeds nothing but the loss; the head kernels compute it in the loss
// kernel and leave the batch sums to the finalize launch of the plain entry.
extern "C" int ga_head_loss_supported(int hidden_width, int A) {
  return ga_head_loss_rule(hidden_width, A);
}

extern "C" int ga_head_ppo_gaussian_loss_f32(
    const float* H, int64_t ldh, const float* W, int64_t ldw, const float* bias,
    int hidden_width, float* mean_out, int64_t ldm, const float* actions, int64_t lda,
    const float* old_ll, const float* adv, const int32_t* idx, const float* log_std,
    int has_min, float min_log_std, int has_max, float max_log_std, int64_t M, int A,
    int algo, float clip, float ent_coeff, int ent_flags, float* dmean, int64_t ldd,
    float* ll_out, float* loss_out, float* grad_slab0, int64_t slab_stride,
    int64_t n_splits, double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(H && W && bias && actions && adv && log_std && loss_out && workspace,
             "ga_head_ppo_gaussian_loss_f32: null pointer");
  GA_REQUIRE(ga_head_loss_supported(hidden_width, A),
             "ga_head_ppo_gaussian_loss_f32: unsupported head %d x %d", A, hidden_width);
  GA_REQUIRE(algo == 1 || old_ll, "ga_head_ppo_gaussian_loss_f32: PPO needs old_ll");
  GA_REQUIRE(M > 0 && ldh >= hidden_width && ldh % 4 == 0 && ldw >= hidden_width &&
                 ldw % 4 == 0 && lda >= A && (!dmean || ldd >= A) &&
                 (!mean_out || ldm >= A) && ga_aligned16(H) && ga_aligned16(W),
             "ga_head_ppo_gaussian_loss_f32: bad sizes / alignment");
  HeadLayer L;
  L.H = H; L.ldh = ldh; L.W = W; L.ldw = ldw; L.bias = bias; L.K = hidden_width;
  L.out = mean_out; L.ldo = ldm;
  const PpoLossParams p =
      ppo_loss_params(nullptr, ldd, actions, lda, old_ll, adv, idx, log_std, has_min,
                      min_log_std, has_max, max_log_std, M, A, algo, clip, ent_coeff,
                      ent_flags, dmean, ll_out, workspace);
  const int nb = head_blocks(M);
  ls_launch_head_ppo_gaussian(L, p, (unsigned)nb, head_lds_bytes(A, hidden_width), stream);
  GA_CHECK_LAUNCH("head_ppo_gaussian");
  ls_launch_ppo_gaussian_finalize(
      ppo_finalize_params(p, nb, loss_out, grad_slab0, slab_stride, n_splits), stream);
  GA_CHECK_LAUNCH("ppo_gaussian_finalize");
  return GA_OK;
}

extern "C" int ga_head_gaussian_nll_loss_f32(
    const float* H, int64_t ldh, const float* W, const float* bias, int hidden_width,
    float* v_out, int64_t ldv_out, const float* returns, const int32_t* idx,
    const float* log_std, int64_t M, float* dv, int64_t ldd, float* loss_out,
    float* grad_slab0, int64_t slab_stride, int64_t n_splits, double* workspace,
    ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(H && W && bias && returns && log_std && loss_out && workspace,
             "ga_head_gaussian_nll_loss_f32: null pointer");
  GA_REQUIRE(ga_head_loss_supported(hidden_width, 1),
             "ga_head_gaussian_nll_loss_f32: unsupported hidden width %d", hidden_width);
  GA_REQUIRE(M > 0 && ldh >= hidden_width && ldh % 4 == 0 && (!dv || ldd >= 1) &&
                 (!v_out || ldv_out >= 1) && ga_aligned16(H) && ga_aligned16(W),
             "ga_head_gaussian_nll_loss_f32: bad sizes / alignment");
  HeadLayer L;
  L.H = H; L.ldh = ldh; L.W = W; L.ldw = hidden_width; L.bias = bias;
  L.K = hidden_width; L.out = v_out; L.ldo = ldv_out;
  const NllParams p = nll_params(nullptr, ldd, returns, idx, log_std, M, dv, workspace);
  const int nb = head_blocks(M);
  ls_launch_head_gaussian_nll(L, p, (unsigned)nb, head_lds_bytes(1, hidden_width), stream);
  GA_CHECK_LAUNCH("head_gaussian_nll");
  ls_launch_gaussian_nll_finalize(workspace, nb, M, loss_out, grad_slab0, slab_stride,
                                  n_splits, stream);
  GA_CHECK_LAUNCH("gaussian_nll_finalize");
  return GA_OK;
}
