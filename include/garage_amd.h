/* garage_amd -- C ABI of the MI355X (gfx950) on-policy rollout + PPO update engine.
 *
 * The reference (akolobov/garage v2021.03.0) is 100 % Python and has no FFI: its
 * plugin surface is a set of Python classes.  This header
 * is the boundary between that Python surface (mirrored by the `garage_amd`
 * package) and the hand-written HIP kernels; each entry point names the
 * reference code it replaces (paths relative to /root/reference/src/garage).
 * INTEGRATION.md shows the ctypes binding a garage maintainer would add.
 *
 * Conventions
 *   - extern "C"; plain pointers and sizes; no torch types.
 *   - every pointer is a caller-owned DEVICE pointer unless the name ends in
 *     `_host`; fp32 unless noted; row-major; "ld*" = floats between rows.
 *   - matrices handed to the MLP entry points must be 16-byte aligned with
 *     leading dimensions that are multiples of 4 floats (garage_amd pads).
 *   - asynchronous on `stream` (a hipStream_t, passed as void*); no allocation,
 *     no synchronisation, graph-capture safe; scratch is passed in.
 *   - return 0 on success, <0 on error; ga_last_error() returns a thread-local
 *     message.  Nothing throws across the boundary.
 */
#ifndef GARAGE_AMD_H_
#define GARAGE_AMD_H_

#include <stdint.h>

/* The library is built with -fvisibility=hidden: what this header declares is
 * exactly what it exports. */
#define GA_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ga_stream_t; /* hipStream_t */

GA_API int ga_abi_version(void); /* 5 */
/* Wherever a policy's scalar std parameter crosses this interface it comes as
 * (log_std pointer, has_min, min_log_std, has_max, max_log_std) and goes through
 * GaussianMLPBaseModule.forward's transformation
 * (torch/modules/gaussian_mlp_module.py:165-181): clamp to [min, max], then
 * std = exp(p) or, when bit 1 of `has_min` is set (std_parameterization =
 * 'softplus'), std = log(1 + exp(exp(p))).  Bit 0 of `has_min` = the lower clamp is
 * present.  The gradient written for the parameter includes the transformation's
 * slope (0 through an active clamp). */
GA_API const char* ga_last_error(void);

/* ---- returns + GAE(lambda) -------------------------------------------------
 * Replaces garage.np.discount_cumsum called per padded row
 * (np/_functions.py:111-128; call site torch/algos/vpg.py:149-153) and
 * garage.torch.compute_advantages (torch/_functions.py:25-85) including the
 * zero-padding semantics of short episodes.
 *   mode 0: rows are env slices of the (n_rows, T) rollout buffer, row stride
 *           ld; tail[i] = episode length at an episode's last step, else 0.
 *   mode 1: every row is one episode (packed batch via offsets[n_rows+1] with
 *           max_len >= the longest row -- a contract: rows are scanned in one
 *           pass of max_len steps when max_len <= 256 -- or a padded (N, P)
 *           batch with offsets = NULL).
 * v0 = value of the all-zero observation (content of padded baselines);
 * bonus / bonus_const = per-step / constant reward bonus added for the
 * advantages only (entropy_method='max', vpg.py:158-160).
 * Algorithmic HBM bytes: 16 per step. */
GA_API int ga_gae_scan_f32(const float* rewards, const float* values, const float* bonus,
                           const uint16_t* tail, const int64_t* offsets, int64_t n_rows,
                           int64_t T, int64_t ld, int64_t max_len, int mode,
                           int max_episode_length, double discount, double gae_lambda,
                           float v0, float bonus_const, float* adv, float* ret,
                           ga_stream_t stream);
/* Whole-episode rows (mode 1) of at most 256 steps without a per-step bonus take
 * constant-decay fast paths (fixed horizon: aligned rows of exactly
 * max_episode_length steps; otherwise the ragged variant) when all four arrays
 * start on 16-byte boundaries; 0 forces the general kernel (A/B runs, tests). */
GA_API int ga_set_gae_fixed_fast_path(int on);
/* Steps per lane of those fast paths: 4 (one 16-B access per array and lane) or 8
 * (two; half the lanes, waves and shuffle steps per row).  Same recurrences in
 * another association order: results agree to fp64 rounding. */
GA_API int ga_set_gae_rows_steps_per_lane(int steps);

/* ---- MLP forward / backward (fp32 MFMA GEMMs) -------------------------------
 * Replaces MLPModule / MultiHeadedMLPModule.forward
 * (torch/modules/multi_headed_mlp_module.py:136-151) and its autograd backward
 * as used by VPG._train_policy / _train_value_function (vpg.py:250-293).
 * Hidden activations: tanh (the GaussianMLP* defaults,
 * torch/policies/gaussian_mlp_policy.py:44-60), relu, none, sigmoid, elu, leaky_relu
 * or softplus (hidden_act below); the output layer takes the same set (output_act). */
typedef struct {
  int32_t n_layers;   /* linear layers incl. the output layer, 1..8 */
  int32_t dims[9];    /* dims[0] = input width, dims[l+1] = width of layer l */
  int64_t w_off[8];   /* W_l [dims[l+1]][round4(dims[l])] offset (floats) in params */
  int64_t b_off[8];   /* b_l [dims[l+1]] offset (floats) in params */
  int64_t act_off[8]; /* hidden layer l output offset in the activation workspace,
                         row stride round4(dims[l+1]) */
  int32_t hidden_act; /* hidden_nonlinearity of MLPModule
                         (torch/modules/mlp_module.py:43-44): 0 = tanh (the
                         GaussianMLP* default; what a zeroed descriptor means),
                         1 = relu, 2 = none, 3 = sigmoid, 4 = elu, 5 = leaky_relu,
                         6 = softplus (torch's defaults).  The fused rollout step
                         (ga_policy_step_fused_f32, the one-launch rollout) takes
                         all of them; the fused TRAINING kernels implement tanh,
                         other networks train through the per-layer GEMMs. */
  int32_t output_act; /* output_nonlinearity of the same module applied to the last
                         layer (the Gaussian mean / the value): 0 = none (default),
                         1 = tanh, 2 = relu, 3 .. 6 as hidden_act.  Per-layer
                         kernels and the fused rollout step; the caller scales the
                         loss's d(output) by the slope before the backward pass
                         (ga_act_slope_mul_f32). */
  int32_t layer_norm; /* layer_normalization of the same module
                         (multi_headed_mlp_module.py:77-81): LayerNorm(eps 1e-5,
                         affine) over the input of every hidden linear layer.
                         Per-layer kernels and the fused rollout step (which
                         normalises the rows in LDS; ln_off[l] % 4 == 0). */
  int32_t pad_;
  int64_t ln_off[8];  /* gamma_l [round4(dims[l])] offset in params; beta_l follows */
  int64_t lnx_off[8]; /* normalised input of hidden layer l in the activation
                         workspace (row stride round4(dims[l])) ... */
  int64_t lns_off[8]; /* ... and its per-row (mean, rstd) pairs */
} ga_mlp_desc;

/* dout[i, j] *= slope of the activation `act` (the codes of ga_mlp_desc.output_act:
 * 0 none -- nothing is launched --, 1 tanh, 2 relu, 3 sigmoid, 4 elu, 5 leaky_relu,
 * 6 softplus) at its OUTPUT
 * out[i, j], j < N: turns the loss's gradient with respect to an output layer
 * with an output_nonlinearity into the gradient with respect to its pre-activation
 * (what ga_mlp_backward_f32 takes). */
GA_API int ga_act_slope_mul_f32(float* dout, int64_t ldd, const float* out, int64_t ldo,
                                int64_t M, int N, int act, ga_stream_t stream);

/* out[M, ldo] = MLP(X[row_idx[i]] or X[i]); acts keeps the hidden outputs. */
GA_API int ga_mlp_forward_f32(const ga_mlp_desc* d, const float* params, const float* X,
                              int64_t ldx, const int32_t* row_idx, int64_t M, float* acts,
                              float* out, int64_t ldo, ga_stream_t stream);
/* The same forward with every layer in ONE launch (activations of 32 rows stay in
 * LDS between layers, weights stream from L2); ga_mlp_forward_f32 dispatches to
 * it when ga_policy_step_fused_supported(d) and the network is the tanh one
 * (hidden_act 0, output_act 0, no layer_norm; anything else is refused here).
 * ga_set_fused_forward(0) forces the per-layer GEMM path (A/B measurements). */
GA_API int ga_mlp_forward_fused_f32(const ga_mlp_desc* d, const float* params,
                                    const float* X, int64_t ldx, const int32_t* row_idx,
                                    int64_t M, float* acts, float* out, int64_t ldo,
                                    ga_stream_t stream);
GA_API int ga_set_fused_forward(int on);
/* Outputs only: ga_mlp_forward_f32 with acts == NULL computes the whole network in
 * one launch without writing any activation (two hidden tanh layers of 128 / 256
 * units, <= 32 inputs, <= 8 linear outputs: the full-batch evaluation passes of
 * vpg.py:147-184 -- baselines, old log-likelihoods, LossBefore / LossAfter / KL).
 * ga_mlp_forward_eval_supported(d) says whether a network qualifies;
 * ga_set_eval_forward(0) (GARAGE_AMD_EVAL_FORWARD=0) makes it answer no. */
GA_API int ga_mlp_forward_eval_supported(const ga_mlp_desc* d);
GA_API int ga_set_eval_forward(int on);
/* Layer products with one dimension <= 32 (first-layer forward, head data
 * gradient, first-layer / head weight gradients) run as HBM-streaming kernels
 * instead of MFMA tiles (default on; 0 = MFMA tiles everywhere, for A/B runs). */
GA_API int ga_set_skinny_kernels(int on);
/* The head layer's weight-gradient streaming kernel also writes the data gradient
 * of the layer below (same pass over the hidden activations) when the head is
 * <= 16 wide (default on; 0 = separate data-gradient launch, for A/B runs). */
GA_API int ga_set_fused_head_dgrad(int on);
/* ga_mlp_forward_f32 applies the head layer (<= 8 outputs) in the epilogue of the
 * last hidden layer's GEMM when that layer is 64 or 128 units wide (mode 2: also
 * 256) and M is a multiple of 64: a workgroup's tile then spans whole rows, so the
 * staged tanh outputs are multiplied with the head weights before they leave the
 * CU and the narrow head GEMM (one more pass over the hidden activations)
 * disappears.  mode 0 = separate head launch, 1 = default, 2 = 256-wide layers too
 * (faster with one update chain on the chip, slower with two; gemm.hip). */
GA_API int ga_set_fused_head_forward(int mode);
/* GEMMs with at most 128 tiles of 128 x 128 (minibatches of a few thousand rows
 * and below, e.g. the reference's default minibatch of 64) run on 64 x 64 tiles
 * with 128-deep k-steps: more workgroups, K / 128 dependent memory round trips
 * instead of K / 32; bit-identical results (default on; 0 for A/B runs). */
GA_API int ga_set_small_m_gemm(int on);
/* ga_update_epoch*: a minibatch of <= 64 rows through a network of two equal
 * tanh hidden layers (32, 64, ... 256 units, <= 32 inputs, <= 8 outputs;
 * Gaussian or categorical PPO / VPG objective with the entropy options, or the
 * value NLL; one process) takes its whole optimizer step -- gather, forward, loss, backward,
 * Adam -- in ONE launch of H / 16 workgroups with two grid barriers
 * (small_step.hip) instead of ten dependent launches.  Same formulas, other
 * summation orders: results agree to rounding.  The last slot of the reduction
 * workspace is raised when a barrier gave up (never seen); that launch and every
 * later one then leave the parameters untouched.  Default on; 0 = per-layer
 * path. */
GA_API int ga_set_small_step(int on);
/* Test hooks of that path.  resident_cap: workgroups the device is taken to hold
 * at once (< 0: ask the occupancy query; 0 forces the per-layer path -- the
 * fallback for shapes whose two concurrent grids would not be co-resident).
 * max_polls: polls after which a waiter at a grid barrier abandons the launch
 * (< 0: default 2^22; 0 forces the abort path).  An abandoned launch writes no
 * parameter; the fault word stays raised and later launches return at once until
 * the caller has cleared the last two workspace slots. */
GA_API int ga_set_small_step_resident_cap(int workgroups);
GA_API int ga_set_small_step_max_polls(int polls);
GA_API int64_t ga_small_step_launches(void); /* launches so far (tests, diagnostics) */
/* Developer hook (tools/small_step_phases.py): the first call arms the recording
 * and returns 1; later calls synchronise and copy 16 timestamps (100 MHz wall
 * clock of workgroup 0 at the phase boundaries of the most recent launch) to the
 * HOST array and return 0. */
GA_API int ga_small_step_debug(long long* host_out16);
/* the same for the one-launch step of 2 x 32 / 2 x 64 networks (narrow_step.hip) */
GA_API int ga_narrow_step_debug(long long* host_out16);
/* ... for the fused rollout step (policy_fused.hip) */
GA_API int ga_policy_step_debug(long long* host_out32);
/* ... and for the fused last-hidden-layer + head + loss kernel (fused_train.hip) */
GA_API int ga_fused_fwd_debug(long long* host_out16);
/* (start, end of the k-loop, end) of the first n <= 4096 workgroups of that launch */
GA_API int ga_fused_fwd_debug_skew(long long* host_out, int n);
/* the data-gradient + first-layer weight-gradient kernel: which = 0 -> 16 phase
 * stamps of one workgroup (the first call arms the hook and returns 1), which = 1
 * -> (start, end of the k-loop, end) of the first n workgroups */
GA_API int ga_fused_dgrad_debug(long long* host_out, int which, int n);
/* -DGA_FT_LOOP_STAMPS builds only (make EXTRA=-DGA_FT_LOOP_STAMPS,
 * tools/fused_fwd_phases.py): after ga_fused_fwd_debug has armed the recording, per
 * workgroup 4 tick sums over the k-loop of the fused last-hidden-layer kernel
 * (fragment reads + MFMAs, first barrier, tile stores, second barrier) of the first
 * n <= 4096 workgroups */
GA_API int ga_fused_fwd_debug_loop(long long* host_out, int n);
/* Keeps the MFMA pipe busy on `stream` for hazard reproduction (tests, tools):
 * `blocks` workgroups of 512 threads run `iters` rounds of bf16 (mode 1) or fp32
 * (otherwise) MFMAs; `sink` is written only to keep the loop alive. */
GA_API int ga_debug_mfma_burn(int mode, int iters, int blocks, float* sink,
                              ga_stream_t stream);
/* Test switch of the split-operand mode (ga_set_split_bf16): 0 = every forward
 * launch computes its bf16 weight planes itself instead of reusing the ones the
 * optimizer step rewrote (default 1; GARAGE_AMD_SPLIT_ADAM_PLANES=0). */
GA_API int ga_set_split_adam_planes(int on);
/* Forward-mode tangent of the MLP (torch/optimizers/conjugate_gradient_optimizer.py
 * :18-66 takes the same product by double backward): with dtheta = tangent (flat
 * parameter layout) and acts = the hidden activations of a forward at the same
 * rows, tout[M, ldo] = d(output); tacts is a workspace shaped like acts. */
GA_API int ga_mlp_jvp_f32(const ga_mlp_desc* d, const float* params, const float* tangent,
                          const float* X, int64_t ldx, const int32_t* row_idx, int64_t M,
                          const float* acts, float* tacts, float* tout, int64_t ldo,
                          ga_stream_t stream);
/* split count ga_mlp_backward_f32 should be called with for M rows */
GA_API int64_t ga_mlp_backward_splits(const ga_mlp_desc* d, int64_t M);
/* dout = dLoss/d(out).  Writes n_splits partial gradient slabs, each laid out
 * like `params` (slab_stride floats apart); ga_reduce_slabs_f32 sums them. */
GA_API int ga_mlp_backward_f32(const ga_mlp_desc* d, const float* params, const float* X,
                               int64_t ldx, const int32_t* row_idx, int64_t M,
                               const float* acts, const float* dout, int64_t ldo,
                               float* dacts, float* grad_slabs, int64_t slab_stride,
                               int64_t n_splits, ga_stream_t stream);
/* C[M,N] = A[M,K] B[N,K]^T, exposed for tests of the GEMM core. */
GA_API int ga_gemm_nt_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                          float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          ga_stream_t stream);

/* ---- losses -----------------------------------------------------------------
 * workspace: ga_reduction_workspace_doubles() doubles of device scratch, ZEROED
 * once by the caller (its last two slots are a ticket / barrier pair every launch
 * leaves at 0 and a fault flag), used by one stream at a time. */
GA_API int64_t ga_reduction_workspace_doubles(void);
/* Loss launches of one block (<= 256 rows) write the loss and the log-std gradient
 * slot themselves.  1 = launches of several blocks do too: the block that draws
 * the last ticket adds the blocks' partial sums in block order (the bits of the
 * one-wave finalize launch it replaces); default 0 -- the device-scope fences cost
 * more than the launch they save (losses.hip). */
GA_API int ga_set_one_launch_losses(int on);

/* PPO clipped surrogate (algo 0; torch/algos/ppo.py:96-132) or VPG objective
 * (algo 1; vpg.py:434-454) for a Gaussian policy with a scalar log-std
 * (torch/modules/gaussian_mlp_module.py:158-192), + entropy regularisation
 * (vpg.py:343-345,408-432; ent_flags bit0 regularized, bit1 softplus, bit2
 * stop-gradient).  Writes loss = -mean(objective), optionally dLoss/dmean,
 * the new log-likelihoods and dLoss/dlog_std (into slot 0 of slab 0). */
GA_API int ga_ppo_gaussian_loss_f32(const float* mean, int64_t ldm, const float* actions,
                                    int64_t lda, const float* old_ll, const float* adv,
                                    const int32_t* idx, const float* log_std, int has_min,
                                    float min_log_std, int has_max, float max_log_std,
                                    int64_t M, int A, int algo, float clip, float ent_coeff,
                                    int ent_flags, float* dmean, float* ll_out,
                                    float* loss_out, float* grad_slab0, int64_t slab_stride,
                                    int64_t n_splits, double* workspace, ga_stream_t stream);
/* The same objective for a categorical MLP head (discrete actions, BASELINE.json
 * configs 1-2).  No torch CategoricalMLPPolicy exists in the reference; the
 * convention follows its torch categorical policies, which pass
 * softmax(net(x)) as `logits=` (torch/policies/categorical_cnn_policy.py:138-139;
 * double_softmax = 1), and log_prob casts float actions with .long()
 * (SURVEY.md Q24).  ent_out / ent_sum_out: per-row / summed entropies. */
GA_API int ga_ppo_categorical_loss_f32(const float* scores, int64_t lds,
                                       const float* actions, int64_t lda,
                                       const float* old_ll, const float* adv,
                                       const int32_t* idx, int64_t M, int A,
                                       int double_softmax, int algo, float clip,
                                       float ent_coeff, int ent_flags, float* dscores,
                                       float* ll_out, float* ent_out, float* loss_out,
                                       double* ent_sum_out, float* grad_slab0,
                                       int64_t slab_stride, int64_t n_splits,
                                       double* workspace, ga_stream_t stream);
GA_API int ga_categorical_kl_f32(const float* scores_old, const float* scores_new,
                                 int64_t ld, int64_t M, int A, int double_softmax,
                                 double* kl_sum_out, double* workspace, ga_stream_t stream);
/* GaussianMLPValueFunction.compute_loss
 * (torch/value_functions/gaussian_mlp_value_function.py:81-98). */
GA_API int ga_gaussian_nll_loss_f32(const float* v, int64_t ldv, const float* returns,
                                    const int32_t* idx, const float* log_std, int64_t M,
                                    float* dv, float* loss_out, float* grad_slab0,
                                    int64_t slab_stride, int64_t n_splits, double* workspace,
                                    ga_stream_t stream);
/* The head layer fused into the loss: H[M, ldh] are the last hidden activations,
 * W[A][ldw] / bias[A] the head's weights (torch/modules/gaussian_mlp_module.py
 * :288-305 output layer).  Same loss, gradient seed (dmean / dv, row stride ldd)
 * and log-std gradient as the unfused entry points above; mean_out / v_out
 * optionally receive the head outputs.  Supported shapes: ga_head_loss_supported.
 * ga_set_fused_head_loss(1) makes ga_update_epoch* use them (default 0: measured
 * equal to the head GEMM + loss kernel pair at the C3 minibatch). */
GA_API int ga_head_loss_supported(int hidden_width, int A);
GA_API int ga_set_fused_head_loss(int on);
GA_API int ga_head_ppo_gaussian_loss_f32(
    const float* H, int64_t ldh, const float* W, int64_t ldw, const float* bias,
    int hidden_width, float* mean_out, int64_t ldm, const float* actions, int64_t lda,
    const float* old_ll, const float* adv, const int32_t* idx, const float* log_std,
    int has_min, float min_log_std, int has_max, float max_log_std, int64_t M, int A,
    int algo, float clip, float ent_coeff, int ent_flags, float* dmean, int64_t ldd,
    float* ll_out, float* loss_out, float* grad_slab0, int64_t slab_stride,
    int64_t n_splits, double* workspace, ga_stream_t stream);
GA_API int ga_head_gaussian_nll_loss_f32(
    const float* H, int64_t ldh, const float* W, const float* bias, int hidden_width,
    float* v_out, int64_t ldv_out, const float* returns, const int32_t* idx,
    const float* log_std, int64_t M, float* dv, int64_t ldd, float* loss_out,
    float* grad_slab0, int64_t slab_stride, int64_t n_splits, double* workspace,
    ga_stream_t stream);
/* sum over rows of KL(old || new), VPG._compute_kl_constraint (vpg.py:381-406) */
GA_API int ga_gaussian_kl_f32(const float* mean_old, const float* mean_new, int64_t ld,
                              int64_t M, int A, float log_std_old, float log_std_new,
                              double* kl_sum_out, double* workspace, ga_stream_t stream);

/* ---- optimiser: OptimizerWrapper.step == torch.optim.Adam.step
 * (torch/optimizers/optimizer_wrapper.py:53-63, _functions.py:25-65) */
GA_API int ga_reduce_slabs_f32(const float* slabs, int64_t n_splits, int64_t slab_stride,
                               int64_t n, float scale, float* out, ga_stream_t stream);
/* ga_reduce_slabs_f32 (scale 1) + ga_adam_step_f32 in one launch; the reduced
 * gradient is also written to `grads`.  zero_slot0: keep element 0 (the log-std
 * slot) untrained. */
GA_API int ga_reduce_adam_f32(const float* slabs, int64_t n_splits, int64_t slab_stride,
                              float* params, float* grads, float* exp_avg,
                              float* exp_avg_sq, int64_t n, int64_t step, double lr,
                              double beta1, double beta2, double eps, int zero_slot0,
                              ga_stream_t stream);
GA_API int ga_adam_step_f32(float* params, const float* grads, float* exp_avg,
                            float* exp_avg_sq, int64_t n, int64_t step, double lr,
                            double beta1, double beta2, double eps, ga_stream_t stream);
/* make_optimizer (_functions.py:25-65) builds ANY torch.optim class; beyond the default
 * Adam (fused into the update kernels) these run as one elementwise launch over the
 * flat buffer, torch's single-tensor arithmetic:
 *   kind 1 torch.optim.SGD      h = {lr, momentum, dampening, weight_decay, -};
 *                               flags bit 0 nesterov; s1 = momentum buffer
 *   kind 2 torch.optim.RMSprop  h = {lr, alpha, eps, weight_decay, momentum}; flags bit 0
 *                               centered; s1 square_avg, s2 momentum buffer, s3 grad_avg
 *   kind 3 torch.optim.Adam / AdamW with weight_decay / amsgrad
 *                               h = {lr, beta1, beta2, eps, weight_decay}; flags bit 0
 *                               amsgrad, bit 1 decoupled decay (AdamW); s1 exp_avg,
 *                               s2 exp_avg_sq, s3 max_exp_avg_sq
 * h: HOST pointer to 5 doubles; step counts from 1; unused state pointers may be NULL.
 * Rounding: one fp32 rounding per torch tensor operation (lerp_ is one fused
 * multiply-add; addcdiv is x + (value * t1) / t2).  Every scalar torch forms in Python
 * -- 1 - beta1, 1 - beta2, 1 - alpha, 1 - dampening, 1 - lr * weight_decay,
 * -lr / bias_correction1, sqrt(bias_correction2), -lr -- is formed here from the
 * doubles in h and rounded to fp32 once, never from constants already rounded. */
GA_API int ga_optimizer_step_f32(int kind, float* params, const float* grads, float* s1,
                                 float* s2, float* s3, int64_t n, int64_t step,
                                 const double* h, int flags, ga_stream_t stream);

/* ---- advantage centring: VPG._compute_advantage (vpg.py:371-377)
 * stats = device double[4]: sum, count, sum of squared deviations, min.
 * what: 0 -> stats[0..1], 1 -> stats[2] (uses the mean in stats), 2 -> stats[3]. */
/* ---- constrained (TRPO) policy step: vectors of n_flat floats -----------------
 * conjugate_gradient_optimizer.py:69-104,146-186.  ga_dot_f32: *out (device
 * double) = sum a[i] b[i], fp64 accumulation, fixed order.  ga_axpby_f32:
 * y = alpha x + beta y.  ga_fisher_seed_gaussian_f32: dout = tmean exp(-2 s) / M,
 * the Gaussian-mean block of the KL Hessian at old == new (s = clamped log-std). */
GA_API int ga_dot_f32(const float* a, const float* b, int64_t n, double* out,
                      ga_stream_t stream);
GA_API int ga_axpby_f32(double alpha, const float* x, double beta, float* y, int64_t n,
                        ga_stream_t stream);
GA_API int ga_fisher_seed_gaussian_f32(const float* tmean, int64_t ldt, int64_t M, int A,
                                       const float* log_std, int has_min, float min_log_std,
                                       int has_max, float max_log_std, float* dout,
                                       int64_t ldd, ga_stream_t stream);
/* The same seed for the categorical head (TRPO with CategoricalMLPPolicy): the KL
 * Hessian with respect to the class scores at old == new, applied to the scores'
 * tangent -- J1 (diag(q) - q q^T) J1 tscores / M with q the class probabilities and J1
 * the Jacobian of the inner softmax of the reference's head
 * (torch/policies/categorical_cnn_policy.py:138-139; identity when double_softmax = 0).
 * A <= 32. */
GA_API int ga_fisher_seed_categorical_f32(const float* scores, int64_t lds,
                                          const float* tscores, int64_t ldt, int64_t M,
                                          int A, int double_softmax, float* dout,
                                          int64_t ldd, ga_stream_t stream);
GA_API int ga_stats_f32(const float* x, int64_t n, int what, double* stats,
                        double* workspace, ga_stream_t stream);
GA_API int ga_adv_center_f32(float* x, int64_t n, const double* stats, float eps,
                             ga_stream_t stream);
GA_API int ga_sub_scalar_f32(float* x, int64_t n, const double* scalar, ga_stream_t stream);

/* ---- rollout ----------------------------------------------------------------
 * Synthetic batched environment (the benchmark workload of BASELINE.json;
 * Environment.reset/step contract of _environment.py:237-276), stepped through
 * ga_env_reset / ga_env_step / ga_env_step_record below like every device env. */
typedef struct {
  int64_t n;
  int64_t env_id0;
  int32_t obs_dim, act_dim, discrete, min_len, max_len;
  uint64_t seed;
  int32_t* episode; /* [n] */
  int32_t* t;       /* [n] */
  int32_t* len;     /* [n] */
} ga_synth_env;

/* NormalizedEnv's observation / reward normalisation
 * (envs/normalized_env.py:118-132,134-164): per-env float64 moving mean and
 * variance, updated before use; rows with mask == 0 (or all when NULL) only.
 * reward = (normalize ? r / (sqrt(var) + 1e-8) : r) * scale. */
GA_API int ga_obs_normalize_f64(int64_t n, int obs_dim, float* obs, int64_t ldo,
                                double* mean, double* var, double alpha,
                                const uint8_t* mask, ga_stream_t stream);
/* The same from src into dst: the wrapped env keeps its own (raw) observations,
 * as the inner env of the reference's NormalizedEnv does. */
GA_API int ga_obs_normalize_from_f64(int64_t n, int obs_dim, const float* src, float* dst,
                                     int64_t ldo, double* mean, double* var, double alpha,
                                     const uint8_t* mask, ga_stream_t stream);
GA_API int ga_reward_normalize_f64(int64_t n, float* reward, double* mean, double* var,
                                   double alpha, double scale, int normalize,
                                   ga_stream_t stream);
/* NormalizedEnv.step's action rescale for a Box with finite bounds
 * (envs/normalized_env.py:90-100): out = clip(low + (a + s) * (0.5 (high - low) / s),
 * low, high) in fp32, s = expected_action_scale; low / high: device float[A]. */
GA_API int ga_action_rescale_f32(int64_t n, int A, const float* actions, int64_t lda,
                                 const float* low, const float* high,
                                 float expected_action_scale, float* out, int64_t ldo,
                                 ga_stream_t stream);

/* dist.sample() of StochasticPolicy.get_actions
 * (torch/policies/stochastic_policy.py:46-89) + the per-env list appends of
 * VecWorker.step_episode (sampler/vec_worker.py:187-197) for observations and
 * actions. */
typedef struct {
  int64_t n, env_id0;
  int32_t A, kind; /* kind 0 gaussian, 1 categorical */
  const float* head; int64_t ldh;
  const float* log_std; int32_t has_min, has_max; float min_log_std, max_log_std;
  const float* noise; int64_t ldn; /* optional teacher-forced noise */
  uint64_t seed; uint32_t step; int32_t double_softmax;
  const float* obs; int64_t ldo; int32_t obs_dim;
  int64_t col, Tcap;
  float* action; int64_t lda;
  float* obs_buf; float* act_buf; float* head_buf;
} ga_head_args;
GA_API int ga_policy_head_sample(const ga_head_args* args, ga_stream_t stream);
/* The same step with the MLP fused in: policy forward (all layers, activations
 * resident in LDS, weights streamed through LDS, hidden layers on MFMA) + the
 * action head + the rollout-buffer writes in ONE launch; `args->head` is
 * ignored.  Supported when the network has 1..8 layers, every layer input is <= 512
 * wide and the head <= 32, for every hidden_act / output_act in 0..6 with or without
 * layer_norm (ga_policy_step_wide_supported); otherwise use ga_mlp_forward_f32 +
 * ga_policy_head_sample.  head_buf receives the Gaussian mean AFTER the
 * output_nonlinearity, as the per-layer path's does.
 * ga_policy_step_fused_supported is the narrower rule -- every layer input <= 256 --
 * of the step kernel's WIDTH = 256 instantiations, which keep the weights resident
 * over a rollout where they fit; the descriptors it accepts run in those, and it is
 * also what ga_mlp_forward_fused_f32 (256-wide tiles) and ga_mlp_forward_f32's
 * dispatch to it ask.  The rest of what ga_policy_step_wide_supported accepts (a
 * superset) runs in the same kernel at WIDTH = 512, which streams the weights;
 * GARAGE_AMD_ROLLOUT_WIDE=0 in the environment makes it refuse them, so that callers
 * take the per-layer path (A/B runs).
 * ga_policy_step_fused_f32, ga_policy_env_step_fused_f32 and ga_rollout_env_steps
 * take every descriptor ga_policy_step_wide_supported accepts. */
GA_API int ga_policy_step_fused_supported(const ga_mlp_desc* d);
GA_API int ga_policy_step_wide_supported(const ga_mlp_desc* d);
GA_API int ga_policy_step_fused_f32(const ga_mlp_desc* d, const float* params,
                                    const ga_head_args* args, ga_stream_t stream);

/* Reward / step-type / episode-end bookkeeping of VecWorker.step_episode and
 * _gather_episode (sampler/vec_worker.py:139-204).  Refused: a null pointer, col
 * outside [0, Tcap), max_episode_length outside 1..65535, ldo < obs_dim. */
typedef struct {
  int64_t n, col, Tcap;
  int32_t max_episode_length;
  const float* reward; const uint8_t* step_type; const float* next_obs;
  int64_t ldo; int32_t obs_dim;
  int32_t* ep_t; float* rew_buf; uint8_t* st_buf; uint16_t* tail_buf;
  float* lastobs_buf; uint8_t* done; int32_t* step_eps; int32_t* step_samples;
  int32_t terminal_only; /* 1: FragmentWorker rule, only TERMINAL ends an episode
                            (sampler/fragment_worker.py:114-115) */
} ga_record_args;
GA_API int ga_record_step(const ga_record_args* args, ga_stream_t stream);
/* NormalizedEnv's observation / reward normalisation fused into ga_env_step_record
 * (the north star's "fused obs-normalise"): the env steps on its raw observations
 * (raw_obs -> raw_next_obs), the moving statistics are updated and
 * rec->next_obs receives the normalised observation the policy sees next -- for
 * the step's observation (recorded as the terminal one where an episode ends)
 * and again for the first observation of a new episode, in that order, as
 * envs/normalized_env.py:134-151 does. */
typedef struct ga_norm_args {
  int32_t normalize_obs, normalize_reward;
  double* obs_mean;      /* [n, obs_dim] float64 moving mean */
  double* obs_var;
  double obs_alpha;
  double* reward_mean;   /* [n] */
  double* reward_var;
  double reward_alpha, reward_scale;
  const float* raw_obs;  /* [n, ldo] the wrapped env's current observations */
  float* raw_next_obs;   /* [n, ldo] where its next observations go */
  /* action rescale (normalized_env.py:90-100) when act_low != NULL: the wrapped env
   * steps on scaled_action (scratch [n, lda], lda the action rows' stride) =
   * ga_action_rescale_f32(policy action); the action buffer and the rollout buffers
   * keep the policy's own.  Read by ga_policy_env_step_fused_f32 and
   * ga_rollout_env_steps, which rescale (columns j < act_dim of the scratch rows are
   * written, nothing else); ga_env_step_record does not read these four fields: it
   * steps on the actions it is handed. */
  const float* act_low;  /* [act_dim] */
  const float* act_high;
  float expected_action_scale;
  float* scaled_action;
} ga_norm_args;

/* ---- device copies of the reference's own environments ---------------------
 * One thread per env, numpy's fp32 arithmetic, the same entry points as the
 * synthetic env (ga_env_reset / ga_env_step / ga_env_step_record below).
 * max_episode_length must be finite (1..65535).
 *
 * PointEnv (envs/point_env.py:79-170): a = clip(action, -0.1, 0.1), point =
 * clip(point + a, -arena_size, arena_size), dist = |point - goal|, success = dist <
 * |(-0.1, -0.1)|, reward = -dist (+ done_bonus on success), done = success and not
 * never_done; observation (x, y, dist), obs_dim 3, act_dim 2.  `success` (optional)
 * receives env_info['success'] as uint8: success[i] from ga_env_step,
 * success[i * rec->Tcap + rec->col] from ga_env_step_record (env-major [n, Tcap],
 * like the other rollout buffers). */
typedef struct {
  int64_t n;
  float arena_size, done_bonus;
  int32_t never_done, max_episode_length;
  float* point;      /* [n, 2] */
  const float* goal; /* [n, 2] */
  int32_t* t;        /* [n] steps taken in the current episode */
  uint8_t* success;  /* optional, see above */
} ga_point_env;

/* GridWorldEnv (envs/grid_world_env.py:111-215): `map` holds every env's grid as
 * rows * cols cell codes (0 = F or S, 1 = W, 2 = H, 3 = G); action 0..3 = left, down,
 * right, up, clipped to the grid; the env stays put on a wall or when already on H
 * or G; reward 1 on G, else 0; done on H or G.  The observation is the one-hot of
 * the cell (obs_dim = rows * cols); reset puts env i on start[i]. */
typedef struct {
  int64_t n;
  int32_t rows, cols, max_episode_length, pad_;
  const uint8_t* map;   /* [n, rows * cols] */
  const int32_t* start; /* [n] */
  int32_t* state;       /* [n] current cell */
  int32_t* t;           /* [n] steps taken in the current episode */
} ga_grid_env;

/* MultiEnvWrapper([PointEnv(goal=task_goals[k], ...) for k < num_tasks], strategy, mode)
 * (envs/multi_env_wrapper.py:169-226), one wrapper per member.  The fields of
 * ga_point_env (the other PointEnv parameters are shared by the tasks) plus the task
 * layer: every reset -- ga_env_reset, and the reset of a finished env
 * inside ga_env_step_record -- picks the member's next task from its own last_task
 * (round robin: 0 after -1, else (last + 1) % num_tasks; uniform random: the first
 * word of Philox4x32-10 keyed (seed; env index, the member's reset counter), scaled
 * to [0, num_tasks) by the high half of u * num_tasks -- the reference draws from
 * Python's global `random` there), copies task_goals[task] into goal[i] and resets
 * the PointEnv.  mode GA_TASK_ADD_ONEHOT: obs_dim = 3 + num_tasks, the one-hot of the
 * active task follows the PointEnv observation on reset and on every step (the
 * observation of an episode's last step carries that episode's task);
 * GA_TASK_VANILLA: obs_dim = 3.  `task_id` (optional) receives env_info['task_id']
 * as uint8, addressed like `success`; num_tasks is 1..256. */
#define GA_TASK_ROUND_ROBIN 0
#define GA_TASK_UNIFORM_RANDOM 1
#define GA_TASK_VANILLA 0
#define GA_TASK_ADD_ONEHOT 1
typedef struct {
  int64_t n;
  float arena_size, done_bonus;
  int32_t never_done, max_episode_length;
  float* point;      /* [n, 2] */
  float* goal;       /* [n, 2] the active task's goal, written at reset */
  int32_t* t;        /* [n] steps taken in the current episode */
  uint8_t* success;  /* optional, as in ga_point_env */
  int32_t num_tasks, strategy, mode, pad_;
  uint64_t seed;
  const float* task_goals; /* [num_tasks, 2] */
  int32_t* last_task;      /* [n] active task, -1 before the first reset */
  uint32_t* resets;        /* [n] resets so far */
  uint8_t* task_id;        /* optional, see above */
} ga_multi_point_env;

/* Host-only (no GPU needed): the task the uniform random strategy gives env `env_id`
 * at its reset number `counter` (< 0: num_tasks outside 1..256). */
GA_API int ga_multi_env_task_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                  int num_tasks);

/* CartPole (gym's CartPole-v1: Barto, Sutton and Anderson's cart-pole, Euler step),
 * observation = state (x, x_dot, theta, theta_dot), obs_dim 4, one action column
 * holding a class index: 1 pushes right, anything else left.  Reward 1 on every step,
 * the terminating one included.
 *
 * The arithmetic is fixed here, so that a numpy twin (garage_amd.envs.CartPoleEnv)
 * and the kernels give the same bits: every operation below is ONE fp32 operation,
 * rounded to nearest on its own (no fused multiply-add, correctly rounded division),
 * evaluated in the order the parentheses give; a constant written (float)(expr) is
 * the double value of expr rounded to fp32.  sin and cos are fixed polynomials, not
 * library calls: an episode ends once |theta| passes 0.2094, so |theta| < 0.3 at every
 * step, where their truncation error is below 1e-10.
 *
 *   force = action == 1 ? 10.0f : -10.0f
 *   t2 = th * th
 *   sn = th * (1.0f + t2 * (S3 + t2 * (S5 + t2 * S7)))
 *   cs = 1.0f + t2 * (C2 + t2 * (C4 + t2 * (C6 + t2 * C8)))
 *     S3 = (float)(-1.0 / 6.0), S5 = (float)(1.0 / 120.0), S7 = (float)(-1.0 / 5040.0),
 *     C2 = -0.5f, C4 = (float)(1.0 / 24.0), C6 = (float)(-1.0 / 720.0),
 *     C8 = (float)(1.0 / 40320.0)
 *   temp   = (force + ((0.05f * (thd * thd)) * sn)) / 1.1f
 *   th_acc = ((9.8f * sn) - (cs * temp)) /
 *            (0.5f * ((float)(4.0 / 3.0) - ((0.1f * (cs * cs)) / 1.1f)))
 *   x_acc  = temp - (((0.05f * th_acc) * cs) / 1.1f)
 *   x'   = x + (0.02f * xd)        xd'  = xd + (0.02f * x_acc)
 *   th'  = th + (0.02f * thd)      thd' = thd + (0.02f * th_acc)
 *   done = |x'| > 2.4f || |th'| > (float)(12.0 * 2.0 * 3.141592653589793 / 360.0)
 *   step type: TIMEOUT when the episode reaches max_episode_length (1..65535), else
 *   TERMINAL when done, as for the other envs.
 *
 * Reset number c (= resets[i], which then advances) of env i takes the four words
 * w_0..w_3 of Philox4x32-10 with counter (env_id0 + i, c, 0, 5 << 16) -- stream 5 --
 * and key (seed & 0xffffffff, seed >> 32):
 *   u_j = ((float)(w_j >> 8) + 0.5f) * 0x1p-24f,   state[j] = -0.05f + (0.1f * u_j)
 * (gym draws U(-0.05, 0.05) from its np_random).  ga_cartpole_reset_draw below gives
 * the same four values on the host. */
typedef struct {
  int64_t n, env_id0;
  int32_t max_episode_length, pad_;
  uint64_t seed;
  float* state;     /* [n, 4] x, x_dot, theta, theta_dot */
  int32_t* t;       /* [n] steps taken in the current episode */
  uint32_t* resets; /* [n] resets so far */
} ga_cartpole_env;

/* Host-only (no GPU needed): the state reset number `counter` gives env `env_id`
 * (= env_id0 + i) of a ga_cartpole_env with this seed. */
GA_API int ga_cartpole_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                  float out4[4]);

/* Pendulum (gym 0.17's Pendulum-v0: g = 10, m = l = 1, dt = 0.05, speed clipped to
 * [-8, 8], torque to [-2, 2]), observation (cos th, sin th, thdot), obs_dim 3, one
 * action column holding the torque (the env clips it; any float may be passed).  An
 * episode never terminates: the step that reaches max_episode_length (1..65535) is
 * TIMEOUT.
 *
 * The arithmetic is fixed here as CartPole's is above: every operation below is ONE
 * fp32 operation, rounded to nearest on its own (no fused multiply-add), evaluated in
 * the order the parentheses give; a constant written (float)(expr) is the double value
 * of expr rounded to fp32.  The state is (th, thd) with th kept in [-PI, PI]:
 *
 *   PI = (float)3.141592653589793   TWO_PI = (float)6.283185307179586 ( = 2 PI exactly)
 *   HALF_PI = (float)1.5707963267948966
 *
 * sincos(th), |th| <= PI: the angle is folded to |r| <= HALF_PI (+ half an ulp of PI),
 * where the two fixed Horner polynomials -- not library calls -- stay within 2e-7 of
 * sin and cos:
 *   th >  HALF_PI: r = PI - th,    sg = -1
 *   th < -HALF_PI: r = (-PI) - th, sg = -1
 *   else           r = th,         sg =  1
 *   t2 = r * r
 *   sp = r * (1.0f + t2 * (S3 + t2 * (S5 + t2 * (S7 + t2 * (S9 + t2 * (S11 + t2 * S13))))))
 *   sn = sp < -1.0f ? -1.0f : (sp > 1.0f ? 1.0f : sp)   (sp reaches 1 + 2^-23 next to
 *                                                        +-HALF_PI; cs cannot pass 1)
 *   cs = sg * (1.0f + t2 * (C2 + t2 * (C4 + t2 * (C6 + t2 * (C8 + t2 * (C10 +
 *                                                     t2 * (C12 + t2 * C14)))))))
 *     S(2k+1) = (float)((-1)^k / (2k+1)!):  S3 = (float)(-1.0 / 6.0), S5 = (float)(1.0 /
 *     120.0), S7 = (float)(-1.0 / 5040.0), S9 = (float)(1.0 / 362880.0), S11 =
 *     (float)(-1.0 / 39916800.0), S13 = (float)(1.0 / 6227020800.0)
 *     C(2k) = (float)((-1)^k / (2k)!):  C2 = -0.5f, C4 = (float)(1.0 / 24.0), C6 =
 *     (float)(-1.0 / 720.0), C8 = (float)(1.0 / 40320.0), C10 = (float)(-1.0 /
 *     3628800.0), C12 = (float)(1.0 / 479001600.0), C14 = (float)(-1.0 / 87178291200.0)
 *
 * step with action a (th, thd: the state BEFORE the step):
 *   u    = a < -2.0f ? -2.0f : (a > 2.0f ? 2.0f : a)
 *   sn   = the sine of sincos(th)
 *   cost = ((th * th) + (0.1f * (thd * thd))) + (0.001f * (u * u))
 *   v    = thd + (((15.0f * sn) + (3.0f * u)) * 0.05f)
 *   nth  = th + (v * 0.05f)                 (the UNCLIPPED new speed: Pendulum-v0's order)
 *   nthd = v < -8.0f ? -8.0f : (v > 8.0f ? 8.0f : v)
 *   nth >= PI: nth = nth - TWO_PI;   nth < -PI: nth = nth + TWO_PI
 *   (cs', sn') = sincos(nth)
 *   observation = (cs', sn', nthd), reward = -cost, state = (nth, nthd)
 * |v * 0.05f| <= 0.4525, so one wrap is enough; gym's angle_normalize of a wrapped angle
 * is the angle itself, and the observation is periodic: the wrap leaves the dynamics
 * as they are.
 *
 * Reset number c (= resets[i], which then advances) of env i takes the words w_0, w_1
 * of Philox4x32-10 with counter (env_id0 + i, c, 0, 6 << 16) -- stream 6 -- and key
 * (seed & 0xffffffff, seed >> 32):
 *   u_j = ((float)(w_j >> 8) + 0.5f) * 0x1p-24f
 *   th  = (-PI) + (TWO_PI * u_0)            (may round to exactly PI)
 *   thd = -1.0f + (2.0f * u_1)
 * (gym draws th ~ U(-pi, pi), thdot ~ U(-1, 1) from its np_random); the first
 * observation is (sincos(th), thd).  ga_pendulum_reset_draw below gives (th, thd) on
 * the host. */
typedef struct {
  int64_t n, env_id0;
  int32_t max_episode_length, pad_;
  uint64_t seed;
  float* state;     /* [n, 2] theta, theta_dot */
  int32_t* t;       /* [n] steps taken in the current episode */
  uint32_t* resets; /* [n] resets so far */
} ga_pendulum_env;

/* Host-only (no GPU needed): the state (th, thd) reset number `counter` gives env
 * `env_id` (= env_id0 + i) of a ga_pendulum_env with this seed. */
GA_API int ga_pendulum_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                  float out2[2]);

/* Inverted double pendulum on a cart (the task of gym's InvertedDoublePendulum-v2: a
 * cart on a rail carrying two uniform rods, upright at rest), obs_dim 11, one action
 * column holding the push in [-1, 1] (the env clips it; any float may be passed).
 * MuJoCo cannot be matched bit for bit, so the env is this model of the same machine,
 * with these deviations from MuJoCo's: the capsule masses rounded (10.5 for the cart,
 * 4.2 for each rod of length 0.6, g = 9.81), no joint damping (the XML has 0.05), no
 * rail stops, semi-implicit Euler instead of RK4, uniform instead of Gaussian start
 * velocities, and zeros where MuJoCo reports its constraint forces.
 *
 * The arithmetic is fixed here as CartPole's and Pendulum's are above: every operation
 * below is ONE fp32 operation, rounded to nearest on its own (no fused multiply-add,
 * correctly rounded division), evaluated in the order the parentheses give; a constant
 * written (float)(expr) is the double value of expr rounded to fp32; sincos, PI and
 * TWO_PI are Pendulum's.  The state is (x, th1, th2, xd, th1d, th2d); th1 and th2 are
 * the rods' ABSOLUTE angles from the upright, positive towards +x, kept in [-PI, PI].
 *
 *   D1 = (float)(10.5 + 4.2 + 4.2)                  D2 = (float)((4.2 / 2.0 + 4.2) * 0.6)
 *   D3 = (float)(4.2 * 0.6 / 2.0)                   D4 = (float)((4.2 / 3.0 + 4.2) * 0.6 * 0.6)
 *   D5 = (float)(4.2 * 0.6 * 0.6 / 2.0)             D6 = (float)(4.2 * 0.6 * 0.6 / 3.0)
 *   F1 = (float)((4.2 / 2.0 + 4.2) * 0.6 * 9.81)    F2 = (float)(4.2 * 0.6 * 9.81 / 2.0)
 *   (18.9, 3.78, 1.26, 2.016, 0.756, 0.504, 37.0818, 12.3606 rounded to fp32)
 *   clip(v, b) = v < -b ? -b : (v > b ? b : v)
 *   wrap(th):  th >= PI: th - TWO_PI;   th < -PI: th + TWO_PI;   else th
 *
 * step with action a:
 *   F = 500.0f * clip(a, 1.0f)
 * then FIVE times, on the running state (the equations of motion D(q) qdd = r of the
 * three bodies, solved by one LDL^T elimination without pivoting: the condition number
 * of D is 39..108 over all angles):
 *   (s1, c1) = sincos(th1)      (s2, c2) = sincos(th2)
 *   cd = (c1 * c2) + (s1 * s2)              sd = (s1 * c2) - (c1 * s2)
 *   q1 = th1d * th1d                        q2 = th2d * th2d
 *   a12 = D2 * c1      a13 = D3 * c2        a23 = D5 * cd
 *   r1 = (F + ((D2 * s1) * q1)) + ((D3 * s2) * q2)
 *   e1 = D5 * sd
 *   r2 = (F1 * s1) - (e1 * q2)
 *   r3 = (F2 * s2) + (e1 * q1)
 *   l21 = a12 / D1                          l31 = a13 / D1
 *   p22 = D4 - (l21 * a12)                  t23 = a23 - (l21 * a13)
 *   t33 = D6 - (l31 * a13)                  l32 = t23 / p22
 *   p33 = t33 - (l32 * t23)
 *   y2 = r2 - (l21 * r1)                    y3 = (r3 - (l31 * r1)) - (l32 * y2)
 *   z1 = r1 / D1       z2 = y2 / p22        acc3 = y3 / p33
 *   acc2 = z2 - (l32 * acc3)                acc1 = (z1 - (l21 * acc2)) - (l31 * acc3)
 *   xd   = clip(xd   + (0.01f * acc1), 100.0f)
 *   th1d = clip(th1d + (0.01f * acc2), 100.0f)
 *   th2d = clip(th2d + (0.01f * acc3), 100.0f)      (a guard: free runs stay below 14)
 *   x   = x + (0.01f * xd)                          (the NEW speeds: semi-implicit Euler)
 *   th1 = wrap(th1 + (0.01f * th1d))        th2 = wrap(th2 + (0.01f * th2d))
 * (|0.01f * v| <= 1, so one wrap is enough), and on the state they leave:
 *   (s1, c1) = sincos(th1)      (s2, c2) = sincos(th2)
 *   cd = (c1 * c2) + (s1 * s2)              sd = (s1 * c2) - (c1 * s2)
 *   yt = (0.6f * c1) + (0.6f * c2)          xt = (x + (0.6f * s1)) + (0.6f * s2)
 *   dist = (0.01f * (xt * xt)) + ((yt - 2.0f) * (yt - 2.0f))
 *   w2  = th2d - th1d                       (MuJoCo's second joint speed; its first is th1d)
 *   vel = (0.001f * (th1d * th1d)) + (0.005f * (w2 * w2))
 *   reward = (10.0f - dist) - vel           (the terminating step keeps its reward)
 *   done = yt <= 1.0f
 *   observation = (x, s1, -sd, c1, cd, clip(xd, 10.0f), clip(th1d, 10.0f),
 *                  clip(w2, 10.0f), 0, 0, 0)
 *   (-sd = sin(th2 - th1), cd = cos(th2 - th1): the reference task's layout
 *   (x, sin q1, sin q2, cos q1, cos q2, clipped joint speeds, constraint forces) with
 *   MuJoCo's relative second joint angle q2 = th2 - th1)
 *   step type: TIMEOUT when the episode reaches max_episode_length (1..65535), else
 *   TERMINAL when done, as for the other envs.
 *
 * Reset number c (= resets[i], which then advances) of env i takes the words w_0..w_3
 * of Philox4x32-10 with counter (env_id0 + i, c, 0, 7 << 16) and w_4, w_5, the first two
 * words with counter (env_id0 + i, c, 1, 7 << 16) -- stream 7 -- and key
 * (seed & 0xffffffff, seed >> 32):
 *   u_j = ((float)(w_j >> 8) + 0.5f) * 0x1p-24f,   state[j] = -0.1f + (0.2f * u_j)
 * the first observation is the observation above of that state.
 * ga_double_pendulum_reset_draw below gives the six values on the host. */
typedef struct {
  int64_t n, env_id0;
  int32_t max_episode_length, pad_;
  uint64_t seed;
  float* state;     /* [n, 6] x, th1, th2, xd, th1d, th2d */
  int32_t* t;       /* [n] steps taken in the current episode */
  uint32_t* resets; /* [n] resets so far */
} ga_double_pendulum_env;

/* Host-only (no GPU needed): the state reset number `counter` gives env `env_id`
 * (= env_id0 + i) of a ga_double_pendulum_env with this seed. */
GA_API int ga_double_pendulum_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                         float out6[6]);

/* Acrobot (gym 0.17's Acrobot-v1: two unit links, unit masses, centres of mass at 0.5,
 * moments of inertia 1, g = 9.8, the "book" dynamics, no torque noise, dt = 0.2),
 * observation (cos th1, sin th1, cos th2, sin th2, thd1, thd2), obs_dim 6, one action
 * column holding a class index k: 0 is torque a = -1.0f, 2 is a = 1.0f, anything else
 * (1, and any index out of range) a = 0.0f.  th1 is the first link's angle from hanging
 * straight down, th2 the second link's angle relative to the first.
 *
 * The arithmetic is fixed here as CartPole's and Pendulum's are above: every operation
 * below is ONE fp32 operation, rounded to nearest on its own (no fused multiply-add,
 * correctly rounded division), evaluated in the order the parentheses give; a constant
 * written (float)(expr) is the double value of expr rounded to fp32; sincos, PI and
 * TWO_PI are Pendulum's.  The state is (th1, th2, w1, w2) with both angles kept in
 * [-PI, PI], |w1| <= V1 and |w2| <= V2:
 *
 *   V1 = (float)(4.0 * 3.141592653589793)      V2 = (float)(9.0 * 3.141592653589793)
 *   clip(v, b) = v < -b ? -b : (v > b ? b : v)
 *
 * reduce(th), any stage angle -> [-PI, PI]:
 *   k = rintf(th * (float)(1.0 / 6.283185307179586))       (round half to even)
 *   r = (th - (k * R_HI)) - (k * R_LO)
 *     R_HI = 6.28125f   R_LO = (float)(6.283185307179586 - 6.28125)
 *   r >= PI: r = r - TWO_PI;   r < -PI: r = r + TWO_PI
 * The stage angles of the RK4 step below are NOT in [-PI, PI]: the accelerations reach
 * thousands at the speed bounds, and over the whole state box and the three torques
 * the largest |stage angle| (the angle after the step, before its reduce, included) is
 * 33.32, at (th1, th2, w1, w2) = (-+1.598, +-1.980, +-V1, +-V2), found by a random search
 * of 4e6 states plus local refinement over the float64 equations; reduce is trusted,
 * and tested, on |th| <= 34 (|k| <= 5).  The two-constant form is a change to the
 * proposal r = th - (k * TWO_PI): R_HI has 9 significant bits, so k * R_HI and the first
 * subtraction are exact and the error of r is half an ulp of PI plus |k| * 1e-10, where
 * the one-constant form adds the rounding of k * TWO_PI and |k| times TWO_PI's own
 * 1.7e-7.  Measured over |th| <= 34 against float64 sin / cos of the same fp32 angle:
 * reduce + sincos within 2.2e-7 / 2.5e-7, the one-constant form within 1.4e-6 / 1.6e-6,
 * for two more operations per reduction.
 *
 * f(th1, th2, w1, w2) with torque a = (w1, w2, acc1, acc2):
 *   (s1, c1) = sincos(reduce(th1))          (s2, c2) = sincos(reduce(th2))
 *   d1 = 3.5f + c2                          d2 = 1.25f + (0.5f * c2)
 *   s12 = (s1 * c2) + (c1 * s2)             (sin(th1 + th2): no sincos of a sum)
 *   phi2 = 4.9f * s12
 *   phi1 = (((-0.5f * (w2 * w2)) * s2) - ((w2 * w1) * s2)) + ((14.7f * s1) + phi2)
 *   r    = d2 / d1
 *   acc2 = (((a + (r * phi1)) - ((0.5f * (w1 * w1)) * s2)) - phi2) / (1.25f - (d2 * r))
 *   acc1 = -(((d2 * acc2) + phi1) / d1)
 *   (1.25f - (d2 * r) lies in [0.56, 1.03] for every c2 in [-1, 1])
 *
 * step with action class k, y = (th1, th2, w1, w2) the state before it, one classical
 * RK4 step of 0.2 (each line for all four components j):
 *   k1 = f(y)
 *   k2 = f(y + (0.1f * k1))       k3 = f(y + (0.1f * k2))       k4 = f(y + (0.2f * k3))
 *   sum_j = ((k1_j + (2.0f * k2_j)) + (2.0f * k3_j)) + k4_j
 *   y'_j  = y_j + ((float)(0.2 / 6.0) * sum_j)
 *   th1 = reduce(y'_0)    th2 = reduce(y'_1)    w1 = clip(y'_2, V1)    w2 = clip(y'_3, V2)
 * and on the state that leaves:
 *   (s1, c1) = sincos(th1)                  (s2, c2) = sincos(th2)
 *   done = ((-c1) - ((c1 * c2) - (s1 * s2))) > 1.0f
 *   reward = done ? 0.0f : -1.0f
 *   observation = (c1, s1, c2, s2, w1, w2)
 *   step type: TIMEOUT when the episode reaches max_episode_length (1..65535), else
 *   TERMINAL when done, as for the other envs.
 *
 * Reset number c (= resets[i], which then advances) of env i takes the words w_0..w_3
 * of Philox4x32-10 with counter (env_id0 + i, c, 0, 8 << 16) -- stream 8 -- and key
 * (seed & 0xffffffff, seed >> 32):
 *   u_j = ((float)(w_j >> 8) + 0.5f) * 0x1p-24f,   state[j] = -0.1f + (0.2f * u_j)
 * (gym draws the four from U(-0.1, 0.1) of its np_random); the first observation is the
 * observation above of that state.  ga_acrobot_reset_draw below gives the four values
 * on the host. */
typedef struct {
  int64_t n, env_id0;
  int32_t max_episode_length, pad_;
  uint64_t seed;
  float* state;     /* [n, 4] th1, th2, thd1, thd2 */
  int32_t* t;       /* [n] steps taken in the current episode */
  uint32_t* resets; /* [n] resets so far */
} ga_acrobot_env;

/* Host-only (no GPU needed): the state reset number `counter` gives env `env_id`
 * (= env_id0 + i) of a ga_acrobot_env with this seed. */
GA_API int ga_acrobot_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                 float out4[4]);

/* MountainCar (gym 0.17's MountainCar-v0, and with continuous = 1 its
 * MountainCarContinuous-v0), state and observation (x, v), obs_dim 2, one action column:
 * a class index k (0 pushes left, p = -1.0f; 2 pushes right, p = 1.0f; anything else
 * coasts, p = 0.0f), or with continuous = 1 the force a (the env clips it; any float may
 * be passed).  Whether the env takes a class index or a force is this struct's field,
 * not its kind's.
 *
 * The arithmetic is fixed as above (one fp32 operation at a time, no fused
 * multiply-add, the order the parentheses give); sincos, PI and TWO_PI are Pendulum's,
 * clip is Acrobot's.  x is kept in [-1.2f, 0.6f] and v in [-0.07f, 0.07f].
 *
 * step:
 *   g = 3.0f * x;   g >= PI: g = g - TWO_PI;   g < -PI: g = g + TWO_PI
 *   cs = the cosine of sincos(g)     (3 x lies in [-3.6, 1.8]: one wrap is enough)
 *   continuous == 0:   v1 = v + ((p * 0.001f) + (cs * -0.0025f))
 *   continuous == 1:   v1 = v + ((clip(a, 1.0f) * 0.0015f) - (0.0025f * cs))
 *   v' = clip(v1, 0.07f)
 *   x1 = x + v'
 *   x' = x1 < -1.2f ? -1.2f : (x1 > 0.6f ? 0.6f : x1)
 *   x' == -1.2f and v' < 0.0f:  v' = 0.0f          (the left wall)
 *   continuous == 0:   done = x' >= 0.5f and v' >= 0.0f      reward = -1.0f (every step)
 *   continuous == 1:   done = x' >= 0.45f and v' >= 0.0f
 *                      reward = (done ? 100.0f : 0.0f) - (0.1f * (a * a))
 *                      (the UNCLIPPED a, as in gym)
 *   observation = state = (x', v')
 *   step type: TIMEOUT when the episode reaches max_episode_length (1..65535; gym's
 *   limits are 200 and, continuous, 999), else TERMINAL when done.
 *
 * Reset number c (= resets[i], which then advances) of env i takes the word w_0 of
 * Philox4x32-10 with counter (env_id0 + i, c, 0, 9 << 16) -- stream 9 -- and key
 * (seed & 0xffffffff, seed >> 32):
 *   u_0 = ((float)(w_0 >> 8) + 0.5f) * 0x1p-24f,   x = -0.6f + (0.2f * u_0),   v = 0.0f
 * (gym draws x ~ U(-0.6, -0.4) from its np_random); the first observation is (x, v).
 * ga_mountain_car_reset_draw below gives (x, v) on the host. */
typedef struct {
  int64_t n, env_id0;
  int32_t max_episode_length;
  int32_t continuous; /* 0: MountainCar-v0, 1: MountainCarContinuous-v0 */
  uint64_t seed;
  float* state;     /* [n, 2] x, v */
  int32_t* t;       /* [n] steps taken in the current episode */
  uint32_t* resets; /* [n] resets so far */
} ga_mountain_car_env;

/* Host-only (no GPU needed): the state (x, v) reset number `counter` gives env `env_id`
 * (= env_id0 + i) of a ga_mountain_car_env with this seed (either variant). */
GA_API int ga_mountain_car_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                      float out2[2]);

/* Any device env: `env` points to a ga_synth_env, ga_point_env, ga_grid_env,
 * ga_multi_point_env, ga_cartpole_env, ga_pendulum_env, ga_double_pendulum_env,
 * ga_acrobot_env or ga_mountain_car_env. */
#define GA_ENV_SYNTH 0
#define GA_ENV_POINT 1
#define GA_ENV_GRID 2
#define GA_ENV_MULTI_POINT 3
#define GA_ENV_CARTPOLE 4
#define GA_ENV_PENDULUM 5
#define GA_ENV_DOUBLE_PENDULUM 6
/* (7 and 9 are not kinds, and will not become kinds: callers and the tests of the
 * earlier kinds rely on both being refused as "unknown env kind") */
#define GA_ENV_ACROBOT 8
#define GA_ENV_MOUNTAIN_CAR 10
typedef struct {
  int32_t kind, pad_;
  const void* env;
} ga_env_ref;

/* One thread per env, one launch per call, for every env kind.
 * ga_env_reset: Environment.reset of the envs with mask != 0 (mask == NULL: all); obs
 * [n, ldo] receives their first observations (envs/point_env.py:79-98,
 * grid_world_env.py:91-109, multi_env_wrapper.py:169-194).
 * ga_env_step: Environment.step with actions [n, lda] into next_obs, reward [n] and
 * step_type [n] (envs/point_env.py:100-170, grid_world_env.py:111-215,
 * multi_env_wrapper.py:196-226); `obs`, the current observations, is read by the
 * synthetic env only (the state of the others is their own).
 * ga_env_step_record: ga_env_step -> NormalizedEnv statistics of `norm` (may be
 * NULL; normalized_env.py:134-164) -> ga_record_step -> ga_env_reset of the finished
 * envs in one launch, same per-env results (vec_worker.py:176-204): rec->next_obs
 * receives the next observation, or the first one of the new episode where one
 * ended. */
GA_API int ga_env_reset(const ga_env_ref* env, const uint8_t* mask, float* obs, int64_t ldo,
                        ga_stream_t stream);
GA_API int ga_env_step(const ga_env_ref* env, const float* actions, int64_t lda,
                       const float* obs, float* next_obs, int64_t ldo, float* reward,
                       uint8_t* step_type, ga_stream_t stream);
GA_API int ga_env_step_record(const ga_env_ref* env, const ga_record_args* rec,
                              const ga_norm_args* norm, const float* actions, int64_t lda,
                              const float* obs, ga_stream_t stream);

/* ga_policy_step_fused_f32 followed, per env and in the same launch, by what
 * ga_env_step_record does (env step with `head->action`, NormalizedEnv
 * statistics, bookkeeping, reset of the finished envs), for n_steps consecutive
 * rollout steps in ONE launch: a workgroup takes its 16 envs
 * through all of them (envs do not interact within a rollout), alternating between
 * the buffers head->obs / rec->next_obs (norm: raw_obs / raw_next_obs); columns
 * head->col .. head->col + n_steps - 1, Philox counters head->step + s.  Device
 * noise only (head->noise must be null for n_steps > 1).
 * With norm->act_low set the thread that sampled an env's action also rescales it
 * (ga_action_rescale_f32's arithmetic, the same function) into its row of
 * norm->scaled_action and steps the env on that row.  Refused before any device call:
 * act_low without act_high or without scaled_action, or with an env kind whose action
 * is a class index ("action rescale needs bounds, scratch and a continuous action
 * space"); a head of another width than the env's action. */
GA_API int ga_policy_env_step_fused_f32(const ga_mlp_desc* d, const float* params,
                                        const ga_head_args* head, const ga_env_ref* env,
                                        const ga_record_args* rec, const ga_norm_args* norm,
                                        int64_t n_steps, ga_stream_t stream);
/* The same launch behind a POPULATION of parameter vectors: member m (0 <= m <
 * n_members) owns the envs [m g, (m + 1) g), g = head->n / n_members, and its
 * workgroups read every weight, bias, LayerNorm gain and the Gaussian head's log-std
 * from params + m * member_stride (floats; each vector in the layout `d` describes).
 * Nothing else differs: one env batch, one set of rollout buffers, Philox counters by
 * env id.  Refused before any launch (negative return, ga_last_error): n_members < 1;
 * head->n not a multiple of n_members; with n_members > 1, g not a multiple of the 16
 * envs a workgroup owns; member_stride not a multiple of 4 or smaller than the
 * vector `d` describes; 2^31 floats or more up to the last member's end; head->noise;
 * norm->act_low (a population is not rescaled: the refusal stands, with its wording,
 * though the kernel could); a network the fused step does
 * not take.  n_members == 1 is
 * ga_policy_env_step_fused_f32.  ga_launch_count(13) counts every call with
 * n_steps > 1 once. */
GA_API int ga_policy_env_step_members_f32(const ga_mlp_desc* d, const float* params,
                                          const ga_head_args* head, const ga_env_ref* env,
                                          const ga_record_args* rec,
                                          const ga_norm_args* norm, int64_t n_steps,
                                          int64_t n_members, int64_t member_stride,
                                          ga_stream_t stream);
/* 1 (default): ga_rollout_env_steps takes that launch, the action rescale of
 * norm->act_low included; 0: policy step and env step as two launches, with
 * ga_action_rescale_f32 as a third between them under norm->act_low. */
GA_API int ga_set_fused_env_step(int on);
/* n_steps consecutive vectorised steps (fused policy step, env step,
 * bookkeeping, reset of finished envs) starting at head->col / head->step,
 * alternating the observation buffers obs_a (current) / obs_b; after an odd
 * number of steps the current observations are in obs_b.  The while-loop body of
 * VecWorker.rollout (sampler/default_worker.py:176-186 + vec_worker.py:176-204)
 * enqueued natively.  With norm != NULL (NormalizedEnv around the env)
 * obs_a / obs_b hold the normalised observations and raw_a / raw_b, alternating
 * the same way, the env's own; with norm->act_low the env steps on the rescaled
 * actions (norm->scaled_action) in either form of the loop, bit for bit the same.
 * One launch for all n_steps unless ga_set_fused_env_step(0) or head->noise. */
GA_API int ga_rollout_env_steps(const ga_mlp_desc* desc, const float* params,
                                const ga_head_args* head, const ga_env_ref* env,
                                const ga_record_args* rec, float* obs_a, float* obs_b,
                                const ga_norm_args* norm, float* raw_a, float* raw_b,
                                int64_t n_steps, ga_stream_t stream);

/* EpisodeBatch.concatenate in completion order (sampler/vec_worker.py:206-219,
 * local_sampler.py:134-166; order = (completion step, env index)).
 * ga_pack_src_index writes the flat cell env * Tcap + column of every packed sample
 * as int32, and the gathers read such cells: the caller must guarantee
 * n * Tcap < 2^31 for the n envs of its buffers.  The entry sees Tcap and the episodes
 * only and refuses Tcap outside 1..2^31 - 1 and n_eps outside 1..2^31 - 1. */
GA_API int ga_pack_episodes(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                            int64_t n_steps, const int32_t* ep_base, int32_t* ep_env,
                            int32_t* ep_end, int32_t* ep_len, ga_stream_t stream);
GA_API int ga_pack_src_index(const int32_t* ep_env, const int32_t* ep_end,
                             const int32_t* ep_len, const int64_t* ep_off, int64_t n_eps,
                             int64_t Tcap, int32_t* src, ga_stream_t stream);
GA_API int ga_gather_rows_f32(const float* src, int64_t ld_src, const int32_t* idx,
                              int64_t rows, int64_t width, float* dst, int64_t ld_dst,
                              ga_stream_t stream);
GA_API int ga_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst,
                         ga_stream_t stream);
GA_API int ga_gather_u8(const uint8_t* src, const int32_t* idx, int64_t n, uint8_t* dst,
                        ga_stream_t stream);
/* Minibatch id permutation of BatchDataset
 * (np/optimizers/minibatch_dataset.py:4-35), throughput mode: a keyed Feistel
 * permutation of [0, n) evaluated on the device (the parity mode ships the host
 * np.random.shuffle ids instead). */
GA_API int ga_permutation_i32(int64_t n, uint64_t key, int32_t* out, ga_stream_t stream);
/* undiscounted return per episode (log_performance, _functions.py:233-275) */
GA_API int ga_episode_sums_f32(const float* rewards, const int64_t* ep_off, int64_t n_eps,
                               double* sums, ga_stream_t stream);

/* ---- a population's score from the raw rollout buffers -------------------------
 * The buffers are the ones ga_policy_env_step_members_f32 fills: tail_buf [n, Tcap]
 * (an episode's length at its last cell, else 0), columns [0, n_cols) stepped so far;
 * member m owns the rows [m g, (m + 1) g), g = n / n_members (any g >= 1).
 *
 * progress[3 m ..] = {c_m, episodes, samples} per member: c_m is the first column
 * count at which the episodes the member has completed hold >= num_samples steps --
 * the columns GpuPopulationSampler.obtain_samples keeps -- or 0 when that is not
 * reached within n_cols; `episodes` those that ended in [0, c_m) (in [0, n_cols)
 * while c_m == 0); `samples` the steps of all episodes completed in [0, n_cols).
 * col_base [n_members, Tcap] (workspace): per member and column t < n_cols, its
 * episodes that ended before t.  One launch; the caller copies 3 n_members integers.
 * Refused before any launch: NULL pointers; n_members < 1; n not a multiple of
 * n_members; n_cols outside 1..Tcap; num_samples < 1; n * Tcap >= 2^31. */
GA_API int ga_member_progress(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                              int64_t n_cols, int64_t n_members, int64_t num_samples,
                              int32_t* progress, int32_t* col_base, ga_stream_t stream);
/* What log_performance (_functions.py:233-275) reduces an episode to, for every
 * episode of member m that ended in a column < c_m, written compactly in the order
 * (member, end column, env index) -- ga_pack_episodes' order within a member; a member
 * with c_m == 0 contributes none, nor do episodes in flight.  Two launches:
 * ga_member_progress' (progress and col_base are written as above) and the statistics.
 *   length        the episode's steps
 *   undiscounted  its rewards (rew_buf [n, Tcap] f32) added in time order into an fp64
 *                 accumulator: ga_episode_sums_f32's sum (_functions.py:253)
 *   discounted    ret = (double)r_t + discount * ret from the last step back to the
 *                 first, product and sum rounded once each (no fused multiply-add):
 *                 the first element of discount_cumsum (_functions.py:250-252) in the
 *                 host's own fp64 arithmetic
 *   terminated    1 when a step of st_buf [n, Tcap] is StepType.TERMINAL
 *                 (_functions.py:254-256)
 *   success       1 when a step's flag in success_buf [n, Tcap] is set
 *                 (_functions.py:257-259); success_buf NULL: the env records none and
 *                 `success` is not written (it may be NULL)
 * max_eps: the episodes the output arrays hold; nothing is written past it.
 * Refusals: as ga_member_progress, and max_eps < 1. */
GA_API int ga_member_episode_statistics(
    const float* rew_buf, const uint8_t* st_buf, const uint16_t* tail_buf,
    const uint8_t* success_buf, int64_t n, int64_t Tcap, int64_t n_cols,
    int64_t n_members, int64_t num_samples, double discount, int32_t* progress,
    int32_t* col_base, int64_t max_eps, int32_t* length, double* undiscounted,
    double* discounted, uint8_t* terminated, uint8_t* success, ga_stream_t stream);

/* ---- a population's episodes packed in one pass over the rollout buffers --------
 * EpisodeBatch.concatenate (sampler/vec_worker.py:206-219, local_sampler.py:134-166)
 * for every member at once: what ga_pack_episodes, ga_pack_src_index and the gathers do
 * for one member's rows, for all of them, from `progress` and `col_base` as
 * ga_member_progress wrote them for the same tail_buf, n_cols and num_samples.  Both
 * entries are graph-capture safe: they allocate nothing, copy nothing to the host and
 * do not synchronise.
 *
 * ga_member_pack_index (two launches) writes, for every episode of member m that ended
 * in a column < c_m, in the order (member, end column, env index) --
 * ga_pack_episodes' inside a member, ga_member_episode_statistics' overall; a member
 * with c_m == 0 contributes no episode:
 *   ep_env, ep_end, ep_len  int32 [max_eps]: the GLOBAL env index, the last column and
 *                 the length of episode e = episode_start[m] + (its rank in the
 *                 member), episode_start[m] the episodes of the members before m
 *   ep_off        int64 [max_eps + n_members]: member m owns the episodes_m + 1 entries
 *                 from episode_start[m] + m, relative to the member's first sample:
 *                 they start at 0 and end at S_m (a lone batch's ep_off)
 *   member_samples int64 [n_members]: S_m, the steps of the member's episodes
 *   member_off    int64 [n_members + 1]: the member's first row in the packed arrays,
 *                 member_off[0] = 0 and member_off[m + 1] = member_off[m] + S_m rounded
 *                 up to a multiple of 16 rows, so that every member's slice of every
 *                 packed array (1-byte rows included) starts on a 16-byte boundary
 *   src           int32 [max_samples]: the cell env * Tcap + column of the sample in
 *                 row member_off[m] + ep_off[..] + j, and -1 in every other row below
 *                 max_samples (the padding behind a member's samples and whatever lies
 *                 behind member_off[n_members])
 * Nothing is written past max_eps episodes or max_samples rows; S_m <= g c_m, so
 * max_samples = sum over m of (g c_m rounded up to 16) always suffices.
 * Refused before any launch: NULL pointers; n_members outside 1..1024; n not a
 * multiple of n_members; n_cols outside 1..Tcap; n * Tcap >= 2^31; max_eps < 1;
 * max_samples outside 1..2^31 - 1. */
GA_API int ga_member_pack_index(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                                int64_t n_cols, int64_t n_members,
                                const int32_t* progress, const int32_t* col_base,
                                int64_t max_eps, int64_t max_samples, int32_t* ep_env,
                                int32_t* ep_end, int32_t* ep_len, int64_t* ep_off,
                                int64_t* member_samples, int64_t* member_off,
                                int32_t* src, ga_stream_t stream);
/* One plane of the packed batch: dst[r, 0:width] = src[cell(r), 0:width], rows of
 * `width` elements of elem_size bytes, ld_src / ld_dst elements apart.  per_episode 0:
 * one row per packed sample, cell(r) = src[r], and a row with src[r] < 0 (padding) is
 * written as zeros; per_episode 1: one row per episode, cell(e) = ep_env[e] * Tcap +
 * ep_end[e], the episode's last cell (lastobs, an env_info at the episode's end). */
typedef struct {
  const void* src; void* dst;
  int64_t ld_src, ld_dst;
  int32_t elem_size;    /* 1 or 4 */
  int32_t width;
  int32_t per_episode;
  int32_t pad_;
} ga_pack_plane;
#define GA_PACK_MAX_PLANES 16
/* ga_member_pack_gather: every plane of the batch in ONE launch.  n_rows: the rows of
 * `src` (every one of them is written in every per-sample plane: no byte of the packed
 * arrays stays uninitialised; padding is where src says so, member_off is not read);
 * n_eps: the episodes (0: no per-episode plane may be given).  4-byte planes of width
 * >= 4 are copied in 16-byte pieces.
 * Refused before the launch: NULL planes / src, a NULL pointer in a plane, NULL ep_env /
 * ep_end with a per-episode plane; n_planes outside 1..16; n_rows outside 1..2^31 - 1;
 * n_eps < 0, or 0 with a per-episode plane; Tcap outside 1..2^31 - 1; an elem_size other
 * than 1 or 4; width < 1 or a stride below it; a 4-byte plane of width >= 4 whose width
 * or strides are no multiple of 4 or whose pointers are not 16-byte aligned. */
GA_API int ga_member_pack_gather(const ga_pack_plane* planes, int64_t n_planes,
                                 const int32_t* src, int64_t n_rows,
                                 const int32_t* ep_env, const int32_t* ep_end,
                                 int64_t n_eps, int64_t Tcap, ga_stream_t stream);

/* ---- one optimisation pass, enqueued natively --------------------------------
 * All minibatches of one epoch of VPG._train (torch/algos/vpg.py:230-293) for
 * one network: forward, fused loss + gradient seed, backward, slab reduction,
 * optional RCCL all-reduce(mean) of the flat gradient, Adam.  Same kernels and
 * order as driving the entry points above one by one; exists because ~14
 * launches per minibatch through ctypes starve the GPU. */
typedef struct {
  const ga_mlp_desc* desc;
  float* params; float* grads; float* exp_avg; float* exp_avg_sq; int64_t n_flat;
  float* acts; float* dacts; float* out; float* dout; int64_t ldo;
  float* slabs; int64_t max_splits;
  int64_t step0;           /* Adam steps already taken */
  double lr, beta1, beta2, eps;
  int32_t learn_std;       /* 0: the log-std slot is not trained */
  const float* X; int64_t ldx; int64_t S;
  const int32_t* perm;     /* S minibatch ids of this pass, NULL = one full batch */
  int64_t mb;
  int32_t kind;            /* 0 Gaussian policy, 1 value (Gaussian NLL),
                              2 categorical policy */
  const float* actions; int64_t lda; const float* old_ll; const float* adv;
  const float* returns;
  int32_t has_min; float min_log_std; int32_t has_max; float max_log_std;
  int32_t algo; float clip; float ent_coeff; int32_t ent_flags;
  float* losses;           /* optional [n_minibatches] per-step losses */
  float* loss_scratch;     /* 1 float, used when losses == NULL */
  double* workspace;
  void* comm; int32_t world; /* RCCL communicator from ga_comm_init_rank, or NULL */
  int32_t double_softmax;    /* kind 2 */
  float grad_scale;          /* with comm: this rank's share S_local / S_global of the
                                minibatch, applied before the all-reduce(sum) */
  int64_t n_mb;              /* > 0 (with perm): the S ids of the pass are split into
                                exactly n_mb minibatches, minibatch k = ids
                                [k*S/n_mb, (k+1)*S/n_mb) -- data parallel ranks hold
                                different S but must issue the same number of
                                all-reduces; 0: ceil(S/mb) minibatches of mb ids,
                                the last one partial (BatchDataset) */
  const float* grad_scales_host; /* optional HOST array [n_mb]: per-minibatch
                                replacement of grad_scale (rows of this rank's
                                minibatch k / rows of the global minibatch k) */
  float* partials;           /* optional scratch for the fused step kernels: with at
                                least ga_update_partials_floats(desc, rows of the
                                largest minibatch) floats the step takes them (last
                                hidden layer + head + loss + gradient seed in one
                                launch, ...; see ga_set_fused_train) */
  int64_t partials_floats;
  int32_t phase;             /* 0: whole steps.  1: gradients only -- forward, loss,
                                backward, slab sum scaled by grad_scale into `grads`;
                                no all-reduce, no optimizer (the Python minibatch
                                loop exchanges and steps itself) */
} ga_update_args;
GA_API int ga_update_epoch(const ga_update_args* args, ga_stream_t stream);
/* Host-only (no GPU needed): the split of a pass into minibatches that
 * ga_update_epoch* walks -- ids [*start, *start + *M) of the permutation form
 * minibatch k; returns the number of minibatches of the pass (< 0: bad arguments).
 * S, mb, n_mb as in ga_update_args; has_perm = (perm != NULL).  The Python side's
 * OptimizerWrapper.minibatch_bounds must agree with it on every rank (the reference's
 * BatchDataset split, np/optimizers/minibatch_dataset.py:20-35, and the even split of
 * data-parallel runs); tests/test_host_logic_cpu.py compares the two. */
GA_API int64_t ga_minibatch_range(int64_t S, int64_t mb, int64_t n_mb, int has_perm,
                                  int64_t k, int64_t* start, int64_t* M);
/* Floats of `partials` scratch the fused step needs for minibatches of up to M rows
 * of this network; 0: the network's shapes take the per-layer kernels (last hidden
 * layer not 64 / 128 / 256 wide, or a head of more than 8 outputs). */
GA_API int64_t ga_update_partials_floats(const ga_mlp_desc* desc, int64_t M);
/* 1 (default): ga_update_epoch* steps take the fused kernels when `partials` is
 * given and the shapes allow: the last hidden layer, the head layer, the loss with
 * its gradient seed and the head's weight gradient in ONE launch (the hidden
 * activation never reaches HBM), the data gradient into the first hidden layer and
 * the first layer's weight gradient in one launch, one reduction + Adam launch
 * that also finishes the loss.  Same formulas, other summation orders than the
 * per-layer kernels (0 selects those): results agree to rounding. */
GA_API int ga_set_fused_train(int on);
/* 1 (default): networks of two equal tanh hidden layers of 32 or 64 units (<= 32
 * inputs, <= 8 outputs) take forward + loss + backward of a minibatch in ONE launch
 * (every weight in LDS, 64 rows per workgroup) followed by the same reduction +
 * Adam launch; 0: the kernels above.  Needs `partials` like them. */
GA_API int ga_set_narrow_step(int on);
/* 1 (default): with two hidden layers and <= 32 inputs (first-layer weights of at
 * most 5120 padded floats) the fused last-hidden-layer kernel computes the first
 * layer's outputs itself, k-chunk by k-chunk, instead of reading them back from a
 * separate launch (they are still written once for the backward pass); 0: the
 * first layer runs as its own launch. */
GA_API int ga_set_fused_first_layer(int on);
/* The software-pipelined k-loop of the fused forward kernels (first-layer producer,
 * H1 spill and weight prefetch issued in the shadow of the step's MFMAs; compiled for
 * first layers of 17 .. 20 inputs at 256 units): 1 default, 0 the plain loop (also
 * GARAGE_AMD_PIPELINED_KLOOP=0).  Bit-identical results either way. */
GA_API int ga_set_pipelined_kloop(int on);
/* The weight-gradient GEMM of layers whose two sides are multiples of 128 (row-major
 * operands, no gather, slabs with an even leading dimension) runs in an instantiation
 * whose waves own 32 x 64 outputs with lane pairs of columns: one 8-B LDS read per pair
 * of B values, 8-B stores straight from the accumulators, buffer addressing.  1 default,
 * 0 the one kernel for every shape (also GARAGE_AMD_WGRAD_PAIRED=0).  Same tiles, slabs
 * and summation order: bit-identical results either way. */
GA_API int ga_set_wgrad_paired_columns(int on);
/* Launches of that instantiation since the library was loaded (ga_launch_count(2) counts
 * the weight-gradient GEMM whichever kernel takes it). */
GA_API int64_t ga_wgrad_paired_launches(void);
/* The split-K weight-gradient slabs of the middle layer (two hidden layers, more than
 * one split) are summed inside the data-gradient launch that follows the
 * weight-gradient GEMM, in the optimizer launch's own order, and the optimizer launch
 * reads one partial of them instead of all: 1 default, 0 the optimizer launch sums
 * them (also GARAGE_AMD_SLAB_SUM_IN_DGRAD=0).  Bit-identical results either way. */
GA_API int ga_set_slab_sum_in_dgrad(int on);
/* Fused optimizer steps of ONE network with two hidden layers of the same width (64, 128
 * or 256 units, <= 32 inputs), exact fp32: the forward + loss launch and the
 * data-gradient launch go out as one launch whose workgroups keep the last hidden
 * layer's data gradient in LDS between the two; the middle layer's weight-gradient GEMM
 * follows it and the optimizer launch sums that layer's slabs itself
 * (ga_set_slab_sum_in_dgrad has nothing to act on in such a step).  0: two launches
 * (also GARAGE_AMD_FUSED_FWD_DGRAD=0).  Bit-identical results either way. */
GA_API int ga_set_fused_fwd_dgrad(int on);
/* EXPERIMENT, off by default (also GARAGE_AMD_SPLIT_BF16=1): the k-loops of the fused
 * update kernels that have such an instantiation (256-unit networks, first layer in
 * the kernel) run on v_mfma_f32_32x32x16_bf16 with every fp32 operand split exactly
 * into three bf16 terms and the six products i + j <= 2 accumulated in fp32
 * (about 2^-22 relative error per product against 2^-24 of the exact fp32 MFMA).
 * Results differ from the default in the last bits; the default stays exact fp32. */
GA_API int ga_set_split_bf16(int on);
/* The policy pass and the value-function pass of one epoch, minibatch by
 * minibatch alternately on two streams.  The reference runs them back to back
 * (vpg.py:244-248); they share no written state, so the results are identical
 * and the two launch chains overlap on the device.  The two argument sets must
 * not share parameter, slab, activation or reduction buffers. */
GA_API int ga_update_epoch_pair(const ga_update_args* a, ga_stream_t stream_a,
                                const ga_update_args* b, ga_stream_t stream_b);

/* ---- one optimisation pass of a POPULATION of networks, in shared launches -------
 * ga_update_epoch for n_members networks of one shape at once (new: the reference
 * trains one learner per process).  Step k of every member's pass goes out as two
 * launches -- forward + loss + backward of every member's minibatch k, then every
 * member's reduction + Adam -- instead of two per member.  Each member gets, bit for
 * bit, what ga_update_epoch (with ga_set_small_step(0), the narrow step on) gives a
 * lone network on the member's data: the same kernel body, summation trees and Adam.
 * Members may hold different sample counts; a member whose pass has fewer steps than
 * another's is left alone in the remaining ones (nothing of it is written, its step
 * count does not advance).
 *
 * One member: rows of (n_members, stride) tensors with stride % 4 == 0 -- the layout
 * ga_policy_env_step_members_f32 rolls out from, so the tensor that trains is the
 * tensor that rolls out -- and the member's own batch and hyperparameters. */
typedef struct ga_member_update {
  float* params; float* grads; float* exp_avg; float* exp_avg_sq;
  const float* X; int64_t ldx; int64_t S;
  const int32_t* perm;     /* S minibatch ids of this pass; NULL only with mb == 0 */
  const float* actions; int64_t lda; const float* old_ll; const float* adv;
  const float* returns;
  int64_t step0;           /* Adam steps this member has already taken */
  double lr;
  float clip; float ent_coeff;
  float* losses;           /* optional [steps of this member's pass] per-step losses */
} ga_member_update;
/* What the members share.  Minibatch k of member m = ids [k * mb, min(S_m, (k + 1) *
 * mb)) of its permutation (ga_minibatch_range with n_mb = 0); mb == 0: rows [0, S_m)
 * in one step.  kind / algo / ent_flags / has_min .. max_log_std / double_softmax /
 * learn_std / beta1 .. eps as in ga_update_args.  partials: at least
 * ga_update_members_partials_floats(desc, n_members, rows of the largest minibatch of
 * any member) floats, 16-byte aligned.  workspace: reserved, may be NULL. */
typedef struct ga_update_members_args {
  const ga_mlp_desc* desc;
  int32_t kind; int32_t algo; int32_t ent_flags;
  int32_t has_min; float min_log_std; int32_t has_max; float max_log_std;
  int32_t double_softmax; int32_t learn_std;
  double beta1, beta2, eps;
  int64_t mb;
  int64_t n_members;
  const ga_member_update* members_host; /* HOST array [n_members] */
  float* partials; int64_t partials_floats;
  double* workspace;
} ga_update_members_args;
/* 1: networks ga_update_epoch_members takes -- two equal tanh hidden layers of 32 or 64
 * units, <= 32 inputs, <= 8 linear outputs, no layer normalisation (the narrow step's
 * shapes); 0 otherwise, NULL included. */
GA_API int ga_update_members_supported(const ga_mlp_desc* desc);
/* Floats of `partials` for n_members members with minibatches of up to max_rows rows;
 * 0: unsupported network or sizes out of range. */
GA_API int64_t ga_update_members_partials_floats(const ga_mlp_desc* desc, int64_t n_members,
                                                 int64_t max_rows);
/* One pass: max over the members of ceil(S_m / mb) pairs of launches on `stream`, after
 * one asynchronous copy of the member and Adam tables (built in pinned host memory
 * the library keeps, eight passes' worth, grown on demand and kept).  The call MAY
 * BLOCK its caller: from the ninth call on it first waits on the host for the pass that
 * used its tables eight calls earlier; it never waits inside the pass.  The one entry
 * point that is therefore not graph-capture safe.  Refused before any launch (negative
 * return, ga_last_error): null pointers (args, desc, members_host, partials, a
 * member's params / grads / moments / X, the arrays its kind reads, perm with mb > 0),
 * n_members outside 1 .. 1024, a network ga_update_members_supported refuses, a member
 * pointer, ldx or lda that is not a 16-byte aligned quad (actions of kinds 0; params,
 * grads, moments, X, partials always), parameter offsets that are not quads from 4 up,
 * S_m < 1 or >= 2^31, mb < 0 or >= 2^31, step0 < 0, partials_floats smaller than
 * ga_update_members_partials_floats returns, a kind outside 0 .. 2, an algo outside
 * 0 .. 1. */
GA_API int ga_update_epoch_members(const ga_update_members_args* args, ga_stream_t stream);

/* ---- the diagnostics of a POPULATION in joint launches -----------------------------
 * What VPG._after_train runs per member after the update (vpg.py:178-184 and
 * log_performance, _functions.py:233-275) -- ga_mlp_forward_f32, ga_ppo_*_loss_f32,
 * ga_*_kl_f32, ga_gaussian_nll_loss_f32, ga_episode_sums_f32 -- for every member of a
 * population in a FIXED number of launches per entry point, whatever the member count
 * (new: the reference trains one learner per process).  Member m gets, bit for bit, what
 * the lone entry point gives on its arguments alone: each launch runs the lone kernel's
 * body for the member a workgroup belongs to (its parameter struct comes from a device
 * table, its block index and block count are those of the lone launch), every member has
 * its own stretch of the partials, and sums finish in a second fixed-order launch.  The
 * members arrays are HOST arrays; the tables are built in pinned memory the library keeps
 * and uploaded by one asynchronous copy per call, as ga_update_epoch_members' tables are
 * (eight calls' worth: a call MAY BLOCK its caller on the call that used its slot eight
 * calls earlier, and is not graph-capture safe).  Every entry refuses before any copy or
 * launch (negative return, ga_last_error): null pointers, a member count outside 1 .. 1024
 * (1 .. 2048 where it says so: a member's batch and its one padded cell are two entries),
 * a member with rows < 1 or >= 2^31, strides narrower than the width they hold, partials
 * smaller than ga_members_diag_partials_doubles of the members' rows. */
/* ga_mlp_forward_f32(desc, params, X, ldx, NULL, rows, acts, out, ldo) of every entry.
 * acts: rows * (round4(dims[1]) + round4(dims[2])) floats, layer l's block at (the widths
 * below it) * rows -- the layout of ga_mlp_forward_f32's workspace at a capacity of
 * exactly `rows`; desc->act_off is not read.  At most three launches per kernel kind a
 * layer takes (the plans are those of ga_mlp_forward_f32 under the same switches; entries
 * whose row counts take different kernels go to different launches).  Refuses networks
 * ga_update_members_supported refuses and pointers / strides that are not 16-byte aligned
 * quads.  1 .. 2048 entries. */
typedef struct ga_member_forward {
  const float* params; const float* X; int64_t ldx; int64_t rows;
  float* acts; float* out; int64_t ldo;
} ga_member_forward;
GA_API int ga_mlp_forward_members_f32(const ga_mlp_desc* desc, const ga_member_forward* members,
                                      int64_t n_members, ga_stream_t stream);
/* 1: ga_mlp_forward_members_f32 takes this network under the developer switches as they
 * stand NOW (ga_update_members_supported's shapes, and every layer on a kernel that has a
 * members instantiation: not with ga_set_fused_forward(1), which takes the network in one
 * launch of another kernel); 0 otherwise, with the reason in ga_last_error.  Callers ask
 * before they begin work that the refusal would interrupt. */
GA_API int ga_mlp_forward_members_supported(const ga_mlp_desc* desc);
/* doubles of `partials` for members of these row counts (2 per block of a member's own
 * grid; the KL entry needs half); 0: a bad count or row count */
GA_API int64_t ga_members_diag_partials_doubles(const int64_t* rows, int64_t n_members);
/* ga_ppo_gaussian_loss_f32 (kind 0) / ga_ppo_categorical_loss_f32 (kind 2) of every entry,
 * forward only: no gradient seed, no log-likelihoods, rows in order.  One launch, and one
 * more where an entry has more than 256 rows.  ent_sum_out (categorical, optional): the
 * sum of the rows' entropies.  1 .. 2048 entries. */
typedef struct ga_members_loss_args {
  int32_t kind; int32_t A; int32_t algo; int32_t ent_flags;
  int32_t has_min; float min_log_std; int32_t has_max; float max_log_std;
  int32_t double_softmax;
} ga_members_loss_args;
typedef struct ga_member_loss {
  const float* head; int64_t ld;          /* [rows, ld] means / class scores */
  const float* actions; int64_t lda;
  const float* old_ll; const float* adv;  /* old_ll: NULL with algo 1 */
  const float* log_std;                   /* kind 0: the device scalar parameter */
  int64_t rows;
  float clip; float ent_coeff;
  float* loss_out; double* ent_sum_out;
} ga_member_loss;
GA_API int ga_ppo_loss_members_f32(const ga_members_loss_args* args,
                                   const ga_member_loss* members, int64_t n_members,
                                   double* partials, int64_t partials_doubles,
                                   ga_stream_t stream);
/* ga_gaussian_nll_loss_f32 of every member, forward only.  1 .. 1024 members. */
typedef struct ga_member_nll {
  const float* v; int64_t ldv; const float* returns; const float* log_std;
  int64_t rows; float* loss_out;
} ga_member_nll;
GA_API int ga_gaussian_nll_members_f32(const ga_member_nll* members, int64_t n_members,
                                       double* partials, int64_t partials_doubles,
                                       ga_stream_t stream);
/* ga_gaussian_kl_f32 (categorical 0) / ga_categorical_kl_f32 (1) of every entry: two
 * launches.  1 .. 2048 entries. */
typedef struct ga_member_kl {
  const float* head_old; const float* head_new; int64_t ld; int64_t rows;
  float log_std_old; float log_std_new;   /* Gaussian heads */
  double* kl_sum_out;
} ga_member_kl;
GA_API int ga_kl_members_f32(int categorical, int A, int double_softmax,
                             const ga_member_kl* members, int64_t n_members, double* partials,
                             int64_t partials_doubles, ga_stream_t stream);
/* log_performance's device part of every member in one launch: out[0 .. n_eps) =
 * ga_episode_sums_f32(rewards, ep_off), out[n_eps .. 2 n_eps) = returns[ep_off[e]],
 * out[2 n_eps .. 3 n_eps) = 1.0 where step_types[ep_off[e + 1] - 1] == terminal, else 0.0.
 * 1 .. 1024 members. */
typedef struct ga_member_episodes {
  const float* rewards; const int64_t* ep_off; int64_t n_eps;
  const float* returns; const uint8_t* step_types; double* out;
} ga_member_episodes;
GA_API int ga_episode_stats_members_f32(const ga_member_episodes* members, int64_t n_members,
                                        int terminal, ga_stream_t stream);
/* frees the pinned / device table slots of the entries above (tests) */
GA_API void ga_members_diag_release(void);

/* RCCL communicator for the data-parallel gradient all-reduce (new: the
 * reference has no collective on this path).
 * ga_comm_unique_id fills 128 bytes on rank 0 (HOST pointer) to be broadcast by
 * the caller; ga_comm_init_rank returns an opaque handle. */
/* The all-reduce ga_update_epoch* calls on args->comm between the slab reduction
 * and Adam: fn(comm, buf, n, stream) sums buf over the ranks in place, returns 0.
 * ga_comm_init_rank installs RCCL's; a caller with another transport (or a test
 * standing in for the second rank) installs its own. */
typedef int (*ga_allreduce_fn)(void* comm, float* buf, int64_t n, void* stream);
GA_API void ga_set_allreduce_hook(ga_allreduce_fn fn);
GA_API int ga_comm_available(void); /* 1 if librccl could be loaded in this process */
GA_API int ga_comm_unique_id(void* id128_host);
GA_API void* ga_comm_init_rank(const void* id128_host, int rank, int world);
GA_API int ga_comm_allreduce_sum_f32(void* comm, float* buf, int64_t n, ga_stream_t stream);
/* ranks of the communicator as RCCL reports them (ncclCommCount); < 0 on error */
GA_API int ga_comm_count(void* comm);
GA_API int ga_comm_destroy(void* comm);
/* ga_update_epoch_pair with communicators: the two networks' all-reduces sit on two
 * streams and two communicators.  1 (default): every all-reduce waits (HIP event)
 * for the previously enqueued one of the OTHER network, so each GPU executes them
 * in the host's issue order, identical on every rank -- no rank can sit in network
 * A's collective while its peer sits in network B's.  0: no such edges (the two
 * collectives may run concurrently; they are small enough to co-reside). */
GA_API int ga_set_ordered_allreduce(int on);
/* ga_update_epoch_pair, one process: 1 (opt-in, also GARAGE_AMD_MERGED_PAIR=1) step k of
 * BOTH passes as four launches on stream_a, each a grid over the tiles of both networks
 * (when both take the fused 256-wide kernels with the same shapes; stream_b is ordered
 * around the epoch); 0 (default) two four-launch chains on the two streams.
 * Bit-identical results; the merged schedule is the same every time but measured
 * slower. */
GA_API int ga_set_merged_pair(int on);

/* ---- linear feature baseline ---------------------------------------------------
 * garage.np.baselines.LinearFeatureBaseline (np/baselines/linear_feature_baseline.py):
 * a ridge regression of the returns on the F = 2 * obs_dim + 4 features
 *   [clip(obs, -10, 10), clip(obs)^2, al, al^2, al^3, 1],  al = t / 100.0,
 * t the sample's index inside its episode (_features, lines 43-58).  Both passes form
 * the feature rows on the fly, in fp64 from the clip on, and never write them to HBM.
 *   obs     [S, ldo] fp32 (a DeviceEpisodeBatch's obs_dev); columns obs_dim .. ldo are
 *           never read
 *   ep_off  [n_eps + 1] int64, strictly increasing from 0 to S (episodes of length >= 1);
 *           its CONTENT is the caller's contract: whatever it holds, no pass reads or
 *           writes outside the arrays' stated sizes
 * 1 <= obs_dim <= 128, 1 <= S < 2^31, 1 <= n_eps <= S; refused otherwise, and on a null
 * pointer, ldo < obs_dim, ldv < 1 or an fp64 array that is not 8-byte aligned. */
GA_API int ga_linear_features_supported(int obs_dim); /* 1 <= obs_dim <= 128 */
/* doubles of `workspace` the Gram pass writes for (obs_dim, S) -- all of them, and
 * nothing beyond; -1 for an obs_dim or S the passes refuse */
GA_API int64_t ga_linear_gram_workspace_doubles(int obs_dim, int64_t S);
/* gram [F, F] = featmat.T.dot(featmat) (full, exactly symmetric), rhs [F] =
 * featmat.T.dot(returns) of LinearFeatureBaseline.fit (lines 68-75), fp64, returns [S]
 * fp32.  The 16x16 tiles of the upper triangle run on the fp64 matrix instruction, one
 * workgroup per slab of 2048 rows (every 1024th slab beyond 1024 of them); the
 * workgroups' partials are added in a fixed order by a second launch: no atomics, the
 * same inputs give the same bits.  The F x F solve is the caller's (numpy's lstsq, as the
 * reference).  Algorithmic flops S * F * (F + 1) in fp64, HBM bytes 4 * S * (obs_dim + 1). */
GA_API int ga_linear_features_gram_f64(const float* obs, int64_t ldo, int obs_dim,
                                       const int64_t* ep_off, int64_t n_eps, int64_t S,
                                       const float* returns, double* gram, double* rhs,
                                       double* workspace, ga_stream_t stream);
/* values[i * ldv] = (float)(features(i) . coeffs), coeffs [F] fp64 on the device: predict
 * (lines 91-93) for every sample of the batch; one fp64 sum per row, in feature order. */
GA_API int ga_linear_features_predict_f32(const float* obs, int64_t ldo, int obs_dim,
                                          const int64_t* ep_off, int64_t n_eps, int64_t S,
                                          const double* coeffs, float* values, int64_t ldv,
                                          ga_stream_t stream);

/* The same two passes for a POPULATION of baselines of one obs_dim, every member's batch in
 * ONE launch of each kernel (new: the reference fits one baseline per process).  Member m
 * gets, bit for bit, what the lone entry point gives on its batch alone: the kernels share
 * the lone kernels' bodies, a member owns the workgroups its lone grid would have (a flat
 * grid, found through a prefix table), and its partials are added in its own workgroups'
 * order.  members_host is a HOST array; the table the kernels read is built in pinned
 * memory the library keeps and uploaded by one asynchronous copy, as
 * ga_update_epoch_members' tables are (eight calls' worth: a call MAY BLOCK its caller on
 * the call that used its slot eight calls earlier, and is not graph-capture safe). */
typedef struct ga_linear_gram_member {
  const float* obs; int64_t ldo;             /* [S, ldo] */
  const int64_t* ep_off; int64_t n_eps;      /* [n_eps + 1] */
  int64_t S;
  const float* returns;                      /* [S] */
  double* gram;                              /* [F, F] */
  double* rhs;                               /* [F] */
} ga_linear_gram_member;
typedef struct ga_linear_predict_member {
  const float* obs; int64_t ldo;
  const int64_t* ep_off; int64_t n_eps;
  int64_t S;
  const double* coeffs;                      /* [F] fp64, or NULL: this member's values
                                                are zeros (predict before the first fit,
                                                linear_feature_baseline.py:91-92) */
  float* values; int64_t ldv;                /* values[i * ldv] */
} ga_linear_predict_member;
/* doubles of `workspace` for members of S[0 .. n_members) samples (a HOST array): the sum of
 * ga_linear_gram_workspace_doubles over them; -1 for anything the pass refuses */
GA_API int64_t ga_linear_gram_members_workspace_doubles(int obs_dim, int64_t n_members,
                                                        const int64_t* S);
/* featmat.T.dot(featmat) and featmat.T.dot(returns) of LinearFeatureBaseline.fit
 * (linear_feature_baseline.py:68-75, with _features' rows, lines 43-58) for every member:
 * one Gram launch of sum_m blocks(S_m) workgroups and one reduce launch.  Refused before
 * any launch or copy: null pointers, n_members outside 1 .. 1024, for any member what
 * ga_linear_features_gram_f64 refuses, gram / rhs / workspace not 8-byte aligned,
 * workspace_doubles below ga_linear_gram_members_workspace_doubles. */
GA_API int ga_linear_features_gram_members_f64(const ga_linear_gram_member* members_host,
                                               int64_t n_members, int obs_dim,
                                               double* workspace, int64_t workspace_doubles,
                                               ga_stream_t stream);
/* _features(path).dot(self._coeffs) of predict (linear_feature_baseline.py:91-93) for every
 * sample of every member, one launch.  Refused before any launch or copy: null pointers
 * (coeffs excepted), n_members outside 1 .. 1024, for any member what
 * ga_linear_features_predict_f32 refuses, more than 2^31 - 1 workgroups of 256 rows. */
GA_API int ga_linear_features_predict_members_f32(const ga_linear_predict_member* members_host,
                                                  int64_t n_members, int obs_dim,
                                                  ga_stream_t stream);
/* frees the member tables' slots (tests; the library otherwise keeps them) */
GA_API void ga_linear_members_release(void);

/* ---- measurement ----------------------------------------------------------
 * Optional HIP-event timing of every GEMM / scan launch on its own stream
 * (bench.py's roofline leg; no reference counterpart).  kinds: 0..2 =
 * gemm_f32_kernel<128,128,..> forward / data-grad / weight-grad, 3..5 = the
 * <256,32,..> variants, 6 = gae_scan_kernel.  ga_prof_collect synchronises and
 * fills out_host[kind*3 + {0,1,2}] = {total ms, total flops or bytes, launches}
 * (a HOST pointer). */
GA_API int ga_prof_enable(int on);
GA_API int ga_prof_collect(double* out_host, int n_kinds);
/* Launches of kernel kind `kind` (csrc/prof.h: 9 = fwd_head_loss_kernel, 10 =
 * dgrad_wgrad0_kernel, 11 = narrow_train_kernel, 12 = mlp_eval_forward_kernel, 13 =
 * a whole rollout in one policy_step_fused_kernel launch, 15 = a step of a whole
 * population in one narrow_train_members_kernel launch, ...)
 * since the library was loaded, counted whether timing is on or not; -1 for an
 * unknown kind.  Tests use it to assert WHICH kernels an update dispatched to. */
GA_API int64_t ga_launch_count(int kind);

#ifdef __cplusplus
}
#endif
#endif /* GARAGE_AMD_H_ */
