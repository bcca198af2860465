// Entry points that one source file of the library defines and another calls, and
// the public header every source file compiles against.  Not part of the C ABI:
// the library is built with -fvisibility=hidden and exports include/garage_amd.h
// only.  Host C++ (no device code), so that the CPU harnesses under tests/host can
// build the library's host sources (update.cpp, rollout_loop.cpp, mlp_layers.cpp, the
// *_host.cpp files) against it too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/garage_amd.h"

// errors.cpp: sets the thread-local message ga_last_error() returns
void ga_set_error(const char* fmt, ...);

// lnorm.hip: LayerNorm of the hidden-layer inputs (forward, backward, tangent)
int ga_ln_forward(const float* X, int64_t ldx, const int32_t* idx, int64_t M, int D,
                  const float* gamma, const float* beta, float* Y, int64_t ldy,
                  float* stats, hipStream_t stream);
int ga_ln_backward(float* dY, int64_t ldd, const float* X, int64_t ldx, const int32_t* idx,
                   const float* stats, int64_t M, int D, const float* gamma, int want_dx,
                   int hact, int rows_per_split, int n_splits, float* dgamma, float* dbeta,
                   int64_t split_stride, hipStream_t stream);
int ga_ln_jvp(const float* tX, int64_t ldt, const float* X, int64_t ldx, const int32_t* idx,
              const float* stats, int64_t M, int D, const float* gamma,
              const float* tgamma, const float* tbeta, float* tY, int64_t ldy,
              hipStream_t stream);

// ---- device envs: what every kind states about itself, and the ONE dispatch from a
// ga_env_ref to its typed struct (rollout_host.cpp, rollout_loop.cpp).
// Every struct has `n`; the observation width, the columns of an action row and
// whether the action is a class index are the overloads below.
//
// The seeded state-vector kinds (rollout_dev.h: StateEnv<K>) state their facts in ONE
// row each: X(C-ABI struct, kind code, device kind description, observation width,
// whether the action -- always one column -- is a class index, as an expression in
// the struct `e`).  MountainCar is the one kind whose answer is the struct's:
// MountainCar-v0 takes a class index, MountainCarContinuous-v0 a force.
#define GA_STATE_ENV_KINDS(X)                                                      \
  X(ga_cartpole_env, GA_ENV_CARTPOLE, CartPoleKind, 4, 1)                          \
  X(ga_pendulum_env, GA_ENV_PENDULUM, PendulumKind, 3, 0)                          \
  X(ga_double_pendulum_env, GA_ENV_DOUBLE_PENDULUM, DoublePendulumKind, 11, 0)     \
  X(ga_acrobot_env, GA_ENV_ACROBOT, AcrobotKind, 6, 1)                             \
  X(ga_mountain_car_env, GA_ENV_MOUNTAIN_CAR, MountainCarKind, 2, e->continuous == 0)

inline int ga_env_obs_dim(const ga_synth_env* e) { return e->obs_dim; }
inline int ga_env_obs_dim(const ga_point_env*) { return 3; }
inline int ga_env_obs_dim(const ga_grid_env* e) { return e->rows * e->cols; }
inline int ga_env_obs_dim(const ga_multi_point_env* e) {
  return 3 + (e->mode == GA_TASK_ADD_ONEHOT ? e->num_tasks : 0);
}
inline int ga_env_discrete(const ga_synth_env* e) { return e->discrete != 0; }
inline int ga_env_discrete(const ga_point_env*) { return 0; }
inline int ga_env_discrete(const ga_grid_env*) { return 1; }
inline int ga_env_discrete(const ga_multi_point_env*) { return 0; }
inline int ga_env_act_width(const ga_synth_env* e) { return e->discrete ? 1 : e->act_dim; }
inline int ga_env_act_width(const ga_point_env*) { return 2; }
inline int ga_env_act_width(const ga_grid_env*) { return 1; }
inline int ga_env_act_width(const ga_multi_point_env*) { return 2; }
#define GA_STATE_ENV_FACTS(GaEnv, KIND, DEV, OBS, DISCRETE)             \
  inline int ga_env_obs_dim(const GaEnv*) { return OBS; }               \
  inline int ga_env_discrete(const GaEnv* e) { return (void)e, (DISCRETE); } \
  inline int ga_env_act_width(const GaEnv*) { return 1; }
GA_STATE_ENV_KINDS(GA_STATE_ENV_FACTS)
#undef GA_STATE_ENV_FACTS

// EVERY device env kind, once: X(C-ABI struct, kind code, ...) -- the four kinds written by
// hand and the rows of GA_STATE_ENV_KINDS with their further columns.  ga_visit_env's
// switch and the per-kind instantiations of the launch seam (rollout_params.h) are
// generated from it.
#define GA_ENV_KINDS(X)                       \
  X(ga_synth_env, GA_ENV_SYNTH)               \
  X(ga_point_env, GA_ENV_POINT)               \
  X(ga_grid_env, GA_ENV_GRID)                 \
  X(ga_multi_point_env, GA_ENV_MULTI_POINT)   \
  GA_STATE_ENV_KINDS(X)

// f(const ga_<kind>_env*) of the env `ref` points to; `who` names the entry point in
// the two errors this owns
template <class F>
int ga_visit_env(const ga_env_ref* ref, const char* who, F&& f) {
  if (!ref || !ref->env) {
    ga_set_error("%s: null env", who);
    return -1;
  }
  switch (ref->kind) {
#define GA_ENV_CASE(GaEnv, KIND, ...) \
  case KIND: return f((const GaEnv*)ref->env);
    GA_ENV_KINDS(GA_ENV_CASE)
#undef GA_ENV_CASE
  }
  ga_set_error("%s: unknown env kind %d", who, ref->kind);
  return -1;
}

// What NormalizedEnv's action rescale (norm->act_low set) needs, stated once:
// ga_rollout_env_steps and ga_build_env_step (rollout_host.cpp) both refuse through here.
inline int ga_rescale_refused(const ga_norm_args* norm, int discrete, const char* who) {
  if (norm->act_high && norm->scaled_action && !discrete) return 0;
  ga_set_error("%s: action rescale needs bounds, scratch and a continuous action space", who);
  return -1;
}

extern "C" {
// mlp_layers.cpp: the backward pass of layers l_start .. 0 given d(loss)/d(pre-activation)
// of layer l_start in dacts (l_start = n_layers - 1 with `dout`: the whole pass, what
// ga_mlp_backward_f32 does); fused_first: the data gradient into layer 0's output and
// layer 0's weight gradient are computed elsewhere (ga_fused_dgrad_wgrad0)
int ga_mlp_backward_range_f32(const ga_mlp_desc* d, const float* params, const float* X,
                              int64_t ldx, const int32_t* row_idx, int64_t M,
                              const float* acts, const float* dout, int64_t ldo,
                              float* dacts, float* grad_slabs, int64_t slab_stride,
                              int64_t n_splits, int l_start, int fused_first,
                              hipStream_t stream);
// policy_fused.hip: 1 when ga_policy_env_step_fused_f32 rescales the action inside its
// launch under norm->act_low.  ga_rollout_env_steps asks before it hands such a rollout
// to the one launch; a kernel side that answers 0 (tests/host/rollout_loop_harness.cpp)
// keeps the three launches per step.
int ga_policy_env_step_rescales(void);
// losses_host.cpp: doubles of per-block partial sums at the front of the reduction
// workspace (ga_reduction_workspace_doubles)
int64_t ga_reduction_partials_doubles(void);
}
