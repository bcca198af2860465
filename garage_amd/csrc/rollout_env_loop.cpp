// ga_rollout_synth_steps (rollout_loop.cpp) for any device env: `n_steps`
// vectorised rollout steps enqueued from C++ -- the fused policy step, then env step
// -> bookkeeping -> reset of finished envs, ping-ponging the two observation
// buffers, or the whole rollout in one fused launch where it applies.  The env is
// a tagged pointer (ga_env_ref); the kernels are instantiated per env kind.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace {
// what the loop needs to know of the env: its size and action columns
struct EnvShape {
  int64_t n;
  int act_dim, discrete;
};

int env_shape(const ga_env_ref* env, EnvShape* out) {
  if (!env || !env->env) {
    ga_set_error("ga_rollout_env_steps: null env");
    return -1;
  }
  switch (env->kind) {
    case GA_ENV_SYNTH: {
      const ga_synth_env* e = (const ga_synth_env*)env->env;
      *out = EnvShape{e->n, e->act_dim, e->discrete};
      return 0;
    }
    case GA_ENV_POINT:
      *out = EnvShape{((const ga_point_env*)env->env)->n, 2, 0};
      return 0;
    case GA_ENV_GRID:
      *out = EnvShape{((const ga_grid_env*)env->env)->n, 1, 1};
      return 0;
    case GA_ENV_MULTI_POINT:
      *out = EnvShape{((const ga_multi_point_env*)env->env)->n, 2, 0};
      return 0;
  }
  ga_set_error("ga_rollout_env_steps: unknown env kind %d", env->kind);
  return -1;
}
}  // namespace

extern "C" int ga_rollout_env_steps(const ga_mlp_desc* desc, const float* params,
                                    const ga_head_args* head, const ga_env_ref* env,
                                    const ga_record_args* rec, float* obs_a, float* obs_b,
                                    const ga_norm_args* norm, float* raw_a, float* raw_b,
                                    int64_t n_steps, ga_stream_t stream) {
  if (!desc || !params || !head || !env || !rec || !obs_a || !obs_b) {
    ga_set_error("ga_rollout_env_steps: null pointer");
    return -1;
  }
  EnvShape shape;
  if (env_shape(env, &shape)) return -1;
  if (norm && norm->act_low && (!norm->act_high || !norm->scaled_action || shape.discrete)) {
    ga_set_error("ga_rollout_env_steps: action rescale needs bounds, scratch and a "
                 "continuous action space");
    return -1;
  }
  if (norm && norm->normalize_obs && (!raw_a || !raw_b)) {
    ga_set_error("ga_rollout_env_steps: observation normalisation needs the raw "
                 "observation buffers");
    return -1;
  }
  if (n_steps < 0 || head->col + n_steps > head->Tcap) {
    ga_set_error("ga_rollout_env_steps: steps exceed the rollout buffer");
    return -1;
  }
  if (!ga_policy_step_fused_supported(desc)) {
    ga_set_error("ga_rollout_env_steps: network not supported by the fused step");
    return -1;
  }
  float* cur = obs_a;
  float* nxt = obs_b;
  float* raw_cur = raw_a;
  float* raw_nxt = raw_b;
  ga_head_args h = *head;
  ga_record_args r = *rec;
  ga_norm_args nm;
  if (norm) nm = *norm;
  if (ga_fused_env_step_enabled() && !(norm && nm.act_low) && !head->noise && n_steps >= 1) {
    // the whole rollout in ONE launch (ga_policy_env_step_fused_f32)
    r.col = h.col;
    r.next_obs = nxt;
    h.obs = cur;
    if (norm) {
      nm.raw_obs = raw_cur;
      nm.raw_next_obs = raw_nxt;
    }
    return ga_policy_env_step_fused_ref(desc, params, &h, env, &r, norm ? &nm : nullptr,
                                        n_steps, stream);
  }
  for (int64_t s = 0; s < n_steps; ++s) {
    h.col = head->col + s;
    h.step = head->step + (uint32_t)s;
    h.obs = cur;
    r.col = h.col;
    r.next_obs = nxt;
    if (norm) {
      nm.raw_obs = raw_cur;
      nm.raw_next_obs = raw_nxt;
    }
    int rc = ga_policy_step_fused_f32(desc, params, &h, stream);
    if (rc) return rc;
    const float* env_action = h.action;
    if (norm && nm.act_low) {
      // NormalizedEnv.step: the wrapped env sees the rescaled, clipped action; the
      // batch keeps the policy's own (normalized_env.py:90-114)
      rc = ga_action_rescale_f32(shape.n, shape.act_dim, h.action, h.lda, nm.act_low,
                                 nm.act_high, nm.expected_action_scale,
                                 nm.scaled_action, h.lda, stream);
      if (rc) return rc;
      env_action = nm.scaled_action;
    }
    rc = ga_env_step_record_ref(env, &r, norm ? &nm : nullptr, env_action, h.lda, cur,
                                stream);
    if (rc) return rc;
    float* t = cur;
    cur = nxt;
    nxt = t;
    t = raw_cur;
    raw_cur = raw_nxt;
    raw_nxt = t;
  }
  return 0;
}
