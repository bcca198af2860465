// `n_steps` vectorised rollout steps of any device env enqueued from C++: fused
// policy step, then env step -> bookkeeping -> reset of finished envs in one launch,
// ping-ponging the two observation buffers -- or the whole rollout in one fused
// launch where it applies.  Same per-env operations and order as GpuVecWorker._step
// drives from Python (VecWorker.step_episode, sampler/vec_worker.py:176-204); it
// exists because the Python/ctypes overhead per launch (~12 us) exceeds the device
// time of a step.  The env is a tagged pointer (ga_env_ref); the kernels are
// instantiated per env kind.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "internal.h"
#include "shape_rules.h"

// 1 (default): policy step and env step of a rollout step in ONE launch
// (ga_policy_env_step_fused_f32), NormalizedEnv's action rescale included;
// 0, or GARAGE_AMD_FUSED_ENV_STEP=0 in the environment: two launches, three with the
// rescale
static int g_fused_env_step = -1;
extern "C" int ga_set_fused_env_step(int on) {
  g_fused_env_step = on != 0;
  return 0;
}
static int fused_env_step_on() {
  if (g_fused_env_step < 0) {
    const char* e = getenv("GARAGE_AMD_FUSED_ENV_STEP");
    g_fused_env_step = (e && e[0] == '0') ? 0 : 1;
  }
  return g_fused_env_step;
}

extern "C" int ga_rollout_env_steps(const ga_mlp_desc* desc, const float* params,
                                    const ga_head_args* head, const ga_env_ref* env,
                                    const ga_record_args* rec, float* obs_a, float* obs_b,
                                    const ga_norm_args* norm, float* raw_a, float* raw_b,
                                    int64_t n_steps, ga_stream_t stream) {
  if (!desc || !params || !head || !env || !rec || !obs_a || !obs_b) {
    ga_set_error("ga_rollout_env_steps: null pointer");
    return -1;
  }
  // what the loop needs to know of the env: its size and action columns
  int64_t n = 0;
  int act_width = 0, discrete = 0;
  if (ga_visit_env(env, "ga_rollout_env_steps", [&](auto* e) {
        n = e->n;
        act_width = ga_env_act_width(e);
        discrete = ga_env_discrete(e);
        return 0;
      }))
    return -1;
  if (norm && norm->act_low && ga_rescale_refused(norm, discrete, "ga_rollout_env_steps"))
    return -1;
  if (norm && norm->normalize_obs && (!raw_a || !raw_b)) {
    ga_set_error("ga_rollout_env_steps: observation normalisation needs the raw "
                 "observation buffers");
    return -1;
  }
  if (n_steps < 0 || head->col + n_steps > head->Tcap) {
    ga_set_error("ga_rollout_env_steps: steps exceed the rollout buffer");
    return -1;
  }
  if (!ga_policy_step_fused_supported(desc) && !ga_policy_step_rule(desc, PS_WMAX)) {
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
  // (the one launch rescales the actions itself where the kernel side says it does:
  // policy_fused.hip always, the recording fakes of the loop's first harness never)
  const bool rescale_in_launch = !(norm && nm.act_low) || ga_policy_env_step_rescales();
  if (fused_env_step_on() && rescale_in_launch && !head->noise && n_steps >= 1) {
    // every rollout step -- policy, env, bookkeeping, reset of the finished envs --
    // in ONE launch for all n_steps: a workgroup owns its envs for the whole rollout
    // (with nm.act_low set the env thread rescales its action row into
    // nm.scaled_action, as ga_action_rescale_f32 does below)
    r.col = h.col;
    r.next_obs = nxt;
    h.obs = cur;
    if (norm) {
      nm.raw_obs = raw_cur;
      nm.raw_next_obs = raw_nxt;
    }
    return ga_policy_env_step_fused_f32(desc, params, &h, env, &r, norm ? &nm : nullptr,
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
    // env step -> bookkeeping -> reset of the finished envs: one launch
    const float* env_action = h.action;
    if (norm && nm.act_low) {
      // NormalizedEnv.step: the wrapped env sees the rescaled, clipped action; the
      // batch keeps the policy's own (normalized_env.py:90-114)
      rc = ga_action_rescale_f32(n, act_width, h.action, h.lda, nm.act_low, nm.act_high,
                                 nm.expected_action_scale, nm.scaled_action, h.lda,
                                 stream);
      if (rc) return rc;
      env_action = nm.scaled_action;
    }
    rc = ga_env_step_record(env, &r, norm ? &nm : nullptr, env_action, h.lda, cur, stream);
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
