// The fake kernel side of garage_amd/csrc/rollout_loop.cpp: the launches
// ga_rollout_env_steps makes, defined once.  Each appends one line to g_log with every
// field a suite compares: columns, Philox steps, the observation buffers (A / B), the
// action rows (action / scaled), and what a rescaling launch is handed (bounds, scratch,
// scale).  Include once per program, after harness.h.
#pragma once
#include "../../garage_amd/csrc/internal.h"
#include "harness.h"

// ---- switches; a suite sets each one at entry ---------------------------------------------
// what ga_policy_env_step_rescales answers: the fused launch rescales the actions itself
// (1, as policy_fused.hip does), or the loop keeps ga_action_rescale_f32 between the policy
// step and the env step (0)
static int g_rescales_in_launch = 1;
// lines with the buffers' addresses and the NormalizedEnv flag (the synthetic-env checks)
// instead of the labels
static bool g_addresses = false;
// the buffers the labels name
static const float* g_obs_a = nullptr;
static const float* g_action = nullptr;
static const float* g_scaled = nullptr;

static const char* which(const void* p) { return p == g_obs_a ? "A" : "B"; }
static const char* rows(const void* p) {
  return p && p == g_action ? "action" : p && p == g_scaled ? "scaled" : "?";
}

extern "C" {
int ga_policy_env_step_rescales(void) { return g_rescales_in_launch; }

int ga_policy_step_fused_f32(const ga_mlp_desc*, const float*, const ga_head_args* a,
                             ga_stream_t) {
  if (g_addresses)
    logf("policy_step col=%lld step=%u obs=%p", (long long)a->col, a->step, (void*)a->obs);
  else
    logf("policy col=%lld step=%u obs=%s", (long long)a->col, a->step, which(a->obs));
  return 0;
}

int ga_action_rescale_f32(int64_t n, int A, const float* act, int64_t lda, const float*,
                          const float*, float scale, float* out, int64_t ldo, ga_stream_t) {
  logf("rescale n=%lld A=%d %s->%s lda=%lld ldo=%lld scale=%g", (long long)n, A, rows(act),
       rows(out), (long long)lda, (long long)ldo, scale);
  return 0;
}

int ga_policy_env_step_fused_f32(const ga_mlp_desc*, const float*, const ga_head_args* h,
                                 const ga_env_ref* env, const ga_record_args* r,
                                 const ga_norm_args* nm, int64_t n_steps, ga_stream_t) {
  if (g_addresses)
    logf("policy_env_step col=%lld step=%u obs=%p next=%p norm=%d steps=%lld",
         (long long)h->col, h->step, (void*)h->obs, (void*)r->next_obs, nm != nullptr,
         (long long)n_steps);
  else
    logf("fused kind=%d col=%lld steps=%lld obs=%s next=%s bounds=%d scratch=%s scale=%g",
         env->kind, (long long)h->col, (long long)n_steps, which(h->obs), which(r->next_obs),
         nm && nm->act_low && nm->act_high, nm ? rows(nm->scaled_action) : "-",
         nm ? nm->expected_action_scale : 0.f);
  return 0;
}

int ga_env_step_record(const ga_env_ref* env, const ga_record_args* r, const ga_norm_args* nm,
                       const float* act, int64_t, const float* obs, ga_stream_t) {
  if (g_addresses)
    logf("env_step col=%lld obs=%p next=%p act=%p norm=%d", (long long)r->col, (void*)obs,
         (void*)r->next_obs, (void*)act, nm != nullptr);
  else
    logf("env kind=%d col=%lld obs=%s next=%s act=%s", env->kind, (long long)r->col,
         which(obs), which(r->next_obs), rows(act));
  return 0;
}
}  // extern "C"
