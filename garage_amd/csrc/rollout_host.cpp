// The host side of a rollout step (the kernels of rollout.hip and policy_fused.hip): the
// one converter and check of each C-ABI struct (ga_head_to_dev, ga_record_to_dev /
// check_record, ga_env_to_dev / check_env, ga_build_env_step), the entry points of the
// per-layer path, and the fused step's predicates, switches, argument checks,
// FusedParams, grid, member split, choice of the instantiation (ps_variant) and profile
// counts (ps_count).  Host C++ only: the kernels are behind the launch seam of
// rollout_params.h, so this file builds for the CPU too and runs there against fakes of
// the seam under AddressSanitizer (tests/host/rollout_host_harness.cpp) -- a wrong
// extent here becomes an out-of-range device access.
#include "common.h"
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

#include "prof.h"

#include "rollout_params.h"

using namespace ga_rollout;

// ---- the head and the record of a step ---------------------------------------------------
static HeadDev ga_head_to_dev(const ga_head_args* a) {
  HeadDev d;
  d.n = a->n; d.env_id0 = a->env_id0; d.kind = a->kind; d.has_min = a->has_min;
  d.has_max = a->has_max; d.min_log_std = a->min_log_std; d.max_log_std = a->max_log_std;
  d.noise = a->noise; d.ldn = a->ldn; ga_key(a->seed, &d.k0, &d.k1); d.step = a->step;
  d.double_softmax = a->double_softmax; d.obs = a->obs; d.ldo = a->ldo; d.col = a->col;
  d.Tcap = a->Tcap; d.action = a->action; d.lda = a->lda; d.obs_buf = a->obs_buf;
  d.act_buf = a->act_buf; d.head_buf = a->head_buf; d.ldh = a->ldh;
  return d;
}

// the kernel-side record of a step, and its checks (`n`: the batch it must cover)
static RecordParams ga_record_to_dev(const ga_record_args* a) {
  RecordParams p;
  p.n = a->n; p.col = a->col; p.Tcap = a->Tcap;
  p.max_episode_length = a->max_episode_length; p.reward = a->reward;
  p.step_type = a->step_type; p.next_obs = a->next_obs; p.ldo = a->ldo;
  p.obs_dim = a->obs_dim; p.ep_t = a->ep_t; p.rew_buf = a->rew_buf;
  p.st_buf = a->st_buf; p.tail_buf = a->tail_buf; p.lastobs_buf = a->lastobs_buf;
  p.done = a->done; p.step_eps = a->step_eps; p.step_samples = a->step_samples;
  p.terminal_only = a->terminal_only;
  return p;
}

static int check_record(const ga_record_args* a, int64_t n, const char* who) {
  GA_REQUIRE(a->reward && a->step_type && a->next_obs && a->ep_t && a->rew_buf &&
                 a->st_buf && a->tail_buf && a->lastobs_buf && a->done &&
                 a->step_eps && a->step_samples,
             "%s: null pointer", who);
  GA_REQUIRE(a->n == n && n > 0 && a->col >= 0 && a->col < a->Tcap,
             "%s: col %lld out of range (Tcap %lld)", who, (long long)a->col,
             (long long)a->Tcap);
  GA_REQUIRE(a->max_episode_length >= 1 && a->max_episode_length <= 65535,
             "%s: max_episode_length must be in 1..65535", who);
  // (the terminal observation is copied row to row, as ga_policy_head_sample's)
  GA_REQUIRE(a->obs_dim >= 0 && a->ldo >= a->obs_dim,
             "%s: leading dimensions too small (observation rows of %lld columns, "
             "obs_dim %d)", who, (long long)a->ldo, (int)a->obs_dim);
  return GA_OK;
}

// one thread per env: the grid of every launch of the per-layer path
static unsigned env_blocks(int64_t n) { return (unsigned)ga_ceil_div(n, 256); }

extern "C" int ga_policy_head_sample(const ga_head_args* a, ga_stream_t stream) {
  GA_REQUIRE(a && a->head && a->obs && a->action && a->obs_buf && a->act_buf,
             "ga_policy_head_sample: null pointer");
  GA_REQUIRE(a->n > 0 && a->A > 0 && a->ldh >= a->A && a->ldo >= a->obs_dim,
             "ga_policy_head_sample: bad sizes");
  GA_REQUIRE(a->col >= 0 && a->col < a->Tcap, "ga_policy_head_sample: col %lld out of "
             "range (Tcap %lld)", (long long)a->col, (long long)a->Tcap);
  GA_REQUIRE(a->kind == 1 || (a->log_std && a->lda >= a->A),
             "ga_policy_head_sample: gaussian head needs log_std and lda >= A");
  const HeadParams p = {ga_head_to_dev(a), a->A, a->head, a->log_std, a->obs_dim};
  ro_launch_head_sample(p, env_blocks(a->n), (hipStream_t)stream);
  GA_CHECK_LAUNCH("policy_head_sample");
  return GA_OK;
}

extern "C" int ga_record_step(const ga_record_args* a, ga_stream_t stream) {
  const char* who = "ga_record_step";
  GA_REQUIRE(a, "%s: null pointer", who);
  int rc = check_record(a, a->n, who);
  if (rc) return rc;
  ro_launch_record(ga_record_to_dev(a), env_blocks(a->n), (hipStream_t)stream);
  GA_CHECK_LAUNCH("record_step");
  return GA_OK;
}

// ---- the device envs ---------------------------------------------------------------
// The kernel-side struct of each C-ABI env.  info_ld: row stride of the env_info buffers
// (1: [n], Tcap: the [n, Tcap] record buffers).
static SynthEnv ga_env_to_dev(const ga_synth_env* e, int64_t) {
  SynthEnv d;
  d.n = e->n; d.env_id0 = e->env_id0; d.obs_dim = e->obs_dim; d.act_dim = e->act_dim;
  d.discrete = e->discrete; d.min_len = e->min_len; d.max_len = e->max_len;
  ga_key(e->seed, &d.k0, &d.k1);
  d.episode = e->episode; d.t = e->t; d.len = e->len;
  return d;
}

static PointEnv ga_env_to_dev(const ga_point_env* e, int64_t succ_ld) {
  PointEnv d;
  d.n = e->n; d.arena = e->arena_size; d.bonus = e->done_bonus;
  d.never_done = e->never_done; d.max_len = e->max_episode_length;
  d.point = e->point; d.goal = e->goal; d.t = e->t; d.success = e->success;
  d.succ_ld = succ_ld;
  return d;
}

static GridEnv ga_env_to_dev(const ga_grid_env* e, int64_t) {
  GridEnv d;
  d.n = e->n; d.rows = e->rows; d.cols = e->cols; d.max_len = e->max_episode_length;
  d.map = e->map; d.start = e->start; d.state = e->state; d.t = e->t;
  return d;
}

// the PointEnv part of a multi-task batch
static ga_point_env point_part(const ga_multi_point_env* e) {
  ga_point_env p;
  p.n = e->n; p.arena_size = e->arena_size; p.done_bonus = e->done_bonus;
  p.never_done = e->never_done; p.max_episode_length = e->max_episode_length;
  p.point = e->point; p.goal = e->goal; p.t = e->t; p.success = e->success;
  return p;
}

static MultiTaskEnv<PointEnv> ga_env_to_dev(const ga_multi_point_env* e, int64_t info_ld) {
  MultiTaskEnv<PointEnv> d;
  const ga_point_env p = point_part(e);
  d.n = e->n; d.in = ga_env_to_dev(&p, info_ld);
  d.num_tasks = e->num_tasks; d.strategy = e->strategy;
  d.one_hot = e->mode == GA_TASK_ADD_ONEHOT;
  ga_key(e->seed, &d.k0, &d.k1);
  d.payload = e->task_goals; d.last_task = e->last_task; d.resets = e->resets;
  d.task_id = e->task_id; d.info_ld = info_ld;
  return d;
}

// the five seeded state-vector kinds share their field names; MountainCar's
// `continuous` is the frame's `variant` (0 for the others, whose slot is padding)
static int state_env_variant(const ga_mountain_car_env* e) { return e->continuous; }
template <class GaEnv>
static int state_env_variant(const GaEnv*) { return 0; }

template <class GaEnv, class K = typename ga_state_kind_of<GaEnv>::type>
static StateEnv<K> ga_env_to_dev(const GaEnv* e, int64_t) {
  StateEnv<K> d;
  d.n = e->n; d.env_id0 = e->env_id0; d.max_len = e->max_episode_length;
  d.variant = state_env_variant(e);
  ga_key(e->seed, &d.k0, &d.k1);
  d.state = e->state; d.t = e->t; d.resets = e->resets;
  return d;
}

static int check_env(const ga_synth_env* e, const char* who) {
  GA_REQUIRE(e && e->episode && e->t && e->len, "%s: null env state", who);
  GA_REQUIRE(e->n > 0 && e->obs_dim > 0 && e->act_dim > 0, "%s: bad env sizes", who);
  GA_REQUIRE(e->min_len >= 1 && e->min_len <= e->max_len && e->max_len <= 65535,
             "%s: episode lengths must satisfy 1 <= min <= max <= 65535", who);
  return GA_OK;
}

static int check_env(const ga_point_env* e, const char* who) {
  GA_REQUIRE(e && e->point && e->goal && e->t, "%s: null env state", who);
  GA_REQUIRE(e->n > 0, "%s: bad env size", who);
  GA_REQUIRE(e->arena_size >= 0.f, "%s: arena_size must be >= 0", who);
  GA_REQUIRE(e->max_episode_length >= 1 && e->max_episode_length <= 65535,
             "%s: max_episode_length must be in 1..65535", who);
  return GA_OK;
}

static int check_env(const ga_grid_env* e, const char* who) {
  GA_REQUIRE(e && e->map && e->start && e->state && e->t, "%s: null env state", who);
  GA_REQUIRE(e->n > 0 && e->rows > 0 && e->cols > 0 && e->rows <= 4096 &&
                 e->cols <= 4096 && (int64_t)e->rows * e->cols <= (1 << 20),
             "%s: bad env sizes", who);
  GA_REQUIRE(e->max_episode_length >= 1 && e->max_episode_length <= 65535,
             "%s: max_episode_length must be in 1..65535", who);
  return GA_OK;
}

static int check_env(const ga_multi_point_env* e, const char* who) {
  GA_REQUIRE(e && e->point && e->goal && e->t && e->task_goals && e->last_task &&
                 e->resets, "%s: null env state", who);
  const ga_point_env p = point_part(e);
  int rc = check_env(&p, who);
  if (rc) return rc;
  GA_REQUIRE(e->num_tasks >= 1 && e->num_tasks <= 256,
             "%s: num_tasks must be in 1..256 (got %d)", who, e->num_tasks);
  GA_REQUIRE(e->strategy == GA_TASK_ROUND_ROBIN || e->strategy == GA_TASK_UNIFORM_RANDOM,
             "%s: unknown sample strategy %d", who, e->strategy);
  GA_REQUIRE(e->mode == GA_TASK_VANILLA || e->mode == GA_TASK_ADD_ONEHOT,
             "%s: unknown mode %d", who, e->mode);
  return GA_OK;
}

template <class GaEnv, class K = typename ga_state_kind_of<GaEnv>::type>
static int check_env(const GaEnv* e, const char* who) {
  GA_REQUIRE(e && e->state && e->t && e->resets, "%s: null env state", who);
  GA_REQUIRE(e->n > 0, "%s: bad env size", who);
  GA_REQUIRE(e->max_episode_length >= 1 && e->max_episode_length <= 65535,
             "%s: max_episode_length must be in 1..65535", who);
  const int variant = state_env_variant(e);
  GA_REQUIRE(variant == 0 || variant == 1, "%s: continuous must be 0 or 1", who);
  return GA_OK;
}

// Validated conversion of the C-ABI arguments of one env step into EnvStepArgsT: the env,
// the record and the NormalizedEnv part.  rescale_inside: the caller's kernel rescales the
// policy's action itself when norm->act_low is set (the fused rollout step); otherwise
// the bounds are not read and the env steps on `actions` as they are
// (ga_env_step_record).
template <class GaEnv>
static int ga_build_env_step(const GaEnv* env, const ga_record_args* a,
                             const ga_norm_args* norm, const float* actions, int64_t lda,
                             const float* obs, const char* who,
                             ga_env_step_args_t<GaEnv>* out, bool rescale_inside = false) {
  int rc = check_env(env, who);
  if (rc) return rc;
  const int obs_dim = ga_env_obs_dim(env);
  GA_REQUIRE(a, "%s: null pointer", who);
  if (std::is_same<GaEnv, ga_multi_point_env>::value)
    GA_REQUIRE(a->ldo >= obs_dim,
               "%s: observation rows of %lld columns are narrower than 3 + num_tasks = %d",
               who, (long long)a->ldo, obs_dim);
  GA_REQUIRE(actions && obs, "%s: null pointer", who);
  rc = check_record(a, env->n, who);
  if (rc) return rc;
  GA_REQUIRE(a->ldo >= obs_dim && a->obs_dim == obs_dim && lda >= ga_env_act_width(env),
             "%s: leading dimensions too small", who);
  NormParams nm;
  memset(&nm, 0, sizeof(nm));
  const float* raw_obs = obs;
  float* raw_next = (float*)a->next_obs;
  if (norm) {
    nm.norm_obs = norm->normalize_obs != 0;
    nm.norm_reward = norm->normalize_reward != 0;
    nm.scale_reward = norm->reward_scale != 1.0;
    nm.obs_mean = norm->obs_mean; nm.obs_var = norm->obs_var;
    nm.obs_alpha = norm->obs_alpha; nm.rew_mean = norm->reward_mean;
    nm.rew_var = norm->reward_var; nm.rew_alpha = norm->reward_alpha;
    nm.rew_scale = norm->reward_scale;
    GA_REQUIRE(!nm.norm_obs || (nm.obs_mean && nm.obs_var && norm->raw_obs &&
                                norm->raw_next_obs),
               "%s: observation statistics / raw buffers", who);
    GA_REQUIRE(!nm.norm_reward || (nm.rew_mean && nm.rew_var), "%s: reward statistics",
               who);
    if (nm.norm_obs) {
      raw_obs = norm->raw_obs;
      raw_next = norm->raw_next_obs;
    }
    if (rescale_inside && norm->act_low) {
      // normalized_env.py:90-100 in the env thread of the caller's kernel: the scratch
      // rows have the action rows' stride
      rc = ga_rescale_refused(norm, ga_env_discrete(env), who);
      if (rc) return rc;
      nm.act_low = norm->act_low; nm.act_high = norm->act_high;
      nm.expected_action_scale = norm->expected_action_scale;
      nm.scaled_action = norm->scaled_action; nm.scaled_ld = lda;
    }
  }
  out->e = ga_env_to_dev(env, a->Tcap);  // env_infos go into the [n, Tcap] buffers
  out->p = ga_record_to_dev(a); out->nm = nm;
  out->actions = actions; out->lda = lda; out->raw_obs = raw_obs; out->raw_next = raw_next;
  out->seen_next = (float*)a->next_obs; out->reward = (float*)a->reward;
  out->step_type = (uint8_t*)a->step_type;
  return GA_OK;
}

// Environment.reset (_environment.py:237-276; envs/point_env.py:79-98,
// grid_world_env.py:91-109, multi_env_wrapper.py:169-194)
extern "C" int ga_env_reset(const ga_env_ref* ref, const uint8_t* mask, float* obs,
                            int64_t ldo, ga_stream_t stream) {
  const char* who = "ga_env_reset";
  return ga_visit_env(ref, who, [&](auto* env) {
    int rc = check_env(env, who);
    if (rc) return rc;
    GA_REQUIRE(obs && ldo >= ga_env_obs_dim(env), "%s: bad obs buffer", who);
    ro_launch_env_reset(ga_env_to_dev(env, 1), mask, obs, ldo, env_blocks(env->n),
                        (hipStream_t)stream);
    GA_CHECK_LAUNCH("env_reset");
    return GA_OK;
  });
}

// Environment.step (envs/point_env.py:100-170, grid_world_env.py:111-215,
// multi_env_wrapper.py:196-226)
extern "C" int ga_env_step(const ga_env_ref* ref, const float* actions, int64_t lda,
                           const float* obs, float* next_obs, int64_t ldo, float* reward,
                           uint8_t* step_type, ga_stream_t stream) {
  const char* who = "ga_env_step";
  return ga_visit_env(ref, who, [&](auto* env) {
    int rc = check_env(env, who);
    if (rc) return rc;
    const bool reads_obs = std::is_same<decltype(env), const ga_synth_env*>::value;
    GA_REQUIRE(actions && next_obs && reward && step_type && (obs || !reads_obs),
               "%s: null pointer", who);
    GA_REQUIRE(ldo >= ga_env_obs_dim(env) && lda >= ga_env_act_width(env),
               "%s: leading dimensions too small", who);
    ro_launch_env_step(ga_env_to_dev(env, 1), actions, lda, obs, next_obs, ldo, reward,
                       step_type, env_blocks(env->n), (hipStream_t)stream);
    GA_CHECK_LAUNCH("env_step");
    return GA_OK;
  });
}

// the step + normalized_env.py:134-164 + vec_worker.py:176-204
extern "C" int ga_env_step_record(const ga_env_ref* ref, const ga_record_args* rec,
                                  const ga_norm_args* norm, const float* actions,
                                  int64_t lda, const float* obs, ga_stream_t stream) {
  const char* who = "ga_env_step_record";
  return ga_visit_env(ref, who, [&](auto* env) {
    using GaEnv = std::remove_cv_t<std::remove_pointer_t<decltype(env)>>;
    ga_env_step_args_t<GaEnv> args;
    int rc = ga_build_env_step(env, rec, norm, actions, lda, obs, who, &args);
    if (rc) return rc;
    ro_launch_env_step_record(args, env_blocks(rec->n), (hipStream_t)stream);
    GA_CHECK_LAUNCH("env_step_record");
    return GA_OK;
  });
}

// ---- the fused rollout step (policy_fused.hip) -------------------------------------------
static NetDev net_to_dev(const ga_mlp_desc* d) {
  NetDev n;
  n.n_layers = d->n_layers;
  for (int i = 0; i < 9; ++i) n.dims[i] = d->dims[i];
  for (int i = 0; i < 8; ++i) { n.w_off[i] = d->w_off[i]; n.b_off[i] = d->b_off[i]; }
  return n;
}

// GARAGE_AMD_ROLLOUT_WIDE=0: networks only the WIDTH = 512 kernels take go back to the
// per-layer path; GARAGE_AMD_ROLLOUT_RESIDENT=0: a whole rollout streams its weights as a
// single step does (A/B runs).  Read at the first question; ga_rollout_set_switches
// (rollout_params.h) is the harness's way to flip them.
static int g_ps_wide = -1, g_ps_resident = -1;
static bool switch_on(int* state, const char* name) {
  if (*state < 0) {
    const char* e = getenv(name);
    *state = (e && atoi(e) == 0) ? 0 : 1;
  }
  return *state != 0;
}
static bool ps_wide_on() { return switch_on(&g_ps_wide, "GARAGE_AMD_ROLLOUT_WIDE"); }
static bool ps_resident_on() {
  return switch_on(&g_ps_resident, "GARAGE_AMD_ROLLOUT_RESIDENT");
}
void ga_rollout_set_switches(int wide, int resident) {
  g_ps_wide = wide != 0;
  g_ps_resident = resident != 0;
}

// 1 when ga_policy_step_fused_f32 supports this network shape at WIDTH = 256.
extern "C" int ga_policy_step_fused_supported(const ga_mlp_desc* d) {
  return ga_policy_step_rule(d, PS_HMAX);
}

// 1 when ga_policy_step_fused_f32 / ga_policy_env_step_fused_f32 / ga_rollout_env_steps
// take this network: what the predicate above accepts (the kernels it always had), or
// layer inputs up to 512 (the WIDTH = 512 kernels).
extern "C" int ga_policy_step_wide_supported(const ga_mlp_desc* d) {
  if (ga_policy_step_fused_supported(d)) return 1;
  return ps_wide_on() && ga_policy_step_rule(d, PS_WMAX);
}

// ---- which instantiation a launch runs (PsVariant, rollout_params.h), written once ------
// Every descriptor the 256 rule accepts keeps the kernel it had; the others run at 512
// unless switched off (width 0: refused).  A whole rollout in one launch (n_steps > 1)
// keeps the weights on the CU where the kernel can: observations no wider than one k
// chunk, one or two hidden layers, layer inputs up to 256.  The tanh / linear-output /
// no-LayerNorm network keeps the kernel it always had (general 0).
static PsVariant ps_variant(const ga_mlp_desc* d, int64_t n_steps, bool wide_on,
                            bool resident_on) {
  PsVariant v = {0, 0, 0};
  if (ga_policy_step_rule(d, PS_HMAX)) v.width = PS_HMAX;
  else if (wide_on && ga_policy_step_rule(d, PS_WMAX)) v.width = PS_WMAX;
  else return v;
  v.resident = v.width == PS_HMAX && n_steps > 1 && d->dims[0] <= PS_KC &&
               (d->n_layers == 2 || d->n_layers == 3) && resident_on;
  v.general = d->hidden_act != 0 || d->output_act != 0 || d->layer_norm;
  return v;
}

// ... and the profile counters it bumps (prof.h), in this order.  GA_PROF_ROLLOUT: a whole
// rollout with resident weights, and every whole rollout of the population entry point
// (n_members >= 1) whatever the kernel; GA_PROF_ROLLOUT_WIDE: a whole rollout at 512.
static void ps_count(PsVariant v, int64_t n_steps, int64_t n_members) {
  if (n_steps > 1 && (v.resident || n_members >= 1)) ga_prof_count(GA_PROF_ROLLOUT);
  if (n_steps > 1 && v.width == PS_WMAX) ga_prof_count(GA_PROF_ROLLOUT_WIDE);
}

static long long* g_ps_dbg = nullptr;
// developer hook: phase timestamps (100 MHz wall clock) of workgroup 0 of the most
// recent fused rollout step -- first call arms it, second call reads 32 values back
// (0 start, 1 observations staged, 2 + l hidden layer l done, 10 output layer,
// 11 sampled + env stepped; + 16: the same of the resident-weights kernel; the middle step of the launch;
// the WIDTH = 512 kernels write the streamed slots)
extern "C" int ga_policy_step_debug(long long* host_out32) {
  if (!g_ps_dbg) {
    if (hipMalloc(&g_ps_dbg, 32 * sizeof(long long)) != hipSuccess) return -1;
    (void)hipMemset(g_ps_dbg, 0, 32 * sizeof(long long));
    return 1;
  }
  (void)hipDeviceSynchronize();
  return hipMemcpy(host_out32, g_ps_dbg, 32 * sizeof(long long), hipMemcpyDeviceToHost) ==
                 hipSuccess ? 0 : -1;
}

// Check, fill, choose, count, launch.  `head` of args is ignored (the means / scores
// stay on chip); everything else as in ga_policy_head_sample.  n_members > 1
// (ga_policy_env_step_members_f32, which checked the split): member m owns the
// blocks / n_members workgroups of its envs.
template <class Env>
static int policy_step_launch(const ga_mlp_desc* d, const float* params,
                              const ga_head_args* a, const EnvStepArgsT<Env>* es,
                              int64_t n_steps, hipStream_t stream, int64_t n_members = 0,
                              int64_t member_stride = 0) {
  GA_REQUIRE(d && params && a, "ga_policy_step_fused_f32: null pointer");
  const PsVariant v = ps_variant(d, n_steps, ps_wide_on(), ps_resident_on());
  GA_REQUIRE(v.width, "ga_policy_step_fused_f32: unsupported network shape");
  GA_REQUIRE(a->obs && a->action && a->obs_buf && a->act_buf,
             "ga_policy_step_fused_f32: null buffer");
  GA_REQUIRE(a->n > 0 && a->A == d->dims[d->n_layers] && a->obs_dim == d->dims[0],
             "ga_policy_step_fused_f32: head / network size mismatch");
  GA_REQUIRE(a->col >= 0 && a->col < a->Tcap,
             "ga_policy_step_fused_f32: col out of range");
  GA_REQUIRE(ga_aligned16(params), "ga_policy_step_fused_f32: params alignment");
  if (d->layer_norm)
    for (int l = 0; l + 1 < d->n_layers; ++l)
      GA_REQUIRE(d->ln_off[l] > 0 && d->ln_off[l] % 4 == 0,
                 "ga_policy_step_fused_f32: ln_off[%d] is not a multiple of 4", l);
  FusedParams<Env> p;
  p.net = net_to_dev(d);
  p.params = params;
  p.hd = ga_head_to_dev(a);
  p.dbg = g_ps_dbg;
  p.hidden_act = d->hidden_act; p.output_act = d->output_act;
  p.layer_norm = d->layer_norm != 0;
  for (int i = 0; i < 8; ++i) p.ln_off[i] = d->ln_off[i];
  p.env_step = es ? (es->nm.act_low ? 1 | ENV_STEP_RESCALE : 1) : 0;
  p.n_steps = (int)n_steps;
  const unsigned blocks = (unsigned)ga_ceil_div(a->n, PS_ROWS);
  p.wg_per_member = n_members > 1 ? (int)(blocks / n_members) : 1;
  p.member_stride = n_members > 1 ? (int)member_stride : 0;
  if (es) p.es = *es;
  else memset(&p.es, 0, sizeof(p.es));
  ps_count(v, n_steps, n_members);
  ps_launch_policy_step(p, v, blocks, stream);
  if (v.width == PS_WMAX) GA_CHECK_LAUNCH("policy_step_wide");
  else GA_CHECK_LAUNCH("policy_step_fused");
  return GA_OK;
}

extern "C" int ga_policy_step_fused_f32(const ga_mlp_desc* d, const float* params,
                                        const ga_head_args* a, ga_stream_t stream) {
  return policy_step_launch<SynthEnv>(d, params, a, nullptr, 1, (hipStream_t)stream);
}

// The same launch followed, per env, by the env's step + NormalizedEnv statistics +
// bookkeeping + reset (what ga_env_step_record does as its own launch), for n_steps
// consecutive rollout steps: every workgroup takes its 16 envs through all of them
// (nothing couples envs within a rollout), alternating between `a->obs` and
// `rec->next_obs` (and the raw pair of `norm`).  `a->action` is what the env is
// stepped with -- or, with norm->act_low set, its rescaled copy in
// norm->scaled_action, which the env thread writes (ga_build_env_step refuses missing
// bounds or scratch and a discrete kind; none of the checks touches the device).
static int policy_env_step(const char* who, const ga_mlp_desc* d, const float* params,
                           const ga_head_args* a, const ga_env_ref* ref,
                           const ga_record_args* rec, const ga_norm_args* norm,
                           int64_t n_steps, int64_t n_members, int64_t member_stride,
                           ga_stream_t stream) {
  return ga_visit_env(ref, who, [&](auto* env) {
    GA_REQUIRE(a && rec, "%s: null pointer", who);
    GA_REQUIRE(n_steps >= 1 && a->col + n_steps <= a->Tcap,
               "%s: steps exceed the rollout buffer", who);
    GA_REQUIRE(!a->noise || n_steps == 1, "%s: teacher-forced noise is per step", who);
    using GaEnv = std::remove_cv_t<std::remove_pointer_t<decltype(env)>>;
    ga_env_step_args_t<GaEnv> es;
    int rc = ga_build_env_step(env, rec, norm, a->action, a->lda, a->obs, who, &es,
                               /*rescale_inside=*/true);
    if (rc) return rc;
    GA_REQUIRE(es.e.n == a->n, "%s: env count mismatch", who);
    // (the kernel rescales the head's A columns)
    GA_REQUIRE(!es.nm.act_low || a->A == ga_env_act_width(env),
               "%s: action rescale of %d columns for an env of %d", who, a->A,
               ga_env_act_width(env));
    GA_REQUIRE(es.p.col == a->col && es.p.col + n_steps <= es.p.Tcap,
               "%s: record columns do not match the policy's", who);
    return policy_step_launch(d, params, a, &es, n_steps, (hipStream_t)stream, n_members,
                              member_stride);
  });
}

extern "C" int ga_policy_env_step_fused_f32(const ga_mlp_desc* d, const float* params,
                                            const ga_head_args* a, const ga_env_ref* ref,
                                            const ga_record_args* rec,
                                            const ga_norm_args* norm, int64_t n_steps,
                                            ga_stream_t stream) {
  return policy_env_step("ga_policy_env_step_fused_f32", d, params, a, ref, rec, norm,
                         n_steps, 0, 0, stream);
}

// floats of the parameter vector `d` describes: the end of its last block
static int64_t desc_flat_size(const ga_mlp_desc* d) {
  int64_t end = 4;
  for (int l = 0; l < d->n_layers; ++l) {
    end = std::max(end, d->w_off[l] + (int64_t)d->dims[l + 1] * ((d->dims[l] + 3) & ~3));
    end = std::max(end, d->b_off[l] + ((d->dims[l + 1] + 3) & ~3));
    if (d->layer_norm && l + 1 < d->n_layers)
      end = std::max(end, d->ln_off[l] + 2 * ((d->dims[l] + 3) & ~3));
  }
  return end;
}

// The same launch over a population: member m's envs [m g, (m + 1) g), g = n /
// n_members, are stepped by the parameter vector at params + m * member_stride.  Every
// check precedes the first device call.
extern "C" int ga_policy_env_step_members_f32(const ga_mlp_desc* d, const float* params,
                                              const ga_head_args* a, const ga_env_ref* ref,
                                              const ga_record_args* rec,
                                              const ga_norm_args* norm, int64_t n_steps,
                                              int64_t n_members, int64_t member_stride,
                                              ga_stream_t stream) {
  const char* who = "ga_policy_env_step_members_f32";
  GA_REQUIRE(d && params && a && ref && rec, "%s: null pointer", who);
  GA_REQUIRE(n_members >= 1, "%s: n_members must be at least 1", who);
  GA_REQUIRE(a->n > 0 && a->n % n_members == 0,
             "%s: %lld envs do not split into %lld members", who, (long long)a->n,
             (long long)n_members);
  // (one member is the single-policy launch, whose last workgroup may be ragged)
  GA_REQUIRE(n_members == 1 || a->n / n_members % PS_ROWS == 0,
             "%s: %lld envs per member are not a multiple of the %d rows of a workgroup",
             who, (long long)(a->n / n_members), PS_ROWS);
  GA_REQUIRE(ga_policy_step_wide_supported(d),
             "%s: network not supported by the fused step", who);
  GA_REQUIRE(member_stride % 4 == 0 && member_stride >= desc_flat_size(d),
             "%s: member_stride %lld is not a multiple of 4 floats or is smaller than "
             "the %lld floats of a parameter vector",
             who, (long long)member_stride, (long long)desc_flat_size(d));
  // (the kernel adds a member's offset as a 32-bit count of floats)
  GA_REQUIRE((n_members - 1) * member_stride + desc_flat_size(d) < (1ll << 31),
             "%s: %lld members x %lld floats exceed 2^31 floats", who,
             (long long)n_members, (long long)member_stride);
  GA_REQUIRE(!a->noise, "%s: teacher-forced noise is not supported", who);
  GA_REQUIRE(!(norm && norm->act_low),
             "%s: the action rescale is its own launch (not supported)", who);
  return policy_env_step(who, d, params, a, ref, rec, norm, n_steps, n_members,
                         member_stride, stream);
}

// Training / evaluation forward of the whole MLP in one launch (same contract
// as ga_mlp_forward_f32, which dispatches here when the shape is supported).
extern "C" int ga_mlp_forward_fused_f32(const ga_mlp_desc* d, const float* params,
                                        const float* X, int64_t ldx,
                                        const int32_t* row_idx, int64_t M,
                                        float* acts, float* out, int64_t ldo,
                                        ga_stream_t stream) {
  GA_REQUIRE(d && params && X && out, "ga_mlp_forward_fused_f32: null pointer");
  // (this kernel is the tanh network only; the rollout step's predicate is wider)
  GA_REQUIRE(ga_policy_step_fused_supported(d) && d->hidden_act == 0 &&
                 d->output_act == 0 && !d->layer_norm,
             "ga_mlp_forward_fused_f32: unsupported network shape or options");
  GA_REQUIRE(d->n_layers == 1 || acts, "ga_mlp_forward_fused_f32: acts needed");
  GA_REQUIRE(M > 0 && M < (1ll << 31), "ga_mlp_forward_fused_f32: bad M");
  GA_REQUIRE(ga_aligned16(params), "ga_mlp_forward_fused_f32: params alignment");
  TrainFwdParams p;
  p.net = net_to_dev(d);
  for (int i = 0; i < 8; ++i) p.act_off[i] = d->act_off[i];
  p.params = params; p.X = X; p.ldx = ldx; p.idx = row_idx; p.M = M; p.acts = acts;
  p.out = out; p.ldo = ldo;
  ps_launch_train_forward(p, (unsigned)ga_ceil_div(M, PS_TRAIN_ROWS), (hipStream_t)stream);
  GA_CHECK_LAUNCH("mlp_train_fwd_fused");
  return GA_OK;
}
