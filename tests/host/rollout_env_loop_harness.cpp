// Host-logic harness for ga_rollout_env_steps (garage_amd/csrc/rollout_loop.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-env-loop`).  The
// kernel entry points the loop calls are fakes that record each call, so the checks
// are about the loop itself: which launch a rollout takes for each env kind, the
// ping-pong of the observation buffers, the columns and Philox steps, the action
// rescale, and that argument errors are refused before anything is launched.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/garage_amd.h"
#include "../../garage_amd/csrc/internal.h"

static std::vector<std::string> g_log;
static std::string g_error;
// log lines with buffer labels (A / B), or -- for the synthetic-env checks -- with the
// buffers' addresses and the NormalizedEnv flag
static bool g_addresses = false;

static void logf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log.push_back(buf);
}

void ga_set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}

extern "C" int ga_policy_step_fused_supported(const ga_mlp_desc* d) {
  return d->n_layers >= 1;
}

static float* g_obs_a;  // labels for the two observation buffers
static const char* which(const void* p) { return p == g_obs_a ? "A" : "B"; }

extern "C" int ga_policy_step_fused_f32(const ga_mlp_desc*, const float*,
                                        const ga_head_args* a, ga_stream_t) {
  if (g_addresses)
    logf("policy_step col=%lld step=%u obs=%p", (long long)a->col, a->step, (void*)a->obs);
  else
    logf("policy col=%lld step=%u obs=%s", (long long)a->col, a->step, which(a->obs));
  return 0;
}

extern "C" int ga_action_rescale_f32(int64_t n, int A, const float*, int64_t, const float*,
                                     const float*, float, float*, int64_t, ga_stream_t) {
  logf("rescale n=%lld A=%d", (long long)n, A);
  return 0;
}

extern "C" int ga_policy_env_step_fused_f32(const ga_mlp_desc*, const float*,
                                            const ga_head_args* h, const ga_env_ref* env,
                                            const ga_record_args* r, const ga_norm_args* nm,
                                            int64_t n_steps, ga_stream_t) {
  if (g_addresses)
    logf("policy_env_step col=%lld step=%u obs=%p next=%p norm=%d steps=%lld",
         (long long)h->col, h->step, (void*)h->obs, (void*)r->next_obs, nm != nullptr,
         (long long)n_steps);
  else
    logf("fused kind=%d col=%lld steps=%lld obs=%s next=%s", env->kind, (long long)h->col,
         (long long)n_steps, which(h->obs), which(r->next_obs));
  return 0;
}

extern "C" int ga_env_step_record(const ga_env_ref* env, const ga_record_args* r,
                                  const ga_norm_args* nm, const float* act, int64_t,
                                  const float* obs, ga_stream_t) {
  if (g_addresses)
    logf("env_step col=%lld obs=%p next=%p act=%p norm=%d", (long long)r->col, (void*)obs,
         (void*)r->next_obs, (void*)act, nm != nullptr);
  else
    logf("env kind=%d col=%lld obs=%s next=%s", env->kind, (long long)r->col, which(obs),
         which(r->next_obs));
  return 0;
}

static int count(const char* prefix) {
  int n = 0;
  for (auto& l : g_log) n += l.rfind(prefix, 0) == 0;
  return n;
}

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

int main() {
  std::vector<float> a(64), b(64), lo(2, -1.f), hi(2, 1.f), scaled(64);
  g_obs_a = a.data();
  ga_mlp_desc desc;
  memset(&desc, 0, sizeof(desc));
  desc.n_layers = 3;
  float params[4] = {0};
  ga_head_args head;
  memset(&head, 0, sizeof(head));
  head.n = 8; head.Tcap = 16; head.col = 2; head.step = 40;
  ga_record_args rec;
  memset(&rec, 0, sizeof(rec));
  int32_t scratch[8];
  ga_point_env point;
  memset(&point, 0, sizeof(point));
  point.n = 8;
  ga_grid_env grid;
  memset(&grid, 0, sizeof(grid));
  grid.n = 8;
  ga_env_ref pref = {GA_ENV_POINT, 0, &point};
  ga_env_ref gref = {GA_ENV_GRID, 0, &grid};
  (void)scratch;

  // argument errors: nothing launched
  CHECK(ga_rollout_env_steps(&desc, params, &head, nullptr, &rec, a.data(), b.data(),
                             nullptr, nullptr, nullptr, 3, nullptr) < 0);
  ga_env_ref bad = {9, 0, &point};
  CHECK(ga_rollout_env_steps(&desc, params, &head, &bad, &rec, a.data(), b.data(), nullptr,
                             nullptr, nullptr, 3, nullptr) < 0);
  CHECK(g_error.find("unknown env kind") != std::string::npos);
  CHECK(ga_rollout_env_steps(&desc, params, &head, &pref, &rec, a.data(), b.data(),
                             nullptr, nullptr, nullptr, 15, nullptr) < 0);
  CHECK(g_error.find("exceed") != std::string::npos);
  ga_norm_args nm;
  memset(&nm, 0, sizeof(nm));
  nm.act_low = lo.data(); nm.act_high = hi.data(); nm.scaled_action = scaled.data();
  CHECK(ga_rollout_env_steps(&desc, params, &head, &gref, &rec, a.data(), b.data(), &nm,
                             nullptr, nullptr, 3, nullptr) < 0);
  CHECK(g_error.find("continuous") != std::string::npos);
  CHECK(g_log.empty());

  // the whole rollout in one fused launch
  CHECK(ga_rollout_env_steps(&desc, params, &head, &gref, &rec, a.data(), b.data(),
                             nullptr, nullptr, nullptr, 5, nullptr) == 0);
  CHECK(g_log.size() == 1 && g_log[0] == "fused kind=2 col=2 steps=5 obs=A next=B");

  // two launches per step: columns, Philox steps and buffers alternate
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(ga_rollout_env_steps(&desc, params, &head, &gref, &rec, a.data(), b.data(),
                             nullptr, nullptr, nullptr, 3, nullptr) == 0);
  const char* want[] = {"policy col=2 step=40 obs=A", "env kind=2 col=2 obs=A next=B",
                        "policy col=3 step=41 obs=B", "env kind=2 col=3 obs=B next=A",
                        "policy col=4 step=42 obs=A", "env kind=2 col=4 obs=A next=B"};
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want[i]);

  // action rescale (PointEnv's Box): per-step launches even with fusion on
  g_log.clear();
  ga_set_fused_env_step(1);
  CHECK(ga_rollout_env_steps(&desc, params, &head, &pref, &rec, a.data(), b.data(), &nm,
                             nullptr, nullptr, 2, nullptr) == 0);
  const char* want2[] = {"policy col=2 step=40 obs=A", "rescale n=8 A=2",
                         "env kind=1 col=2 obs=A next=B", "policy col=3 step=41 obs=B",
                         "rescale n=8 A=2", "env kind=1 col=3 obs=B next=A"};
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want2[i]);

  // the synthetic env takes the same loop: the observation buffers ping-pong
  {
    g_log.clear();
    g_addresses = true;
    ga_head_args h;
    memset(&h, 0, sizeof(h));
    h.col = 3; h.Tcap = 16; h.step = 100;
    ga_synth_env env;
    memset(&env, 0, sizeof(env));
    env.n = 4; env.act_dim = 2;
    ga_env_ref sref = {GA_ENV_SYNTH, 0, &env};
    float A[4], B[4];
    CHECK(ga_rollout_env_steps(&desc, params, &h, &sref, &rec, A, B, nullptr, nullptr,
                               nullptr, 3, nullptr) == 0);
    // (ONE launch for all the steps by default)
    CHECK(count("policy_env_step") == 1 && count("policy_step ") == 0);
    char want[160];
    snprintf(want, sizeof(want),
             "policy_env_step col=3 step=100 obs=%p next=%p norm=0 steps=3", (void*)A,
             (void*)B);
    CHECK(count(want) == 1);
    ga_set_fused_env_step(0);
    g_log.clear();
    CHECK(ga_rollout_env_steps(&desc, params, &h, &sref, &rec, A, B, nullptr, nullptr,
                               nullptr, 3, nullptr) == 0);
    CHECK(count("policy_step") == 3 && count("env_step col") == 3);
    snprintf(want, sizeof(want), "env_step col=4 obs=%p next=%p", (void*)B, (void*)A);
    CHECK(count(want) == 1);
    ga_set_fused_env_step(1);
    CHECK(ga_rollout_env_steps(&desc, params, &h, &sref, &rec, A, B, nullptr, nullptr,
                               nullptr, 14, nullptr) != 0);  // past Tcap
  }

  if (g_fail) {
    fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("rollout_env_loop harness: all checks passed\n");
  return 0;
}
