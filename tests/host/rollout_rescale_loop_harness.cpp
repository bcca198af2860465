// Host-logic harness for ga_rollout_env_steps (garage_amd/csrc/rollout_loop.cpp) under
// NormalizedEnv's action rescale, built with -fsanitize=address,undefined on the CPU
// (`make asan-rescale-loop`).  The kernel side is recording fakes that, like
// policy_fused.hip, rescale inside the fused launch: a rescaled rollout is ONE launch
// that is handed the bounds and the scratch, three launches per step under
// ga_set_fused_env_step(0) or teacher-forced noise, and the refusals keep their order.
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
extern "C" int ga_policy_env_step_rescales(void) { return 1; }

static float* g_obs_a;  // labels for the two observation buffers
static float* g_action;
static float* g_scaled;
static const char* which(const void* p) { return p == g_obs_a ? "A" : "B"; }
static const char* rows(const void* p) {
  return p == g_action ? "action" : p == g_scaled ? "scaled" : "?";
}

extern "C" int ga_policy_step_fused_f32(const ga_mlp_desc*, const float*,
                                        const ga_head_args* a, ga_stream_t) {
  logf("policy col=%lld step=%u obs=%s", (long long)a->col, a->step, which(a->obs));
  return 0;
}

extern "C" int ga_action_rescale_f32(int64_t n, int A, const float* act, int64_t lda,
                                     const float*, const float*, float scale, float* out,
                                     int64_t ldo, ga_stream_t) {
  logf("rescale n=%lld A=%d %s->%s lda=%lld ldo=%lld scale=%g", (long long)n, A, rows(act),
       rows(out), (long long)lda, (long long)ldo, scale);
  return 0;
}

extern "C" int ga_policy_env_step_fused_f32(const ga_mlp_desc*, const float*,
                                            const ga_head_args* h, const ga_env_ref* env,
                                            const ga_record_args* r, const ga_norm_args* nm,
                                            int64_t n_steps, ga_stream_t) {
  logf("fused kind=%d col=%lld steps=%lld obs=%s next=%s bounds=%d scratch=%s scale=%g",
       env->kind, (long long)h->col, (long long)n_steps, which(h->obs), which(r->next_obs),
       nm && nm->act_low && nm->act_high, nm ? rows(nm->scaled_action) : "-",
       nm ? nm->expected_action_scale : 0.f);
  return 0;
}

extern "C" int ga_env_step_record(const ga_env_ref* env, const ga_record_args* r,
                                  const ga_norm_args*, const float* act, int64_t,
                                  const float* obs, ga_stream_t) {
  logf("env kind=%d col=%lld obs=%s next=%s act=%s", env->kind, (long long)r->col,
       which(obs), which(r->next_obs), rows(act));
  return 0;
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
  std::vector<float> a(64), b(64), lo(2, -1.f), hi(2, 1.f), action(32), scaled(32);
  g_obs_a = a.data();
  g_action = action.data();
  g_scaled = scaled.data();
  ga_mlp_desc desc;
  memset(&desc, 0, sizeof(desc));
  desc.n_layers = 3;
  float params[4] = {0};
  ga_head_args head;
  memset(&head, 0, sizeof(head));
  head.n = 8; head.Tcap = 16; head.col = 2; head.step = 40;
  head.action = action.data(); head.lda = 4;
  ga_record_args rec;
  memset(&rec, 0, sizeof(rec));
  ga_point_env point;
  memset(&point, 0, sizeof(point));
  point.n = 8;
  ga_grid_env grid;
  memset(&grid, 0, sizeof(grid));
  grid.n = 8;
  ga_env_ref pref = {GA_ENV_POINT, 0, &point};
  ga_env_ref gref = {GA_ENV_GRID, 0, &grid};
  ga_norm_args nm;
  memset(&nm, 0, sizeof(nm));
  nm.act_low = lo.data(); nm.act_high = hi.data(); nm.scaled_action = scaled.data();
  nm.expected_action_scale = 1.5f;

  // refusals: nothing launched; the rescale's comes before the buffer's
  auto steps = [&](const ga_env_ref* env, const ga_norm_args* norm, int64_t n) {
    return ga_rollout_env_steps(&desc, params, &head, env, &rec, a.data(), b.data(), norm,
                                nullptr, nullptr, n, nullptr);
  };
  CHECK(steps(&gref, &nm, 15) < 0);  // a class index, and past Tcap
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  ga_norm_args bad = nm;
  bad.act_high = nullptr;
  CHECK(steps(&pref, &bad, 2) < 0);
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  bad = nm;
  bad.scaled_action = nullptr;
  CHECK(steps(&pref, &bad, 2) < 0);
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  CHECK(steps(&pref, &nm, 15) < 0);
  CHECK(g_error.find("exceed") != std::string::npos);
  CHECK(g_log.empty());

  // the rescaled rollout in one fused launch, which gets bounds, scale and scratch
  CHECK(steps(&pref, &nm, 5) == 0);
  CHECK(g_log.size() == 1 &&
        g_log[0] == "fused kind=1 col=2 steps=5 obs=A next=B bounds=1 scratch=scaled "
                    "scale=1.5");

  // fusion off: three launches per step, the env steps on the scratch rows
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(steps(&pref, &nm, 2) == 0);
  const char* want[] = {"policy col=2 step=40 obs=A",
                        "rescale n=8 A=2 action->scaled lda=4 ldo=4 scale=1.5",
                        "env kind=1 col=2 obs=A next=B act=scaled",
                        "policy col=3 step=41 obs=B",
                        "rescale n=8 A=2 action->scaled lda=4 ldo=4 scale=1.5",
                        "env kind=1 col=3 obs=B next=A act=scaled"};
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want[i]);
  ga_set_fused_env_step(1);

  // teacher-forced noise is per step, rescaled or not
  g_log.clear();
  float noise[32] = {0};
  head.noise = noise; head.ldn = 4;
  CHECK(steps(&pref, &nm, 2) == 0);
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want[i]);
  head.noise = nullptr;

  // without bounds the env steps on the policy's own rows
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(steps(&pref, nullptr, 1) == 0);
  CHECK(g_log.size() == 2 && g_log[1] == "env kind=1 col=2 obs=A next=B act=action");
  ga_set_fused_env_step(1);

  if (g_fail) {
    fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("rollout_rescale_loop harness: all checks passed\n");
  return 0;
}
