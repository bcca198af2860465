// Host-logic harness for ga_rollout_env_steps (garage_amd/csrc/rollout_loop.cpp), built
// with -fsanitize=address,undefined on the CPU.  The kernel entry points the loop calls
// are fakes that record each call (fake_rollout_kernels.h), so the checks are about the
// loop itself.  Two suites, chosen on the command line (none: both):
//   env-loop      `make asan-env-loop`: against a kernel side whose fused policy + env
//                 step does NOT rescale the actions itself -- which launch a rollout takes
//                 for each env kind, the ping-pong of the observation buffers, the columns
//                 and Philox steps, the three launches per step of a rescaled rollout,
//                 and that argument errors are refused before anything is launched;
//   rescale-loop  `make asan-rescale-loop`: against one that, like policy_fused.hip,
//                 rescales inside the fused launch -- a rescaled rollout is ONE launch
//                 that is handed the bounds and the scratch, three launches per step under
//                 ga_set_fused_env_step(0) or teacher-forced noise, and the refusals keep
//                 their order.
// Each suite sets the product's switch and the fake side's at entry.
#include "fake_rollout_kernels.h"

// what both suites roll out
struct Rollout {
  std::vector<float> a, b, lo, hi, action, scaled;
  ga_mlp_desc desc;
  float params[4];
  ga_head_args head;
  ga_record_args rec;
  ga_point_env point;
  ga_grid_env grid;
  ga_env_ref pref, gref;
  ga_norm_args nm;
  explicit Rollout(int rescales_in_launch)
      : a(64), b(64), lo(2, -1.f), hi(2, 1.f), action(32), scaled(32) {
    ga_set_fused_env_step(1);
    g_rescales_in_launch = rescales_in_launch;
    g_addresses = false;
    g_policy_step_fused_ok = 1;
    g_obs_a = a.data();
    g_action = action.data();
    g_scaled = scaled.data();
    g_log.clear();
    g_error.clear();
    memset(&desc, 0, sizeof(desc));
    desc.n_layers = 3;
    memset(params, 0, sizeof(params));
    memset(&head, 0, sizeof(head));
    head.n = 8; head.Tcap = 16; head.col = 2; head.step = 40;
    head.action = action.data(); head.lda = 4;
    memset(&rec, 0, sizeof(rec));
    memset(&point, 0, sizeof(point));
    point.n = 8;
    memset(&grid, 0, sizeof(grid));
    grid.n = 8;
    pref = ga_env_ref{GA_ENV_POINT, 0, &point};
    gref = ga_env_ref{GA_ENV_GRID, 0, &grid};
    memset(&nm, 0, sizeof(nm));
    nm.act_low = lo.data(); nm.act_high = hi.data(); nm.scaled_action = scaled.data();
  }
  int steps(const ga_env_ref* env, const ga_norm_args* norm, int64_t n) {
    return ga_rollout_env_steps(&desc, params, &head, env, &rec, a.data(), b.data(), norm,
                                nullptr, nullptr, n, nullptr);
  }
};

static void suite_env_loop() {
  Rollout r(0);
  // argument errors: nothing launched
  CHECK(r.steps(nullptr, nullptr, 3) < 0);
  ga_env_ref bad = {9, 0, &r.point};
  CHECK(r.steps(&bad, nullptr, 3) < 0);
  CHECK(g_error.find("unknown env kind") != std::string::npos);
  CHECK(r.steps(&r.pref, nullptr, 15) < 0);
  CHECK(g_error.find("exceed") != std::string::npos);
  CHECK(r.steps(&r.gref, &r.nm, 3) < 0);
  CHECK(g_error.find("continuous") != std::string::npos);
  CHECK(g_log.empty());

  // the whole rollout in one fused launch
  CHECK(r.steps(&r.gref, nullptr, 5) == 0);
  CHECK(g_log.size() == 1 &&
        g_log[0] == "fused kind=2 col=2 steps=5 obs=A next=B bounds=0 scratch=- scale=0");

  // two launches per step: columns, Philox steps and buffers alternate
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(r.steps(&r.gref, nullptr, 3) == 0);
  const char* want[] = {
      "policy col=2 step=40 obs=A", "env kind=2 col=2 obs=A next=B act=action",
      "policy col=3 step=41 obs=B", "env kind=2 col=3 obs=B next=A act=action",
      "policy col=4 step=42 obs=A", "env kind=2 col=4 obs=A next=B act=action"};
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want[i]);

  // action rescale (PointEnv's Box): per-step launches even with fusion on, the env steps
  // on the scratch rows
  g_log.clear();
  ga_set_fused_env_step(1);
  CHECK(r.steps(&r.pref, &r.nm, 2) == 0);
  const char* want2[] = {"policy col=2 step=40 obs=A",
                         "rescale n=8 A=2 action->scaled lda=4 ldo=4 scale=0",
                         "env kind=1 col=2 obs=A next=B act=scaled",
                         "policy col=3 step=41 obs=B",
                         "rescale n=8 A=2 action->scaled lda=4 ldo=4 scale=0",
                         "env kind=1 col=3 obs=B next=A act=scaled"};
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want2[i]);

  // a NormalizedEnv that does not rescale (no bounds) still takes the one launch
  {
    g_log.clear();
    ga_norm_args plain = r.nm;
    plain.act_low = plain.act_high = nullptr;
    CHECK(r.steps(&r.pref, &plain, 2) == 0);
    CHECK(g_log.size() == 1 &&
          g_log[0] == "fused kind=1 col=2 steps=2 obs=A next=B bounds=0 scratch=scaled scale=0");
  }

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
    auto synth = [&](int64_t n) {
      return ga_rollout_env_steps(&r.desc, r.params, &h, &sref, &r.rec, A, B, nullptr,
                                  nullptr, nullptr, n, nullptr);
    };
    CHECK(synth(3) == 0);
    // (ONE launch for all the steps by default)
    CHECK(count("policy_env_step") == 1 && count("policy_step ") == 0);
    char line[160];
    snprintf(line, sizeof(line),
             "policy_env_step col=3 step=100 obs=%p next=%p norm=0 steps=3", (void*)A,
             (void*)B);
    CHECK(count(line) == 1);
    ga_set_fused_env_step(0);
    g_log.clear();
    CHECK(synth(3) == 0);
    CHECK(count("policy_step") == 3 && count("env_step col") == 3);
    snprintf(line, sizeof(line), "env_step col=4 obs=%p next=%p", (void*)B, (void*)A);
    CHECK(count(line) == 1);
    ga_set_fused_env_step(1);
    CHECK(synth(14) != 0);  // past Tcap
    g_addresses = false;
  }
}

static void suite_rescale_loop() {
  Rollout r(1);
  r.nm.expected_action_scale = 1.5f;

  // refusals: nothing launched; the rescale's comes before the buffer's
  CHECK(r.steps(&r.gref, &r.nm, 15) < 0);  // a class index, and past Tcap
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  ga_norm_args bad = r.nm;
  bad.act_high = nullptr;
  CHECK(r.steps(&r.pref, &bad, 2) < 0);
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  bad = r.nm;
  bad.scaled_action = nullptr;
  CHECK(r.steps(&r.pref, &bad, 2) < 0);
  CHECK(g_error.find("action rescale needs") != std::string::npos);
  CHECK(r.steps(&r.pref, &r.nm, 15) < 0);
  CHECK(g_error.find("exceed") != std::string::npos);
  CHECK(g_log.empty());

  // the rescaled rollout in one fused launch, which gets bounds, scale and scratch
  CHECK(r.steps(&r.pref, &r.nm, 5) == 0);
  CHECK(g_log.size() == 1 &&
        g_log[0] == "fused kind=1 col=2 steps=5 obs=A next=B bounds=1 scratch=scaled "
                    "scale=1.5");

  // fusion off: three launches per step, the env steps on the scratch rows
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(r.steps(&r.pref, &r.nm, 2) == 0);
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
  r.head.noise = noise; r.head.ldn = 4;
  CHECK(r.steps(&r.pref, &r.nm, 2) == 0);
  CHECK(g_log.size() == 6);
  for (size_t i = 0; i < g_log.size() && i < 6; ++i) CHECK(g_log[i] == want[i]);
  r.head.noise = nullptr;

  // without bounds the env steps on the policy's own rows
  g_log.clear();
  ga_set_fused_env_step(0);
  CHECK(r.steps(&r.pref, nullptr, 1) == 0);
  CHECK(g_log.size() == 2 && g_log[1] == "env kind=1 col=2 obs=A next=B act=action");
  CHECK(g_log.size() == 2 && g_log[0] == "policy col=2 step=40 obs=A");
  ga_set_fused_env_step(1);
}

int main(int argc, char** argv) {
  return run_suites(
      {{"env-loop", suite_env_loop, "rollout_env_loop harness: all checks passed"},
       {"rescale-loop", suite_rescale_loop, "rollout_rescale_loop harness: all checks passed"}},
      argc, argv);
}
