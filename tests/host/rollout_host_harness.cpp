// Host-logic harness for the rollout step's host side (garage_amd/csrc/rollout_host.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-rollout-host`).  The
// launch seam of rollout_params.h, the profiler's counter and the HIP calls the file makes
// are replaced by fakes.  Every seam fake records its grid (and the fused step its
// variant), compares the kernel-side structs field by field with the C-ABI structs the
// running case was called with, and touches the last element its kernel would reach in
// buffers of exactly the documented size, so that a stride, a column or a member offset
// that is off trips the sanitizer.  The checks are about the host's own work: which
// instantiation a fused step runs and which counters it bumps (against a literal table),
// the grid and the member split, every refusal of every entry point with its message and
// before any launch for every env kind, the conversions, the debug hook's buffer.
#define GA_HARNESS_REAL_STEP_PREDICATE  // this program links the real one
#include "../../garage_amd/csrc/rollout_params.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/prof.h"
#include "harness.h"

#include <functional>

using namespace ga_rollout;

static_assert(PS_ROWS == 16 && PS_HMAX == 256 && PS_WMAX == 512 && PS_MAX_OUT == 32 &&
                  PS_KC == 32 && PS_TRAIN_ROWS == 64,
              "the constants the cases below are written for");

// every env kind there is, by hand: a kind missing from GA_ENV_KINDS (internal.h) is
// refused as unknown and fails the cases below
static const int KINDS[] = {GA_ENV_SYNTH,    GA_ENV_POINT,    GA_ENV_GRID,
                            GA_ENV_MULTI_POINT, GA_ENV_CARTPOLE, GA_ENV_PENDULUM,
                            GA_ENV_DOUBLE_PENDULUM, GA_ENV_ACROBOT, GA_ENV_MOUNTAIN_CAR};
// state floats of the seeded state-vector kinds (include/garage_amd.h)
template <class K> struct StateFloats;
template <> struct StateFloats<CartPoleKind> { static constexpr int S = 4, OBS = 4; };
template <> struct StateFloats<PendulumKind> { static constexpr int S = 2, OBS = 3; };
template <> struct StateFloats<DoublePendulumKind> { static constexpr int S = 6, OBS = 11; };
template <> struct StateFloats<AcrobotKind> { static constexpr int S = 4, OBS = 6; };
template <> struct StateFloats<MountainCarKind> { static constexpr int S = 2, OBS = 2; };

// ---- "device" memory: exactly n elements, 16-byte aligned, zeroed, freed at exit ----------
static std::vector<void*> g_owned;
template <class T>
static T* dev(int64_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, (size_t)n * sizeof(T))) abort();
  memset(p, 0, (size_t)n * sizeof(T));
  g_owned.push_back(p);
  return static_cast<T*>(p);
}
static void free_all() {
  for (void* p : g_owned) free(p);
  g_owned.clear();
}
static int round4(int v) { return (v + 3) & ~3; }

// ---- a network: its descriptor and the floats of its parameter vector ----------------------
// (the LayerNorm blocks lie behind the weights: they are the end of the vector)
struct Net {
  ga_mlp_desc d;
  int64_t flat;
};
static Net make_net(const std::vector<int>& dims, int hact = 0, int oact = 0, int ln = 0) {
  Net n;
  memset(&n, 0, sizeof(n));
  n.d.n_layers = (int)dims.size() - 1;
  for (size_t i = 0; i < dims.size(); ++i) n.d.dims[i] = dims[i];
  int64_t off = 4;
  for (int l = 0; l < n.d.n_layers; ++l) {
    n.d.w_off[l] = off; off += (int64_t)dims[l + 1] * round4(dims[l]);
    n.d.b_off[l] = off; off += round4(dims[l + 1]);
  }
  int64_t act = 0;
  for (int l = 0; l + 1 < n.d.n_layers; ++l) { n.d.act_off[l] = act; act += 1000; }
  if (ln)
    for (int l = 0; l + 1 < n.d.n_layers; ++l) {
      n.d.ln_off[l] = off; off += 2 * round4(dims[l]);
    }
  n.d.hidden_act = hact; n.d.output_act = oact; n.d.layer_norm = ln;
  n.flat = off;
  return n;
}

// ---- one case: a batch of one env kind, a policy for it, the step's buffers -----------------
struct Opt {
  int kind = GA_ENV_SYNTH;
  int64_t n = 20, Tcap = 6, col = 1;
  std::vector<int> hidden = {8};
  int in_w = 5, A = 3;        // the synthetic env's widths (A: also a categorical head's classes)
  int synth_discrete = 0;
  int hact = 0, oact = 0, ln = 0;
  int64_t members = 1, stride_extra = 0;
  int continuous = 1, onehot = 1;
  int norm = 0;               // 1: reward only, 2: observations too
  int rescale = 0;
};
struct Case {
  Opt o;
  ga_synth_env synth; ga_point_env point; ga_grid_env grid; ga_multi_point_env multi;
  ga_cartpole_env cartpole; ga_pendulum_env pendulum; ga_double_pendulum_env dpend;
  ga_acrobot_env acrobot; ga_mountain_car_env mcar;
  ga_env_ref ref_;
  int obs_dim, act_w, discrete, A;
  int64_t ldo, lda, ldh, stride;
  Net net;
  float* params;
  ga_head_args h; ga_record_args r; ga_norm_args nm;
  float *obs, *next, *raw, *raw_next;
  bool skip_params = false;  // the parameter vectors are not there (the 2^31 edge)

  template <class E>
  void state_env(E* e, int S) {
    e->n = o.n; e->env_id0 = 7; e->max_episode_length = 9; e->seed = 0x1122334455667788ull;
    e->state = dev<float>(o.n * S); e->t = dev<int32_t>(o.n); e->resets = dev<uint32_t>(o.n);
  }
  explicit Case(const Opt& o_) : o(o_) {
    const int64_t n = o.n, T = o.Tcap;
    memset(&synth, 0, sizeof(synth)); memset(&point, 0, sizeof(point));
    memset(&grid, 0, sizeof(grid)); memset(&multi, 0, sizeof(multi));
    memset(&cartpole, 0, sizeof(cartpole)); memset(&pendulum, 0, sizeof(pendulum));
    memset(&dpend, 0, sizeof(dpend)); memset(&acrobot, 0, sizeof(acrobot));
    memset(&mcar, 0, sizeof(mcar));
    synth.n = n; synth.env_id0 = 3; synth.obs_dim = o.in_w; synth.act_dim = o.A;
    synth.discrete = o.synth_discrete; synth.min_len = 2; synth.max_len = 9;
    synth.seed = 0xa1b2c3d4e5f60718ull;
    synth.episode = dev<int32_t>(n); synth.t = dev<int32_t>(n); synth.len = dev<int32_t>(n);
    point.n = n; point.arena_size = 5.f; point.done_bonus = 1.f; point.max_episode_length = 9;
    point.point = dev<float>(2 * n); point.goal = dev<float>(2 * n);
    point.t = dev<int32_t>(n); point.success = dev<uint8_t>(n * T);
    grid.n = n; grid.rows = 3; grid.cols = 4; grid.max_episode_length = 9;
    grid.map = dev<uint8_t>(n * 12); grid.start = dev<int32_t>(n);
    grid.state = dev<int32_t>(n); grid.t = dev<int32_t>(n);
    multi.n = n; multi.arena_size = 5.f; multi.done_bonus = 1.f; multi.max_episode_length = 9;
    multi.point = dev<float>(2 * n); multi.goal = dev<float>(2 * n);
    multi.t = dev<int32_t>(n); multi.success = dev<uint8_t>(n * T);
    multi.num_tasks = 3; multi.strategy = GA_TASK_UNIFORM_RANDOM;
    multi.mode = o.onehot ? GA_TASK_ADD_ONEHOT : GA_TASK_VANILLA;
    multi.seed = 0x0102030405060708ull; multi.task_goals = dev<float>(2 * 3);
    multi.last_task = dev<int32_t>(n); multi.resets = dev<uint32_t>(n);
    multi.task_id = dev<uint8_t>(n * T);
    state_env(&cartpole, 4); state_env(&pendulum, 2); state_env(&dpend, 6);
    state_env(&acrobot, 4); state_env(&mcar, 2);
    mcar.continuous = o.continuous;
    // the kind's own facts, through the product's dispatch
    obs_dim = act_w = discrete = -1;
    ga_visit_env(ref(), "harness", [&](auto* e) {
      obs_dim = ga_env_obs_dim(e); act_w = ga_env_act_width(e); discrete = ga_env_discrete(e);
      return 0;
    });
    CHECK(obs_dim > 0);
    if (obs_dim <= 0) obs_dim = act_w = 1;
    A = discrete ? o.A : act_w;
    ldo = round4(obs_dim) + 4; lda = round4(act_w) + 4; ldh = round4(A);
    std::vector<int> dims = {obs_dim};
    for (int hdn : o.hidden) dims.push_back(hdn);
    dims.push_back(A);
    net = make_net(dims, o.hact, o.oact, o.ln);
    stride = o.members > 1 ? net.flat + o.stride_extra : 0;
    params = dev<float>((o.members - 1) * (net.flat + o.stride_extra) + net.flat);
    const int64_t rows = (n - 1) * T + T;  // cells of an [n, Tcap] buffer
    obs = dev<float>((n - 1) * ldo + obs_dim); next = dev<float>((n - 1) * ldo + obs_dim);
    raw = dev<float>((n - 1) * ldo + obs_dim); raw_next = dev<float>((n - 1) * ldo + obs_dim);
    memset(&h, 0, sizeof(h)); memset(&r, 0, sizeof(r)); memset(&nm, 0, sizeof(nm));
    h.n = n; h.env_id0 = 3; h.A = A; h.kind = discrete ? 1 : 0;
    h.head = dev<float>((n - 1) * ldh + A); h.ldh = ldh; h.log_std = dev<float>(1);
    h.has_min = 1; h.has_max = 1; h.min_log_std = -3.f; h.max_log_std = 2.f;
    h.seed = 0x5566778899aabbccull; h.step = 41; h.double_softmax = 1;
    h.obs = obs; h.ldo = ldo; h.obs_dim = obs_dim; h.col = o.col; h.Tcap = T;
    h.action = dev<float>((n - 1) * lda + act_w); h.lda = lda;
    h.obs_buf = dev<float>((rows - 1) * ldo + obs_dim);
    h.act_buf = dev<float>((rows - 1) * lda + act_w);
    h.head_buf = dev<float>((rows - 1) * ldh + A);
    r.n = n; r.col = o.col; r.Tcap = T; r.max_episode_length = 9;
    r.reward = dev<float>(n); r.step_type = dev<uint8_t>(n); r.next_obs = next;
    r.ldo = ldo; r.obs_dim = obs_dim; r.ep_t = dev<int32_t>(n); r.rew_buf = dev<float>(rows);
    r.st_buf = dev<uint8_t>(rows); r.tail_buf = dev<uint16_t>(rows);
    r.lastobs_buf = dev<float>((rows - 1) * ldo + obs_dim); r.done = dev<uint8_t>(n);
    r.step_eps = dev<int32_t>(T); r.step_samples = dev<int32_t>(T); r.terminal_only = 1;
    nm.normalize_reward = o.norm >= 1; nm.normalize_obs = o.norm >= 2;
    nm.obs_mean = dev<double>(n * obs_dim); nm.obs_var = dev<double>(n * obs_dim);
    nm.obs_alpha = 0.25; nm.reward_mean = dev<double>(n); nm.reward_var = dev<double>(n);
    nm.reward_alpha = 0.125; nm.reward_scale = 2.0;
    nm.raw_obs = raw; nm.raw_next_obs = raw_next;
    if (o.rescale) {
      nm.act_low = dev<float>(act_w); nm.act_high = dev<float>(act_w);
      nm.expected_action_scale = 1.5f;
      nm.scaled_action = dev<float>((n - 1) * lda + act_w);
    }
  }
  const ga_env_ref* ref() {
    ref_.kind = o.kind; ref_.pad_ = 0;
    switch (o.kind) {
      case GA_ENV_SYNTH: ref_.env = &synth; break;
      case GA_ENV_POINT: ref_.env = &point; break;
      case GA_ENV_GRID: ref_.env = &grid; break;
      case GA_ENV_MULTI_POINT: ref_.env = &multi; break;
      case GA_ENV_CARTPOLE: ref_.env = &cartpole; break;
      case GA_ENV_PENDULUM: ref_.env = &pendulum; break;
      case GA_ENV_DOUBLE_PENDULUM: ref_.env = &dpend; break;
      case GA_ENV_ACROBOT: ref_.env = &acrobot; break;
      default: ref_.env = &mcar; break;
    }
    return &ref_;
  }
  const ga_norm_args* norm() { return (o.norm || o.rescale) ? &nm : nullptr; }
};
static Case* g_case = nullptr;  // what the entry point under test was called with

// ---- what the fakes record ----------------------------------------------------------------
struct Launch {
  std::string what;
  unsigned blocks;
  hipStream_t stream;
  PsVariant v;
  int env_step, n_steps, wg_per_member, member_stride;
  const void* dbg;
};
static std::vector<Launch> g_launches;
static std::vector<int> g_prof_counts;
static std::vector<size_t> g_sync_copies;
static int g_syncs = 0, g_memsets = 0, g_syncs_at_copy = -1;
static volatile float g_sink;
static hipStream_t const S1 = (hipStream_t)0x100;

static void record(const char* what, unsigned blocks, hipStream_t s) {
  g_launches.push_back(Launch{what, blocks, s, PsVariant{0, 0, 0}, 0, 0, 0, 0, nullptr});
  CHECK(s == S1);
}
template <class T> static void rd(const T* p, int64_t i) {
  const volatile T* q = p;
  g_sink = (float)q[0] + (float)q[i];
}
// (through a volatile pointer: a plain self-assignment is removed before the sanitizer
// instruments it)
template <class T> static void wr(T* p, int64_t i) {
  volatile T* q = p;
  q[0] = q[0]; q[i] = q[i];
}
static void reset() { g_launches.clear(); g_prof_counts.clear(); g_error.clear(); }

// ---- the kernel-side env against the C-ABI one; what a kernel reaches of its state ----------
static void key_is(uint64_t seed, uint32_t k0, uint32_t k1) {
  CHECK(k0 == (uint32_t)seed && k1 == (uint32_t)(seed >> 32));
}
static int env_obs_dim(const SynthEnv& e) { return e.obs_dim; }
static int env_obs_dim(const PointEnv&) { return 3; }
static int env_obs_dim(const GridEnv& e) { return e.rows * e.cols; }
static int env_obs_dim(const MultiTaskEnv<PointEnv>& e) { return 3 + (e.one_hot ? e.num_tasks : 0); }
template <class K> static int env_obs_dim(const StateEnv<K>&) { return StateFloats<K>::OBS; }

static void env_is(const SynthEnv& d, const Case& c, int64_t, int64_t) {
  const ga_synth_env& e = c.synth;
  CHECK(d.n == e.n && d.env_id0 == e.env_id0 && d.obs_dim == e.obs_dim &&
        d.act_dim == e.act_dim && d.discrete == e.discrete && d.min_len == e.min_len &&
        d.max_len == e.max_len && d.episode == e.episode && d.t == e.t && d.len == e.len);
  key_is(e.seed, d.k0, d.k1);
  wr(d.episode, d.n - 1); wr(d.t, d.n - 1); wr(d.len, d.n - 1);
}
static void point_is(const PointEnv& d, int64_t n, float arena, float bonus, int never_done,
                     int mel, float* point, const float* goal, int32_t* t, uint8_t* success,
                     int64_t info_ld, int64_t col) {
  CHECK(d.n == n && d.arena == arena && d.bonus == bonus && d.never_done == never_done &&
        d.max_len == mel && d.point == point && d.goal == goal && d.t == t &&
        d.success == success && d.succ_ld == info_ld);
  wr(d.point, 2 * n - 1); rd(d.goal, 2 * n - 1); wr(d.t, n - 1);
  if (d.success) wr(d.success, (n - 1) * d.succ_ld + col);
}
static void env_is(const PointEnv& d, const Case& c, int64_t info_ld, int64_t col) {
  const ga_point_env& e = c.point;
  point_is(d, e.n, e.arena_size, e.done_bonus, e.never_done, e.max_episode_length, e.point,
           e.goal, e.t, e.success, info_ld, col);
}
static void env_is(const GridEnv& d, const Case& c, int64_t, int64_t) {
  const ga_grid_env& e = c.grid;
  CHECK(d.n == e.n && d.rows == e.rows && d.cols == e.cols &&
        d.max_len == e.max_episode_length && d.map == e.map && d.start == e.start &&
        d.state == e.state && d.t == e.t);
  rd(d.map, d.n * d.rows * d.cols - 1); rd(d.start, d.n - 1); wr(d.state, d.n - 1);
  wr(d.t, d.n - 1);
}
static void env_is(const MultiTaskEnv<PointEnv>& d, const Case& c, int64_t info_ld,
                   int64_t col) {
  const ga_multi_point_env& e = c.multi;
  point_is(d.in, e.n, e.arena_size, e.done_bonus, e.never_done, e.max_episode_length, e.point,
           e.goal, e.t, e.success, info_ld, col);
  CHECK(d.n == e.n && d.num_tasks == e.num_tasks && d.strategy == e.strategy &&
        d.one_hot == (e.mode == GA_TASK_ADD_ONEHOT) && d.payload == e.task_goals &&
        d.last_task == e.last_task && d.resets == e.resets && d.task_id == e.task_id &&
        d.info_ld == info_ld);
  key_is(e.seed, d.k0, d.k1);
  rd(d.payload, 2 * d.num_tasks - 1); wr(d.last_task, d.n - 1); wr(d.resets, d.n - 1);
  if (d.task_id) wr(d.task_id, (d.n - 1) * d.info_ld + col);
}
template <class K, class E>
static void state_is(const StateEnv<K>& d, const E& e, int variant) {
  CHECK(d.n == e.n && d.env_id0 == e.env_id0 && d.max_len == e.max_episode_length &&
        d.variant == variant && d.state == e.state && d.t == e.t && d.resets == e.resets);
  key_is(e.seed, d.k0, d.k1);
  wr(d.state, d.n * StateFloats<K>::S - 1); wr(d.t, d.n - 1); wr(d.resets, d.n - 1);
}
static void env_is(const StateEnv<CartPoleKind>& d, const Case& c, int64_t, int64_t) {
  state_is(d, c.cartpole, 0);
}
static void env_is(const StateEnv<PendulumKind>& d, const Case& c, int64_t, int64_t) {
  state_is(d, c.pendulum, 0);
}
static void env_is(const StateEnv<DoublePendulumKind>& d, const Case& c, int64_t, int64_t) {
  state_is(d, c.dpend, 0);
}
static void env_is(const StateEnv<AcrobotKind>& d, const Case& c, int64_t, int64_t) {
  state_is(d, c.acrobot, 0);
}
static void env_is(const StateEnv<MountainCarKind>& d, const Case& c, int64_t, int64_t) {
  state_is(d, c.mcar, c.mcar.continuous);
}

// the record of a step, its buffers reached at column `col` by the last env
static void record_is(const RecordParams& p, const ga_record_args& a, int64_t col) {
  CHECK(p.n == a.n && p.col == a.col && p.Tcap == a.Tcap &&
        p.max_episode_length == a.max_episode_length && p.reward == a.reward &&
        p.step_type == a.step_type && p.next_obs == a.next_obs && p.ldo == a.ldo &&
        p.obs_dim == a.obs_dim && p.ep_t == a.ep_t && p.rew_buf == a.rew_buf &&
        p.st_buf == a.st_buf && p.tail_buf == a.tail_buf && p.lastobs_buf == a.lastobs_buf &&
        p.done == a.done && p.step_eps == a.step_eps && p.step_samples == a.step_samples &&
        p.terminal_only == a.terminal_only);
  const int64_t last = p.n - 1, cell = last * p.Tcap + col;
  rd(p.reward, last); rd(p.step_type, last); wr(p.ep_t, last); wr(p.rew_buf, cell);
  wr(p.st_buf, cell); wr(p.tail_buf, cell); wr(p.done, last); wr(p.step_eps, col);
  wr(p.step_samples, col);
  if (p.obs_dim > 0) {
    rd(p.next_obs, last * p.ldo + p.obs_dim - 1);
    wr(p.lastobs_buf, cell * p.ldo + p.obs_dim - 1);
  }
}

static void head_is(const HeadDev& d, const ga_head_args& a) {
  CHECK(d.n == a.n && d.env_id0 == a.env_id0 && d.kind == a.kind && d.has_min == a.has_min &&
        d.has_max == a.has_max && d.min_log_std == a.min_log_std &&
        d.max_log_std == a.max_log_std && d.noise == a.noise && d.ldn == a.ldn &&
        d.step == a.step && d.double_softmax == a.double_softmax && d.obs == a.obs &&
        d.ldo == a.ldo && d.col == a.col && d.Tcap == a.Tcap && d.action == a.action &&
        d.lda == a.lda && d.obs_buf == a.obs_buf && d.act_buf == a.act_buf &&
        d.head_buf == a.head_buf && d.ldh == a.ldh);
  key_is(a.seed, d.k0, d.k1);
}
// what the head of a step reaches at column `col`: in_w observation columns, the action
// row (A columns, or the class index) and the agent_info row
static void head_touch(const HeadDev& d, int in_w, int A, int64_t col) {
  const int64_t last = d.n - 1, cell = last * d.Tcap + col;
  const int aw = d.kind ? 1 : A;
  rd(d.obs, last * d.ldo + in_w - 1); wr(d.obs_buf, cell * d.ldo + in_w - 1);
  wr(d.action, last * d.lda + aw - 1); wr(d.act_buf, cell * d.lda + aw - 1);
  if (d.head_buf) wr(d.head_buf, cell * d.ldh + A - 1);
}

// the whole of an env step's arguments: `fused`: built for the one-launch step (the
// rescale inside it); the column the last sub-step of the launch reaches
template <class Env>
static void step_is(const EnvStepArgsT<Env>& a, bool fused, int64_t last_col) {
  Case& c = *g_case;
  env_is(a.e, c, c.o.Tcap, last_col);  // env_infos go into the [n, Tcap] buffers
  CHECK(env_obs_dim(a.e) == c.obs_dim);
  record_is(a.p, c.r, last_col);
  const ga_norm_args* nm = c.norm();
  const bool nobs = nm && nm->normalize_obs, nrew = nm && nm->normalize_reward;
  CHECK(a.nm.norm_obs == nobs && a.nm.norm_reward == nrew);
  CHECK(a.nm.scale_reward == (nm != nullptr));  // (reward_scale 2)
  if (nm)
    CHECK(a.nm.obs_mean == nm->obs_mean && a.nm.obs_var == nm->obs_var &&
          a.nm.obs_alpha == nm->obs_alpha && a.nm.rew_mean == nm->reward_mean &&
          a.nm.rew_var == nm->reward_var && a.nm.rew_alpha == nm->reward_alpha &&
          a.nm.rew_scale == nm->reward_scale);
  else
    CHECK(!a.nm.obs_mean && !a.nm.obs_var && !a.nm.rew_mean && !a.nm.rew_var);
  // the env's own rows: the raw pair under observation normalisation only
  CHECK(a.raw_obs == (nobs ? c.raw : c.obs));
  CHECK(a.raw_next == (nobs ? c.raw_next : c.next));
  CHECK(a.seen_next == c.next);
  CHECK(a.actions == c.h.action && a.lda == c.lda && a.reward == c.r.reward &&
        a.step_type == c.r.step_type);
  const bool rescaled = fused && nm && nm->act_low;
  if (rescaled)
    CHECK(a.nm.act_low == nm->act_low && a.nm.act_high == nm->act_high &&
          a.nm.expected_action_scale == nm->expected_action_scale &&
          a.nm.scaled_action == nm->scaled_action && a.nm.scaled_ld == c.lda);
  else
    CHECK(!a.nm.act_low && !a.nm.act_high && !a.nm.scaled_action && a.nm.scaled_ld == 0 &&
          a.nm.expected_action_scale == 0.f);
  const int64_t last = a.e.n - 1;
  rd(a.actions, last * a.lda + c.act_w - 1);
  rd(a.raw_obs, last * a.p.ldo + c.obs_dim - 1); wr(a.raw_next, last * a.p.ldo + c.obs_dim - 1);
  wr(a.seen_next, last * a.p.ldo + c.obs_dim - 1); wr(a.reward, last); wr(a.step_type, last);
  if (a.nm.norm_obs) {
    wr(a.nm.obs_mean, a.e.n * c.obs_dim - 1); wr(a.nm.obs_var, a.e.n * c.obs_dim - 1);
  }
  if (a.nm.norm_reward) { wr(a.nm.rew_mean, last); wr(a.nm.rew_var, last); }
  if (rescaled) {
    rd(a.nm.act_low, c.act_w - 1); rd(a.nm.act_high, c.act_w - 1);
    wr(a.nm.scaled_action, last * a.nm.scaled_ld + c.act_w - 1);
  }
}

// ---- the seam's fakes ---------------------------------------------------------------------
void ro_launch_head_sample(const HeadParams& p, unsigned blocks, hipStream_t s) {
  record("head", blocks, s);
  Case& c = *g_case;
  CHECK(blocks == (unsigned)((p.hd.n + 255) / 256));
  head_is(p.hd, c.h);
  CHECK(p.A == c.h.A && p.head == c.h.head && p.log_std == c.h.log_std &&
        p.obs_dim == c.h.obs_dim);
  rd(p.head, (p.hd.n - 1) * p.hd.ldh + p.A - 1);
  if (p.hd.kind == 0) rd(p.log_std, 0);
  head_touch(p.hd, p.obs_dim, p.A, p.hd.col);
}
void ro_launch_record(const RecordParams& p, unsigned blocks, hipStream_t s) {
  record("record", blocks, s);
  CHECK(blocks == (unsigned)((p.n + 255) / 256));
  record_is(p, g_case->r, p.col);
}
template <class Env>
void ro_launch_env_reset(const Env& e, const uint8_t* mask, float* obs, int64_t ldo,
                         unsigned blocks, hipStream_t s) {
  record("env_reset", blocks, s);
  CHECK(blocks == (unsigned)((e.n + 255) / 256));
  env_is(e, *g_case, 1, 0);  // env_infos of a bare reset / step: [n]
  CHECK(obs == g_case->obs && ldo == g_case->ldo && mask == g_case->r.done);
  rd(mask, e.n - 1);
  wr(obs, (e.n - 1) * ldo + env_obs_dim(e) - 1);
}
template <class Env>
void ro_launch_env_step(const Env& e, const float* actions, int64_t lda, const float* obs,
                        float* next_obs, int64_t ldo, float* reward, uint8_t* step_type,
                        unsigned blocks, hipStream_t s) {
  record("env_step", blocks, s);
  Case& c = *g_case;
  CHECK(blocks == (unsigned)((e.n + 255) / 256));
  env_is(e, c, 1, 0);
  CHECK(actions == c.h.action && lda == c.lda && obs == c.obs && next_obs == c.next &&
        ldo == c.ldo && reward == c.r.reward && step_type == c.r.step_type);
  rd(actions, (e.n - 1) * lda + c.act_w - 1); rd(obs, (e.n - 1) * ldo + c.obs_dim - 1);
  wr(next_obs, (e.n - 1) * ldo + c.obs_dim - 1); wr(reward, e.n - 1); wr(step_type, e.n - 1);
}
template <class Env>
void ro_launch_env_step_record(const EnvStepArgsT<Env>& a, unsigned blocks, hipStream_t s) {
  record("env_step_record", blocks, s);
  CHECK(blocks == (unsigned)((a.e.n + 255) / 256));
  step_is(a, false, a.p.col);
}
template <class Env>
void ps_launch_policy_step(const FusedParams<Env>& p, PsVariant v, unsigned blocks,
                           hipStream_t s) {
  record("policy_step", blocks, s);
  Launch& l = g_launches.back();
  l.v = v; l.env_step = p.env_step; l.n_steps = p.n_steps;
  l.wg_per_member = p.wg_per_member; l.member_stride = p.member_stride; l.dbg = p.dbg;
  Case& c = *g_case;
  const ga_mlp_desc& d = c.net.d;
  CHECK(p.net.n_layers == d.n_layers && p.hidden_act == d.hidden_act &&
        p.output_act == d.output_act && p.layer_norm == (d.layer_norm != 0));
  for (int i = 0; i < 9; ++i) CHECK(p.net.dims[i] == d.dims[i]);
  for (int i = 0; i < 8; ++i)
    CHECK(p.net.w_off[i] == d.w_off[i] && p.net.b_off[i] == d.b_off[i] &&
          p.ln_off[i] == d.ln_off[i]);
  CHECK(p.params == c.params);
  head_is(p.hd, c.h);
  // workgroup b reads the vector of member b / wg_per_member
  CHECK(p.wg_per_member >= 1 && p.member_stride >= 0);
  if (!c.skip_params && p.wg_per_member >= 1)
    for (unsigned b = 0; b < blocks; ++b)
      rd(p.params + (int64_t)(b / (unsigned)p.wg_per_member) * p.member_stride, c.net.flat - 1);
  // ... and takes the envs [16 b, 16 b + 16) through n_steps columns
  CHECK((int64_t)blocks * PS_ROWS >= p.hd.n && (int64_t)(blocks - 1) * PS_ROWS < p.hd.n);
  const int L = d.n_layers;
  head_touch(p.hd, d.dims[0], d.dims[L], p.hd.col);
  head_touch(p.hd, d.dims[0], d.dims[L], p.hd.col + p.n_steps - 1);
  if (p.env_step) {
    CHECK(((p.env_step & ENV_STEP_RESCALE) != 0) == (p.es.nm.act_low != nullptr));
    CHECK((p.env_step & 1) == 1);
    step_is(p.es, true, p.hd.col + p.n_steps - 1);
  } else {
    const char* z = reinterpret_cast<const char*>(&p.es);
    bool zero = true;
    for (size_t i = 0; i < sizeof(p.es); ++i) zero = zero && z[i] == 0;
    CHECK(zero);
  }
}
void ps_launch_train_forward(const TrainFwdParams& p, unsigned blocks, hipStream_t s) {
  record("train_forward", blocks, s);
  Case& c = *g_case;
  const ga_mlp_desc& d = c.net.d;
  CHECK(blocks == (unsigned)((p.M + 63) / 64));
  CHECK(p.net.n_layers == d.n_layers && p.params == c.params && p.M == c.o.n);
  for (int i = 0; i < 8; ++i)
    CHECK(p.net.w_off[i] == d.w_off[i] && p.net.b_off[i] == d.b_off[i] &&
          p.act_off[i] == d.act_off[i] && p.net.dims[i] == d.dims[i]);
  rd(p.params, c.net.flat - 1);
  rd(p.X, (p.M - 1) * p.ldx + d.dims[0] - 1);
  wr(p.out, (p.M - 1) * p.ldo + d.dims[d.n_layers] - 1);
}
#define GA_SEAM_OF(GaEnv, ...)                                                             \
  template void ro_launch_env_reset(const ga_env_dev_t<GaEnv>&, const uint8_t*, float*,    \
                                    int64_t, unsigned, hipStream_t);                       \
  template void ro_launch_env_step(const ga_env_dev_t<GaEnv>&, const float*, int64_t,      \
                                   const float*, float*, int64_t, float*, uint8_t*,        \
                                   unsigned, hipStream_t);                                 \
  template void ro_launch_env_step_record(const ga_env_step_args_t<GaEnv>&, unsigned,      \
                                          hipStream_t);                                    \
  template void ps_launch_policy_step(const FusedParams<ga_env_dev_t<GaEnv>>&, PsVariant,  \
                                      unsigned, hipStream_t);
GA_ENV_KINDS(GA_SEAM_OF)
#undef GA_SEAM_OF

void ga_prof_count(int kind) { g_prof_counts.push_back(kind); }

extern "C" {
hipError_t hipMemset(void* p, int v, size_t bytes) {
  ++g_memsets;
  memset(p, v, bytes);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  g_sync_copies.push_back(bytes);
  g_syncs_at_copy = g_syncs;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { ++g_syncs; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "fake"; }
}

// ---- the entry points on a case -------------------------------------------------------------
static int run_fused(Case& c, int64_t n_steps) {
  g_case = &c;
  return ga_policy_env_step_fused_f32(&c.net.d, c.params, &c.h, c.ref(), &c.r, c.norm(),
                                      n_steps, (ga_stream_t)S1);
}
static int run_members(Case& c, int64_t n_steps) {
  g_case = &c;
  return ga_policy_env_step_members_f32(&c.net.d, c.params, &c.h, c.ref(), &c.r, c.norm(),
                                        n_steps, c.o.members,
                                        c.o.members > 1 ? c.stride : c.net.flat + c.o.stride_extra,
                                        (ga_stream_t)S1);
}
static int run_policy_only(Case& c) {
  g_case = &c;
  return ga_policy_step_fused_f32(&c.net.d, c.params, &c.h, (ga_stream_t)S1);
}
static int run_step_record(Case& c) {
  g_case = &c;
  return ga_env_step_record(c.ref(), &c.r, c.norm(), c.h.action, c.lda, c.obs,
                            (ga_stream_t)S1);
}
static int run_env_step(Case& c) {
  g_case = &c;
  return ga_env_step(c.ref(), c.h.action, c.lda, c.obs, c.next, c.ldo, (float*)c.r.reward,
                     (uint8_t*)c.r.step_type, (ga_stream_t)S1);
}
static int run_env_reset(Case& c) {
  g_case = &c;
  return ga_env_reset(c.ref(), c.r.done, c.obs, c.ldo, (ga_stream_t)S1);
}
static int run_head(Case& c) {
  g_case = &c;
  return ga_policy_head_sample(&c.h, (ga_stream_t)S1);
}
static int run_record(Case& c) {
  g_case = &c;
  return ga_record_step(&c.r, (ga_stream_t)S1);
}

// `rc` is a refusal with this message, and nothing was launched or counted
static void refused(const std::string& what, int rc, const std::string& message) {
  const bool ok = rc == -1 && g_error == message && g_launches.empty() && g_prof_counts.empty();
  if (!ok)
    fprintf(stderr, "not refused as expected: %s (rc %d, '%s', want '%s', %zu launches)\n",
            what.c_str(), rc, g_error.c_str(), message.c_str(), g_launches.size());
  CHECK(ok);
  reset();
}
static void accepted(const std::string& what, int rc, const char* launch, size_t n = 1) {
  const bool ok = rc == 0 && g_launches.size() == n && g_launches.back().what == launch;
  if (!ok)
    fprintf(stderr, "not accepted: %s (rc %d, '%s', %zu launches)\n", what.c_str(), rc,
            g_error.c_str(), g_launches.size());
  CHECK(ok);
}

// ---- which instantiation a fused step runs, its grid, member split and counters -------------
// One row per (network, options, n_steps, members; 0 = ga_policy_env_step_fused_f32, the
// synthetic env with `in` observation columns and a head of `out`), switches
// (GARAGE_AMD_ROLLOUT_WIDE, _RESIDENT) and what the launch must be: width (0: refused),
// resident, general, and the counters in order (R = GA_PROF_ROLLOUT, W = _WIDE).
struct VariantRow {
  int in; std::vector<int> hidden; int out, hact, oact, ln;
  int64_t n_steps, members;
  int wide_on, res_on;
  int width, resident, general;
  const char* counts;
};
static const VariantRow VARIANTS[] = {
    // tanh, 2 and 3 layers, one step and a whole rollout
    {5, {8}, 3, 0, 0, 0, 1, 0, 1, 1, 256, 0, 0, ""},
    {5, {8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 1, 0, "R"},
    {5, {8, 8}, 3, 0, 0, 0, 1, 0, 1, 1, 256, 0, 0, ""},
    {5, {8, 8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 1, 0, "R"},
    {5, {256, 256}, 32, 0, 0, 0, 4, 0, 1, 1, 256, 1, 0, "R"},
    // 1 and 4 layers stream their weights
    {5, {}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 0, 0, ""},
    {5, {8, 8, 8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 0, 0, ""},
    // observations of one k chunk, and one more
    {32, {8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 1, 0, "R"},
    {33, {8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 0, 0, ""},
    // a 256 and a 257 input: the observations, a hidden layer
    {256, {8, 8}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 0, 0, ""},
    {257, {8, 8}, 3, 0, 0, 0, 4, 0, 1, 1, 512, 0, 0, "W"},
    {5, {256}, 3, 0, 0, 0, 4, 0, 1, 1, 256, 1, 0, "R"},
    {5, {257}, 3, 0, 0, 0, 4, 0, 1, 1, 512, 0, 0, "W"},
    {5, {257}, 3, 0, 0, 0, 1, 0, 1, 1, 512, 0, 0, ""},
    // the 512 / 32 limits
    {512, {512, 512}, 32, 0, 0, 0, 4, 0, 1, 1, 512, 0, 0, "W"},
    {513, {8}, 3, 0, 0, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    {5, {513}, 3, 0, 0, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    {5, {8}, 33, 0, 0, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    {5, {300}, 33, 0, 0, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    // each non-default option
    {5, {8, 8}, 3, 2, 0, 0, 4, 0, 1, 1, 256, 1, 1, "R"},
    {5, {8, 8}, 3, 0, 1, 0, 4, 0, 1, 1, 256, 1, 1, "R"},
    {5, {8, 8}, 3, 0, 0, 1, 4, 0, 1, 1, 256, 1, 1, "R"},
    {5, {8, 8}, 3, 6, 6, 1, 1, 0, 1, 1, 256, 0, 1, ""},
    {5, {300, 8}, 3, 0, 0, 1, 4, 0, 1, 1, 512, 0, 1, "W"},
    {5, {8}, 3, 7, 0, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    {5, {8}, 3, 0, -1, 0, 4, 0, 1, 1, 0, 0, 0, ""},
    // the switches off: no wide kernels (refused), no resident weights
    {5, {257}, 3, 0, 0, 0, 4, 0, 0, 1, 0, 0, 0, ""},
    {5, {8, 8}, 3, 0, 0, 0, 4, 0, 0, 1, 256, 1, 0, "R"},
    {5, {8, 8}, 3, 0, 0, 0, 4, 0, 1, 0, 256, 0, 0, ""},
    {5, {8, 8}, 3, 0, 0, 0, 4, 0, 0, 0, 256, 0, 0, ""},
    {5, {257}, 3, 0, 0, 0, 4, 0, 1, 0, 512, 0, 0, "W"},
    // the population entry: every whole rollout counts once, whatever the kernel
    {5, {8, 8}, 3, 0, 0, 0, 4, 1, 1, 1, 256, 1, 0, "R"},
    {5, {8, 8}, 3, 0, 0, 0, 4, 1, 1, 0, 256, 0, 0, "R"},
    {5, {8, 8}, 3, 0, 0, 0, 1, 1, 1, 1, 256, 0, 0, ""},
    {5, {8, 8, 8}, 3, 0, 0, 0, 4, 3, 1, 1, 256, 0, 0, "R"},
    {5, {8, 8}, 3, 0, 0, 0, 4, 3, 1, 1, 256, 1, 0, "R"},
    {5, {257}, 3, 0, 0, 0, 4, 3, 1, 1, 512, 0, 0, "RW"},
    {5, {257}, 3, 0, 0, 1, 4, 1, 1, 1, 512, 0, 1, "RW"},
    {5, {257}, 3, 0, 0, 0, 1, 3, 1, 1, 512, 0, 0, ""},
};

static void check_variant(const VariantRow& row) {
  reset();
  ga_rollout_set_switches(row.wide_on, row.res_on);
  Opt o;
  o.in_w = row.in; o.hidden = row.hidden; o.A = row.out; o.hact = row.hact; o.oact = row.oact;
  o.ln = row.ln; o.Tcap = 6; o.col = 1;
  o.members = row.members ? row.members : 1;
  // 3 members of 16 envs; one policy: a ragged last workgroup
  o.n = row.members > 1 ? 16 * row.members : 37;
  Case c(o);
  const int rc = row.members ? run_members(c, row.n_steps) : run_fused(c, row.n_steps);
  bool ok;
  if (!row.width) {
    ok = rc == -1 && g_launches.empty() && g_prof_counts.empty() &&
         g_error == (row.members
                         ? "ga_policy_env_step_members_f32: network not supported by the fused step"
                         : "ga_policy_step_fused_f32: unsupported network shape");
  } else {
    ok = rc == 0 && g_launches.size() == 1;
    if (ok) {
      const Launch& l = g_launches[0];
      std::string counts;
      for (int k : g_prof_counts)
        counts += k == GA_PROF_ROLLOUT ? "R" : (k == GA_PROF_ROLLOUT_WIDE ? "W" : "?");
      ok = l.what == "policy_step" && l.v.width == row.width && l.v.resident == row.resident &&
           l.v.general == row.general && counts == row.counts &&
           l.blocks == (unsigned)((o.n + 15) / 16) && l.n_steps == row.n_steps &&
           l.env_step == 1 &&
           l.wg_per_member == 1 &&
           l.member_stride == (row.members > 1 ? (int)c.net.flat : 0);
    }
  }
  if (!ok)
    fprintf(stderr, "variant: in=%d layers=%zu out=%d opts=%d/%d/%d steps=%lld members=%lld "
            "switches=%d/%d: rc %d '%s'\n", row.in, row.hidden.size() + 1, row.out, row.hact,
            row.oact, row.ln, (long long)row.n_steps, (long long)row.members, row.wide_on,
            row.res_on, rc, g_error.c_str());
  CHECK(ok);
  // the two predicates of the C ABI say the same
  CHECK(ga_policy_step_fused_supported(&c.net.d) == (row.width == 256));
  CHECK(ga_policy_step_wide_supported(&c.net.d) == (row.width != 0));
  free_all();
}

static void suite_variants() {
  for (const VariantRow& row : VARIANTS) check_variant(row);
  ga_rollout_set_switches(1, 1);
  // members of more than one workgroup: 2 members x 48 envs, 6 workgroups, 3 each; the
  // stride may exceed the vector
  reset();
  Opt o; o.n = 96; o.members = 2; o.stride_extra = 8;
  Case c(o);
  accepted("2 x 48", run_members(c, 3), "policy_step");
  CHECK(g_launches[0].blocks == 6 && g_launches[0].wg_per_member == 3 &&
        g_launches[0].member_stride == (int)c.net.flat + 8);
  // the policy step alone: no env, one step, never counted
  reset();
  Opt p; p.n = 17;
  Case d(p);
  accepted("policy only", run_policy_only(d), "policy_step");
  CHECK(g_launches[0].env_step == 0 && g_launches[0].n_steps == 1 &&
        g_launches[0].blocks == 2 && g_prof_counts.empty());
  // a rescaled rollout sets the bit; bounds without the fused entry do not reach the env
  reset();
  Opt q; q.rescale = 1; q.norm = 2;
  Case e(q);
  accepted("rescaled", run_fused(e, 2), "policy_step");
  CHECK(g_launches[0].env_step == (1 | ENV_STEP_RESCALE));
  reset();
  accepted("rescale bounds, per-layer path", run_step_record(e), "env_step_record");
  reset();
  free_all();
}

// ---- the conversions, every kind, every entry point -----------------------------------------
static void suite_conversions() {
  ga_rollout_set_switches(1, 1);
  for (int kind : KINDS)
    for (int norm = 0; norm < 3; ++norm)
      for (int rescale = 0; rescale < 2; ++rescale) {
        Opt o; o.kind = kind; o.norm = norm; o.rescale = rescale; o.n = 300; o.col = 2;
        Case c(o);
        const std::string what = "kind " + std::to_string(kind);
        reset(); accepted(what + " reset", run_env_reset(c), "env_reset");
        CHECK(g_launches[0].blocks == 2);
        reset(); accepted(what + " step", run_env_step(c), "env_step");
        reset(); accepted(what + " step_record", run_step_record(c), "env_step_record");
        reset(); accepted(what + " record", run_record(c), "record");
        reset(); accepted(what + " head", run_head(c), "head");
        reset();
        if (rescale && c.discrete) {
          refused(what + " rescale of a discrete kind", run_fused(c, 3),
                  "ga_policy_env_step_fused_f32: action rescale needs bounds, scratch and a "
                  "continuous action space");
        } else {
          accepted(what + " fused", run_fused(c, 3), "policy_step");
          CHECK(g_launches[0].blocks == 19);
          if (!rescale) {
            reset(); accepted(what + " members", run_members(c, 3), "policy_step");
          }
        }
        reset();
        free_all();
      }
  // MountainCar-v0 and the plain multi-task mode: the other value of each kind's switch
  {
    Opt o; o.kind = GA_ENV_MOUNTAIN_CAR; o.continuous = 0;
    Case c(o);
    CHECK(c.discrete == 1);
    reset(); accepted("MountainCar-v0", run_fused(c, 2), "policy_step");
    Opt m; m.kind = GA_ENV_MULTI_POINT; m.onehot = 0;
    Case d(m);
    CHECK(d.obs_dim == 3);
    reset(); accepted("multi vanilla", run_fused(d, 2), "policy_step");
    // a discrete synthetic env takes a class index: one action column
    Opt s; s.synth_discrete = 1;
    Case e(s);
    CHECK(e.act_w == 1 && e.h.kind == 1);
    reset(); accepted("synth discrete", run_fused(e, 2), "policy_step");
    reset();
    free_all();
  }
  // the training forward: 64 rows per workgroup
  {
    Opt o; o.n = 65; o.hidden = {16, 16};
    Case c(o);
    g_case = &c;
    float* X = dev<float>(64 * 8 + 5);
    float* out = dev<float>(64 * 4 + 3);
    float* acts = dev<float>(4);
    reset();
    accepted("train forward",
             ga_mlp_forward_fused_f32(&c.net.d, c.params, X, 8, nullptr, 65, acts, out, 4,
                                      (ga_stream_t)S1), "train_forward");
    CHECK(g_launches[0].blocks == 2);
    reset();
    refused("train forward: options",
            (c.net.d.hidden_act = 2,
             ga_mlp_forward_fused_f32(&c.net.d, c.params, X, 8, nullptr, 65, acts, out, 4,
                                      (ga_stream_t)S1)),
            "ga_mlp_forward_fused_f32: unsupported network shape or options");
    c.net.d.hidden_act = 0;
    refused("train forward: acts",
            ga_mlp_forward_fused_f32(&c.net.d, c.params, X, 8, nullptr, 65, nullptr, out, 4,
                                     (ga_stream_t)S1),
            "ga_mlp_forward_fused_f32: acts needed");
    refused("train forward: M",
            ga_mlp_forward_fused_f32(&c.net.d, c.params, X, 8, nullptr, 1ll << 31, acts, out, 4,
                                     (ga_stream_t)S1),
            "ga_mlp_forward_fused_f32: bad M");
    refused("train forward: alignment",
            ga_mlp_forward_fused_f32(&c.net.d, c.params + 1, X, 8, nullptr, 65, acts, out, 4,
                                     (ga_stream_t)S1),
            "ga_mlp_forward_fused_f32: params alignment");
    free_all();
  }
}

// ---- every refusal, before any launch ---------------------------------------------------------
struct Spoil {
  std::string name;
  std::function<void(Case&)> spoil;
  std::string message;  // after "<entry point>: "
};
template <class E>
static void state_spoilers(std::vector<Spoil>& v, E Case::*m) {
  v.push_back({"state", [m](Case& c) { (c.*m).state = nullptr; }, "null env state"});
  v.push_back({"t", [m](Case& c) { (c.*m).t = nullptr; }, "null env state"});
  v.push_back({"resets", [m](Case& c) { (c.*m).resets = nullptr; }, "null env state"});
  v.push_back({"n", [m](Case& c) { (c.*m).n = 0; }, "bad env size"});
  v.push_back({"mel 0", [m](Case& c) { (c.*m).max_episode_length = 0; },
               "max_episode_length must be in 1..65535"});
  v.push_back({"mel 65536", [m](Case& c) { (c.*m).max_episode_length = 65536; },
               "max_episode_length must be in 1..65535"});
}
// what is wrong with the env itself: every entry point that takes the env says the same
static std::vector<Spoil> env_spoilers(int kind) {
  std::vector<Spoil> v;
  const char* mel = "max_episode_length must be in 1..65535";
  switch (kind) {
    case GA_ENV_SYNTH:
      v.push_back({"episode", [](Case& c) { c.synth.episode = nullptr; }, "null env state"});
      v.push_back({"t", [](Case& c) { c.synth.t = nullptr; }, "null env state"});
      v.push_back({"len", [](Case& c) { c.synth.len = nullptr; }, "null env state"});
      v.push_back({"n", [](Case& c) { c.synth.n = 0; }, "bad env sizes"});
      v.push_back({"act_dim", [](Case& c) { c.synth.act_dim = 0; }, "bad env sizes"});
      v.push_back({"min_len 0", [](Case& c) { c.synth.min_len = 0; },
                   "episode lengths must satisfy 1 <= min <= max <= 65535"});
      v.push_back({"max_len 65536", [](Case& c) { c.synth.max_len = 65536; },
                   "episode lengths must satisfy 1 <= min <= max <= 65535"});
      v.push_back({"min > max", [](Case& c) { c.synth.min_len = 10; },
                   "episode lengths must satisfy 1 <= min <= max <= 65535"});
      break;
    case GA_ENV_POINT:
      v.push_back({"point", [](Case& c) { c.point.point = nullptr; }, "null env state"});
      v.push_back({"goal", [](Case& c) { c.point.goal = nullptr; }, "null env state"});
      v.push_back({"t", [](Case& c) { c.point.t = nullptr; }, "null env state"});
      v.push_back({"n", [](Case& c) { c.point.n = 0; }, "bad env size"});
      v.push_back({"arena", [](Case& c) { c.point.arena_size = -1.f; },
                   "arena_size must be >= 0"});
      v.push_back({"mel 0", [](Case& c) { c.point.max_episode_length = 0; }, mel});
      v.push_back({"mel 65536", [](Case& c) { c.point.max_episode_length = 65536; }, mel});
      break;
    case GA_ENV_GRID:
      v.push_back({"map", [](Case& c) { c.grid.map = nullptr; }, "null env state"});
      v.push_back({"start", [](Case& c) { c.grid.start = nullptr; }, "null env state"});
      v.push_back({"state", [](Case& c) { c.grid.state = nullptr; }, "null env state"});
      v.push_back({"t", [](Case& c) { c.grid.t = nullptr; }, "null env state"});
      v.push_back({"n", [](Case& c) { c.grid.n = 0; }, "bad env sizes"});
      v.push_back({"4097 columns", [](Case& c) { c.grid.rows = 1; c.grid.cols = 4097; },
                   "bad env sizes"});
      v.push_back({"2^20 + cells", [](Case& c) { c.grid.rows = 1025; c.grid.cols = 1024; },
                   "bad env sizes"});
      v.push_back({"mel 0", [](Case& c) { c.grid.max_episode_length = 0; }, mel});
      v.push_back({"mel 65536", [](Case& c) { c.grid.max_episode_length = 65536; }, mel});
      break;
    case GA_ENV_MULTI_POINT:
      v.push_back({"point", [](Case& c) { c.multi.point = nullptr; }, "null env state"});
      v.push_back({"goal", [](Case& c) { c.multi.goal = nullptr; }, "null env state"});
      v.push_back({"t", [](Case& c) { c.multi.t = nullptr; }, "null env state"});
      v.push_back({"task_goals", [](Case& c) { c.multi.task_goals = nullptr; },
                   "null env state"});
      v.push_back({"last_task", [](Case& c) { c.multi.last_task = nullptr; },
                   "null env state"});
      v.push_back({"resets", [](Case& c) { c.multi.resets = nullptr; }, "null env state"});
      v.push_back({"n", [](Case& c) { c.multi.n = 0; }, "bad env size"});
      v.push_back({"arena", [](Case& c) { c.multi.arena_size = -1.f; },
                   "arena_size must be >= 0"});
      v.push_back({"mel 0", [](Case& c) { c.multi.max_episode_length = 0; }, mel});
      v.push_back({"mel 65536", [](Case& c) { c.multi.max_episode_length = 65536; }, mel});
      v.push_back({"num_tasks 0", [](Case& c) { c.multi.num_tasks = 0; },
                   "num_tasks must be in 1..256 (got 0)"});
      v.push_back({"num_tasks 257", [](Case& c) { c.multi.num_tasks = 257; },
                   "num_tasks must be in 1..256 (got 257)"});
      v.push_back({"strategy", [](Case& c) { c.multi.strategy = 2; },
                   "unknown sample strategy 2"});
      v.push_back({"mode", [](Case& c) { c.multi.mode = 2; }, "unknown mode 2"});
      break;
    case GA_ENV_CARTPOLE: state_spoilers(v, &Case::cartpole); break;
    case GA_ENV_PENDULUM: state_spoilers(v, &Case::pendulum); break;
    case GA_ENV_DOUBLE_PENDULUM: state_spoilers(v, &Case::dpend); break;
    case GA_ENV_ACROBOT: state_spoilers(v, &Case::acrobot); break;
    default:
      state_spoilers(v, &Case::mcar);
      v.push_back({"continuous 2", [](Case& c) { c.mcar.continuous = 2; },
                   "continuous must be 0 or 1"});
      break;
  }
  return v;
}
// what is wrong with the step around the env: the entry points that record a step
static std::vector<Spoil> step_spoilers(int kind) {
  std::vector<Spoil> v;
  v.push_back({"reward", [](Case& c) { c.r.reward = nullptr; }, "null pointer"});
  v.push_back({"step_samples", [](Case& c) { c.r.step_samples = nullptr; }, "null pointer"});
  v.push_back({"record n", [](Case& c) { c.r.n = c.o.n - 1; },
               "col 1 out of range (Tcap 6)"});
  v.push_back({"record mel 0", [](Case& c) { c.r.max_episode_length = 0; },
               "max_episode_length must be in 1..65535"});
  v.push_back({"record mel 65536", [](Case& c) { c.r.max_episode_length = 65536; },
               "max_episode_length must be in 1..65535"});
  v.push_back({"record obs_dim", [](Case& c) { c.r.obs_dim += 1; },
               "leading dimensions too small"});
  v.push_back({"reward statistics", [](Case& c) { c.nm.reward_var = nullptr; },
               "reward statistics"});
  v.push_back({"observation statistics", [](Case& c) { c.nm.raw_next_obs = nullptr; },
               "observation statistics / raw buffers"});
  if (kind == GA_ENV_MULTI_POINT)
    v.push_back({"ldo", [](Case& c) { c.r.ldo = c.obs_dim - 1; },
                 "observation rows of 5 columns are narrower than 3 + num_tasks = 6"});
  return v;
}

static void suite_refusals() {
  ga_rollout_set_switches(1, 1);
  struct Entry {
    const char* who;
    std::function<int(Case&)> run;
    bool records;
  };
  const std::vector<Entry> entries = {
      {"ga_env_reset", run_env_reset, false},
      {"ga_env_step", run_env_step, false},
      {"ga_env_step_record", run_step_record, true},
      {"ga_policy_env_step_fused_f32", [](Case& c) { return run_fused(c, 3); }, true},
      {"ga_policy_env_step_members_f32", [](Case& c) { return run_members(c, 3); }, true},
  };
  for (int kind : KINDS)
    for (const Entry& en : entries) {
      std::vector<Spoil> spoilers = env_spoilers(kind);
      if (en.records)
        for (const Spoil& s : step_spoilers(kind)) spoilers.push_back(s);
      for (const Spoil& s : spoilers) {
        Opt o; o.kind = kind; o.norm = 2;
        Case c(o);
        s.spoil(c);
        reset();
        refused(std::string(en.who) + " kind " + std::to_string(kind) + ": " + s.name,
                en.run(c), std::string(en.who) + ": " + s.message);
        free_all();
      }
    }
  // a null or unknown env, every entry point
  for (const Entry& en : entries) {
    Opt o;
    Case c(o);
    reset();
    c.o.kind = 7;
    refused(std::string(en.who) + ": kind 7", en.run(c),
            std::string(en.who) + ": unknown env kind 7");
    free_all();
  }
  // one case per remaining message; `o.kind` a continuous kind unless said otherwise
#define REFUSED(msg, opt, spoil, call)  \
  do {                                  \
    Opt o; opt;                         \
    Case c(o);                          \
    spoil;                              \
    reset();                            \
    refused(msg, call, msg);            \
    free_all();                         \
  } while (0)
  // ---- the leading dimensions and columns of a step
  REFUSED("ga_env_reset: bad obs buffer", o.kind = GA_ENV_POINT, c.ldo = 2, run_env_reset(c));
  REFUSED("ga_env_reset: bad obs buffer", o.kind = GA_ENV_POINT, c.obs = nullptr,
          run_env_reset(c));
  REFUSED("ga_env_step: leading dimensions too small", o.kind = GA_ENV_POINT, c.ldo = 2,
          run_env_step(c));
  REFUSED("ga_env_step: leading dimensions too small", o.kind = GA_ENV_POINT, c.lda = 1,
          run_env_step(c));
  REFUSED("ga_env_step: null pointer", o.kind = GA_ENV_POINT, c.next = nullptr,
          run_env_step(c));
  REFUSED("ga_env_step: null pointer", o.kind = GA_ENV_SYNTH, c.obs = nullptr,
          run_env_step(c));
  REFUSED("ga_env_step_record: leading dimensions too small", o.kind = GA_ENV_POINT,
          c.lda = 1, run_step_record(c));
  REFUSED("ga_env_step_record: leading dimensions too small (observation rows of 2 columns, "
          "obs_dim 3)", o.kind = GA_ENV_POINT, c.r.ldo = 2, run_step_record(c));
  REFUSED("ga_env_step_record: col 6 out of range (Tcap 6)", o.kind = GA_ENV_POINT,
          c.r.col = 6, run_step_record(c));
  REFUSED("ga_env_step_record: col -1 out of range (Tcap 6)", o.kind = GA_ENV_POINT,
          c.r.col = -1, run_step_record(c));
  REFUSED("ga_env_step_record: null pointer", o.kind = GA_ENV_POINT, c.obs = nullptr,
          run_step_record(c));
  REFUSED("ga_record_step: col 6 out of range (Tcap 6)", , c.r.col = 6, run_record(c));
  REFUSED("ga_record_step: null pointer", , c.r.done = nullptr, run_record(c));
  REFUSED("ga_record_step: max_episode_length must be in 1..65535", ,
          c.r.max_episode_length = 65536, run_record(c));
  REFUSED("ga_record_step: leading dimensions too small (observation rows of 4 columns, "
          "obs_dim 5)", , c.r.ldo = 4, run_record(c));
  REFUSED("ga_policy_head_sample: col 6 out of range (Tcap 6)", , c.h.col = 6, run_head(c));
  REFUSED("ga_policy_head_sample: null pointer", , c.h.head = nullptr, run_head(c));
  REFUSED("ga_policy_head_sample: bad sizes", , c.h.ldh = 2, run_head(c));
  REFUSED("ga_policy_head_sample: bad sizes", , c.h.ldo = 4, run_head(c));
  REFUSED("ga_policy_head_sample: gaussian head needs log_std and lda >= A", , c.h.lda = 2,
          run_head(c));
  REFUSED("ga_policy_head_sample: gaussian head needs log_std and lda >= A", ,
          c.h.log_std = nullptr, run_head(c));
  // ---- the fused step
  REFUSED("ga_policy_env_step_fused_f32: steps exceed the rollout buffer", , ,
          run_fused(c, 6));  // col 1 + 6 == Tcap + 1
  REFUSED("ga_policy_env_step_fused_f32: steps exceed the rollout buffer", , , run_fused(c, 0));
  REFUSED("ga_policy_env_step_fused_f32: steps exceed the rollout buffer", , c.h.col = 6,
          run_fused(c, 1));
  REFUSED("ga_policy_env_step_fused_f32: teacher-forced noise is per step", ,
          c.h.noise = c.obs, run_fused(c, 2));
  REFUSED("ga_policy_env_step_fused_f32: null pointer", , , (g_case = &c,
          ga_policy_env_step_fused_f32(&c.net.d, c.params, nullptr, c.ref(), &c.r, nullptr, 1,
                                       (ga_stream_t)S1)));
  REFUSED("ga_policy_env_step_fused_f32: null env", , , (g_case = &c,
          ga_policy_env_step_fused_f32(&c.net.d, c.params, &c.h, nullptr, &c.r, nullptr, 1,
                                       (ga_stream_t)S1)));
  REFUSED("ga_policy_env_step_fused_f32: env count mismatch", , (c.h.n = 19), run_fused(c, 2));
  REFUSED("ga_policy_env_step_fused_f32: record columns do not match the policy's", ,
          c.r.col = 2, run_fused(c, 2));
  REFUSED("ga_policy_env_step_fused_f32: record columns do not match the policy's", ,
          c.r.Tcap = 3, run_fused(c, 3));
  REFUSED("ga_policy_env_step_fused_f32: action rescale of 2 columns for an env of 3",
          o.rescale = 1, (c.h.A = 2), run_fused(c, 2));
  REFUSED("ga_policy_env_step_fused_f32: action rescale needs bounds, scratch and a "
          "continuous action space", o.rescale = 1, c.nm.act_high = nullptr, run_fused(c, 2));
  REFUSED("ga_policy_env_step_fused_f32: action rescale needs bounds, scratch and a "
          "continuous action space", o.rescale = 1, c.nm.scaled_action = nullptr,
          run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: head / network size mismatch", , (c.h.A = 2),
          run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: head / network size mismatch", , (c.h.obs_dim = 4),
          run_policy_only(c));
  REFUSED("ga_policy_step_fused_f32: params alignment", , c.params += 1, run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: ln_off[1] is not a multiple of 4",
          (o.ln = 1, o.hidden = {8, 8}), c.net.d.ln_off[1] += 2, run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: ln_off[0] is not a multiple of 4", o.ln = 1,
          c.net.d.ln_off[0] = 0, run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: null buffer", , c.h.act_buf = nullptr, run_fused(c, 2));
  REFUSED("ga_policy_step_fused_f32: col out of range", , c.h.col = 6, run_policy_only(c));
  REFUSED("ga_policy_step_fused_f32: null pointer", , c.params = nullptr, run_policy_only(c));
  // ---- the population entry
  REFUSED("ga_policy_env_step_members_f32: n_members must be at least 1", , c.o.members = 0,
          run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: 20 envs do not split into 3 members", ,
          c.o.members = 3, run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: 24 envs per member are not a multiple of the 16 "
          "rows of a workgroup", (o.n = 48, o.members = 2), , run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: member_stride 106 is not a multiple of 4 floats or "
          "is smaller than the 104 floats of a parameter vector",
          (o.n = 32, o.members = 2, o.stride_extra = 2), , run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: member_stride 100 is not a multiple of 4 floats or "
          "is smaller than the 104 floats of a parameter vector",
          (o.n = 32, o.members = 2), c.stride -= 4, run_members(c, 2));
  // (with layer normalisation the vector ends behind gamma and beta)
  REFUSED("ga_policy_env_step_members_f32: member_stride 116 is not a multiple of 4 floats or "
          "is smaller than the 120 floats of a parameter vector",
          (o.n = 32, o.members = 2, o.ln = 1), c.stride -= 4, run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: teacher-forced noise is not supported", ,
          c.h.noise = c.obs, run_members(c, 1));
  REFUSED("ga_policy_env_step_members_f32: the action rescale is its own launch (not "
          "supported)", o.rescale = 1, , run_members(c, 2));
  REFUSED("ga_policy_env_step_members_f32: null pointer", , c.params = nullptr,
          run_members(c, 2));
#undef REFUSED
  // a stride equal to the vector, and one ragged member, are taken
  {
    Opt o; o.n = 32; o.members = 2; o.ln = 1;
    Case c(o);
    CHECK(c.net.flat == 120 && c.stride == 120);
    reset(); accepted("stride == flat size", run_members(c, 2), "policy_step");
    Opt p; p.n = 21;
    Case d(p);
    reset(); accepted("one ragged member", run_members(d, 2), "policy_step");
    CHECK(g_launches[0].blocks == 2 && g_launches[0].member_stride == 0);
    reset();
    free_all();
  }
  // a member's offset is a 32-bit count of floats: the last vector ends below 2^31
  {
    Opt o; o.n = 32; o.members = 2;
    Case c(o);
    c.skip_params = true;
    c.stride = (1ll << 31) - c.net.flat;
    reset();
    refused("2^31 floats", run_members(c, 2),
            "ga_policy_env_step_members_f32: 2 members x 2147483544 floats exceed 2^31 floats");
    c.stride -= 4;
    accepted("2^31 - 4 floats", run_members(c, 2), "policy_step");
    CHECK(g_launches[0].member_stride == (int)((1ll << 31) - c.net.flat - 4));
    reset();
    free_all();
  }
}

// ---- the developer hook's buffer ----------------------------------------------------------------
static void suite_debug() {
  long long out[32];
  memset(out, 0x55, sizeof(out));
  g_dev_allocs.clear(); g_sync_copies.clear(); g_syncs = g_memsets = 0;
  CHECK(ga_policy_step_debug(out) == 1);  // arms
  CHECK(g_dev_allocs.size() == 1 && g_dev_allocs[0] == 32 * 8 && g_memsets == 1 &&
        g_sync_copies.empty() && g_syncs == 0);
  {  // the next launch carries the buffer
    Opt o;
    Case c(o);
    reset(); accepted("armed", run_fused(c, 2), "policy_step");
    CHECK(g_launches[0].dbg != nullptr);
    reset();
  }
  CHECK(ga_policy_step_debug(out) == 0);  // reads: one sync, then one copy
  CHECK(g_dev_allocs.size() == 1 && g_sync_copies.size() == 1 && g_sync_copies[0] == 32 * 8 &&
        g_syncs == 1 && g_syncs_at_copy == 1);
  for (int i = 0; i < 32; ++i) CHECK(out[i] == 0);
}

int main(int argc, char** argv) {
  const std::vector<Suite> suites = {
      {"variants", suite_variants, "rollout host variants ok"},
      {"conversions", suite_conversions, "rollout host conversions ok"},
      {"refusals", suite_refusals, "rollout host refusals ok"},
      {"debug", suite_debug, "rollout host debug ok"},
  };
  const int rc = run_suites(suites, argc, argv);
  free_all();
  if (!rc) printf("rollout host ok\n");
  return rc;
}
