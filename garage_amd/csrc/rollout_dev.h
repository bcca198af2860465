// Device-side pieces of the rollout step shared by rollout.hip and the fused
// policy + env step of policy_fused.hip, each written once: Philox, the head of a step
// (HeadDev, head_one), the device environments (synthetic, PointEnv, GridWorldEnv,
// MultiEnvWrapper over PointEnv, CartPole, Pendulum, the inverted double pendulum,
// Acrobot, MountainCar;
// env_pre / env_core / env_reset_one of each -- of the last five, the seeded
// state-vector kinds, written once over a kind description: StateEnv<K>),
// the NormalizedEnv statistics, the per-step bookkeeping of VecWorker.step_episode
// (sampler/vec_worker.py:176-204; RecordParams).  One thread owns one env.
#pragma once
#include "common.h"
#include "rollout_params.h"  // the structs these functions read: host C++

namespace ga_rollout {

// ---- Philox4x32-10 (Random123; Salmon et al. SC'11) --------------------------
struct U4 { uint32_t x, y, z, w; };

static __host__ __device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                            uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}

// The env's arithmetic is numpy's: every product and sum rounded on its own.  The
// __fmul_rn / __fadd_rn intrinsics are plain operators in this toolchain and may
// be contracted into FMAs with their neighbours, so the functions below switch
// contraction off for their own statements instead.
//
// uint32 -> fp32 uniform on [-sqrt3, sqrt3): every step exact or singly rounded,
// so the CPU twin (oracle/envs.py) reproduces it bit for bit.
static __device__ __forceinline__ float u32_unit_variance(uint32_t u) {
#pragma clang fp contract(off)
  const float f = (float)(u >> 8) * 1.1920928955078125e-07f;  // 2^-23
  const float c = f - 1.0f;
  return c * 1.7320508f;
}
static __host__ __device__ __forceinline__ float u32_unit_interval(uint32_t u) {
  return ((float)(u >> 8) + 0.5f) * 5.9604644775390625e-08f;  // (0,1)
}

static constexpr uint32_t STREAM_OBS = 0, STREAM_REWARD = 1, STREAM_LENGTH = 2;
static constexpr uint32_t STREAM_ACTION = 3;
static constexpr uint32_t STREAM_TASK = 4;
static constexpr uint32_t STREAM_CARTPOLE = 5;
static constexpr uint32_t STREAM_PENDULUM = 6;
static constexpr uint32_t STREAM_DOUBLE_PENDULUM = 7;
static constexpr uint32_t STREAM_ACROBOT = 8;
static constexpr uint32_t STREAM_MOUNTAIN_CAR = 9;

// ---- action sampling ------------------------------------------------------------
static __device__ __forceinline__ void box_muller(uint32_t u0, uint32_t u1, float* z0,
                                                  float* z1) {
  const float a = u32_unit_interval(u0), b = u32_unit_interval(u1);
  const float rad = sqrtf(-2.f * logf(a));
  float s, c;
  sincosf(6.28318530717958647692f * b, &s, &c);
  *z0 = rad * c;
  *z1 = rad * s;
}

// The action noise of env `row` (global id env_id0 + row): row `row` of `noise`
// [*, ldn] when given, else the env's action stream of Philox at `step`.
struct ActionNoise {
  const float* noise;
  int64_t ldn;
  int64_t env_id0;
  uint32_t step, k0, k1;
};

// Gaussian action of one env: a_j = mu_j + sd z_j, j < A, with z from the noise row,
// or Box-Muller on the action stream (4 draws per Philox block b); emit(j, a_j)
// stores each.
template <class Emit>
static __device__ __forceinline__ void sample_gaussian(const float* mu, float sd, int A,
                                                       const ActionNoise& r, int64_t row,
                                                       Emit emit) {
  for (int b = 0; b * 4 < A; ++b) {
    float z[4];
    if (r.noise) {
      for (int j = 0; j < 4 && b * 4 + j < A; ++j) z[j] = r.noise[row * r.ldn + b * 4 + j];
    } else {
      const U4 u = philox4x32_10((uint32_t)(r.env_id0 + row), r.step, (uint32_t)b,
                                 STREAM_ACTION << 16, r.k0, r.k1);
      box_muller(u.x, u.y, &z[0], &z[1]);
      box_muller(u.z, u.w, &z[2], &z[3]);
    }
    for (int j = 0; j < 4 && b * 4 + j < A; ++j) emit(b * 4 + j, mu[b * 4 + j] + sd * z[j]);
  }
}

// Categorical action of one env by inverse CDF over softmax(sc), or
// softmax(softmax(sc)) with double_softmax, with u from the noise
// row or the first uniform of the action stream.  probs (optional) <- the
// probabilities.
static __device__ __forceinline__ int sample_categorical(const float* sc, int A,
                                                         int double_softmax,
                                                         const ActionNoise& r, int64_t row,
                                                         float* probs) {
  float mx = sc[0];
  for (int j = 1; j < A; ++j) mx = fmaxf(mx, sc[j]);
  float den = 0.f;
  for (int j = 0; j < A; ++j) den += expf(sc[j] - mx);
  float den2 = 0.f;
  if (double_softmax)
    for (int j = 0; j < A; ++j) den2 += expf(expf(sc[j] - mx) / den);
  float u;
  if (r.noise) {
    u = r.noise[row * r.ldn];
  } else {
    const U4 v = philox4x32_10((uint32_t)(r.env_id0 + row), r.step, 0u, STREAM_ACTION << 16,
                               r.k0, r.k1);
    u = u32_unit_interval(v.x);
  }
  float cdf = 0.f;
  int pick = A - 1;
  bool found = false;
  for (int j = 0; j < A; ++j) {
    float pr = expf(sc[j] - mx) / den;
    if (double_softmax) pr = expf(pr) / den2;
    if (probs) probs[j] = pr;
    cdf += pr;
    if (!found && u < cdf) { pick = j; found = true; }
  }
  return pick;
}

// ---- the head of a rollout step ------------------------------------------------
// (HeadDev: rollout_params.h)
// The head of env `env`: h = its A means (kind 0; log_std: the device scalar) or class
// scores (kind 1).  Mean / probabilities -> head_buf when given, the sample -> action
// and act_buf.  The per-layer head kernel calls it, and the fused step kernel with a
// HeadDev at its sub-step's column and Philox step.
static __device__ __forceinline__ void head_one(const HeadDev& p, const float* h, int A,
                                                const float* log_std, int64_t env) {
  const int64_t cell = env * p.Tcap + p.col;
  const ActionNoise rng = {p.noise, p.ldn, p.env_id0, p.step, p.k0, p.k1};
  if (p.head_buf && p.kind == 0)  // agent_info 'mean' (sample_categorical: the probs)
    for (int j = 0; j < A; ++j) p.head_buf[cell * p.ldh + j] = h[j];
  if (p.kind == 0) {
    const float s = ga_log_std(*log_std, p.has_min, p.min_log_std, p.has_max,
                               p.max_log_std, nullptr);
    sample_gaussian(h, expf(s), A, rng, env, [&](int j, float a) {
      p.action[env * p.lda + j] = a;
      p.act_buf[cell * p.lda + j] = a;
    });
  } else {
    const int pick = sample_categorical(h, A, p.double_softmax, rng, env,
                                        p.head_buf ? p.head_buf + cell * p.ldh : nullptr);
    p.action[env * p.lda] = (float)pick;
    p.act_buf[cell * p.lda] = (float)pick;
  }
}

// ---- synthetic environment ---------------------------------------------------
// (SynthEnv: rollout_params.h)
static __device__ __forceinline__ void synth_obs(const SynthEnv& e, uint32_t env,
                                          uint32_t episode, uint32_t t, float* out) {
  for (int b = 0; b * 4 < e.obs_dim; ++b) {
    const U4 r = philox4x32_10(env, episode, t, (STREAM_OBS << 16) | (uint32_t)b,
                               e.k0, e.k1);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    for (int j = 0; j < 4 && b * 4 + j < e.obs_dim; ++j)
      out[b * 4 + j] = u32_unit_variance(w[j]);
  }
}

static __device__ __forceinline__ int synth_len(const SynthEnv& e, uint32_t env,
                                         uint32_t episode) {
  if (e.min_len >= e.max_len) return e.max_len;
  const U4 r = philox4x32_10(env, episode, 0, STREAM_LENGTH << 16, e.k0, e.k1);
  return e.min_len + (int)(r.x % (uint32_t)(e.max_len - e.min_len + 1));
}

// reset envs where mask != 0 (mask == null: all); writes the first observation.
static __device__ __forceinline__ void env_reset_one(const SynthEnv& e, int64_t i,
                                                     float* obs, int64_t ldo) {
  const uint32_t env = (uint32_t)(e.env_id0 + i);
  const int ep = e.episode[i] + 1;
  e.episode[i] = ep;
  e.t[i] = 0;
  e.len[i] = synth_len(e, env, (uint32_t)ep);
  synth_obs(e, env, (uint32_t)ep, 0u, obs + i * ldo);
}

// ---- PointEnv (envs/point_env.py:79-170) ----------------------------------------
// numpy's fp32 arithmetic: np.clip keeps a NaN, np.linalg.norm of a 2-vector is the
// correctly rounded sqrt of the unfused sum of the two squares, and the Python
// scalars arena_size / done_bonus enter as fp32 (numpy's weak-scalar rule).
// (PointEnv: rollout_params.h)
struct PointPre {
  float px, py, gx, gy;
  int t, ep_t;
};

static __device__ __forceinline__ float np_clip(float v, float lo, float hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}
// numpy's float32 sqrt is correctly rounded; what sqrtf and __fsqrt_rn compile to
// here (v_sqrt_f32 with exponent scaling) is within 1 ulp of it.  Step to the
// neighbour whose product with the estimate brackets v (the correction LLVM emits
// for a correctly rounded f32 sqrt); tiny v is scaled by 2^32 first.
static __device__ __forceinline__ float sqrt_rn(float v) {
  const bool tiny = v < 0x1.0p-96f;
  const float x = tiny ? v * 0x1.0p+32f : v;
  const float s = __builtin_sqrtf(x);
  const float down = __int_as_float(__float_as_int(s) - 1);
  const float up = __int_as_float(__float_as_int(s) + 1);
  float r = s;
  if (__builtin_fmaf(-down, s, x) <= 0.f) r = down;
  if (__builtin_fmaf(-up, s, x) > 0.f) r = up;
  r = tiny ? r * 0x1.0p-16f : r;
  return (x == 0.f || __builtin_isinf(x)) ? x : r;
}
static __device__ __forceinline__ float norm2(float x, float y) {
#pragma clang fp contract(off)
  const float xx = x * x;
  const float yy = y * y;
  return sqrt_rn(xx + yy);
}

// reset(): point = 0, observation (0, 0, |0 - goal|)
static __device__ __forceinline__ void env_reset_one(const PointEnv& e, int64_t i,
                                                     float* obs, int64_t ldo) {
  const float gx = e.goal[2 * i], gy = e.goal[2 * i + 1];
  e.point[2 * i] = 0.f;
  e.point[2 * i + 1] = 0.f;
  e.t[i] = 0;
  float* o = obs + i * ldo;
  o[0] = 0.f;
  o[1] = 0.f;
  o[2] = norm2(0.f - gx, 0.f - gy);
}

static __device__ __forceinline__ void env_core(const PointEnv& e, int64_t i,
                                                const PointPre& s, const float* a,
                                                const float*, float* next_row,
                                                int64_t col, float* reward,
                                                uint8_t* step_type) {
#pragma clang fp contract(off)
  const float ax = np_clip(a[0], -0.1f, 0.1f), ay = np_clip(a[1], -0.1f, 0.1f);
  const float sx = s.px + ax, sy = s.py + ay;
  const float px = np_clip(sx, -e.arena, e.arena), py = np_clip(sy, -e.arena, e.arena);
  e.point[2 * i] = px;
  e.point[2 * i + 1] = py;
  const float dist = norm2(px - s.gx, py - s.gy);
  const bool succ = dist < norm2(-0.1f, -0.1f);
  float r = -dist;
  if (succ) r = r + e.bonus;
  *reward = r;
  const bool done = succ && !e.never_done;
  const int tn = s.t + 1;
  e.t[i] = tn;
  // StepType.get_step_type (_dtypes.py:42-68): TIMEOUT wins over done
  *step_type = tn >= e.max_len ? 3 : done ? 2 : tn == 1 ? 0 : 1;
  next_row[0] = px;
  next_row[1] = py;
  next_row[2] = dist;
  if (e.success) e.success[i * e.succ_ld + col] = succ ? 1 : 0;
}

// ---- MultiEnvWrapper (envs/multi_env_wrapper.py:169-226) over an inner env ------
// Every member is its own wrapper over the K task envs, which differ by a task
// payload only (PointEnv: the goal): reset() picks the next task from the member's
// own last one, copies the task's payload into the member's state and resets the
// inner env; with one_hot the K columns after the inner observation hold the
// one-hot of the active task, on reset and on every step.  An inner env joins by
// defining env_inner_obs_dim and env_apply_task.
constexpr int TASK_ROUND_ROBIN = 0, TASK_UNIFORM_RANDOM = 1;
// (MultiTaskEnv<Inner>: rollout_params.h)
template <class InnerPre>
struct MultiTaskPre {
  InnerPre in;
  int task, ep_t;
};

static __device__ __forceinline__ int env_inner_obs_dim(const PointEnv&) { return 3; }
// the member becomes PointEnv(goal=task_goals[task]); goal is the member's own row
static __device__ __forceinline__ void env_apply_task(const PointEnv& e, int64_t i,
                                                      const float* task_goals, int task) {
  float* g = const_cast<float*>(e.goal) + 2 * i;
  g[0] = task_goals[2 * task];
  g[1] = task_goals[2 * task + 1];
}

// uniform_random_strategy: the reference draws random.randint(0, K - 1) from Python's
// global generator; here reset number `counter` of env `env` takes the first word of
// its own Philox block and scales it to [0, K) by the high half of u * K (a task's
// probability is off from 1 / K by less than K / 2^32).
static __host__ __device__ __forceinline__ int task_draw(uint32_t k0, uint32_t k1,
                                                         uint32_t env, uint32_t counter,
                                                         int num_tasks) {
  const U4 r = philox4x32_10(env, counter, 0u, STREAM_TASK << 16, k0, k1);
  return (int)(((uint64_t)r.x * (uint64_t)(uint32_t)num_tasks) >> 32);
}

template <class Inner>
static __device__ __forceinline__ void task_one_hot(const MultiTaskEnv<Inner>& e, int task,
                                                    float* row) {
  if (!e.one_hot) return;
  float* h = row + env_inner_obs_dim(e.in);
  for (int j = 0; j < e.num_tasks; ++j) h[j] = j == task ? 1.f : 0.f;
}

template <class Inner>
static __device__ __forceinline__ void env_reset_one(const MultiTaskEnv<Inner>& e,
                                                     int64_t i, float* obs, int64_t ldo) {
  const int last = e.last_task[i];
  const uint32_t cnt = e.resets[i];
  // round_robin_strategy: 0 after None, else (last + 1) % K
  const int task = e.strategy == TASK_UNIFORM_RANDOM
                       ? task_draw(e.k0, e.k1, (uint32_t)i, cnt, e.num_tasks)
                       : (last < 0 ? 0 : (last + 1) % e.num_tasks);
  e.last_task[i] = task;
  e.resets[i] = cnt + 1u;
  env_apply_task(e.in, i, e.payload, task);
  env_reset_one(e.in, i, obs, ldo);
  task_one_hot(e, task, obs + i * ldo);
}

// the step's observation and env_info carry the task of the episode the step
// belongs to: env_step_one records the last observation before it resets the env
template <class Inner, class InnerPre>
static __device__ __forceinline__ void env_core(const MultiTaskEnv<Inner>& e, int64_t i,
                                                const MultiTaskPre<InnerPre>& s,
                                                const float* a, const float* o,
                                                float* next_row, int64_t col,
                                                float* reward, uint8_t* step_type) {
  env_core(e.in, i, s.in, a, o, next_row, col, reward, step_type);
  task_one_hot(e, s.task, next_row);
  if (e.task_id) e.task_id[i * e.info_ld + col] = (uint8_t)s.task;
}

// ---- GridWorldEnv (envs/grid_world_env.py:111-215) ------------------------------
// The map is read from memory (cell codes below), never from a per-thread array.
constexpr uint8_t GRID_FREE = 0, GRID_WALL = 1, GRID_HOLE = 2, GRID_GOAL = 3;
// (GridEnv: rollout_params.h)
struct GridPre {
  int s, t, ep_t;
};

// the observation row: the one-hot of the cell (HostVecEnv._put_obs of a Discrete
// observation space)
static __device__ __forceinline__ void grid_one_hot(const GridEnv& e, int cell,
                                                    float* row) {
  const int cells = e.rows * e.cols;
  for (int j = 0; j < cells; ++j) row[j] = j == cell ? 1.f : 0.f;
}

static __device__ __forceinline__ void env_reset_one(const GridEnv& e, int64_t i,
                                                     float* obs, int64_t ldo) {
  const int s = e.start[i];
  e.state[i] = s;
  e.t[i] = 0;
  grid_one_hot(e, s, obs + i * ldo);
}

static __device__ __forceinline__ void env_core(const GridEnv& e, int64_t i,
                                                const GridPre& s, const float* a,
                                                const float*, float* next_row, int64_t,
                                                float* reward, uint8_t* step_type) {
  const uint8_t* m = e.map + i * (int64_t)(e.rows * e.cols);
  const int x = s.s / e.cols, y = s.s % e.cols;
  // increments [[0, -1], [1, 0], [0, 1], [-1, 0]] for actions 0..3, clipped to the grid
  const int act = (int)a[0];
  const int nx = min(max(x + (act == 1) - (act == 3), 0), e.rows - 1);
  const int ny = min(max(y + (act == 2) - (act == 0), 0), e.cols - 1);
  const int here = m[s.s], there = m[nx * e.cols + ny];
  const bool stay = there == GRID_WALL || here == GRID_HOLE || here == GRID_GOAL;
  const int next = stay ? s.s : nx * e.cols + ny;
  const int type = stay ? here : there;
  const bool done = type == GRID_HOLE || type == GRID_GOAL;
  *reward = type == GRID_GOAL ? 1.f : 0.f;
  e.state[i] = next;
  const int tn = s.t + 1;
  e.t[i] = tn;
  *step_type = tn >= e.max_len ? 3 : done ? 2 : tn == 1 ? 0 : 1;
  grid_one_hot(e, next, next_row);
}

// ---- seeded state-vector envs: the frame ------------------------------------------
// CartPole, Pendulum, the inverted double pendulum, Acrobot and MountainCar are one
// kind of object: an [n, S] fp32 state, a step counter and a reset counter per member,
// a Philox reset stream keyed (seed; env_id0 + i, resets[i]) and a finite max_len
// whose last step is TIMEOUT.  What is not dynamics is written once, here, over a
// kind description K (CartPoleKind ... MountainCarKind below), which states
//   State, S    the state: a struct of S floats, in the order of its row of `state`
//   OBS         the observation width
//   reset_draw  (k0, k1, env, counter) -> State, on the kind's own Philox stream
//   observe     (State, o): the observation of a state (what a reset shows)
//   step        (State*, action row, variant, reward*, o) -> done: one step; o is the
//               observation of the new state
// A new kind costs that description, its C-ABI struct and its row of
// GA_STATE_ENV_KINDS (internal.h).
// (StateEnv<K>: rollout_params.h)
template <class K>
struct StatePre {
  typename K::State s;
  int t, ep_t;
};

// A State and its row: S floats either way.  The copies index with compile-time
// constants, so a state lives in registers.
template <class K>
struct StateRow { float v[K::S]; };
template <class K>
static __host__ __device__ __forceinline__ typename K::State state_load(const float* row) {
  static_assert(sizeof(typename K::State) == sizeof(StateRow<K>), "State is S floats");
  StateRow<K> w;
#pragma unroll
  for (int j = 0; j < K::S; ++j) w.v[j] = row[j];
  return __builtin_bit_cast(typename K::State, w);
}
template <class K>
static __host__ __device__ __forceinline__ void state_store(const typename K::State& s,
                                                            float* row) {
  const StateRow<K> w = __builtin_bit_cast(StateRow<K>, s);
#pragma unroll
  for (int j = 0; j < K::S; ++j) row[j] = w.v[j];
}

// The stores of a reset and of a step keep one order: (counters,) state, t, observation.
template <class K>
static __device__ __forceinline__ void env_reset_one(const StateEnv<K>& e, int64_t i,
                                                     float* obs, int64_t ldo) {
  const uint32_t cnt = e.resets[i];
  const typename K::State s = K::reset_draw(e.k0, e.k1, (uint32_t)(e.env_id0 + i), cnt);
  e.resets[i] = cnt + 1u;
  e.t[i] = 0;
  float o[K::OBS];
  K::observe(s, o);
  state_store<K>(s, e.state + K::S * i);
  float* row = obs + i * ldo;
#pragma unroll
  for (int j = 0; j < K::OBS; ++j) row[j] = o[j];
}

template <class K>
static __device__ __forceinline__ void env_core(const StateEnv<K>& e, int64_t i,
                                                const StatePre<K>& p, const float* a,
                                                const float*, float* next_row, int64_t,
                                                float* reward, uint8_t* step_type) {
  typename K::State s = p.s;
  float o[K::OBS];
  const bool done = K::step(&s, a, e.variant, reward, o);
  state_store<K>(s, e.state + K::S * i);
  const int tn = p.t + 1;
  e.t[i] = tn;
  // StepType.get_step_type (_dtypes.py:42-68): TIMEOUT wins over done
  *step_type = tn >= e.max_len ? 3 : done ? 2 : tn == 1 ? 0 : 1;
#pragma unroll
  for (int j = 0; j < K::OBS; ++j) next_row[j] = o[j];
}

// ---- CartPole (include/garage_amd.h states the arithmetic, operation by operation) ----
// One fp32 operation per statement, no contraction; `/` is the correctly rounded
// division.  The step and the reset draw are written once, here.
struct CartPoleState { float x, xd, th, thd; };

// the state reset number `counter` gives env `env` (global id)
static __host__ __device__ __forceinline__ CartPoleState cartpole_reset_draw(
    uint32_t k0, uint32_t k1, uint32_t env, uint32_t counter) {
#pragma clang fp contract(off)
  const U4 r = philox4x32_10(env, counter, 0u, STREAM_CARTPOLE << 16, k0, k1);
  const float w0 = 0.1f * u32_unit_interval(r.x);
  const float w1 = 0.1f * u32_unit_interval(r.y);
  const float w2 = 0.1f * u32_unit_interval(r.z);
  const float w3 = 0.1f * u32_unit_interval(r.w);
  return CartPoleState{-0.05f + w0, -0.05f + w1, -0.05f + w2, -0.05f + w3};
}

// one Euler step; returns done (evaluated on the new state)
static __host__ __device__ __forceinline__ bool cartpole_advance(CartPoleState* s,
                                                                 bool push_right) {
#pragma clang fp contract(off)
  constexpr float S3 = (float)(-1.0 / 6.0), S5 = (float)(1.0 / 120.0),
                  S7 = (float)(-1.0 / 5040.0);
  constexpr float C2 = -0.5f, C4 = (float)(1.0 / 24.0), C6 = (float)(-1.0 / 720.0),
                  C8 = (float)(1.0 / 40320.0);
  constexpr float FOUR_THIRDS = (float)(4.0 / 3.0);
  constexpr float TH_LIMIT = (float)(12.0 * 2.0 * 3.141592653589793 / 360.0);
  const float x = s->x, xd = s->xd, th = s->th, thd = s->thd;
  const float force = push_right ? 10.0f : -10.0f;
  const float t2 = th * th;
  float ps = t2 * S7;
  ps = S5 + ps;
  ps = t2 * ps;
  ps = S3 + ps;
  ps = t2 * ps;
  ps = 1.0f + ps;
  const float sn = th * ps;
  float pc = t2 * C8;
  pc = C6 + pc;
  pc = t2 * pc;
  pc = C4 + pc;
  pc = t2 * pc;
  pc = C2 + pc;
  pc = t2 * pc;
  const float cs = 1.0f + pc;
  const float thd2 = thd * thd;
  const float pl = 0.05f * thd2;
  const float pls = pl * sn;
  const float fsum = force + pls;
  const float temp = fsum / 1.1f;
  const float gs = 9.8f * sn;
  const float ct = cs * temp;
  const float num = gs - ct;
  const float cs2 = cs * cs;
  const float mc = 0.1f * cs2;
  const float mct = mc / 1.1f;
  const float br = FOUR_THIRDS - mct;
  const float den = 0.5f * br;
  const float th_acc = num / den;
  const float pa = 0.05f * th_acc;
  const float pac = pa * cs;
  const float pact = pac / 1.1f;
  const float x_acc = temp - pact;
  const float dx = 0.02f * xd;
  const float dxd = 0.02f * x_acc;
  const float dth = 0.02f * thd;
  const float dthd = 0.02f * th_acc;
  const float nx = x + dx;
  const float nth = th + dth;
  s->x = nx;
  s->xd = xd + dxd;
  s->th = nth;
  s->thd = thd + dthd;
  return __builtin_fabsf(nx) > 2.4f || __builtin_fabsf(nth) > TH_LIMIT;
}

// state [n, 4] x, x_dot, theta, theta_dot; the observation is the state
struct CartPoleKind {
  using State = CartPoleState;
  static constexpr int S = 4, OBS = 4;
  static __host__ __device__ __forceinline__ State reset_draw(uint32_t k0, uint32_t k1,
                                                              uint32_t env,
                                                              uint32_t counter) {
    return cartpole_reset_draw(k0, k1, env, counter);
  }
  static __device__ __forceinline__ void observe(const State& s, float* o) {
    o[0] = s.x; o[1] = s.xd; o[2] = s.th; o[3] = s.thd;
  }
  static __device__ __forceinline__ bool step(State* s, const float* a, int,
                                              float* reward, float* o) {
    const bool done = cartpole_advance(s, (int)a[0] == 1);
    *reward = 1.0f;
    observe(*s, o);
    return done;
  }
};

// ---- Pendulum (include/garage_amd.h states the arithmetic, operation by operation) ----
// One fp32 operation per statement, no contraction.  sincos, the step and the reset
// draw are written once, here.
struct PendulumState { float th, thd; };

constexpr float PENDULUM_PI = (float)3.141592653589793;
constexpr float PENDULUM_TWO_PI = (float)6.283185307179586;
constexpr float PENDULUM_HALF_PI = (float)1.5707963267948966;

// sin and cos of |th| <= PI: folded to |r| <= HALF_PI, then two fixed polynomials
static __host__ __device__ __forceinline__ void pendulum_sincos(float th, float* sn,
                                                                float* cs) {
#pragma clang fp contract(off)
  constexpr float S3 = (float)(-1.0 / 6.0), S5 = (float)(1.0 / 120.0),
                  S7 = (float)(-1.0 / 5040.0), S9 = (float)(1.0 / 362880.0),
                  S11 = (float)(-1.0 / 39916800.0), S13 = (float)(1.0 / 6227020800.0);
  constexpr float C2 = -0.5f, C4 = (float)(1.0 / 24.0), C6 = (float)(-1.0 / 720.0),
                  C8 = (float)(1.0 / 40320.0), C10 = (float)(-1.0 / 3628800.0),
                  C12 = (float)(1.0 / 479001600.0), C14 = (float)(-1.0 / 87178291200.0);
  float r = th, sg = 1.0f;
  if (th > PENDULUM_HALF_PI) {
    r = PENDULUM_PI - th;
    sg = -1.0f;
  } else if (th < -PENDULUM_HALF_PI) {
    r = -PENDULUM_PI - th;
    sg = -1.0f;
  }
  const float t2 = r * r;
  float ps = t2 * S13;
  ps = S11 + ps;
  ps = t2 * ps;
  ps = S9 + ps;
  ps = t2 * ps;
  ps = S7 + ps;
  ps = t2 * ps;
  ps = S5 + ps;
  ps = t2 * ps;
  ps = S3 + ps;
  ps = t2 * ps;
  ps = 1.0f + ps;
  const float sp = r * ps;
  // (next to +-HALF_PI the product can round to 1 + 2^-23; the cosine is 1 + a sum
  // that is never positive)
  *sn = sp < -1.0f ? -1.0f : (sp > 1.0f ? 1.0f : sp);
  float pc = t2 * C14;
  pc = C12 + pc;
  pc = t2 * pc;
  pc = C10 + pc;
  pc = t2 * pc;
  pc = C8 + pc;
  pc = t2 * pc;
  pc = C6 + pc;
  pc = t2 * pc;
  pc = C4 + pc;
  pc = t2 * pc;
  pc = C2 + pc;
  pc = t2 * pc;
  pc = 1.0f + pc;
  *cs = sg * pc;
}

// the state reset number `counter` gives env `env` (global id)
static __host__ __device__ __forceinline__ PendulumState pendulum_reset_draw(
    uint32_t k0, uint32_t k1, uint32_t env, uint32_t counter) {
#pragma clang fp contract(off)
  const U4 r = philox4x32_10(env, counter, 0u, STREAM_PENDULUM << 16, k0, k1);
  const float w0 = PENDULUM_TWO_PI * u32_unit_interval(r.x);
  const float w1 = 2.0f * u32_unit_interval(r.y);
  return PendulumState{-PENDULUM_PI + w0, -1.0f + w1};
}

// one step with torque `a` (clipped here); returns the reward.  Only the sine of the
// old angle is evaluated: the cost and the dynamics need no cosine.
static __host__ __device__ __forceinline__ float pendulum_advance(PendulumState* s,
                                                                  float a) {
#pragma clang fp contract(off)
  const float th = s->th, thd = s->thd;
  const float u = a < -2.0f ? -2.0f : (a > 2.0f ? 2.0f : a);
  float sn, cs_unused;
  pendulum_sincos(th, &sn, &cs_unused);
  const float c1 = th * th;
  const float c2 = thd * thd;
  const float c3 = 0.1f * c2;
  const float c4 = c1 + c3;
  const float c5 = u * u;
  const float c6 = 0.001f * c5;
  const float cost = c4 + c6;
  const float g1 = 15.0f * sn;
  const float g2 = 3.0f * u;
  const float acc = g1 + g2;
  const float dv = acc * 0.05f;
  const float v = thd + dv;
  const float dth = v * 0.05f;
  float nth = th + dth;
  const float nthd = v < -8.0f ? -8.0f : (v > 8.0f ? 8.0f : v);
  if (nth >= PENDULUM_PI) nth = nth - PENDULUM_TWO_PI;
  else if (nth < -PENDULUM_PI) nth = nth + PENDULUM_TWO_PI;
  s->th = nth;
  s->thd = nthd;
  return -cost;
}

// state [n, 2] theta in [-PI, PI], theta_dot in [-8, 8]
struct PendulumKind {
  using State = PendulumState;
  static constexpr int S = 2, OBS = 3;
  static __host__ __device__ __forceinline__ State reset_draw(uint32_t k0, uint32_t k1,
                                                              uint32_t env,
                                                              uint32_t counter) {
    return pendulum_reset_draw(k0, k1, env, counter);
  }
  static __device__ __forceinline__ void observe(const State& s, float* o) {
    float sn, cs;
    pendulum_sincos(s.th, &sn, &cs);
    o[0] = cs; o[1] = sn; o[2] = s.thd;
  }
  // never done: the step that reaches max_len is TIMEOUT
  static __device__ __forceinline__ bool step(State* s, const float* a, int,
                                              float* reward, float* o) {
    *reward = pendulum_advance(s, a[0]);
    observe(*s, o);
    return false;
  }
};

// ---- Inverted double pendulum on a cart (include/garage_amd.h states the arithmetic,
// operation by operation) ----
// One fp32 operation per statement, no contraction; `/` is the correctly rounded
// division.  The step and the reset draw are written once, here; sin and cos are
// Pendulum's.
struct DoublePendulumState { float x, th1, th2, xd, th1d, th2d; };
// what a step (or a reset) shows of the state it leaves: the sines and cosines of the
// two angles and of their difference
struct DoublePendulumTrig { float s1, c1, sd, cd, yt; };

constexpr float DP_D1 = (float)(10.5 + 4.2 + 4.2);
constexpr float DP_D2 = (float)((4.2 / 2.0 + 4.2) * 0.6);
constexpr float DP_D3 = (float)(4.2 * 0.6 / 2.0);
constexpr float DP_D4 = (float)((4.2 / 3.0 + 4.2) * 0.6 * 0.6);
constexpr float DP_D5 = (float)(4.2 * 0.6 * 0.6 / 2.0);
constexpr float DP_D6 = (float)(4.2 * 0.6 * 0.6 / 3.0);
constexpr float DP_F1 = (float)((4.2 / 2.0 + 4.2) * 0.6 * 9.81);
constexpr float DP_F2 = (float)(4.2 * 0.6 * 9.81 / 2.0);

// the state reset number `counter` gives env `env` (global id)
static __host__ __device__ __forceinline__ DoublePendulumState double_pendulum_reset_draw(
    uint32_t k0, uint32_t k1, uint32_t env, uint32_t counter) {
#pragma clang fp contract(off)
  const U4 a = philox4x32_10(env, counter, 0u, STREAM_DOUBLE_PENDULUM << 16, k0, k1);
  const U4 b = philox4x32_10(env, counter, 1u, STREAM_DOUBLE_PENDULUM << 16, k0, k1);
  const float w0 = 0.2f * u32_unit_interval(a.x);
  const float w1 = 0.2f * u32_unit_interval(a.y);
  const float w2 = 0.2f * u32_unit_interval(a.z);
  const float w3 = 0.2f * u32_unit_interval(a.w);
  const float w4 = 0.2f * u32_unit_interval(b.x);
  const float w5 = 0.2f * u32_unit_interval(b.y);
  return DoublePendulumState{-0.1f + w0, -0.1f + w1, -0.1f + w2,
                             -0.1f + w3, -0.1f + w4, -0.1f + w5};
}

static __host__ __device__ __forceinline__ float double_pendulum_clip(float v, float b) {
  return v < -b ? -b : (v > b ? b : v);
}

static __host__ __device__ __forceinline__ float double_pendulum_wrap(float th) {
#pragma clang fp contract(off)
  if (th >= PENDULUM_PI) th = th - PENDULUM_TWO_PI;
  else if (th < -PENDULUM_PI) th = th + PENDULUM_TWO_PI;
  return th;
}

// sincos of the two angles of `s`, and what follows from them alone
static __host__ __device__ __forceinline__ DoublePendulumTrig double_pendulum_trig(
    const DoublePendulumState& s, float* s2_out) {
#pragma clang fp contract(off)
  float s1, c1, s2, c2;
  pendulum_sincos(s.th1, &s1, &c1);
  pendulum_sincos(s.th2, &s2, &c2);
  const float cc = c1 * c2;
  const float ss = s1 * s2;
  const float sc = s1 * c2;
  const float cs = c1 * s2;
  const float y1 = 0.6f * c1;
  const float y2 = 0.6f * c2;
  *s2_out = s2;
  return DoublePendulumTrig{s1, c1, sc - cs, cc + ss, y1 + y2};
}

// the observation of state `s` (11 entries)
static __host__ __device__ __forceinline__ void double_pendulum_obs(
    const DoublePendulumState& s, const DoublePendulumTrig& g, float* o) {
#pragma clang fp contract(off)
  const float w2 = s.th2d - s.th1d;
  o[0] = s.x; o[1] = g.s1; o[2] = -g.sd; o[3] = g.c1; o[4] = g.cd;
  o[5] = double_pendulum_clip(s.xd, 10.0f);
  o[6] = double_pendulum_clip(s.th1d, 10.0f);
  o[7] = double_pendulum_clip(w2, 10.0f);
  o[8] = 0.0f; o[9] = 0.0f; o[10] = 0.0f;
}

// one env step (five substeps) with action `a` (clipped here): the reward, done, and
// the trigonometry of the new state.  The solve lives in named scalars: nothing is
// indexed dynamically.  (The substep loop is left to the compiler, which unrolls it:
// kept rolled, the streamed tanh rollout kernel reserved 180 B of private segment.)
static __host__ __device__ __forceinline__ float double_pendulum_advance(
    DoublePendulumState* st, float a, DoublePendulumTrig* trig, bool* done) {
#pragma clang fp contract(off)
  constexpr float H = 0.01f, VMAX = 100.0f;
  const float u = double_pendulum_clip(a, 1.0f);
  const float F = 500.0f * u;
  float x = st->x, th1 = st->th1, th2 = st->th2;
  float xd = st->xd, th1d = st->th1d, th2d = st->th2d;
  for (int k = 0; k < 5; ++k) {
    float s1, c1, s2, c2;
    pendulum_sincos(th1, &s1, &c1);
    pendulum_sincos(th2, &s2, &c2);
    const float cc = c1 * c2;
    const float ss = s1 * s2;
    const float cd = cc + ss;
    const float sc = s1 * c2;
    const float cs = c1 * s2;
    const float sd = sc - cs;
    const float q1 = th1d * th1d;
    const float q2 = th2d * th2d;
    const float a12 = DP_D2 * c1;
    const float a13 = DP_D3 * c2;
    const float a23 = DP_D5 * cd;
    const float b1 = DP_D2 * s1;
    const float b2 = b1 * q1;
    const float b3 = DP_D3 * s2;
    const float b4 = b3 * q2;
    const float b5 = F + b2;
    const float r1 = b5 + b4;
    const float e1 = DP_D5 * sd;
    const float g1 = DP_F1 * s1;
    const float e2 = e1 * q2;
    const float r2 = g1 - e2;
    const float g2 = DP_F2 * s2;
    const float e3 = e1 * q1;
    const float r3 = g2 + e3;
    // D = L diag(D1, p22, p33) L^T, L unit lower triangular (l21, l31, l32)
    const float l21 = a12 / DP_D1;
    const float l31 = a13 / DP_D1;
    const float m1 = l21 * a12;
    const float p22 = DP_D4 - m1;
    const float m2 = l21 * a13;
    const float t23 = a23 - m2;
    const float m3 = l31 * a13;
    const float t33 = DP_D6 - m3;
    const float l32 = t23 / p22;
    const float m4 = l32 * t23;
    const float p33 = t33 - m4;
    // L y = r
    const float m5 = l21 * r1;
    const float y2 = r2 - m5;
    const float m6 = l31 * r1;
    const float y3a = r3 - m6;
    const float m7 = l32 * y2;
    const float y3 = y3a - m7;
    // diag z = y, L^T qdd = z
    const float z1 = r1 / DP_D1;
    const float z2 = y2 / p22;
    const float acc3 = y3 / p33;
    const float m8 = l32 * acc3;
    const float acc2 = z2 - m8;
    const float m9 = l21 * acc2;
    const float z1a = z1 - m9;
    const float m10 = l31 * acc3;
    const float acc1 = z1a - m10;
    const float dv1 = H * acc1;
    const float dv2 = H * acc2;
    const float dv3 = H * acc3;
    const float v1 = xd + dv1;
    const float v2 = th1d + dv2;
    const float v3 = th2d + dv3;
    xd = double_pendulum_clip(v1, VMAX);
    th1d = double_pendulum_clip(v2, VMAX);
    th2d = double_pendulum_clip(v3, VMAX);
    const float dx = H * xd;
    const float dt1 = H * th1d;
    const float dt2 = H * th2d;
    x = x + dx;
    const float n1 = th1 + dt1;
    const float n2 = th2 + dt2;
    th1 = double_pendulum_wrap(n1);
    th2 = double_pendulum_wrap(n2);
  }
  st->x = x; st->th1 = th1; st->th2 = th2;
  st->xd = xd; st->th1d = th1d; st->th2d = th2d;
  float s2;
  const DoublePendulumTrig g = double_pendulum_trig(*st, &s2);
  const float xa = 0.6f * g.s1;
  const float xb = 0.6f * s2;
  const float xc = x + xa;
  const float xt = xc + xb;
  const float xt2 = xt * xt;
  const float dist_x = 0.01f * xt2;
  const float dy = g.yt - 2.0f;
  const float dy2 = dy * dy;
  const float dist = dist_x + dy2;
  const float w2 = th2d - th1d;
  const float w1s = th1d * th1d;
  const float w2s = w2 * w2;
  const float vp1 = 0.001f * w1s;
  const float vp2 = 0.005f * w2s;
  const float vel = vp1 + vp2;
  const float alive = 10.0f - dist;
  *trig = g;
  *done = g.yt <= 1.0f;
  return alive - vel;
}

// state [n, 6] x, th1, th2, xd, th1d, th2d; th1, th2 in [-PI, PI]
struct DoublePendulumKind {
  using State = DoublePendulumState;
  static constexpr int S = 6, OBS = 11;
  static __host__ __device__ __forceinline__ State reset_draw(uint32_t k0, uint32_t k1,
                                                              uint32_t env,
                                                              uint32_t counter) {
    return double_pendulum_reset_draw(k0, k1, env, counter);
  }
  static __device__ __forceinline__ void observe(const State& s, float* o) {
    float s2_unused;
    double_pendulum_obs(s, double_pendulum_trig(s, &s2_unused), o);
  }
  // the observation comes from the trigonometry the step has already evaluated
  static __device__ __forceinline__ bool step(State* s, const float* a, int,
                                              float* reward, float* o) {
    DoublePendulumTrig g;
    bool done;
    *reward = double_pendulum_advance(s, a[0], &g, &done);
    double_pendulum_obs(*s, g, o);
    return done;
  }
};

// ---- Acrobot (include/garage_amd.h states the arithmetic, operation by operation) ----
// One fp32 operation per statement, no contraction; `/` is the correctly rounded
// division.  The reduction, the dynamics, the RK4 step and the reset draw are written
// once, here; sin and cos are Pendulum's.
struct AcrobotState { float th1, th2, w1, w2; };
struct AcrobotTrig { float s1, c1, s2, c2; };

constexpr float ACROBOT_INV_TWO_PI = (float)(1.0 / 6.283185307179586);
constexpr float ACROBOT_R_HI = 6.28125f;
constexpr float ACROBOT_R_LO = (float)(6.283185307179586 - 6.28125);
constexpr float ACROBOT_MAX_VEL_1 = (float)(4.0 * 3.141592653589793);
constexpr float ACROBOT_MAX_VEL_2 = (float)(9.0 * 3.141592653589793);

// the state reset number `counter` gives env `env` (global id)
static __host__ __device__ __forceinline__ AcrobotState acrobot_reset_draw(
    uint32_t k0, uint32_t k1, uint32_t env, uint32_t counter) {
#pragma clang fp contract(off)
  const U4 r = philox4x32_10(env, counter, 0u, STREAM_ACROBOT << 16, k0, k1);
  const float w0 = 0.2f * u32_unit_interval(r.x);
  const float w1 = 0.2f * u32_unit_interval(r.y);
  const float w2 = 0.2f * u32_unit_interval(r.z);
  const float w3 = 0.2f * u32_unit_interval(r.w);
  return AcrobotState{-0.1f + w0, -0.1f + w1, -0.1f + w2, -0.1f + w3};
}

// any stage angle (|th| < 34, the header says why) brought into [-PI, PI]: k * R_HI is
// exact, so the only roundings of size are the last subtraction's and the wrap's
static __host__ __device__ __forceinline__ float acrobot_reduce(float th) {
#pragma clang fp contract(off)
  const float q = th * ACROBOT_INV_TWO_PI;
  const float k = __builtin_rintf(q);
  const float m1 = k * ACROBOT_R_HI;
  const float r1 = th - m1;
  const float m2 = k * ACROBOT_R_LO;
  float r = r1 - m2;
  if (r >= PENDULUM_PI) r = r - PENDULUM_TWO_PI;
  else if (r < -PENDULUM_PI) r = r + PENDULUM_TWO_PI;
  return r;
}

// the accelerations of the book dynamics at (unreduced) angles th1, th2 and speeds w1,
// w2 under torque a
static __host__ __device__ __forceinline__ void acrobot_dynamics(float th1, float th2,
                                                                 float w1, float w2,
                                                                 float a, float* acc1_out,
                                                                 float* acc2_out) {
#pragma clang fp contract(off)
  float s1, c1, s2, c2;
  pendulum_sincos(acrobot_reduce(th1), &s1, &c1);
  pendulum_sincos(acrobot_reduce(th2), &s2, &c2);
  const float d1 = 3.5f + c2;
  const float hc = 0.5f * c2;
  const float d2 = 1.25f + hc;
  const float sc = s1 * c2;
  const float cs = c1 * s2;
  const float s12 = sc + cs;
  const float phi2 = 4.9f * s12;
  const float q2 = w2 * w2;
  const float p1 = -0.5f * q2;
  const float p2 = p1 * s2;
  const float p3 = w2 * w1;
  const float p4 = p3 * s2;
  const float p5 = p2 - p4;
  const float p6 = 14.7f * s1;
  const float p7 = p6 + phi2;
  const float phi1 = p5 + p7;
  const float r = d2 / d1;
  const float e1 = r * phi1;
  const float e2 = a + e1;
  const float q1 = w1 * w1;
  const float e3 = 0.5f * q1;
  const float e4 = e3 * s2;
  const float e5 = e2 - e4;
  const float e6 = e5 - phi2;
  const float e7 = d2 * r;
  const float den = 1.25f - e7;
  const float acc2 = e6 / den;
  const float g1 = d2 * acc2;
  const float g2 = g1 + phi1;
  const float g3 = g2 / d1;
  *acc1_out = -g3;
  *acc2_out = acc2;
}

// one env step (one classical RK4 step of 0.2) with torque `a`: the new state, its
// sines and cosines, and done.  k1..k4 are summed as they come (the order the header
// gives), so one stage is live at a time.
static __host__ __device__ __forceinline__ bool acrobot_advance(AcrobotState* st, float a,
                                                                AcrobotTrig* trig) {
#pragma clang fp contract(off)
  constexpr float H6 = (float)(0.2 / 6.0);
  const float th1 = st->th1, th2 = st->th2, w1 = st->w1, w2 = st->w2;
  float k1 = w1, k2 = w2, k3, k4;
  acrobot_dynamics(th1, th2, w1, w2, a, &k3, &k4);
  float s_t1 = k1, s_t2 = k2, s_w1 = k3, s_w2 = k4;
#pragma unroll
  for (int stage = 0; stage < 3; ++stage) {
    const float h = stage == 2 ? 0.2f : 0.1f;
    const float dt1 = h * k1;
    const float dt2 = h * k2;
    const float dw1 = h * k3;
    const float dw2 = h * k4;
    const float y1 = th1 + dt1;
    const float y2 = th2 + dt2;
    const float v1 = w1 + dw1;
    const float v2 = w2 + dw2;
    acrobot_dynamics(y1, y2, v1, v2, a, &k3, &k4);
    k1 = v1;
    k2 = v2;
    if (stage == 2) {
      s_t1 = s_t1 + k1;
      s_t2 = s_t2 + k2;
      s_w1 = s_w1 + k3;
      s_w2 = s_w2 + k4;
    } else {
      const float b1 = 2.0f * k1;
      const float b2 = 2.0f * k2;
      const float b3 = 2.0f * k3;
      const float b4 = 2.0f * k4;
      s_t1 = s_t1 + b1;
      s_t2 = s_t2 + b2;
      s_w1 = s_w1 + b3;
      s_w2 = s_w2 + b4;
    }
  }
  const float i1 = H6 * s_t1;
  const float i2 = H6 * s_t2;
  const float i3 = H6 * s_w1;
  const float i4 = H6 * s_w2;
  const float n1 = th1 + i1;
  const float n2 = th2 + i2;
  const float u1 = w1 + i3;
  const float u2 = w2 + i4;
  st->th1 = acrobot_reduce(n1);
  st->th2 = acrobot_reduce(n2);
  st->w1 = double_pendulum_clip(u1, ACROBOT_MAX_VEL_1);
  st->w2 = double_pendulum_clip(u2, ACROBOT_MAX_VEL_2);
  AcrobotTrig g;
  pendulum_sincos(st->th1, &g.s1, &g.c1);
  pendulum_sincos(st->th2, &g.s2, &g.c2);
  const float cc = g.c1 * g.c2;
  const float ss = g.s1 * g.s2;
  const float c12 = cc - ss;
  const float hgt = (-g.c1) - c12;
  *trig = g;
  return hgt > 1.0f;
}

// class index -> torque: 0 is -1, 2 is +1, anything else none
static __host__ __device__ __forceinline__ float three_way_push(int k) {
  return k == 0 ? -1.0f : (k == 2 ? 1.0f : 0.0f);
}

// state [n, 4] th1, th2, thd1, thd2; th1, th2 in [-PI, PI]
struct AcrobotKind {
  using State = AcrobotState;
  static constexpr int S = 4, OBS = 6;
  static __host__ __device__ __forceinline__ State reset_draw(uint32_t k0, uint32_t k1,
                                                              uint32_t env,
                                                              uint32_t counter) {
    return acrobot_reset_draw(k0, k1, env, counter);
  }
  static __device__ __forceinline__ void show(const State& s, const AcrobotTrig& g,
                                              float* o) {
    o[0] = g.c1; o[1] = g.s1; o[2] = g.c2; o[3] = g.s2; o[4] = s.w1; o[5] = s.w2;
  }
  static __device__ __forceinline__ void observe(const State& s, float* o) {
    AcrobotTrig g;
    pendulum_sincos(s.th1, &g.s1, &g.c1);
    pendulum_sincos(s.th2, &g.s2, &g.c2);
    show(s, g, o);
  }
  // the observation comes from the sines and cosines the step has already evaluated
  static __device__ __forceinline__ bool step(State* s, const float* a, int,
                                              float* reward, float* o) {
    AcrobotTrig g;
    const bool done = acrobot_advance(s, three_way_push((int)a[0]), &g);
    *reward = done ? 0.0f : -1.0f;
    show(*s, g, o);
    return done;
  }
};

// ---- MountainCar, discrete and continuous (include/garage_amd.h states the arithmetic,
// operation by operation) ----
// One fp32 operation per statement, no contraction.  The step and the reset draw are
// written once, here; the cosine is Pendulum's.
struct MountainCarState { float x, v; };

// the state reset number `counter` gives env `env` (global id)
static __host__ __device__ __forceinline__ MountainCarState mountain_car_reset_draw(
    uint32_t k0, uint32_t k1, uint32_t env, uint32_t counter) {
#pragma clang fp contract(off)
  const U4 r = philox4x32_10(env, counter, 0u, STREAM_MOUNTAIN_CAR << 16, k0, k1);
  const float w0 = 0.2f * u32_unit_interval(r.x);
  return MountainCarState{-0.6f + w0, 0.0f};
}

// one step with the action column's value `a` (a class index, or the force when
// `continuous`); returns done and the reward
static __host__ __device__ __forceinline__ bool mountain_car_advance(MountainCarState* s,
                                                                     float a,
                                                                     bool continuous,
                                                                     float* reward) {
#pragma clang fp contract(off)
  const float x = s->x, v = s->v;
  float ang = 3.0f * x;
  if (ang >= PENDULUM_PI) ang = ang - PENDULUM_TWO_PI;
  else if (ang < -PENDULUM_PI) ang = ang + PENDULUM_TWO_PI;
  float sn_unused, cs;
  pendulum_sincos(ang, &sn_unused, &cs);
  float dv;
  if (continuous) {
    const float u = double_pendulum_clip(a, 1.0f);
    const float f1 = u * 0.0015f;
    const float f2 = 0.0025f * cs;
    dv = f1 - f2;
  } else {
    const float f1 = three_way_push((int)a) * 0.001f;
    const float f2 = cs * -0.0025f;
    dv = f1 + f2;
  }
  const float v1 = v + dv;
  float nv = double_pendulum_clip(v1, 0.07f);
  const float x1 = x + nv;
  const float nx = x1 < -1.2f ? -1.2f : (x1 > 0.6f ? 0.6f : x1);
  if (nx == -1.2f && nv < 0.0f) nv = 0.0f;
  s->x = nx;
  s->v = nv;
  const bool done = nx >= (continuous ? 0.45f : 0.5f) && nv >= 0.0f;
  if (continuous) {
    const float a2 = a * a;
    const float cost = 0.1f * a2;
    *reward = (done ? 100.0f : 0.0f) - cost;
  } else {
    *reward = -1.0f;
  }
  return done;
}

// state [n, 2] x in [-1.2, 0.6], v in [-0.07, 0.07]; the observation is the state.
// variant 0: MountainCar-v0 (class index), 1: MountainCarContinuous-v0
struct MountainCarKind {
  using State = MountainCarState;
  static constexpr int S = 2, OBS = 2;
  static __host__ __device__ __forceinline__ State reset_draw(uint32_t k0, uint32_t k1,
                                                              uint32_t env,
                                                              uint32_t counter) {
    return mountain_car_reset_draw(k0, k1, env, counter);
  }
  static __device__ __forceinline__ void observe(const State& s, float* o) {
    o[0] = s.x; o[1] = s.v;
  }
  static __device__ __forceinline__ bool step(State* s, const float* a, int continuous,
                                              float* reward, float* o) {
    const bool done = mountain_car_advance(s, a[0], continuous != 0, reward);
    observe(*s, o);
    return done;
  }
};

// What a step of env i reads of the env's and the worker's state: loaded up front,
// so that no load waits behind the step's own stores (the memory counter retires in
// order).  `o` holds the observation entries the reward looks at when they are few.
constexpr int PRE_OBS = 8;
struct EnvPre {
  int ep, t, len, ep_t;
  float o[PRE_OBS];
  bool has_o;
};
static __device__ __forceinline__ int synth_reward_width(const SynthEnv& e) {
  return e.discrete ? e.obs_dim : min(e.act_dim, e.obs_dim);
}

// one env step: reward, step type and the (true) next observation.  `a` is the
// env's action row (any address space), `o` its observation row.
static __device__ __forceinline__ void env_core(const SynthEnv& e, int64_t i,
                                                const EnvPre& s, const float* a,
                                                const float* o, float* next_row, int64_t,
                                                float* reward, uint8_t* step_type) {
#pragma clang fp contract(off)
  const uint32_t env = (uint32_t)(e.env_id0 + i);
  const uint32_t ep = (uint32_t)s.ep;
  const int t = s.t;
  const U4 r = philox4x32_10(env, ep, (uint32_t)t, STREAM_REWARD << 16, e.k0, e.k1);
  const float noise = u32_unit_variance(r.x);
  float shaped = 0.f;
  if (e.discrete) {
    const int k = ((int)a[0]) % e.obs_dim;
    if (s.has_o) {
#pragma unroll
      for (int j = 0; j < PRE_OBS; ++j) shaped = j == k ? s.o[j] : shaped;
    } else {
      shaped = o[k];
    }
  } else {
    const int m = min(e.act_dim, e.obs_dim);
    if (s.has_o) {
#pragma unroll
      for (int j = 0; j < PRE_OBS; ++j)
        if (j < m) {
          const float aj = fminf(fmaxf(a[j], -1.f), 1.f);
          const float prod = aj * s.o[j];
          shaped = shaped + prod;
        }
    } else {
      for (int j = 0; j < m; ++j) {
        const float aj = fminf(fmaxf(a[j], -1.f), 1.f);
        const float prod = aj * o[j];
        shaped = shaped + prod;
      }
    }
  }
  const float tenth = 0.1f * shaped;
  *reward = noise + tenth;
  const int tn = t + 1;
  e.t[i] = tn;
  synth_obs(e, env, ep, (uint32_t)tn, next_row);
  // StepType.get_step_type (_dtypes.py:42-68): TIMEOUT wins over done
  uint8_t st;
  if (tn >= e.max_len) st = 3;
  else if (tn >= s.len) st = 2;
  else if (tn == 1) st = 0;
  else st = 1;
  *step_type = st;
}

// ---- NormalizedEnv observation / reward path -----------------------------------
// envs/normalized_env.py:118-132,134-164: per-env exponential moving mean and
// variance (float64 state, alpha = 0.001 by default); the mean is updated first,
// the variance uses the NEW mean, and the value is normalised with the updated
// statistics.  One thread per env; rows with mask == 0 are left untouched.
static __device__ __forceinline__ void obs_normalize_one(const float* src, float* dst,
                                                  double* m, double* v, int obs_dim,
                                                  double alpha) {
#pragma clang fp contract(off)
  for (int j = 0; j < obs_dim; ++j) {
    const double x = (double)src[j];
    const double mn = (1.0 - alpha) * m[j] + alpha * x;
    const double d = x - mn;
    const double vn = (1.0 - alpha) * v[j] + alpha * (d * d);
    m[j] = mn;
    v[j] = vn;
    dst[j] = (float)((x - mn) / (sqrt(vn) + 1e-8));
  }
}

static __device__ __forceinline__ float reward_normalize_one(float reward, double* mean,
                                                      double* var, double alpha,
                                                      double scale, int normalize) {
#pragma clang fp contract(off)
  double r = (double)reward;
  if (normalize) {  // normalized_env.py:126-132,153-164
    const double mn = (1.0 - alpha) * *mean + alpha * r;
    const double d = r - mn;
    const double vn = (1.0 - alpha) * *var + alpha * (d * d);
    *mean = mn;
    *var = vn;
    r = r / (sqrt(vn) + 1e-8);
  }
  return (float)(r * scale);
}

// ---- per-step bookkeeping (VecWorker.step_episode, vec_worker.py:176-204) ------
// (RecordParams: rollout_params.h)

// bookkeeping of env i; returns the length of the episode that ended (else 0)
static __device__ __forceinline__ int record_core(const RecordParams& p, int64_t i,
                                                  int ep_t, float reward, uint8_t st) {
  int ended_len = 0;
  {
    const int64_t cell = i * p.Tcap + p.col;
    const int t = ep_t + 1;
    // VecWorker ends an episode on any last step (vec_worker.py:198);
    // FragmentWorker only on TERMINAL (fragment_worker.py:114-115)
    const bool ended = (t >= p.max_episode_length) ||
                       (p.terminal_only ? (st == 2) : (st >= 2));
    p.rew_buf[cell] = reward;
    p.st_buf[cell] = st;
    p.tail_buf[cell] = ended ? (uint16_t)t : (uint16_t)0;
    p.done[i] = ended ? 1 : 0;
    p.ep_t[i] = ended ? 0 : t;
    if (ended) {
      ended_len = t;
      const float* o = p.next_obs + i * p.ldo;
      float* lo = p.lastobs_buf + cell * p.ldo;
      for (int j = 0; j < p.obs_dim; ++j) lo[j] = o[j];
    }
  }
  return ended_len;
}

static __device__ __forceinline__ int record_one(const RecordParams& p, int64_t i) {
  return record_core(p, i, p.ep_t[i], p.reward[i], p.step_type[i]);
}

// per-step completion counts: wave-aggregated integer atomics (deterministic:
// integer adds commute)
static __device__ __forceinline__ void record_counts(const RecordParams& p, int ended_len) {
  const uint64_t ballot = __ballot(ended_len > 0);
  int sum = ended_len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if ((threadIdx.x & 63) == 0 && ballot) {
    atomicAdd(&p.step_eps[p.col], (int)__popcll(ballot));
    atomicAdd(&p.step_samples[p.col], sum);
  }
}

// NormalizedEnv.step's action rescale of one env (envs/normalized_env.py:90-100): the
// A columns of `act` from [-scale, scale] to [lb_j, ub_j], clipped, into `out`.  fp32,
// one rounding per numpy operation (no fused multiply-add), np.clip's comparisons (a
// NaN stays a NaN).  The rescale launch and the fused rollout step both call it.
static __device__ __forceinline__ void action_rescale_row(const float* act, const float* lb,
                                                          const float* ub, float scale,
                                                          int A, float* out) {
#pragma clang fp contract(off)
  for (int j = 0; j < A; ++j) {
    const float a = act[j];
    const float lo = lb[j], hi = ub[j];
    const float slope = (0.5f * (hi - lo)) / scale;
    float v = lo + (a + scale) * slope;
    v = v < lo ? lo : (v > hi ? hi : v);
    out[j] = v;
  }
}

// env step -> (NormalizedEnv statistics + normalisation) -> bookkeeping -> reset of
// env i when it finished; returns the length of the episode that ended (else 0).
// `raw_obs` / `raw_next` are the env's own observations; seen_next is what the
// policy sees next and what is recorded as the terminal observation -- the same
// buffer as raw_next without normalisation.
// (NormParams, EnvStepArgsT<Env>: rollout_params.h)
using EnvStepArgs = EnvStepArgsT<SynthEnv>;

static __device__ __forceinline__ EnvPre env_prefetch(const EnvStepArgs& a, int64_t i) {
  EnvPre s;
  s.ep = a.e.episode[i];
  s.t = a.e.t[i];
  s.len = a.e.len[i];
  s.ep_t = a.p.ep_t[i];
  const int m = synth_reward_width(a.e);
  s.has_o = m <= PRE_OBS;
  const float* o = a.raw_obs + i * a.p.ldo;
#pragma unroll
  for (int j = 0; j < PRE_OBS; ++j) s.o[j] = (s.has_o && j < m) ? o[j] : 0.f;
  return s;
}

// the state a step of env i reads (env_prefetch adds the worker's ep_t)
static __device__ __forceinline__ EnvPre env_pre(const SynthEnv& e, int64_t i) {
  EnvPre s;
  s.ep = e.episode[i];
  s.t = e.t[i];
  s.len = e.len[i];
  s.ep_t = 0;
  s.has_o = false;  // the reward reads its observation entries from memory
  return s;
}
static __device__ __forceinline__ PointPre env_pre(const PointEnv& e, int64_t i) {
  PointPre s;
  s.px = e.point[2 * i];
  s.py = e.point[2 * i + 1];
  s.gx = e.goal[2 * i];
  s.gy = e.goal[2 * i + 1];
  s.t = e.t[i];
  s.ep_t = 0;
  return s;
}
static __device__ __forceinline__ GridPre env_pre(const GridEnv& e, int64_t i) {
  GridPre s;
  s.s = e.state[i];
  s.t = e.t[i];
  s.ep_t = 0;
  return s;
}
template <class K>
static __device__ __forceinline__ StatePre<K> env_pre(const StateEnv<K>& e, int64_t i) {
  StatePre<K> s;
  s.s = state_load<K>(e.state + K::S * i);
  s.t = e.t[i];
  s.ep_t = 0;
  return s;
}
template <class Inner>
static __device__ __forceinline__ auto env_pre(const MultiTaskEnv<Inner>& e, int64_t i) {
  MultiTaskPre<decltype(env_pre(e.in, i))> s;
  s.in = env_pre(e.in, i);
  s.task = e.last_task[i];
  s.ep_t = 0;
  return s;
}
template <class Env>
static __device__ __forceinline__ auto env_prefetch(const EnvStepArgsT<Env>& a, int64_t i) {
  auto s = env_pre(a.e, i);
  s.ep_t = a.p.ep_t[i];
  return s;
}

// `s`: env_prefetch(a, i), taken before anything of this step was stored;
// `act_row`: the env's action (a.actions + i * a.lda, or a copy on chip).  The env
// kind is the type of `a.e`: every kernel that steps envs is instantiated per kind.
template <class Env, class Pre>
static __device__ __forceinline__ int env_step_one(const EnvStepArgsT<Env>& a, int64_t i,
                                                   const Pre& s, const float* act_row) {
  const Env& e = a.e;
  const RecordParams& p = a.p;
  const NormParams& nm = a.nm;
  float rew;
  uint8_t st;
  env_core(e, i, s, act_row, a.raw_obs + i * p.ldo, a.raw_next + i * p.ldo, p.col, &rew,
           &st);
  a.step_type[i] = st;
  if (nm.norm_obs)  // normalized_env.py:134-151: statistics first, then the value
    obs_normalize_one(a.raw_next + i * p.ldo, a.seen_next + i * p.ldo,
                      nm.obs_mean + i * p.obs_dim, nm.obs_var + i * p.obs_dim, p.obs_dim,
                      nm.obs_alpha);
  if (nm.norm_reward || nm.scale_reward)
    rew = reward_normalize_one(rew, nm.rew_mean + i, nm.rew_var + i, nm.rew_alpha,
                               nm.rew_scale, nm.norm_reward);
  a.reward[i] = rew;
  const int ended_len = record_core(p, i, s.ep_t, rew, st);
  if (ended_len > 0) {
    env_reset_one(e, i, a.raw_next, p.ldo);
    if (nm.norm_obs)
      obs_normalize_one(a.raw_next + i * p.ldo, a.seen_next + i * p.ldo,
                        nm.obs_mean + i * p.obs_dim, nm.obs_var + i * p.obs_dim,
                        p.obs_dim, nm.obs_alpha);
  }
  return ended_len;
}
template <class Env>
static __device__ __forceinline__ int env_step_one(const EnvStepArgsT<Env>& a, int64_t i) {
  return env_step_one(a, i, env_prefetch(a, i), a.actions + i * a.lda);
}

}  // namespace ga_rollout

// a row of GA_STATE_ENV_KINDS (internal.h) states the observation width its kind
// description has
#define GA_STATE_ENV_WIDTH(GaEnv, KIND, DEV, WIDTH, DISCRETE) \
  static_assert(ga_rollout::DEV::OBS == WIDTH, "observation width of " #GaEnv);
GA_STATE_ENV_KINDS(GA_STATE_ENV_WIDTH)
#undef GA_STATE_ENV_WIDTH
