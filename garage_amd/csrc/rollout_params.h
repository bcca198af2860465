// What the host says to the kernels of a rollout step (rollout.hip, policy_fused.hip)
// about one launch, and the launch seam that takes it.  Host C++ only, in the style of
// fused_params.h: the host side (rollout_host.cpp) checks the C-ABI arguments, fills these
// structs and chooses the variant and the grid, the seam instantiates and launches -- so
// that the host side builds for the CPU harness under tests/host
// (rollout_host_harness.cpp) against fakes of the seam.  The device code that reads the
// structs is rollout_dev.h's; ga_key, the two key words of a seed, is the one function
// here that device code shares with the host.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "shape_rules.h"

namespace ga_rollout {

// the two Philox key words of a 64-bit seed
static __host__ __device__ __forceinline__ void ga_key(uint64_t seed, uint32_t* k0,
                                                       uint32_t* k1) {
  *k0 = (uint32_t)(seed & 0xffffffffu);
  *k1 = (uint32_t)(seed >> 32);
}

// ---- the head of a rollout step ------------------------------------------------
// What the head reads and where it writes: ga_head_args (ga_head_to_dev) without the
// per-layer path's own `head`, `A`, `log_std`, `obs_dim`.  The fused kernel's
// parameters and the per-layer head kernel's both hold one.
struct HeadDev {
  int64_t n, env_id0;
  int kind;  // 0 gaussian, 1 categorical
  int has_min, has_max;
  float min_log_std, max_log_std;
  const float* noise; int64_t ldn;  // optional [n, ldn]: N(0,1) / U(0,1) by kind
  uint32_t k0, k1, step;            // seed, global step counter (Philox counter)
  int double_softmax;
  const float* obs; int64_t ldo;    // [n, ldo] current observations
  int64_t col, Tcap;                // the rollout buffers' column of this step
  float* action; int64_t lda;       // [n, lda] actions handed to the env
  float* obs_buf; float* act_buf;   // [n, Tcap, ldo], [n, Tcap, lda]
  float* head_buf; int64_t ldh;     // optional [n, Tcap, ldh]: agent_info mean / probs
};

// the shared description of a step's head plus what only the per-layer path reads
struct HeadParams {
  HeadDev hd;
  int A;                 // action dim (gaussian) or number of classes (categorical)
  const float* head;     // [n, ldh] means or class scores
  const float* log_std;  // gaussian: device scalar
  int obs_dim;
};

// ---- the device envs (rollout_dev.h: env_pre / env_core / env_reset_one of each) ----
struct SynthEnv {
  int64_t n;
  int64_t env_id0;       // global id of env 0 of this shard
  int obs_dim, act_dim, discrete;
  int min_len, max_len;
  uint32_t k0, k1;       // seed
  int32_t* episode;      // [n] episode counter (-1 before the first reset)
  int32_t* t;            // [n] steps taken in the current episode
  int32_t* len;          // [n] length of the current episode
};

struct PointEnv {
  int64_t n;
  float arena, bonus;   // arena_size, done_bonus
  int never_done, max_len;
  float* point;         // [n, 2]
  const float* goal;    // [n, 2]
  int32_t* t;           // [n] steps taken in the current episode
  uint8_t* success;     // optional env_info 'success' at success[i * succ_ld + col]
  int64_t succ_ld;
};

template <class Inner>
struct MultiTaskEnv {
  int64_t n;
  Inner in;
  int num_tasks, strategy, one_hot;
  uint32_t k0, k1;        // seed of the uniform_random_strategy stream
  const float* payload;   // [num_tasks, ...] what env_apply_task copies from
  int32_t* last_task;     // [n] the active task (-1: no reset yet)
  uint32_t* resets;       // [n] resets so far (the random stream's counter)
  uint8_t* task_id;       // optional env_info 'task_id' at task_id[i * info_ld + col]
  int64_t info_ld;
};

struct GridEnv {
  int64_t n;
  int rows, cols, max_len;
  const uint8_t* map;    // [n, rows * cols] cell codes (F and S are GRID_FREE)
  const int32_t* start;  // [n] the S cell
  int32_t* state;        // [n] current cell
  int32_t* t;            // [n] steps taken in the current episode
};

// the seeded state-vector kinds: one frame over a kind description K, which stays
// device code (rollout_dev.h) -- no member depends on it
template <class K>
struct StateEnv {
  int64_t n;
  int64_t env_id0;   // global id of env 0 of this shard
  int max_len;
  int variant;       // the kind's own switch (MountainCar: continuous), else 0
  uint32_t k0, k1;   // seed
  float* state;      // [n, K::S]
  int32_t* t;        // [n] steps taken in the current episode
  uint32_t* resets;  // [n] resets so far (the reset stream's counter)
};
#define GA_STATE_KIND_DECL(GaEnv, KIND, DEV, OBS, DISCRETE) struct DEV;
GA_STATE_ENV_KINDS(GA_STATE_KIND_DECL)
#undef GA_STATE_KIND_DECL

// ---- per-step bookkeeping (VecWorker.step_episode, vec_worker.py:176-204) ------
struct RecordParams {
  int64_t n, col, Tcap;
  int max_episode_length;
  const float* reward;       // [n]
  const uint8_t* step_type;  // [n]
  const float* next_obs;     // [n, ldo]
  int64_t ldo;
  int obs_dim;
  int32_t* ep_t;             // [n] steps so far in the running episode
  float* rew_buf;            // [n, Tcap]
  uint8_t* st_buf;           // [n, Tcap]
  uint16_t* tail_buf;        // [n, Tcap] episode length at its last step, else 0
  float* lastobs_buf;        // [n, Tcap, ldo] written at episode ends only
  uint8_t* done;             // [n] 1 where the env must be reset
  int32_t* step_eps;         // [Tcap] episodes finished at this step
  int32_t* step_samples;     // [Tcap] their total length
  int terminal_only;         // 1: only TERMINAL (not TIMEOUT) ends an episode
};

struct NormParams {
  int norm_obs, norm_reward, scale_reward;
  double* obs_mean;   // [n, obs_dim]
  double* obs_var;
  double obs_alpha;
  double* rew_mean;   // [n]
  double* rew_var;
  double rew_alpha, rew_scale;
  // the action rescale inside the fused rollout step (null act_low: none; always null
  // for ga_env_step_record, which steps on the actions it is handed)
  const float* act_low;   // [act_dim]
  const float* act_high;
  float expected_action_scale;
  float* scaled_action;   // [n, scaled_ld] what the wrapped env steps on
  int64_t scaled_ld;
};

// env step -> (NormalizedEnv statistics + normalisation) -> bookkeeping -> reset of
// env i when it finished (rollout_dev.h: env_step_one).
// `raw_obs` / `raw_next` are the env's own observations; seen_next is what the
// policy sees next and what is recorded as the terminal observation -- the same
// buffer as raw_next without normalisation.
template <class Env>
struct EnvStepArgsT {
  Env e;
  RecordParams p;
  NormParams nm;
  const float* actions; int64_t lda;
  const float* raw_obs; float* raw_next; float* seen_next;
  float* reward; uint8_t* step_type;
};

}  // namespace ga_rollout

// ---- the fused rollout step and the training forward (policy_fused.hip) -------------
// the layers of a ga_mlp_desc
struct NetDev {
  int n_layers;
  int dims[9];
  int64_t w_off[8], b_off[8];
};

constexpr int ENV_STEP_RESCALE = 2;  // bit of FusedParams::env_step

template <class Env>
struct FusedParams {
  NetDev net;
  const float* params;
  ga_rollout::HeadDev hd;  // the step's head and rollout-buffer writes
  // env_step: the env's step, the NormalizedEnv statistics, the bookkeeping and the
  // reset of finished envs follow in the same launch, each env by the thread that
  // sampled its action (rollout_dev.h: the code of env_step_record_kernel);
  // | ENV_STEP_RESCALE: es.nm.act_low is set, the env steps on the rescaled action
  int env_step;
  ga_rollout::EnvStepArgsT<Env> es;
  // n_steps > 1 (needs env_step): the workgroup takes its envs through n_steps
  // consecutive rollout steps in this one launch -- nothing couples the envs of
  // different workgroups within a rollout -- alternating between the two
  // observation buffers (obs / es.seen_next and, with observation normalisation,
  // es.raw_obs / es.raw_next)
  int n_steps;
  // a population of parameter vectors behind one launch: workgroups
  // [m * wg_per_member, (m + 1) * wg_per_member) read member m's vector at
  // params + m * member_stride floats (one policy: stride 0, wg_per_member 1)
  int wg_per_member;
  int member_stride;
  long long* dbg;  // developer hook: phase timestamps of workgroup 0
  // GEN kernels only (behind everything the tanh kernels read): the descriptor's
  // network options -- hidden_act in network code, output_act in forward code
  int hidden_act, output_act, layer_norm;
  int64_t ln_off[8];
};

struct TrainFwdParams {
  NetDev net;
  int64_t act_off[8];
  const float* params;
  const float* X;
  int64_t ldx;
  const int32_t* idx;
  int64_t M;
  float* acts;
  float* out;
  int64_t ldo;
};

// ---- the device struct of each C-ABI env struct --------------------------------------
// the kind description of each row of GA_STATE_ENV_KINDS (internal.h)
template <class GaEnv>
struct ga_state_kind_of {};
#define GA_STATE_ENV_KIND_OF(GaEnv, KIND, DEV, WIDTH, DISCRETE) \
  template <>                                                   \
  struct ga_state_kind_of<GaEnv> {                              \
    using type = ga_rollout::DEV;                               \
  };
GA_STATE_ENV_KINDS(GA_STATE_ENV_KIND_OF)
#undef GA_STATE_ENV_KIND_OF
template <class GaEnv>
struct ga_env_dev {
  using type = ga_rollout::StateEnv<typename ga_state_kind_of<GaEnv>::type>;
};
template <> struct ga_env_dev<ga_synth_env> { using type = ga_rollout::SynthEnv; };
template <> struct ga_env_dev<ga_point_env> { using type = ga_rollout::PointEnv; };
template <> struct ga_env_dev<ga_grid_env> { using type = ga_rollout::GridEnv; };
template <> struct ga_env_dev<ga_multi_point_env> {
  using type = ga_rollout::MultiTaskEnv<ga_rollout::PointEnv>;
};
template <class GaEnv>
using ga_env_dev_t = typename ga_env_dev<GaEnv>::type;
template <class GaEnv>
using ga_env_step_args_t = ga_rollout::EnvStepArgsT<ga_env_dev_t<GaEnv>>;

// ---- the instantiation a fused step runs: the activation tiles hold layer inputs up to
// `width` (PS_HMAX or PS_WMAX), resident: the weights stay on the CU for a whole rollout
// (width PS_HMAX only), general: the descriptor names an option the tanh kernels do not
// have.  width 0: no kernel takes the network.
struct PsVariant {
  int width;
  int resident;
  int general;
};

// rollout_host.cpp: GARAGE_AMD_ROLLOUT_WIDE / GARAGE_AMD_ROLLOUT_RESIDENT, which are read
// from the environment at the first question, set by hand (the harness's A/B rows)
void ga_rollout_set_switches(int wide, int resident);

// ---- the launch seam, one function per kernel family.  Each does nothing but
// instantiate and launch `blocks` workgroups on `stream`; the per-env ones are
// instantiated for the device struct of every row of GA_ENV_KINDS (internal.h).
// rollout.hip (256 threads, one per env):
void ro_launch_head_sample(const ga_rollout::HeadParams& p, unsigned blocks,
                           hipStream_t stream);
void ro_launch_record(const ga_rollout::RecordParams& p, unsigned blocks,
                      hipStream_t stream);
template <class Env>
void ro_launch_env_reset(const Env& e, const uint8_t* mask, float* obs, int64_t ldo,
                         unsigned blocks, hipStream_t stream);
template <class Env>
void ro_launch_env_step(const Env& e, const float* actions, int64_t lda, const float* obs,
                        float* next_obs, int64_t ldo, float* reward, uint8_t* step_type,
                        unsigned blocks, hipStream_t stream);
template <class Env>
void ro_launch_env_step_record(const ga_rollout::EnvStepArgsT<Env>& a, unsigned blocks,
                               hipStream_t stream);
// policy_fused.hip (256 threads per PS_ROWS envs; 512 per PS_TRAIN_ROWS rows):
template <class Env>
void ps_launch_policy_step(const FusedParams<Env>& p, PsVariant v, unsigned blocks,
                           hipStream_t stream);
void ps_launch_train_forward(const TrainFwdParams& p, unsigned blocks, hipStream_t stream);
