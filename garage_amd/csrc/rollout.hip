// Rollout-side kernels: the per-layer path's action head, the device environments
// (synthetic, PointEnv, GridWorldEnv, MultiEnvWrapper over PointEnv, CartPole,
// Pendulum, the inverted double pendulum, Acrobot, MountainCar), per-step
// episode bookkeeping and the ragged -> packed compaction.  A step's device code is
// rollout_dev.h's and its host side rollout_host.cpp's; here are its kernels behind the
// launch seam of rollout_params.h.
//
// Together they replace the Python per-env loop of VecWorker.step_episode /
// _gather_episode / collect_episode (sampler/vec_worker.py:139-219) and
// StochasticPolicy.get_actions' dist.sample() (torch/policies/stochastic_policy.py:
// 46-89).  Rollout buffers are env-major (n_envs, Tcap[, width]) in HBM; one
// thread owns one env (its row tails are 16-B friendly: widths are padded to 4).
#include "common.h"

#include "rollout_dev.h"

namespace {
using namespace ga_rollout;

// reset / step of a batch of any env kind (rollout_dev.h)
template <class Env>
__global__ __launch_bounds__(256) void env_reset_kernel(Env e, const uint8_t* mask,
                                                        float* obs, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= e.n) return;
  if (mask && !mask[i]) return;
  env_reset_one(e, i, obs, ldo);
}

// `obs`: the current observations, read by the synthetic env only (the others keep
// their state themselves)
template <class Env>
__global__ __launch_bounds__(256) void env_step_kernel(Env e, const float* actions,
                                                       int64_t lda, const float* obs,
                                                       float* next_obs, int64_t ldo,
                                                       float* reward, uint8_t* step_type) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= e.n) return;
  float rew;
  uint8_t st;
  env_core(e, i, env_pre(e, i), actions + i * lda, obs + i * ldo, next_obs + i * ldo, 0,
           &rew, &st);
  reward[i] = rew;
  step_type[i] = st;
}

// src == dst normalises in place; otherwise the raw rows stay untouched (the
// wrapped env keeps its own, un-normalised, state)
__global__ __launch_bounds__(256) void obs_normalize_kernel(
    int64_t n, int obs_dim, const float* src, float* dst, int64_t ldo, double* mean,
    double* var, double alpha, const uint8_t* mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (mask && !mask[i]) return;
  obs_normalize_one(src + i * ldo, dst + i * ldo, mean + i * obs_dim,
                    var + i * obs_dim, obs_dim, alpha);
}

__global__ __launch_bounds__(256) void reward_normalize_kernel(
    int64_t n, float* reward, double* mean, double* var, double alpha, double scale,
    int normalize) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  reward[i] = reward_normalize_one(reward[i], normalize ? mean + i : nullptr,
                                   normalize ? var + i : nullptr, alpha, scale,
                                   normalize);
}

// ---- action head ---------------------------------------------------------------
// (HeadParams: rollout_params.h)
// The step's observations into the rollout buffer (the list append of
// vec_worker.py:188), by the whole workgroup: consecutive threads copy consecutive
// columns of a row.  (One thread per env copying its own row -- obs_dim strided
// scalar loads and stores per thread -- cost 156 us per step at C5's 8192 x 376.)
__device__ __forceinline__ void copy_obs_rows(const HeadParams& p) {
  const int64_t env0 = (int64_t)blockIdx.x * 256;
  const int64_t rows = min((int64_t)256, p.hd.n - env0);
  const int64_t total = rows * p.obs_dim;
  for (int64_t e = threadIdx.x; e < total; e += 256) {
    const int64_t env = env0 + e / p.obs_dim;
    const int j = (int)(e % p.obs_dim);
    p.hd.obs_buf[(env * p.hd.Tcap + p.hd.col) * p.hd.ldo + j] = p.hd.obs[env * p.hd.ldo + j];
  }
}

// one thread per env; hd.kind is wave-uniform
__global__ __launch_bounds__(256) void head_sample_kernel(HeadParams p) {
  copy_obs_rows(p);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.hd.n) return;
  head_one(p.hd, p.head + i * p.hd.ldh, p.A, p.log_std, i);
}

__global__ __launch_bounds__(256) void record_step_kernel(RecordParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  record_counts(p, i < p.n ? record_one(p, i) : 0);
}

// env step -> (NormalizedEnv statistics + normalisation) -> bookkeeping -> reset
// of the envs that finished, one thread per env and one launch (every stage only
// touches env i's own state).  `raw_obs` / `raw_next` are the env's own
// observations; p.next_obs is what the policy sees next and what is recorded as
// the terminal observation -- the same buffer as raw_next without normalisation.
// One instantiation per env kind (the type of a.e).
template <class Env>
__global__ __launch_bounds__(256) void env_step_record_kernel(EnvStepArgsT<Env> a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  record_counts(a.p, i < a.e.n ? env_step_one(a, i) : 0);
}

// ---- ragged -> packed ------------------------------------------------------------
// Episodes in batch order = (completion step, env index).
// One block per completion step t <= t_star ranks the envs that ended there.
__global__ __launch_bounds__(256) void pack_episodes_kernel(
    const uint16_t* tail_buf, int64_t n, int64_t Tcap, const int32_t* ep_base,
    int32_t* ep_env, int32_t* ep_end, int32_t* ep_len) {
  __shared__ int wave_cnt[4];
  __shared__ int running;
  const int t = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) running = ep_base[t];
  __syncthreads();
  for (int64_t i0 = 0; i0 < n; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const int L = (i < n) ? (int)tail_buf[i * Tcap + t] : 0;
    const uint64_t ballot = __ballot(L > 0);
    const int before = (int)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[w] = (int)__popcll(ballot);
    __syncthreads();
    int base = running;
    for (int k = 0; k < w; ++k) base += wave_cnt[k];
    if (L > 0) {
      const int e = base + before;
      ep_env[e] = (int)i;
      ep_end[e] = t;
      ep_len[e] = L;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
}

// src[off[e] + j] = env * Tcap + (end - len + 1 + j): flat cell of packed sample.
__global__ __launch_bounds__(256) void pack_src_index_kernel(
    const int32_t* ep_env, const int32_t* ep_end, const int32_t* ep_len,
    const int64_t* ep_off, int64_t n_eps, int64_t Tcap, int32_t* src) {
  const int64_t e = blockIdx.x;
  if (e >= n_eps) return;
  const int L = ep_len[e];
  const int64_t first = (int64_t)ep_env[e] * Tcap + (ep_end[e] - L + 1);
  const int64_t off = ep_off[e];
  for (int j = threadIdx.x; j < L; j += 256) src[off + j] = (int32_t)(first + j);
}

// dst[i, 0:width] = src[idx[i], 0:width]  (width multiple of 4, 16-B vectors)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* src,
                                                          int64_t lds_,
                                                          const int32_t* idx,
                                                          int64_t rows, int width4,
                                                          float* dst, int64_t ldd) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = g / width4;
  const int v = (int)(g % width4);
  if (row >= rows) return;
  const int64_t s = idx[row];
  const float4 x = *reinterpret_cast<const float4*>(src + s * lds_ + 4 * v);
  *reinterpret_cast<float4*>(dst + row * ldd + 4 * v) = x;
}

template <typename T>
__global__ __launch_bounds__(256) void gather_scalar_kernel(const T* src,
                                                            const int32_t* idx,
                                                            int64_t n, T* dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}

// per-episode undiscounted reward sums (log_performance, _functions.py:233-275)
__global__ __launch_bounds__(256) void episode_sums_kernel(const float* rewards,
                                                           const int64_t* ep_off,
                                                           int64_t n_eps,
                                                           double* sums) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_eps) return;
  double acc = 0.0;
  for (int64_t j = ep_off[e]; j < ep_off[e + 1]; ++j) acc += (double)rewards[j];
  sums[e] = acc;
}

// ---- a population's score straight from the rollout buffers ---------------------
// Member m owns the rows [m g, (m + 1) g).  What log_performance
// (_functions.py:233-275) reduces an episode to is computed where the episode lies:
// nothing is packed or gathered.

// Inclusive sums of (a, b) over the block's 256 threads; *ta / *tb: the block's totals.
__device__ __forceinline__ void block_scan2_256(int& a, int& b, int (*smem)[2], int* ta,
                                                int* tb) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ua = __shfl_up(a, o, 64), ub = __shfl_up(b, o, 64);
    if (lane >= o) { a += ua; b += ub; }
  }
  if (lane == 63) { smem[w][0] = a; smem[w][1] = b; }
  __syncthreads();
  int sa = 0, sb = 0;
  for (int k = 0; k < w; ++k) { sa += smem[k][0]; sb += smem[k][1]; }
  *ta = smem[0][0] + smem[1][0] + smem[2][0] + smem[3][0];
  *tb = smem[0][1] + smem[1][1] + smem[2][1] + smem[3][1];
  a += sa; b += sb;
  __syncthreads();
}

// One block per member, one thread per column (consecutive threads read consecutive
// cells of a row).  progress[3 m ..] = {c_m, episodes, samples}: c_m the first column
// count at which the member's completed episodes hold >= num_samples steps (0: not
// within n_cols), the episodes that ended in [0, c_m) (in [0, n_cols) while c_m == 0)
// and the steps of all episodes completed in [0, n_cols).  col_base[m Tcap + t]: the
// member's episodes that ended before column t.
__global__ __launch_bounds__(256) void member_progress_kernel(
    const uint16_t* tail, int64_t g, int64_t Tcap, int n_cols, int num_samples,
    int32_t* progress, int32_t* col_base) {
  __shared__ int part[4][2];
  __shared__ int found[2];
  const int m = blockIdx.x;
  const uint16_t* rows = tail + (int64_t)m * g * Tcap;
  if (threadIdx.x == 0) found[0] = 0;
  __syncthreads();
  int carry_s = 0, carry_e = 0;
  for (int t0 = 0; t0 < n_cols; t0 += 256) {
    const int t = t0 + (int)threadIdx.x;
    int s = 0, e = 0;
    if (t < n_cols)
      for (int64_t i = 0; i < g; ++i) {
        const int L = (int)rows[i * Tcap + t];
        s += L;
        e += L > 0;
      }
    int cs = s, ce = e, ts, te;
    block_scan2_256(cs, ce, part, &ts, &te);
    cs += carry_s;
    ce += carry_e;
    if (t < n_cols) {
      col_base[(int64_t)m * Tcap + t] = ce - e;
      // the crossing: samples never decrease, so exactly one column sees it
      if (cs >= num_samples && cs - s < num_samples) {
        found[0] = t + 1;
        found[1] = ce;
      }
    }
    carry_s += ts;
    carry_e += te;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    progress[3 * m + 0] = found[0];
    progress[3 * m + 1] = found[0] ? found[1] : carry_e;
    progress[3 * m + 2] = carry_s;
  }
}

// The first element of discount_cumsum in the host's own arithmetic
// (functions.log_performance_host): ret = r_t + discount * ret from the last step
// back, product and sum rounded once each.  Plain operators with contraction switched
// off (as ga_adam_update): HIP's __dmul_rn / __dadd_rn are plain operators inside a
// header compiled with contraction on, and came out as one v_fmac_f64 here.
__device__ __forceinline__ double first_discounted_return(const float* r, int L,
                                                          double discount) {
#pragma clang fp contract(off)
  double ret = 0.0;
  for (int j = L - 1; j >= 0; --j) {
    const double carried = discount * ret;
    ret = (double)r[j] + carried;
  }
  return ret;
}

struct EpisodeStatsOut {
  int32_t* length;
  double* undiscounted;
  double* discounted;
  uint8_t* terminated;
  uint8_t* success;  // written only with a success plane
};

// One block per (column t, member m): the envs whose episode ended at t, ranked by env
// index 256 at a time as pack_episodes_kernel ranks them; the thread of such an env
// walks its own episode.  Episode e of the output = (episodes of the members before m
// that reached their target) + col_base[m, t] + rank.
__global__ __launch_bounds__(256) void member_episode_stats_kernel(
    const float* rew, const uint8_t* st, const uint16_t* tail, const uint8_t* success,
    int64_t g, int64_t Tcap, const int32_t* progress, const int32_t* col_base,
    double discount, int64_t max_eps, EpisodeStatsOut out) {
  __shared__ int wave_cnt[4];
  __shared__ int before_members[4];
  const int t = blockIdx.x, m = blockIdx.y;
  if (t >= progress[3 * m]) return;  // (block-uniform) at or after c_m: left out
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int mine = 0;
  for (int k = threadIdx.x; k < m; k += 256)
    if (progress[3 * k]) mine += progress[3 * k + 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if (lane == 0) before_members[w] = mine;
  __syncthreads();
  int64_t running = (int64_t)before_members[0] + before_members[1] + before_members[2] +
                    before_members[3] + col_base[(int64_t)m * Tcap + t];
  for (int64_t i0 = 0; i0 < g; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const int64_t row = (int64_t)m * g + i;
    int L = (i < g) ? (int)tail[row * Tcap + t] : 0;
    if (L > t + 1) L = t + 1;  // (an episode cannot be longer than the columns behind it)
    const uint64_t ballot = __ballot(L > 0);
    const int before = (int)__popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[w] = (int)__popcll(ballot);
    __syncthreads();
    int64_t e = running + before;
    for (int k = 0; k < w; ++k) e += wave_cnt[k];
    running += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
    if (L > 0 && e < max_eps) {
      const int64_t first = row * Tcap + (t - L + 1);
      const float* r = rew + first;
      // episode_sums_kernel's sum: in time order, fp64
      double acc = 0.0;
      for (int j = 0; j < L; ++j) acc += (double)r[j];
      const double ret = first_discounted_return(r, L, discount);
      int term = 0, succ = 0;
      for (int j = 0; j < L; ++j) term |= st[first + j] == 2;  // StepType.TERMINAL
      if (success)
        for (int j = 0; j < L; ++j) succ |= success[first + j] != 0;
      out.length[e] = L;
      out.undiscounted[e] = acc;
      out.discounted[e] = ret;
      out.terminated[e] = (uint8_t)term;
      if (success) out.success[e] = (uint8_t)succ;
    }
  }
}


// ---- keyed pseudo-random permutation of [0, n) --------------------------------
// BatchDataset (np/optimizers/minibatch_dataset.py:4-35) shuffles ids on the host
// with the global numpy RNG; the throughput mode replaces that by a 4-round
// Feistel network over 2h bits with cycle walking: out[i] = PRP_key(i), computed
// independently per element (no sort, no host round trip).
__device__ __forceinline__ uint32_t feistel_f(uint32_t x, uint32_t k) {
  x ^= k;
  x *= 0x9E3779B1u; x ^= x >> 15;
  x *= 0x85EBCA77u; x ^= x >> 13;
  x *= 0xC2B2AE3Du; x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(256) void feistel_perm_kernel(int64_t n, int half_bits,
                                                           uint32_t k0, uint32_t k1,
                                                           int32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t mask = (1u << half_bits) - 1u;
  uint32_t x = (uint32_t)i;
  do {
    uint32_t L = x >> half_bits, R = x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t t = L ^ (feistel_f(R, k0 + 0x9E3779B9u * r + (k1 ^ r)) & mask);
      L = R;
      R = t;
    }
    x = (L << half_bits) | R;
  } while ((int64_t)x >= n);
  out[i] = (int32_t)x;
}

}  // namespace

// ---------------------------------------------------------------------------
// The launch seam of a rollout step (rollout_params.h): instantiate and launch, nothing
// else.  The checks, the conversions of the C-ABI structs and the grids are
// rollout_host.cpp's.
// ---------------------------------------------------------------------------
void ro_launch_head_sample(const HeadParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(head_sample_kernel, dim3(blocks), dim3(256), 0, stream, p);
}

void ro_launch_record(const RecordParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(record_step_kernel, dim3(blocks), dim3(256), 0, stream, p);
}

template <class Env>
void ro_launch_env_reset(const Env& e, const uint8_t* mask, float* obs, int64_t ldo,
                         unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(env_reset_kernel<Env>, dim3(blocks), dim3(256), 0, stream, e, mask,
                     obs, ldo);
}

template <class Env>
void ro_launch_env_step(const Env& e, const float* actions, int64_t lda, const float* obs,
                        float* next_obs, int64_t ldo, float* reward, uint8_t* step_type,
                        unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(env_step_kernel<Env>, dim3(blocks), dim3(256), 0, stream, e, actions,
                     lda, obs, next_obs, ldo, reward, step_type);
}

template <class Env>
void ro_launch_env_step_record(const EnvStepArgsT<Env>& a, unsigned blocks,
                               hipStream_t stream) {
  hipLaunchKernelGGL(env_step_record_kernel<Env>, dim3(blocks), dim3(256), 0, stream, a);
}

#define GA_ENV_SEAM_OF(GaEnv, ...)                                                        \
  template void ro_launch_env_reset(const ga_env_dev_t<GaEnv>&, const uint8_t*, float*,   \
                                    int64_t, unsigned, hipStream_t);                      \
  template void ro_launch_env_step(const ga_env_dev_t<GaEnv>&, const float*, int64_t,     \
                                   const float*, float*, int64_t, float*, uint8_t*,       \
                                   unsigned, hipStream_t);                                \
  template void ro_launch_env_step_record(const ga_env_step_args_t<GaEnv>&, unsigned,     \
                                          hipStream_t);
GA_ENV_KINDS(GA_ENV_SEAM_OF)
#undef GA_ENV_SEAM_OF

// ---------------------------------------------------------------------------
// C ABI (see include/garage_amd.h): the entry points that are one kernel each, and the
// host twins of the device's draws
// ---------------------------------------------------------------------------
// the device's task_draw on the host (tests compare it with a numpy restatement)
extern "C" int ga_multi_env_task_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                      int num_tasks) {
  GA_REQUIRE(num_tasks >= 1 && num_tasks <= 256,
             "ga_multi_env_task_draw: num_tasks must be in 1..256 (got %d)", num_tasks);
  uint32_t k0, k1;
  ga_key(seed, &k0, &k1);
  return task_draw(k0, k1, (uint32_t)env_id, counter, num_tasks);
}

// The device's reset draws on the host: the state reset number `counter` gives env
// `env_id` of kind K (tests compare them with a pure-Python Philox; the host twins of
// garage_amd.envs start their episodes from them)
template <class K>
static int state_reset_draw(const char* who, uint64_t seed, int64_t env_id,
                            uint32_t counter, float* out) {
  GA_REQUIRE(out, "%s: null pointer", who);
  uint32_t k0, k1;
  ga_key(seed, &k0, &k1);
  state_store<K>(K::reset_draw(k0, k1, (uint32_t)env_id, counter), out);
  return GA_OK;
}

extern "C" int ga_cartpole_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                      float out4[4]) {
  return state_reset_draw<CartPoleKind>("ga_cartpole_reset_draw", seed, env_id, counter,
                                        out4);
}

extern "C" int ga_pendulum_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                      float out2[2]) {
  return state_reset_draw<PendulumKind>("ga_pendulum_reset_draw", seed, env_id, counter,
                                        out2);
}

extern "C" int ga_double_pendulum_reset_draw(uint64_t seed, int64_t env_id,
                                             uint32_t counter, float out6[6]) {
  return state_reset_draw<DoublePendulumKind>("ga_double_pendulum_reset_draw", seed,
                                              env_id, counter, out6);
}

extern "C" int ga_acrobot_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                     float out4[4]) {
  return state_reset_draw<AcrobotKind>("ga_acrobot_reset_draw", seed, env_id, counter,
                                       out4);
}

extern "C" int ga_mountain_car_reset_draw(uint64_t seed, int64_t env_id, uint32_t counter,
                                          float out2[2]) {
  return state_reset_draw<MountainCarKind>("ga_mountain_car_reset_draw", seed, env_id,
                                           counter, out2);
}

extern "C" int ga_pack_episodes(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                                int64_t n_steps, const int32_t* ep_base,
                                int32_t* ep_env, int32_t* ep_end, int32_t* ep_len,
                                ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(tail_buf && ep_base && ep_env && ep_end && ep_len,
             "ga_pack_episodes: null pointer");
  GA_REQUIRE(n > 0 && n_steps > 0 && n_steps <= Tcap, "ga_pack_episodes: bad sizes");
  hipLaunchKernelGGL(pack_episodes_kernel, dim3((unsigned)n_steps), dim3(256), 0,
                     stream, tail_buf, n, Tcap, ep_base, ep_env, ep_end, ep_len);
  GA_CHECK_LAUNCH("pack_episodes");
  return GA_OK;
}

extern "C" int ga_pack_src_index(const int32_t* ep_env, const int32_t* ep_end,
                                 const int32_t* ep_len, const int64_t* ep_off,
                                 int64_t n_eps, int64_t Tcap, int32_t* src,
                                 ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(ep_env && ep_end && ep_len && ep_off && src,
             "ga_pack_src_index: null pointer");
  GA_REQUIRE(n_eps > 0 && n_eps < (1ll << 31), "ga_pack_src_index: bad n_eps");
  // (src holds int32 cells: the caller guarantees n * Tcap < 2^31 for its n envs, of
  // which only Tcap and the episodes -- one cell each at the least -- are seen here)
  GA_REQUIRE(Tcap > 0 && Tcap < (1ll << 31),
             "ga_pack_src_index: rollout buffers too large (Tcap %lld: cells are "
             "addressed in int32)", (long long)Tcap);
  hipLaunchKernelGGL(pack_src_index_kernel, dim3((unsigned)n_eps), dim3(256), 0,
                     stream, ep_env, ep_end, ep_len, ep_off, n_eps, Tcap, src);
  GA_CHECK_LAUNCH("pack_src_index");
  return GA_OK;
}

extern "C" int ga_gather_rows_f32(const float* src, int64_t ld_src,
                                  const int32_t* idx, int64_t rows, int64_t width,
                                  float* dst, int64_t ld_dst, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(src && idx && dst, "ga_gather_rows_f32: null pointer");
  GA_REQUIRE(rows > 0 && width > 0 && width % 4 == 0 && ld_src % 4 == 0 &&
                 ld_dst % 4 == 0 && ld_src >= width && ld_dst >= width,
             "ga_gather_rows_f32: widths / strides must be multiples of 4");
  GA_REQUIRE(ga_aligned16(src) && ga_aligned16(dst),
             "ga_gather_rows_f32: 16-B alignment required");
  const int w4 = (int)(width / 4);
  hipLaunchKernelGGL(gather_rows_kernel,
                     dim3((unsigned)ga_ceil_div(rows * w4, 256)), dim3(256), 0, stream,
                     src, ld_src, idx, rows, w4, dst, ld_dst);
  GA_CHECK_LAUNCH("gather_rows");
  return GA_OK;
}

extern "C" int ga_gather_f32(const float* src, const int32_t* idx, int64_t n,
                             float* dst, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(src && idx && dst && n > 0, "ga_gather_f32: bad arguments");
  hipLaunchKernelGGL(gather_scalar_kernel<float>,
                     dim3((unsigned)ga_ceil_div(n, 256)), dim3(256), 0, stream, src,
                     idx, n, dst);
  GA_CHECK_LAUNCH("gather_f32");
  return GA_OK;
}

extern "C" int ga_gather_u8(const uint8_t* src, const int32_t* idx, int64_t n,
                            uint8_t* dst, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(src && idx && dst && n > 0, "ga_gather_u8: bad arguments");
  hipLaunchKernelGGL(gather_scalar_kernel<uint8_t>,
                     dim3((unsigned)ga_ceil_div(n, 256)), dim3(256), 0, stream, src,
                     idx, n, dst);
  GA_CHECK_LAUNCH("gather_u8");
  return GA_OK;
}

extern "C" int ga_episode_sums_f32(const float* rewards, const int64_t* ep_off,
                                   int64_t n_eps, double* sums, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(rewards && ep_off && sums && n_eps > 0, "ga_episode_sums_f32: bad args");
  hipLaunchKernelGGL(episode_sums_kernel, dim3((unsigned)ga_ceil_div(n_eps, 256)),
                     dim3(256), 0, stream, rewards, ep_off, n_eps, sums);
  GA_CHECK_LAUNCH("episode_sums");
  return GA_OK;
}

// what both population-score entries check before any launch
static int check_member_args(const char* who, int64_t n, int64_t Tcap, int64_t n_cols,
                             int64_t n_members, int64_t num_samples) {
  GA_REQUIRE(n_members >= 1, "%s: n_members must be at least 1 (got %lld)", who,
             (long long)n_members);
  GA_REQUIRE(n > 0 && n % n_members == 0, "%s: %lld envs do not split into %lld members",
             who, (long long)n, (long long)n_members);
  GA_REQUIRE(n_cols >= 1 && n_cols <= Tcap,
             "%s: n_cols must be in 1..Tcap (got %lld, Tcap %lld)", who, (long long)n_cols,
             (long long)Tcap);
  GA_REQUIRE(num_samples >= 1 && num_samples < (1ll << 31),
             "%s: num_samples must be at least 1 (got %lld)", who, (long long)num_samples);
  // (cells are counted in int32, as ga_pack_src_index addresses them)
  GA_REQUIRE(n * Tcap < (1ll << 31) && n_members < (1ll << 16),
             "%s: rollout buffers too large (%lld x %lld cells, %lld members)", who,
             (long long)n, (long long)Tcap, (long long)n_members);
  return GA_OK;
}

extern "C" int ga_member_progress(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                                  int64_t n_cols, int64_t n_members, int64_t num_samples,
                                  int32_t* progress, int32_t* col_base,
                                  ga_stream_t stream) {
  const char* who = "ga_member_progress";
  GA_REQUIRE(tail_buf && progress && col_base, "%s: null pointer", who);
  int rc = check_member_args(who, n, Tcap, n_cols, n_members, num_samples);
  if (rc) return rc;
  hipLaunchKernelGGL(member_progress_kernel, dim3((unsigned)n_members), dim3(256), 0,
                     (hipStream_t)stream, tail_buf, n / n_members, Tcap, (int)n_cols,
                     (int)num_samples, progress, col_base);
  GA_CHECK_LAUNCH("member_progress");
  return GA_OK;
}

extern "C" int ga_member_episode_statistics(
    const float* rew_buf, const uint8_t* st_buf, const uint16_t* tail_buf,
    const uint8_t* success_buf, int64_t n, int64_t Tcap, int64_t n_cols,
    int64_t n_members, int64_t num_samples, double discount, int32_t* progress,
    int32_t* col_base, int64_t max_eps, int32_t* length, double* undiscounted,
    double* discounted, uint8_t* terminated, uint8_t* success, ga_stream_t stream) {
  const char* who = "ga_member_episode_statistics";
  GA_REQUIRE(rew_buf && st_buf && tail_buf && progress && col_base && length &&
                 undiscounted && discounted && terminated && (success || !success_buf),
             "%s: null pointer", who);
  int rc = check_member_args(who, n, Tcap, n_cols, n_members, num_samples);
  if (rc) return rc;
  GA_REQUIRE(max_eps >= 1, "%s: max_eps must be at least 1 (got %lld)", who,
             (long long)max_eps);
  const int64_t g = n / n_members;
  hipLaunchKernelGGL(member_progress_kernel, dim3((unsigned)n_members), dim3(256), 0,
                     (hipStream_t)stream, tail_buf, g, Tcap, (int)n_cols,
                     (int)num_samples, progress, col_base);
  GA_CHECK_LAUNCH("member_progress");
  EpisodeStatsOut out{length, undiscounted, discounted, terminated, success};
  hipLaunchKernelGGL(member_episode_stats_kernel,
                     dim3((unsigned)n_cols, (unsigned)n_members), dim3(256), 0,
                     (hipStream_t)stream, rew_buf, st_buf, tail_buf, success_buf, g, Tcap,
                     progress, col_base, discount, max_eps, out);
  GA_CHECK_LAUNCH("member_episode_stats");
  return GA_OK;
}

extern "C" int ga_permutation_i32(int64_t n, uint64_t key, int32_t* out,
                                  ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(out && n > 0 && n < (1ll << 30), "ga_permutation_i32: bad arguments");
  int half_bits = 1;
  while ((1ll << (2 * half_bits)) < n) ++half_bits;
  uint32_t k0, k1;
  ga_key(key, &k0, &k1);
  hipLaunchKernelGGL(feistel_perm_kernel, dim3((unsigned)ga_ceil_div(n, 256)),
                     dim3(256), 0, stream, n, half_bits, k0, k1, out);
  GA_CHECK_LAUNCH("feistel_perm");
  return GA_OK;
}

extern "C" int ga_obs_normalize_from_f64(int64_t n, int obs_dim, const float* src,
                                         float* dst, int64_t ldo, double* mean,
                                         double* var, double alpha,
                                         const uint8_t* mask, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(src && dst && mean && var, "ga_obs_normalize_from_f64: null pointer");
  GA_REQUIRE(n > 0 && obs_dim > 0 && ldo >= obs_dim,
             "ga_obs_normalize_from_f64: bad sizes");
  hipLaunchKernelGGL(obs_normalize_kernel, dim3((unsigned)ga_ceil_div(n, 256)),
                     dim3(256), 0, stream, n, obs_dim, src, dst, ldo, mean, var, alpha,
                     mask);
  GA_CHECK_LAUNCH("obs_normalize");
  return GA_OK;
}

extern "C" int ga_obs_normalize_f64(int64_t n, int obs_dim, float* obs, int64_t ldo,
                                    double* mean, double* var, double alpha,
                                    const uint8_t* mask, ga_stream_t stream) {
  return ga_obs_normalize_from_f64(n, obs_dim, obs, obs, ldo, mean, var, alpha, mask,
                                   stream);
}

namespace {
// NormalizedEnv.step's action rescale (envs/normalized_env.py:90-100) as a launch of
// its own: one thread per env runs rollout_dev.h's action_rescale_row
__global__ __launch_bounds__(256) void action_rescale_kernel(
    int64_t n, int A, const float* __restrict__ act, int64_t lda,
    const float* __restrict__ lb, const float* __restrict__ ub, float scale,
    float* __restrict__ out, int64_t ldo) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  action_rescale_row(act + r * lda, lb, ub, scale, A, out + r * ldo);
}
}  // namespace

extern "C" int ga_action_rescale_f32(int64_t n, int A, const float* actions, int64_t lda,
                                     const float* low, const float* high,
                                     float expected_action_scale, float* out,
                                     int64_t ldo, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(actions && low && high && out, "ga_action_rescale_f32: null pointer");
  GA_REQUIRE(n > 0 && A > 0 && lda >= A && ldo >= A, "ga_action_rescale_f32: bad sizes");
  hipLaunchKernelGGL(action_rescale_kernel, dim3((unsigned)ga_ceil_div(n, 256)),
                     dim3(256), 0, stream, n, A, actions, lda, low, high,
                     expected_action_scale, out, ldo);
  GA_CHECK_LAUNCH("action_rescale");
  return GA_OK;
}

extern "C" int ga_reward_normalize_f64(int64_t n, float* reward, double* mean,
                                       double* var, double alpha, double scale,
                                       int normalize, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(reward && (!normalize || (mean && var)),
             "ga_reward_normalize_f64: null pointer");
  GA_REQUIRE(n > 0, "ga_reward_normalize_f64: bad size");
  hipLaunchKernelGGL(reward_normalize_kernel, dim3((unsigned)ga_ceil_div(n, 256)),
                     dim3(256), 0, stream, n, reward, mean, var, alpha, scale,
                     normalize);
  GA_CHECK_LAUNCH("reward_normalize");
  return GA_OK;
}
