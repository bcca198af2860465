// Rollout-side kernels: the per-layer path's action head, the device environments
// (synthetic, PointEnv, GridWorldEnv, MultiEnvWrapper over PointEnv, CartPole,
// Pendulum, the inverted double pendulum, Acrobot, MountainCar), per-step
// episode bookkeeping and the ragged -> packed compaction.  A step's device code is
// rollout_dev.h's; here are its kernels and the one converter and check of each C-ABI
// struct: ga_head_to_dev, ga_record_to_dev / check_record, ga_env_to_dev / check_env.
//
// Together they replace the Python per-env loop of VecWorker.step_episode /
// _gather_episode / collect_episode (sampler/vec_worker.py:139-219) and
// StochasticPolicy.get_actions' dist.sample() (torch/policies/stochastic_policy.py:
// 46-89).  Rollout buffers are env-major (n_envs, Tcap[, width]) in HBM; one
// thread owns one env (its row tails are 16-B friendly: widths are padded to 4).
#include <type_traits>

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
// the shared description of a step's head plus what only the per-layer path reads
struct HeadParams {
  HeadDev hd;
  int A;                 // action dim (gaussian) or number of classes (categorical)
  const float* head;     // [n, ldh] means or class scores
  const float* log_std;  // gaussian: device scalar
  int obs_dim;
};

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
// C ABI (see include/garage_amd.h)
// ---------------------------------------------------------------------------
// the kernel-side head of a step (rollout_dev.h)
HeadDev ga_head_to_dev(const ga_head_args* a) {
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

extern "C" int ga_policy_head_sample(const ga_head_args* a, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(a && a->head && a->obs && a->action && a->obs_buf && a->act_buf,
             "ga_policy_head_sample: null pointer");
  GA_REQUIRE(a->n > 0 && a->A > 0 && a->ldh >= a->A && a->ldo >= a->obs_dim,
             "ga_policy_head_sample: bad sizes");
  GA_REQUIRE(a->col >= 0 && a->col < a->Tcap, "ga_policy_head_sample: col %lld out of "
             "range (Tcap %lld)", (long long)a->col, (long long)a->Tcap);
  GA_REQUIRE(a->kind == 1 || (a->log_std && a->lda >= a->A),
             "ga_policy_head_sample: gaussian head needs log_std and lda >= A");
  const HeadParams p = {ga_head_to_dev(a), a->A, a->head, a->log_std, a->obs_dim};
  hipLaunchKernelGGL(head_sample_kernel, dim3((unsigned)ga_ceil_div(a->n, 256)),
                     dim3(256), 0, stream, p);
  GA_CHECK_LAUNCH("policy_head_sample");
  return GA_OK;
}

extern "C" int ga_record_step(const ga_record_args* a, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "ga_record_step";
  GA_REQUIRE(a, "%s: null pointer", who);
  int rc = check_record(a, a->n, who);
  if (rc) return rc;
  const RecordParams p = ga_record_to_dev(a);
  hipLaunchKernelGGL(record_step_kernel, dim3((unsigned)ga_ceil_div(a->n, 256)),
                     dim3(256), 0, stream, p);
  GA_CHECK_LAUNCH("record_step");
  return GA_OK;
}

// ---- the device envs ---------------------------------------------------------------
// the kernel-side struct of each C-ABI env (rollout_dev.h)
SynthEnv ga_env_to_dev(const ga_synth_env* e, int64_t) {
  SynthEnv d;
  d.n = e->n; d.env_id0 = e->env_id0; d.obs_dim = e->obs_dim; d.act_dim = e->act_dim;
  d.discrete = e->discrete; d.min_len = e->min_len; d.max_len = e->max_len;
  ga_key(e->seed, &d.k0, &d.k1);
  d.episode = e->episode; d.t = e->t; d.len = e->len;
  return d;
}

PointEnv ga_env_to_dev(const ga_point_env* e, int64_t succ_ld) {
  PointEnv d;
  d.n = e->n; d.arena = e->arena_size; d.bonus = e->done_bonus;
  d.never_done = e->never_done; d.max_len = e->max_episode_length;
  d.point = e->point; d.goal = e->goal; d.t = e->t; d.success = e->success;
  d.succ_ld = succ_ld;
  return d;
}

GridEnv ga_env_to_dev(const ga_grid_env* e, int64_t) {
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

MultiTaskEnv<PointEnv> ga_env_to_dev(const ga_multi_point_env* e, int64_t info_ld) {
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

template <class GaEnv, class K>
StateEnv<K> ga_env_to_dev(const GaEnv* e, int64_t) {
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

// Validation + conversion of the C-ABI arguments of one env step (also used by the
// fused policy + env step of policy_fused.hip): the env, the record and the
// NormalizedEnv part
template <class GaEnv>
int ga_build_env_step(const GaEnv* env, const ga_record_args* a, const ga_norm_args* norm,
                      const float* actions, int64_t lda, const float* obs, const char* who,
                      ga_env_step_args_t<GaEnv>* out, bool rescale_inside) {
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
      GA_REQUIRE(norm->act_high && norm->scaled_action && !ga_env_discrete(env),
                 "%s: action rescale needs bounds, scratch and a continuous action space",
                 who);
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
#define GA_BUILD_ENV_STEP_OF(E)                                                        \
  template int ga_build_env_step<E>(const E*, const ga_record_args*, const ga_norm_args*, \
                                    const float*, int64_t, const float*, const char*,  \
                                    ga_env_step_args_t<E>*, bool);
GA_BUILD_ENV_STEP_OF(ga_synth_env)
GA_BUILD_ENV_STEP_OF(ga_point_env)
GA_BUILD_ENV_STEP_OF(ga_grid_env)
GA_BUILD_ENV_STEP_OF(ga_multi_point_env)
#define GA_BUILD_STATE_ENV_STEP_OF(E, KIND, DEV, OBS, DISCRETE) GA_BUILD_ENV_STEP_OF(E)
GA_STATE_ENV_KINDS(GA_BUILD_STATE_ENV_STEP_OF)
#undef GA_BUILD_STATE_ENV_STEP_OF
#undef GA_BUILD_ENV_STEP_OF

// Environment.reset (_environment.py:237-276; envs/point_env.py:79-98,
// grid_world_env.py:91-109, multi_env_wrapper.py:169-194)
extern "C" int ga_env_reset(const ga_env_ref* ref, const uint8_t* mask, float* obs,
                            int64_t ldo, ga_stream_t stream) {
  const char* who = "ga_env_reset";
  return ga_visit_env(ref, who, [&](auto* env) {
    int rc = check_env(env, who);
    if (rc) return rc;
    GA_REQUIRE(obs && ldo >= ga_env_obs_dim(env), "%s: bad obs buffer", who);
    const auto e = ga_env_to_dev(env, 1);
    hipLaunchKernelGGL(env_reset_kernel<decltype(e)>,
                       dim3((unsigned)ga_ceil_div(env->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, e, mask, obs, ldo);
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
    const auto e = ga_env_to_dev(env, 1);
    hipLaunchKernelGGL(env_step_kernel<decltype(e)>,
                       dim3((unsigned)ga_ceil_div(env->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, e, actions, lda, obs, next_obs, ldo, reward,
                       step_type);
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
    hipLaunchKernelGGL(env_step_record_kernel<decltype(args.e)>,
                       dim3((unsigned)ga_ceil_div(rec->n, 256)), dim3(256), 0,
                       (hipStream_t)stream, args);
    GA_CHECK_LAUNCH("env_step_record");
    return GA_OK;
  });
}

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
