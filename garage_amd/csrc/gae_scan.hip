// Wavefront-segmented reverse scan: discounted returns + GAE(lambda) advantages.
//
// Replaces, in one HBM pass,
//   * garage.np.discount_cumsum called row by row   (np/_functions.py:111-128,
//     call site torch/algos/vpg.py:149-153)
//   * garage.torch.compute_advantages               (torch/_functions.py:25-85)
// including the reference's zero-padding semantics for short episodes
// (SURVEY.md Q2): padded baseline cells hold v0 = V(0-obs), so an episode of
// length L < P starts its backward recursion from a closed-form carry C0(P-L)
// and bootstraps its last step from v0.
//
// Layout: a "row" is a contiguous run of fp32 steps -- one env's slice of the
// env-major (n_envs, T) rollout buffer (mode 0: episode ends are marked by
// tail[i] = episode length, 0 elsewhere), or one episode of a packed /
// padded batch (mode 1: the row's last element is the episode end).  A group of
// `lpr` lanes (power of two <= 64) owns a row; each lane owns 4 consecutive
// steps (one 16-B load per array), composes their affine maps right-to-left,
// and the group runs a log-step suffix scan over (decay, offset) pairs with
// wave shuffles.  Rows longer than 4*lpr are walked chunk by chunk from the
// right with a group-uniform carry.  Both recurrences run in fp64 registers
// (the reference does the returns in float64; HBM, not the VALU, bounds this
// kernel) and are stored as fp32.
//
// Algorithmic HBM bytes: 16 per step (r, V in; A, G out) (+2 for the tail flag).
#include "common.h"
#include <hip/hip_ext.h>

#include "gae_scan_body.h"
#include "prof.h"

namespace {

template <bool VEC>
__global__ __launch_bounds__(256, 4) void gae_scan_kernel(ScanParams p) {
  gae_scan_wave<VEC>(p, p.v0, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6),
                     threadIdx.x & 63, AdvToHbm{p.adv});
}

// Fast path for rows that are whole episodes of at most 256 steps (mode 1, no
// per-step bonus): fixed-horizon batches, padded rows shorter than P, and packed
// ragged batches.  A row's only special step is its last one, and what the
// zero-padded tail hands it -- bootstrap value V(0-obs) and the closed-form carry
// C0(P - L); nothing when L == P -- is a constant added to that
// step's offset.  After that every step decays by the same constant, so the
// suffix scan carries only the offsets: the decay a lane applies at scan step s is
// c^(4 * 2^s), precomputed on the host by the same repeated squaring the general
// kernel does in registers, and the per-step kind selection disappears: ~5x
// fewer instructions than the general kernel, which is issue bound (not HBM
// bound) at 4096 x 256.  Rows may start at any float (packed batches): the four
// steps of a lane are then loaded and stored one by one, still coalesced across
// the lanes.
template <int NQ>
__global__ __launch_bounds__(256) void gae_scan_rows_kernel(RowsScanParams p) {
  gae_scan_rows_wave<NQ>(p, p.v0, (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6),
                         threadIdx.x & 63, AdvToHbm{p.adv});
}

}  // namespace

static int g_fixed_fast_path = 1;
// steps per lane of the whole-episode fast path: 4 or 8 (A/B runs)
static int g_rows_steps_per_lane = 4;
extern "C" int ga_set_gae_rows_steps_per_lane(int steps) {
  g_rows_steps_per_lane = steps == 8 ? 8 : 4;
  return 0;
}
extern "C" int ga_set_gae_fixed_fast_path(int on) {
  g_fixed_fast_path = on != 0;
  return 0;
}
int ga_gae_fixed_fast_path(void) { return g_fixed_fast_path; }
int ga_gae_rows_steps_per_lane(void) { return g_rows_steps_per_lane; }

// See include/garage_amd.h for the contract.
extern "C" int ga_gae_scan_f32(const float* rewards, const float* values,
                               const float* bonus, const uint16_t* tail,
                               const int64_t* offsets, int64_t n_rows, int64_t T,
                               int64_t ld, int64_t max_len, int mode,
                               int max_episode_length, double discount,
                               double gae_lambda, float v0, float bonus_const,
                               float* adv, float* ret, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(rewards && values && adv && ret, "ga_gae_scan_f32: null pointer");
  GA_REQUIRE(n_rows >= 0 && T >= 0, "ga_gae_scan_f32: negative size");
  GA_REQUIRE(mode == 0 || mode == 1, "ga_gae_scan_f32: mode must be 0 or 1");
  GA_REQUIRE(mode == 1 || tail != nullptr,
             "ga_gae_scan_f32: mode 0 needs the tail array");
  GA_REQUIRE(max_episode_length >= 1, "ga_gae_scan_f32: max_episode_length < 1");
  if (!offsets) {
    GA_REQUIRE(ld >= T, "ga_gae_scan_f32: ld (%lld) < T (%lld)", (long long)ld,
               (long long)T);
    max_len = T;
  } else {
    GA_REQUIRE(max_len >= 0, "ga_gae_scan_f32: max_len required with offsets");
  }
  const int64_t prof_steps = T;  // packed mode: callers pass the total step count in T
  if (n_rows == 0 || max_len == 0) return GA_OK;

  // (which kernel, with which parameters: gae_scan_params.h)
  GaScanPlan plan;
  ga_gae_scan_plan(rewards, values, bonus, tail, offsets, n_rows, T, ld, max_len, mode,
                   max_episode_length, discount, gae_lambda, (double)v0, bonus_const, adv, ret,
                   &plan);
  const int64_t blocks = ga_ceil_div(plan.waves, 4);
  GA_REQUIRE(blocks < (1ll << 31), "ga_gae_scan_f32: grid too large");
  // algorithmic bytes: 16 per step (r, V in; A, G out)
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_GAE_SCAN,
                 16.0 * (offsets ? (double)prof_steps : (double)n_rows * (double)T),
                 &e0, &e1);
  switch (plan.kernel) {
    case GS_ROWS_2:
      hipExtLaunchKernelGGL(gae_scan_rows_kernel<2>, dim3((unsigned)blocks), dim3(256),
                            0, stream, e0, e1, 0, plan.f);
      break;
    case GS_ROWS_1:
      hipExtLaunchKernelGGL(gae_scan_rows_kernel<1>, dim3((unsigned)blocks), dim3(256),
                            0, stream, e0, e1, 0, plan.f);
      break;
    case GS_GENERAL_VEC:
      hipExtLaunchKernelGGL(gae_scan_kernel<true>, dim3((unsigned)blocks), dim3(256),
                            0, stream, e0, e1, 0, plan.p);
      break;
    default:
      hipExtLaunchKernelGGL(gae_scan_kernel<false>, dim3((unsigned)blocks), dim3(256),
                            0, stream, e0, e1, 0, plan.p);
  }
  GA_CHECK_LAUNCH("ga_gae_scan_f32");
  return GA_OK;
}
