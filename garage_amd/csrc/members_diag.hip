// Device code of the members' joint diagnostics that has no lone body to share
// (members_diag.h): what log_performance reduces every member's episodes to, in one grid.
// The twins of the forward, loss and KL kernels sit beside their lone kernels' bodies
// (gemm.hip, skinny.hip, losses.hip).
#include "common.h"
#include "members_diag.h"

namespace {

// Entry blockIdx.y, one thread per episode.  The reward sum is episode_sums_kernel's
// (rollout.hip): in time order, fp64 -- the same additions, the same bits.  The first
// return and the terminal flag are conversions of single values.
__global__ __launch_bounds__(256) void episodes_members_kernel(const MdEpisodes* table) {
  const MdEpisodes m = table[blockIdx.y];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m.n_eps) return;
  const int64_t beg = m.ep_off[e], end = m.ep_off[e + 1];
  double acc = 0.0;
  for (int64_t j = beg; j < end; ++j) acc += (double)m.rewards[j];
  m.out[e] = acc;
  m.out[m.n_eps + e] = (double)m.returns[beg];
  m.out[2 * m.n_eps + e] = (int)m.step_types[end - 1] == m.terminal ? 1.0 : 0.0;
}

}  // namespace

int md_launch_episodes_members(const MdEpisodes* table, unsigned n, unsigned blocks,
                               hipStream_t stream) {
  hipLaunchKernelGGL(episodes_members_kernel, dim3(blocks, n), dim3(256), 0, stream, table);
  GA_CHECK_LAUNCH("episodes_members");
  return GA_OK;
}
