// The fixed summation trees of the optimizer launches, written once for the kernels
// that run them: reduce_regions_adam_kernel and dgrad_wgrad0_body (fused_train.hip),
// reduce_members_adam_kernel (members_step.hip).  Device code only.
#pragma once
#include "common.h"

namespace {

// The sum of one parameter quad's partials, written once for the kernels that run
// it (reduce_regions_adam_kernel, dgrad_wgrad0_body for the middle layer's split-K
// slabs, reduce_members_adam_kernel).  4 * (64 / Q) shares per quad: a share sums a
// contiguous run of ceil(n_part / shares) partials, in groups of four, then singly; the
// lane-shares meet
// in a butterfly, the wave-shares (four of them; or, where one wave holds all four
// shares of a quad, lanes 16 and 32 apart in a two-step butterfly: the same tree) as
// (a0 + a1) + (a2 + a3).  An accumulator starts at +0 and so never becomes -0: a
// share with an empty run adds an exact zero.
__device__ __forceinline__ void ft_sum_group4(float4& acc, const float4& v0,
                                              const float4& v1, const float4& v2,
                                              const float4& v3) {
  acc.x += (v0.x + v1.x) + (v2.x + v3.x);
  acc.y += (v0.y + v1.y) + (v2.y + v3.y);
  acc.z += (v0.z + v1.z) + (v2.z + v3.z);
  acc.w += (v0.w + v1.w) + (v2.w + v3.w);
}
__device__ __forceinline__ void ft_sum_single(float4& acc, const float4& v0) {
  acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
}
// partials [p0, p1) of the quad at s, four independent 16-B loads in flight
__device__ __forceinline__ float4 ft_share_run(const float* s, int64_t stride, int p0,
                                               int p1) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int k = p0;
  for (; k + 4 <= p1; k += 4) {
    const float4 v0 = *reinterpret_cast<const float4*>(s + (int64_t)k * stride);
    const float4 v1 = *reinterpret_cast<const float4*>(s + (int64_t)(k + 1) * stride);
    const float4 v2 = *reinterpret_cast<const float4*>(s + (int64_t)(k + 2) * stride);
    const float4 v3 = *reinterpret_cast<const float4*>(s + (int64_t)(k + 3) * stride);
    ft_sum_group4(acc, v0, v1, v2, v3);
  }
  for (; k < p1; ++k)
    ft_sum_single(acc, *reinterpret_cast<const float4*>(s + (int64_t)k * stride));
  return acc;
}
// lanes Q, 2 Q, .. 32 apart: lane-share 0 ends with ((a0 + a1) + (a2 + a3)) + ...
__device__ __forceinline__ void ft_lane_shares_meet(float (&g)[4], int Q) {
  for (int off = Q; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] += __shfl_xor(g[j], off, 64);
  }
}
__device__ __forceinline__ void ft_wave_shares_meet(float (&g)[4], const float4& a0,
                                                    const float4& a1, const float4& a2,
                                                    const float4& a3) {
  g[0] = (a0.x + a1.x) + (a2.x + a3.x);
  g[1] = (a0.y + a1.y) + (a2.y + a3.y);
  g[2] = (a0.z + a1.z) + (a2.z + a3.z);
  g[3] = (a0.w + a1.w) + (a2.w + a3.w);
}

}  // namespace
