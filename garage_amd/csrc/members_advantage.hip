// Every member's returns, GAE(lambda) advantages and advantage normalisation in ONE launch.
//
// Replaces, per member of a population, the eight launches of the lone path
// (ga_gae_scan_f32; ga_stats_f32 twice, two launches each; ga_adv_center_f32; ga_stats_f32(2)
// and ga_sub_scalar_f32 for positive_adv), which move 32..44 bytes per step, by one
// workgroup's work at the algorithmic 16 bytes per step (r, V in; A, G out).
//
// Work split: one workgroup of MA_THREADS (16 waves) per member; no workgroup talks to
// another.  The member's advantage vector lives in 4 * S bytes of dynamic LDS
// (S <= MA_MAX_STEPS) between the scan and the one store:
//   A  the scan.  The 16 waves take the wave indices w, w + 16, .. of the lone launch and
//      run that kernel's row arithmetic (gae_scan_body.h; which kernel: the entry says, by
//      the rule of gae_scan_params.h).  Returns go straight to HBM, the raw advantages --
//      rounded to fp32 where the lone kernel rounds them -- to LDS at their packed position.
//   B  the moments out of LDS, fp64, in the order of stats_partial_kernel +
//      stats_finalize_kernel (losses.hip) at ga_red_blocks(S) blocks: the four 256-thread
//      quarters play the virtual blocks q, q + 4, ..; one wave finishes the partials.  Then
//      (a - mean) / (var + 1e-8) in fp32 as adv_center_kernel, back into LDS.
//   C  positive_adv: the minimum in the order of stats_partial_kernel<2>, subtracted as
//      sub_scalar_kernel does.
// and the advantages go to HBM once, in 16-byte pieces where they are contiguous and
// their base is aligned.  Every member gets the bits of its lone launches.
#include "common.h"
#include <hip/hip_ext.h>

#include "gae_scan_body.h"
#include "members_advantage.h"
#include "prof.h"

namespace {

// The advantages of a member: to LDS at the packed position (row * T + step where the
// rows lie ld > T apart).  Positions beyond S (offsets that do not describe S packed
// steps) are dropped.
struct AdvToLds {
  float* x;
  int64_t S, T;
  bool packed;
  __device__ __forceinline__ int64_t pos(int64_t row, int64_t start, int64_t i) const {
    return packed ? start + i : row * T + i;
  }
  __device__ __forceinline__ void quad(int64_t row, int64_t start, int64_t i, float a0,
                                       float a1, float a2, float a3) const {
    const int64_t at = pos(row, start, i);
    if (at < 0 || at + 3 >= S) {
      one_at(at, a0); one_at(at + 1, a1); one_at(at + 2, a2); one_at(at + 3, a3);
    } else if ((at & 3) == 0) {
      *reinterpret_cast<float4*>(x + at) = make_float4(a0, a1, a2, a3);
    } else {
      x[at] = a0; x[at + 1] = a1; x[at + 2] = a2; x[at + 3] = a3;
    }
  }
  __device__ __forceinline__ void one(int64_t row, int64_t start, int64_t i, float a) const {
    one_at(pos(row, start, i), a);
  }
  __device__ __forceinline__ void one_at(int64_t at, float a) const {
    if (at >= 0 && at < S) x[at] = a;
  }
};

// THE summation order of the statistics, as stats_partial_kernel<WHAT> (losses.hip) walks
// it: what thread `thread` of block `block` of `nb` blocks of 256 accumulates over
// source[0 .. n).  WHAT 0: sum, 1: squared deviations from `mean`, 2: minimum.
template <int WHAT>
__device__ __forceinline__ double ma_thread_part(const float* source, int64_t n, int nb,
                                                 int block, int thread, double mean) {
  double acc = (WHAT == 2) ? 1.0e300 : 0.0;
  for (int64_t i = (int64_t)block * 256 + thread; i < n; i += (int64_t)nb * 256) {
    const double v = (double)source[i];
    if (WHAT == 0) acc += v;
    if (WHAT == 1) acc += (v - mean) * (v - mean);
    if (WHAT == 2) acc = fmin(acc, v);
  }
  return acc;
}

// One statistic of source[0 .. n) by the whole workgroup; the result is valid in thread 0.
// wave_parts: [nb][4] doubles of LDS, a virtual block's four wave results -- the block's
// partial is ((s0 + s1) + s2) + s3 (ga_block_sum_256) or the minimum of the pairs' minima,
// and lane l of the finishing wave takes the partials l, l + 64, .. (stats_finalize_kernel).
template <int WHAT>
__device__ __forceinline__ double ma_statistic(const float* source, int64_t n, int nb,
                                               double mean, double (*wave_parts)[4]) {
  const int quarter = threadIdx.x >> 8, t = threadIdx.x & 255;
  for (int b = quarter; b < nb; b += 4) {
    double acc = ma_thread_part<WHAT>(source, n, nb, b, t, mean);
    if (WHAT == 2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc = fmin(acc, __shfl_down(acc, o, 64));
    } else {
      acc = ga_wave_sum(acc);
    }
    if ((t & 63) == 0) wave_parts[b][t >> 6] = acc;
  }
  __syncthreads();
  double a = (WHAT == 2) ? 1.0e300 : 0.0;
  if (threadIdx.x < 64) {
    for (int k = threadIdx.x; k < nb; k += 64) {
      const double* s = wave_parts[k];
      if (WHAT == 2)
        a = fmin(a, fmin(fmin(s[0], s[1]), fmin(s[2], s[3])));
      else
        a += s[0] + s[1] + s[2] + s[3];
    }
    if (WHAT == 2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a = fmin(a, __shfl_down(a, o, 64));
    } else {
      a = ga_wave_sum(a);
    }
  }
  return a;
}

extern __shared__ __align__(16) float ma_adv[];  // [S] (round4), the member's advantages

__global__ __launch_bounds__(MA_THREADS) void members_advantage_kernel(
    const MaEntry* __restrict__ table) {
  __shared__ double wave_parts[MA_MAX_STEPS / 256][4];
  __shared__ double st[4];  // sum, count, squared deviations, minimum
  const MaEntry& e = table[blockIdx.x];
  const int64_t S = e.S;
  const int flags = e.flags;
  const int tid = threadIdx.x;
  float* x = ma_adv;

  // ---- A: the scan
  {
    const double v0 = e.v0 ? (double)*e.v0 : 0.0;
    const int lane = tid & 63;
    const int64_t waves = e.waves;
    const bool packed = (flags & MA_PACKED) != 0;
    switch (e.kernel) {
      case GS_ROWS_1:
        for (int64_t wave = tid >> 6; wave < waves; wave += MA_THREADS / 64)
          gae_scan_rows_wave<1>(e.r, v0, wave, lane, AdvToLds{x, S, e.r.T, packed});
        break;
      case GS_ROWS_2:
        for (int64_t wave = tid >> 6; wave < waves; wave += MA_THREADS / 64)
          gae_scan_rows_wave<2>(e.r, v0, wave, lane, AdvToLds{x, S, e.r.T, packed});
        break;
      case GS_GENERAL_VEC:
        for (int64_t wave = tid >> 6; wave < waves; wave += MA_THREADS / 64)
          gae_scan_wave<true>(e.g, v0, wave, lane, AdvToLds{x, S, e.g.T, packed});
        break;
      default:
        for (int64_t wave = tid >> 6; wave < waves; wave += MA_THREADS / 64)
          gae_scan_wave<false>(e.g, v0, wave, lane, AdvToLds{x, S, e.g.T, packed});
    }
  }
  __syncthreads();

  const int nb = ga_red_blocks(S);
  // ---- B: mean and unbiased variance, then the centring (adv_center_kernel)
  if (flags & MA_CENTER) {
    const double sum = ma_statistic<0>(x, S, nb, 0.0, wave_parts);
    if (tid == 0) {
      st[0] = sum;
      st[1] = (double)S;
    }
    __syncthreads();
    const double dev = ma_statistic<1>(x, S, nb, st[0] / st[1], wave_parts);
    if (tid == 0) st[2] = dev;
    __syncthreads();
    const float mean = (float)(st[0] / st[1]);
    const float var = (float)(st[2] / (st[1] - 1.0));
    const float denom = var + 1e-8f;
    for (int64_t i = tid; i < S; i += MA_THREADS) x[i] = (x[i] - mean) / denom;
    __syncthreads();
  }
  // ---- C: positive_adv (stats_partial_kernel<2>, sub_scalar_kernel)
  if (flags & MA_POSITIVE) {
    const double lo = ma_statistic<2>(x, S, nb, 0.0, wave_parts);
    if (tid == 0) st[3] = lo;
    __syncthreads();
    const float s = (float)st[3];
    for (int64_t i = tid; i < S; i += MA_THREADS) x[i] -= s;
    __syncthreads();
  }

  // ---- the one store of the advantages, and the statistics of the phases that ran
  float* adv = e.adv;
  if (!(flags & MA_PACKED)) {
    const int64_t T = e.g.T, ld = e.g.ld;  // (both parameter structs hold them)
    for (int64_t i = tid; i < S; i += MA_THREADS) adv[(i / T) * ld + i % T] = x[i];
  } else if ((reinterpret_cast<uintptr_t>(adv) & 15u) == 0) {
    const int64_t quads = S >> 2;
    for (int64_t i = tid; i < quads; i += MA_THREADS)
      reinterpret_cast<float4*>(adv)[i] = reinterpret_cast<const float4*>(x)[i];
    for (int64_t i = 4 * quads + tid; i < S; i += MA_THREADS) adv[i] = x[i];
  } else {
    for (int64_t i = tid; i < S; i += MA_THREADS) adv[i] = x[i];
  }
  if (tid == 0) {
    if (flags & MA_CENTER) {
      e.stats[0] = st[0];
      e.stats[1] = st[1];
      e.stats[2] = st[2];
    }
    if (flags & MA_POSITIVE) e.stats[3] = st[3];
  }
}

}  // namespace

int ma_launch_advantage_members(const MaEntry* table, unsigned n, unsigned lds_bytes,
                                double work, hipStream_t stream) {
  // (more than 64 KiB of dynamic LDS has to be asked for; once is enough)
  static const hipError_t attr = hipFuncSetAttribute(
      reinterpret_cast<const void*>(members_advantage_kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, 4 * MA_MAX_STEPS);
  if (attr != hipSuccess) {
    ga_set_error("ga_advantages_members_f32: cannot ask for %d bytes of LDS: %s",
                 4 * MA_MAX_STEPS, hipGetErrorString(attr));
    return GA_ERR_HIP;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_GAE_SCAN, work, &e0, &e1);
  hipExtLaunchKernelGGL(members_advantage_kernel, dim3(n), dim3(MA_THREADS), lds_bytes,
                        stream, e0, e1, 0, table);
  GA_CHECK_LAUNCH("ga_advantages_members_f32");
  return GA_OK;
}
