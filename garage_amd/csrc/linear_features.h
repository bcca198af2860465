// The feature row of garage's LinearFeatureBaseline, written ONCE for the Gram pass and
// the predict pass of linear_baseline.hip (np/baselines/linear_feature_baseline.py:43-58):
//   [clip(obs, -10, 10), clip(obs)^2, al, al^2, al^3, 1],  al = t / 100.0,
// t the row's index inside its episode, F = 2 * obs_dim + 4 columns in that order.
// Everything from the clip on is fp64, as the reference, which is handed float64
// observations.  A row comes in two kinds of pieces, each handing (column, value) pairs to
// a sink: one observation gives its clipped value and the square of that, the step index
// gives the last four columns.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LB_CLIP_LOW (-10.0)  // LinearFeatureBaseline.lower_bound / upper_bound
#define LB_CLIP_HIGH 10.0

// np.clip of one observation (a NaN passes through, as it does there)
__device__ __forceinline__ double lb_clip(float o) {
  const double x = (double)o;
  return x < LB_CLIP_LOW ? LB_CLIP_LOW : (x > LB_CLIP_HIGH ? LB_CLIP_HIGH : x);
}

// observation j (0 <= j < O) of the row -> columns j and O + j
template <class Sink>
__device__ __forceinline__ void lb_obs_features(float obs_j, int O, int j, Sink&& sink) {
  const double x = lb_clip(obs_j);
  sink(j, x);
  sink(O + j, x * x);
}

// step t of the episode -> columns 2 O .. 2 O + 3
template <class Sink>
__device__ __forceinline__ void lb_time_features(int64_t t, int O, Sink&& sink) {
  const double al = (double)t / 100.0;
  sink(2 * O, al);
  sink(2 * O + 1, al * al);
  sink(2 * O + 2, al * al * al);
  sink(2 * O + 3, 1.0);
}

// The episode e of sample `row`: ep_off[e] <= row < ep_off[e + 1], for strictly increasing
// ep_off[0 .. n_eps] with ep_off[0] = 0 (episodes of length >= 1).  Reads ep_off[1 .. n_eps - 1]
// only, whatever the array holds.
__device__ __forceinline__ int64_t lb_episode_of(const int64_t* __restrict__ ep_off,
                                                 int64_t n_eps, int64_t row) {
  int64_t lo = 0, hi = n_eps;
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ep_off[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}
