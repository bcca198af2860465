// The hidden activations and their slopes, each expression stated ONCE, by NETWORK code
// (ga_mlp_desc::hidden_act: 0 tanh, 1 relu, 2 none, 3 sigmoid, 4 elu (alpha 1),
// 5 leaky_relu (slope 0.01), 6 softplus (beta 1, threshold 20): torch.nn.functional's
// defaults).  Every slope is a function of the layer's OUTPUT h, so a backward pass needs
// no pre-activation in memory.  The per-layer epilogues (gemm_core.h: act_apply_more /
// act_slope_more, a run-time code behind a call) and the narrow one-launch step
// (narrow_body.h: one force-inlined copy per code behind a wave-uniform switch) both
// evaluate these, so the two paths differ in summation order alone.  Device code only.
#pragma once
#include <type_traits>

#include "common.h"

template <int HACT>
__device__ __forceinline__ float ga_hact_apply(float v) {
  if constexpr (HACT == 0) return ga_tanh(v);  // common.h
  else if constexpr (HACT == 1) return fmaxf(v, 0.f);
  else if constexpr (HACT == 3) return 1.f / (1.f + expf(-v));
  else if constexpr (HACT == 4) return v > 0.f ? v : expm1f(v);
  else if constexpr (HACT == 5) return v > 0.f ? v : 0.01f * v;
  else if constexpr (HACT == 6) return v > 20.f ? v : log1pf(expf(v));
  else return v;
}

template <int HACT>
__device__ __forceinline__ float ga_hact_slope(float h) {
  if constexpr (HACT == 0) return 1.f - h * h;
  else if constexpr (HACT == 1) return h > 0.f ? 1.f : 0.f;
  else if constexpr (HACT == 3) return h * (1.f - h);
  else if constexpr (HACT == 4) return h > 0.f ? 1.f : h + 1.f;  // exp(x) = h + 1 for x <= 0
  else if constexpr (HACT == 5) return h > 0.f ? 1.f : 0.01f;
  else if constexpr (HACT == 6) return 1.f - expf(-h);  // sigmoid(x), h = log(1 + e^x)
  else return 1.f;
}

// f(integral_constant<network code>) for a non-tanh code 1 .. 6, behind a switch on a
// value the caller keeps wave-uniform (a kernel argument: an SGPR compare and branch)
template <class F>
__device__ __forceinline__ void ga_hact_dispatch(int hact, F&& f) {
  switch (hact) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 2>{}); break;
  }
}
