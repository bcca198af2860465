// Shared helpers for the gfx950 kernels of garage_amd.  CDNA4 only: wave = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include <string.h>

#include "internal.h"

#define GA_WAVE 64

// ---- error plumbing (ga_set_error: thread-local message, negative return codes) --

#define GA_OK 0
#define GA_ERR_ARG (-1)
#define GA_ERR_HIP (-2)

#define GA_REQUIRE(cond, ...)            \
  do {                                   \
    if (!(cond)) {                       \
      ga_set_error(__VA_ARGS__);         \
      return GA_ERR_ARG;                 \
    }                                    \
  } while (0)

#define GA_CHECK_LAUNCH(name)                                          \
  do {                                                                 \
    hipError_t e__ = hipGetLastError();                                \
    if (e__ != hipSuccess) {                                           \
      ga_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return GA_ERR_HIP;                                               \
    }                                                                  \
  } while (0)

static inline bool ga_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

static inline int64_t ga_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- torch.optim.Adam (OptimizerWrapper.step, torch/optimizers/optimizer_wrapper.py:53-63)
// The per-step constants, derived on the host in double and rounded once.
struct GaAdam {
  float lerp_w;         // 1 - beta1
  float beta2, one_minus_beta2;
  float neg_step_size;  // -lr / (1 - beta1^t)
  float bc2_sqrt;       // sqrt(1 - beta2^t)
  float eps;
};

static inline GaAdam ga_adam_coeffs(double lr, double beta1, double beta2, double eps,
                                    int64_t step) {
  GaAdam a;
  a.lerp_w = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.one_minus_beta2 = (float)(1.0 - beta2);
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  a.neg_step_size = (float)(-(lr / bc1));
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)eps;
  return a;
}

// Everything below is for the device compiler; the host C++ that the CPU harnesses
// under tests/host build (mlp_layers.cpp) takes the plumbing above.
#ifdef __HIP__

// One element of torch.optim.Adam's single-tensor step, the ONE Adam of every kernel,
// with fused multiply-add contraction switched off (HIP's __fmul_rn / __fadd_rn are
// plain operators, so the compiler would otherwise be free to contract differently in
// each kernel): one rounding per torch operation.
__device__ __forceinline__ void ga_adam_update(const GaAdam& a, float g, float& p,
                                               float& m, float& v) {
#pragma clang fp contract(off)
  const float diff = g - m;
  m = fmaf(a.lerp_w, diff, m);             // exp_avg.lerp_(grad, 1 - beta1): torch's
                                           // lerp is one fused multiply-add
  const float gg = (a.one_minus_beta2 * g) * g;
  v = v * a.beta2 + gg;                    // mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  const float num = a.neg_step_size * m;
  p = p + num / denom;                     // addcdiv_(exp_avg, denom, -step_size)
}

// ---- device helpers --------------------------------------------------------
// XCD-aware workgroup order.  Workgroups are dealt to the 8 XCDs round-robin by
// their linear id, and each XCD has its own L2, so workgroups that read the same
// operand tile should have equal id % 8 (one L2 fetch instead of one per XCD) and
// close ids (co-resident).  Groups of `n_members` such workgroups are laid out as
//   id = (grp / 8) * 8 * n_members + member * 8 + grp % 8
// with the last n_groups % 8 groups in plain order.
__device__ __forceinline__ void ga_xcd_group(int id, int n_groups, int n_members,
                                             int* grp, int* member) {
  const int chunk = 8 * n_members;
  const int full = (n_groups / 8) * chunk;
  if (id < full) {
    const int c = id / chunk, r = id % chunk;
    *grp = c * 8 + (r & 7);
    *member = r >> 3;
  } else {
    const int r = id - full;
    *grp = (n_groups / 8) * 8 + r / n_members;
    *member = r % n_members;
  }
}

// tanh(x) = 1 - 2 / (exp(2x) + 1) on the hardware exp / rcp units, the ONE tanh of
// every kernel (forward, rollout and training paths must agree): v_exp, v_rcp and
// one Newton step on the reciprocal (8 VALU instructions; an IEEE division in its
// place costs 11 more, and the activation epilogues are VALU bound).  Absolute error
// <= ~2e-7 over the whole range; the exponent is capped so that exp stays finite
// (2 / (e^80 + 1) is 0 in fp32: the result is exactly 1 from x = 40 on), -1 at the
// other end, NaN in -> NaN out.
__device__ __forceinline__ float ga_tanh(float x) {
  const float t = 2.f * x;
  const float e = __expf(t > 80.f ? 80.f : t);  // (not fminf: a NaN must get through)
  const float d = e + 1.f;
  float r = __builtin_amdgcn_rcpf(d);
  r = fmaf(fmaf(-d, r, 1.f), r, r);
  return fmaf(-2.f, r, 1.f);
}

// The scalar std parameter of GaussianMLPBaseModule.forward
// (torch/modules/gaussian_mlp_module.py:165-181): clamp to [log min_std,
// log max_std], then 'exp' -> log std = p, or 'softplus' -> std =
// log(1 + exp(exp(p))).  `has_min` carries two flags: bit 0 = a lower clamp is
// present, bit 1 = softplus parameterisation.  Returns log std and
// *chain = d(log std) / d(parameter) (0 through an active clamp: torch.clamp
// passes no gradient outside the range).
__host__ __device__ inline float ga_log_std(float param, int has_min, float min_log_std,
                                            int has_max, float max_log_std,
                                            float* chain) {
  float p = param, c = 1.f;
  if ((has_min & 1) && p < min_log_std) { p = min_log_std; c = 0.f; }
  if (has_max && p > max_log_std) { p = max_log_std; c = 0.f; }
  if (has_min & 2) {
    const float e = expf(p);
    const float sp = logf(1.f + expf(e));  // the reference's .exp().exp().add(1).log()
    c *= e / ((1.f + expf(-e)) * sp);
    p = logf(sp);
  }
  if (chain) *chain = c;
  return p;
}

// ---- scalar-offset addressing.  A buffer instruction's address is
//   base (descriptor, 4 SGPRs) + scalar offset (SGPR) + lane offset (ONE VGPR) + immediate
// (< 4096): where a loop's accesses differ from each other by wave-uniform amounts only,
// the lane offset is computed once in front of the loop and the loop itself needs no
// vector arithmetic for its addresses -- a global_load takes a 64-bit vector address per
// access instead (beside an fp32 MFMA every vector instruction costs its issue time).
// `base` and `bytes` must be wave-uniform (kernel arguments, blockIdx, a readfirstlane'd
// wave id), so must every `soff`; all offsets are bytes, and base + every offset stays
// below 4 GB from `base`.  `bytes` is the exact extent behind `base` that the caller may
// touch: the unit drops an access whose lane offset + immediate reaches beyond it (a load
// returns zero, a store writes nothing).  The scalar offset is NOT part of that test, so
// this is a second line behind the caller's own clamps and predicates, never their
// replacement.  Vector memory instructions only.
struct GaBuffer {
  __amdgpu_buffer_rsrc_t r;
  __device__ __forceinline__ GaBuffer(const void* base, uint32_t bytes)
      : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes,
                                            0x00020000)) {}
  __device__ __forceinline__ float load(uint32_t voff, uint32_t soff) const {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
  }
  __device__ __forceinline__ float4 load4(uint32_t voff, uint32_t soff) const {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                       __uint_as_float(v[3]));
  }
  __device__ __forceinline__ void store4(const float4& x, uint32_t voff, uint32_t soff) const {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {__float_as_uint(x.x), __float_as_uint(x.y), __float_as_uint(x.z),
                     __float_as_uint(x.w)};
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, (int)soff, 0);
  }
  __device__ __forceinline__ void store2(float x, float y, uint32_t voff, uint32_t soff) const {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 v = {__float_as_uint(x), __float_as_uint(y)};
    __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)voff, (int)soff, 0);
  }
};

__device__ __forceinline__ float ga_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // valid in lane 0
}

__device__ __forceinline__ double ga_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ float ga_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}

// Block-wide sum of doubles for blockDim.x == 256 (4 waves); result in thread 0.
__device__ __forceinline__ double ga_block_sum_256(double v, double* smem4) {
  v = ga_wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) smem4[w] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) r = smem4[0] + smem4[1] + smem4[2] + smem4[3];
  __syncthreads();
  return r;
}
#endif  // __HIP__
