// Fused loss / gradient-seed / optimiser kernels of the PPO update (gfx950): the device
// code, and at the end of the file the launch seam of loss_params.h, which only
// instantiates and launches.  The entry points -- checks, parameter structs, grids, one
// launch or two -- are losses_host.cpp's; the parameter structs loss_params.h's.
//
// All are HBM / latency bound elementwise passes: one thread per sample (rows
// are <= a few tens of floats), fp32 math, fp64 block partials reduced in a
// fixed order (bitwise reproducible run to run; no float atomics).
#include "common.h"
#include "loss_params.h"
#include "loss_rows.h"
#include "members_diag.h"
#include "shape_rules.h"

namespace {

// (the row kernels' bodies, loss_row_bodies.inc: the lone kernels take their own grid)
#define GA_GRID_X gridDim.x

// Multi-block reductions finish in the same launch: every block publishes its
// partial sums, then takes a ticket; the block that draws the last one sees all of
// them (release fence before the ticket, acquire fence after it, device-scope
// loads) and adds them in block order -- the same order, hence the same bits, as a
// separate one-wave finalize launch -- and leaves the ticket at 0 for the next
// launch on this workspace.  The ticket lives behind the partials
// (ga_reduction_workspace_doubles() counts it; the workspace starts zeroed).
__device__ __forceinline__ bool ga_take_last_ticket(unsigned* ticket) {
  __shared__ int is_last;
  if (threadIdx.x == 0) {
    __threadfence();  // this block's partials before its ticket
    const unsigned t = atomicAdd(ticket, 1u);
    is_last = (t == gridDim.x - 1);
    if (is_last) *ticket = 0;
  }
  __syncthreads();
  const bool last = is_last != 0;
  if (last) __threadfence();  // every block's partials after its ticket
  return last;
}
__device__ __forceinline__ double ga_peek(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Sum of partials[2 b + which] over the blocks, one wave, fixed order.
__device__ __forceinline__ double ga_sum_partials(const double* partials, int nblocks,
                                                  int which) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) v += ga_peek(partials + 2 * b + which);
  return ga_wave_sum(v);
}

// Loss value and the log-std gradient slot from the batch sums (thread 0 of the
// finalize kernel, or of the loss kernel when it is the only block).
__device__ void ppo_gaussian_finish(double obj, double ds, const float* log_std,
                                    int has_min, float min_log_std, int has_max,
                                    float max_log_std, int64_t M, int A,
                                    const LossEnt& ent, float* loss_out,
                                    float* grad_slab0, int64_t slab_stride,
                                    int64_t n_splits) {
  float chain, dlogstd;
  const float s = ga_log_std(*log_std, has_min, min_log_std, has_max, max_log_std, &chain);
  lr_gaussian_finish(ent, A, s, chain, obj, ds, M, loss_out, &dlogstd);
  if (grad_slab0) {
    grad_slab0[0] = dlogstd;
    for (int64_t k = 1; k < n_splits; ++k) grad_slab0[k * slab_stride] = 0.f;
  }
}

__global__ __launch_bounds__(256) void ppo_gaussian_loss_kernel(PpoLossParams p) {
#define GA_LOSS_BODY 1
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}

__global__ void ppo_gaussian_finalize_kernel(PpoFinalizeParams p) {
  // one wave: lanes stride over the block partials, then a fixed-order wave sum
  double obj = 0.0, ds = 0.0;
  for (int b = threadIdx.x; b < p.nblocks; b += 64) {
    obj += p.partials[2 * b + 0];
    ds += p.partials[2 * b + 1];
  }
  obj = ga_wave_sum(obj);
  ds = ga_wave_sum(ds);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ppo_gaussian_finish(obj, ds, p.log_std, p.has_min, p.min_log_std, p.has_max,
                      p.max_log_std, p.M, p.A, p.ent, p.loss_out, p.grad_slab0,
                      p.slab_stride, p.n_splits);
}

// ---- categorical policy head (CatLossParams, loss_params.h) ------------------------
// Final log-probabilities lp[j] of the row, its entropy, and (for the
// gradient) the softmax p of the raw scores.  A is small (number of actions).
__device__ __forceinline__ void cat_row(const float* sc, int A, int dbl, float* lse_out,
                                        float* mx_out, float* den_out) {
  float mx = sc[0];
  for (int j = 1; j < A; ++j) mx = fmaxf(mx, sc[j]);
  float den = 0.f;
  for (int j = 0; j < A; ++j) den += expf(sc[j] - mx);
  *mx_out = mx;
  *den_out = den;
  if (!dbl) {
    *lse_out = mx + logf(den);  // lp[j] = sc[j] - lse
  } else {
    // logits' = p in [0,1]: logsumexp without a shift is safe
    float s2 = 0.f;
    for (int j = 0; j < A; ++j) s2 += expf(expf(sc[j] - mx) / den);
    *lse_out = logf(s2);        // lp[j] = p[j] - lse
  }
}

__global__ __launch_bounds__(256) void ppo_categorical_loss_kernel(CatLossParams p) {
#define GA_LOSS_BODY 2
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}

__global__ void ppo_categorical_finalize_kernel(const double* partials, int nblocks,
                                                int64_t M, float* loss_out,
                                                double* ent_sum_out, float* grad_slab0,
                                                int64_t slab_stride, int64_t n_splits) {
  double o = 0.0, e = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) {
    o += partials[2 * b];
    e += partials[2 * b + 1];
  }
  o = ga_wave_sum(o);
  e = ga_wave_sum(e);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *loss_out = (float)(-(o / (double)M));
  if (ent_sum_out) *ent_sum_out = e;
  if (grad_slab0)  // the (unused) log-std slot of the flat layout stays 0
    for (int64_t k = 0; k < n_splits; ++k) grad_slab0[k * slab_stride] = 0.f;
}

// sum over rows of KL(old || new) for categorical heads
__global__ __launch_bounds__(256) void categorical_kl_kernel(
    const float* sc_old, const float* sc_new, int64_t ld, int64_t M, int A, int dbl,
    double* partials) {
#define GA_LOSS_BODY 3
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}

__global__ __launch_bounds__(256) void gaussian_nll_kernel(NllParams p) {
#define GA_LOSS_BODY 4
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}

__global__ void gaussian_nll_finalize_kernel(const double* partials, int nblocks,
                                             int64_t M, float* loss_out,
                                             float* grad_slab0, int64_t slab_stride,
                                             int64_t n_splits) {
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < nblocks; k += 64) {
    a += partials[2 * k];
    b += partials[2 * k + 1];
  }
  a = ga_wave_sum(a);
  b = ga_wave_sum(b);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *loss_out = (float)(a / (double)M);
  if (grad_slab0) {
    grad_slab0[0] = (float)(b / (double)M);
    for (int64_t k = 1; k < n_splits; ++k) grad_slab0[k * slab_stride] = 0.f;
  }
}

// KL(old || new) of Independent Normals with scalar log-stds, summed over rows.
__global__ __launch_bounds__(256) void gaussian_kl_kernel(
    const float* mean_old, const float* mean_new, int64_t ld, int64_t M, int A,
    float s_old, float s_new, double* partials) {
#define GA_LOSS_BODY 5
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}

__global__ void sum_partials_kernel(const double* partials, int nblocks, double* out) {
  double a = 0.0;
  for (int k = threadIdx.x; k < nblocks; k += 64) a += partials[k];
  a = ga_wave_sum(a);
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = a;
}

// ---- optimiser --------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* slabs,
                                                           int64_t n_splits,
                                                           int64_t stride, int64_t n,
                                                           float* out, float scale) {
  __builtin_amdgcn_s_setprio(3);  // (see adam_kernel)
  // 64 float4 columns x 4 slab groups per block: 4x the workgroups of a
  // column-per-thread layout and 4 independent 16-B loads in flight per thread;
  // the groups are combined through LDS in a fixed order (deterministic).
  __shared__ float4 part[4][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t i4 = ((int64_t)blockIdx.x * 64 + col) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < n) {  // n is a multiple of 4 (flat buffers are padded)
    int64_t s = grp;
    for (; s + 12 < n_splits; s += 16) {
      const float4 v0 = *reinterpret_cast<const float4*>(slabs + s * stride + i4);
      const float4 v1 =
          *reinterpret_cast<const float4*>(slabs + (s + 4) * stride + i4);
      const float4 v2 =
          *reinterpret_cast<const float4*>(slabs + (s + 8) * stride + i4);
      const float4 v3 =
          *reinterpret_cast<const float4*>(slabs + (s + 12) * stride + i4);
      acc.x += (v0.x + v1.x) + (v2.x + v3.x);
      acc.y += (v0.y + v1.y) + (v2.y + v3.y);
      acc.z += (v0.z + v1.z) + (v2.z + v3.z);
      acc.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; s < n_splits; s += 4) {
      const float4 v = *reinterpret_cast<const float4*>(slabs + s * stride + i4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  part[grp][col] = acc;
  __syncthreads();
  if (grp == 0 && i4 < n) {
    const float4 a = part[0][col], b = part[1][col], c = part[2][col],
                 d = part[3][col];
    float4 r;
    r.x = ((a.x + b.x) + (c.x + d.x)) * scale;
    r.y = ((a.y + b.y) + (c.y + d.y)) * scale;
    r.z = ((a.z + b.z) + (c.z + d.z)) * scale;
    r.w = ((a.w + b.w) + (c.w + d.w)) * scale;
    *reinterpret_cast<float4*>(out + i4) = r;
  }
}

__global__ __launch_bounds__(256) void adam_kernel(AdamParams a) {
  // (a short launch on its chain's critical path: its waves go first beside the other
  // chain's GEMMs, see reduce_regions_adam_kernel)
  __builtin_amdgcn_s_setprio(3);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  float p = a.p[i], m = a.m[i], v = a.v[i];
  ga_adam_update(a.c, a.g[i], p, m, v);
  a.p[i] = p;
  a.m[i] = m;
  a.v[i] = v;
}

// Optimizers other than the default Adam: the kinds, their hyper-parameters and state
// buffers are OptParams' (loss_params.h); torch's single-tensor arithmetic, one rounding
// per torch operation, and never a difference of two rounded constants.
__global__ __launch_bounds__(256) void optimizer_step_kernel(OptParams a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  float p = a.p[i], g = a.g[i];
  if (a.kind == 1) {
    const float momentum = a.h1, wd = a.h3;
    if (wd != 0.f) g = g + wd * p;                      // grad.add(param, alpha=wd)
    if (momentum != 0.f) {
      float buf;
      if (a.first) {
        buf = g;                                        // torch.clone(grad)
      } else {
        buf = a.s1[i] * momentum;                       // buf.mul_(momentum)
        buf = buf + a.w1 * g;                           //    .add_(grad, alpha=1-damp)
      }
      a.s1[i] = buf;
      g = (a.flags & 1) ? g + momentum * buf : buf;     // nesterov
    }
    p = p + a.neg_lr * g;                               // param.add_(grad, alpha=-lr)
  } else if (a.kind == 2) {
    const float alpha = a.h1, eps = a.h2, wd = a.h3, momentum = a.h4;
    if (wd != 0.f) g = g + wd * p;
    float sq = a.s1[i] * alpha;                         // square_avg.mul_(alpha)
    sq = sq + (a.w1 * g) * g;                           //    .addcmul_(g, g, 1-alpha)
    a.s1[i] = sq;
    float avg;
    if (a.flags & 1) {
      float ga = a.s3[i];
      ga = fmaf(a.w1, g - ga, ga);                      // grad_avg.lerp_(g, 1-alpha)
      a.s3[i] = ga;
      avg = sqrtf(sq + (-1.f * ga) * ga);               // addcmul(ga, ga, -1).sqrt_()
    } else {
      avg = sqrtf(sq);
    }
    avg = avg + eps;
    if (momentum > 0.f) {
      float buf = a.s2[i] * momentum;                   // buf.mul_(momentum)
      buf = buf + g / avg;                              //    .addcdiv_(grad, avg)
      a.s2[i] = buf;
      p = p + a.neg_lr * buf;                           // add_(buf, alpha=-lr)
    } else {
      p = p + (a.neg_lr * g) / avg;                     // addcdiv_(grad, avg, -lr)
    }
  } else {
    const float beta2 = a.h2, eps = a.h3, wd = a.h4;
    if (a.flags & 2) {
      p = p * a.decay;                                  // AdamW: param.mul_(1 - lr wd)
    } else if (wd != 0.f) {
      g = g + wd * p;
    }
    float m = a.s1[i], v = a.s2[i];
    m = fmaf(a.w1, g - m, m);                           // exp_avg.lerp_(grad, 1-beta1)
    v = v * beta2 + (a.w2 * g) * g;
    a.s1[i] = m;
    a.s2[i] = v;
    float vv = v;
    if (a.flags & 1) {                                  // amsgrad
      vv = fmaxf(a.s3[i], v);
      a.s3[i] = vv;
    }
    const float denom = sqrtf(vv) / a.bc2_sqrt + eps;
    p = p + (a.neg_step_size * m) / denom;
  }
  a.p[i] = p;
}

// reduce_slabs_kernel + adam_kernel in one launch (single process: nothing has
// to happen between the slab sum and the optimizer step).  Same arithmetic and
// the same summation order as the two separate kernels.
__global__ __launch_bounds__(256) void reduce_adam_kernel(const float* slabs,
                                                          int64_t n_splits,
                                                          int64_t stride, int zero_slot0,
                                                          AdamParams a, float* grads) {
  __builtin_amdgcn_s_setprio(3);  // (see adam_kernel)
  __shared__ float4 part[4][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t i4 = ((int64_t)blockIdx.x * 64 + col) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i4 < a.n) {
    int64_t s = grp;
    for (; s + 12 < n_splits; s += 16) {
      const float4 v0 = *reinterpret_cast<const float4*>(slabs + s * stride + i4);
      const float4 v1 =
          *reinterpret_cast<const float4*>(slabs + (s + 4) * stride + i4);
      const float4 v2 =
          *reinterpret_cast<const float4*>(slabs + (s + 8) * stride + i4);
      const float4 v3 =
          *reinterpret_cast<const float4*>(slabs + (s + 12) * stride + i4);
      acc.x += (v0.x + v1.x) + (v2.x + v3.x);
      acc.y += (v0.y + v1.y) + (v2.y + v3.y);
      acc.z += (v0.z + v1.z) + (v2.z + v3.z);
      acc.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; s < n_splits; s += 4) {
      const float4 v = *reinterpret_cast<const float4*>(slabs + s * stride + i4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  part[grp][col] = acc;
  __syncthreads();
  if (grp != 0 || i4 >= a.n) return;
  const float4 pa = part[0][col], pb = part[1][col], pc = part[2][col],
               pd = part[3][col];
  float g[4] = {(pa.x + pb.x) + (pc.x + pd.x), (pa.y + pb.y) + (pc.y + pd.y),
                (pa.z + pb.z) + (pc.z + pd.z), (pa.w + pb.w) + (pc.w + pd.w)};
  if (zero_slot0 && i4 == 0) g[0] = 0.f;  // log-std slot of a fixed-std module
  *reinterpret_cast<float4*>(grads + i4) = make_float4(g[0], g[1], g[2], g[3]);
  float4 p4 = *reinterpret_cast<float4*>(a.p + i4);
  float4 m4 = *reinterpret_cast<float4*>(a.m + i4);
  float4 v4 = *reinterpret_cast<float4*>(a.v + i4);
  float pp[4] = {p4.x, p4.y, p4.z, p4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w},
        vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) ga_adam_update(a.c, g[j], pp[j], mm[j], vv[j]);
  *reinterpret_cast<float4*>(a.p + i4) = make_float4(pp[0], pp[1], pp[2], pp[3]);
  *reinterpret_cast<float4*>(a.m + i4) = make_float4(mm[0], mm[1], mm[2], mm[3]);
  *reinterpret_cast<float4*>(a.v + i4) = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

// ---- advantage statistics ---------------------------------------------------
// stats (device, double[4]): [0] sum, [1] count, [2] sum of squared deviations,
// [3] minimum.  Between the stages a multi-GPU caller all-reduces the slots.
template <int WHAT>  // 0: sum, 1: squared deviations from stats mean, 2: min
__global__ __launch_bounds__(256) void stats_partial_kernel(const float* x, int64_t n,
                                                            const double* stats,
                                                            double* partials) {
  __shared__ double red[4];
  double mean = 0.0;
  if (WHAT == 1) mean = stats[0] / stats[1];
  double acc = (WHAT == 2) ? 1.0e300 : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256) {
    const double v = (double)x[i];
    if (WHAT == 0) acc += v;
    if (WHAT == 1) acc += (v - mean) * (v - mean);
    if (WHAT == 2) acc = fmin(acc, v);
  }
  if (WHAT == 2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = fmin(acc, __shfl_down(acc, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      partials[blockIdx.x] = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
  } else {
    const double r = ga_block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;
  }
}

template <int WHAT>
__global__ void stats_finalize_kernel(const double* partials, int nblocks, int64_t n,
                                      double* stats) {
  if (WHAT == 2) {
    double a = 1.0e300;
    for (int k = threadIdx.x; k < nblocks; k += 64) a = fmin(a, partials[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmin(a, __shfl_down(a, o, 64));
    if (threadIdx.x == 0 && blockIdx.x == 0) stats[3] = a;
  } else {
    double a = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 64) a += partials[k];
    a = ga_wave_sum(a);
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (WHAT == 0) {
      stats[0] = a;
      stats[1] = (double)n;
    } else {
      stats[2] = a;
    }
  }
}

__global__ __launch_bounds__(256) void adv_center_kernel(float* x, int64_t n,
                                                         const double* stats,
                                                         float eps) {
  // (a - mean) / (var + 1e-8), unbiased variance, in fp32 like the reference
  const float mean = (float)(stats[0] / stats[1]);
  const float var = (float)(stats[2] / (stats[1] - 1.0));
  const float denom = var + eps;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    x[i] = (x[i] - mean) / denom;
}

__global__ __launch_bounds__(256) void sub_scalar_kernel(float* x, int64_t n,
                                                         const double* scalar) {
  const float s = (float)(*scalar);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * 256)
    x[i] -= s;
}

// ---- vector ops of the constrained (TRPO) policy step ------------------------------
// torch/optimizers/conjugate_gradient_optimizer.py:69-104,146-186 works on the flat
// parameter vector (~72 k floats at C3): dot products and axpy-type updates.

// one workgroup, fp64 accumulation in a fixed order: bitwise reproducible
static_assert(LS_DOT_THREADS == 1024, "dot_kernel adds up 16 waves");
__global__ __launch_bounds__(LS_DOT_THREADS) void dot_kernel(const float* a, const float* b,
                                                             int64_t n, double* out) {
  __shared__ double part[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += LS_DOT_THREADS)
    s += (double)a[i] * (double)b[i];
  s = ga_wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    *out = t;
  }
}

// y = alpha * x + beta * y  (fp32, one fma rounding like torch's addcmul-free form)
__global__ __launch_bounds__(256) void axpby_kernel(float alpha, const float* x,
                                                    float beta, float* y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = alpha * x[i] + beta * y[i];
}

// Gaussian metric seed of the Fisher-vector product: with old == new, the Hessian
// of mean_i KL(old || new) with respect to the means is 1 / (sigma^2 M)
// (kl_normal_normal: 0.5 ((mu_o - mu)^2 / sigma^2 + ...)), so
//   dout[i, j] = tmean[i, j] * exp(-2 s) / M.
__global__ __launch_bounds__(256) void fisher_seed_kernel(
    const float* tmean, int64_t ldt, int64_t M, int A, const float* log_std,
    int has_min, float min_log_std, int has_max, float max_log_std, float* dout,
    int64_t ldd) {
  const float s = ga_log_std(*log_std, has_min, min_log_std, has_max, max_log_std, nullptr);
  const float scale = expf(-2.f * s) / (float)M;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  for (int j = 0; j < (int)ldd; ++j)
    dout[i * ldd + j] = (j < A) ? tmean[i * ldt + j] * scale : 0.f;
}

// Categorical metric seed of the Fisher-vector product (TRPO with the categorical
// head).  With old == new the Hessian of mean_i KL(old || new) with respect to the
// LOGITS l of Categorical(logits=l) is (diag(q) - q q^T) / M, q = softmax(l)
// (the KL's gradient vanishes there, so no second-derivative term of the network
// enters: conjugate_gradient_optimizer.py:18-66 differentiates the same KL twice).
// The reference's head feeds l = softmax(scores) (categorical_cnn_policy.py:138-139,
// double_softmax), whose Jacobian J1 = diag(z) - z z^T is symmetric, so with the
// tangent t of the scores:
//   u = J1 t,  w = (diag(q) - q q^T) u,  dout = J1 w / M      (J1 = I without it).
// One thread per row, A <= FS_MAX_A classes in registers.
__global__ __launch_bounds__(256) void fisher_seed_categorical_kernel(
    const float* scores, int64_t lds, const float* tscores, int64_t ldt, int64_t M, int A,
    int double_softmax, float* dout, int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  float z[FS_MAX_A], q[FS_MAX_A], u[FS_MAX_A];
  float mx = scores[i * lds];
  for (int j = 1; j < A; ++j) mx = fmaxf(mx, scores[i * lds + j]);
  float den = 0.f;
  for (int j = 0; j < A; ++j) {
    z[j] = expf(scores[i * lds + j] - mx);
    den += z[j];
  }
  for (int j = 0; j < A; ++j) z[j] /= den;
  if (double_softmax) {
    float den2 = 0.f;
    for (int j = 0; j < A; ++j) {
      q[j] = expf(z[j]);  // z in (0, 1]: no shift needed
      den2 += q[j];
    }
    for (int j = 0; j < A; ++j) q[j] /= den2;
    float zt = 0.f;
    for (int j = 0; j < A; ++j) zt += z[j] * tscores[i * ldt + j];
    for (int j = 0; j < A; ++j) u[j] = z[j] * (tscores[i * ldt + j] - zt);
  } else {
    for (int j = 0; j < A; ++j) {
      q[j] = z[j];
      u[j] = tscores[i * ldt + j];
    }
  }
  float qu = 0.f;
  for (int j = 0; j < A; ++j) qu += q[j] * u[j];
  for (int j = 0; j < A; ++j) u[j] = q[j] * (u[j] - qu);  // w
  const float inv_m = 1.f / (float)M;
  if (double_softmax) {
    float zw = 0.f;
    for (int j = 0; j < A; ++j) zw += z[j] * u[j];
    for (int j = 0; j < A; ++j) u[j] = z[j] * (u[j] - zw);
  }
  for (int j = 0; j < (int)ldd; ++j) dout[i * ldd + j] = (j < A) ? u[j] * inv_m : 0.f;
}

// ---- head layer fused into the loss ------------------------------------------------
// In a minibatch step the network's last linear layer (hidden -> action means, or
// hidden -> value) feeds nothing but the loss.  These kernels compute it in the
// loss kernel: 16 lanes own one row of the last hidden activations (16-B loads, a
// whole row coalesced), the head weights sit in LDS, the A dot products are
// reduced over the 16 lanes with xor shuffles, and the per-row loss / gradient
// seed comes from the helpers of loss_rows.h, like ppo_gaussian_loss_kernel's and
// gaussian_nll_kernel's.
// One pass over the [rows x hidden] matrix replaces the narrow GEMM launch, the
// round trip of its output and the loss launch.  (HeadLayer: loss_params.h; the thread
// count, the rows per group and the LDS layout: shape_rules.h.)
static_assert(HL_GROUPS == 16, "group16_sum, and gl / rg below, are written for 16 groups of 16");

__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// Rows per 16-lane group and block iteration: all their loads are issued before
// any arithmetic (two dependent global-memory latencies per 64 rows: the gathered
// row ids, then everything else).
template <int KV>
struct HeadRows {
  static constexpr int R = ga_head_rows(KV);
  static_assert(R <= HL_ROWS_MAX, "ga_head_lds sizes the row buffers for HL_ROWS_MAX");
};

// Floats from smem to the row buffers: ga_head_lds's w + bias (shape_rules.h).  The kernels
// keep their own expression -- with the sum taken from the struct, the compiler orders three
// scalar instructions of head_ppo_gaussian_kernel differently -- and the static_assert ties
// the two at every shape ga_head_loss_rule admits.  (No outer parentheses: the kernels add
// the two terms to the pointer one after the other.)
#define HL_ROWS_AT(A, K) (A) * (K) + (((A) + 3) & ~3)
constexpr bool hl_rows_at_is_the_layout() {
  for (int K = 64; K <= 512; K *= 2)
    for (int A = 1; A <= 64; ++A)
      if ((HL_ROWS_AT(A, K)) != ga_head_lds(A, K).w + ga_head_lds(A, K).bias) return false;
  return true;
}
static_assert(hl_rows_at_is_the_layout(), "HL_ROWS_AT and ga_head_lds disagree");

// head outputs of one row from its activations h[KV] -> rowbuf[0..A) (LDS)
template <int KV>
__device__ __forceinline__ void head_row(const HeadLayer& L, int A, const float* wlds,
                                         const float4 (&h)[KV], int64_t row, bool live,
                                         int gl, float* rowbuf) {
  for (int a = 0; a < A; ++a) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      const float4 w =
          *reinterpret_cast<const float4*>(wlds + a * L.K + 4 * gl + 64 * v);
      s = fmaf(h[v].x, w.x, s);
      s = fmaf(h[v].y, w.y, s);
      s = fmaf(h[v].z, w.z, s);
      s = fmaf(h[v].w, w.w, s);
    }
    s = group16_sum(s) + wlds[A * L.K + a];
    if (gl == 0) {
      rowbuf[a] = s;
      if (L.out && live) L.out[row * L.ldo + a] = s;
    }
  }
}

// W[A][K] and bias[A] -> LDS
__device__ __forceinline__ void stage_head(const HeadLayer& L, int A, float* wlds) {
  for (int i = threadIdx.x; i < A * L.K / 4; i += HL_THREADS) {
    const int a = (4 * i) / L.K, k = (4 * i) % L.K;
    *reinterpret_cast<float4*>(wlds + 4 * i) =
        *reinterpret_cast<const float4*>(L.W + (int64_t)a * L.ldw + k);
  }
  for (int a = threadIdx.x; a < A; a += HL_THREADS) wlds[A * L.K + a] = L.bias[a];
}

template <int KV>
__global__ __launch_bounds__(HL_THREADS) void head_ppo_gaussian_kernel(HeadLayer L,
                                                                       PpoLossParams p) {
  constexpr int R = HeadRows<KV>::R;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wlds = smem;                                  // [A][K] + bias[A]
  float* rows = smem + HL_ROWS_AT(p.A, L.K);           // [16 groups][R][A]
  __shared__ double red[4];
  stage_head(L, p.A, wlds);
  __syncthreads();
  const float s = ga_log_std(*p.log_std, p.has_min, p.min_log_std, p.has_max,
                             p.max_log_std, nullptr);
  const float inv_var = expf(-2.f * s);
  const float lognorm = s + (float)HALF_LOG_2PI;
  const float invM = 1.f / (float)p.M;
  const int gl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  double obj_sum = 0.0, ds_sum = 0.0;
  // whole 16 R-row chunks so that every lane of a wave stays in the shuffles
  const int64_t n_chunk = (p.M + 16 * R - 1) / (16 * R);
  for (int64_t c = blockIdx.x; c < n_chunk; c += gridDim.x) {
    int64_t irow[R], src[R];
    bool live[R];
    float4 h[R][KV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      irow[r] = (c * R + r) * 16 + rg;
      live[r] = irow[r] < p.M;
      const int64_t row = live[r] ? irow[r] : p.M - 1;
      src[r] = p.idx ? (int64_t)p.idx[row] : row;
#pragma unroll
      for (int v = 0; v < KV; ++v)
        h[r][v] = *reinterpret_cast<const float4*>(L.H + row * L.ldh + 4 * gl + 64 * v);
    }
    float advr[R], oldr[R], actr[R][4];  // lane gl holds action dims gl, gl+16, ..
#pragma unroll
    for (int r = 0; r < R; ++r) {
      advr[r] = p.adv[src[r]];
      oldr[r] = (p.algo == 1) ? 0.f : p.old_ll[src[r]];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = gl + 16 * t;
        actr[r][t] = (j < p.A) ? p.actions[src[r] * p.lda + j] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float* rowbuf = rows + (rg * R + r) * p.A;
      const int64_t row = live[r] ? irow[r] : p.M - 1;
      head_row<KV>(L, p.A, wlds, h[r], row, live[r], gl, rowbuf);
      // the 16 lanes of a group are in one wave: lane 0's LDS writes become
      // visible to the group after the wave-level fence
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float ll_part = 0.f, q_part = 0.f, dj[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = gl + 16 * t;
        dj[t] = 0.f;
        if (j < p.A)
          dj[t] = lr_gauss_dim(actr[r][t], rowbuf[j], inv_var, lognorm, q_part, ll_part);
      }
      const float q = group16_sum(q_part);
      const float ll = group16_sum(ll_part);
      float g;
      const float obj = lr_surrogate(p.algo, p.clip, ll, oldr[r], advr[r], &g);
      if (live[r]) {
        if (p.ll_out && gl == 0) p.ll_out[irow[r]] = ll;
        if (p.dmean) {
          const float scale = -g * invM * inv_var;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int j = gl + 16 * t;
            if (j < p.A) p.dmean[irow[r] * p.ldm + j] = scale * dj[t];
          }
        }
        if (gl == 0) {
          obj_sum += (double)obj;
          ds_sum += (double)(-g * (q - (float)p.A));
        }
      }
    }
  }
  const double o = ga_block_sum_256(obj_sum, red);
  const double d = ga_block_sum_256(ds_sum, red);
  if (threadIdx.x == 0) {
    p.partials[2 * blockIdx.x + 0] = o;
    p.partials[2 * blockIdx.x + 1] = d;
  }
}

template <int KV>
__global__ __launch_bounds__(HL_THREADS) void head_gaussian_nll_kernel(HeadLayer L,
                                                                       NllParams p) {
  constexpr int R = HeadRows<KV>::R;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wlds = smem;                 // [1][K] + bias
  float* rows = smem + HL_ROWS_AT(1, L.K);  // [16 groups][R]
  __shared__ double red[4];
  stage_head(L, 1, wlds);
  __syncthreads();
  const float s = *p.log_std;
  const float inv_var = expf(-2.f * s);
  const float invM = 1.f / (float)p.M;
  const int gl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  double nll = 0.0, ds = 0.0;
  const int64_t n_chunk = (p.M + 16 * R - 1) / (16 * R);
  for (int64_t c = blockIdx.x; c < n_chunk; c += gridDim.x) {
    int64_t irow[R];
    bool live[R];
    float4 h[R][KV];
    float retr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      irow[r] = (c * R + r) * 16 + rg;
      live[r] = irow[r] < p.M;
      const int64_t row = live[r] ? irow[r] : p.M - 1;
      const int64_t src = p.idx ? (int64_t)p.idx[row] : row;
#pragma unroll
      for (int v = 0; v < KV; ++v)
        h[r][v] = *reinterpret_cast<const float4*>(L.H + row * L.ldh + 4 * gl + 64 * v);
      retr[r] = p.returns[src];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float* rowbuf = rows + rg * R + r;
      const int64_t row = live[r] ? irow[r] : p.M - 1;
      head_row<KV>(L, 1, wlds, h[r], row, live[r], gl, rowbuf);
      if (live[r] && gl == 0) {
        float dsi, dvi;
        nll += (double)lr_nll_row(retr[r], rowbuf[0], s, inv_var, invM, &dsi, &dvi);
        ds += (double)dsi;
        if (p.dv) p.dv[irow[r] * p.ldv] = dvi;
      }
    }
  }
  const double a = ga_block_sum_256(nll, red);
  const double b = ga_block_sum_256(ds, red);
  if (threadIdx.x == 0) {
    p.partials[2 * blockIdx.x + 0] = a;
    p.partials[2 * blockIdx.x + 1] = b;
  }
}

// ---- the member-indexed twins (members_diag.h) ---------------------------------------------
// Row kernels: entry blockIdx.y of a device table, the lone kernel's body
// (loss_row_bodies.inc) with the entry's own block count.  A members launch never takes the
// single-launch finish: its host side asks for partials whenever an entry has more than one
// block, and a one-block entry finishes itself as the lone kernel does.  They stay in this
// file because the helpers the bodies call do.
#undef GA_GRID_X
#define GA_GRID_X md_entry.nb
__global__ __launch_bounds__(256) void ppo_gaussian_loss_members_kernel(
    const MdPpoEntry* table) {
  const MdPpoEntry md_entry = table[blockIdx.y];
  if (blockIdx.x >= md_entry.nb) return;
  const PpoLossParams& p = md_entry.p;
#define GA_LOSS_BODY 1
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}
__global__ __launch_bounds__(256) void ppo_categorical_loss_members_kernel(
    const MdCatEntry* table) {
  const MdCatEntry md_entry = table[blockIdx.y];
  if (blockIdx.x >= md_entry.nb) return;
  const CatLossParams& p = md_entry.p;
#define GA_LOSS_BODY 2
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}
__global__ __launch_bounds__(256) void gaussian_nll_members_kernel(const MdNllEntry* table) {
  const MdNllEntry md_entry = table[blockIdx.y];
  if (blockIdx.x >= md_entry.nb) return;
  const NllParams& p = md_entry.p;
#define GA_LOSS_BODY 4
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}
__global__ __launch_bounds__(256) void categorical_kl_members_kernel(const MdKlEntry* table) {
  const MdKlEntry md_entry = table[blockIdx.y];
  if (blockIdx.x >= md_entry.nb) return;
  const float* sc_old = md_entry.head_old;
  const float* sc_new = md_entry.head_new;
  const int64_t ld = md_entry.ld, M = md_entry.M;
  const int A = md_entry.A, dbl = md_entry.dbl;
  double* partials = md_entry.partials;
#define GA_LOSS_BODY 3
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}
__global__ __launch_bounds__(256) void gaussian_kl_members_kernel(const MdKlEntry* table) {
  const MdKlEntry md_entry = table[blockIdx.y];
  if (blockIdx.x >= md_entry.nb) return;
  const float* mean_old = md_entry.head_old;
  const float* mean_new = md_entry.head_new;
  const int64_t ld = md_entry.ld, M = md_entry.M;
  const int A = md_entry.A;
  const float s_old = md_entry.s_old, s_new = md_entry.s_new;
  double* partials = md_entry.partials;
#define GA_LOSS_BODY 5
#include "loss_row_bodies.inc"
#undef GA_LOSS_BODY
}
#undef GA_GRID_X
// The fixed-order sums, one wave per entry (blockIdx.x): the lone finalize kernels' loops
// and the same finish.  fp64 additions in the same order: the same bits.
__global__ void ppo_gaussian_finalize_members_kernel(const PpoFinalizeParams* table) {
  const PpoFinalizeParams p = table[blockIdx.x];
  double obj = 0.0, ds = 0.0;
  for (int b = threadIdx.x; b < p.nblocks; b += 64) {
    obj += p.partials[2 * b + 0];
    ds += p.partials[2 * b + 1];
  }
  obj = ga_wave_sum(obj);
  ds = ga_wave_sum(ds);
  if (threadIdx.x != 0) return;
  ppo_gaussian_finish(obj, ds, p.log_std, p.has_min, p.min_log_std, p.has_max,
                      p.max_log_std, p.M, p.A, p.ent, p.loss_out, p.grad_slab0,
                      p.slab_stride, p.n_splits);
}
__global__ void ppo_categorical_finalize_members_kernel(const MdCatFinalize* table) {
  const MdCatFinalize p = table[blockIdx.x];
  double o = 0.0, e = 0.0;
  for (int b = threadIdx.x; b < p.nblocks; b += 64) {
    o += p.partials[2 * b];
    e += p.partials[2 * b + 1];
  }
  o = ga_wave_sum(o);
  e = ga_wave_sum(e);
  if (threadIdx.x != 0) return;
  *p.loss_out = (float)(-(o / (double)p.M));
  if (p.ent_sum_out) *p.ent_sum_out = e;
}
__global__ void gaussian_nll_finalize_members_kernel(const MdNllFinalize* table) {
  const MdNllFinalize p = table[blockIdx.x];
  double a = 0.0;
  for (int k = threadIdx.x; k < p.nblocks; k += 64) a += p.partials[2 * k];
  a = ga_wave_sum(a);
  if (threadIdx.x != 0) return;
  *p.loss_out = (float)(a / (double)p.M);
}
__global__ void sum_partials_members_kernel(const MdSum* table) {
  const MdSum p = table[blockIdx.x];
  double a = 0.0;
  for (int k = threadIdx.x; k < p.nblocks; k += 64) a += p.partials[k];
  a = ga_wave_sum(a);
  if (threadIdx.x == 0) *p.out = a;
}

}  // namespace

// ---- the members' launch seam (members_diag.h) ---------------------------------------------
#define MD_LAUNCH(name, kernel, grid, threads, table)                        \
  do {                                                                       \
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, stream, table);       \
    GA_CHECK_LAUNCH(name);                                                   \
    return GA_OK;                                                            \
  } while (0)
int md_launch_ppo_gaussian_members(const MdPpoEntry* table, unsigned n, unsigned blocks,
                                   hipStream_t stream) {
  MD_LAUNCH("ppo_gaussian_loss_members", ppo_gaussian_loss_members_kernel, dim3(blocks, n),
            256, table);
}
int md_launch_ppo_gaussian_finalize_members(const PpoFinalizeParams* table, unsigned n,
                                            hipStream_t stream) {
  MD_LAUNCH("ppo_gaussian_finalize_members", ppo_gaussian_finalize_members_kernel, dim3(n), 64,
            table);
}
int md_launch_ppo_categorical_members(const MdCatEntry* table, unsigned n, unsigned blocks,
                                      hipStream_t stream) {
  MD_LAUNCH("ppo_categorical_loss_members", ppo_categorical_loss_members_kernel,
            dim3(blocks, n), 256, table);
}
int md_launch_ppo_categorical_finalize_members(const MdCatFinalize* table, unsigned n,
                                               hipStream_t stream) {
  MD_LAUNCH("ppo_categorical_finalize_members", ppo_categorical_finalize_members_kernel,
            dim3(n), 64, table);
}
int md_launch_nll_members(const MdNllEntry* table, unsigned n, unsigned blocks,
                          hipStream_t stream) {
  MD_LAUNCH("gaussian_nll_members", gaussian_nll_members_kernel, dim3(blocks, n), 256, table);
}
int md_launch_nll_finalize_members(const MdNllFinalize* table, unsigned n,
                                   hipStream_t stream) {
  MD_LAUNCH("gaussian_nll_finalize_members", gaussian_nll_finalize_members_kernel, dim3(n), 64,
            table);
}
int md_launch_kl_members(int categorical, const MdKlEntry* table, unsigned n, unsigned blocks,
                         hipStream_t stream) {
  if (categorical)
    MD_LAUNCH("categorical_kl_members", categorical_kl_members_kernel, dim3(blocks, n), 256, table);
  MD_LAUNCH("gaussian_kl_members", gaussian_kl_members_kernel, dim3(blocks, n), 256, table);
}
int md_launch_sum_members(const MdSum* table, unsigned n, hipStream_t stream) {
  MD_LAUNCH("sum_partials_members", sum_partials_members_kernel, dim3(n), 64, table);
}
#undef MD_LAUNCH

// ---- the launch seam (loss_params.h): instantiate and launch, nothing else ----------------
#define LS_LAUNCH(kernel, blocks, threads, lds, ...) \
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, __VA_ARGS__)

void ls_launch_ppo_gaussian_loss(const PpoLossParams& p, unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(ppo_gaussian_loss_kernel, blocks, 256, 0, p);
}
void ls_launch_ppo_gaussian_finalize(const PpoFinalizeParams& f, hipStream_t stream) {
  LS_LAUNCH(ppo_gaussian_finalize_kernel, 1, 64, 0, f);
}
void ls_launch_ppo_categorical_loss(const CatLossParams& p, unsigned blocks,
                                    hipStream_t stream) {
  LS_LAUNCH(ppo_categorical_loss_kernel, blocks, 256, 0, p);
}
void ls_launch_ppo_categorical_finalize(const double* partials, int nblocks, int64_t M,
                                        float* loss_out, double* ent_sum_out,
                                        float* grad_slab0, int64_t slab_stride,
                                        int64_t n_splits, hipStream_t stream) {
  LS_LAUNCH(ppo_categorical_finalize_kernel, 1, 64, 0, partials, nblocks, M, loss_out,
            ent_sum_out, grad_slab0, slab_stride, n_splits);
}
void ls_launch_gaussian_nll(const NllParams& p, unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(gaussian_nll_kernel, blocks, 256, 0, p);
}
void ls_launch_gaussian_nll_finalize(const double* partials, int nblocks, int64_t M,
                                     float* loss_out, float* grad_slab0,
                                     int64_t slab_stride, int64_t n_splits,
                                     hipStream_t stream) {
  LS_LAUNCH(gaussian_nll_finalize_kernel, 1, 64, 0, partials, nblocks, M, loss_out,
            grad_slab0, slab_stride, n_splits);
}
void ls_launch_categorical_kl(const float* sc_old, const float* sc_new, int64_t ld, int64_t M,
                              int A, int dbl, double* partials, unsigned blocks,
                              hipStream_t stream) {
  LS_LAUNCH(categorical_kl_kernel, blocks, 256, 0, sc_old, sc_new, ld, M, A, dbl, partials);
}
void ls_launch_gaussian_kl(const float* mean_old, const float* mean_new, int64_t ld,
                           int64_t M, int A, float s_old, float s_new, double* partials,
                           unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(gaussian_kl_kernel, blocks, 256, 0, mean_old, mean_new, ld, M, A, s_old, s_new,
            partials);
}
void ls_launch_sum_partials(const double* partials, int nblocks, double* out,
                            hipStream_t stream) {
  LS_LAUNCH(sum_partials_kernel, 1, 64, 0, partials, nblocks, out);
}
void ls_launch_reduce_slabs(const float* slabs, int64_t n_splits, int64_t stride, int64_t n,
                            float* out, float scale, unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(reduce_slabs_kernel, blocks, 256, 0, slabs, n_splits, stride, n, out, scale);
}
void ls_launch_reduce_adam(const float* slabs, int64_t n_splits, int64_t stride,
                           int zero_slot0, const AdamParams& a, float* grads, unsigned blocks,
                           hipStream_t stream) {
  LS_LAUNCH(reduce_adam_kernel, blocks, 256, 0, slabs, n_splits, stride, zero_slot0, a,
            grads);
}
void ls_launch_adam(const AdamParams& a, unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(adam_kernel, blocks, 256, 0, a);
}
void ls_launch_optimizer_step(const OptParams& a, unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(optimizer_step_kernel, blocks, 256, 0, a);
}
template <int WHAT>
static void stats_pair(const float* x, int64_t n, double* stats, double* partials,
                       unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(stats_partial_kernel<WHAT>, blocks, 256, 0, x, n, (const double*)stats,
            partials);
  LS_LAUNCH(stats_finalize_kernel<WHAT>, 1, 64, 0, (const double*)partials, (int)blocks, n,
            stats);
}
void ls_launch_stats(int what, const float* x, int64_t n, double* stats, double* partials,
                     unsigned blocks, hipStream_t stream) {
  switch (what) {
    case 0: stats_pair<0>(x, n, stats, partials, blocks, stream); break;
    case 1: stats_pair<1>(x, n, stats, partials, blocks, stream); break;
    default: stats_pair<2>(x, n, stats, partials, blocks, stream); break;
  }
}
void ls_launch_adv_center(float* x, int64_t n, const double* stats, float eps,
                          unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(adv_center_kernel, blocks, 256, 0, x, n, stats, eps);
}
void ls_launch_sub_scalar(float* x, int64_t n, const double* scalar, unsigned blocks,
                          hipStream_t stream) {
  LS_LAUNCH(sub_scalar_kernel, blocks, 256, 0, x, n, scalar);
}
void ls_launch_dot(const float* a, const float* b, int64_t n, double* out, unsigned blocks,
                   hipStream_t stream) {
  LS_LAUNCH(dot_kernel, blocks, LS_DOT_THREADS, 0, a, b, n, out);
}
void ls_launch_axpby(float alpha, const float* x, float beta, float* y, int64_t n,
                     unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(axpby_kernel, blocks, 256, 0, alpha, x, beta, y, n);
}
void ls_launch_fisher_seed_gaussian(const float* tmean, int64_t ldt, int64_t M, int A,
                                    const float* log_std, int has_min, float min_log_std,
                                    int has_max, float max_log_std, float* dout, int64_t ldd,
                                    unsigned blocks, hipStream_t stream) {
  LS_LAUNCH(fisher_seed_kernel, blocks, 256, 0, tmean, ldt, M, A, log_std, has_min,
            min_log_std, has_max, max_log_std, dout, ldd);
}
void ls_launch_fisher_seed_categorical(const float* scores, int64_t lds, const float* tscores,
                                       int64_t ldt, int64_t M, int A, int double_softmax,
                                       float* dout, int64_t ldd, unsigned blocks,
                                       hipStream_t stream) {
  LS_LAUNCH(fisher_seed_categorical_kernel, blocks, 256, 0, scores, lds, tscores, ldt, M, A,
            double_softmax, dout, ldd);
}
// one instantiation per hidden width: KV = L.K / 64 of 1, 2, 4, 8 (ga_head_loss_rule)
#define LS_HEAD_LAUNCH(kernel)                                                     \
  switch (L.K / 64) {                                                              \
    case 1: LS_LAUNCH(kernel<1>, blocks, HL_THREADS, lds_bytes, L, p); break;      \
    case 2: LS_LAUNCH(kernel<2>, blocks, HL_THREADS, lds_bytes, L, p); break;      \
    case 4: LS_LAUNCH(kernel<4>, blocks, HL_THREADS, lds_bytes, L, p); break;      \
    default: LS_LAUNCH(kernel<8>, blocks, HL_THREADS, lds_bytes, L, p); break;     \
  }
void ls_launch_head_ppo_gaussian(const HeadLayer& L, const PpoLossParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t stream) {
  LS_HEAD_LAUNCH(head_ppo_gaussian_kernel)
}
void ls_launch_head_gaussian_nll(const HeadLayer& L, const NllParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t stream) {
  LS_HEAD_LAUNCH(head_gaussian_nll_kernel)
}
