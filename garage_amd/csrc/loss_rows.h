// Per-row loss arithmetic of the PPO / VPG / TRPO update, the ONE copy of it: the
// stand-alone loss kernels (losses.hip), the one-launch small-minibatch step
// (small_step.hip) and the kernels that compute the loss inside a GEMM epilogue
// (fused_train.hip, narrow_step.hip) all call these, so every path rounds the same
// operations in the same order:
//   gaussian policy   PPO._compute_objective (torch/algos/ppo.py:96-132) /
//                     VPG._compute_objective (vpg.py:434-454) on an
//                     Independent(Normal(mean, exp(log_std))) with a scalar,
//                     clamped log-std (torch/modules/gaussian_mlp_module.py:158-192)
//   categorical       the same objectives on Categorical(logits = softmax(scores)),
//                     the convention of the reference's torch categorical policies
//                     (torch/policies/categorical_cnn_policy.py:138-139; Q15)
//   value function    GaussianMLPValueFunction.compute_loss
//                     (torch/value_functions/gaussian_mlp_value_function.py:81-98)
// The scalar helpers serve kernels with any loop shape; lr_row / lr_finish are the
// whole row / batch finish for heads of <= 8 outputs.  The order of the batch sums
// is each caller's own.
#pragma once
#include "common.h"
#include "fused_train.h"
#include "loss_args.h"

namespace {

constexpr double HALF_LOG_2PI = 0.91893853320467274178;

// (LossEnt, lr_ent, LossRowArgs and loss_args(): loss_args.h, which host C++ compiles too)

// F.softplus (beta 1, threshold 20, torch's default); *slope <- its derivative
__device__ __forceinline__ float lr_softplus(float x, float* slope) {
  *slope = 1.f / (1.f + expf(-x));
  return x > 20.f ? x : log1pf(expf(x));
}

// The objective of a row from its log-likelihood, and *g = d obj / d ll:
//   algo 0  PPO clipped surrogate (ppo.py:119-132); torch.min backward gives the
//           smaller input the gradient and splits ties
//   algo 1  VPG, ll * adv (old_ll is not read)
//   algo 2  TRPO, likelihood ratio times advantage (torch/algos/trpo.py:113-117)
__device__ __forceinline__ float lr_surrogate(int algo, float clip, float ll, float old_ll,
                                              float adv, float* g) {
  float obj;
  if (algo == 1) {
    obj = ll * adv;
    *g = adv;
  } else if (algo == 2) {
    const float ratio = expf(ll - old_ll);
    obj = ratio * adv;
    *g = obj;
  } else {
    const float ratio = expf(ll - old_ll);
    const float lo = 1.f - clip, hi = 1.f + clip;
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * adv, s2 = rc * adv;
    obj = fminf(s1, s2);
    const float g1 = adv * ratio;                                       // via surr
    const float g2 = (ratio >= lo && ratio <= hi) ? adv * ratio : 0.f;  // via clip
    *g = (s1 < s2) ? g1 : ((s1 > s2) ? g2 : 0.5f * (g1 + g2));
  }
  return obj;
}

// One action dimension of the Gaussian log-likelihood (lognorm = s + log sqrt(2 pi)):
// z = (a - mu)^2 / var goes into q, the dimension's log-density into ll; returns a - mu
__device__ __forceinline__ float lr_gauss_dim(float a, float mu, float inv_var,
                                              float lognorm, float& q, float& ll) {
  const float d = a - mu;
  const float z = d * d * inv_var;
  q += z;
  ll += -0.5f * z - lognorm;
  return d;
}

// One row of the value function's Gaussian NLL: returns the row's NLL; *ds <- its
// d/ds term, *dv <- d(loss)/dv (already / M)
__device__ __forceinline__ float lr_nll_row(float ret, float v, float s, float inv_var,
                                            float invM, float* ds, float* dv) {
  const float d = ret - v;
  const float z = d * d * inv_var;
  *ds = 1.f - z;
  *dv = -d * inv_var * invM;
  return 0.5f * z + s + (float)HALF_LOG_2PI;
}

// d obj / d lp_j of a categorical row with entropy H (cH: the entropy term's
// coefficient): g (1[j = a] - q_j) - cH q_j (lp_j + H), q_j = exp(lp_j)
__device__ __forceinline__ float lr_cat_grad(float g, float cH, float lp, float H,
                                             bool taken) {
  const float q = expf(lp);
  return g * ((taken ? 1.f : 0.f) - q) - cH * q * (lp + H);
}

// Gaussian policy row: returns the objective; dout[j < A] <- d(loss)/d(out_j)
// (already / M), *second <- the row's term of the log-std gradient numerator
__device__ __forceinline__ float lr_gauss_row(int algo, float clip, int A, float s,
                                              float inv_var, float invM,
                                              const float (&out)[8], const float (&act)[8],
                                              float adv, float old_ll, float (&dout)[8],
                                              float* second) {
  const float lognorm = s + (float)HALF_LOG_2PI;
  float ll = 0.f, q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < A) lr_gauss_dim(act[j], out[j], inv_var, lognorm, q, ll);
  float g;
  const float obj = lr_surrogate(algo, clip, ll, old_ll, adv, &g);
  const float scale = -g * invM * inv_var;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < A) dout[j] = scale * (act[j] - out[j]);
  // d ll / d s = sum_j ((a-mu)^2/var - 1)
  *second = -g * (q - (float)A);
  return obj;
}

// Categorical policy row (scores out[0..A), taken class cls): returns the objective
// (entropy term included); dout[j < A] <- d(loss)/d(out_j) (already / M), *Hs <- the
// row's entropy (after softplus when set)
__device__ __forceinline__ float lr_cat_row(int algo, float clip, const LossEnt& e,
                                            int double_softmax, int A, float invM,
                                            const float (&out)[8], int cls, float adv,
                                            float old_ll, float (&dout)[8], float* Hs) {
  float mx = out[0];
#pragma unroll
  for (int j = 1; j < 8; ++j)
    if (j < A) mx = fmaxf(mx, out[j]);
  float den = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < A) den += expf(out[j] - mx);
  float lse;
  if (!double_softmax) {
    lse = mx + logf(den);  // lp[j] = out[j] - lse
  } else {
    // logits' = p in [0,1]: logsumexp without a shift is safe
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < A) s2 += expf(expf(out[j] - mx) / den);
    lse = logf(s2);        // lp[j] = p[j] - lse
  }
  float pr[8], lp[8];
  float ll = 0.f, H = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    pr[j] = 0.f; lp[j] = 0.f;
    if (j < A) {
      pr[j] = expf(out[j] - mx) / den;
      lp[j] = (double_softmax ? pr[j] : out[j]) - lse;
      H -= expf(lp[j]) * lp[j];
      if (j == cls) ll = lp[j];
    }
  }
  float dHs = 1.f;
  *Hs = H;
  if (e.softplus) *Hs = lr_softplus(H, &dHs);
  float g;
  float obj = lr_surrogate(algo, clip, ll, old_ll, adv, &g);
  if (e.regularized) obj += e.coeff * *Hs;
  const float cH = (e.regularized && !e.stop_grad) ? e.coeff * dHs : 0.f;
  // double_softmax: chain through p = softmax(scores), dz_k = p_k (dp_k - sum_j dp_j p_j)
  float dp[8];
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    dp[j] = 0.f;
    if (j < A) {
      dp[j] = lr_cat_grad(g, cH, lp[j], H, j == cls);
      dot += dp[j] * pr[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < A)
      dout[j] = double_softmax ? -(pr[j] * (dp[j] - dot)) * invM : -dp[j] * invM;
  return obj;
}

// One row.  out[8]: the head outputs of the row; act[8] / adv / old_ll / ret: the
// row's sample (already gathered).  dout[8] <- d(loss)/d(out) (zero beyond A);
// returns the row's term of the first batch sum (objective, or NLL) and, through
// *second, of the second one (log-std gradient numerator; entropy for categorical).
__device__ __forceinline__ double lr_row(const LossRowArgs& a, float s, float inv_var,
                                         const float (&out)[8], const float (&act)[8],
                                         float adv, float old_ll, float ret,
                                         float (&dout)[8], double* second) {
#pragma unroll
  for (int j = 0; j < 8; ++j) dout[j] = 0.f;
  if (a.kind == 0) {
    float sec;
    const float obj = lr_gauss_row(a.algo, a.clip, a.A, s, inv_var, a.invM, out, act, adv,
                                   old_ll, dout, &sec);
    *second = (double)sec;
    return (double)obj;
  }
  if (a.kind == 1) {
    float ds;
    const float nll = lr_nll_row(ret, out[0], s, inv_var, a.invM, &ds, &dout[0]);
    *second = (double)ds;
    return (double)nll;
  }
  float Hs;
  const float obj = lr_cat_row(a.algo, a.clip, a.ent, a.double_softmax, a.A, a.invM, out,
                               (int)act[0], adv, old_ll, dout, &Hs);
  *second = (double)Hs;
  return (double)obj;
}

// The Gaussian policy's batch scalars from its two batch sums: the loss and
// d(loss)/d(log-std parameter).  s: the clamped log std, chain: d s / d parameter
// (ga_log_std; 0 where the clamp is active, and then so is the gradient).
__device__ __forceinline__ void lr_gaussian_finish(const LossEnt& e, int A, float s,
                                                   float chain, double first,
                                                   double second, int64_t M, float* loss,
                                                   float* dlogstd) {
  double mean_obj = first / (double)M;
  double dls = second / (double)M;  // d(-mean obj)/ds through the likelihood
  if (e.regularized) {
    // Independent Normal entropy: A * (0.5 + 0.5 log 2pi + s), state independent
    float ent = (float)A * (0.5f + (float)HALF_LOG_2PI + s);
    float dent = (float)A;
    if (e.softplus) {
      float slope;
      ent = lr_softplus(ent, &slope);
      dent *= slope;
    }
    mean_obj += (double)(e.coeff * ent);
    if (!e.stop_grad) dls += -(double)(e.coeff * dent);
  }
  *loss = (float)(-mean_obj);
  *dlogstd = chain != 0.f ? (float)dls * chain : 0.f;
}

// The batch scalars from the batch sums of lr_row (the finalize step): loss value and
// d(loss)/d(log_std) (0 where the clamp is active or the kind has no log-std
// parameter).
__device__ __forceinline__ void lr_finish(const LossRowArgs& a, double first, double second,
                                          int64_t M, float* loss, float* dlogstd) {
  if (a.kind == 2) {
    *loss = (float)(-(first / (double)M));
    *dlogstd = 0.f;
    return;
  }
  float s = *a.log_std;
  if (a.kind == 1) {
    *loss = (float)(first / (double)M);
    *dlogstd = (float)(second / (double)M);
    return;
  }
  float chain;
  s = ga_log_std(s, a.has_min, a.min_log_std, a.has_max, a.max_log_std, &chain);
  lr_gaussian_finish(a.ent, a.A, s, chain, first, second, M, loss, dlogstd);
}

}  // namespace
