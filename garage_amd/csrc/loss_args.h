// What a kernel is told about the loss of a minibatch (loss_rows.h holds the arithmetic):
// the argument struct the kernels' parameter structs embed, and its filling from the
// epoch loop's arguments.  Host-compilable (no device code beyond a __host__ __device__
// one-liner), so that the host side of the fused step (fused_train_host.cpp) builds for
// the CPU harnesses under tests/host as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "fused_train.h"

// The entropy options of the policy objective
struct LossEnt {
  float coeff;  // added to the objective when regularized
  int regularized, softplus, stop_grad;
};

// ent_flags of the C ABI: bit 0 regularized, bit 1 softplus, bit 2 stop gradient
__host__ __device__ inline LossEnt lr_ent(float coeff, int ent_flags) {
  LossEnt e;
  e.coeff = coeff;
  e.regularized = ent_flags & 1;
  e.softplus = (ent_flags >> 1) & 1;
  e.stop_grad = (ent_flags >> 2) & 1;
  return e;
}

struct LossRowArgs {
  int kind;                  // 0 Gaussian policy, 1 value NLL, 2 categorical policy
  const float* actions;      // [*, lda] gathered through idx
  int64_t lda;
  const float* old_ll;       // gathered through idx (algo 0)
  const float* adv;          // gathered through idx
  const float* returns;      // gathered through idx (kind 1)
  const int32_t* idx;        // row m of the minibatch is sample idx[m] (null: m)
  const float* log_std;      // device scalar parameter (kinds 0, 1)
  int has_min, has_max;
  float min_log_std, max_log_std;
  int A;                     // head width
  int algo;                  // 0 PPO clipped surrogate, 1 VPG (2 TRPO: not here)
  float clip;
  LossEnt ent;
  int double_softmax;
  float invM;
};

// LossRowArgs from the epoch loop's arguments (host)
inline LossRowArgs loss_args(const ga_fused_loss_args* l, int64_t M) {
  LossRowArgs L;
  memset(&L, 0, sizeof(L));
  L.kind = l->kind; L.actions = l->actions; L.lda = l->lda; L.old_ll = l->old_ll;
  L.adv = l->adv; L.returns = l->returns; L.idx = l->idx; L.log_std = l->log_std;
  L.has_min = l->has_min; L.has_max = l->has_max; L.min_log_std = l->min_log_std;
  L.max_log_std = l->max_log_std; L.A = l->A; L.algo = l->algo; L.clip = l->clip;
  L.ent = lr_ent(l->ent_coeff, l->ent_flags);
  L.double_softmax = l->double_softmax;
  L.invM = 1.f / (float)M;
  return L;
}
