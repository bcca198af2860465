// The natural-gradient (TRPO) step of a POPULATION of narrow networks: the device tables
// and the launch seam between the host side (members_natural_host.cpp) and the kernels
// (members_natural.hip).  Not part of the C ABI: ga_members_natural_* is what callers see.
// Host C++ (no device code), so that the CPU harness under tests/host can build
// members_natural_host.cpp against it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "shape_rules.h"

// A member's vectors of round4(n_flat) floats in the workspace: vector v of member m lies
// at vectors + (v * n_members + m) * round4(n_flat).
enum GaNaturalVec {
  NG_GRAD = 0, NG_X = 1, NG_R = 2, NG_P = 3, NG_Z = 4, NG_DESCENT = 5, NG_PREV = 6,
  NG_VECS = 7
};
// ... and its doubles: scalars + NG_SCALARS * m
enum GaNaturalScalar {
  NG_RDOTR = 0, NG_SAS = 1, NG_STEP = 2, NG_LOSS_BEFORE = 3, NG_DONE = 4, NG_ITERS = 5,
  NG_SCALARS = 8
};
// passes of narrow_natural_members_kernel
enum GaNaturalMode { NG_MODE_GRAD = 0, NG_MODE_FVP = 1, NG_MODE_EVAL = 2 };
// entries of members_cg_kernel
enum GaCgMode { NG_CG_BEGIN = 0, NG_CG_STEP = 1, NG_CG_FINISH = 2, NG_CG_PRODUCT = 3 };
// ga_member_natural.state
enum GaNaturalState { NG_SEARCHING = 0, NG_ACCEPTED = 1, NG_REJECTED = 2 };

// One member, as the kernels read it (device table [n_members]).
struct GaNaturalDev {
  float* params;
  const float* X; int64_t ldx;
  const float* actions; int64_t lda;
  const float* old_ll; const float* adv;
  const float* vec;   // NG_CG_PRODUCT / the product of caller-given vectors: tangent in
  float* out;         // ... and product out
  float* vectors;     // vector 0 of this member (stride between vectors: vec_stride)
  double* scalars;    // [NG_SCALARS]
  float* part;        // [shares][ga_narrow_step_stride]: gradient shares
  double* lpart;      // [shares][2]: loss sums (MODE_GRAD), loss and KL sums (MODE_EVAL)
  float* heads;       // [S][NS_HN]: head outputs of the step's starting point
  double* result;     // [2]: loss and KL of a candidate
  int32_t S, state;
  float inv_S;        // 1 / S, rounded once
  float ent_coeff;
  float delta, reg;   // max_constraint_value, hvp_reg_coeff
  float neg_ratio;    // -backtrack_ratio^k of this round
  int32_t pad_;
};

// What the members share
struct GaNaturalShared {
  int64_t w_off[3], b_off[3];
  int32_t in_w, H, out_w;
  int32_t kind, ent_flags, has_min, has_max;
  float min_log_std, max_log_std;
  int32_t double_softmax, zero_slot0;
  int64_t stride;      // ga_narrow_step_stride(in_w, H)
  int64_t n_flat;
  int64_t vec_stride;  // floats between two vectors of one member
  int32_t n_members;
  int32_t vec_sel;       // MODE_FVP's tangent: a GaNaturalVec, or -1: the member's `vec`
  int32_t respect_done;  // skip members whose conjugate gradient has finished
  int32_t pad_;
};

// The split of a member's rows among workgroups, a function of S alone: `shares`
// workgroups, workgroup g takes the 64-row tiles [g * tiles / shares, (g + 1) * tiles /
// shares).
inline int64_t ga_natural_tiles(int64_t S) { return (S + NS_ROWS - 1) / NS_ROWS; }
inline int ga_natural_shares(int64_t S) {
  const int64_t t = ga_natural_tiles(S);
  return (int)(t < NG_SHARES ? t : NG_SHARES);
}

extern "C" {
// narrow_natural_members_kernel<H, NS_LDX, mode>: grid (NG_SHARES, n_members)
int ga_members_natural_launch(const GaNaturalShared* sh, const GaNaturalDev* table_dev,
                              int mode, hipStream_t stream);
// members_cg_kernel: grid (n_members)
int ga_members_cg_launch(const GaNaturalShared* sh, const GaNaturalDev* table_dev, int mode,
                         hipStream_t stream);
// members_candidate_kernel: `prev` back into the parameters of the rejected members (a
// searching member's candidate, prev + neg_ratio * descent, is composed by MODE_EVAL while
// it stages the weights; the member's first workgroup stores it)
int ga_members_candidate_launch(const GaNaturalShared* sh, const GaNaturalDev* table_dev,
                                hipStream_t stream);
// members_eval_finish_kernel: each member's loss and KL from its workgroups' sums
int ga_members_eval_finish_launch(const GaNaturalShared* sh, const GaNaturalDev* table_dev,
                                  hipStream_t stream);
// members_natural_host.cpp: waits for what is in flight and frees the table slots (tests)
void ga_members_natural_release(void);
}
