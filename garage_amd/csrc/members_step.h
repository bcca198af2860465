// The two launches of one optimizer step of a POPULATION of narrow networks
// (members_step.hip) and the device tables they read, used by the members' epoch loop
// (update_members.cpp).  Not part of the C ABI: ga_update_epoch_members is what callers
// see.  Host C++ (no device code), so that the CPU harness under tests/host can build
// update_members.cpp against it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

// One member of the population, as the kernels read it (device table [n_members]).
// Step k of the pass works on ids [k * mb, k * mb + M_k) of `perm`, M_k = mb for
// k < n_steps - 1 and last_M for k = n_steps - 1; a member with k >= n_steps is
// inactive in step k: neither launch touches its memory.
struct GaMemberDev {
  float* params; float* grads; float* exp_avg; float* exp_avg_sq;
  const float* X; int64_t ldx;
  const float* actions; int64_t lda;
  const float* old_ll; const float* adv; const float* returns;
  const int32_t* perm;  // null (mb = 0 only): row m is sample m
  float* part;          // [tiles][ga_narrow_step_stride]: this member's gradient shares
  double* lpart;        // [tiles][2]: its loss sums
  float* losses;        // [n_steps] or null
  int32_t n_steps, last_M;
  float inv_full, inv_last;  // 1 / M of a full step and of the last one, rounded once
  float clip, ent_coeff;
};

// What the members share: the network's shape and the loss configuration.
struct GaMembersShared {
  int64_t w_off[3], b_off[3];
  int32_t in_w, H, out_w;
  int32_t kind, algo, ent_flags, has_min, has_max;
  float min_log_std, max_log_std;
  int32_t double_softmax, zero_slot0;
  int64_t stride;       // ga_narrow_step_stride(in_w, H)
  int64_t mb;           // rows of a full step (0: the whole batch in step 0)
  int32_t n_members;
};

extern "C" {
// Step k of every member: forward + loss + backward, grid (max_tiles, n_members).
// max_tiles: tiles of the largest minibatch any member has in step k.
int ga_members_train_step(const GaMembersShared* sh, const GaMemberDev* table_dev,
                          int64_t k, int64_t max_tiles, hipStream_t stream);
// ... and its shares -> gradient -> Adam, the loss finished; adam_dev: the GaAdam of
// step k, [n_members]; max_tiles as above (it sizes the grid).
int ga_members_reduce_adam(const GaMembersShared* sh, const GaMemberDev* table_dev,
                           const GaAdam* adam_dev, int64_t k, int64_t max_tiles,
                           hipStream_t stream);
// update_members.cpp: waits for the passes in flight and frees the table slots the loop
// keeps (tests)
void ga_update_members_release(void);
}
