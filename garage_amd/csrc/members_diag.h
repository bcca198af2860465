// The diagnostics passes of a POPULATION in joint launches (members_diag_host.cpp): what
// the host says to the member-indexed twins of the per-layer forward kernels, the loss row
// kernels, the KL kernels and the episode statistics, and the launch seam that takes it.
// A twin reads its parameter struct from a device table at its entry index, leaves when its
// block index is past that entry's own grid, and runs the BODY of the lone kernel with the
// block index and block count the lone launch would have -- so every entry gets the bits of
// its lone launch.  Sums finish in a second, fixed-order launch as the lone kernels' do: no
// grid barrier, no waiting on another workgroup.  Host C++ only (no device code), in the
// style of loss_params.h and layer_plans.h, whose structs the tables carry: the host side
// builds for the CPU harness under tests/host (members_diag_harness.cpp) against fakes of
// this seam.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "layer_plans.h"
#include "loss_params.h"

// ---- the forward pass of one network, as the launches ga_mlp_forward_f32 makes ---------
enum MdFwdKind {
  MD_FWD_SKINNY = 0,     // skinny_fwd_kernel<KV, true, 0>
  MD_FWD_GEMM_HEAD = 1,  // the last hidden layer and the head in one launch
  MD_FWD_GEMM = 2,       // gemm_f32_kernel, the tile of the plan
};
struct GaForwardStep {
  int kind;       // MdFwdKind
  int layer;      // the (first) layer the step computes
  GemmParams g;   // the product; MD_FWD_GEMM / _HEAD: with the plan applied
  GemmPlan gp;          // MD_FWD_GEMM
  GemmHeadPlan hp;      // MD_FWD_GEMM_HEAD
  SkinnyFwdPlan sp;     // MD_FWD_SKINNY
  SkinnyFwdParams s;
};
// mlp_layers.cpp: the launches ga_mlp_forward_f32 makes for these arguments under the
// switches as they stand, in order, WITHOUT making them: steps[<= 8], *n_steps of them.
// ga_mlp_forward_f32 itself walks the same steps.  Refuses what is no per-layer launch
// (layer normalisation, the whole-network forwards, weight planes).
int ga_mlp_forward_steps(const ga_mlp_desc* d, const float* params, const float* X,
                         int64_t ldx, const int32_t* row_idx, int64_t M, float* acts,
                         float* out, int64_t ldo, GaForwardStep* steps, int* n_steps);

// ---- table entries ---------------------------------------------------------------------
// which instantiation a GEMM table goes to (all forward: both operands k-contiguous)
enum MdGemmKind {
  MD_GEMM_128x32 = 0,   // gemm_f32_kernel<128, 32, 4, 1, true, true>      (GT_128x32)
  MD_GEMM_64x64 = 1,    // gemm_f32_kernel<64, 64, 2, 2, true, true>       (GT_64x64)
  MD_GEMM_HEAD_64 = 2,  // gemm_f32_kernel<64, 64, 2, 2, true, true, BK, true>
  MD_GEMM_KINDS = 3,
};
struct MdSkinnyEntry {
  SkinnyFwdParams p;
  unsigned gx, gy;  // the entry's own grid
};
// a loss row kernel's entry: nb blocks of 256 rows; p.loss_out set only where nb == 1
struct MdPpoEntry { PpoLossParams p; unsigned nb; };
struct MdCatEntry { CatLossParams p; unsigned nb; };
struct MdNllEntry { NllParams p; unsigned nb; };
struct MdKlEntry {
  const float* head_old;
  const float* head_new;
  int64_t ld, M;
  int A, dbl;
  float s_old, s_new;   // Gaussian heads: the log stds, as ga_gaussian_kl_f32 takes them
  double* partials;     // [nb]
  unsigned nb;
};
// the fixed-order sums of entries with more than one block (one wave each)
struct MdCatFinalize {
  const double* partials;
  int nblocks;
  int64_t M;
  float* loss_out;
  double* ent_sum_out;
};
struct MdNllFinalize {
  const double* partials;
  int nblocks;
  int64_t M;
  float* loss_out;
};
struct MdSum {
  const double* partials;
  int nblocks;
  double* out;
};
// log_performance's device part of one member: out[0 .. n) the episodes' reward sums
// (ga_episode_sums_f32's), out[n .. 2n) returns[ep_off[e]], out[2n .. 3n) 1.0 where the
// episode's last step type is `terminal`
struct MdEpisodes {
  const float* rewards;
  const int64_t* ep_off;
  int64_t n_eps;
  const float* returns;
  const uint8_t* step_types;
  int terminal;
  double* out;
};

// ---- the launch seam: each launches ONE grid over the n entries of a device table on
// `stream` and checks the launch.  `blocks`: the largest own grid among the entries.
// gemm.hip
int md_launch_gemm_members(int kind, const GemmParams* table, unsigned n, unsigned blocks,
                           hipStream_t stream);
// skinny.hip (KV: the instantiation; lds_bytes: the largest among the entries)
int md_launch_skinny_fwd_members(int KV, const MdSkinnyEntry* table, unsigned n, unsigned gx,
                                 unsigned gy, unsigned lds_bytes, hipStream_t stream);
// losses.hip
int md_launch_ppo_gaussian_members(const MdPpoEntry* table, unsigned n, unsigned blocks,
                                   hipStream_t stream);
int md_launch_ppo_gaussian_finalize_members(const PpoFinalizeParams* table, unsigned n,
                                            hipStream_t stream);
int md_launch_ppo_categorical_members(const MdCatEntry* table, unsigned n, unsigned blocks,
                                      hipStream_t stream);
int md_launch_ppo_categorical_finalize_members(const MdCatFinalize* table, unsigned n,
                                               hipStream_t stream);
int md_launch_nll_members(const MdNllEntry* table, unsigned n, unsigned blocks,
                          hipStream_t stream);
int md_launch_nll_finalize_members(const MdNllFinalize* table, unsigned n,
                                   hipStream_t stream);
int md_launch_kl_members(int categorical, const MdKlEntry* table, unsigned n, unsigned blocks,
                         hipStream_t stream);
int md_launch_sum_members(const MdSum* table, unsigned n, hipStream_t stream);
// members_diag.hip
int md_launch_episodes_members(const MdEpisodes* table, unsigned n, unsigned blocks,
                               hipStream_t stream);
