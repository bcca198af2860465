// What the host says to the kernels of a fused optimizer step (fused_train.hip) about one
// launch, and the launch seam that takes it.  Host C++ only (no device code), in the
// style of gemm_params.h: the host side (fused_train_host.cpp) fills these structs and
// chooses the variant and the grid, the seam instantiates and launches -- so that the
// host side builds for the CPU harness under tests/host (fused_host_harness.cpp) against
// fakes of the seam.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "gemm_params.h"
#include "loss_args.h"

struct FwdLossParams {
  GemmParams g;          // A, lda, a_idx, B (= W [BN][ldb]), bias, M, N (= BN), K
  const float* head_W;   // [A][head_ldw]
  int64_t head_ldw;
  const float* head_bias;
  LossRowArgs loss;
  float* dZ;             // [M][lddz]
  int64_t lddz;
  float* hpart;          // [gx][8 * BN + 8]: dW_head (j major), then db_head
  double* lpart;         // [gx][2]
  // L1 instantiation: the layer below is the FIRST layer (<= 32 inputs) and its
  // output -- this GEMM's A operand -- is produced by the kernel itself:
  // H1 = tanh(X W1^T + b1) chunk by chunk; g.A / g.lda are unused
  const float* l1_X;     // observations [*][l1_ldx], gathered through loss.idx
  int64_t l1_ldx;
  const float* l1_W;     // [K][round4(l1_in)]
  const float* l1_b;     // [K]
  int l1_in;
  float* l1_H;           // [M][l1_ldh]: H1 is written once, for the backward pass
  int64_t l1_ldh;
  float* eval_out;       // EVAL: the head outputs [M][eval_ldo], nothing else is kept
  int64_t eval_ldo;
  // SPLIT instantiation (opt-in, see "split-operand k-loop" in fused_train.hip): W as three bf16
  // planes in fragment order (split_planes_kernel), plane p at bplanes + p * bplane_stride
  const uint16_t* bplanes;
  int64_t bplane_stride;
  long long* dbg;        // developer hook: phase timestamps of one workgroup
};

// The same step of TWO networks (the policy's and the value function's minibatch k:
// vpg.py:244-248 runs them one after the other, neither reads what the other
// writes) in one grid: workgroup b takes tile b / 2 of network b % 2.  Twice the
// workgroups per launch: the second generation starts as first-generation
// workgroups retire, one launch ramp and drain instead of two, and -- unlike two
// free-running streams -- the same schedule every time.
struct FwdLossPair {
  FwdLossParams a, b;
};

// Slab ranges one data-gradient launch sums on the side (ga_fused_dgrad_net::sum_w /
// sum_b): quad v of the launch is quad v of range 0 for v < nq[0], quad v - nq[0] of
// range 1 after that; off: floats from `base` to partial 0 of a range's element 0.
struct FtSlabSum {
  float* base;
  uint32_t off[2];
  int nq[2];
  int64_t stride;   // floats between partials
  int n_part;       // 0: nothing to sum
  int tiles;        // workgroups of this network's launch
};

struct DgradWgrad0Params {
  GemmParams g;        // A = dZ2 [M][lda], B = W2 [K][ldb] (n contiguous), M, N = BN, K
  const float* H;      // tanh outputs of the first hidden layer [M][ldh]
  int64_t ldh;
  const float* X;      // observations [*][ldx], in_w valid columns, gathered
  int64_t ldx;
  const int32_t* idx;
  int in_w;            // <= 32
  float* wpart;        // [gx][BN * ld0 + BN]: dW1 [n][ld0], then db1 [n]
  // SPLIT instantiation: W2 as the B operand B(k = unit of layer 2, n = unit of layer
  // 1) in three bf16 planes, fragment order (split_planes_kernel<true>)
  const uint16_t* bplanes;
  int64_t bplane_stride;
  long long* dbg;      // developer hook: phase timestamps (FT_STAMP / FT_MARK)
  FtSlabSum sum;       // the middle layer's split-K slabs, summed on the side
};

struct DgradWgrad0Pair {
  DgradWgrad0Params a, b;
};

// fwd_dgrad_kernel: the forward + loss body and the data-gradient body of one tile
struct FwdDgradParams {
  FwdLossParams f;
  DgradWgrad0Params d;
};

// ---------------------------------------------------------------------------
struct FtAdam {
  float* p; float* m; float* v;
  GaAdam c;
};

constexpr int FT_MAX_REGIONS = 16;
struct FtRegion {
  int64_t beg;        // first flat parameter index
  int64_t n;          // elements (a multiple of 4)
  const float* src;   // partial 0 of element 0
  int64_t stride;     // floats between consecutive partials
  int n_part;
  int quads;          // quads per workgroup: 64 or 16 (pre: 256)
  int pre;            // partial 0 holds the sum already: nothing else is read
  int64_t vbeg;       // first workgroup of the region
  int net;            // which network's buffers (a pair launch steps two)
};
struct FtNet {
  FtAdam a;
  float* grads;       // the reduced (scaled) gradient is also written here
  float scale;
  int do_adam;        // 0: stop after writing grads (an all-reduce follows)
  int zero_slot0;     // the log-std slot is not trained
  // loss finish (one extra block per network): batch sums -> loss value, log-std
  // gradient
  const double* lpart;
  int n_lpart;
  int64_t M;
  LossRowArgs loss;
  float* loss_out;
  // split-operand experiment: the planes of ONE weight matrix (rows x cols, ld = cols, at
  // flat index pl_beg) are rewritten with the updated values, so that the next step's
  // forward launch needs no plane launch (null: nothing)
  uint32_t* pl_fwd;
  uint32_t* pl_bwd;
  int64_t pl_beg;
  int pl_rows, pl_cols;
};
struct ReduceRegionsParams {
  FtRegion r[FT_MAX_REGIONS];
  int n_regions;
  int n_nets;         // 1 or 2
  int64_t n_virtual;  // workgroups over all regions
  FtNet net[2];
};

// Who asks for the planes of a weight matrix (fused_train_host.cpp: planes_for).
// PLANES_BWD: the fused data-gradient launch of the step whose forward launch asked with
// PLANES_TRAIN_FWD (may reuse); PLANES_BWD_ALWAYS: anybody else (always recomputes)
enum { PLANES_TRAIN_FWD = 0, PLANES_BWD = 1, PLANES_EVAL_FWD = 2, PLANES_BWD_ALWAYS = 3 };

// ---- the instantiation a launch runs.  width: the tile spans the layer's 64, 128 or 256
// units (<64, 2, 2>, <128, 1, 4>: 256 threads; <256, 1, 8>: 512 threads).  At 256 units
// there are two more k-loops: ksc = 5, the software-pipelined one for first layers of
// 17 .. 20 inputs, and split, the split-operand (3 x bf16) one.
struct FtVariant {
  int width;
  int l1;     // the network's first layer is computed in the kernel (forward + loss only:
              // the other families always / never do)
  int ksc;    // 0 or 5
  int split;
};

// ---- fused_train.hip: the launch seam, one function per kernel family.  Each does
// nothing but instantiate and launch on `stream`: `blocks` workgroups of the variant's
// thread count, timed by (e0, e1) when they are set (prof.h).
void ft_launch_fwd_loss(const FwdLossParams& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                        hipEvent_t e1, hipStream_t stream);
void ft_launch_fwd_loss_pair(const FwdLossPair& pp, FtVariant v, unsigned blocks,
                             hipEvent_t e0, hipEvent_t e1, hipStream_t stream);
void ft_launch_eval_forward(const FwdLossParams& p, FtVariant v, unsigned blocks,
                            hipEvent_t e0, hipEvent_t e1, hipStream_t stream);
void ft_launch_dgrad(const DgradWgrad0Params& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                     hipEvent_t e1, hipStream_t stream);
void ft_launch_dgrad_pair(const DgradWgrad0Pair& pp, FtVariant v, unsigned blocks,
                          hipEvent_t e0, hipEvent_t e1, hipStream_t stream);
void ft_launch_fwd_dgrad(const FwdDgradParams& pp, FtVariant v, unsigned blocks,
                         hipEvent_t e0, hipEvent_t e1, hipStream_t stream);
void ft_launch_reduce_regions(const ReduceRegionsParams& p, unsigned blocks,
                              hipStream_t stream);
// W [rows][ld] -> planes; bwd_only: `blocks` workgroups write bwd, else blocks [0, half)
// write fwd and, when blocks covers them, [half, 2 half) bwd (split_planes_kernel)
void ft_launch_split_planes(bool bwd_only, unsigned blocks, const float* W, int64_t ld,
                            int rows, int cols, uint32_t* fwd, uint32_t* bwd,
                            hipStream_t stream);
void ft_launch_mfma_burn(int mode, int iters, int blocks, float* sink, hipStream_t stream);
