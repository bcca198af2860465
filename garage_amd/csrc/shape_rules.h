// The kernel side's shape rules, each stated ONCE: which shapes a kernel family takes and
// the tile arithmetic the host code sizes buffers and grids with (fused_train.hip,
// narrow_step.hip, small_step.hip, policy_fused.hip, losses.hip, skinny.hip).  The kernels
// take their constants from here, the library's host code and the CPU harnesses under
// tests/host the rules.
// No device code.
// Not part of the C ABI.
#pragma once
#include <stdint.h>

#include "../../include/garage_amd.h"

// ---- fused_train.hip, narrow_body.h: a workgroup takes a 64-row tile of the minibatch
constexpr int FT_ROWS = 64;          // rows per workgroup tile
constexpr int FT_W1_FLOATS = 5120;   // LDS floats for the first layer's weights
// ---- narrow_body.h: two hidden layers of equal width 32 or 64
constexpr int NS_ROWS = FT_ROWS;     // (its launches size their grids by ga_fused_tiles)
constexpr int NS_HN = 8;             // head outputs, at most
// ---- small_step.hip: one tile of up to 64 rows, hidden width up to 256
constexpr int SS_ROWS = 64;
constexpr int SS_HMAX = 256;
// ---- policy_fused.hip: the rollout step (and, at PS_HMAX, the training forward)
constexpr int PS_ROWS = 16;          // envs per workgroup (one 16 x 16 MFMA tile of rows)
constexpr int PS_HMAX = 256;         // output columns per panel; widest layer input of the
                                     // WIDTH = 256 kernels and the training forward
constexpr int PS_WMAX = 512;         // widest layer input of the WIDTH = 512 kernels
constexpr int PS_MAX_OUT = 32;       // widest output head
constexpr int PS_KC = 32;            // k chunk
constexpr int PS_TRAIN_ROWS = 64;    // rows per workgroup of the training forward
// ---- losses.hip: the stand-alone loss, statistics and optimizer kernels
constexpr int RED_BLOCKS = 512;      // upper bound on partial-producing blocks
// blocks of a row kernel over n rows: one row per thread of 256 up to RED_BLOCKS blocks
// (losses_host.cpp, and members_diag_host.cpp for every member of a joint launch)
constexpr int ga_red_blocks(int64_t n) {
  return n <= 256 ? 1 : ((n + 255) / 256 > RED_BLOCKS ? RED_BLOCKS : (int)((n + 255) / 256));
}
constexpr int LS_DOT_THREADS = 1024; // the one workgroup of the dot product
constexpr int FS_MAX_A = 32;         // classes of the categorical Fisher seed (in registers)
// the head layer inside the loss kernel: 16 lanes own one row of the hidden activations
constexpr int HL_THREADS = 256;
constexpr int HL_GROUPS = HL_THREADS / 16;
// rows per 16-lane group and block iteration at KV = hidden width / 64
constexpr int ga_head_rows(int KV) { return KV <= 4 ? 4 : 2; }
constexpr int HL_ROWS_MAX = ga_head_rows(1);
// The head kernels' dynamic LDS, in floats: W [A][K] and the bias [round4(A)] -- what lies
// before the row buffers -- then the row buffers [HL_GROUPS][rows per group][A], sized for
// HL_ROWS_MAX at every width.  The kernels find the row buffers at smem + w + bias, the
// host asks for floats() of them.
struct HeadLds {
  int w, bias, rows;
  constexpr int floats() const { return w + bias + rows; }
};
constexpr HeadLds ga_head_lds(int A, int K) {
  return HeadLds{A * K, (A + 3) & ~3, HL_GROUPS * HL_ROWS_MAX * A};
}

// ---- skinny.hip: the streaming layer products (one dimension <= 32)
constexpr int SK_THREADS = 256;      // forward / data gradient: threads per workgroup
constexpr int SK_UNROLL = 4;         // rows a thread has in flight; rows_per_thread % 4 == 0
constexpr int SK_KMAX = 32;          // the narrow operand: KV = round4(K) / 4 <= 8 quads
constexpr int SK_LDS_CAP = 48 * 1024;  // bytes of staged narrow rows per workgroup, at most
constexpr int SW_THREADS = 256;      // weight gradient: threads per workgroup
constexpr int SW_QPR = 16;           // column quads (64 floats) per workgroup
// (16 NV accumulator registers per thread: beyond NS = 24 the kernel spills; the
// data-gradient instantiations exist for NV <= 4)
constexpr int SW_NS_MAX = 24;
constexpr int SW_NS_MAX_DZ = 16;
constexpr bool ga_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// forward: column quads per workgroup -- the whole row when it is a power of two <= 256
// floats, else 256-float column blocks; 0: no streaming shape
constexpr int ga_skinny_fwd_qpr(int wide) {
  return wide % 4 != 0 ? 0
         : wide <= 256 ? (ga_pow2(wide / 4) ? wide / 4 : 0)
                       : (wide % 256 == 0 ? 64 : 0);
}
// weight gradient: whole rows of <= 64 floats (a power of two), else 64-float column blocks
constexpr int ga_skinny_wgrad_qpr(int wide) {
  return wide % 4 != 0 ? 0
         : wide <= 4 * SW_QPR ? (ga_pow2(wide / 4) ? wide / 4 : 0)
                              : SW_QPR;
}

// The networks the step kernel takes with layer inputs up to `max_in`: up to 8 layers,
// every activation code the descriptor can name (0 .. 6), with or without layer
// normalisation, every layer INPUT in an LDS tile of max_in columns, a head up to
// PS_MAX_OUT.  ga_policy_step_fused_supported is this rule at PS_HMAX, the wide rule
// (ga_policy_step_wide_supported, ga_rollout_env_steps) this rule at PS_WMAX.
inline int ga_policy_step_rule(const ga_mlp_desc* d, int max_in) {
  if (!d || d->n_layers < 1 || d->n_layers > 8) return 0;
  if (d->hidden_act < 0 || d->hidden_act > 6 || d->output_act < 0 || d->output_act > 6)
    return 0;
  for (int l = 0; l < d->n_layers; ++l)
    if (d->dims[l] > max_in) return 0;
  return d->dims[d->n_layers] <= PS_MAX_OUT;
}

extern "C" {
// workgroups (= partial sets) for M rows
inline int64_t ga_fused_tiles(int64_t M) { return (M + FT_ROWS - 1) / FT_ROWS; }
// the last hidden layer's width: one instantiation each
inline int ga_fused_width_ok(int width) { return width == 64 || width == 128 || width == 256; }
// the FIRST layer produced inside the forward kernel: in_w inputs, K units
inline int ga_fused_first_layer_ok(int in_w, int K) {
  return in_w >= 1 && in_w <= 32 && K >= 32 && K % 32 == 0 &&
         (int64_t)K * ((in_w + 3) & ~3) <= FT_W1_FLOATS;
}
// Pair launches are compiled for 256-wide last hidden layers with the first layer in
// the kernel (the C3-class networks the two-chain schedule was built for).
inline int ga_fused_pair_supported(int width, int K, int in_w) {
  return width == 256 && K <= 256 && ga_fused_first_layer_ok(in_w, K);
}
inline int ga_narrow_step_supported(int n_layers, const int* dims) {
  return n_layers == 3 && dims[1] == dims[2] && (dims[1] == 32 || dims[1] == 64) &&
         dims[0] >= 1 && dims[0] <= 32 && dims[3] >= 1 && dims[3] <= NS_HN;
}
// floats of one tile's gradient shares: dW1 [H][round4(in_w)], db1, dW2 [H][H], db2,
// dW_head [8][H], db_head [8]
inline int64_t ga_narrow_step_stride(int in_w, int H) {
  const int64_t ld0 = (in_w + 3) & ~3;
  return (int64_t)H * ld0 + H + (int64_t)H * H + H + NS_HN * (int64_t)H + NS_HN;
}
}  // extern "C"

// The rules behind the entry points that stay link-time seams (a harness makes them
// answer 0): ga_fused_fwd_dgrad_supported, ga_fused_eval_supported, ga_head_loss_supported
// and the shape part of ga_small_step_supported are one-line wrappers over these.
// fwd_dgrad_kernel is compiled for two hidden layers of the same width (K = the first
// one's, width = the second one's) with the first layer in the kernel.
inline int ga_fused_fwd_dgrad_rule(int width, int K, int in_w) {
  return ga_fused_width_ok(width) && K == width && ga_fused_first_layer_ok(in_w, K);
}
inline int ga_fused_eval_rule(int n_layers, const int* dims) {
  return n_layers == 3 && dims && ga_fused_first_layer_ok(dims[0], dims[1]) &&
         dims[1] <= 256 && ga_fused_width_ok(dims[2]) && dims[3] >= 1 && dims[3] <= 8;
}
// the head layer inside the loss kernel: one instantiation per hidden width, the head's
// weights ([A][hidden_width]) within 60 KiB of LDS
inline int ga_head_loss_rule(int hidden_width, int A) {
  return (hidden_width == 64 || hidden_width == 128 || hidden_width == 256 ||
          hidden_width == 512) && A >= 1 && A <= 64 &&
         (int64_t)A * hidden_width * 4 <= 60 * 1024;
}
inline int ga_small_step_rule(int n_layers, const int* dims, int64_t M) {
  if (n_layers != 3) return 0;
  const int in_w = dims[0], H = dims[1], out_w = dims[3];
  return dims[2] == H && H % 32 == 0 && H >= 32 && H <= SS_HMAX && in_w >= 1 &&
         in_w <= 32 && out_w >= 1 && out_w <= 8 && M >= 1 && M <= SS_ROWS;
}
