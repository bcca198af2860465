// The kernel side's shape rules, restated for the host harnesses: which shapes each
// kernel family takes and the tile arithmetic the host code sizes buffers with
// (fused_train.hip, narrow_step.hip, small_step.hip).  This is the one restatement under
// tests/host/; include it once per program, after harness.h.
#pragma once
#include <stdint.h>

#include "../../garage_amd/csrc/fused_train.h"

extern "C" {
int64_t ga_fused_tiles(int64_t M) { return (M + 63) / 64; }
int ga_fused_width_ok(int w) { return w == 64 || w == 128 || w == 256; }
int ga_fused_first_layer_ok(int in_w, int K) {
  return in_w >= 1 && in_w <= 32 && K >= 32 && K % 32 == 0 &&
         (int64_t)K * ((in_w + 3) & ~3) <= 5120;
}
int ga_fused_pair_supported(int width, int K, int in_w) {
  return width == 256 && K <= 256 && ga_fused_first_layer_ok(in_w, K);
}
int ga_narrow_step_supported(int n_layers, const int* dims) {
  return n_layers == 3 && dims[1] == dims[2] && (dims[1] == 32 || dims[1] == 64) &&
         dims[0] >= 1 && dims[0] <= 32 && dims[3] >= 1 && dims[3] <= 8;
}
int64_t ga_narrow_step_stride(int in_w, int H) {
  const int64_t ld0 = (in_w + 3) & ~3;
  return (int64_t)H * ld0 + H + (int64_t)H * H + H + 8 * (int64_t)H + 8;
}
}  // extern "C"

// (these two are answered through switches of the fake kernel side of update.cpp)
static int small_step_rule(int n_layers, const int* dims, int64_t M) {
  return n_layers == 3 && dims[1] == dims[2] && dims[1] % 32 == 0 && dims[1] >= 32 &&
         dims[1] <= 256 && dims[0] >= 1 && dims[0] <= 32 && dims[3] >= 1 && dims[3] <= 8 &&
         M >= 1 && M <= 64;
}
static int fused_fwd_dgrad_rule(int width, int K, int in_w) {
  return ga_fused_width_ok(width) && K == width && ga_fused_first_layer_ok(in_w, K);
}
