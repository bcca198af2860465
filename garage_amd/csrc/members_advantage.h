// Every member's returns, GAE(lambda) advantages and advantage normalisation in ONE launch
// (ga_advantages_members_f32): the device table and the launch seam between the host side
// (members_advantage_host.cpp) and the kernel (members_advantage.hip).  One workgroup of
// MA_THREADS per member; the member's advantages stay in 4 * S bytes of LDS from the scan
// to the one store.  Host C++ only (no device code).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "gae_scan_params.h"
#include "shape_rules.h"

constexpr int MA_THREADS = 1024;  // 16 waves; four quarters of 256 play the stats blocks

enum MaFlags {
  MA_CENTER = 1,    // (a - mean) / (var + 1e-8)
  MA_POSITIVE = 2,  // a - min(a)
  MA_PACKED = 4,    // the advantages are S contiguous floats (offsets, or ld == T)
};

// One member, as the kernel reads it (device table [n_members]).
struct MaEntry {
  int32_t kernel;    // GaScanKernel: the kernel ga_gae_scan_f32 takes for this member
  int32_t flags;     // MaFlags
  int64_t waves;     // waves of that lone launch
  int64_t S;         // samples
  const float* v0;   // device scalar, or null: 0.0
  float* adv;        // as the rows lie in rewards: [S], or [n_rows, ld]
  double* stats;     // [4]: sum, count, squared deviations, minimum
  ScanParams g;      // GS_GENERAL, GS_GENERAL_VEC (adv unused, v0 from the pointer)
  RowsScanParams r;  // GS_ROWS_1, GS_ROWS_2      (likewise)
};

// members_advantage.hip: one grid of n workgroups, lds_bytes of dynamic LDS (4 * the
// largest S among the entries); work: the algorithmic bytes (16 per step)
int ma_launch_advantage_members(const MaEntry* table, unsigned n, unsigned lds_bytes,
                                double work, hipStream_t stream);
