// The three launches of a population's joint pack (member_pack.hip) and the plane
// table the gather reads, used by the two C-ABI entries (member_pack_host.cpp).  Not part
// of the C ABI.  Host C++ (no device code), so that the CPU harness under tests/host
// can build member_pack_host.cpp against it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

// how a plane is copied (wave-uniform: a workgroup works on one plane)
enum GaPackPath {
  GA_PACK_QUADS = 0,   // 4-byte elements, width a multiple of 4: 16-byte pieces
  GA_PACK_SCALAR = 1,  // width 1: four rows per thread, one 16-byte / 4-byte store
  GA_PACK_ELEMS = 2,   // anything else: one element per thread
};

struct GaPackPlaneDev {
  const void* src; void* dst;
  int64_t ld_src, ld_dst;  // in elements
  int64_t rows;            // n_rows, or n_eps of a per-episode plane
  int64_t units;           // what the plane's threads share out (see the paths)
  int32_t elem_size, width, per_episode, path;
};

// kernel argument of the gather: the whole table by value
struct GaPackTable {
  GaPackPlaneDev plane[GA_PACK_MAX_PLANES];
  const int32_t* src;
  const int32_t* ep_env;
  const int32_t* ep_end;
  int64_t Tcap;
  int32_t n_planes;
};

struct GaPackIndexArgs {
  const uint16_t* tail;
  int64_t g, Tcap;
  int32_t n_cols, n_members;
  const int32_t* progress;
  const int32_t* col_base;
  int64_t max_eps, max_samples;
  int32_t* ep_env; int32_t* ep_end; int32_t* ep_len;
  int64_t* ep_off; int64_t* member_samples; int64_t* member_off;
  int32_t* src;
};

extern "C" {
// grid (n_members): the member's episodes in batch order, their relative offsets, S_m
int ga_launch_member_episodes(const GaPackIndexArgs* a, hipStream_t stream);
// grid (blocks_x, n_members): member_off and the cell of every row below max_samples
int ga_launch_member_src(const GaPackIndexArgs* a, int64_t blocks_x, hipStream_t stream);
// grid (blocks_x, n_planes): every plane's rows
int ga_launch_member_gather(const GaPackTable* t, int64_t blocks_x, hipStream_t stream);
}
