// What the host says to the kernels of the linear feature baseline (linear_baseline.hip)
// about one launch, the shape rules both sides share, and the launch seam that takes
// them.  Host C++ only (no device code), in the style of loss_params.h: the host side
// (linear_baseline_host.cpp) checks the C-ABI arguments, fills these structs and chooses
// the grid and the dynamic LDS size, the seam instantiates and launches -- so that the host
// side builds for the CPU harness under tests/host (linear_baseline_harness.cpp) against
// fakes of the seam.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LB_MAX_OBS 128       // F = 2 * obs_dim + 4 <= 260: 17 column tiles of 16
#define LB_THREADS 512       // of a Gram workgroup: 8 waves
#define LB_WAVES 8
#define LB_MAX_CHUNK_ROWS 32  // rows whose features stand in LDS at once, at most
#define LB_LDS_BUDGET 65536  // bytes of LDS a Gram workgroup may ask for
#define LB_SLAB_ROWS 2048    // contiguous rows a workgroup takes at a time
#define LB_MAX_BLOCKS 1024   // Gram workgroups; beyond, a workgroup takes every
                             // LB_MAX_BLOCKS-th slab
#define LB_LDS_PAD 4         // doubles between the feature rows of a chunk
#define LB_MAX_TPW 20        // upper-triangle tiles a wave accumulates, at most
#define LB_PREDICT_THREADS 256
#define LB_REDUCE_THREADS 256

inline int lb_features(int obs_dim) { return 2 * obs_dim + 4; }
inline int lb_tiles(int obs_dim) { return (lb_features(obs_dim) + 15) / 16; }
// 16x16 tiles of the upper triangle, the diagonal's included
inline int lb_upper_tiles(int obs_dim) {
  const int T = lb_tiles(obs_dim);
  return T * (T + 1) / 2;
}
// a workgroup's partial: its tiles as 256 doubles each ([row][col] of the tile), then
// Phi^T r padded to the tiles' 16 * T columns
inline int64_t lb_block_doubles(int obs_dim) {
  return (int64_t)lb_upper_tiles(obs_dim) * 256 + 16 * lb_tiles(obs_dim);
}
inline int64_t lb_slabs(int64_t S) { return (S + LB_SLAB_ROWS - 1) / LB_SLAB_ROWS; }
inline int lb_gram_blocks(int64_t S) {
  const int64_t n = lb_slabs(S);
  return (int)(n > LB_MAX_BLOCKS ? LB_MAX_BLOCKS : n);
}
// Tiles a wave accumulates when the features have T column tiles: the upper triangle's,
// dealt to the waves in runs (the Gram kernel is instantiated per T and asks this too)
constexpr int lb_tiles_per_wave_of(int T) {
  return (T * (T + 1) / 2 + LB_WAVES - 1) / LB_WAVES;
}
inline int lb_tiles_per_wave(int obs_dim) { return lb_tiles_per_wave_of(lb_tiles(obs_dim)); }
// dynamic LDS: two chunks of `rows` feature rows (double-buffered) with their returns, and
// the slab's step indices
inline unsigned lb_gram_lds_bytes(int obs_dim, int rows) {
  const int ld = 16 * lb_tiles(obs_dim) + LB_LDS_PAD;
  return (unsigned)(2 * rows * ld * sizeof(double) + 2 * LB_MAX_CHUNK_ROWS * sizeof(double) +
                    LB_SLAB_ROWS * sizeof(int32_t));
}
// rows of a chunk: 32, 16 or 8 (k-steps of 4 rows), the most that fit the budget
inline int lb_chunk_rows(int obs_dim) {
  int rows = LB_MAX_CHUNK_ROWS;
  while (rows > 8 && lb_gram_lds_bytes(obs_dim, rows) > LB_LDS_BUDGET) rows /= 2;
  return rows;
}

struct LinGramParams {
  const float* obs;        // [S, ldo]; columns obs_dim .. ldo are never read
  int64_t ldo;
  int obs_dim;
  const int64_t* ep_off;   // [n_eps + 1]
  int64_t n_eps;
  int64_t S;
  const float* returns;    // [S]
  double* partials;        // [blocks][block_doubles]
  int64_t block_doubles;
  int64_t n_slabs;
  int F, T, NT;            // features, column tiles, upper-triangle tiles
  int tpw;                 // tiles per wave: wave w owns tiles [w * tpw, (w + 1) * tpw)
  int chunk_rows;          // lb_chunk_rows(obs_dim)
};

struct LinReduceParams {
  const double* partials;
  int n_blocks;            // partials to add, in this order
  int64_t block_doubles;
  int F, T, NT;
  double* gram;            // [F, F]
  double* rhs;             // [F]
};

struct LinPredictParams {
  const float* obs;
  int64_t ldo;
  int obs_dim;
  const int64_t* ep_off;
  int64_t n_eps;
  int64_t S;
  const double* coeffs;    // [F]
  float* values;           // values[i * ldv]
  int64_t ldv;
};

// ---- a population: every member's batch in ONE launch of each pass -----------------------
// (linear_baseline_members_host.cpp).  The grids are flat: member m owns `n_blocks`
// consecutive workgroups from `block0` on -- the prefix table a workgroup searches for its
// member -- and inside them it is the lone kernel's grid: the workgroup's index and the
// slab stride are relative to the member.
struct LinGramMemberDev {
  const float* obs;
  int64_t ldo;
  const int64_t* ep_off;
  int64_t n_eps;
  int64_t S;
  const float* returns;
  double* partials;        // the member's stretch: [n_blocks][block_doubles]
  double* gram;            // [F, F]
  double* rhs;             // [F]
  int64_t n_slabs;         // lb_slabs(S)
  int32_t block0;          // sum of the n_blocks of the members before this one
  int32_t n_blocks;        // lb_gram_blocks(S)
};

// what the Gram launch and its reduce launch share
struct LinGramMembersParams {
  const LinGramMemberDev* members;  // DEVICE [n_members]
  int n_members;
  int obs_dim;
  int64_t block_doubles;
  int F, T, NT;
  int tpw;
  int chunk_rows;
};

struct LinPredictMemberDev {
  const float* obs;
  int64_t ldo;
  const int64_t* ep_off;
  int64_t n_eps;
  int64_t S;
  const double* coeffs;    // [F], or null: the member's values are zeros
  float* values;
  int64_t ldv;
  int64_t block0;          // sum over the members before of ceil(S / LB_PREDICT_THREADS)
};

struct LinPredictMembersParams {
  const LinPredictMemberDev* members;  // DEVICE [n_members]
  int n_members;
  int obs_dim;
};

// ---- linear_baseline.hip: the launch seam.  Each does nothing but launch on `stream`:
// the Gram pass `blocks` workgroups of LB_THREADS with `lds_bytes` of dynamic LDS, the
// instantiation p.T's; the other two `blocks` workgroups of their own thread count.
void lb_launch_gram(const LinGramParams& p, unsigned blocks, unsigned lds_bytes,
                    hipStream_t stream);
void lb_launch_gram_reduce(const LinReduceParams& p, unsigned blocks, hipStream_t stream);
void lb_launch_predict(const LinPredictParams& p, unsigned blocks, hipStream_t stream);
// The population's: `blocks` is the sum of the members' workgroups (Gram, predict); the
// reduce launch is a grid of (`blocks`, n_members) workgroups, row m member m's.
void lb_launch_gram_members(const LinGramMembersParams& p, unsigned blocks, unsigned lds_bytes,
                            hipStream_t stream);
void lb_launch_gram_reduce_members(const LinGramMembersParams& p, unsigned blocks,
                                   hipStream_t stream);
void lb_launch_predict_members(const LinPredictMembersParams& p, unsigned blocks,
                               hipStream_t stream);
