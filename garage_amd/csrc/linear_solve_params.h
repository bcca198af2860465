// What the host says to the solve kernel of the linear feature baseline (linear_solve.hip)
// about one launch, the shape rules both sides share, and the launch seam that takes them.
// Host C++ only (no device code), in the style of linear_baseline_params.h -- and a file of
// its own beside it, so that the harnesses of the Gram and predict entries, which fake that
// header's seam, build as they are.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LS_THREADS 512     // of a solve workgroup: 8 waves, one workgroup a member
#define LS_WAVES 8
#define LS_MAX_TILES 17    // 16-wide block columns: F = 2 * 128 + 4 = 260 <= 16 * 17
#define LS_TPW 3           // tiles of a block column a wave accumulates, at most
#define LS_PANEL_LD 17     // doubles from a row of the LDS block column to the next: odd, so
                           // that threads reading a row each do not meet in a bank
#define LS_TRIES 5         // attempts, the regulariser times 10 after each that broke down

inline int ls_features(int obs_dim) { return 2 * obs_dim + 4; }
inline int ls_tiles(int obs_dim) { return (ls_features(obs_dim) + 15) / 16; }
// A member's factor in the workspace: U = L^T with the pad rows and columns up to N = 16 T,
// block row k (rows 16 k .. 16 k + 15, columns 16 k .. N) packed behind block row k - 1:
// the T (T + 1) / 2 tiles of a triangle, 256 doubles each.
inline int64_t ls_member_doubles(int obs_dim) {
  const int64_t T = ls_tiles(obs_dim);
  return 256 * (T * (T + 1) / 2);
}

struct LinSolveMemberDev {
  const double* gram;    // [F, F] row-major, symmetric; read only
  const double* rhs;     // [F]
  double reg_coeff;      // of the first attempt
  double* coeffs;        // [F]
  int32_t* status;       // retries used 0 .. LS_TRIES - 1, or -1: every attempt broke down
  double* factor;        // the member's stretch of the workspace: ls_member_doubles
};

struct LinSolveParams {
  const LinSolveMemberDev* members;  // DEVICE [n_members]; workgroup m reads entry m
  int n_members;
  int F, T;
};

// ---- linear_solve.hip: the launch seam.  Does nothing but launch `blocks` (= n_members)
// workgroups of LS_THREADS on `stream`; the kernel's LDS is static.
void ls_launch_solve_members(const LinSolveParams& p, unsigned blocks, hipStream_t stream);
