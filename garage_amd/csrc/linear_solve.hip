// The F x F solve of garage's LinearFeatureBaseline on the device
// (np/baselines/linear_feature_baseline.py:70-79): for every member of a launch
//   (G + reg I) x = b,  reg *= 10 and again while the result is broken, five times at most,
// in fp64, by a blocked Cholesky factorisation.  One workgroup of 8 waves a member; member
// m's pointers are entry blockIdx.x of a table.  G is the F x F matrix gram_reduce_body
// (linear_baseline.hip) writes and is only read: a retry starts from it again.
//
// The matrix is padded to N = 16 T rows and columns with an identity block, so that every
// tile is a whole 16 x 16 tile and the matrix instruction needs no masks: the factor of
// diag(A, I) is diag(L, I), and with zeros under b the pad part of x is zero.
//
// Left-looking, block column k = 0 .. T - 1 (every tile of L is written once, never
// read-modified-written in memory):
//   1. wave w takes the tiles (i, k), i = k + w, k + w + 8, ..: G_ik (+ reg on the diagonal)
//      - sum_{j<k} L_ij L_kj^T, accumulated by v_mfma_f64_16x16x4_f64 with the operand map
//      stated at the top of linear_baseline.hip: lane l gives L[16 i + (l & 15)][c] as A and
//      L[16 k + (l & 15)][c] as B, c = 4 step + (l >> 4) -- the same read of two block rows.
//      The result goes to LDS, the block column [N][16] with rows LS_PANEL_LD doubles apart.
//   2. wave 0 factors the diagonal tile in place (unblocked, a row a lane, the column
//      passed round by lane reads).  A pivot that is not finite or not > 0 sets `broke`.
//   3. thread t takes row 16 k + t of the block column into registers, solves it against
//      L_kk^T (rows below the diagonal tile; L_kk is read from LDS, every thread the same
//      word) and stores its 16 values to the member's factor.
//
// Where the operands come from.  The operands of step 1 are block rows i and k of ALL
// columns before k -- the whole factor so far, 306 KB at F = 260, which LDS cannot hold --
// so they are read from the factor in the workspace (L2; a member's stretch is written and
// read by its own workgroup only, between barriers).  It is stored TRANSPOSED, U = L^T,
// block row k of U (= block column k of L) packed behind block row k - 1: a lane group's
// operand read is then 16 consecutive doubles of one row of U, one 128-byte line, and the
// stores of step 3 are consecutive across threads.  LDS holds the current block column,
// where the tiles change hands from the matrix instruction's result layout to a row a
// thread.
//
// Then L y = b and L^T x = y, blocked by the same tiles: wave 0 solves a diagonal tile (its
// 16 unknowns passed round by lane reads), then a thread a row takes the tile's unknowns
// out of the rows that remain.  A coefficient that is not finite sets `broke` too.  Every
// decision on `broke` is read from LDS behind a barrier: uniform over the workgroup.
// No atomics, a fixed order of every sum: the same inputs give the same bits, and a member
// gets the same bits alone or among others.
#include "common.h"
#include "linear_solve_params.h"

namespace {

typedef double ls_f64x4 __attribute__((ext_vector_type(4)));

// first double of block row k of U in a member's factor; its rows are N - 16 k doubles
// (columns 16 k .. N)
__device__ __forceinline__ int ls_base(int k, int N) { return 16 * k * N - 128 * k * (k - 1); }

__global__ __launch_bounds__(LS_THREADS) void solve_members_kernel(const LinSolveParams p) {
  constexpr int LD = LS_PANEL_LD;
  __shared__ double panel[16 * LS_MAX_TILES * LS_PANEL_LD];  // block column k: [N][LD]
  __shared__ double vec[16 * LS_MAX_TILES];                  // b, then y, then x
  __shared__ int broke;

  const LinSolveMemberDev& mem = p.members[blockIdx.x];
  const double* const G = mem.gram;
  const double* const rhs = mem.rhs;
  double* const W = mem.factor;
  const int F = p.F, T = p.T, N = 16 * T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;

  double reg = mem.reg_coeff;
  int status = -1;
  for (int attempt = 0; attempt < LS_TRIES; ++attempt, reg *= 10.0) {
    if (tid == 0) broke = 0;
    __syncthreads();
    bool bad = false;
    for (int k = 0; k < T; ++k) {
      const int ldk = N - 16 * k;
      // ---- 1. this wave's tiles of block column k
      {
        ls_f64x4 acc[LS_TPW];
#pragma unroll
        for (int q = 0; q < LS_TPW; ++q) acc[q] = ls_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < k; ++j) {
          const int ld = N - 16 * j;
          // row c = 4 ks + l4 of block row j of U, at column 16 j + l15
          const double* const frag = W + ls_base(j, N) + l4 * ld - 16 * j + l15;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const double* const row = frag + 4 * ks * ld;
            const double b = row[16 * k];
#pragma unroll
            for (int q = 0; q < LS_TPW; ++q) {
              const int i = k + wave + LS_WAVES * q;
              if (i < T)  // (uniform in the wave)
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * i], b, acc[q], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < LS_TPW; ++q) {
          const int i = k + wave + LS_WAVES * q;
          if (i < T) {
            const int C = 16 * k + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int R = 16 * i + l4 + 4 * r;
              double g = (R < F && C < F) ? G[R * F + C] : (R == C ? 1.0 : 0.0);
              if (R == C && R < F) g += reg;
              panel[R * LD + l15] = g - acc[q][r];
            }
          }
        }
      }
      __syncthreads();
      // ---- 2. the diagonal tile, in place: lane r (and its three copies) holds row r
      if (wave == 0) {
        double* const prow = panel + (16 * k + l15) * LD;
        double x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) x[c] = prow[c];
        bool bad_pivot = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const double d = __shfl(x[j], j, 64);
          if (!(d > 0.0) || !(d < INFINITY)) bad_pivot = true;
          const double s = sqrt(d);
          x[j] = (l15 == j) ? s : x[j] / s;  // L[r][j], r >= j
#pragma unroll
          for (int c = j + 1; c < 16; ++c) {
            const double lcj = __shfl(x[j], c, 64);  // L[c][j]
            x[c] = fma(-x[j], lcj, x[c]);            // (used where c <= r)
          }
        }
        if (lane < 16) {
#pragma unroll
          for (int c = 0; c < 16; ++c) prow[c] = c <= l15 ? x[c] : 0.0;
        }
        if (bad_pivot && lane == 0) broke = 1;
      }
      __syncthreads();
      bad = broke != 0;
      if (bad) break;
      // ---- 3. a row a thread: solve against L_kk^T, store column-wise into U
      if (tid < ldk) {
        const double* const prow = panel + (16 * k + tid) * LD;
        double x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) x[c] = prow[c];
        if (tid >= 16) {
          const double* const dk = panel + 16 * k * LD;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            double s = x[j];
#pragma unroll
            for (int c = 0; c < j; ++c) s = fma(-x[c], dk[j * LD + c], s);
            x[j] = s / dk[j * LD + j];
          }
        }
        double* const out = W + ls_base(k, N) + tid;
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j * ldk] = x[j];
      }
      __syncthreads();
    }

    if (!bad) {
      if (tid < N) vec[tid] = tid < F ? rhs[tid] : 0.0;
      __syncthreads();
      // ---- L y = b
      for (int k = 0; k < T; ++k) {
        const int ldk = N - 16 * k;
        const double* const blk = W + ls_base(k, N);
        if (wave == 0) {
          double Lr[16];  // L[16 k + r][16 k + c] = U[16 k + c][16 k + r]
#pragma unroll
          for (int c = 0; c < 16; ++c) Lr[c] = blk[c * ldk + l15];
          double v = vec[16 * k + l15];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const double yj = __shfl(v / Lr[j], j, 64);
            if (l15 == j) v = yj;
            else if (l15 > j) v = fma(-Lr[j], yj, v);
          }
          if (lane < 16) vec[16 * k + l15] = v;
        }
        __syncthreads();
        if (tid < ldk - 16) {
          const double* const col = blk + 16 + tid;  // column 16 (k + 1) + tid of U
          double s = vec[16 * (k + 1) + tid];
#pragma unroll
          for (int j = 0; j < 16; ++j) s = fma(-col[j * ldk], vec[16 * k + j], s);
          vec[16 * (k + 1) + tid] = s;
        }
        __syncthreads();
      }
      // ---- L^T x = y
      for (int k = T - 1; k >= 0; --k) {
        const int ldk = N - 16 * k;
        if (wave == 0) {
          const double* const urow = W + ls_base(k, N) + l15 * ldk;
          double Ur[16];  // U[16 k + r][16 k + c]
#pragma unroll
          for (int c = 0; c < 16; ++c) Ur[c] = urow[c];
          double v = vec[16 * k + l15];
#pragma unroll
          for (int j = 15; j >= 0; --j) {
            const double xj = __shfl(v / Ur[j], j, 64);
            if (l15 == j) v = xj;
            else if (l15 < j) v = fma(-Ur[j], xj, v);
          }
          if (lane < 16) vec[16 * k + l15] = v;
        }
        __syncthreads();
        if (tid < 16 * k) {
          const int kb = tid >> 4;
          const double* const urow =
              W + ls_base(kb, N) + (tid & 15) * (N - 16 * kb) + 16 * (k - kb);
          double s = vec[tid];
#pragma unroll
          for (int j = 0; j < 16; ++j) s = fma(-urow[j], vec[16 * k + j], s);
          vec[tid] = s;
        }
        __syncthreads();
      }
      if (tid < F && !(fabs(vec[tid]) < INFINITY)) broke = 1;
      __syncthreads();
      bad = broke != 0;
    }
    if (!bad) {
      status = attempt;
      break;
    }
    __syncthreads();  // (everyone has read `broke` before the next attempt clears it)
  }
  if (tid < F) mem.coeffs[tid] = status < 0 ? __builtin_nan("") : vec[tid];
  if (tid == 0) *mem.status = status;
}

}  // namespace

// ---- the launch seam (linear_solve_params.h): launch, nothing else ------------------------
void ls_launch_solve_members(const LinSolveParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(solve_members_kernel, dim3(blocks), dim3(LS_THREADS), 0, stream, p);
}
