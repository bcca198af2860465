// The device side of garage's LinearFeatureBaseline (np/baselines/linear_feature_baseline.py):
// the normal equations of its ridge regression, G = Phi^T Phi and b = Phi^T r in fp64, and
// its predictions Phi c, with the feature rows (linear_features.h) formed on the fly and
// never written to HBM.  The F x F solve stays on the host (garage_amd/baselines.py).
//
// Gram pass.  A workgroup of 8 waves takes contiguous slabs of LB_SLAB_ROWS rows.  It
// first finds every row's step index t inside its episode (one binary search over ep_off
// and a short walk per thread) and keeps them in LDS.  Then, chunk by chunk (32, 16 or 8
// rows), the feature rows are written to LDS as doubles -- [row][16 T + pad] with the
// columns from F on and the rows past the slab's end exact zeros -- and every wave feeds
// its share of the 16x16 tiles of the UPPER triangle to v_mfma_f64_16x16x4_f64, four rows
// a k-step.  The chunks are double-buffered: the observations of the next chunk are
// loaded before the products of this one and converted after them, one barrier a chunk.
//
// The f64 MFMA's operand maps (they are not the other formats'): lane l holds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one double each, and result
// register r of lane l is C[row = (l >> 4) + 4 r][col = l & 15].  With A = Phi_chunk^T
// (tile ti's columns) and B = Phi_chunk (tile tj's columns) both operands are the SAME
// read: lane l takes Phi[4 ks + (l >> 4)][16 t + (l & 15)] for t = ti and for t = tj.
//
// Phi^T r is a vector sum: thread c adds column c's products in row order.
//
// Each workgroup leaves its tiles and its Phi^T r in its own stretch of the workspace;
// gram_reduce_kernel adds the stretches in workgroup order, one thread an element, and
// writes every element of the upper triangle to both of its places (the lower half of
// a diagonal tile is dropped, so G is exactly symmetric).  No atomics anywhere: the
// same inputs give the same bits.
//
// A population.  gram_members_kernel, gram_reduce_members_kernel and predict_members_kernel
// run every member's batch in one launch each: flat grids in which member m owns the
// workgroups its lone grid would have, found through a prefix table, around the SAME
// device functions (gram_body, gram_reduce_body, predict_body) with the workgroup's index
// and count relative to the member -- so every member gets the lone kernels' bits.
#include "common.h"
#include "linear_baseline_params.h"
#include "linear_features.h"

namespace {

typedef double lb_f64x4 __attribute__((ext_vector_type(4)));

// tile p of the upper triangle, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void lb_tile_of(int p, int T, int* ti, int* tj) {
  int i = 0, rem = p;
  while (rem >= T - i) {
    rem -= T - i;
    ++i;
  }
  *ti = i;
  *tj = i + rem;
}

// The Gram pass of ONE batch by workgroup `block` of the `n_blocks` that share it: the body
// of gram_kernel (a batch a launch) and of gram_members_kernel (a population a launch),
// written once.  The workgroup takes slabs block, block + n_blocks, .. and leaves its
// partial in stretch `block` of p.partials.
// One instantiation per number of column tiles T (1 .. 17), so that the waves' tiles and a
// thread's loads are register arrays of exactly the size the shape needs.
template <int T>
__device__ __forceinline__ void gram_body(const LinGramParams& p, const unsigned block,
                                          const unsigned n_blocks) {
  constexpr int TPW = lb_tiles_per_wave_of(T);
  constexpr int NT = T * (T + 1) / 2;
  constexpr int LD = 16 * T + LB_LDS_PAD;
  // observations a fill thread loads: it takes j = fc, fc + 16, .. < O, and
  // O <= 8 T - 2 (F = 2 O + 4 <= 16 T)
  constexpr int U = (T + 1) / 2;
  extern __shared__ double lb_lds[];
  const int O = p.obs_dim, F = p.F;
  const int R = p.chunk_rows;
  double* const feat = lb_lds;                                   // [2][R][LD]
  double* const rets = feat + 2 * R * LD;                        // [2][LB_MAX_CHUNK_ROWS]
  int32_t* const tstep = reinterpret_cast<int32_t*>(rets + 2 * LB_MAX_CHUNK_ROWS);  // [slab]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: so are its tiles)
  // the fill: thread (fr, fc) takes observations fc, fc + 16, .. of chunk row fr
  const int fr = tid >> 4, fc = tid & 15;
  const bool fills = fr < R;

  // this wave's tiles: [wave * TPW, (wave + 1) * TPW) of the NT
  int ti[TPW], tj[TPW];
  lb_f64x4 acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int tile = wave * TPW + q;
    lb_tile_of(tile < NT ? tile : 0, T, &ti[q], &tj[q]);
    acc[q] = lb_f64x4{0.0, 0.0, 0.0, 0.0};
  }
  double bacc = 0.0;  // (Phi^T r)[tid], tid < 16 T

  for (int64_t slab = block; slab < p.n_slabs; slab += n_blocks) {
    const int64_t row0 = slab * LB_SLAB_ROWS;
    const int n_rows = (int)(p.S - row0 < LB_SLAB_ROWS ? p.S - row0 : LB_SLAB_ROWS);
    // ---- every row's step index: LB_SLAB_ROWS / LB_THREADS consecutive rows a thread
    {
      const int r_first = tid * (LB_SLAB_ROWS / LB_THREADS);
      if (r_first < n_rows) {
        int64_t e = lb_episode_of(p.ep_off, p.n_eps, row0 + r_first);
        int64_t start = p.ep_off[e];
        for (int k = 0; k < LB_SLAB_ROWS / LB_THREADS; ++k) {
          const int r = r_first + k;
          if (r >= n_rows) break;
          const int64_t row = row0 + r;
          while (e + 1 < p.n_eps && p.ep_off[e + 1] <= row) {
            ++e;
            start = p.ep_off[e];
          }
          tstep[r] = (int32_t)(row - start);
        }
      }
    }
    __syncthreads();

    const int n_chunks = (n_rows + R - 1) / R;
    float raw[U] = {};  // the loads of the chunk being filled
    float raw_ret = 0.f;
    // issue the loads of chunk c
    auto load_chunk = [&](int c) {
      const int r = c * R + fr;
      if (fills && r < n_rows) {
        const float* obs_row = p.obs + (row0 + r) * p.ldo;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = fc + 16 * u;
          if (j < O) raw[u] = obs_row[j];
        }
      }
      if (tid < R) raw_ret = (c * R + tid < n_rows) ? p.returns[row0 + c * R + tid] : 0.f;
    };
    // form the feature rows of chunk c in buffer c & 1
    auto store_chunk = [&](int c) {
      double* const out = feat + ((c & 1) * R + fr) * LD;
      const int r = c * R + fr;
      if (fills) {
        if (r < n_rows) {
          auto put = [&](int col, double v) { out[col] = v; };
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int j = fc + 16 * u;
            if (j < O) lb_obs_features(raw[u], O, j, put);
          }
          if (fc == 0) lb_time_features(tstep[r], O, put);
          if (F + fc < 16 * T) out[F + fc] = 0.0;  // the last tile's columns from F on
        } else {
#pragma unroll
          for (int t = 0; t < T; ++t) out[16 * t + fc] = 0.0;  // a row past the slab's end
        }
      }
      if (tid < R) rets[(c & 1) * LB_MAX_CHUNK_ROWS + tid] = (double)raw_ret;
    };

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
      const bool more = c + 1 < n_chunks;
      if (more) load_chunk(c + 1);
      const double* const buf = feat + (c & 1) * R * LD;
      // ---- the tiles: a k-step of 4 rows for every tile of the wave in turn, so that
      // consecutive matrix instructions do not wait for one another's result; a tile in
      // the same tile row as the one before it keeps the A operand
      const double* const frag = buf + (lane >> 4) * LD + (lane & 15);
      for (int ks = 0; ks < R / 4; ++ks) {
        const double* const f = frag + 4 * ks * LD;
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
          if (wave * TPW + q < NT) {  // (uniform in the wave)
            if (q == 0 || ti[q] != ti[q - 1]) a = f[16 * ti[q]];
            const double b = f[16 * tj[q]];
            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
          }
          // (a scheduling fence every four tiles: bounds how many operands are loaded
          // ahead of their matrix instruction beside up to 20 tiles' accumulators)
          if (q % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- Phi^T r
      if (tid < 16 * T) {
        const double* const rr = rets + (c & 1) * LB_MAX_CHUNK_ROWS;
        for (int r = 0; r < R; ++r) bacc = fma(buf[r * LD + tid], rr[r], bacc);
      }
      if (more) store_chunk(c + 1);
      __syncthreads();
    }
  }

  // ---- this workgroup's partial
  double* const out = p.partials + (int64_t)block * p.block_doubles;
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int tile = wave * TPW + q;
    if (tile < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[tile * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[q][r];
    }
  }
  if (tid < 16 * T) out[NT * 256 + tid] = bacc;
}

template <int T>
__global__ __launch_bounds__(LB_THREADS) void gram_kernel(const LinGramParams p) {
  gram_body<T>(p, blockIdx.x, gridDim.x);
}

// The member of workgroup `block` of a flat grid: the last m with block0[m] <= block, for
// block0 increasing from 0 (every member owns at least one workgroup).
template <class Member>
__device__ __forceinline__ int lb_member_of(const Member* __restrict__ members, int n_members,
                                            int64_t block) {
  int lo = 0, hi = n_members;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)members[mid].block0 <= block) lo = mid; else hi = mid;
  }
  return lo;
}

// Every member of a population in one launch: the workgroup finds its member, and is
// workgroup blockIdx.x - block0 of the n_blocks of that member's lone grid.
template <int T>
__global__ __launch_bounds__(LB_THREADS) void gram_members_kernel(const LinGramMembersParams g) {
  const int m = lb_member_of(g.members, g.n_members, (int64_t)blockIdx.x);
  const LinGramMemberDev& mem = g.members[m];
  LinGramParams p;
  p.obs = mem.obs; p.ldo = mem.ldo; p.obs_dim = g.obs_dim; p.ep_off = mem.ep_off;
  p.n_eps = mem.n_eps; p.S = mem.S; p.returns = mem.returns; p.partials = mem.partials;
  p.block_doubles = g.block_doubles; p.n_slabs = mem.n_slabs;
  p.F = g.F; p.T = g.T; p.NT = g.NT; p.tpw = g.tpw; p.chunk_rows = g.chunk_rows;
  gram_body<T>(p, blockIdx.x - (unsigned)mem.block0, (unsigned)mem.n_blocks);
}

// element e of a batch's G and b: its workgroups' partials added in workgroup order
__device__ __forceinline__ void gram_reduce_body(const LinReduceParams& p, const int64_t e) {
  if (e >= p.block_doubles) return;
  double sum = 0.0;
  for (int b = 0; b < p.n_blocks; ++b) sum += p.partials[(int64_t)b * p.block_doubles + e];
  const int64_t tile_doubles = (int64_t)p.NT * 256;
  if (e < tile_doubles) {
    int ti, tj;
    lb_tile_of((int)(e >> 8), p.T, &ti, &tj);
    const int i = 16 * ti + (int)((e & 255) >> 4), j = 16 * tj + (int)(e & 15);
    if (j < p.F && i <= j) {  // (i <= j < F)
      p.gram[(int64_t)i * p.F + j] = sum;
      p.gram[(int64_t)j * p.F + i] = sum;
    }
  } else {
    const int c = (int)(e - tile_doubles);
    if (c < p.F) p.rhs[c] = sum;
  }
}

__global__ __launch_bounds__(LB_REDUCE_THREADS) void gram_reduce_kernel(const LinReduceParams p) {
  gram_reduce_body(p, (int64_t)blockIdx.x * LB_REDUCE_THREADS + threadIdx.x);
}

// row blockIdx.y of the grid is member blockIdx.y's reduce launch
__global__ __launch_bounds__(LB_REDUCE_THREADS) void gram_reduce_members_kernel(
    const LinGramMembersParams g) {
  const LinGramMemberDev& mem = g.members[blockIdx.y];
  LinReduceParams p;
  p.partials = mem.partials; p.n_blocks = mem.n_blocks; p.block_doubles = g.block_doubles;
  p.F = g.F; p.T = g.T; p.NT = g.NT; p.gram = mem.gram; p.rhs = mem.rhs;
  gram_reduce_body(p, (int64_t)blockIdx.x * LB_REDUCE_THREADS + threadIdx.x);
}

// one thread a row; the sum runs in feature order, in fp64
__device__ __forceinline__ void predict_body(const LinPredictParams& p, const int64_t row) {
  if (row >= p.S) return;
  const int64_t e = lb_episode_of(p.ep_off, p.n_eps, row);
  const int64_t t = row - p.ep_off[e];
  const float* obs_row = p.obs + row * p.ldo;
  const int O = p.obs_dim;
  double v = 0.0;
  // (an observation gives two columns O apart: one walk for each, to keep the order)
  for (int j = 0; j < O; ++j)
    lb_obs_features(obs_row[j], O, j, [&](int col, double f) {
      if (col < O) v = fma(f, p.coeffs[col], v);
    });
  for (int j = 0; j < O; ++j)
    lb_obs_features(obs_row[j], O, j, [&](int col, double f) {
      if (col >= O) v = fma(f, p.coeffs[col], v);
    });
  lb_time_features(t, O, [&](int col, double f) { v = fma(f, p.coeffs[col], v); });
  p.values[row * p.ldv] = (float)v;
}

__global__ __launch_bounds__(LB_PREDICT_THREADS) void predict_kernel(const LinPredictParams p) {
  predict_body(p, (int64_t)blockIdx.x * LB_PREDICT_THREADS + threadIdx.x);
}

// Every member of a population in one launch; a member without coefficients (a baseline
// before its first fit) gets zeros.
__global__ __launch_bounds__(LB_PREDICT_THREADS) void predict_members_kernel(
    const LinPredictMembersParams g) {
  const int m = lb_member_of(g.members, g.n_members, (int64_t)blockIdx.x);
  const LinPredictMemberDev& mem = g.members[m];
  const int64_t row =
      ((int64_t)blockIdx.x - mem.block0) * LB_PREDICT_THREADS + threadIdx.x;
  if (!mem.coeffs) {
    if (row < mem.S) mem.values[row * mem.ldv] = 0.f;
    return;
  }
  LinPredictParams p;
  p.obs = mem.obs; p.ldo = mem.ldo; p.obs_dim = g.obs_dim; p.ep_off = mem.ep_off;
  p.n_eps = mem.n_eps; p.S = mem.S; p.coeffs = mem.coeffs; p.values = mem.values;
  p.ldv = mem.ldv;
  predict_body(p, row);
}

}  // namespace

// ---- the launch seam (linear_baseline_params.h): instantiate and launch, nothing else -----
void lb_launch_gram(const LinGramParams& p, unsigned blocks, unsigned lds_bytes,
                    hipStream_t stream) {
#define LB_GRAM(T)                                                                       \
  case T:                                                                                \
    hipLaunchKernelGGL(gram_kernel<T>, dim3(blocks), dim3(LB_THREADS), lds_bytes, stream, p); \
    break
  switch (p.T) {
    LB_GRAM(1); LB_GRAM(2); LB_GRAM(3); LB_GRAM(4); LB_GRAM(5); LB_GRAM(6);
    LB_GRAM(7); LB_GRAM(8); LB_GRAM(9); LB_GRAM(10); LB_GRAM(11); LB_GRAM(12);
    LB_GRAM(13); LB_GRAM(14); LB_GRAM(15); LB_GRAM(16); LB_GRAM(17);
  }
#undef LB_GRAM
}
void lb_launch_gram_members(const LinGramMembersParams& p, unsigned blocks, unsigned lds_bytes,
                            hipStream_t stream) {
#define LB_GRAM(T)                                                                          \
  case T:                                                                                   \
    hipLaunchKernelGGL(gram_members_kernel<T>, dim3(blocks), dim3(LB_THREADS), lds_bytes,   \
                       stream, p);                                                          \
    break
  switch (p.T) {
    LB_GRAM(1); LB_GRAM(2); LB_GRAM(3); LB_GRAM(4); LB_GRAM(5); LB_GRAM(6);
    LB_GRAM(7); LB_GRAM(8); LB_GRAM(9); LB_GRAM(10); LB_GRAM(11); LB_GRAM(12);
    LB_GRAM(13); LB_GRAM(14); LB_GRAM(15); LB_GRAM(16); LB_GRAM(17);
  }
#undef LB_GRAM
}
void lb_launch_gram_reduce_members(const LinGramMembersParams& p, unsigned blocks,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(gram_reduce_members_kernel, dim3(blocks, (unsigned)p.n_members),
                     dim3(LB_REDUCE_THREADS), 0, stream, p);
}
void lb_launch_predict_members(const LinPredictMembersParams& p, unsigned blocks,
                               hipStream_t stream) {
  hipLaunchKernelGGL(predict_members_kernel, dim3(blocks), dim3(LB_PREDICT_THREADS), 0, stream,
                     p);
}
void lb_launch_gram_reduce(const LinReduceParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(gram_reduce_kernel, dim3(blocks), dim3(LB_REDUCE_THREADS), 0, stream, p);
}
void lb_launch_predict(const LinPredictParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(predict_kernel, dim3(blocks), dim3(LB_PREDICT_THREADS), 0, stream, p);
}
