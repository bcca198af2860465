// A population's joint pack (ga_member_pack_index / ga_member_pack_gather,
// member_pack_host.cpp): every member's episodes in batch order, the cell of every packed
// sample and all planes of the batch, in three launches whatever the number of members.
// What GpuVecWorker._pack does per member with ga_pack_episodes, ga_pack_src_index and
// the gathers (rollout.hip) -- EpisodeBatch.concatenate in completion order,
// sampler/vec_worker.py:206-219.
//
// The rollout buffers are env-major ([n, Tcap, w]), so an episode is one contiguous run
// in source and destination: consecutive rows of the packed arrays read consecutive
// cells, and a wave's 16-byte pieces are contiguous on both sides except where an
// episode ends.  No atomics: ga_member_progress' col_base gives a column's first
// episode, the rank inside the column is counted by the column's own thread.
#include "member_pack.h"

namespace {

__device__ __forceinline__ int64_t round16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// Inclusive sum of `a` over the block's 256 threads; *total: the block's sum.
__device__ __forceinline__ void block_scan_256(int64_t& a, int64_t* smem4, int64_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t u = __shfl_up(a, o, 64);
    if (lane >= o) a += u;
  }
  if (lane == 63) smem4[w] = a;
  __syncthreads();
  int64_t s = 0;
  for (int k = 0; k < w; ++k) s += smem4[k];
  *total = smem4[0] + smem4[1] + smem4[2] + smem4[3];
  a += s;
  __syncthreads();
}

// Sums of (a, b) over the block, in every thread.
__device__ __forceinline__ void block_sum2_256(int64_t& a, int64_t& b, int64_t (*smem)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, 64);
    b += __shfl_down(b, o, 64);
  }
  if (lane == 0) { smem[w][0] = a; smem[w][1] = b; }
  __syncthreads();
  a = smem[0][0] + smem[1][0] + smem[2][0] + smem[3][0];
  b = smem[0][1] + smem[1][1] + smem[2][1] + smem[3][1];
  __syncthreads();
}

// (member_off, episode_start) of member m: the rows, rounded up to 16 per member, and
// the episodes of the members before it.  with_rows 0: the episodes only (the members'
// sample counts are not written yet).
__device__ __forceinline__ void member_bases(const GaPackIndexArgs& a, int m, int with_rows,
                                             int64_t (*smem)[2], int64_t* row0,
                                             int64_t* ep0) {
  int64_t rows = 0, eps = 0;
  for (int k = threadIdx.x; k < m; k += 256) {
    if (with_rows) rows += round16(a.member_samples[k]);
    if (a.progress[3 * k]) eps += a.progress[3 * k + 1];
  }
  block_sum2_256(rows, eps, smem);
  *row0 = rows;
  *ep0 = eps;
}

// One block per member, one thread per column t < c_m (consecutive threads read
// consecutive cells of a row, as member_progress_kernel): the column's steps, a scan
// over the columns for its first sample, then the column's episodes by env index from
// col_base[m, t] on.
__global__ __launch_bounds__(256) void member_episodes_kernel(GaPackIndexArgs a) {
  __shared__ int64_t part[4];
  __shared__ int64_t sums[4][2];
  const int m = blockIdx.x;
  // (block-uniform) 0: the member contributes nothing; never past the columns stepped
  const int c = min(a.progress[3 * m], a.n_cols);
  int64_t unused, ep0;
  member_bases(a, m, 0, sums, &unused, &ep0);
  const int64_t env0 = (int64_t)m * a.g;
  const uint16_t* rows = a.tail + env0 * a.Tcap;
  int64_t carry = 0;  // the member's steps in the columns before t0
  for (int t0 = 0; t0 < c; t0 += 256) {
    const int t = t0 + (int)threadIdx.x;
    int64_t s = 0;
    if (t < c)
      for (int64_t i = 0; i < a.g; ++i) {
        // (an episode cannot be longer than the columns behind it)
        s += min((int)rows[i * a.Tcap + t], t + 1);
      }
    int64_t cs = s, total;
    block_scan_256(cs, part, &total);
    if (t < c) {
      int64_t off = carry + cs - s;
      int64_t e = ep0 + a.col_base[(int64_t)m * a.Tcap + t];
      for (int64_t i = 0; i < a.g; ++i) {
        const int L = min((int)rows[i * a.Tcap + t], t + 1);
        if (L > 0) {
          if (e < a.max_eps) {
            a.ep_env[e] = (int32_t)(env0 + i);
            a.ep_end[e] = t;
            a.ep_len[e] = L;
            a.ep_off[e + m] = off;
          }
          off += L;
          ++e;
        }
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    const int64_t last = ep0 + (c ? a.progress[3 * m + 1] : 0);
    if (last <= a.max_eps) a.ep_off[last + m] = carry;  // the closing entry: S_m
    a.member_samples[m] = carry;
  }
}

// grid (x, member): row r of the member's slice -> its cell, found by bisecting the
// member's episode offsets (L2-resident); -1 behind the member's samples, for the last
// member up to max_samples.
__global__ __launch_bounds__(256) void member_src_kernel(GaPackIndexArgs a) {
  __shared__ int64_t sums[4][2];
  const int m = blockIdx.y;
  int64_t row0, ep0;
  member_bases(a, m, 1, sums, &row0, &ep0);
  const int64_t S = a.member_samples[m];
  const bool last = m == a.n_members - 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.member_off[m] = row0;
    if (last) a.member_off[m + 1] = row0 + round16(S);
  }
  int64_t n_e = a.progress[3 * m] ? a.progress[3 * m + 1] : 0;
  n_e = max((int64_t)0, min(n_e, a.max_eps - ep0));  // the episodes that were written
  const int64_t* offs = a.ep_off + ep0 + m;
  const int64_t rows = min(last ? a.max_samples : row0 + round16(S), a.max_samples) - row0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows;
       r += (int64_t)gridDim.x * 256) {
    int32_t cell = -1;
    if (r < S && n_e > 0) {
      int64_t lo = 0, hi = n_e;  // offs[lo] <= r < offs[hi]
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (offs[mid] <= r) lo = mid; else hi = mid;
      }
      const int64_t e = ep0 + lo, j = r - offs[lo];
      const int L = a.ep_len[e];
      if (j < L) cell = (int32_t)((int64_t)a.ep_env[e] * a.Tcap + (a.ep_end[e] - L + 1) + j);
    }
    a.src[row0 + r] = cell;
  }
}

// ---- the planes --------------------------------------------------------------------
__device__ __forceinline__ int64_t cell_of(const GaPackTable& t, int per_episode,
                                           int64_t r) {
  return per_episode ? (int64_t)t.ep_env[r] * t.Tcap + t.ep_end[r] : (int64_t)t.src[r];
}

template <typename T, typename T4>
__device__ __forceinline__ void copy_scalar4(const GaPackTable& t, const GaPackPlaneDev& p,
                                             int64_t u) {
  const T* src = static_cast<const T*>(p.src);
  T* dst = static_cast<T*>(p.dst);
  const int64_t r0 = 4 * u;
  if (r0 + 3 < p.rows) {
    int64_t c[4];
    if (!p.per_episode && (reinterpret_cast<uintptr_t>(t.src) & 15u) == 0) {
      const int4 q = *reinterpret_cast<const int4*>(t.src + r0);
      c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = cell_of(t, p.per_episode, r0 + k);
    }
    T4 v;
    v.x = c[0] >= 0 ? src[c[0] * p.ld_src] : T(0);
    v.y = c[1] >= 0 ? src[c[1] * p.ld_src] : T(0);
    v.z = c[2] >= 0 ? src[c[2] * p.ld_src] : T(0);
    v.w = c[3] >= 0 ? src[c[3] * p.ld_src] : T(0);
    *reinterpret_cast<T4*>(dst + r0) = v;  // (dst is aligned to four elements)
  } else {
    for (int64_t r = r0; r < p.rows; ++r) {
      const int64_t c = cell_of(t, p.per_episode, r);
      dst[r] = c >= 0 ? src[c * p.ld_src] : T(0);
    }
  }
}

template <typename T>
__device__ __forceinline__ void copy_elem(const GaPackTable& t, const GaPackPlaneDev& p,
                                          int64_t u) {
  const int64_t row = u / p.width;
  const int j = (int)(u - row * p.width);
  const int64_t c = cell_of(t, p.per_episode, row);
  static_cast<T*>(p.dst)[row * p.ld_dst + j] =
      c >= 0 ? static_cast<const T*>(p.src)[c * p.ld_src + j] : T(0);
}

// grid (x, plane); the plane's path is block-uniform
__global__ __launch_bounds__(256) void member_gather_kernel(GaPackTable t) {
  const GaPackPlaneDev p = t.plane[blockIdx.y];
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (p.path == GA_PACK_QUADS) {
    const float* src = static_cast<const float*>(p.src);
    float* dst = static_cast<float*>(p.dst);
    const int w4 = p.width >> 2;
    const bool narrow = p.units < (1ll << 32);  // (32-bit division where it fits)
    for (int64_t u = first; u < p.units; u += stride) {
      const int64_t row = w4 == 1 ? u
                          : narrow ? (int64_t)((uint32_t)u / (uint32_t)w4) : u / w4;
      const int v = (int)(u - row * w4);
      const int64_t c = cell_of(t, p.per_episode, row);
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c >= 0) x = *reinterpret_cast<const float4*>(src + c * p.ld_src + 4 * v);
      *reinterpret_cast<float4*>(dst + row * p.ld_dst + 4 * v) = x;
    }
  } else if (p.path == GA_PACK_SCALAR) {
    for (int64_t u = first; u < p.units; u += stride) {
      if (p.elem_size == 4) copy_scalar4<float, float4>(t, p, u);
      else copy_scalar4<uint8_t, uchar4>(t, p, u);
    }
  } else {
    for (int64_t u = first; u < p.units; u += stride) {
      if (p.elem_size == 4) copy_elem<float>(t, p, u);
      else copy_elem<uint8_t>(t, p, u);
    }
  }
}

}  // namespace

extern "C" int ga_launch_member_episodes(const GaPackIndexArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(member_episodes_kernel, dim3((unsigned)a->n_members), dim3(256), 0,
                     stream, *a);
  GA_CHECK_LAUNCH("member_episodes");
  return GA_OK;
}

extern "C" int ga_launch_member_src(const GaPackIndexArgs* a, int64_t blocks_x,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(member_src_kernel, dim3((unsigned)blocks_x, (unsigned)a->n_members),
                     dim3(256), 0, stream, *a);
  GA_CHECK_LAUNCH("member_src");
  return GA_OK;
}

extern "C" int ga_launch_member_gather(const GaPackTable* t, int64_t blocks_x,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(member_gather_kernel, dim3((unsigned)blocks_x, (unsigned)t->n_planes),
                     dim3(256), 0, stream, *t);
  GA_CHECK_LAUNCH("member_gather");
  return GA_OK;
}
