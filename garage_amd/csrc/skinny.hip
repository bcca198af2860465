// Bandwidth-bound layer products of the MLP update (gfx950).
//
// An MLP whose input (observations) or head (action mean / value) is narrow has
// four products per minibatch in which one dimension is <= 32:
//   first-layer forward      H1 = tanh(X W0^T + b0)        K = obs_dim
//   head data gradient       dZ = (dout W_head) * (1 - H^2) K = act_dim
//   first-layer weight grad  dW0 = dZ1^T X                  one side = obs_dim
//   head weight grad         dW_head = dout^T H             one side = act_dim
// (reference: the nn.Linear forward/backward of torch/modules/mlp_module.py:62-73
// under torch/algos/vpg.py:250-293).  Each moves one full [rows x hidden]
// activation matrix (33.5 MB at the C3 minibatch) for a few flops per byte, so
// they are HBM/latency bound: an MFMA tile pipeline (load -> LDS -> MFMA -> store,
// one resident wave of workgroups in lock step) exposes every phase.  Here they
// are plain streaming kernels: a thread owns 4 adjacent hidden columns, rows
// stream through registers with several 16-B loads in flight per thread, the
// narrow operand is staged in LDS and read back as same-address broadcasts, and
// the arithmetic is a sequential fp32 FMA chain on the vector ALU.
#include "common.h"
#include <hip/hip_ext.h>

#include "prof.h"

#include "members_diag.h"
#include "layer_plans.h"  // SkinnyFwdParams, SkinnyWgradParams; shape_rules.h: SK_*, SW_*

namespace {

__device__ __forceinline__ float tanh_fast(float x) {
  return ga_tanh(x);  // common.h
}

// ---------------------------------------------------------------------------
// Y[m, n] = epi(sum_k X[row(m), k] * W(n, k)),  K <= 32, N = 4 * QPR * n_colblk
// ---------------------------------------------------------------------------
typedef float sk_v2f __attribute__((ext_vector_type(2)));

// KV = round4(K) / 4 float4 of the narrow operand per row.  The X rows of the
// workgroup are staged once in LDS (one gathered 16-B load per vector) and read
// back as same-address broadcasts, so the per-row cost is KV ds_read_b128 + 16 KV
// FMAs + one 16-B store per thread.
template <int KV, bool W_KC, int EPI>
__global__ __launch_bounds__(SK_THREADS) void skinny_fwd_kernel(SkinnyFwdParams p) {
#include "skinny_fwd_body.inc"
}

// The same product for every entry of a device table in one grid (members_diag.h): entry
// blockIdx.z, whose own grid the launch's (x, y) covers or exceeds.
template <int KV>
__global__ __launch_bounds__(SK_THREADS) void skinny_fwd_members_kernel(
    const MdSkinnyEntry* table) {
  constexpr bool W_KC = true;
  constexpr int EPI = 0;
  const MdSkinnyEntry md_entry = table[blockIdx.z];
  if (blockIdx.x >= md_entry.gx || blockIdx.y >= md_entry.gy) return;
  const SkinnyFwdParams& p = md_entry.p;
#include "skinny_fwd_body.inc"
}

// ---------------------------------------------------------------------------
// C(wide c, narrow j) = sum_r Wd[row_w(r), c] * Nr[row_n(r), j] per split of rows
// ---------------------------------------------------------------------------
constexpr int SW_CHUNK = 256;          // rows of the narrow operand staged at a time
constexpr int SW_LDS_FLOATS = 8192;    // 32 KB: narrow stage, then reduction stage

// One workgroup = (64 wide columns) x (one split of the rows): 16 row groups of
// 16 threads; a thread owns 4 columns and keeps 2 x UNROLL 16-B loads of the wide
// operand in flight (the loads of the next step are issued before the FMAs of
// the current one).  grid = (wide / 64, n_splits): 512 workgroups at the C3
// minibatch, several per CU.
// NV = round4(NS) / 4; NSUM: also the column sums of the narrow operand; DZ: also
// the data gradient of the layer below (the wide operand is then its tanh output)
template <int NV, bool NSUM, bool DZ = false>
// (two waves per SIMD: a streaming kernel lives on the loads it has in flight; left
// alone the compiler takes 280-350 registers for the DZ variants: one wave per SIMD)
__global__ __launch_bounds__(SW_THREADS, (DZ && NV >= 4) ? 1 : 2) void skinny_wgrad_kernel(
    SkinnyWgradParams p) {
  constexpr int U = NV <= 2 ? (DZ ? 4 : 8) : 4;
  __shared__ __attribute__((aligned(16))) float red[SW_LDS_FLOATS];
  const int tid = threadIdx.x;
  const int q = tid % p.qpr;
  const int rg = tid / p.qpr;
  const int n_rg = SW_THREADS / p.qpr;
  // the column blocks of a split read the same narrow rows: same XCD (common.h)
  int split, colblk;
  ga_xcd_group((int)blockIdx.x, p.n_splits, p.n_colblk, &split, &colblk);
  const int c0 = (colblk * p.qpr + q) * 4;
  const bool col_ok = c0 < p.wide;
  const int cc = col_ok ? c0 : 0;
  const int r_beg = split * p.rows_per_split;
  const int r_end = min(p.rows, r_beg + p.rows_per_split);

  float4 acc[4 * NV];   // acc[j] = C(c0..c0+3, j)
  float4 wsum = make_float4(0.f, 0.f, 0.f, 0.f);
  float nsum[NSUM ? 4 * NV : 1];
#pragma unroll
  for (int j = 0; j < 4 * NV; ++j) {
    acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NSUM) nsum[j] = 0.f;
  }
  const bool want_nsum = NSUM && colblk == 0 && q == 0;
  float4 wq[DZ ? 4 * NV : 1];  // head weights of this thread's 4 columns
  if (DZ) {
#pragma unroll
    for (int j = 0; j < 4 * NV; ++j)
      wq[j] = (j < p.NS) ? *reinterpret_cast<const float4*>(p.Wn + (int64_t)j * p.ldwn + cc)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  for (int rc = r_beg; rc < r_end; rc += SW_CHUNK) {
    const int rc_end = min(r_end, rc + SW_CHUNK);
    float4 w[U], wn[U];
    // first step's wide loads go out before the narrow stage is waited for
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = min(rc + rg + u * n_rg, rc_end - 1);
      const int64_t rw = p.w_idx ? (int64_t)p.w_idx[r] : (int64_t)r;
      w[u] = *reinterpret_cast<const float4*>(p.Wd + rw * p.ldw + cc);
    }
    __syncthreads();
    for (int i = tid; i < SW_CHUNK * NV; i += SW_THREADS) {
      const int r = i / NV, v = i % NV;
      const int row = min(rc + r, r_end - 1);
      const int64_t src = p.n_idx ? (int64_t)p.n_idx[row] : (int64_t)row;
      float4 nv4 = *reinterpret_cast<const float4*>(p.Nr + src * p.ldn + 4 * v);
      if (DZ) {  // padding columns may hold anything: they must not reach dz
        nv4.x = (4 * v + 0 < p.NS) ? nv4.x : 0.f;
        nv4.y = (4 * v + 1 < p.NS) ? nv4.y : 0.f;
        nv4.z = (4 * v + 2 < p.NS) ? nv4.z : 0.f;
        nv4.w = (4 * v + 3 < p.NS) ? nv4.w : 0.f;
      }
      *reinterpret_cast<float4*>(red + (r * NV + v) * 4) = nv4;
    }
    __syncthreads();
    for (int rb = rc + rg; rb < rc_end; rb += n_rg * U) {
      const int rb_next = rb + n_rg * U;
      if (rb_next < rc_end) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int r = min(rb_next + u * n_rg, rc_end - 1);
          const int64_t rw = p.w_idx ? (int64_t)p.w_idx[r] : (int64_t)r;
          wn[u] = *reinterpret_cast<const float4*>(p.Wd + rw * p.ldw + cc);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = rb + u * n_rg;
        const bool live = r < rc_end;
        const int rl = min(r, rc_end - 1) - rc;
        const float4 wv = live ? w[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        wsum.x += wv.x; wsum.y += wv.y; wsum.z += wv.z; wsum.w += wv.w;
        float4 dz = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float4 nv = *reinterpret_cast<const float4*>(red + (rl * NV + v) * 4);
          const float ns[4] = {nv.x, nv.y, nv.z, nv.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float4& a = acc[4 * v + j];
            a.x = fmaf(wv.x, ns[j], a.x);
            a.y = fmaf(wv.y, ns[j], a.y);
            a.z = fmaf(wv.z, ns[j], a.z);
            a.w = fmaf(wv.w, ns[j], a.w);
            if (NSUM && want_nsum && live) nsum[4 * v + j] += ns[j];
            if (DZ) {
              const float4 wn = wq[4 * v + j];
              dz.x = fmaf(ns[j], wn.x, dz.x);
              dz.y = fmaf(ns[j], wn.y, dz.y);
              dz.z = fmaf(ns[j], wn.z, dz.z);
              dz.w = fmaf(ns[j], wn.w, dz.w);
            }
          }
        }
        if (DZ && live && col_ok) {
          dz.x *= (1.f - wv.x * wv.x); dz.y *= (1.f - wv.y * wv.y);
          dz.z *= (1.f - wv.z * wv.z); dz.w *= (1.f - wv.w * wv.w);
          *reinterpret_cast<float4*>(p.dz_out + (int64_t)r * p.lddz + c0) = dz;
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the LDS reads row by row
      }
#pragma unroll
      for (int u = 0; u < U; ++u) w[u] = wn[u];
    }
  }

  // ---- sum the row groups in a fixed order through LDS, a few j at a time
  float* Cs = p.C + (int64_t)split * p.split_stride;
  const int quads = p.qpr;                         // float4 per (group, j)
  const int per_j = n_rg * quads * 4;              // = 1024 floats staged per j
  const int jp = SW_LDS_FLOATS / per_j;            // j per pass
  constexpr int n_j = 4 * NV + 1;                  // + 1: the wide column sums
  for (int j0 = 0; j0 < n_j; j0 += jp) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < n_j; ++j) {
      if (j >= j0 && j < j0 + jp) {
        const float4 v = (j < 4 * NV) ? acc[j < 4 * NV ? j : 0] : wsum;
        *reinterpret_cast<float4*>(red + ((j - j0) * n_rg + rg) * quads * 4 + q * 4) = v;
      }
    }
    __syncthreads();
    const int jn = min(jp, n_j - j0);
    for (int o = tid; o < jn * quads; o += SW_THREADS) {
      const int jj = o / quads, qq = o % quads;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int g = 0; g < n_rg; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(
            red + (jj * n_rg + g) * quads * 4 + qq * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      const int j = j0 + jj;
      const int c = (colblk * p.qpr + qq) * 4;
      if (c >= p.wide) continue;
      if (j < 4 * NV) {
        if (j >= p.NS) continue;
        if (p.c_wide_stride == 1) {
          *reinterpret_cast<float4*>(Cs + (int64_t)j * p.c_narrow_stride + c) = s;
        } else {
          Cs[(int64_t)(c + 0) * p.c_wide_stride + j * p.c_narrow_stride] = s.x;
          Cs[(int64_t)(c + 1) * p.c_wide_stride + j * p.c_narrow_stride] = s.y;
          Cs[(int64_t)(c + 2) * p.c_wide_stride + j * p.c_narrow_stride] = s.z;
          Cs[(int64_t)(c + 3) * p.c_wide_stride + j * p.c_narrow_stride] = s.w;
        }
      } else if (p.colsum_wide) {
        *reinterpret_cast<float4*>(p.colsum_wide + (int64_t)split * p.split_stride + c) = s;
      }
    }
  }
  // ---- narrow column sums: thread q == 0 of every row group holds a partial
  if (NSUM && colblk == 0) {
    __syncthreads();
    if (q == 0) {
#pragma unroll
      for (int j = 0; j < 4 * NV; ++j) red[rg * 4 * NV + j] = nsum[j];
    }
    __syncthreads();
    if (tid < p.NS) {
      float s = 0.f;
      for (int g = 0; g < n_rg; ++g) s += red[g * 4 * NV + tid];
      p.colsum_narrow[(int64_t)split * p.split_stride + tid] = s;
    }
  }
}

// ---- the launch seam (layer_plans.h): the plan's words become an instantiation
template <int KV>
void launch_fwd(const SkinnyFwdPlan& plan, const SkinnyFwdParams& p, hipStream_t stream,
                hipEvent_t e0, hipEvent_t e1) {
  const dim3 grid(plan.gx, plan.gy);
  if (plan.w_kc && plan.epi == 0)
    hipExtLaunchKernelGGL((skinny_fwd_kernel<KV, true, 0>), grid, dim3(SK_THREADS),
                          plan.lds_bytes, stream, e0, e1, 0, p);
  else if (!plan.w_kc && plan.epi == 1)
    hipExtLaunchKernelGGL((skinny_fwd_kernel<KV, false, 1>), grid, dim3(SK_THREADS),
                          plan.lds_bytes, stream, e0, e1, 0, p);
}

template <int NV>
void launch_wgrad(const SkinnyWgradPlan& plan, const SkinnyWgradParams& p, hipStream_t stream,
                  hipEvent_t e0, hipEvent_t e1) {
  const dim3 grid(plan.grid), block(SW_THREADS);
  if constexpr (NV <= 4) {  // (SW_NS_MAX_DZ)
    if (plan.variant == SWV_DZ) {
      hipExtLaunchKernelGGL((skinny_wgrad_kernel<NV, true, true>), grid, block, 0, stream, e0,
                            e1, 0, p);
      return;
    }
  }
  if (plan.variant == SWV_NSUM)
    hipExtLaunchKernelGGL((skinny_wgrad_kernel<NV, true>), grid, block, 0, stream, e0, e1, 0, p);
  else if (plan.variant == SWV_PLAIN)
    hipExtLaunchKernelGGL((skinny_wgrad_kernel<NV, false>), grid, block, 0, stream, e0, e1, 0,
                          p);
}

}  // namespace

int ga_skinny_fwd_launch(const SkinnyFwdPlan& plan, const SkinnyFwdParams& p,
                         hipStream_t stream) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_SKINNY_FWD, plan.work, &e0, &e1);
  switch (plan.KV) {
    case 1: launch_fwd<1>(plan, p, stream, e0, e1); break;
    case 2: launch_fwd<2>(plan, p, stream, e0, e1); break;
    case 3: launch_fwd<3>(plan, p, stream, e0, e1); break;
    case 4: launch_fwd<4>(plan, p, stream, e0, e1); break;
    case 5: launch_fwd<5>(plan, p, stream, e0, e1); break;
    case 6: launch_fwd<6>(plan, p, stream, e0, e1); break;
    case 7: launch_fwd<7>(plan, p, stream, e0, e1); break;
    default: launch_fwd<8>(plan, p, stream, e0, e1); break;
  }
  GA_CHECK_LAUNCH("skinny_fwd");
  return GA_OK;
}

int md_launch_skinny_fwd_members(int KV, const MdSkinnyEntry* table, unsigned n, unsigned gx,
                                 unsigned gy, unsigned lds_bytes, hipStream_t stream) {
  ga_prof_count(GA_PROF_SKINNY_FWD);  // (one launch of the lone kernel's kind, never timed)
  const dim3 grid(gx, gy, n), block(SK_THREADS);
  switch (KV) {
#define MD_CASE(V)                                                                          \
  case V:                                                                                   \
    hipLaunchKernelGGL((skinny_fwd_members_kernel<V>), grid, block, lds_bytes, stream, table); \
    break;
    MD_CASE(1) MD_CASE(2) MD_CASE(3) MD_CASE(4) MD_CASE(5) MD_CASE(6) MD_CASE(7) MD_CASE(8)
#undef MD_CASE
    default:
      ga_set_error("skinny_fwd_members: KV %d not instantiated", KV);
      return GA_ERR_ARG;
  }
  GA_CHECK_LAUNCH("skinny_fwd_members");
  return GA_OK;
}

int ga_skinny_wgrad_launch(const SkinnyWgradPlan& plan, const SkinnyWgradParams& p,
                           hipStream_t stream) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_SKINNY_WGRAD, plan.work, &e0, &e1);
  switch (plan.NV) {
    case 1: launch_wgrad<1>(plan, p, stream, e0, e1); break;
    case 2: launch_wgrad<2>(plan, p, stream, e0, e1); break;
    case 3: launch_wgrad<3>(plan, p, stream, e0, e1); break;
    case 4: launch_wgrad<4>(plan, p, stream, e0, e1); break;
    case 5: launch_wgrad<5>(plan, p, stream, e0, e1); break;
    default: launch_wgrad<6>(plan, p, stream, e0, e1); break;
  }
  GA_CHECK_LAUNCH("skinny_wgrad");
  return GA_OK;
}
