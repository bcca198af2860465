// One optimizer step of a POPULATION of narrow networks in two launches (gfx950).
//
// A member of a population trains on a few thousand samples: a minibatch is one to four
// 64-row tiles of narrow_train_kernel, a handful of workgroups on a chip with 256 CUs,
// and a population trained member after member pays two launches per member, network
// and minibatch.  Here step k of EVERY member goes out as two launches:
//   narrow_train_members_kernel   narrow_train_kernel's body (narrow_body.h) for tile
//                                 blockIdx.x of member blockIdx.y, described by a
//                                 device-resident table (members_step.h)
//   reduce_members_adam_kernel    reduce_regions_adam_kernel's arithmetic -- the same
//                                 summation trees (reduce_trees.h), loss finish
//                                 (loss_rows.h) and Adam (common.h) -- per member, with
//                                 the member's own Adam constants from a device table
// Each member gets, bit for bit, what the lone pair of launches gives a lone learner on
// the member's minibatch: tile t of a member covers the rows tile t of the lone launch
// covers and writes the same shares; the shares are summed by the tree the lone
// optimizer launch picks for that many partials.  A member whose pass has no step k is
// inactive: both kernels return for it before touching memory.
#include "common.h"

#include "prof.h"

#include "fused_train.h"
#include "loss_rows.h"
#include "members_step.h"
#include "narrow_body.h"
#include "reduce_trees.h"

namespace {

struct MembersTrainParams {
  GaMembersShared sh;
  const GaMemberDev* table;
  int k;
};

// rows of member m's step k (0: none)
__device__ __forceinline__ int members_rows(const GaMemberDev& m, const GaMembersShared& sh,
                                            int k) {
  if (k >= m.n_steps) return 0;
  return k == m.n_steps - 1 ? m.last_M : (int)sh.mb;
}

__device__ __forceinline__ LossRowArgs members_loss(const GaMemberDev& m,
                                                    const GaMembersShared& sh, int k,
                                                    int M) {
  LossRowArgs L;
  L.kind = sh.kind; L.actions = m.actions; L.lda = m.lda; L.old_ll = m.old_ll;
  L.adv = m.adv; L.returns = m.returns;
  L.idx = m.perm ? m.perm + (int64_t)k * sh.mb : nullptr;
  L.log_std = m.params;
  L.has_min = sh.has_min; L.has_max = sh.has_max; L.min_log_std = sh.min_log_std;
  L.max_log_std = sh.max_log_std; L.A = sh.out_w; L.algo = sh.algo; L.clip = m.clip;
  L.ent = lr_ent(m.ent_coeff, sh.ent_flags);
  L.double_softmax = sh.double_softmax;
  L.invM = k == m.n_steps - 1 ? m.inv_last : m.inv_full;
  return L;
}

// Grid (max tiles of a member in this step, n_members); a workgroup beyond its
// member's tiles returns.  Every global access is the body's own, behind the body's
// bounds tests on the member's M (narrow_body.h).
template <int H, int NS_LDX>
__global__ __launch_bounds__(NS_THREADS, NS_LDX <= 20 ? 2 : 1) void
narrow_train_members_kernel(MembersTrainParams q) {
  const GaMemberDev& m = q.table[blockIdx.y];
  const int M = members_rows(m, q.sh, q.k);
  const int tile = blockIdx.x;
  if (tile * NS_ROWS >= M) return;
  NarrowParams p;
  p.params = m.params;
#pragma unroll
  for (int l = 0; l < 3; ++l) { p.w_off[l] = q.sh.w_off[l]; p.b_off[l] = q.sh.b_off[l]; }
  p.in_w = q.sh.in_w; p.out_w = q.sh.out_w; p.M = M;
  p.X = m.X; p.ldx = m.ldx;
  p.loss = members_loss(m, q.sh, q.k, M);
  p.part = m.part; p.stride = q.sh.stride; p.lpart = m.lpart;
  p.dbg = nullptr;
  narrow_train_body<H, NS_LDX>(p, tile);
}

// The six regions of a narrow network (W0 | b0 | W1 | b1 | 8 head rows | 8), the same
// for every member: flat range [beg, beg + n) and where a tile's share of it starts.
// A member's regions are summed with quads = 64 when its step has <= 128 tiles and 16
// above, the lone optimizer launch's rule, so a region has two workgroup ranges.
constexpr int MB_REGIONS = 6;
struct MembersRegion {
  int64_t beg, n, src_off;
  int vbeg[2];  // first workgroup of the region at quads = 64 / 16
};
struct MembersReduceParams {
  GaMembersShared sh;
  const GaMemberDev* table;
  const GaAdam* adam;  // [n_members]: this step's constants
  int k;
  MembersRegion r[MB_REGIONS];
  int n_virtual[2];    // workgroups over all regions at quads = 64 / 16
};

// Grid (n_virtual + 1, n_members), n_virtual = n_virtual[0] when no member has more
// than 128 tiles in this step and n_virtual[1] otherwise: the last workgroup of a
// member finishes its loss, the others take Q quads of a region each (in the wider
// grid those beyond n_virtual[0] return for a member summed with Q = 64).
__global__ __launch_bounds__(256) void reduce_members_adam_kernel(MembersReduceParams p) {
  __builtin_amdgcn_s_setprio(3);
  const GaMemberDev& m = p.table[blockIdx.y];
  const int M = members_rows(m, p.sh, p.k);
  if (M <= 0) return;
  const int n_part = (M + NS_ROWS - 1) / NS_ROWS;
  const GaAdam adam = p.adam[blockIdx.y];
  if (blockIdx.x == gridDim.x - 1) {
    // ---- the loss scalars and the log-std slot (flat index 0), one wave
    if (threadIdx.x >= 64) return;
    double first = 0.0, second = 0.0;
    for (int b = threadIdx.x; b < n_part; b += 64) {
      first += m.lpart[2 * b + 0];
      second += m.lpart[2 * b + 1];
    }
    first = ga_wave_sum(first);
    second = ga_wave_sum(second);
    if (threadIdx.x != 0) return;
    const LossRowArgs L = members_loss(m, p.sh, p.k, M);
    float loss, dls;
    lr_finish(L, first, second, M, &loss, &dls);
    if (m.losses) m.losses[p.k] = loss;
    const float g = p.sh.zero_slot0 ? 0.f : dls;
    m.grads[0] = g;
    float pp = m.params[0], mm = m.exp_avg[0], vv = m.exp_avg_sq[0];
    ga_adam_update(adam, g, pp, mm, vv);
    m.params[0] = pp; m.exp_avg[0] = mm; m.exp_avg_sq[0] = vv;
    return;
  }
  __shared__ float4 wsum[4][64];
  const int Q = n_part <= 128 ? 64 : 16;
  const int qi = Q == 64 ? 0 : 1;
  const int b = blockIdx.x;
  if (b >= p.n_virtual[qi]) return;
  int ri = 0;
#pragma unroll 1
  for (int k = 1; k < MB_REGIONS; ++k)
    if (b >= p.r[k].vbeg[qi]) ri = k;
  const MembersRegion& R = p.r[ri];
  const float* src = m.part + R.src_off;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float g[4];
  const int lwc = 64 / Q;
  const int q = lane % Q, lw = lane / Q;
  const int way = lwc * wv + lw;
  const int64_t e4 = (int64_t)(b - R.vbeg[qi]) * Q + q;  // this lane's quad
  const bool on = 4 * e4 < R.n;
  const int shares = 4 * lwc;
  const int chunk = (n_part + shares - 1) / shares;
  const int p0 = way * chunk, p1 = min(n_part, p0 + chunk);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) acc = ft_share_run(src + 4 * e4, p.sh.stride, p0, p1);
  g[0] = acc.x; g[1] = acc.y; g[2] = acc.z; g[3] = acc.w;
  ft_lane_shares_meet(g, Q);
  if (lw == 0) wsum[wv][q] = make_float4(g[0], g[1], g[2], g[3]);
  __syncthreads();
  if ((int)threadIdx.x >= Q || !on) return;
  ft_wave_shares_meet(g, wsum[0][q], wsum[1][q], wsum[2][q], wsum[3][q]);
  const int64_t i = R.beg + 4 * e4;
  *reinterpret_cast<float4*>(m.grads + i) = make_float4(g[0], g[1], g[2], g[3]);
  float4 p4 = *reinterpret_cast<float4*>(m.params + i);
  float4 m4 = *reinterpret_cast<float4*>(m.exp_avg + i);
  float4 v4 = *reinterpret_cast<float4*>(m.exp_avg_sq + i);
  float pp[4] = {p4.x, p4.y, p4.z, p4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w},
        vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) ga_adam_update(adam, g[j], pp[j], mm[j], vv[j]);
  *reinterpret_cast<float4*>(m.params + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
  *reinterpret_cast<float4*>(m.exp_avg + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
  *reinterpret_cast<float4*>(m.exp_avg_sq + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

}  // namespace

extern "C" int ga_members_train_step(const GaMembersShared* sh,
                                     const GaMemberDev* table_dev, int64_t k,
                                     int64_t max_tiles, hipStream_t stream) {
  GA_REQUIRE(sh && table_dev, "ga_members_train_step: null pointer");
  const int dims[4] = {sh->in_w, sh->H, sh->H, sh->out_w};
  GA_REQUIRE(ga_narrow_step_supported(3, dims) && sh->n_members >= 1 &&
                 sh->n_members <= 65535 && max_tiles >= 1 && max_tiles < (1ll << 25) &&
                 k >= 0 && k < (1ll << 31),
             "ga_members_train_step: unsupported shape");
  MembersTrainParams q;
  memset(&q, 0, sizeof(q));
  q.sh = *sh; q.table = table_dev; q.k = (int)k;
  const dim3 grid((unsigned)max_tiles, (unsigned)sh->n_members);
  ga_prof_count(GA_PROF_MEMBERS_STEP);
#define GA_MEMBERS_LAUNCH(HH, LL)                                                       \
  hipLaunchKernelGGL((narrow_train_members_kernel<HH, LL>), grid, dim3(NS_THREADS), 0, \
                     stream, q)
  const int in_w = sh->in_w;
  const int ldx_s = in_w <= 8 ? 12 : (in_w <= 16 ? 20 : 36);
  if (sh->H == 64) {
    if (ldx_s == 12) GA_MEMBERS_LAUNCH(64, 12);
    else if (ldx_s == 20) GA_MEMBERS_LAUNCH(64, 20);
    else GA_MEMBERS_LAUNCH(64, 36);
  } else {
    if (ldx_s == 12) GA_MEMBERS_LAUNCH(32, 12);
    else if (ldx_s == 20) GA_MEMBERS_LAUNCH(32, 20);
    else GA_MEMBERS_LAUNCH(32, 36);
  }
#undef GA_MEMBERS_LAUNCH
  GA_CHECK_LAUNCH("narrow_train_members");
  return GA_OK;
}

extern "C" int ga_members_reduce_adam(const GaMembersShared* sh,
                                      const GaMemberDev* table_dev, const GaAdam* adam_dev,
                                      int64_t k, int64_t max_tiles, hipStream_t stream) {
  GA_REQUIRE(sh && table_dev && adam_dev, "ga_members_reduce_adam: null pointer");
  const int dims[4] = {sh->in_w, sh->H, sh->H, sh->out_w};
  GA_REQUIRE(ga_narrow_step_supported(3, dims) && sh->n_members >= 1 &&
                 sh->n_members <= 65535 && max_tiles >= 1 && k >= 0 && k < (1ll << 31),
             "ga_members_reduce_adam: unsupported shape");
  MembersReduceParams p;
  memset(&p, 0, sizeof(p));
  p.sh = *sh; p.table = table_dev; p.adam = adam_dev; p.k = (int)k;
  // the regions of update.cpp's fused_step for a narrow network
  int64_t src = 0;
  int v[2] = {0, 0};
  for (int l = 0; l < 3; ++l) {
    const int64_t wn = (int64_t)dims[l + 1] * ((dims[l] + 3) & ~3);
    const int64_t bsrc = src + (l == 2 ? 8 * (int64_t)sh->H : wn);
    const int64_t beg[2] = {sh->w_off[l], sh->b_off[l]};
    const int64_t n[2] = {wn, dims[l + 1]};
    const int64_t off[2] = {src, bsrc};
    for (int i = 0; i < 2; ++i) {
      GA_REQUIRE(beg[i] >= 4 && beg[i] % 4 == 0, "ga_members_reduce_adam: bad region");
      MembersRegion& r = p.r[2 * l + i];
      r.beg = beg[i]; r.n = (n[i] + 3) & ~(int64_t)3; r.src_off = off[i];
      r.vbeg[0] = v[0]; r.vbeg[1] = v[1];
      v[0] += (int)ga_ceil_div(r.n / 4, 64);
      v[1] += (int)ga_ceil_div(r.n / 4, 16);
    }
    src = bsrc + dims[l + 1];
  }
  p.n_virtual[0] = v[0]; p.n_virtual[1] = v[1];
  // (+ the loss workgroup)
  const dim3 grid((unsigned)v[max_tiles <= 128 ? 0 : 1] + 1, (unsigned)sh->n_members);
  hipLaunchKernelGGL(reduce_members_adam_kernel, grid, dim3(256), 0, stream, p);
  GA_CHECK_LAUNCH("reduce_members_adam");
  return GA_OK;
}
