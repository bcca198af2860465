// Which kernel a layer product takes, stated ONCE: one plan per product of the per-layer
// MLP passes (mlp_layers.cpp), and the launch seam below it (gemm.hip, skinny.hip).  A
// plan function is pure -- it reads no global and no environment and calls nothing of the
// HIP runtime; the developer switches come in as arguments -- and answers everything the
// host decides about a launch: taken or not, the instantiation, the grid, the LDS bytes,
// the profiling figure.  The seam instantiates and launches what the plan says, nothing
// else.  Host C++ only (no device code): tests/host/mlp_layers_harness.cpp pins every
// boundary of these rules on the CPU.  Not part of the C ABI.
#pragma once
#include "common.h"
#include "gemm_params.h"
#include "prof.h"
#include "shape_rules.h"

// ---------------------------------------------------------------------------
// gemm.hip: the fp32 MFMA tile kernels
// ---------------------------------------------------------------------------
struct GemmSwitches {
  bool small_m;      // ga_set_small_m_gemm
  bool split_gemm;   // ga_split_bf16_gemm(): split-operand forward / data-gradient GEMM
  bool split_wgrad;  // ga_split_bf16_enabled(): split-operand weight-gradient GEMM
  bool wgrad_paired; // ga_set_wgrad_paired_columns: the paired-column weight-gradient GEMM
};

// One value per arm of the chain in ga_gemm_plan, in its precedence.
enum GemmTile {
  GT_SMALL_M = 0,   // gemm_f32_kernel<64, 64, 2, 2, ., ., 128>: 64 x 64 tiles, 128-deep k
  GT_128x32 = 1,    // gemm_f32_kernel<128, 32, 4, 1>
  GT_64x64 = 2,     // gemm_f32_kernel<64, 64, 2, 2>
  GT_KC_SPLIT = 3,  // gemm_kc_split_kernel: 128 x 128, weights as bf16 planes
  GT_NT_SPLIT = 4,  // gemm_nt_split_kernel: 128 x 128, both operands split in LDS
  GT_128x128 = 5,   // gemm_f32_kernel<128, 128, 2, 4>
};
struct GemmTileShape {
  int bm, bn, threads;
};
constexpr GemmTileShape ga_gemm_tile_shape(GemmTile t) {
  return t == GT_SMALL_M || t == GT_64x64 ? GemmTileShape{64, 64, 256}
         : t == GT_128x32                 ? GemmTileShape{128, 32, 256}
                                          : GemmTileShape{128, 128, 512};
}

struct GemmPlan {
  GemmTile tile;
  int a_kc, b_kc;      // the operand is k-contiguous in memory: (1, 1) forward, (1, 0)
                       // data gradient, (0, 0) weight gradient
  int gx, gy, gz;      // logical grid (m blocks, n blocks, splits); launched 1-D
  int k_per_split;
  int threads;         // per workgroup
  int prof_kind;       // GaProfKind
  double work;         // algorithmic flops: 2 M N K (the padding of ragged tiles is not counted)
  bool planes;         // GT_KC_SPLIT: the weight planes of B (ga_weight_planes) are wanted,
  int planes_bwd;      // in the data gradient's orientation (B(k, n) = W[k][n]) or the
  int64_t bplane_stride;  // forward's (B(k, n) = W[n][k]), with this GemmParams geometry
  int bplane_nblk;
  bool paired_cols;    // GT_128x128: gemm_rr_paired_kernel (same tiles, grid, k ranges and
                       // bits as gemm_f32_kernel<128, 128, 2, 4, false, false>)
};

// The product is one gemm_rr_paired_kernel (gemm.hip) takes: both operands row-major with k
// as the row index, no gather, every tile interior, the plain epilogue into a row-major C
// whose lane pairs (n, n + 1) are 8-B aligned, and every byte offset of a slab's operand
// rows and of a C tile's rows in 32 bits (the kernel addresses them through buffer
// descriptors, as the fused step does: fused_train_host.cpp, ft_ld_ok).  A product that
// is refused here takes gemm_f32_kernel and raises no error.
inline bool ga_gemm_paired_ok(const GemmParams& p, int a_kc, int b_kc) {
  const auto ld_ok = [](int64_t ld, int64_t rows) {
    return ld >= 128 && ld < (1ll << 22) && rows * ld * 4 < (1ll << 31);
  };
  return !a_kc && !b_kc && !p.a_idx && !p.b_idx && p.epi == EPI_PLAIN && !p.accum && !p.H &&
         !p.bias && !p.head_W && p.M >= 128 && p.N >= 128 && p.M % 128 == 0 &&
         p.N % 128 == 0 && p.K >= 1 && p.k_per_split >= BK && p.k_per_split % BK == 0 &&
         p.c_cs == 1 && p.c_rs % 2 == 0 && p.c_split_stride % 2 == 0 &&
         (reinterpret_cast<uintptr_t>(p.C) & 7u) == 0 && p.lda % 4 == 0 && p.ldb % 4 == 0 &&
         ga_aligned16(p.A) && ga_aligned16(p.B) && ld_ok(p.lda, p.k_per_split) &&
         ld_ok(p.ldb, p.k_per_split) && ld_ok(p.c_rs, 128);
}

// C(m, n) = epi(sum_k A(m, k) B(k, n)) over `splits` slabs of k.
inline GemmPlan ga_gemm_plan(const GemmParams& p, int a_kc, int b_kc, int splits,
                             const GemmSwitches& sw) {
  GemmPlan g = {};
  g.a_kc = a_kc; g.b_kc = b_kc;
  g.k_per_split = p.k_per_split;
  if (sw.small_m && splits == 1 && p.K > 64 &&
      (p.N > 32 ? ga_ceil_div(p.M, 128) * ga_ceil_div(p.N, 128) <= 128 : p.M <= 4096)) {
    // fewer 128x128 tiles than half the CUs: the k-loop of one workgroup is then a
    // chain of dependent memory round trips (the weights were rewritten by the
    // optimizer step just before, so they come from beyond this XCD's L2) with
    // nothing else on the CU to hide them.  64x64 tiles spread rows and columns
    // over 4x the workgroups and a 128-deep k-step cuts the chain to K / 128 round
    // trips with 16 16-B loads in flight per thread.  Same k order per output
    // element as every other tile shape, so the results are bit-identical.
    // MLP(256,256) forward + backward at 64 rows: 43.6 + 54.3 -> 26.5 + 33.3 us,
    // at 4096 rows 43.5 + 81.2 -> 31.3 + 66.8 us; MLP(512,512,512) at 64 rows
    // 149.5 + 141.9 -> 61.7 + 69.5 us (tools/small_m_ab.py).  Narrow outputs (the
    // head layer) take the same kernel up to 4096 rows: a half-empty tile costs
    // nothing when the launch is one round-trip chain anyway.
    g.tile = GT_SMALL_M;
    g.k_per_split = (int)ga_ceil_div(p.K, 128) * 128;
  } else if (p.N <= 32) {
    // narrow outputs are HBM bound on the wide operand: 128-row tiles give
    // M/128 workgroups (256 at the C3 minibatch) to pull it through
    // (a 128-deep k tile -- 80 KB in flight per workgroup -- was tried for these
    // latency-bound shapes and measured no better than 32: one workgroup per CU)
    g.tile = GT_128x32;
  } else if (p.N <= 64) {
    // 33..64 wide outputs (the 64-unit layers of the CartPole-shaped config): a
    // 128x128 tile would be half empty and give M/128 workgroups; 64x64 tiles
    // (4 waves, one 32x32 accumulator each) give 4x as many
    g.tile = GT_64x64;
  } else if (a_kc && sw.split_gemm && splits == 1 && p.N >= 128 && p.K >= 128 &&
             p.K % 4 == 0 && p.M >= 1024 && !p.b_idx && !p.accum && !p.colsum &&
             !p.head_W && p.c_cs == 1) {
    // wide layers: forward (B(k, n) = W[n][k]) and data gradient (B(k, n) = W[k][n]);
    // b_kc tells which orientation the weight planes are needed in
    g.tile = GT_KC_SPLIT;
    g.k_per_split = (int)ga_ceil_div(p.K, BK) * BK;
    g.planes = true;
    g.planes_bwd = b_kc ? 0 : 1;
    const int np = (p.N + 31) & ~31, kp = (p.K + 31) & ~31;
    g.bplane_stride = (int64_t)np * kp;
    g.bplane_nblk = np / 32;
  } else if (!a_kc && !b_kc && sw.split_wgrad && p.M % 128 == 0 && p.N % 128 == 0 &&
             !p.a_idx && !p.b_idx && p.epi == EPI_PLAIN && !p.accum &&
             p.k_per_split % 16 == 0 && !p.colsum_of_b) {
    // interior shapes only: the kernel masks nothing
    g.tile = GT_NT_SPLIT;
  } else {
    // 8 waves (64x32 each): two workgroups per CU put 4 waves on every SIMD, so
    // the matrix pipe has work while other waves sit at the barrier / vmcnt
    g.tile = GT_128x128;
    g.paired_cols = sw.wgrad_paired && ga_gemm_paired_ok(p, a_kc, b_kc);
  }
  const GemmTileShape t = ga_gemm_tile_shape(g.tile);
  // (the two arms that take the whole of K ask for splits == 1)
  g.gx = (int)ga_ceil_div(p.M, t.bm); g.gy = (int)ga_ceil_div(p.N, t.bn); g.gz = splits;
  g.threads = t.threads;
  const int mode = (a_kc && b_kc) ? 0 : (a_kc ? 1 : 2);
  g.prof_kind = (g.tile == GT_128x32 ? GA_PROF_GEMM_NT_256 : GA_PROF_GEMM_NT_128) + mode;
  g.work = 2.0 * (double)p.M * (double)p.N * (double)p.K;
  return g;
}
// what of a GemmParams is the plan's to fill in (bplanes: the caller's, when g.planes)
inline void ga_gemm_apply(const GemmPlan& g, GemmParams* p) {
  p->gx = g.gx; p->gy = g.gy; p->gz = g.gz;
  p->k_per_split = g.k_per_split;
  if (g.planes) { p->bplane_stride = g.bplane_stride; p->bplane_nblk = g.bplane_nblk; }
}

// The last hidden layer and the head layer (p.head_*) in one launch: tiles of 64 rows
// that span the layer's whole width -- 64, 128 or 256 units, one instantiation each.
// Every workgroup must be on the staged-epilogue path, which the kernel decides from
// the same conditions.
struct GemmHeadPlan {
  bool taken;
  int width;    // 64, 128, 256: the instantiation
  int gx;       // workgroups = 64-row tiles
  int threads;
  double work;  // algorithmic flops of both layers
};
inline GemmHeadPlan ga_gemm_head_plan(const GemmParams& p) {
  GemmHeadPlan h = {};
  const int bm = 64;
  if (!(p.N == 64 || p.N == 128 || p.N == 256) || p.M % bm != 0 || p.M < bm ||
      !p.head_W || p.head_n < 1 || p.head_n > 8 || p.head_ld < p.head_n ||
      p.head_ldw % 4 != 0 || !ga_aligned16(p.head_W) || p.c_cs != 1 || (p.c_rs & 3) != 0 ||
      !ga_aligned16(p.C) || (p.bias && !ga_aligned16(p.bias)) || p.H || p.accum ||
      p.colsum || p.epi != EPI_BIAS_ACT || p.K < 1)
    return h;
  h.taken = true;
  h.width = p.N;
  h.gx = p.M / bm;
  h.threads = p.N == 256 ? 512 : 256;
  h.work = 2.0 * (double)p.M * (double)p.N * ((double)p.K + p.head_n);
  return h;
}
inline void ga_gemm_head_apply(const GemmHeadPlan& h, GemmParams* p) {
  p->gx = h.gx; p->gy = 1; p->gz = 1;
}

// Two weight-gradient products of the same shape (128 x 128 tiles, gz = the caller's k
// splits) in one grid of 2 gx gy gz workgroups.
struct GemmPairPlan {
  bool taken;
  int gx, gy, gz;
  double work;
};
inline GemmPairPlan ga_gemm_pair_plan(const GemmParams& a, const GemmParams& b) {
  GemmPairPlan g = {};
  g.taken = a.M == b.M && a.N == b.N && a.K == b.K && a.gz == b.gz && a.gz >= 1;
  g.gx = (int)ga_ceil_div(a.M, 128); g.gy = (int)ga_ceil_div(a.N, 128); g.gz = a.gz;
  g.work = 2.0 * 2.0 * (double)a.M * (double)a.N * (double)a.K;
  return g;
}

// ---------------------------------------------------------------------------
// skinny.hip: the streaming kernels for products with one dimension <= 32
// ---------------------------------------------------------------------------
// Y[m, n] = epi(sum_k X[row(m), k] * W(n, k)),  K <= 32, N = 4 * qpr * n_colblk
struct SkinnyFwdParams {
  const float* X;        // [rows][ldx], K valid floats per row (ldx % 4 == 0)
  int64_t ldx;
  const int32_t* idx;    // optional row gather
  const float* W;        // w_kc: W[n][ldw] (k contiguous) else W[k][ldw]
  int64_t ldw;
  const float* bias;     // epi 0: per-n bias (may be null)
  const float* H;        // epi 1: tanh outputs H[m][ldh]
  int64_t ldh;
  float* Y;
  int64_t ldy;
  int M, N, K;
  int act;               // epi 0: 1 = tanh
  int qpr;               // column quads per row handled by one workgroup (<= 64)
  int rows_per_thread;   // multiple of SK_UNROLL
};

// The two layer products that are instantiated, each from its GemmParams:
//   w_kc      Y = act(X W^T + b), W[n][ldw] k-contiguous, tanh or the identity   epi 0
//   otherwise Y = (X W) * (1 - H^2), W[k][ldw] n-contiguous, a tanh layer below  epi 1
struct SkinnyFwdPlan {
  bool taken;
  bool w_kc;
  int epi;
  int KV;               // round4(K) / 4: the instantiation
  int qpr, rows_per_thread;
  unsigned gx, gy;      // row blocks, column blocks
  unsigned lds_bytes;   // the workgroup's staged X rows
  double work;          // algorithmic bytes: the [M x N] output (+ H) + X
};
// rows_wg: rows per workgroup.  32 (never fewer than one unroll per thread): two
// generations of workgroups per CU, so one's prologue (gathered X rows, 20 KB of W quads
// from L2) runs under the other's stores.  Round 1 preferred 128 rows while the other
// update chain's streaming kernels shared the chip (146.2 / 143.3 / 152.9 ms per C3
// iteration at 32 / 128 / 256); with those kernels folded into the GEMMs it is 131.5 /
// 133.0 / 132.7 ms at 32 / 64 / 128 (18.5 / 18.9 / 20.2 us a launch).  Packed FMAs
// changed nothing: the kernel is bound by its store stream.
inline SkinnyFwdPlan ga_skinny_fwd_plan(const GemmParams& g, bool w_kc, bool enabled,
                                        int rows_wg = 32) {
  SkinnyFwdPlan s = {};
  s.w_kc = w_kc;
  s.epi = w_kc ? 0 : 1;
  const int qpr = ga_skinny_fwd_qpr(g.N);
  if (!enabled || g.K < 1 || g.K > SK_KMAX || g.N <= 32 || qpr == 0) return s;
  // (the streaming kernels know tanh and the identity, and tanh's slope)
  if (w_kc ? (g.epi != EPI_BIAS_ACT || g.H || g.act > 1)
           : (g.epi != EPI_MUL_DTANH || !g.H || g.hact != 0))
    return s;
  if (g.b_idx || g.accum || g.colsum || g.c_cs != 1) return s;
  if (g.lda % 4 != 0 || g.ldb % 4 != 0 || g.c_rs % 4 != 0 || (g.H && g.ldh % 4 != 0) ||
      !ga_aligned16(g.A) || !ga_aligned16(g.B) || !ga_aligned16(g.C) ||
      (g.bias && !ga_aligned16(g.bias)) || (g.H && !ga_aligned16(g.H)) ||
      g.lda < ((g.K + 3) & ~3))
    return s;
  s.KV = (g.K + 3) / 4;
  s.qpr = qpr;
  const int n_rg = SK_THREADS / qpr;
  // (... but at least one workgroup per CU)
  while (rows_wg > 32 && (int64_t)g.M < 256 * (int64_t)rows_wg) rows_wg >>= 1;
  s.rows_per_thread = ((rows_wg / n_rg + SK_UNROLL - 1) / SK_UNROLL) * SK_UNROLL;
  if (s.rows_per_thread < SK_UNROLL) s.rows_per_thread = SK_UNROLL;
  const int rows_per_block = n_rg * s.rows_per_thread;
  if ((int64_t)rows_per_block * s.KV * 16 > SK_LDS_CAP) return s;
  s.lds_bytes = (unsigned)(rows_per_block * s.KV * 16);
  s.gx = (unsigned)ga_ceil_div(g.M, rows_per_block);
  s.gy = (unsigned)ga_ceil_div(g.N, 4 * qpr);
  s.work = 4.0 * g.M * ((double)g.N * (g.H ? 2 : 1) + g.K);
  s.taken = true;
  return s;
}
inline SkinnyFwdParams ga_skinny_fwd_params(const GemmParams& g, const SkinnyFwdPlan& s) {
  SkinnyFwdParams p = {};
  p.X = g.A; p.ldx = g.lda; p.idx = g.a_idx;
  p.W = g.B; p.ldw = g.ldb;
  p.bias = s.w_kc ? g.bias : nullptr;
  p.H = g.H; p.ldh = g.ldh;
  p.Y = g.C; p.ldy = g.c_rs;
  p.M = g.M; p.N = g.N; p.K = g.K;
  p.act = s.w_kc ? g.act : 0;
  p.qpr = s.qpr; p.rows_per_thread = s.rows_per_thread;
  return p;
}

// C(wide c, narrow j) = sum_r Wd[row_w(r), c] * Nr[row_n(r), j] per split of rows
struct SkinnyWgradParams {
  const float* Wd;       // wide operand  [rows][ldw]
  int64_t ldw;
  const int32_t* w_idx;
  const float* Nr;       // narrow operand [rows][ldn], NS valid floats
  int64_t ldn;
  const int32_t* n_idx;
  int rows, wide, NS;
  int rows_per_split;
  int qpr;               // wide column quads per workgroup (<= 64)
  int n_colblk, n_splits;  // logical grid; launched 1-D in XCD-aware order
  float* C;
  int64_t c_wide_stride, c_narrow_stride;  // C(c, j) at c * cws + j * cns
  int64_t split_stride;
  float* colsum_wide;    // optional: sum_r Wd[., c]  -> [split][c]
  float* colsum_narrow;  // optional: sum_r Nr[., j]  -> [split][j]
  // DZ instantiation (head weight gradient + the data gradient of the layer below
  // in one pass over H): dz_out[r, c] = (sum_j Nr[r, j] * Wn[j, c]) * (1 - Wd[r, c]^2)
  const float* Wn;       // [NS][ldwn] head weights, wide-contiguous
  int64_t ldwn;
  float* dz_out;         // [rows][lddz]
  int64_t lddz;
};

enum SkinnyWgradVariant {
  SWV_PLAIN = 0,  // skinny_wgrad_kernel<NV, false>
  SWV_NSUM = 1,   // <NV, true>: also the column sums of the narrow operand
  SWV_DZ = 2,     // <NV, true, true>: also the data gradient of the layer below, NV <= 4
};
struct SkinnyWgradPlan {
  bool taken;
  SkinnyWgradVariant variant;
  int NV;          // round4(NS) / 4: the instantiation
  int qpr, n_colblk;
  unsigned grid;   // n_colblk * n_splits workgroups
  double work;     // algorithmic bytes: both operands once (+ the data gradient written once)
};
// Everything of `p` but qpr and n_colblk is the caller's.  p.dz_out set asks for the data
// gradient in the same pass: a shape that takes no data gradient is NOT taken (the caller
// asks again without).
inline SkinnyWgradPlan ga_skinny_wgrad_plan(const SkinnyWgradParams& p, bool enabled) {
  SkinnyWgradPlan s = {};
  const int qpr = ga_skinny_wgrad_qpr(p.wide);
  if (!enabled || p.wide <= 32 || p.NS < 1 || p.NS > SW_NS_MAX || qpr == 0 ||
      p.n_splits < 1 || p.ldw % 4 != 0 || p.ldn % 4 != 0 || p.ldn < ((p.NS + 3) & ~3) ||
      !ga_aligned16(p.Wd) || !ga_aligned16(p.Nr) || p.split_stride % 4 != 0 ||
      (p.c_wide_stride == 1 && (p.c_narrow_stride % 4 != 0 || !ga_aligned16(p.C))) ||
      (p.colsum_wide && !ga_aligned16(p.colsum_wide)))
    return s;
  const bool dz = p.dz_out != nullptr;
  if (dz && (p.w_idx || !p.Wn || p.ldwn % 4 != 0 || p.lddz % 4 != 0 || !ga_aligned16(p.Wn) ||
             !ga_aligned16(p.dz_out) || p.NS > SW_NS_MAX_DZ || p.colsum_narrow == nullptr))
    return s;
  s.variant = dz ? SWV_DZ : (p.colsum_narrow ? SWV_NSUM : SWV_PLAIN);
  s.NV = (p.NS + 3) / 4;
  s.qpr = qpr;
  s.n_colblk = (int)ga_ceil_div(p.wide, 4 * qpr);
  s.grid = (unsigned)(s.n_colblk * p.n_splits);
  s.work = 4.0 * p.rows * ((double)p.wide * (dz ? 2 : 1) + p.NS);
  s.taken = true;
  return s;
}

// ---------------------------------------------------------------------------
// The launch seam: one entry per kernel family.  Each takes a plan that says `taken`
// (where the plan has the word) and the finished parameter struct, switches on the plan
// to the instantiation, launches on `stream` and checks the launch.
// ---------------------------------------------------------------------------
int ga_gemm_launch(const GemmPlan& plan, const GemmParams& p, hipStream_t stream);
int ga_gemm_head_launch(const GemmHeadPlan& plan, const GemmParams& p, hipStream_t stream);
int ga_gemm_pair_launch(const GemmPairPlan& plan, const GemmParams& a, const GemmParams& b,
                        hipStream_t stream);
int ga_skinny_fwd_launch(const SkinnyFwdPlan& plan, const SkinnyFwdParams& p,
                         hipStream_t stream);
int ga_skinny_wgrad_launch(const SkinnyWgradPlan& plan, const SkinnyWgradParams& p,
                           hipStream_t stream);
