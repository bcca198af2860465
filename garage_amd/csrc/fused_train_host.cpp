// The host side of the fused optimizer-step kernels (fused_train.hip): the switches,
// the argument checks and kernel parameters of every launch (fwd_build, dgrad_build,
// reduce_add_net), the choice of the instantiation (ft_variant), the grids, the slab
// sum's 32-bit offsets, the optimizer launch's virtual grid, the weight-plane cache of
// the split-operand mode and the developer hooks' buffers.  Host C++ only: the kernels
// are behind the launch seam of fused_params.h, so this file builds for the CPU too and
// runs there against fakes of the seam under AddressSanitizer
// (tests/host/fused_host_harness.cpp) -- a mistake here becomes an out-of-range device
// access.
#include "common.h"
#include <stdlib.h>
#include <mutex>
#include <vector>

#include "prof.h"

#include "fused_params.h"
#include "fused_train.h"

// ---- switches ---------------------------------------------------------------------------
// The pipelined k-loop is compiled for first layers of 17 .. 20 inputs (KSC = 5: the
// HalfCheetah-shaped configuration the headline metric is quoted on) at 256 units;
// every other shape takes the plain loop.  0 (or GARAGE_AMD_PIPELINED_KLOOP=0 in the
// environment): the plain loop everywhere (A/B runs, tests).
static int g_pipelined_kloop = -1;
static bool pipelined_kloop_on() {
  if (g_pipelined_kloop < 0) {
    const char* e = getenv("GARAGE_AMD_PIPELINED_KLOOP");
    g_pipelined_kloop = (e && e[0] == '0') ? 0 : 1;
  }
  return g_pipelined_kloop != 0;
}

// 1: the update kernels that have a split-operand instantiation use it (opt-in;
// GARAGE_AMD_SPLIT_BF16=1 in the environment or ga_set_split_bf16(1)); default 0:
// exact fp32 everywhere.
static int g_split_bf16 = -1;
static int g_split_parts = -1;  // developer knob: which kernels (1 forward, 2 data gradient,
                                // 4 weight gradient, 8 evaluation forward, 16 the per-layer forward / data-gradient
                                // GEMMs of wide layers); default all
static bool split_bf16_on(int part = 0) {
  if (g_split_bf16 < 0) {
    const char* e = getenv("GARAGE_AMD_SPLIT_BF16");
    g_split_bf16 = (e && e[0] == '1') ? 1 : 0;
  }
  if (g_split_parts < 0) {
    const char* e = getenv("GARAGE_AMD_SPLIT_PARTS");
    g_split_parts = e ? atoi(e) : 31;
  }
  return g_split_bf16 != 0 && (part == 0 || (g_split_parts & part) != 0);
}

extern "C" int ga_set_pipelined_kloop(int on) {
  g_pipelined_kloop = on != 0;
  return 0;
}

extern "C" int ga_set_split_bf16(int on) {
  g_split_bf16 = on != 0;
  return 0;
}

extern "C" int ga_split_bf16_enabled(void) { return split_bf16_on(4) ? 1 : 0; }
extern "C" int ga_split_bf16_gemm(void) { return split_bf16_on(16) ? 1 : 0; }
extern "C" int ga_split_bf16_any(void) { return split_bf16_on() ? 1 : 0; }

// ---- which instantiation a launch runs (FtVariant, fused_params.h), written once ------
// The split-operand loops exist at 256 units for one network: forward + loss and the
// evaluation forward with the first layer in the kernel and at most 20 inputs (five
// groups of four), the data gradient for any input width; each behind its own bit of
// GARAGE_AMD_SPLIT_PARTS.  The pipelined loop: 256 units, first layer in the kernel
// with 17 .. 20 inputs, every family that runs the forward body.
enum FtFamily { FT_FWD_LOSS, FT_EVAL_FWD, FT_DGRAD, FT_FWD_DGRAD };
static FtVariant ft_variant(FtFamily family, int width, bool first, int in_w, int K,
                            int n_nets) {
  FtVariant v = {width, first ? 1 : 0, 0, 0};
  if (width != 256) return v;
  const int part =
      family == FT_FWD_LOSS ? 1 : (family == FT_DGRAD ? 2 : (family == FT_EVAL_FWD ? 8 : 0));
  const bool forward = family != FT_DGRAD;
  if (part && n_nets == 1 && (!forward || first) && split_bf16_on(part) && K % 32 == 0 &&
      (!forward || in_w <= 20))
    v.split = 1;
  else if (forward && first && (in_w + 3) / 4 == 5 && pipelined_kloop_on())
    v.ksc = 5;
  return v;
}

// ---- the weight planes of the split-operand mode -----------------------------------------
// Device buffers for the planes of a weight matrix, one per (matrix, orientation),
// kept for the life of the process (a few 100 KB each); the planes are recomputed by
// every launch that uses them (the weights change every optimizer step).
struct PlaneBuf {
  const float* W;
  int rows, cols;       // W [rows][ld], cols valid
  uint16_t* fwd;        // B(k = col, n = row): the forward kernel's operand
  uint16_t* bwd;        // B(k = row, n = col): the data-gradient kernel's operand
  hipStream_t bwd_stream;  // stream on which `bwd` was last refreshed, not yet consumed
  bool bwd_fresh;
  // both operands were rewritten by the optimizer launch (reduce_regions_adam_kernel)
  // that last changed W, on this stream, inside the epoch call that is still running
  hipStream_t adam_stream;
  bool adam_fresh;
};
static std::mutex g_plane_mu;
static std::vector<PlaneBuf> g_plane_bufs;
// Both operands' planes of W [rows][ld] are written by ONE launch when the forward
// kernel asks (want_bwd = false); the data-gradient launch of the same step -- same
// stream, weights unchanged in between -- then finds its planes fresh and launches
// nothing.  Any other order (a data-gradient launch on its own) recomputes.
// (the modes: fused_params.h)
static const uint16_t* planes_for(const float* W, int64_t ld, int rows, int cols, int mode,
                                  hipStream_t stream) {
  uint16_t *fwd = nullptr, *bwd = nullptr;
  bool reuse = false;
  {
    std::lock_guard<std::mutex> lock(g_plane_mu);
    PlaneBuf* pb = nullptr;
    for (PlaneBuf& b : g_plane_bufs)
      if (b.W == W && b.rows == rows && b.cols == cols) pb = &b;
    if (!pb) {
      uint16_t* buf = nullptr;
      const size_t padded = (size_t)((rows + 31) & ~31) * ((cols + 31) & ~31);
      if (hipMalloc(&buf, 6 * padded * sizeof(uint16_t)) != hipSuccess) return nullptr;
      g_plane_bufs.push_back(PlaneBuf{W, rows, cols, buf, buf + 3 * padded, nullptr, false});
      pb = &g_plane_bufs.back();
    }
    bool from_adam = false;
    if (mode == PLANES_BWD || mode == PLANES_BWD_ALWAYS) {
      reuse = mode == PLANES_BWD && pb->bwd_fresh && pb->bwd_stream == stream;
      pb->bwd_fresh = false;
    } else if (mode == PLANES_TRAIN_FWD) {
      // (the previous step's optimizer launch wrote both operands already)
      from_adam = pb->adam_fresh && pb->adam_stream == stream;
      pb->bwd_fresh = true;
      pb->bwd_stream = stream;
    } else {
      pb->bwd_fresh = false;
    }
    pb->adam_fresh = false;
    fwd = pb->fwd;
    bwd = pb->bwd;
    if (from_adam) return fwd;
  }
  const unsigned blocks = (unsigned)(
      ((int64_t)((rows + 31) & ~31) * ((cols + 31) & ~31) / 2 + 255) / 256);
  uint32_t* fwd32 = reinterpret_cast<uint32_t*>(fwd);
  uint32_t* bwd32 = reinterpret_cast<uint32_t*>(bwd);
  if (mode == PLANES_BWD || mode == PLANES_BWD_ALWAYS) {
    if (!reuse) ft_launch_split_planes(true, blocks, W, ld, rows, cols, fwd32, bwd32, stream);
    return bwd;
  }
  ft_launch_split_planes(false, mode == PLANES_TRAIN_FWD ? 2 * blocks : blocks, W, ld, rows,
                         cols, fwd32, bwd32, stream);
  return fwd;
}

extern "C" const uint16_t* ga_weight_planes(const float* W, int64_t ld, int rows, int cols,
                                            int bwd, hipStream_t stream) {
  return planes_for(W, ld, rows, cols, bwd ? PLANES_BWD_ALWAYS : PLANES_EVAL_FWD, stream);
}

// developer hook (tools/): a register-only MFMA loop on `stream` (mfma_burn_kernel)
extern "C" int ga_debug_mfma_burn(int mode, int iters, int blocks, float* sink,
                                  ga_stream_t stream_) {
  ft_launch_mfma_burn(mode, iters, blocks, sink, (hipStream_t)stream_);
  return 0;
}

// ---- developer hooks: phase timestamps of the forward and the data-gradient kernels ------
// One device buffer per kernel family: 16 stamps of workgroup 8, then (start, end of
// k-loop, end) of every workgroup, then four tick sums per workgroup.  The first call
// of an arming hook allocates and zeroes it (launches record from then on); later calls
// wait for the device and read.
static long long* g_ft_dbg = nullptr;
static long long* g_dg_dbg = nullptr;
constexpr int FT_DBG_BLOCKS = 4096, FT_DBG_WORDS = 16 + 7 * FT_DBG_BLOCKS;
// 1: this call armed *buf (arm only); -1: not armed, or no memory; otherwise the device
// is idle and `words` values from word `at` are in host_out (0), or the copy failed (-1)
static int ft_dbg_read(long long** buf, bool arm, long long* host_out, size_t at,
                       size_t words) {
  if (!*buf) {
    if (!arm) return -1;
    if (hipMalloc(buf, FT_DBG_WORDS * sizeof(long long)) != hipSuccess) return -1;
    (void)hipMemset(*buf, 0, FT_DBG_WORDS * sizeof(long long));
    return 1;
  }
  (void)hipDeviceSynchronize();
  if (!words) return -1;
  return hipMemcpy(host_out, *buf + at, words * sizeof(long long), hipMemcpyDeviceToHost) ==
                 hipSuccess ? 0 : -1;
}
static bool ft_dbg_blocks_ok(int n) { return n >= 1 && n <= FT_DBG_BLOCKS; }

// phase timestamps (100 MHz wall clock) of workgroup 8 of the most recent fwd_head_loss
// launch -- first call arms it, second call reads 16 values back
extern "C" int ga_fused_fwd_debug(long long* host_out16) {
  return ft_dbg_read(&g_ft_dbg, true, host_out16, 0, 16);
}
// -DGA_FT_LOOP_STAMPS builds only (make EXTRA=-DGA_FT_LOOP_STAMPS): per workgroup,
// ticks in (fragment reads + MFMAs, first barrier, tile stores, second barrier)
// summed over the k-loop
extern "C" int ga_fused_fwd_debug_loop(long long* host_out, int n) {
  if (!ft_dbg_blocks_ok(n)) return -1;
  return ft_dbg_read(&g_ft_dbg, false, host_out, 16 + 3 * FT_DBG_BLOCKS, 4 * (size_t)n);
}
// (start, end of k-loop, end) of the first n workgroups of that launch, n <= 4096
extern "C" int ga_fused_fwd_debug_skew(long long* host_out, int n) {
  if (!ft_dbg_blocks_ok(n)) return -1;
  return ft_dbg_read(&g_ft_dbg, false, host_out, 16, 3 * (size_t)n);
}
// the same two hooks for dgrad_wgrad0_kernel: which = 0 -> 16 phase stamps of
// workgroup 8 (first call arms), which = 1 -> (start, end of k-loop, end) of the
// first n workgroups
extern "C" int ga_fused_dgrad_debug(long long* host_out, int which, int n) {
  if (which == 0) return ft_dbg_read(&g_dg_dbg, true, host_out, 0, 16);
  return ft_dbg_read(&g_dg_dbg, true, host_out, 16, ft_dbg_blocks_ok(n) ? 3 * (size_t)n : 0);
}
// which dbg pointer a launch of `tiles` workgroups per network gets
static long long* ft_dbg_for(long long* buf, int64_t tiles) {
  return tiles <= FT_DBG_BLOCKS ? buf : nullptr;
}

// ---- shape rules that stay link-time seams (shape_rules.h) ---------------------------------
extern "C" int ga_fused_eval_supported(int n_layers, const int* dims) {
  return ga_fused_eval_rule(n_layers, dims);
}
extern "C" int ga_fused_fwd_dgrad_supported(int width, int K, int in_w) {
  return ga_fused_fwd_dgrad_rule(width, K, in_w);
}

// The kernels that compute the first layer themselves address a tile's 64 rows and the
// weight matrices' (up to 256) rows with 32-bit BYTE offsets (GaBuffer, common.h): 256
// rows of fewer than 2^22 floats each stay below 4 GB.  Checked where such a kernel may
// be launched: the forward + loss entry (H1 and the weights; dZ2 too, for the fused
// launch's sake) and the fused entry (the data gradient's W2).  The separate
// data-gradient entry keeps 64-bit addresses and takes what it always took.
static bool ft_ld_ok(int64_t ld) { return ld >= 0 && ld < (1ll << 22); }

// ---- 1. forward + loss ---------------------------------------------------------------------
// validation + kernel parameters of one network's launch
static int fwd_build(const ga_fused_fwd_net& n, int64_t M, int width, int K,
                     FwdLossParams* out, double* flops_out) {
  const ga_fused_first_layer* first = n.first;
  const ga_fused_loss_args* loss = n.loss;
  GA_REQUIRE((n.A || first) && n.W && n.bias && n.head_W && n.head_bias && loss && n.dZ &&
                 n.hpart && n.lpart,
             "ga_fused_fwd_head_loss: null pointer");
  const float* A = n.A;
  int64_t lda = n.lda;
  const int32_t* a_idx = n.a_idx;
  if (first) {
    GA_REQUIRE(first->X && first->W && first->b && first->H &&
                   ga_fused_first_layer_ok(first->in_w, K) && K <= 256 &&
                   first->ldx >= first->in_w && first->ldh % 4 == 0 && first->ldh >= K &&
                   ga_aligned16(first->W),
               "ga_fused_fwd_head_loss: unsupported first layer");
    A = first->H;  // (only for the checks below; never read)
    lda = first->ldh;
    a_idx = nullptr;
  }
  GA_REQUIRE(ga_fused_width_ok(width) && M >= 1 && M < (1ll << 31) && K >= 1 &&
                 loss->A >= 1 && loss->A <= 8,
             "ga_fused_fwd_head_loss: unsupported shape");
  GA_REQUIRE(ft_ld_ok(lda) && ft_ld_ok(n.ldw) && ft_ld_ok(n.lddz),
             "ga_fused_fwd_head_loss: leading dimension of 2^22 floats or more");
  GA_REQUIRE(lda % 4 == 0 && n.ldw % 4 == 0 && n.head_ldw % 4 == 0 && n.lddz % 4 == 0 &&
                 ga_aligned16(A) && ga_aligned16(n.W) && ga_aligned16(n.bias) &&
                 ga_aligned16(n.head_W) && ga_aligned16(n.dZ),
             "ga_fused_fwd_head_loss: operands must be 16-B aligned quads");
  GA_REQUIRE(loss->kind == 1 ? loss->returns != nullptr
                             : (loss->actions && loss->adv &&
                                (loss->algo == 1 || loss->old_ll) &&
                                (loss->kind == 2 ||
                                 (loss->lda % 4 == 0 && ga_aligned16(loss->actions) &&
                                  loss->lda >= ((loss->A + 3) & ~3)))),
             "ga_fused_fwd_head_loss: missing / misaligned minibatch arrays");
  GA_REQUIRE(loss->kind == 2 || loss->log_std, "ga_fused_fwd_head_loss: log_std");
  GA_REQUIRE(loss->algo == 0 || loss->algo == 1, "ga_fused_fwd_head_loss: algo");
  FwdLossParams& p = *out;
  memset(&p, 0, sizeof(p));
  p.g.A = A; p.g.lda = lda; p.g.a_idx = a_idx; p.g.B = n.W; p.g.ldb = n.ldw;
  p.g.M = (int)M; p.g.N = width; p.g.K = K; p.g.bias = n.bias;
  p.head_W = n.head_W; p.head_ldw = n.head_ldw; p.head_bias = n.head_bias;
  p.loss = loss_args(loss, M);
  p.dZ = n.dZ; p.lddz = n.lddz; p.hpart = n.hpart; p.lpart = n.lpart;
  // algorithmic flops of the layers computed
  double flops = 2.0 * (double)M * width * ((double)K + loss->A);
  if (first) {
    p.l1_X = first->X; p.l1_ldx = first->ldx; p.l1_W = first->W; p.l1_b = first->b;
    p.l1_in = first->in_w; p.l1_H = first->H; p.l1_ldh = first->ldh;
    flops += 2.0 * (double)M * K * first->in_w;
  }
  *flops_out = flops;
  return GA_OK;
}

// n_nets = 2: the two networks' launches (first layer in the kernel) in ONE grid; both
// have the same width, K, input width and row count.
extern "C" int ga_fused_fwd_head_loss(const ga_fused_fwd_net* nets, int n_nets, int64_t M,
                                      int width, int K, hipStream_t stream) {
  GA_REQUIRE(nets && (n_nets == 1 || n_nets == 2),
             "ga_fused_fwd_head_loss: one or two networks");
  const ga_fused_first_layer* first = nets[0].first;
  if (n_nets == 2)
    GA_REQUIRE(first && nets[1].first && first->in_w == nets[1].first->in_w &&
                   ga_fused_pair_supported(width, K, first->in_w),
               "ga_fused_fwd_head_loss_pair: unsupported shapes");
  FwdLossPair pp;
  FwdLossParams& p = pp.a;
  double flops = 0.0;
  for (int i = 0; i < n_nets; ++i) {
    double f = 0.0;
    const int rc = fwd_build(nets[i], M, width, K, i ? &pp.b : &pp.a, &f);
    if (rc) return rc;
    flops += f;
  }
  const unsigned grid = (unsigned)(n_nets * ga_fused_tiles(M));
  const FtVariant v =
      ft_variant(FT_FWD_LOSS, width, first != nullptr, first ? first->in_w : 0, K, n_nets);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_FUSED_FWD, flops, &e0, &e1);
  if (n_nets == 1) {
    p.dbg = ft_dbg_for(g_ft_dbg, ga_fused_tiles(M));
    if (v.split) {
      p.bplanes = planes_for(nets[0].W, nets[0].ldw, width, K, PLANES_TRAIN_FWD, stream);
      GA_REQUIRE(p.bplanes, "ga_fused_fwd_head_loss: no memory for the weight planes");
      p.bplane_stride = (int64_t)width * K;
    }
    ft_launch_fwd_loss(p, v, grid, e0, e1, stream);
    GA_CHECK_LAUNCH("fwd_head_loss");
    return GA_OK;
  }
  ga_prof_count(GA_PROF_FUSED_FWD);  // (one launch, two networks' steps)
  ft_launch_fwd_loss_pair(pp, v, grid, e0, e1, stream);
  GA_CHECK_LAUNCH("fwd_head_loss_pair");
  return GA_OK;
}

// ---- the whole MLP for its outputs -----------------------------------------------------------
extern "C" int ga_fused_eval_forward(const float* X, int64_t ldx, const int32_t* idx,
                                     int64_t M, const int* dims, const float* W1,
                                     const float* b1, const float* W2, const float* b2,
                                     const float* Wh, const float* bh, float* out,
                                     int64_t ldo, hipStream_t stream) {
  GA_REQUIRE(X && dims && W1 && b1 && W2 && b2 && Wh && bh && out,
             "ga_fused_eval_forward: null pointer");
  GA_REQUIRE(ga_fused_eval_supported(3, dims), "ga_fused_eval_forward: unsupported shape");
  GA_REQUIRE(M >= 1 && M < (1ll << 31) && ldx >= dims[0] && ldo >= dims[3],
             "ga_fused_eval_forward: bad sizes");
  GA_REQUIRE(ga_aligned16(W1) && ga_aligned16(W2) && ga_aligned16(b2) && ga_aligned16(Wh),
             "ga_fused_eval_forward: operands must be 16-B aligned");
  const int in_w = dims[0], K = dims[1], width = dims[2], A = dims[3];
  FwdLossParams p;
  memset(&p, 0, sizeof(p));
  p.g.B = W2; p.g.ldb = (K + 3) & ~3;
  p.g.M = (int)M; p.g.N = width; p.g.K = K; p.g.bias = b2;
  p.head_W = Wh; p.head_ldw = (width + 3) & ~3; p.head_bias = bh;
  p.loss.idx = idx; p.loss.A = A; p.loss.kind = 2;
  p.l1_X = X; p.l1_ldx = ldx; p.l1_W = W1; p.l1_b = b1; p.l1_in = in_w;
  p.eval_out = out; p.eval_ldo = ldo;
  const unsigned grid = (unsigned)ga_fused_tiles(M);
  const FtVariant v = ft_variant(FT_EVAL_FWD, width, true, in_w, K, 1);
  const double flops = 2.0 * (double)M * ((double)K * in_w + (double)width * (K + A));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_EVAL_FWD, flops, &e0, &e1);
  if (v.split) {
    p.bplanes = planes_for(W2, p.g.ldb, width, K, PLANES_EVAL_FWD, stream);
    GA_REQUIRE(p.bplanes, "ga_fused_eval_forward: no memory for the weight planes");
    p.bplane_stride = (int64_t)width * K;
  }
  ft_launch_eval_forward(p, v, grid, e0, e1, stream);
  GA_CHECK_LAUNCH("mlp_eval_forward");
  return GA_OK;
}

// ---- 3. data gradient into the first hidden layer ------------------------------------------------
static int dgrad_build(const ga_fused_dgrad_net& n, int64_t M, int width, int K, int in_w,
                       DgradWgrad0Params* out, double* flops_out) {
  GA_REQUIRE(n.dZ2 && n.W2 && n.H1 && n.X && n.wpart, "ga_fused_dgrad_wgrad0: null pointer");
  GA_REQUIRE(ga_fused_width_ok(width) && M >= 1 && M < (1ll << 31) && K >= 1 &&
                 in_w >= 1 && in_w <= 32,
             "ga_fused_dgrad_wgrad0: unsupported shape");
  GA_REQUIRE(n.lddz % 4 == 0 && n.ldw % 4 == 0 && n.ldh % 4 == 0 && n.ldx % 4 == 0 &&
                 n.ldx >= ((in_w + 3) & ~3) && ga_aligned16(n.dZ2) && ga_aligned16(n.W2) &&
                 ga_aligned16(n.H1) && ga_aligned16(n.X) && ga_aligned16(n.wpart),
             "ga_fused_dgrad_wgrad0: operands must be 16-B aligned quads");
  DgradWgrad0Params& p = *out;
  memset(&p, 0, sizeof(p));
  p.g.A = n.dZ2; p.g.lda = n.lddz; p.g.B = n.W2; p.g.ldb = n.ldw;
  p.g.M = (int)M; p.g.N = width; p.g.K = K;
  p.H = n.H1; p.ldh = n.ldh; p.X = n.X; p.ldx = n.ldx; p.idx = n.idx; p.in_w = in_w;
  p.wpart = n.wpart;
  if (n.sum_w.src || n.sum_b.src) {
    const ga_slab_range* r[2] = {&n.sum_w, &n.sum_b};
    const ga_slab_range& any = n.sum_w.src ? n.sum_w : n.sum_b;
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    for (int i = 0; i < 2; ++i) {
      if (!r[i]->src) continue;
      GA_REQUIRE(r[i]->n >= 4 && r[i]->n % 4 == 0 && r[i]->n_part >= 1 &&
                     r[i]->stride >= r[i]->n && r[i]->stride % 4 == 0 &&
                     ga_aligned16(r[i]->src) && r[i]->stride == any.stride &&
                     r[i]->n_part == any.n_part,
                 "ga_fused_dgrad_wgrad0: bad slab range %d", i);
      const uintptr_t b = reinterpret_cast<uintptr_t>(r[i]->src);
      lo = b < lo ? b : lo;
      const uintptr_t e =
          b + sizeof(float) * (uintptr_t)((r[i]->n_part - 1) * r[i]->stride + r[i]->n);
      hi = e > hi ? e : hi;
    }
    // (the kernel addresses the ranges with 32-bit byte offsets from the lower one)
    GA_REQUIRE(hi - lo <= ((uintptr_t)1 << 32),
               "ga_fused_dgrad_wgrad0: slab ranges further apart than 2^30 floats");
    p.sum.base = reinterpret_cast<float*>(lo);
    for (int i = 0; i < 2; ++i) {
      if (!r[i]->src) continue;
      p.sum.off[i] = (uint32_t)(r[i]->src - p.sum.base);
      p.sum.nq[i] = (int)(r[i]->n / 4);
    }
    p.sum.stride = any.stride;
    p.sum.n_part = any.n_part;
    p.sum.tiles = (int)ga_fused_tiles(M);
  }
  *flops_out = 2.0 * (double)M * width * ((double)K + in_w);
  return GA_OK;
}

// n_nets = 2: two networks' launches in one grid (width 256)
extern "C" int ga_fused_dgrad_wgrad0(const ga_fused_dgrad_net* nets, int n_nets, int64_t M,
                                     int width, int K, int in_w, hipStream_t stream) {
  GA_REQUIRE(nets && (n_nets == 1 || n_nets == 2),
             "ga_fused_dgrad_wgrad0: one or two networks");
  if (n_nets == 2)
    GA_REQUIRE(width == 256, "ga_fused_dgrad_wgrad0_pair: unsupported width");
  DgradWgrad0Pair pp;
  DgradWgrad0Params& p = pp.a;
  double flops = 0.0;
  for (int i = 0; i < n_nets; ++i) {
    double f = 0.0;
    const int rc = dgrad_build(nets[i], M, width, K, in_w, i ? &pp.b : &pp.a, &f);
    if (rc) return rc;
    flops += f;
  }
  const unsigned grid = (unsigned)(n_nets * ga_fused_tiles(M));
  const FtVariant v = ft_variant(FT_DGRAD, width, false, in_w, K, n_nets);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_FUSED_DGRAD, flops, &e0, &e1);
  if (n_nets == 1) {
    p.dbg = ft_dbg_for(g_dg_dbg, ga_fused_tiles(M));
    if (v.split) {
      p.bplanes = planes_for(nets[0].W2, nets[0].ldw, K, width, PLANES_BWD, stream);
      GA_REQUIRE(p.bplanes, "ga_fused_dgrad_wgrad0: no memory for the weight planes");
      p.bplane_stride = (int64_t)width * K;
    }
    ft_launch_dgrad(p, v, grid, e0, e1, stream);
    GA_CHECK_LAUNCH("dgrad_wgrad0");
    return GA_OK;
  }
  ga_prof_count(GA_PROF_FUSED_DGRAD);
  ft_launch_dgrad_pair(pp, v, grid, e0, e1, stream);
  GA_CHECK_LAUNCH("dgrad_wgrad0_pair");
  return GA_OK;
}

// ---- 1 + 3 in one launch -------------------------------------------------------------------------
// Launches 1 and 3 of a step as ONE dispatch (fwd_dgrad_kernel), one network.  `dgrad`
// describes the same step as `fwd`: its dZ2 / H1 / X / idx are what `fwd` writes and
// gathers, and it carries no slab ranges (the weight-gradient GEMM runs after this).
// Timed as one GA_PROF_FUSED_FWD dispatch with both bodies' work; the step counter of
// GA_PROF_FUSED_DGRAD advances too: the counters count network steps.
extern "C" int ga_fused_fwd_dgrad(const ga_fused_fwd_net* fwd, const ga_fused_dgrad_net* dgrad,
                                  int64_t M, int width, int K, hipStream_t stream) {
  GA_REQUIRE(fwd && dgrad && fwd->first && fwd->loss, "ga_fused_fwd_dgrad: null pointer");
  const ga_fused_first_layer* first = fwd->first;
  GA_REQUIRE(ga_fused_fwd_dgrad_supported(width, K, first->in_w) && !split_bf16_on(),
             "ga_fused_fwd_dgrad: unsupported shape or mode");
  GA_REQUIRE(dgrad->dZ2 == fwd->dZ && dgrad->lddz == fwd->lddz && dgrad->H1 == first->H &&
                 dgrad->ldh == first->ldh && dgrad->X == first->X &&
                 dgrad->ldx == first->ldx && dgrad->idx == fwd->loss->idx &&
                 !dgrad->sum_w.src && !dgrad->sum_b.src,
             "ga_fused_fwd_dgrad: the two descriptors are not one step's");
  GA_REQUIRE(ft_ld_ok(dgrad->ldw),
             "ga_fused_fwd_dgrad: leading dimension of 2^22 floats or more");
  FwdDgradParams pp;
  double f0 = 0.0, f1 = 0.0;
  int rc = fwd_build(*fwd, M, width, K, &pp.f, &f0);
  if (rc) return rc;
  rc = dgrad_build(*dgrad, M, K, width, first->in_w, &pp.d, &f1);
  if (rc) return rc;
  pp.f.dbg = ft_dbg_for(g_ft_dbg, ga_fused_tiles(M));
  pp.d.dbg = ft_dbg_for(g_dg_dbg, ga_fused_tiles(M));
  const unsigned grid = (unsigned)ga_fused_tiles(M);
  const FtVariant v = ft_variant(FT_FWD_DGRAD, width, true, first->in_w, K, 1);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_FUSED_FWD, f0 + f1, &e0, &e1);
  ga_prof_count(GA_PROF_FUSED_DGRAD);
  ft_launch_fwd_dgrad(pp, v, grid, e0, e1, stream);
  GA_CHECK_LAUNCH("fwd_dgrad");
  return GA_OK;
}

// ---- 4. partial sums -> gradient -> Adam ------------------------------------------------------------
// regions + optimizer constants of one network into slot `net` of the launch
static int reduce_add_net(ReduceRegionsParams& p, int net, const ga_reduce_net& n) {
  const ga_fused_region* regions = n.regions;
  GA_REQUIRE(regions && n.params && n.grads && n.exp_avg && n.exp_avg_sq && n.lpart &&
                 n.loss,
             "ga_reduce_regions_adam: null pointer");
  GA_REQUIRE(n.n_regions >= 1 && p.n_regions + n.n_regions <= FT_MAX_REGIONS &&
                 n.step >= 1 && n.n_lpart >= 1 && (n.presummed >> n.n_regions) == 0,
             "ga_reduce_regions_adam: bad arguments");
  int64_t v = p.n_virtual;
  for (int k = 0; k < n.n_regions; ++k) {
    // regions are walked 4 elements at a time: the flat layout pads every weight
    // row and bias vector to a multiple of 4 floats, and the padding of every
    // partial is zero, so a region is rounded up to whole quads
    GA_REQUIRE(regions[k].src && regions[k].n >= 1 && regions[k].n_part >= 1 &&
                   regions[k].beg >= 4 && regions[k].beg % 4 == 0 &&
                   regions[k].stride % 4 == 0 && ga_aligned16(regions[k].src),
               "ga_reduce_regions_adam: bad region %d", k);
    FtRegion& r = p.r[p.n_regions + k];
    r.beg = regions[k].beg; r.n = (regions[k].n + 3) & ~(int64_t)3;
    r.src = regions[k].src;
    r.stride = regions[k].stride; r.n_part = regions[k].n_part;
    r.quads = regions[k].n_part <= 128 ? 64 : 16;
    r.pre = (n.presummed >> k) & 1u;
    // (a pre-summed region has a quad per THREAD to move, not per four or sixteen)
    if (r.pre) r.quads = 256;
    r.vbeg = v;
    r.net = net;
    v += ga_ceil_div(r.n / 4, r.quads);  // workgroups of this region
  }
  p.n_regions += n.n_regions;
  p.n_virtual = v;
  FtNet& N = p.net[net];
  N.a.p = n.params; N.a.m = n.exp_avg; N.a.v = n.exp_avg_sq;
  N.a.c = ga_adam_coeffs(n.lr, n.beta1, n.beta2, n.eps, n.step);
  N.grads = n.grads; N.scale = n.scale; N.do_adam = n.do_adam;
  N.zero_slot0 = n.zero_slot0;
  N.lpart = n.lpart; N.n_lpart = n.n_lpart; N.M = n.M;
  N.loss = loss_args(n.loss, n.M);
  N.loss_out = n.loss_out;
  return GA_OK;
}

// developer / test switch: 0 = every forward launch computes its planes itself again
static int g_adam_planes = -1;
static bool adam_planes_on() {
  if (g_adam_planes < 0) {
    const char* e = getenv("GARAGE_AMD_SPLIT_ADAM_PLANES");
    g_adam_planes = (e && e[0] == '0') ? 0 : 1;
  }
  return g_adam_planes != 0;
}
extern "C" int ga_set_split_adam_planes(int on) {
  g_adam_planes = on != 0;
  return 0;
}
// trust in optimizer-written planes never outlives an epoch call (anything may write
// the parameters between two calls)
extern "C" void ga_planes_epoch_begin(void) {
  std::lock_guard<std::mutex> lock(g_plane_mu);
  for (PlaneBuf& b : g_plane_bufs) b.adam_fresh = false;
}

// n_nets = 2: both networks' optimizer steps in one launch (regions of two flat buffers,
// two loss blocks); the same per-element arithmetic and summation trees as two single
// launches
extern "C" int ga_reduce_regions_adam(const ga_reduce_net* nets, int n_nets,
                                      hipStream_t stream) {
  GA_REQUIRE(nets && (n_nets == 1 || n_nets == 2),
             "ga_reduce_regions_adam: one or two networks");
  ReduceRegionsParams p;
  memset(&p, 0, sizeof(p));
  for (int i = 0; i < n_nets; ++i) {
    const int rc = reduce_add_net(p, i, nets[i]);
    if (rc) return rc;
  }
  p.n_nets = n_nets;
  // (with do_adam) the launch also rewrites the planes of W = params + pl_beg
  // ([rows][cols], ld = cols); update.cpp asks for it when the step's forward launch
  // ran the split-operand kernel
  GA_REQUIRE(n_nets == 1 || (!nets[0].pl_rows && !nets[1].pl_rows),
             "ga_reduce_regions_adam: no plane rewriting for two networks");
  const int rows = nets[0].pl_rows, cols = nets[0].pl_cols;
  if (rows > 0 && adam_planes_on() && nets[0].do_adam && split_bf16_on(1) &&
      rows % 32 == 0 && cols % 32 == 0) {
    const float* W = nets[0].params + nets[0].pl_beg;
    PlaneBuf* written = nullptr;
    std::lock_guard<std::mutex> lock(g_plane_mu);
    for (PlaneBuf& b : g_plane_bufs)
      if (b.W == W && b.rows == rows && b.cols == cols) written = &b;
    if (written) {  // (the forward launch of this step created it)
      p.net[0].pl_fwd = reinterpret_cast<uint32_t*>(written->fwd);
      p.net[0].pl_bwd = reinterpret_cast<uint32_t*>(written->bwd);
      p.net[0].pl_beg = nets[0].pl_beg;
      p.net[0].pl_rows = rows;
      p.net[0].pl_cols = cols;
      written->adam_fresh = true;
      written->adam_stream = stream;
      written->bwd_fresh = false;
    }
  }
  const unsigned blocks = (unsigned)p.n_virtual + n_nets;  // + one loss block per network
  ft_launch_reduce_regions(p, blocks, stream);
  GA_CHECK_LAUNCH(n_nets == 2 ? "reduce_regions_adam_pair" : "reduce_regions_adam");
  return GA_OK;
}
