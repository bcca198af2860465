// The per-layer MLP passes: forward, backward (weight + data gradients into split-K
// slabs) and the tangent pass, one launch per layer product.  Every network that is
// not a 2 x {32, 64, 128, 256} tanh net trains on them: wide layers, relu / elu / ...
// hidden layers, layer_normalization, output_nonlinearity, TRPO's tangent pass.
//
// Host C++ only.  A layer is described ONCE (Layer, describe_layer: where its input,
// weights and LayerNorm pieces sit in the flat layouts); a product of a layer is built
// ONCE per kind (forward_product, wgrad_product, dgrad_product and the two tangent
// products); each pass then reads: for each layer, describe, ask the plans
// (layer_plans.h: streaming, head-fused, tile -- which kernel takes a product is written
// there, once) in that order, launch the first that takes the product.  The launch seam
// of layer_plans.h and lnorm.hip's entry points are all this file calls, so
// tests/host/mlp_layers_harness.cpp builds it for the CPU against recording fakes
// (`make asan-mlp`).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "internal.h"
#include "fused_train.h"
#include "layer_plans.h"
#include "members_diag.h"

// ---------------------------------------------------------------------------
// Developer switches of this dispatch
// ---------------------------------------------------------------------------
// The whole-network forward in one launch (ga_mlp_forward_fused_f32,
// policy_fused.hip) for nets whose layers fit its LDS tiles;
// ga_set_fused_forward(0) forces the per-layer GEMMs.
// Off by default: at the C3 minibatch (32768 x 256 x 256) the fused forward
// measures 86-107 us against 82-87 us for the three per-layer GEMMs -- it keeps
// one workgroup per CU (140 KB of LDS) and its per-layer epilogues are exposed,
// which costs what the saved activation round trip gains.  The rollout step
// (policy_step_fused_kernel, n_envs rows) is where the fusion pays.
static int g_fused_forward = 0;
extern "C" int ga_set_fused_forward(int on) {
  g_fused_forward = on != 0;
  return 0;
}

// Outputs-only forward of a whole two-hidden-layer tanh network in one launch
// (fused_train.hip: mlp_eval_forward_kernel); ga_set_eval_forward(0) makes callers
// that ask fall back to the per-layer kernels.
static int g_eval_forward = -1;
extern "C" int ga_set_eval_forward(int on) {
  g_eval_forward = on != 0;
  return GA_OK;
}
extern "C" int ga_mlp_forward_eval_supported(const ga_mlp_desc* d) {
  if (g_eval_forward < 0) {
    const char* e = getenv("GARAGE_AMD_EVAL_FORWARD");
    g_eval_forward = e ? atoi(e) != 0 : 1;
  }
  // (64-wide layers: the per-layer kernels' 64 x 64 tiles are 2 % faster at C2)
  return g_eval_forward && d && d->n_layers == 3 && d->hidden_act == 0 &&
         d->output_act == 0 && !d->layer_norm && d->dims[1] >= 128 && d->dims[2] >= 128 &&
         ga_fused_eval_supported(3, d->dims);
}

// 0 off, 1 hidden layers up to 128 wide, 2 also 256-wide ones.  At 256 units the
// fused launch (64 x 256 tiles, 75 KB of LDS) saves 7.7 us per minibatch with the
// chip to itself (C3, one stream: 167.0 -> 160.6 ms per iteration) but loses 1 %
// when the policy and value chains share the chip on two streams, where the narrow
// head GEMM it replaces was hidden under the other chain's kernels anyway
// (3 x A/B: 147.1 / 148.5 / 149.4 vs 146.6 / 146.7 / 147.5 ms) -- so the default
// stops at 128 and both schedules keep the same arithmetic.
static int g_fuse_head_forward = 1;
extern "C" int ga_set_fused_head_forward(int mode) {
  g_fuse_head_forward = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return 0;
}
static int g_fuse_head_dgrad = 1;
extern "C" int ga_set_fused_head_dgrad(int on) {
  g_fuse_head_dgrad = on != 0;
  return 0;
}
static int g_skinny = 1;
extern "C" int ga_set_skinny_kernels(int on) {
  g_skinny = on != 0;
  return 0;
}
// the 64 x 64 x 128 tiles for products with few 128 x 128 tiles (layer_plans.h: GT_SMALL_M)
static int g_small_m = 1;
extern "C" int ga_set_small_m_gemm(int on) {
  g_small_m = on != 0;
  return 0;
}
// the paired-column instantiation of the 128 x 128 weight-gradient GEMM (layer_plans.h:
// ga_gemm_paired_ok; gemm.hip: gemm_rr_paired_kernel).  0 (or GARAGE_AMD_WGRAD_PAIRED=0
// in the environment when the library is first used): gemm_f32_kernel for every shape.
// Bit-identical results either way.
static int g_wgrad_paired = -1;
static bool wgrad_paired_on() {
  if (g_wgrad_paired < 0) {
    const char* e = getenv("GARAGE_AMD_WGRAD_PAIRED");
    g_wgrad_paired = (e && e[0] == '0') ? 0 : 1;
  }
  return g_wgrad_paired != 0;
}
extern "C" int ga_set_wgrad_paired_columns(int on) {
  g_wgrad_paired = on != 0;
  return 0;
}

extern "C" int64_t ga_mlp_backward_splits(const ga_mlp_desc* d, int64_t M) {
  // Rows of the batch each weight-gradient workgroup reduces before writing a
  // slab: large enough to amortise the slab write, small enough to fill 256 CUs.
  // 256 rows per slab: the widest layer (256x256 -> 2x2 tiles) then launches
  // 4 * M/256 workgroups, i.e. 512 at the C3 minibatch of 32768 rows.
  int64_t s = ga_ceil_div(M, 256);
  // nets whose layers are all <= 64 wide have one weight-gradient tile per split:
  // 128-row slabs double the workgroups (their slabs are a few KB each)
  bool small = true;
  for (int l = 0; l <= d->n_layers; ++l) small = small && d->dims[l] <= 64;
  if (small) s = ga_ceil_div(M, 128);
  // wide layers have many output tiles per split: fewer, longer splits then fill the
  // chip just as well, and every split less is a slab of the whole parameter vector
  // not written and not read back (C5, 512-wide layers: 16 tiles per split; 128 splits
  // of 512 rows moved 744 MB of slabs per optimizer step, 64 splits of 1024 rows --
  // 1024 workgroups for the widest layer -- move half).  256 x 256 layers (4 tiles)
  // keep 128 splits.
  int64_t tiles = 1;
  for (int l = 0; l < d->n_layers; ++l) {
    const int64_t t = ga_ceil_div(d->dims[l + 1], 128) * ga_ceil_div(d->dims[l], 128);
    tiles = t > tiles ? t : tiles;
  }
  static int64_t target_env = -1;  // workgroups of the widest layer's weight gradient
  if (target_env < 0) {
    const char* e = getenv("GARAGE_AMD_WGRAD_WORKGROUPS");  // developer sweep
    target_env = e ? atoll(e) : 0;
    if (target_env < 1) target_env = 0;
  }
  // (the split-operand weight-gradient kernel is three times faster per row: half the
  // workgroups and half the slabs -- 64 splits at C3 -- are the better trade there,
  // measured 82.3 -> 79.8 ms per iteration; an engine keeps the split count it was
  // built with)
  const int64_t target = target_env ? target_env : (ga_split_bf16_enabled() ? 256 : 1024);
  int64_t by_tiles = ga_ceil_div(target, tiles);
  // (never below 64 splits on that account: the streaming weight-gradient kernels of the
  // narrow layers take one workgroup per split and column block)
  if (!target_env && ga_split_bf16_enabled() && by_tiles < 64) by_tiles = 64;
  if (!small && s > by_tiles) s = by_tiles;
  if (s < 1) s = 1;
  if (s > 128) s = 128;
  return s;
}

static int check_desc(const ga_mlp_desc* d, const char* who) {
  GA_REQUIRE(d != nullptr, "%s: null descriptor", who);
  GA_REQUIRE(d->n_layers >= 1 && d->n_layers <= 8, "%s: n_layers %d not in 1..8",
             who, d->n_layers);
  for (int l = 0; l <= d->n_layers; ++l)
    GA_REQUIRE(d->dims[l] >= 1, "%s: dims[%d] < 1", who, l);
  for (int l = 0; l < d->n_layers; ++l)
    GA_REQUIRE(d->w_off[l] % 4 == 0 && d->act_off[l] % 4 == 0,
               "%s: offsets of layer %d not 16-B aligned", who, l);
  GA_REQUIRE(d->hidden_act >= 0 && d->hidden_act <= 6, "%s: hidden_act %d not in 0..6",
             who, d->hidden_act);
  GA_REQUIRE(d->output_act >= 0 && d->output_act <= 6, "%s: output_act %d not in 0..6",
             who, d->output_act);
  if (d->layer_norm)
    for (int l = 0; l + 1 < d->n_layers; ++l)
      GA_REQUIRE(d->ln_off[l] % 4 == 0 && d->lnx_off[l] % 4 == 0 && d->dims[l] <= 1024,
                 "%s: layer normalisation of layer %d: unaligned offsets or more than "
                 "1024 inputs", who, l);
  return GA_OK;
}

// ---------------------------------------------------------------------------
// One layer, described once
// ---------------------------------------------------------------------------
// Layer l of `d` over the flat vector `theta` (the parameters, or a tangent in the
// same layout) and the workspace `acts` (the activations of a forward pass, or their
// tangents): LayerNorm(prev) -> Linear -> nonlinearity
// (multi_headed_mlp_module.py:77-92).
struct Layer {
  int in_w, out_w;
  bool is_last;
  bool norm_in;  // a hidden layer of a layer_norm net: the products read `in` =
                 // the normalised copy of `raw`
  // the layer below's output: X through row_idx, or the previous activation
  const float* raw; int64_t ld_raw; const int32_t* raw_idx;
  // what the layer's products read
  const float* in; int64_t ld_in; const int32_t* in_idx;
  const float* W; int64_t ldw;  // [out_w][ldw], ldw = round4(in_w): the row stride of
                                // every other [.][in_w] matrix of the layer as well
  const float* bias;
  // norm_in: gamma / beta [ldw] in `theta`'s layout; per-row (mean, rstd) pairs and
  // the normalised rows [M][ldw] in `acts`' layout
  int64_t gamma_off, beta_off, stats_off, xn_off;
};

static Layer describe_layer(const ga_mlp_desc* d, int l, const float* theta, const float* X,
                            int64_t ldx, const int32_t* row_idx, const float* acts) {
  Layer y = {};
  y.in_w = d->dims[l];
  y.out_w = d->dims[l + 1];
  y.is_last = l == d->n_layers - 1;
  y.norm_in = d->layer_norm && !y.is_last;
  y.ldw = round4(y.in_w);
  if (l == 0) {
    y.raw = X; y.ld_raw = ldx; y.raw_idx = row_idx;
  } else {
    y.raw = acts + d->act_off[l - 1]; y.ld_raw = y.ldw;
  }
  y.in = y.raw; y.ld_in = y.ld_raw; y.in_idx = y.raw_idx;
  if (y.norm_in) {
    y.gamma_off = d->ln_off[l]; y.beta_off = d->ln_off[l] + y.ldw;
    y.stats_off = d->lns_off[l]; y.xn_off = d->lnx_off[l];
    y.in = acts + y.xn_off; y.ld_in = y.ldw; y.in_idx = nullptr;
  }
  y.W = theta + d->w_off[l];
  y.bias = theta + d->b_off[l];
  return y;
}

// ---------------------------------------------------------------------------
// The products of a layer, one builder per kind
// ---------------------------------------------------------------------------
// one split over the whole of K
static int full_k(int K) { return (int)ga_ceil_div(K, BK) * BK; }
// batch rows per split-K slab
static int rows_per_split(int64_t M, int64_t n_splits) {
  return (int)(ga_ceil_div(ga_ceil_div(M, n_splits), BK) * BK);
}

// C = act(in W^T + b), M rows; head: the next (narrow, linear) layer in the same
// launch, out = C head.W^T + head.bias (ga_gemm_head_launch)
static GemmParams forward_product(const Layer& y, int64_t M, float* C, int64_t ldc, int act,
                                  const Layer* head = nullptr, float* out = nullptr,
                                  int64_t ldo = 0) {
  GemmParams p = {};
  p.A = y.in; p.lda = y.ld_in; p.a_idx = y.in_idx;
  p.B = y.W; p.ldb = y.ldw;
  p.C = C; p.c_rs = ldc; p.c_cs = 1;
  p.M = (int)M; p.N = y.out_w; p.K = y.in_w;
  p.epi = EPI_BIAS_ACT;
  p.bias = y.bias;
  p.act = act;
  p.k_per_split = full_k(p.K);
  if (head) {
    p.head_W = head->W; p.head_ldw = head->ldw;
    p.head_bias = head->bias;
    p.head_n = head->out_w;
    p.head_out = out; p.head_ld = ldo;
  }
  return p;
}

// dW[o][i] = sum_b dz[b][o] * in[b][i] and db = column sums of dz, split-K over the M
// rows into n_splits slabs (slab_w, slab_b: split 0's).  (gz: the pair plan's split
// count; ga_gemm_plan takes it as an argument.)
static GemmParams wgrad_product(const Layer& y, const float* dz, int64_t lddz, int64_t M,
                                int64_t n_splits, float* slab_w, float* slab_b,
                                int64_t slab_stride) {
  GemmParams p = {};
  p.K = (int)M;
  p.k_per_split = rows_per_split(M, n_splits);
  p.gz = (int)n_splits;
  p.epi = EPI_PLAIN;
  p.C = slab_w;
  p.c_split_stride = slab_stride;
  p.colsum = slab_b;
  p.colsum_split_stride = slab_stride;
  if (y.out_w <= 32) {
    // narrow out: compute dW^T = in^T dz so the narrow side is N
    p.A = y.in; p.lda = y.ld_in; p.a_idx = y.in_idx; p.B = dz; p.ldb = lddz;
    p.M = y.in_w; p.N = y.out_w;
    p.c_rs = 1; p.c_cs = y.ldw;
    p.colsum_of_b = 1;
  } else {
    // (out x in), natural orientation: narrow in (256x32 tiles) or both sides wide
    p.A = dz; p.lda = lddz; p.B = y.in; p.ldb = y.ld_in; p.b_idx = y.in_idx;
    p.M = y.out_w; p.N = y.in_w;
    p.c_rs = y.ldw; p.c_cs = 1;
    p.colsum_of_b = 0;
  }
  return p;
}

// The same product as the streaming kernel states it: C(wide, narrow) with the side that
// is <= 32 as the narrow one (wgrad_product's choice of orientation); the bias gradient
// is the column sums of whichever side dz is.
static SkinnyWgradParams skinny_wgrad_product(const Layer& y, const float* dz, int64_t lddz,
                                              int64_t M, int64_t n_splits, float* slab_w,
                                              float* slab_b, int64_t slab_stride) {
  SkinnyWgradParams p = {};
  p.rows = (int)M;
  p.rows_per_split = rows_per_split(M, n_splits);
  p.n_splits = (int)n_splits;
  p.C = slab_w;
  p.split_stride = slab_stride;
  if (y.out_w <= 32) {
    // head layer: wide = the layer input, narrow = dz
    p.Wd = y.in; p.ldw = y.ld_in; p.w_idx = y.in_idx; p.Nr = dz; p.ldn = lddz;
    p.wide = y.in_w; p.NS = y.out_w;
    p.c_wide_stride = 1; p.c_narrow_stride = y.ldw;
    p.colsum_narrow = slab_b;
  } else {
    // wide = dz, narrow = the layer input
    p.Wd = dz; p.ldw = lddz; p.Nr = y.in; p.ldn = y.ld_in; p.n_idx = y.in_idx;
    p.wide = y.out_w; p.NS = y.in_w;
    p.c_wide_stride = y.ldw; p.c_narrow_stride = 1;
    p.colsum_wide = slab_b;
  }
  return p;
}

// dst = dz W, M rows; H: times the slope of the hidden activation at H (the layer
// below's output); null: the plain product (a normalised input: ga_ln_backward follows)
static GemmParams dgrad_product(const Layer& y, int64_t M, const float* dz, int64_t lddz,
                                float* dst, const float* H, int hact) {
  GemmParams p = {};
  p.A = dz; p.lda = lddz;
  p.B = y.W; p.ldb = y.ldw;
  p.C = dst; p.c_rs = y.ldw; p.c_cs = 1;
  p.M = (int)M; p.N = y.in_w; p.K = y.out_w;
  if (H) {
    p.epi = EPI_MUL_DTANH;
    p.H = H; p.ldh = y.ldw;
    p.hact = hact;
  } else {
    p.epi = EPI_PLAIN;
  }
  p.k_per_split = full_k(p.K);
  return p;
}

// The tangent of a layer's pre-activation is two products.  First in dW^T + db, with
// `t` the layer over the tangent vector; `slope`: it is the only product, so the
// activation's slope at H goes with it.
static GemmParams tangent_weight_product(const Layer& t, int64_t M, float* C, int64_t ldc,
                                         bool slope, const float* H, int hact) {
  GemmParams p = forward_product(t, M, C, ldc, 0);
  if (slope) { p.H = H; p.ldh = ldc; p.hact = hact; }
  return p;
}
// ... then += tin W^T, with `w` the layer over the parameters and the TANGENT
// activations, and the slope at H (null: the output layer)
static GemmParams tangent_input_product(const Layer& w, int64_t M, float* C, int64_t ldc,
                                        const float* H, int hact) {
  GemmParams q = {};
  q.A = w.in; q.lda = w.ld_in;
  q.B = w.W; q.ldb = w.ldw;
  q.C = C; q.c_rs = ldc; q.c_cs = 1;
  q.M = (int)M; q.N = w.out_w; q.K = w.in_w;
  q.accum = 1;
  if (H) { q.epi = EPI_MUL_DTANH; q.H = H; q.ldh = ldc; q.hact = hact; }
  else q.epi = EPI_PLAIN;
  q.k_per_split = full_k(q.K);
  return q;
}

// ---------------------------------------------------------------------------
// Plan, then launch (layer_plans.h)
// ---------------------------------------------------------------------------
// The tile kernel takes every product: plan it under the switches, fill in what the plan
// decides -- the weight planes are this side's to fetch -- and launch.
static int launch_product(GemmParams p, int a_kc, int b_kc, int splits, hipStream_t stream) {
  GA_REQUIRE(a_kc || !b_kc, "ga_gemm_launch: orientation not instantiated");
  const GemmSwitches sw = {g_small_m != 0, ga_split_bf16_gemm() != 0,
                           ga_split_bf16_enabled() != 0, wgrad_paired_on()};
  const GemmPlan plan = ga_gemm_plan(p, a_kc, b_kc, splits, sw);
  ga_gemm_apply(plan, &p);
  if (plan.planes) {
    p.bplanes = ga_weight_planes(p.B, p.ldb, b_kc ? p.N : p.K, b_kc ? p.K : p.N,
                                 plan.planes_bwd, stream);
    GA_REQUIRE(p.bplanes, "gemm: no memory for the weight planes");
  }
  return ga_gemm_launch(plan, p, stream);
}

// The plan of the streaming forward (w_kc) / data gradient of `p` under the switches
static SkinnyFwdPlan skinny_forward_plan(const GemmParams& p, bool w_kc) {
  static int rows_wg = -1;  // rows per workgroup
  if (rows_wg < 0) {
    const char* e = getenv("GARAGE_AMD_SKINNY_ROWS");  // A/B runs
    rows_wg = e ? atoi(e) : 0;
    if (rows_wg < 1) rows_wg = 32;
  }
  return ga_skinny_fwd_plan(p, w_kc, g_skinny != 0, rows_wg);
}
// ... launched where it takes the product: *taken says whether it did.
static int try_skinny_forward(const GemmParams& p, bool w_kc, bool* taken,
                              hipStream_t stream) {
  const SkinnyFwdPlan plan = skinny_forward_plan(p, w_kc);
  *taken = plan.taken;
  return plan.taken ? ga_skinny_fwd_launch(plan, ga_skinny_fwd_params(p, plan), stream)
                    : GA_OK;
}

// The launch that computes layer l of a forward pass over M rows (y = describe_layer's),
// decided and NOT made: the streaming kernel, else this layer and the head in one launch,
// else the tiles.  ga_mlp_forward_f32 launches the step; ga_mlp_forward_steps hands it to
// the population's joint forward (members_diag_host.cpp), which launches the same kernel
// for every member at once.
static GaForwardStep plan_forward_step(const ga_mlp_desc* d, int l, const Layer& y,
                                       const float* params, const float* X, int64_t ldx,
                                       const int32_t* row_idx, int64_t M, float* acts,
                                       float* out, int64_t ldo) {
  const int L = d->n_layers;
  GaForwardStep st = {};
  st.layer = l;
  // the last hidden layer of a net with a linear head may take the head along
  const bool with_head =
      out && l == L - 2 && d->output_act == 0 && !d->layer_norm &&
      (g_fuse_head_forward == 2 || (g_fuse_head_forward == 1 && y.out_w <= 128));
  Layer head = {};
  if (with_head) head = describe_layer(d, L - 1, params, X, ldx, row_idx, acts);
  st.g = forward_product(
      y, M, y.is_last ? out : acts + d->act_off[l], y.is_last ? ldo : round4(y.out_w),
      y.is_last ? d->output_act : act_forward_code(d->hidden_act),
      with_head ? &head : nullptr, out, ldo);
  st.sp = skinny_forward_plan(st.g, true);
  if (st.sp.taken) {
    st.kind = MD_FWD_SKINNY;
    st.s = ga_skinny_fwd_params(st.g, st.sp);
    return st;
  }
  if (with_head) {
    st.hp = ga_gemm_head_plan(st.g);
    if (st.hp.taken) {
      st.kind = MD_FWD_GEMM_HEAD;
      ga_gemm_head_apply(st.hp, &st.g);
      return st;
    }
    st.g.head_n = 0;
  }
  st.kind = MD_FWD_GEMM;
  const GemmSwitches sw = {g_small_m != 0, ga_split_bf16_gemm() != 0,
                           ga_split_bf16_enabled() != 0, wgrad_paired_on()};
  st.gp = ga_gemm_plan(st.g, 1, 1, 1, sw);
  ga_gemm_apply(st.gp, &st.g);
  return st;
}

// ---------------------------------------------------------------------------
// C ABI (see include/garage_amd.h)
// ---------------------------------------------------------------------------
extern "C" int ga_mlp_forward_f32(const ga_mlp_desc* d, const float* params,
                                  const float* X, int64_t ldx,
                                  const int32_t* row_idx, int64_t M, float* acts,
                                  float* out, int64_t ldo, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_desc(d, "ga_mlp_forward_f32");
  if (rc) return rc;
  GA_REQUIRE(params && X, "ga_mlp_forward_f32: null pointer");
  // out == NULL: hidden layers only (the head is fused into the loss kernel)
  GA_REQUIRE(out || d->n_layers >= 2, "ga_mlp_forward_f32: nothing to compute");
  // acts == NULL: outputs only (ga_mlp_forward_eval_supported: the whole network in
  // one launch, no activation reaches memory)
  if (!acts && d->n_layers > 1) {
    GA_REQUIRE(out && ga_mlp_forward_eval_supported(d),
               "ga_mlp_forward_f32: acts workspace needed");
    GA_REQUIRE(M >= 0 && M < (1ll << 31), "ga_mlp_forward_f32: bad M");
    if (M == 0) return GA_OK;
    return ga_fused_eval_forward(X, ldx, row_idx, M, d->dims, params + d->w_off[0],
                                 params + d->b_off[0], params + d->w_off[1],
                                 params + d->b_off[1], params + d->w_off[2],
                                 params + d->b_off[2], out, ldo, stream);
  }
  GA_REQUIRE(M >= 0 && M < (1ll << 31), "ga_mlp_forward_f32: bad M");
  GA_REQUIRE(ldx % 4 == 0 && ldx >= d->dims[0], "ga_mlp_forward_f32: ldx %lld",
             (long long)ldx);
  GA_REQUIRE(!out || ldo >= d->dims[d->n_layers], "ga_mlp_forward_f32: ldo too small");
  GA_REQUIRE(ga_aligned16(params) && ga_aligned16(X) && (!acts || ga_aligned16(acts)),
             "ga_mlp_forward_f32: pointers must be 16-B aligned");
  if (M == 0) return GA_OK;
  if (out && g_fused_forward && d->hidden_act == 0 && d->output_act == 0 &&
      !d->layer_norm && ga_policy_step_fused_supported(d))
    return ga_mlp_forward_fused_f32(d, params, X, ldx, row_idx, M, acts, out, ldo,
                                    stream);
  const int L = d->n_layers;
  for (int l = 0; l < L; ++l) {
    const Layer y = describe_layer(d, l, params, X, ldx, row_idx, acts);
    if (y.is_last && !out) break;
    if (y.norm_in) {
      // the GEMM reads the normalised rows
      rc = ga_ln_forward(y.raw, y.ld_raw, y.raw_idx, M, y.in_w, params + y.gamma_off,
                         params + y.beta_off, acts + y.xn_off, y.ldw, acts + y.stats_off,
                         stream);
      if (rc) return rc;
    }
    GaForwardStep st = plan_forward_step(d, l, y, params, X, ldx, row_idx, M, acts, out, ldo);
    if (st.kind == MD_FWD_SKINNY) {
      rc = ga_skinny_fwd_launch(st.sp, st.s, stream);
    } else if (st.kind == MD_FWD_GEMM_HEAD) {
      return ga_gemm_head_launch(st.hp, st.g, stream);  // both layers done
    } else {
      if (st.gp.planes) {  // the weight planes are this side's to fetch
        st.g.bplanes = ga_weight_planes(st.g.B, st.g.ldb, st.g.N, st.g.K, st.gp.planes_bwd,
                                        stream);
        GA_REQUIRE(st.g.bplanes, "gemm: no memory for the weight planes");
      }
      rc = ga_gemm_launch(st.gp, st.g, stream);
    }
    if (rc) return rc;
  }
  return GA_OK;
}

// (members_diag.h)
int ga_mlp_forward_steps(const ga_mlp_desc* d, const float* params, const float* X,
                         int64_t ldx, const int32_t* row_idx, int64_t M, float* acts,
                         float* out, int64_t ldo, GaForwardStep* steps, int* n_steps) {
  int rc = check_desc(d, "ga_mlp_forward_steps");
  if (rc) return rc;
  GA_REQUIRE(params && X && acts && out && steps && n_steps,
             "ga_mlp_forward_steps: null pointer");
  GA_REQUIRE(M >= 1 && M < (1ll << 31), "ga_mlp_forward_steps: bad M");
  GA_REQUIRE(ldx % 4 == 0 && ldx >= d->dims[0], "ga_mlp_forward_steps: ldx %lld",
             (long long)ldx);
  GA_REQUIRE(ldo >= d->dims[d->n_layers], "ga_mlp_forward_steps: ldo too small");
  GA_REQUIRE(ga_aligned16(params) && ga_aligned16(X) && ga_aligned16(acts),
             "ga_mlp_forward_steps: pointers must be 16-B aligned");
  GA_REQUIRE(!d->layer_norm, "ga_mlp_forward_steps: layer normalisation is no layer product");
  GA_REQUIRE(!(g_fused_forward && d->hidden_act == 0 && d->output_act == 0 &&
               ga_policy_step_fused_supported(d)),
             "ga_mlp_forward_steps: ga_set_fused_forward(1) takes this network in one launch");
  *n_steps = 0;
  for (int l = 0; l < d->n_layers; ++l) {
    const Layer y = describe_layer(d, l, params, X, ldx, row_idx, acts);
    GaForwardStep st = plan_forward_step(d, l, y, params, X, ldx, row_idx, M, acts, out, ldo);
    GA_REQUIRE(st.kind != MD_FWD_GEMM || !st.gp.planes,
               "ga_mlp_forward_steps: layer %d takes the split-operand GEMM", l);
    steps[(*n_steps)++] = st;
    if (st.kind == MD_FWD_GEMM_HEAD) break;  // both layers done
  }
  return GA_OK;
}

// dW = dz^T in (+ db = column sums of dz) of the MIDDLE layer of a 3-layer network,
// out_w x in_w with 33 .. wide sides (the 128 x 128-tile kernel), split-K over the M
// rows into n_splits slabs: the launch ga_mlp_backward_range_f32 makes for layer 1 with
// fused_first = 1, for two networks in one grid.  Same tiles, same k ranges, same
// summation order per element: both take their descriptor from wgrad_product.
// (One network: ga_mlp_backward_range_f32, any depth.)
extern "C" int ga_wgrad_mid(const ga_wgrad_mid_net* nets, int n_nets, int64_t M,
                            int64_t n_splits, int out_w, int in_w, hipStream_t stream) {
  GA_REQUIRE(nets && n_nets == 2,
             "ga_wgrad_mid: two networks (one: ga_mlp_backward_range_f32)");
  GA_REQUIRE(M > 0 && M < (1ll << 31) && n_splits >= 1 && n_splits <= 1024 &&
                 out_w > 64 && in_w > 64,
             "ga_wgrad_mid_pair: unsupported shape");
  GemmParams p[2];
  for (int i = 0; i < n_nets; ++i) {
    const ga_wgrad_mid_net& n = nets[i];
    GA_REQUIRE(n.dz && n.in && n.slabs_w && n.slabs_b, "ga_wgrad_mid_pair: null pointer");
    GA_REQUIRE(n.slab_stride % 4 == 0, "ga_wgrad_mid_pair: unsupported shape");
    GA_REQUIRE(ga_aligned16(n.dz) && ga_aligned16(n.in) && ga_aligned16(n.slabs_w),
               "ga_wgrad_mid_pair: pointers must be 16-B aligned");
    // a hidden layer whose input is the activation below it, rows of round4(in_w)
    Layer y = {};
    y.in_w = in_w; y.out_w = out_w;
    y.ldw = round4(in_w);
    y.in = n.in; y.ld_in = y.ldw;
    p[i] = wgrad_product(y, n.dz, round4(out_w), M, n_splits, n.slabs_w, n.slabs_b,
                         n.slab_stride);
  }
  const GemmPairPlan plan = ga_gemm_pair_plan(p[0], p[1]);
  GA_REQUIRE(plan.taken, "ga_gemm_launch_pair: two products of one shape");
  for (GemmParams& q : p) { q.gx = plan.gx; q.gy = plan.gy; }  // (gz: wgrad_product's)
  return ga_gemm_pair_launch(plan, p[0], p[1], stream);
}

extern "C" int ga_mlp_backward_f32(const ga_mlp_desc* d, const float* params,
                                   const float* X, int64_t ldx,
                                   const int32_t* row_idx, int64_t M,
                                   const float* acts, const float* dout,
                                   int64_t ldo, float* dacts, float* grad_slabs,
                                   int64_t slab_stride, int64_t n_splits,
                                   ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(d != nullptr, "ga_mlp_backward_f32: null descriptor");
  return ga_mlp_backward_range_f32(d, params, X, ldx, row_idx, M, acts, dout, ldo, dacts,
                                   grad_slabs, slab_stride, n_splits, d->n_layers - 1, 0,
                                   stream);
}

// Layers l_start .. 0 (fused_train.h).  l_start = n_layers - 1 with `dout` is the
// whole backward pass; the fused optimizer step enters below the head with the
// data gradient of the last hidden layer already in `dacts`.
extern "C" int ga_mlp_backward_range_f32(const ga_mlp_desc* d, const float* params,
                                         const float* X, int64_t ldx,
                                         const int32_t* row_idx, int64_t M,
                                         const float* acts, const float* dout,
                                         int64_t ldo, float* dacts, float* grad_slabs,
                                         int64_t slab_stride, int64_t n_splits,
                                         int l_start, int fused_first,
                                         hipStream_t stream) {
  int rc = check_desc(d, "ga_mlp_backward_f32");
  if (rc) return rc;
  GA_REQUIRE(params && X && grad_slabs, "ga_mlp_backward_f32: null pointer");
  GA_REQUIRE(l_start >= 0 && l_start < d->n_layers &&
                 (l_start < d->n_layers - 1 || dout) && (!fused_first || l_start >= 1),
             "ga_mlp_backward_f32: bad layer range");
  GA_REQUIRE(d->n_layers == 1 || (acts && dacts),
             "ga_mlp_backward_f32: workspaces needed");
  GA_REQUIRE(M > 0 && M < (1ll << 31), "ga_mlp_backward_f32: bad M");
  GA_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0 && slab_stride % 4 == 0,
             "ga_mlp_backward_f32: strides must be multiples of 4");
  GA_REQUIRE(n_splits >= 1 && n_splits <= 1024, "ga_mlp_backward_f32: n_splits");
  GA_REQUIRE(ga_aligned16(params) && ga_aligned16(X) && (!dout || ga_aligned16(dout)) &&
                 ga_aligned16(grad_slabs) && (!acts || ga_aligned16(acts)) &&
                 (!dacts || ga_aligned16(dacts)),
             "ga_mlp_backward_f32: pointers must be 16-B aligned");
  const int kps = rows_per_split(M, n_splits);
  for (int l = l_start; l >= (fused_first ? 1 : 0); --l) {
    const Layer y = describe_layer(d, l, params, X, ldx, row_idx, acts);
    bool dgrad_done = fused_first && l == 1;
    const float* dz = y.is_last ? dout : dacts + d->act_off[l];
    const int64_t lddz = y.is_last ? ldo : round4(y.out_w);
    float* slab_w = grad_slabs + d->w_off[l];
    float* slab_b = grad_slabs + d->b_off[l];
    // ---- weight + bias gradient slabs: the streaming kernel -- for the head layer with
    // the data gradient of the layer below from the same pass over the hidden activations
    // (it needs dz and tanh' of `in` only) where the shape takes it, else without -- else
    // the tiles
    SkinnyWgradParams w =
        skinny_wgrad_product(y, dz, lddz, M, n_splits, slab_w, slab_b, slab_stride);
    const bool with_dz = y.out_w <= 32 && g_fuse_head_dgrad && l > 0 &&
                         y.in_idx == nullptr && d->hidden_act == 0 && !d->layer_norm;
    if (with_dz) {
      w.Wn = y.W; w.ldwn = y.ldw;
      w.dz_out = dacts + d->act_off[l - 1]; w.lddz = y.ldw;
    }
    SkinnyWgradPlan sp = ga_skinny_wgrad_plan(w, g_skinny != 0);
    if (!sp.taken && with_dz) {
      w.Wn = nullptr; w.ldwn = 0;
      w.dz_out = nullptr; w.lddz = 0;
      sp = ga_skinny_wgrad_plan(w, g_skinny != 0);
    }
    if (sp.taken) {
      w.qpr = sp.qpr; w.n_colblk = sp.n_colblk;
      rc = ga_skinny_wgrad_launch(sp, w, stream);
      if (rc) return rc;
      if (sp.variant == SWV_DZ) dgrad_done = true;
    } else {
      rc = launch_product(wgrad_product(y, dz, lddz, M, n_splits, slab_w, slab_b, slab_stride),
                          0, 0, (int)n_splits, stream);
      if (rc) return rc;
    }
    // ---- data gradient for the layer below
    // A normalised layer input (hidden layers with layer_norm) takes the plain
    // product dz W -- also for the first layer, whose gamma / beta need it -- and
    // the LayerNorm's backward pass then turns it, in place, into the data
    // gradient of the layer below.
    if ((l > 0 || y.norm_in) && !dgrad_done) {
      float* dst = l > 0 ? dacts + d->act_off[l - 1] : dacts + y.xn_off;
      const GemmParams p = dgrad_product(y, M, dz, lddz, dst, y.norm_in ? nullptr : y.raw,
                                         d->hidden_act);
      bool streamed;
      rc = try_skinny_forward(p, false, &streamed, stream);
      if (rc) return rc;
      if (!streamed) {
        rc = launch_product(p, 1, 0, 1, stream);
        if (rc) return rc;
      }
      if (y.norm_in) {
        rc = ga_ln_backward(dst, y.ldw, y.raw, l == 0 ? ldx : y.ldw, y.raw_idx,
                            acts + y.stats_off, M, y.in_w, params + y.gamma_off,
                            l > 0 ? 1 : 0, d->hidden_act, kps, (int)n_splits,
                            grad_slabs + y.gamma_off, grad_slabs + y.beta_off, slab_stride,
                            stream);
        if (rc) return rc;
      }
    }
  }
  return GA_OK;
}

// Tangent (forward-mode) pass: with dtheta = `tangent` (flat parameter layout) and
// the activations of a forward at the same rows in `acts`,
//   tz_l = in_l dW_l^T + db_l + tin_l W_l^T,   th_l = tz_l * (1 - h_l^2)
// (in_0 = X, tin_0 = 0); `tout` receives d(output).  This is the J v half of the
// Fisher-vector product the TRPO policy step solves with
// (torch/optimizers/conjugate_gradient_optimizer.py:18-66 takes the same product
// by double backward through the KL constraint).
extern "C" int ga_mlp_jvp_f32(const ga_mlp_desc* d, const float* params,
                              const float* tangent, const float* X, int64_t ldx,
                              const int32_t* row_idx, int64_t M, const float* acts,
                              float* tacts, float* tout, int64_t ldo,
                              ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_desc(d, "ga_mlp_jvp_f32");
  if (rc) return rc;
  GA_REQUIRE(params && tangent && X && tout, "ga_mlp_jvp_f32: null pointer");
  GA_REQUIRE(d->n_layers == 1 || (acts && tacts), "ga_mlp_jvp_f32: workspaces needed");
  GA_REQUIRE(M > 0 && M < (1ll << 31), "ga_mlp_jvp_f32: bad M");
  GA_REQUIRE(ldx % 4 == 0 && ldx >= d->dims[0] && ldo >= d->dims[d->n_layers],
             "ga_mlp_jvp_f32: leading dimensions");
  GA_REQUIRE(ga_aligned16(params) && ga_aligned16(tangent) && ga_aligned16(X) &&
                 (!acts || ga_aligned16(acts)) && (!tacts || ga_aligned16(tacts)),
             "ga_mlp_jvp_f32: pointers must be 16-B aligned");
  const int L = d->n_layers;
  for (int l = 0; l < L; ++l) {
    // the layer over the tangent vector and the activations, and over the parameters
    // and the tangent activations (no tangent comes in through X)
    const Layer t = describe_layer(d, l, tangent, X, ldx, row_idx, acts);
    const Layer w = describe_layer(d, l, params, nullptr, 0, nullptr, tacts);
    float* C = t.is_last ? tout : tacts + d->act_off[l];
    const int64_t ldc = t.is_last ? ldo : round4(t.out_w);
    const float* H = t.is_last ? nullptr : acts + d->act_off[l];
    // a normalised layer input: its tangent (through the LayerNorm, from the
    // tangent of the layer below and of gamma / beta) is a second product even
    // for the first layer
    if (t.norm_in) {
      rc = ga_ln_jvp(w.raw, t.ldw, t.raw, t.ld_raw, t.raw_idx, acts + t.stats_off, M,
                     t.in_w, params + t.gamma_off, tangent + t.gamma_off,
                     tangent + t.beta_off, tacts + t.xn_off, t.ldw, stream);
      if (rc) return rc;
    }
    const bool two = l > 0 || t.norm_in;
    // in_l dW_l^T + db_l  (and the tanh' factor when it is the only product)
    const GemmParams p = tangent_weight_product(t, M, C, ldc, !two, H, d->hidden_act);
    rc = launch_product(p, 1, 1, 1, stream);
    if (rc) return rc;
    if (two) {
      // += tin_l W_l^T, then the tanh' factor
      const GemmParams q = tangent_input_product(w, M, C, ldc, H, d->hidden_act);
      rc = launch_product(q, 1, 1, 1, stream);
      if (rc) return rc;
    }
  }
  return GA_OK;
}

// Plain GEMM entry used by tests: C[M,N] = A[M,K] * B[N,K]^T (both k-contiguous).
extern "C" int ga_gemm_nt_f32(const float* A, int64_t lda, const float* B,
                              int64_t ldb, float* C, int64_t ldc, int64_t M,
                              int64_t N, int64_t K, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(A && B && C, "ga_gemm_nt_f32: null pointer");
  GA_REQUIRE(lda % 4 == 0 && ldb % 4 == 0 && ga_aligned16(A) && ga_aligned16(B),
             "ga_gemm_nt_f32: operands must be 16-B aligned with ld %% 4 == 0");
  GemmParams p = {};
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.c_rs = ldc; p.c_cs = 1;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.epi = EPI_PLAIN;
  p.k_per_split = full_k(p.K);
  return launch_product(p, 1, 1, 1, stream);
}
