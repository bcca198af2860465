// The fake kernel side of garage_amd/csrc/update.cpp: every entry point the epoch loops
// call, defined once.  Each fake records one Event -- the text line (also appended to
// g_log), the launch's name, stream and network count, and copies of the descriptors the
// suites look into -- and touches the memory its kernel would, so that an extent that is
// off trips AddressSanitizer whichever suite runs.  Include once per program, after
// harness.h.
#pragma once
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/shape_rules.h"
#include "../../garage_amd/csrc/small_step.h"
#include "harness.h"

// ---- switches; a suite sets each one it depends on at entry -----------------------------
// ga_small_step_supported answers by the kernel's rule (default) or 0
static bool g_small_step_answers = true;
// ga_fused_fwd_dgrad_supported answers by the kernel's rule (default) or 0 ...
static bool g_fwd_dgrad_answers = true;
// ... and a ga_fused_fwd_dgrad launch while it answers 0 aborts (default) or is recorded
static bool g_fwd_dgrad_unasked_aborts = true;
// floats behind a->params and behind a->xh2 / a->xdz of the pass under test: ga_small_step
// compares the largest offsets its kernel reaches with them (0, the default: not compared)
static int64_t g_ss_n_flat = 0, g_ss_ws_floats = 0;
static int g_ss_extent_errors = 0;

// ---- what the fakes saw, in launch order ------------------------------------------------
struct ReduceSeen {
  uint32_t presummed;
  std::vector<ga_fused_region> regions;
};
struct Event {
  std::string what;  // the launch's name
  std::string line;  // its text line
  void* stream;
  int n_nets;
  bool ends_in_wgrad;  // its last kernel is the middle layer's weight-gradient GEMM
  bool after_wgrad;    // the launch before it was such a one, on the same stream
  ga_fused_dgrad_net dgrad[2];  // "dgrad": one descriptor per network
  ReduceSeen reduce[2];         // "reduce": likewise
};
static std::vector<Event> g_events;

static void clear_log() {
  g_log.clear();
  g_events.clear();
}
static Event& launched(const char* what, void* stream, int n_nets, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log.push_back(buf);
  Event e = {};
  e.what = what; e.line = buf; e.stream = stream; e.n_nets = n_nets;
  e.after_wgrad =
      !g_events.empty() && g_events.back().ends_in_wgrad && g_events.back().stream == stream;
  g_events.push_back(e);
  return g_events.back();
}
static std::vector<const Event*> events_of(const char* what) {
  std::vector<const Event*> out;
  for (const Event& e : g_events)
    if (e.what == what) out.push_back(&e);
  return out;
}

// ---- what the kernels touch ---------------------------------------------------------------
// every tile's loss sums and head shares of a forward + loss launch
static void touch_fwd_tiles(const ga_fused_fwd_net& n, int64_t M, int width) {
  for (int64_t t = 0; t < ga_fused_tiles(M); ++t) {
    n.lpart[2 * t] = n.lpart[2 * t + 1] = 0.0;
    memset(n.hpart + t * (8 * (int64_t)width + 8), 0, sizeof(float) * (8 * width + 8));
  }
}
// every tile's first-layer shares of a data-gradient launch
static void touch_wpart_tiles(const ga_fused_dgrad_net& n, int64_t M, int width, int in_w) {
  const int64_t stride = width * (int64_t)((in_w + 3) & ~3) + width;
  for (int64_t t = 0; t < ga_fused_tiles(M); ++t)
    memset(n.wpart + t * stride, 0, sizeof(float) * stride);
}
// every split's slab of the middle layer
static void touch_mid_slabs(float* slabs_w, float* slabs_b, int64_t stride, int64_t splits,
                            int64_t out_w, int64_t in_w) {
  for (int64_t k = 0; k < splits; ++k) {
    memset(slabs_w + k * stride, 0, sizeof(float) * (size_t)(out_w * in_w));
    memset(slabs_b + k * stride, 0, sizeof(float) * (size_t)out_w);
  }
}

extern "C" {
int ga_mlp_forward_f32(const ga_mlp_desc* d, const float*, const float*, int64_t,
                       const int32_t* idx, int64_t M, float*, float* out, int64_t,
                       ga_stream_t s) {
  launched("fwd", s, 1, "fwd M=%lld idx0=%d layers=%d out=%d stream=%p", (long long)M,
           idx ? idx[0] : -1, d->n_layers, out != nullptr, s);
  if (idx) {  // touch every id of the minibatch: out-of-range slices trip ASAN
    long long sum = 0;
    for (int64_t i = 0; i < M; ++i) sum += idx[i];
    logf("idxsum %lld", sum);
  }
  return 0;
}
int ga_ppo_gaussian_loss_f32(const float*, int64_t, const float*, int64_t, const float*,
                             const float*, const int32_t*, const float*, int, float, int,
                             float, int64_t M, int A, int algo, float, float, int, float*,
                             float*, float* loss_out, float*, int64_t, int64_t splits,
                             double*, ga_stream_t s) {
  launched("ppo_loss", s, 1, "ppo_loss M=%lld A=%d algo=%d splits=%lld", (long long)M, A,
           algo, (long long)splits);
  if (loss_out) *loss_out = (float)M;
  return 0;
}
int ga_ppo_categorical_loss_f32(const float*, int64_t, const float*, int64_t, const float*,
                                const float*, const int32_t*, int64_t M, int, int, int,
                                float, float, int, float*, float*, float*, float*, double*,
                                float*, int64_t, int64_t, double*, ga_stream_t s) {
  launched("cat_loss", s, 1, "cat_loss M=%lld", (long long)M);
  return 0;
}
int ga_gaussian_nll_loss_f32(const float*, int64_t, const float*, const int32_t*,
                             const float*, int64_t M, float*, float*, float*, int64_t,
                             int64_t, double*, ga_stream_t s) {
  launched("nll_loss", s, 1, "nll_loss M=%lld", (long long)M);
  return 0;
}
int ga_head_loss_supported(int, int) { return 0; }
int ga_head_ppo_gaussian_loss_f32(const float*, int64_t, const float*, int64_t,
                                  const float*, int, float*, int64_t, const float*, int64_t,
                                  const float*, const float*, const int32_t*, const float*,
                                  int, float, int, float, int64_t M, int, int, float, float,
                                  int, float*, int64_t, float*, float*, float*, int64_t,
                                  int64_t, double*, ga_stream_t s) {
  launched("head_ppo_loss", s, 1, "head_ppo_loss M=%lld", (long long)M);
  return 0;
}
int ga_head_gaussian_nll_loss_f32(const float*, int64_t, const float*, const float*, int,
                                  float*, int64_t, const float*, const int32_t*,
                                  const float*, int64_t M, float*, int64_t, float*, float*,
                                  int64_t, int64_t, double*, ga_stream_t s) {
  launched("head_nll_loss", s, 1, "head_nll_loss M=%lld", (long long)M);
  return 0;
}
int64_t ga_mlp_backward_splits(const ga_mlp_desc*, int64_t M) { return (M + 255) / 256; }
int ga_mlp_backward_f32(const ga_mlp_desc*, const float*, const float*, int64_t,
                        const int32_t*, int64_t M, const float*, const float*, int64_t,
                        float*, float*, int64_t, int64_t splits, ga_stream_t s) {
  launched("bwd", s, 1, "bwd M=%lld splits=%lld", (long long)M, (long long)splits);
  return 0;
}
// The middle layers' backward GEMMs.  With fused_first the LAST launch it makes is layer
// 1's weight gradient, which writes every partial of that layer; with two hidden layers
// it is the only one ("wgrad").
int ga_mlp_backward_range_f32(const ga_mlp_desc* d, const float*, const float*, int64_t,
                              const int32_t*, int64_t M, const float*, const float*,
                              int64_t, float*, float* slabs, int64_t n_flat, int64_t splits,
                              int l_start, int fused_first, hipStream_t s) {
  Event& e = launched(fused_first && d->n_layers == 3 ? "wgrad" : "bwd_range", s, 1,
                      "bwd_range M=%lld l_start=%d fused_first=%d", (long long)M, l_start,
                      fused_first);
  e.ends_in_wgrad = fused_first != 0;
  if (fused_first)
    touch_mid_slabs(slabs + d->w_off[1], slabs + d->b_off[1], n_flat, splits, d->dims[2],
                    (d->dims[1] + 3) & ~3);
  return 0;
}
int ga_reduce_adam_f32(const float*, int64_t splits, int64_t, float*, float*, float*,
                       float*, int64_t, int64_t step, double, double, double, double,
                       int zero0, ga_stream_t s) {
  launched("reduce_adam", s, 1, "reduce_adam splits=%lld step=%lld zero0=%d",
           (long long)splits, (long long)step, zero0);
  return 0;
}
int ga_reduce_slabs_f32(const float*, int64_t splits, int64_t, int64_t, float scale,
                        float*, ga_stream_t s) {
  launched("reduce_slabs", s, 1, "reduce_slabs splits=%lld scale=%.4f", (long long)splits,
           scale);
  return 0;
}
int ga_adam_step_f32(float*, const float*, float*, float*, int64_t, int64_t step, double,
                     double, double, double, ga_stream_t s) {
  launched("adam", s, 1, "adam step=%lld", (long long)step);
  return 0;
}
int64_t ga_reduction_partials_doubles(void) { return 1024; }
int ga_small_step_supported(int n_layers, const int* dims, int64_t M) {
  return g_small_step_answers && ga_small_step_rule(n_layers, dims, M);
}
int ga_small_step_resident(int, int) { return 1; }
int ga_small_step(const ga_small_step_args* a, void* s) {
  launched("small_step", s, 1, "small_step M=%d step=%lld", a->M, (long long)a->step);
  // the largest offsets small_step_kernel's index formulas reach (small_step.hip),
  // last workgroup (c0 = H - 16), idle waves included -- their prefetches are
  // clamped to the layer's last tile, which is what this arithmetic restates
  const int64_t H = a->H, ld0 = (a->in_w + 3) & ~3, A = a->out_w;
  const int64_t c0 = H - 16;
  int64_t reach[8];
  reach[0] = a->w_off[0] + H * ld0 - 1;                              // W1 staging
  reach[1] = a->w_off[1] + (H - 1) * H + c0 + 15;                    // W2 columns
  reach[2] = a->w_off[1] + (c0 + 15) * H + H - 1;                    // W2 own rows
  reach[3] = a->w_off[1] + (c0 + 15) * H + 32 * (H / 32 - 1) + 31;   // Adam prefetch
  reach[4] = a->w_off[2] + (A - 1) * H + c0 + 15;                    // head columns
  reach[5] = a->b_off[0] + H - 1;
  reach[6] = a->b_off[1] + c0 + 15;
  reach[7] = a->b_off[2] + A - 1;
  if (g_ss_n_flat > 0) {
    for (int i = 0; i < 8; ++i)
      if (reach[i] >= g_ss_n_flat) ++g_ss_extent_errors;
    if ((H / 16) * 64 * 8 > g_ss_ws_floats || 64 * H > g_ss_ws_floats)
      ++g_ss_extent_errors;
  }
  // the two exchanges: head shares [H / 16][64][8], dZ2 [64][H] -- written here
  // so that AddressSanitizer sees the extents
  memset(a->xh2, 0, sizeof(float) * (size_t)((H / 16) * 64 * 8));
  memset(a->xdz, 0, sizeof(float) * (size_t)(64 * H));
  // and the optimizer state at the largest index
  a->params[reach[3]] = a->exp_avg[reach[3]] = a->exp_avg_sq[reach[3]] = 0.f;
  return 0;
}
int ga_act_slope_mul_f32(float*, int64_t, const float*, int64_t, int64_t M, int N, int act,
                         void* s) {
  launched("act_slope_mul", s, 1, "act_slope_mul M=%lld N=%d act=%d", (long long)M, N, act);
  return 0;
}
// ---- the launches of a fused step.  One network: the single launch's line; two networks
// (one grid): the pair_* line.  Either way the fakes touch the same extents for every
// network.
int ga_fused_fwd_head_loss(const ga_fused_fwd_net* n, int n_nets, int64_t M, int width,
                           int K, hipStream_t s) {
  if (n_nets == 1)
    launched("fused_fwd", s, 1, "fused_fwd M=%lld width=%d K=%d a_idx=%d A=%d first=%d",
             (long long)M, width, K, n->a_idx != nullptr, n->loss->A, n->first != nullptr);
  else
    launched("fused_fwd", s, n_nets,
             "pair_fwd stream=%p M=%lld width=%d K=%d A=%d/%d in=%d/%d", (void*)s,
             (long long)M, width, K, n[0].loss->A, n[1].loss->A, n[0].first->in_w,
             n[1].first->in_w);
  for (int i = 0; i < n_nets; ++i) touch_fwd_tiles(n[i], M, width);
  return 0;
}
int ga_fused_fwd_dgrad_supported(int width, int K, int in_w) {
  return g_fwd_dgrad_answers && ga_fused_fwd_dgrad_rule(width, K, in_w);
}
int ga_fused_fwd_dgrad(const ga_fused_fwd_net* f, const ga_fused_dgrad_net* g, int64_t M,
                       int width, int K, hipStream_t s) {
  if (!g_fwd_dgrad_answers && g_fwd_dgrad_unasked_aborts) {
    fprintf(stderr, "ga_fused_fwd_dgrad launched although it is not supported\n");
    abort();
  }
  launched("fwd_dgrad", s, 1, "fwd_dgrad M=%lld width=%d K=%d", (long long)M, width, K);
  // what the launch requires of its two descriptors
  CHECK(f && g && f->first && f->loss);
  if (f && g && f->first && f->loss) {
    CHECK(ga_fused_fwd_dgrad_rule(width, K, f->first->in_w));
    CHECK(g->dZ2 == f->dZ && g->lddz == f->lddz);
    CHECK(g->H1 == f->first->H && g->ldh == f->first->ldh);
    CHECK(g->X == f->first->X && g->ldx == f->first->ldx && g->idx == f->loss->idx);
    CHECK(g->W2 == f->W && g->ldw == f->ldw);
    CHECK(g->wpart != nullptr);
    CHECK(!g->sum_w.src && !g->sum_w.n && !g->sum_w.n_part);
    CHECK(!g->sum_b.src && !g->sum_b.n && !g->sum_b.n_part);
    touch_fwd_tiles(*f, M, width);
    if (g->wpart) touch_wpart_tiles(*g, M, K, f->first->in_w);
  }
  return 0;
}
int ga_wgrad_mid(const ga_wgrad_mid_net* n, int n_nets, int64_t M, int64_t n_splits,
                 int out_w, int in_w, hipStream_t s) {
  Event& e = launched("wgrad", s, n_nets, "pair_wgrad stream=%p M=%lld splits=%lld out=%d in=%d",
                      (void*)s, (long long)M, (long long)n_splits, out_w, in_w);
  e.ends_in_wgrad = true;
  for (int i = 0; i < n_nets; ++i)
    touch_mid_slabs(n[i].slabs_w, n[i].slabs_b, n[i].slab_stride, n_splits, out_w, in_w);
  return 0;
}
int ga_fused_dgrad_wgrad0(const ga_fused_dgrad_net* n, int n_nets, int64_t M, int width,
                          int K, int in_w, hipStream_t s) {
  Event* e;
  if (n_nets == 1)
    e = &launched("dgrad", s, 1, "fused_dgrad M=%lld width=%d K=%d in=%d", (long long)M,
                  width, K, in_w);
  else
    e = &launched("dgrad", s, n_nets, "pair_dgrad stream=%p M=%lld width=%d K=%d in=%d",
                  (void*)s, (long long)M, width, K, in_w);
  for (int i = 0; i < n_nets; ++i) {
    e->dgrad[i] = n[i];
    touch_wpart_tiles(n[i], M, width, in_w);
    // what the kernel does with a range: reads every partial of every element and
    // writes partial 0
    const ga_slab_range* r[2] = {&n[i].sum_w, &n[i].sum_b};
    for (int j = 0; j < 2; ++j) {
      if (!r[j]->src) continue;
      for (int64_t el = 0; el < r[j]->n; ++el) {
        float sum = 0.f;
        for (int k = 0; k < r[j]->n_part; ++k) sum += r[j]->src[k * r[j]->stride + el];
        r[j]->src[el] = sum;
      }
    }
  }
  return 0;
}
int ga_reduce_regions_adam(const ga_reduce_net* n, int n_nets, hipStream_t s) {
  Event* e;
  if (n_nets == 1) {
    e = &launched("reduce", s, 1,
                  "reduce_regions n=%d step=%lld scale=%.4f adam=%d zero0=%d lparts=%d M=%lld",
                  n->n_regions, (long long)n->step, n->scale, n->do_adam, n->zero_slot0,
                  n->n_lpart, (long long)n->M);
    for (int k = 0; k < n->n_regions; ++k)
      logf("  region beg=%lld n=%lld parts=%d stride=%lld", (long long)n->regions[k].beg,
           (long long)n->regions[k].n, n->regions[k].n_part, (long long)n->regions[k].stride);
  } else {
    e = &launched("reduce", s, n_nets,
                  "pair_reduce stream=%p steps=%lld/%lld regions=%d/%d adam=%d/%d M=%lld",
                  (void*)s, (long long)n[0].step, (long long)n[1].step, n[0].n_regions,
                  n[1].n_regions, n[0].do_adam, n[1].do_adam, (long long)n[0].M);
  }
  for (int i = 0; i < n_nets; ++i) {
    ReduceSeen& c = e->reduce[i];
    c.presummed = n[i].presummed;
    c.regions.assign(n[i].regions, n[i].regions + n[i].n_regions);
    // what the kernel does with a region: reads every partial (of a pre-summed one,
    // partial 0 only; the others are memory of the same workspace)
    for (const ga_fused_region& r : c.regions) {
      float sum = 0.f;
      for (int k = 0; k < r.n_part; ++k)
        for (int64_t el = 0; el < r.n; ++el) sum += r.src[k * r.stride + el];
      CHECK(sum == sum);
    }
    if (n[i].loss_out) *n[i].loss_out = 1.f;
  }
  return 0;
}
int ga_split_bf16_any(void) { return 0; }
void ga_planes_epoch_begin(void) {}
int ga_narrow_train_step(const float*, const int64_t*, const int64_t*, int in_w, int H,
                         int out_w, const float*, int64_t, int64_t M,
                         const ga_fused_loss_args*, float* part, double* lpart,
                         hipStream_t s) {
  launched("narrow", s, 1, "narrow M=%lld in=%d H=%d out=%d", (long long)M, in_w, H, out_w);
  const int64_t stride = ga_narrow_step_stride(in_w, H);
  for (int64_t t = 0; t < ga_fused_tiles(M); ++t) {
    lpart[2 * t] = lpart[2 * t + 1] = 0.0;
    memset(part + t * stride, 0, sizeof(float) * stride);
  }
  return 0;
}
}  // extern "C"

// ---- a pass's buffers ---------------------------------------------------------------------
// A tanh MLP of hidden widths h with every buffer at the size the Python side gives it
// for a pass over S samples in minibatches of up to `rows` rows: the slab workspace is
// EXACTLY splits * n_flat floats, the scratch exactly ga_update_partials_floats, the
// activation workspaces rows x the hidden widths, the permutation S ids (the identity;
// a suite may rewrite it).
struct Net {
  ga_mlp_desc d;
  std::vector<float> params, m1, m2, grads, acts, dacts, slabs, partials, scratch;
  std::vector<double> ws;
  std::vector<int32_t> perm;
  int64_t splits;
  Net(int in, std::vector<int> h, int out, int64_t S, int64_t rows) {
    memset(&d, 0, sizeof(d));
    const int L = (int)h.size() + 1;
    d.n_layers = L;
    d.dims[0] = in;
    for (int l = 0; l + 1 < L; ++l) d.dims[l + 1] = h[(size_t)l];
    d.dims[L] = out;
    int64_t off = 4, act = 0;
    for (int l = 0; l < L; ++l) {
      d.w_off[l] = off; off += (int64_t)d.dims[l + 1] * ((d.dims[l] + 3) & ~3);
      d.b_off[l] = off; off += (d.dims[l + 1] + 3) & ~3;
      if (l + 1 < L) { d.act_off[l] = act; act += rows * ((d.dims[l + 1] + 3) & ~3); }
    }
    params.assign((size_t)off, 0.f); m1 = m2 = grads = params;
    acts.assign((size_t)act, 0.f); dacts = acts;
    splits = ga_mlp_backward_splits(&d, rows);
    slabs.assign((size_t)(splits * off), 1.f);
    const int64_t need = ga_update_partials_floats(&d, rows);
    partials.assign((size_t)(need > 0 ? need : 1), 0.f);
    scratch.assign(16, 0.f);
    ws.assign(2048, 0.0);
    perm.resize((size_t)S);
    for (int64_t i = 0; i < S; ++i) perm[(size_t)i] = (int32_t)i;
  }
  ga_update_args args(int64_t S, int64_t mb, int kind) {
    ga_update_args a;
    memset(&a, 0, sizeof(a));
    a.desc = &d; a.params = params.data(); a.grads = grads.data();
    a.exp_avg = m1.data(); a.exp_avg_sq = m2.data(); a.n_flat = (int64_t)params.size();
    a.acts = acts.data(); a.dacts = dacts.data(); a.out = a.dout = acts.data(); a.ldo = 8;
    a.slabs = slabs.data(); a.max_splits = splits;
    a.lr = 1e-3; a.beta1 = 0.9; a.beta2 = 0.999; a.eps = 1e-8; a.learn_std = 1;
    a.X = params.data(); a.ldx = (d.dims[0] + 3) & ~3; a.S = S; a.perm = perm.data();
    a.mb = mb; a.kind = kind; a.actions = params.data(); a.lda = 4;
    a.old_ll = a.adv = a.returns = params.data();
    a.loss_scratch = scratch.data(); a.workspace = ws.data();
    const int64_t need = ga_update_partials_floats(&d, mb > 0 && mb < S ? mb : S);
    a.partials = need > 0 ? partials.data() : nullptr;
    a.partials_floats = need;
    return a;
  }
};
