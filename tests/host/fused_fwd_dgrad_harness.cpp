// Host-logic harness for the fused forward + data-gradient launch of a fused optimizer
// step (garage_amd/csrc/update.cpp: fused_step / run_minibatch_fused;
// ga_set_fused_fwd_dgrad), built with -fsanitize=address,undefined on the CPU
// (`make asan-fwd-dgrad`).  Every launch the epoch loops make is a fake that appends to
// one log; here the kernel side HAS the fused instantiation (the other harnesses link
// no_fused_fwd_dgrad.cpp instead).  Checked: a step that qualifies is exactly
//   fused forward + data gradient -> middle-layer weight gradient -> optimizer launch
// on one stream, the fused launch gets two descriptors of ONE step and no slab ranges,
// the optimizer launch gets no pre-summed region and the middle layer's regions as
// `splits` partials inside the slab workspace; and today's four-launch sequence comes
// back with the switch off, with two networks per launch (the merged pair schedule),
// with one or three hidden layers, and at shapes the kernel side declines.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/garage_amd.h"
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/small_step.h"

static std::string g_error;
void ga_set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}

static int g_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

// what the fakes saw, in launch order
struct Launch {
  std::string what;
  void* stream;
  int n_nets;
};
struct ReduceCall {
  uint32_t presummed;
  std::vector<ga_fused_region> regions;
};
static std::vector<Launch> g_log;
static std::vector<ReduceCall> g_reduce;
static std::vector<ga_fused_dgrad_net> g_dgrad;  // descriptors of the two-launch path
static void launched(const char* what, void* stream, int n_nets = 1) {
  g_log.push_back(Launch{what, stream, n_nets});
}

extern "C" {
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  static char slots[8];
  static int next = 0;
  *e = (hipEvent_t)&slots[next++ % 8];
  return hipSuccess;
}
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

int ga_mlp_forward_f32(const ga_mlp_desc*, const float*, const float*, int64_t,
                       const int32_t*, int64_t, float*, float*, int64_t, ga_stream_t s) {
  launched("fwd", s);
  return 0;
}
int ga_ppo_gaussian_loss_f32(const float*, int64_t, const float*, int64_t, const float*,
                             const float*, const int32_t*, const float*, int, float, int,
                             float, int64_t, int, int, float, float, int, float*, float*,
                             float*, float*, int64_t, int64_t, double*, ga_stream_t) {
  return 0;
}
int ga_ppo_categorical_loss_f32(const float*, int64_t, const float*, int64_t, const float*,
                                const float*, const int32_t*, int64_t, int, int, int, float,
                                float, int, float*, float*, float*, float*, double*, float*,
                                int64_t, int64_t, double*, ga_stream_t) {
  return 0;
}
int ga_gaussian_nll_loss_f32(const float*, int64_t, const float*, const int32_t*,
                             const float*, int64_t, float*, float*, float*, int64_t, int64_t,
                             double*, ga_stream_t) {
  return 0;
}
int ga_head_loss_supported(int, int) { return 0; }
int ga_head_ppo_gaussian_loss_f32(const float*, int64_t, const float*, int64_t,
                                  const float*, int, float*, int64_t, const float*, int64_t,
                                  const float*, const float*, const int32_t*, const float*,
                                  int, float, int, float, int64_t, int, int, float, float,
                                  int, float*, int64_t, float*, float*, float*, int64_t,
                                  int64_t, double*, ga_stream_t) {
  return 0;
}
int ga_head_gaussian_nll_loss_f32(const float*, int64_t, const float*, const float*, int,
                                  float*, int64_t, const float*, const int32_t*,
                                  const float*, int64_t, float*, int64_t, float*, float*,
                                  int64_t, int64_t, double*, ga_stream_t) {
  return 0;
}
int64_t ga_mlp_backward_splits(const ga_mlp_desc*, int64_t M) { return (M + 255) / 256; }
int ga_mlp_backward_f32(const ga_mlp_desc*, const float*, const float*, int64_t,
                        const int32_t*, int64_t, const float*, const float*, int64_t, float*,
                        float*, int64_t, int64_t, ga_stream_t s) {
  launched("bwd", s);
  return 0;
}
// the middle layers' backward GEMMs; with fused_first and two hidden layers it is ONE
// launch, layer 1's weight gradient, and it writes every partial of that layer
int ga_mlp_backward_range_f32(const ga_mlp_desc* d, const float*, const float*, int64_t,
                              const int32_t*, int64_t, const float*, const float*, int64_t,
                              float*, float* slabs, int64_t n_flat, int64_t splits, int,
                              int fused_first, hipStream_t s) {
  if (fused_first)
    for (int64_t k = 0; k < splits; ++k) {
      memset(slabs + k * n_flat + d->w_off[1], 0,
             sizeof(float) * (size_t)d->dims[2] * ((d->dims[1] + 3) & ~3));
      memset(slabs + k * n_flat + d->b_off[1], 0, sizeof(float) * (size_t)d->dims[2]);
    }
  launched(fused_first && d->n_layers == 3 ? "wgrad" : "bwd_range", s);
  return 0;
}
int ga_reduce_adam_f32(const float*, int64_t, int64_t, float*, float*, float*, float*,
                       int64_t, int64_t, double, double, double, double, int, ga_stream_t) {
  return 0;
}
int ga_reduce_slabs_f32(const float*, int64_t, int64_t, int64_t, float, float*,
                        ga_stream_t) {
  return 0;
}
int ga_adam_step_f32(float*, const float*, float*, float*, int64_t, int64_t, double, double,
                     double, double, ga_stream_t) {
  return 0;
}
int64_t ga_reduction_partials_doubles(void) { return 1024; }
int ga_small_step_supported(int, const int*, int64_t) { return 0; }
int ga_small_step_resident(int, int) { return 1; }
int ga_small_step(const ga_small_step_args*, void*) { return 0; }
int ga_act_slope_mul_f32(float*, int64_t, const float*, int64_t, int64_t, int, int, void*) {
  return 0;
}
int ga_fused_width_ok(int w) { return w == 64 || w == 128 || w == 256; }
int ga_fused_first_layer_ok(int in_w, int K) {
  return in_w >= 1 && in_w <= 32 && K % 32 == 0 && K * ((in_w + 3) & ~3) <= 5120;
}
int64_t ga_fused_tiles(int64_t M) { return (M + 63) / 64; }
int ga_fused_fwd_head_loss(const ga_fused_fwd_net*, int n_nets, int64_t, int, int,
                           hipStream_t s) {
  launched("fused_fwd", s, n_nets);
  return 0;
}
// the kernel side's answer (fused_train.hip)
int ga_fused_fwd_dgrad_supported(int width, int K, int in_w) {
  return ga_fused_width_ok(width) && K == width && ga_fused_first_layer_ok(in_w, K);
}
int ga_fused_fwd_dgrad(const ga_fused_fwd_net* f, const ga_fused_dgrad_net* g, int64_t,
                       int width, int K, hipStream_t s) {
  // what the launch requires of its two descriptors
  CHECK(f && g && f->first && f->loss);
  if (f && g && f->first && f->loss) {
    CHECK(ga_fused_fwd_dgrad_supported(width, K, f->first->in_w));
    CHECK(g->dZ2 == f->dZ && g->lddz == f->lddz);
    CHECK(g->H1 == f->first->H && g->ldh == f->first->ldh);
    CHECK(g->X == f->first->X && g->ldx == f->first->ldx && g->idx == f->loss->idx);
    CHECK(g->W2 == f->W && g->ldw == f->ldw);
    CHECK(g->wpart != nullptr);
    CHECK(!g->sum_w.src && !g->sum_w.n && !g->sum_w.n_part);
    CHECK(!g->sum_b.src && !g->sum_b.n && !g->sum_b.n_part);
  }
  launched("fwd_dgrad", s);
  return 0;
}
int ga_wgrad_mid(const ga_wgrad_mid_net* n, int n_nets, int64_t, int64_t n_splits, int out_w,
                 int in_w, hipStream_t s) {
  for (int i = 0; i < n_nets; ++i)
    for (int64_t k = 0; k < n_splits; ++k) {
      memset(n[i].slabs_w + k * n[i].slab_stride, 0, sizeof(float) * (size_t)out_w * in_w);
      memset(n[i].slabs_b + k * n[i].slab_stride, 0, sizeof(float) * (size_t)out_w);
    }
  launched("wgrad", s, n_nets);
  return 0;
}
int ga_fused_dgrad_wgrad0(const ga_fused_dgrad_net* n, int n_nets, int64_t, int, int, int,
                          hipStream_t s) {
  for (int i = 0; i < n_nets; ++i) g_dgrad.push_back(n[i]);
  launched("dgrad", s, n_nets);
  return 0;
}
int ga_reduce_regions_adam(const ga_reduce_net* n, int n_nets, hipStream_t s) {
  for (int i = 0; i < n_nets; ++i) {
    ReduceCall c;
    c.presummed = n[i].presummed;
    c.regions.assign(n[i].regions, n[i].regions + n[i].n_regions);
    // what the kernel does with a region that is not pre-summed: reads every partial
    for (const ga_fused_region& r : c.regions) {
      float sum = 0.f;
      for (int k = 0; k < r.n_part; ++k)
        for (int64_t e = 0; e < r.n; ++e) sum += r.src[k * r.stride + e];
      if (sum != sum) ++g_failed;
    }
    g_reduce.push_back(c);
    if (n[i].loss_out) *n[i].loss_out = 1.f;
  }
  launched("reduce", s, n_nets);
  return 0;
}
int ga_split_bf16_any(void) { return 0; }
void ga_planes_epoch_begin(void) {}
int ga_fused_pair_supported(int width, int K, int in_w) {
  return width == 256 && K <= 256 && ga_fused_first_layer_ok(in_w, K);
}
int ga_narrow_step_supported(int n_layers, const int* dims) {
  return n_layers == 3 && dims[1] == dims[2] && (dims[1] == 32 || dims[1] == 64) &&
         dims[0] <= 32 && dims[3] <= 8;
}
int64_t ga_narrow_step_stride(int in_w, int H) {
  const int64_t ld0 = (in_w + 3) & ~3;
  return (int64_t)H * ld0 + H + (int64_t)H * H + H + 8 * (int64_t)H + 8;
}
int ga_narrow_train_step(const float*, const int64_t*, const int64_t*, int, int, int,
                         const float*, int64_t, int64_t, const ga_fused_loss_args*, float*,
                         double*, hipStream_t s) {
  launched("narrow", s);
  return 0;
}
}  // extern "C"

// a tanh MLP of hidden widths h[0 .. nh) with every buffer at the size the Python side
// gives it for minibatches of up to `rows` rows
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
    slabs.assign((size_t)(splits * off), 1.f);  // EXACTLY splits * n_flat
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
    a.partials = partials.data();
    a.partials_floats = ga_update_partials_floats(&d, mb < S ? mb : S);
    return a;
  }
};

static void clear_log() {
  g_log.clear();
  g_reduce.clear();
  g_dgrad.clear();
}

// launches [at, at + names.size()) of the log are `names`, all on `stream`
static bool log_is(size_t at, const std::vector<const char*>& names, void* stream) {
  if (at + names.size() > g_log.size()) return false;
  for (size_t i = 0; i < names.size(); ++i)
    if (g_log[at + i].what != names[i] || g_log[at + i].stream != stream ||
        g_log[at + i].n_nets != 1)
      return false;
  return true;
}

// the middle layer's regions (2: weights, 3: bias) of an optimizer launch: `splits`
// partials inside the slab workspace, nothing pre-summed
static void check_mid_regions(const ReduceCall& r, Net& n, int64_t M) {
  CHECK(r.presummed == 0u);
  CHECK(r.regions.size() == 2 * (size_t)n.d.n_layers);
  if (r.regions.size() < 4) return;
  const int64_t n_flat = (int64_t)n.params.size();
  const int64_t splits = ga_mlp_backward_splits(&n.d, M);
  const float* slabs = n.slabs.data();
  CHECK(r.regions[2].src == slabs + n.d.w_off[1] && r.regions[3].src == slabs + n.d.b_off[1]);
  for (int i = 2; i < 4; ++i) {
    const ga_fused_region& g = r.regions[(size_t)i];
    CHECK(g.n_part == (int)splits && g.stride == n_flat);
    CHECK(g.src >= slabs && g.src + (g.n_part - 1) * g.stride + g.n <= slabs + splits * n_flat);
  }
}

int main() {
  extern int ga_set_merged_pair(int on);
  void* const st = (void*)0x10;
  const std::vector<const char*> fused_seq = {"fwd_dgrad", "wgrad", "reduce"};
  const std::vector<const char*> old_seq = {"fused_fwd", "wgrad", "dgrad", "reduce"};
  ga_set_merged_pair(0);
  ga_set_slab_sum_in_dgrad(1);
  // ---- one network per launch; `fuses`: the step qualifies for the fused launch
  struct Case { int in; std::vector<int> h; int64_t S, mb; bool fuses; };
  const Case cases[] = {
      {17, {256, 256}, 1000, 1000, true},   // 4 splits
      {17, {256, 256}, 1300, 1300, true},   // 6 splits
      {17, {256, 256}, 600, 300, true},     // 2 splits, two steps
      {17, {256, 256}, 64, 64, true},       // one split, one tile
      {1, {128, 128}, 600, 300, true},
      {32, {128, 128}, 300, 300, true},
      {17, {256, 128}, 300, 300, false},    // hidden layers of different widths
      {17, {128, 256}, 300, 300, false},
  };
  for (int on = 1; on >= 0; --on) {
    CHECK(ga_set_fused_fwd_dgrad(on) == 0);
    for (const Case& c : cases) {
      Net net(c.in, c.h, 6, c.S, c.mb);
      ga_update_args a = net.args(c.S, c.mb, 0);
      clear_log();
      const int rc = ga_update_epoch(&a, st);
      if (rc) fprintf(stderr, "rc %d: %s\n", rc, g_error.c_str());
      CHECK(rc == 0);
      const size_t steps = (size_t)((c.S + c.mb - 1) / c.mb);
      const bool fused = on && c.fuses;
      const std::vector<const char*>& seq = fused ? fused_seq : old_seq;
      CHECK(g_log.size() == steps * seq.size());
      if (g_log.size() != steps * seq.size()) {
        fprintf(stderr, "  on %d, %d -> %d x %d, mb %d:", on, c.in, c.h[0], c.h[1], (int)c.mb);
        for (const Launch& l : g_log) fprintf(stderr, " %s", l.what.c_str());
        fprintf(stderr, "\n");
      }
      for (size_t k = 0; k < steps; ++k) CHECK(log_is(k * seq.size(), seq, st));
      CHECK(g_reduce.size() == steps);
      CHECK(g_dgrad.size() == (fused ? 0 : steps));
      const bool folds = ga_mlp_backward_splits(&net.d, c.mb) > 1;
      for (const ReduceCall& r : g_reduce) {
        if (fused)
          check_mid_regions(r, net, c.mb);
        else  // the slab sum rides in the data-gradient launch as before
          CHECK(r.presummed == (folds ? 0xcu : 0u));
      }
      for (const ga_fused_dgrad_net& g : g_dgrad) CHECK((g.sum_w.src != nullptr) == folds);
    }
  }
  ga_set_fused_fwd_dgrad(1);
  // ---- one and three hidden layers, more than 32 inputs, a first layer too large for
  //      the kernel (32 x 256 weights), the narrow step: no fused launch whatever the
  //      switch says
  {
    struct Other { int in; std::vector<int> h; };
    const Other others[] = {{17, {256}}, {17, {256, 256, 256}}, {40, {256, 256}},
                            {32, {256, 256}}, {17, {64, 64}}};
    for (const Other& o : others) {
      Net net(o.in, o.h, 6, 300, 300);
      ga_update_args a = net.args(300, 300, 0);
      clear_log();
      CHECK(ga_update_epoch(&a, st) == 0);
      CHECK(!g_log.empty() && g_log.back().what == "reduce");
      for (const Launch& l : g_log) CHECK(l.what != "fwd_dgrad");
    }
  }
  // ---- the data-parallel step and phase 1 take the fused launch too: the all-reduce
  //      follows the optimizer launch's sum
  {
    ga_set_allreduce_hook([](void*, float*, int64_t, void*) { return 0; });
    Net net(17, {256, 256}, 6, 1000, 500);
    ga_update_args a = net.args(1000, 500, 0);
    a.comm = (void*)1; a.world = 2; a.n_mb = 2; a.grad_scale = 0.5f;
    clear_log();
    CHECK(ga_update_epoch(&a, st) == 0);
    CHECK(g_log.size() == 6 && log_is(0, fused_seq, st) && log_is(3, fused_seq, st));
    for (const ReduceCall& r : g_reduce) check_mid_regions(r, net, 500);
  }
  // ---- two networks, a stream each (the two-stream schedule): each network's steps are
  //      the fused sequence on ITS stream
  {
    void* const st2 = (void*)0x20;
    Net pol(17, {256, 256}, 6, 600, 300), vf(17, {256, 256}, 1, 600, 300);
    ga_update_args a = pol.args(600, 300, 0), b = vf.args(600, 300, 1);
    clear_log();
    const int rc = ga_update_epoch_pair(&a, st, &b, st2);
    if (rc) fprintf(stderr, "pair rc %d: %s\n", rc, g_error.c_str());
    CHECK(rc == 0);
    for (void* s : {st, st2}) {
      std::vector<Launch> mine;
      for (const Launch& l : g_log)
        if (l.stream == s) mine.push_back(l);
      CHECK(mine.size() == 6);
      for (size_t i = 0; i < mine.size() && i < 6; ++i)
        CHECK(mine[i].what == fused_seq[i % 3] && mine[i].n_nets == 1);
    }
    CHECK(g_log.size() == 12);
    for (const ReduceCall& r : g_reduce) CHECK(r.presummed == 0u);
  }
  // ---- the merged pair schedule (two networks per launch) keeps its four launches and
  //      the slab sum in the data-gradient launch
  {
    ga_set_merged_pair(1);
    Net pol(17, {256, 256}, 6, 600, 300), vf(17, {256, 256}, 1, 600, 300);
    ga_update_args a = pol.args(600, 300, 0), b = vf.args(600, 300, 1);
    clear_log();
    const int rc = ga_update_epoch_pair(&a, st, &b, (void*)0x20);
    if (rc) fprintf(stderr, "merged rc %d: %s\n", rc, g_error.c_str());
    CHECK(rc == 0);
    CHECK(g_log.size() == 8);
    for (size_t i = 0; i < g_log.size() && i < 8; ++i)
      CHECK(g_log[i].what == old_seq[i % 4] && g_log[i].n_nets == 2);
    CHECK(g_reduce.size() == 4);
    for (const ReduceCall& r : g_reduce) CHECK(r.presummed == 0xcu);
    for (const ga_fused_dgrad_net& g : g_dgrad) CHECK(g.sum_w.src && g.sum_b.src);
    ga_set_merged_pair(0);
  }
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("fused fwd dgrad ok\n");
  return 0;
}
