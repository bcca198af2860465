// Host-logic harness for the slab ranges a fused optimizer step hands to its
// data-gradient launch (garage_amd/csrc/update.cpp: fused_step), built with
// -fsanitize=address,undefined on the CPU (`make asan-slab-sum`).  Every launch the
// epoch loops make is a fake; the fakes of the data-gradient launch and of the optimizer
// launch keep their descriptors and walk the memory the kernels would: the ranges are
// set exactly when the step has the fused data-gradient launch, two hidden layers, more
// than one split and ga_set_slab_sum_in_dgrad is on -- in the two-stream schedule and in
// the merged pair schedule --, they lie inside the slab workspace (allocated at exactly
// splits * n_flat floats: a range beyond it is an AddressSanitizer report), the
// weight-gradient launch is the one right before on the same stream, and the optimizer
// launch's pre-summed regions are the middle layer's two and no others.
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

// what the fakes saw
struct DgradCall {
  int n_nets;
  ga_fused_dgrad_net net[2];
  bool after_wgrad;  // the launch before it, on the same stream, was the weight-gradient GEMM
};
struct ReduceCall {
  int n_nets;
  uint32_t presummed[2];
  int n_regions[2];
};
static std::vector<DgradCall> g_dgrad;
static std::vector<ReduceCall> g_reduce;
static const char* g_last_launch = "";
static void* g_last_stream = nullptr;
static void launched(const char* what, void* stream) {
  g_last_launch = what;
  g_last_stream = stream;
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
// the middle layers' backward GEMMs; the LAST launch it makes is layer 1's weight gradient
int ga_mlp_backward_range_f32(const ga_mlp_desc* d, const float*, const float*, int64_t,
                              const int32_t*, int64_t, const float*, const float*, int64_t,
                              float*, float* slabs, int64_t n_flat, int64_t splits, int,
                              int fused_first, hipStream_t s) {
  if (fused_first)  // ... and it writes every partial of that layer
    for (int64_t k = 0; k < splits; ++k) {
      memset(slabs + k * n_flat + d->w_off[1], 0,
             sizeof(float) * (size_t)d->dims[2] * ((d->dims[1] + 3) & ~3));
      memset(slabs + k * n_flat + d->b_off[1], 0, sizeof(float) * (size_t)d->dims[2]);
    }
  launched(fused_first ? "wgrad" : "bwd_range", s);
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
int ga_fused_fwd_head_loss(const ga_fused_fwd_net*, int, int64_t, int, int, hipStream_t s) {
  launched("fused_fwd", s);
  return 0;
}
int ga_wgrad_mid(const ga_wgrad_mid_net* n, int n_nets, int64_t, int64_t n_splits, int out_w,
                 int in_w, hipStream_t s) {
  for (int i = 0; i < n_nets; ++i)
    for (int64_t k = 0; k < n_splits; ++k) {
      memset(n[i].slabs_w + k * n[i].slab_stride, 0, sizeof(float) * (size_t)out_w * in_w);
      memset(n[i].slabs_b + k * n[i].slab_stride, 0, sizeof(float) * (size_t)out_w);
    }
  launched("wgrad", s);
  return 0;
}
int ga_fused_dgrad_wgrad0(const ga_fused_dgrad_net* n, int n_nets, int64_t, int, int, int,
                          hipStream_t s) {
  DgradCall c;
  c.n_nets = n_nets;
  c.after_wgrad = !strcmp(g_last_launch, "wgrad") && g_last_stream == (void*)s;
  for (int i = 0; i < n_nets; ++i) {
    c.net[i] = n[i];
    // what the kernel does with a range: reads every partial of every element and
    // writes partial 0
    const ga_slab_range* r[2] = {&n[i].sum_w, &n[i].sum_b};
    for (int j = 0; j < 2; ++j) {
      if (!r[j]->src) continue;
      for (int64_t e = 0; e < r[j]->n; ++e) {
        float sum = 0.f;
        for (int k = 0; k < r[j]->n_part; ++k) sum += r[j]->src[k * r[j]->stride + e];
        r[j]->src[e] = sum;
      }
    }
  }
  g_dgrad.push_back(c);
  launched("dgrad", s);
  return 0;
}
int ga_reduce_regions_adam(const ga_reduce_net* n, int n_nets, hipStream_t s) {
  ReduceCall c;
  c.n_nets = n_nets;
  for (int i = 0; i < n_nets; ++i) {
    c.presummed[i] = n[i].presummed;
    c.n_regions[i] = n[i].n_regions;
    if (n[i].loss_out) *n[i].loss_out = 1.f;
  }
  g_reduce.push_back(c);
  launched("reduce", s);
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

static int g_failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++g_failed;                                                         \
    }                                                                     \
  } while (0)

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

static bool range_is_null(const ga_slab_range& r) {
  return !r.src && r.n == 0 && r.stride == 0 && r.n_part == 0;
}

// the ranges of one network's data-gradient descriptor for a minibatch of M rows
static void check_ranges(const ga_fused_dgrad_net& g, Net& n, int64_t M, bool want) {
  if (!want) {
    CHECK(range_is_null(g.sum_w) && range_is_null(g.sum_b));
    return;
  }
  const ga_mlp_desc& d = n.d;
  const int64_t n_flat = (int64_t)n.params.size();
  const int64_t splits = ga_mlp_backward_splits(&d, M);
  float* slabs = n.slabs.data();
  CHECK(g.sum_w.src == slabs + d.w_off[1] && g.sum_b.src == slabs + d.b_off[1]);
  CHECK(g.sum_w.n == (int64_t)d.dims[2] * ((d.dims[1] + 3) & ~3) && g.sum_w.n % 4 == 0);
  CHECK(g.sum_b.n == ((d.dims[2] + 3) & ~3));
  const ga_slab_range* r[2] = {&g.sum_w, &g.sum_b};
  for (int i = 0; i < 2; ++i) {
    CHECK(r[i]->stride == n_flat && r[i]->n_part == (int)splits);
    CHECK(r[i]->src >= slabs &&
          r[i]->src + (r[i]->n_part - 1) * r[i]->stride + r[i]->n <= slabs + splits * n_flat);
  }
}

int main() {
  extern int ga_set_merged_pair(int on);
  // ---- the two-stream schedule: one network per launch
  struct Case { int in; std::vector<int> h; int64_t S, mb; bool dgrad, folds; };
  const Case cases[] = {
      {17, {256, 256}, 1000, 1000, true, true},   // 4 splits
      {17, {256, 256}, 1300, 1300, true, true},   // 6 splits: ragged runs
      {17, {128, 128}, 600, 300, true, true},     // 2 splits, two steps
      {17, {256, 256}, 256, 256, true, false},    // one split: nothing to sum
      {17, {256, 256}, 64, 64, true, false},
      {17, {256, 256, 256}, 1000, 1000, true, false},  // three hidden layers: L == 4
      {40, {256, 256}, 1000, 1000, false, false},      // > 32 inputs: no fused data gradient
      {17, {64, 64}, 1000, 1000, false, false},        // the narrow step
  };
  for (int on = 1; on >= 0; --on) {
    CHECK(ga_set_slab_sum_in_dgrad(on) == 0);
    for (const Case& c : cases) {
      Net net(c.in, c.h, 6, c.S, c.mb);
      ga_update_args a = net.args(c.S, c.mb, 0);
      g_dgrad.clear();
      g_reduce.clear();
      const int rc = ga_update_epoch(&a, (void*)0x10);
      if (rc) fprintf(stderr, "rc %d: %s\n", rc, g_error.c_str());
      CHECK(rc == 0);
      const size_t steps = (size_t)((c.S + c.mb - 1) / c.mb);
      CHECK(g_dgrad.size() == (c.dgrad ? steps : 0));
      CHECK(g_reduce.size() == steps);
      const bool want = c.folds && on;
      for (const DgradCall& g : g_dgrad) {
        CHECK(g.n_nets == 1 && g.after_wgrad);
        check_ranges(g.net[0], net, c.mb, want);
      }
      for (const ReduceCall& r : g_reduce) {
        CHECK(r.n_nets == 1 && r.n_regions[0] == 2 * net.d.n_layers);
        // regions 2 and 3: the middle layer's weights and bias
        CHECK(r.presummed[0] == (want ? 0xcu : 0u));
      }
    }
  }
  // ---- the data-parallel step (the all-reduce follows the optimizer launch's sum) and
  //      phase 1 (the scaled gradient only) take the same ranges
  {
    ga_set_slab_sum_in_dgrad(1);
    ga_set_allreduce_hook([](void*, float*, int64_t, void*) { return 0; });
    Net net(17, {256, 256}, 6, 1000, 500);
    ga_update_args a = net.args(1000, 500, 0);
    a.comm = (void*)1; a.world = 2; a.n_mb = 2; a.grad_scale = 0.5f;
    g_dgrad.clear();
    g_reduce.clear();
    CHECK(ga_update_epoch(&a, (void*)0x10) == 0);
    CHECK(g_dgrad.size() == 2 && g_reduce.size() == 2);
    for (const DgradCall& g : g_dgrad) check_ranges(g.net[0], net, 500, true);
    for (const ReduceCall& r : g_reduce) CHECK(r.presummed[0] == 0xcu);
  }
  // ---- the merged pair schedule: both networks' step k in one launch each
  for (int on = 1; on >= 0; --on) {
    ga_set_slab_sum_in_dgrad(on);
    ga_set_merged_pair(1);
    const int64_t S = 1000, mb = 300;  // 300, 300, 300, 100: 2, 2, 2, 1 splits
    Net pol(17, {256, 256}, 6, S, mb), vf(17, {256, 256}, 1, S, mb);
    ga_update_args a = pol.args(S, mb, 0), b = vf.args(S, mb, 1);
    g_dgrad.clear();
    g_reduce.clear();
    const int rc = ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20);
    if (rc) fprintf(stderr, "pair rc %d: %s\n", rc, g_error.c_str());
    CHECK(rc == 0);
    CHECK(g_dgrad.size() == 4 && g_reduce.size() == 4);
    for (size_t k = 0; k < g_dgrad.size() && k < g_reduce.size(); ++k) {
      const int64_t M = k < 3 ? 300 : 100;
      const bool want = on && M > 256;
      CHECK(g_dgrad[k].n_nets == 2 && g_dgrad[k].after_wgrad);
      check_ranges(g_dgrad[k].net[0], pol, M, want);
      check_ranges(g_dgrad[k].net[1], vf, M, want);
      CHECK(g_reduce[k].n_nets == 2);
      for (int i = 0; i < 2; ++i) CHECK(g_reduce[k].presummed[i] == (want ? 0xcu : 0u));
    }
    ga_set_merged_pair(0);
  }
  ga_set_slab_sum_in_dgrad(1);
  if (g_failed) {
    fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("slab sum ok\n");
  return 0;
}
