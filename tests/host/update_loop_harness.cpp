// Host-logic harness for the C++ epoch loops (garage_amd/csrc/update.cpp), built with
// -fsanitize=address,undefined on the CPU (SURVEY.md section 5 "sanitizers": GPU
// sanitizers are not available, the host loops are plain C++).  Every kernel entry point
// the loops call -- and the handful of HIP runtime calls they make -- is a recording fake
// (fake_update_kernels.h, harness.h), so the checks are about the loops' own arithmetic.
// Three suites, chosen on the command line (none: all of them):
//   loops      `make asan-host`: which rows form which minibatch, how many steps a pass
//              takes (single process and data parallel), the order in which two passes
//              interleave, what is skipped in which phase, argument errors refused before
//              anything is launched, the fused / narrow / small step's plans and extents;
//   slab-sum   `make asan-slab-sum`: the slab ranges a fused step hands to its
//              data-gradient launch and the optimizer launch's pre-summed regions;
//   fwd-dgrad  `make asan-fwd-dgrad`: fused_step's choice between the fused forward +
//              data-gradient launch and the two launches (ga_set_fused_fwd_dgrad).
// Every suite builds its passes on exactly-sized buffers (Net) and sets each product and
// fake switch it depends on at entry, so it passes whatever ran before it.
#include "fake_update_kernels.h"

// the product's switches at their defaults, the fake side's as the suite wants them
static void begin_suite(bool small_step_answers, bool fwd_dgrad_answers) {
  ga_set_fused_head_loss(0);
  ga_set_fused_train(1);
  ga_set_narrow_step(1);
  ga_set_fused_first_layer(1);
  ga_set_slab_sum_in_dgrad(1);
  ga_set_fused_fwd_dgrad(1);
  ga_set_small_step(1);
  ga_set_ordered_allreduce(1);
  ga_set_merged_pair(0);
  ga_set_allreduce_hook(nullptr);
  g_small_step_answers = small_step_answers;
  g_fwd_dgrad_answers = fwd_dgrad_answers;
  g_fwd_dgrad_unasked_aborts = true;
  g_ss_n_flat = g_ss_ws_floats = 0;
  g_ss_extent_errors = 0;
  g_error.clear();
  clear_log();
}

static int fake_allreduce(void*, float*, int64_t n, void*) {
  logf("allreduce n=%lld", (long long)n);
  return 0;
}

// ======================================================================================
// loops: a kernel side with the small step and WITHOUT the fused forward + data-gradient
// instantiation (update.cpp asks, is told "no" and never makes the launch)
// ======================================================================================
static void suite_loops() {
  begin_suite(true, false);
  Net net(17, {48, 48}, 6, 23, 23);  // 48-wide: neither the small step nor the fused step
  for (int i = 0; i < 23; ++i) net.perm[(size_t)i] = 22 - i;
  // 1. BatchDataset minibatches: ceil(S / mb) of mb ids, the last one partial
  {
    clear_log();
    ga_update_args a = net.args(23, 5, 0);
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK((ms_of("fwd") == std::vector<long long>{5, 5, 5, 5, 3}));
    CHECK(count("reduce_adam") == 5 && count("adam step") == 0);
    CHECK(g_log[0].find("idx0=22") != std::string::npos);
  }
  // 2. the even split of a data-parallel rank: exactly n_mb steps, per-step scales,
  //    one all-reduce each, Adam after it
  {
    clear_log();
    ga_set_allreduce_hook(fake_allreduce);
    const float scales[4] = {0.25f, 0.5f, 0.75f, 1.0f};
    ga_update_args a = net.args(23, 0, 1);
    a.n_mb = 4; a.grad_scales_host = scales; a.comm = (void*)1; a.world = 2;
    a.step0 = 10;
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK((ms_of("fwd") == std::vector<long long>{5, 6, 6, 6}));
    CHECK(count("allreduce") == 4 && count("reduce_adam") == 0);
    CHECK(count("reduce_slabs splits=1 scale=0.2500") == 1);
    CHECK(count("reduce_slabs splits=1 scale=1.0000") == 1);
    CHECK(count("adam step=11") == 1 && count("adam step=14") == 1);
  }
  // 3. phase 1 stops at the scaled gradient: no exchange, no optimizer
  {
    clear_log();
    ga_update_args a = net.args(23, 23, 0);
    a.phase = 1; a.grad_scale = 0.5f;
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("reduce_slabs splits=1 scale=0.5000") == 1);
    CHECK(count("adam") == 0 && count("allreduce") == 0 && count("reduce_adam") == 0);
  }
  // 4. two passes interleave minibatch by minibatch on their streams
  {
    clear_log();
    Net other(17, {48, 48}, 1, 23, 8);
    ga_update_args a = net.args(23, 8, 0);
    ga_update_args b = other.args(23, 8, 1);
    CHECK(ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20) == 0);
    std::vector<std::string> order;
    for (auto& l : g_log)
      if (l.rfind("fwd", 0) == 0)
        order.push_back(l.find("stream=0x10") != std::string::npos ? "a" : "b");
    CHECK((order == std::vector<std::string>{"a", "b", "a", "b", "a", "b"}));
    // sharing buffers is refused
    CHECK(ga_update_epoch_pair(&a, (void*)0x10, &a, (void*)0x20) != 0);
  }
  // 5. argument errors never launch
  {
    clear_log();
    ga_update_args a = net.args(0, 5, 0);
    CHECK(ga_update_epoch(&a, nullptr) != 0 && g_log.empty());
    a = net.args(23, 0, 0);
    CHECK(ga_update_epoch(&a, nullptr) != 0 && g_log.empty());
    a = net.args(23, 5, 0);
    a.n_mb = 24;  // more minibatches than samples
    CHECK(ga_update_epoch(&a, nullptr) != 0 && g_log.empty());
    CHECK(ga_update_epoch(nullptr, nullptr) != 0);
    a = net.args(4000, 4000, 0);
    a.perm = nullptr;
    a.max_splits = 2;  // slab workspace too small for 16 splits
    CHECK(ga_update_epoch(&a, nullptr) != 0);
    CHECK(g_error.find("slab workspace") != std::string::npos);
    CHECK(g_events.empty());
  }
  // 6. the small step takes minibatches of <= 64 rows of a 2 x H net
  {
    clear_log();
    Net small(17, {64, 64}, 6, 200, 64);
    ga_update_args a = small.args(200, 64, 0);
    ga_set_fused_train(0);
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("small_step") == 4 && count("fwd") == 0);  // 64, 64, 64, 8
    ga_set_small_step(0);
    clear_log();
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("small_step") == 0 && count("fwd") == 4);
    ga_set_small_step(1);
    ga_set_fused_train(1);
  }
  // 7. the fused step: plan, scratch layout, regions
  {
    clear_log();
    const int64_t M = 1000;
    Net wide(17, {256, 256}, 6, M, M);
    const int64_t need = ga_update_partials_floats(&wide.d, M);
    const int64_t tiles = ga_fused_tiles(M);
    CHECK(need == 4 * tiles + tiles * (8 * 256 + 8) + tiles * (256 * 20 + 256));
    CHECK(ga_update_partials_floats(&net.d, M) == 0);  // 48-wide: per-layer path
    ga_update_args a = wide.args(M, M, 0);
    // (the scratch is exactly what was asked for)
    CHECK((int64_t)wide.partials.size() == need && a.partials_floats == need);
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    // (the first layer is computed inside the fused kernel: no forward launch)
    CHECK(count("fused_fwd M=1000 width=256 K=256 a_idx=0 A=6 first=1") == 1);
    CHECK(count("bwd_range M=1000 l_start=1 fused_first=1") == 1);
    CHECK(count("fused_dgrad M=1000 width=256 K=256 in=17") == 1);
    CHECK(count("reduce_regions n=6 step=1 scale=1.0000 adam=1 zero0=0 lparts=16") == 1);
    CHECK(count("fwd M=1000") == 0);
    ga_set_fused_first_layer(0);
    clear_log();
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("fused_fwd M=1000 width=256 K=256 a_idx=0 A=6 first=0") == 1);
    CHECK(count("fwd M=1000") == 1);  // the hidden layer below the last one
    ga_set_fused_first_layer(1);
    // a scratch one float short falls back to the per-layer kernels
    clear_log();
    a.partials_floats = need - 1;
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("fused_fwd") == 0 && count("reduce_adam") == 1);
  }
  // 7b. 2 x 64 networks: the whole step in one launch + the reduction
  {
    clear_log();
    const int64_t M = 200, tiles = 4;
    Net narrow(4, {64, 64}, 2, M, 100);
    const int64_t need = ga_update_partials_floats(&narrow.d, M);
    CHECK(need == 4 * tiles + tiles * ga_narrow_step_stride(4, 64));
    ga_update_args a = narrow.args(M, 100, 2);
    CHECK(ga_update_epoch(&a, nullptr) == 0);
    CHECK(count("narrow M=100 in=4 H=64 out=2") == 2 && count("fwd") == 0);
    CHECK(count("reduce_regions n=6 step=1") == 1 && count("reduce_regions n=6 step=2") == 1);
    CHECK(count("  region beg=4 n=256 parts=2") == 2);  // W1, both steps
  }
  // 8b. Two 256-wide passes with equal shapes: ga_update_epoch_pair runs step k of
  //     both as four pair launches on stream_a, ordered against stream_b on both
  //     sides; a different minibatch count, a data-parallel communicator or
  //     ga_set_merged_pair(0) give the two-stream schedule back
  {
    ga_set_merged_pair(1);  // (opt-in: the two-stream schedule is the default)
    const int64_t S = 1000, mb = 300;  // 4 minibatches: 300, 300, 300, 100
    Net pol(17, {256, 256}, 6, S, mb), vf(17, {256, 256}, 1, S, mb);
    for (int64_t i = 0; i < S; ++i) vf.perm[(size_t)i] = (int32_t)(S - 1 - i);
    const int64_t need = ga_update_partials_floats(&pol.d, mb);
    CHECK(need > 0 && need == ga_update_partials_floats(&vf.d, mb));
    ga_update_args a = pol.args(S, mb, 0);
    ga_update_args b = vf.args(S, mb, 1);
    a.step0 = 10; b.step0 = 20;
    clear_log();
    {
      const int rc8 = ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20);
      if (rc8) fprintf(stderr, "8b: rc %d error '%s'\n", rc8, g_error.c_str());
      if (getenv("GA_HARNESS_DUMP"))
        for (auto& l : g_log) fprintf(stderr, "  | %s\n", l.c_str());
      CHECK(rc8 == 0);
    }
    CHECK(count("pair_fwd stream=0x10") == 4 && count("pair_wgrad stream=0x10") == 4);
    CHECK(count("pair_dgrad stream=0x10") == 4 && count("pair_reduce stream=0x10") == 4);
    CHECK(count("pair_fwd stream=0x10 M=300 width=256 K=256 A=6/1 in=17/17") == 3);
    CHECK(count("pair_fwd stream=0x10 M=100") == 1);
    CHECK(count("pair_reduce stream=0x10 steps=11/21 regions=6/6 adam=1/1 M=300") == 1);
    CHECK(count("pair_reduce stream=0x10 steps=14/24") == 1);
    CHECK(count("fused_fwd") == 0 && count("reduce_regions") == 0);
    // stream_a first waits for what stream_b holds, stream_b then for the epoch
    CHECK(g_log.size() > 4 && g_log[0].rfind("record stream=0x20", 0) == 0 &&
          g_log[1].rfind("wait stream=0x10", 0) == 0 &&
          g_log[g_log.size() - 2].rfind("record stream=0x10", 0) == 0 &&
          g_log.back().rfind("wait stream=0x20", 0) == 0);
    // the two-stream schedule on request
    ga_set_merged_pair(0);
    clear_log();
    CHECK(ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20) == 0);
    CHECK(count("pair_") == 0 && count("fused_fwd") == 8 && count("reduce_regions n=") == 8);
    ga_set_merged_pair(1);
    // data parallel: never merged (each chain's all-reduce hides under the other)
    ga_set_allreduce_hook(fake_allreduce);
    a.comm = b.comm = (void*)0x1; a.world = b.world = 2; a.grad_scale = b.grad_scale = 0.5f;
    clear_log();
    CHECK(ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20) == 0);
    CHECK(count("pair_") == 0 && count("allreduce") == 8);
    a.comm = b.comm = nullptr;
    // unequal minibatch counts: not merged
    b.mb = 250;
    clear_log();
    CHECK(ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20) == 0);
    CHECK(count("pair_") == 0 && count("fused_fwd") == 8);
    ga_set_merged_pair(0);
  }
  // 9. Host-computed extents against what the kernels' index formulas reach, at the
  //    extreme shapes (32-wide nets, 1-row minibatches, 8 outputs, 32 inputs): every
  //    buffer is allocated at EXACTLY the size the Python side computes
  //    (ga_update_partials_floats; activation workspaces = largest minibatch x sum of
  //    the hidden widths; the flat parameter layout) and the fakes write / index the
  //    kernels' full extents, so an undersized buffer is an AddressSanitizer report.
  {
    const int ins[] = {1, 4, 17, 31, 32};
    const int hs[] = {32, 64, 128, 256};
    const int outs[] = {1, 6, 8};
    const int64_t ms[] = {1, 31, 32, 63, 64, 65, 200, 4096};
    int fused = 0, narrow = 0, small = 0;
    for (int in : ins) for (int h : hs) for (int out : outs) for (int64_t M : ms) {
      Net n(in, {h, h}, out, M, M);
      ga_update_args a = n.args(M, M, out == 1 ? 1 : 0);
      // activation workspaces as garage_amd/engine.py sizes them: rows x (h1 + h2)
      CHECK((int64_t)n.acts.size() == M * 2 * (int64_t)h);
      g_ss_n_flat = (int64_t)n.params.size();
      g_ss_ws_floats = (int64_t)n.acts.size();
      clear_log();
      CHECK(ga_update_epoch(&a, nullptr) == 0);
      fused += count("fused_fwd");
      narrow += count("narrow M=");
      small += count("small_step");
      // a 2 x H net with <= 64 rows must only take the one-launch step when its two
      // exchanges fit the activation workspaces (32 rows up)
      if (count("small_step")) CHECK(M >= 32 && M <= 64);
    }
    g_ss_n_flat = g_ss_ws_floats = 0;
    CHECK(g_ss_extent_errors == 0);
    CHECK(fused > 0 && narrow > 0 && small > 0);
  }
}

// ======================================================================================
// slab-sum: the ranges are set exactly when the step has the fused data-gradient launch,
// two hidden layers, more than one split and ga_set_slab_sum_in_dgrad is on -- in the
// two-stream schedule and in the merged pair schedule --, they lie inside the slab
// workspace (a range beyond it is an AddressSanitizer report: the data-gradient fake
// walks it), the weight-gradient launch is the one right before on the same stream, and
// the optimizer launch's pre-summed regions are the middle layer's two and no others.
// The kernel side has neither the small step nor the fused forward + data gradient.
// ======================================================================================
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

static void suite_slab_sum() {
  begin_suite(false, false);
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
      CHECK((int64_t)net.slabs.size() == net.splits * (int64_t)net.params.size());
      ga_update_args a = net.args(c.S, c.mb, 0);
      clear_log();
      const int rc = ga_update_epoch(&a, (void*)0x10);
      if (rc) fprintf(stderr, "rc %d: %s\n", rc, g_error.c_str());
      CHECK(rc == 0);
      const size_t steps = (size_t)((c.S + c.mb - 1) / c.mb);
      CHECK(events_of("dgrad").size() == (c.dgrad ? steps : 0));
      CHECK(events_of("reduce").size() == steps);
      const bool want = c.folds && on;
      for (const Event* g : events_of("dgrad")) {
        CHECK(g->n_nets == 1 && g->after_wgrad);
        check_ranges(g->dgrad[0], net, c.mb, want);
      }
      for (const Event* r : events_of("reduce")) {
        CHECK(r->n_nets == 1 && (int)r->reduce[0].regions.size() == 2 * net.d.n_layers);
        // regions 2 and 3: the middle layer's weights and bias
        CHECK(r->reduce[0].presummed == (want ? 0xcu : 0u));
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
    clear_log();
    CHECK(ga_update_epoch(&a, (void*)0x10) == 0);
    CHECK(events_of("dgrad").size() == 2 && events_of("reduce").size() == 2);
    for (const Event* g : events_of("dgrad")) check_ranges(g->dgrad[0], net, 500, true);
    for (const Event* r : events_of("reduce")) CHECK(r->reduce[0].presummed == 0xcu);
  }
  // ---- the merged pair schedule: both networks' step k in one launch each
  for (int on = 1; on >= 0; --on) {
    ga_set_slab_sum_in_dgrad(on);
    ga_set_merged_pair(1);
    const int64_t S = 1000, mb = 300;  // 300, 300, 300, 100: 2, 2, 2, 1 splits
    Net pol(17, {256, 256}, 6, S, mb), vf(17, {256, 256}, 1, S, mb);
    ga_update_args a = pol.args(S, mb, 0), b = vf.args(S, mb, 1);
    clear_log();
    const int rc = ga_update_epoch_pair(&a, (void*)0x10, &b, (void*)0x20);
    if (rc) fprintf(stderr, "pair rc %d: %s\n", rc, g_error.c_str());
    CHECK(rc == 0);
    const std::vector<const Event*> dgrad = events_of("dgrad"), reduce = events_of("reduce");
    CHECK(dgrad.size() == 4 && reduce.size() == 4);
    for (size_t k = 0; k < dgrad.size() && k < reduce.size(); ++k) {
      const int64_t M = k < 3 ? 300 : 100;
      const bool want = on && M > 256;
      CHECK(dgrad[k]->n_nets == 2 && dgrad[k]->after_wgrad);
      check_ranges(dgrad[k]->dgrad[0], pol, M, want);
      check_ranges(dgrad[k]->dgrad[1], vf, M, want);
      CHECK(reduce[k]->n_nets == 2);
      for (int i = 0; i < 2; ++i) CHECK(reduce[k]->reduce[i].presummed == (want ? 0xcu : 0u));
    }
    ga_set_merged_pair(0);
  }
  ga_set_slab_sum_in_dgrad(1);
}

// ======================================================================================
// fwd-dgrad: here the kernel side HAS the fused instantiation.  A step that qualifies is
// exactly
//   fused forward + data gradient -> middle-layer weight gradient -> optimizer launch
// on one stream, the fused launch gets two descriptors of ONE step and no slab ranges
// (the fake checks them), the optimizer launch gets no pre-summed region and the middle
// layer's regions as `splits` partials inside the slab workspace; and the four-launch
// sequence comes back with the switch off, with two networks per launch (the merged pair
// schedule), with one or three hidden layers, and at shapes the kernel side declines.
// ======================================================================================
// events [at, at + names.size()) are `names`, all on `stream`, one network each
static bool log_is(size_t at, const std::vector<const char*>& names, void* stream) {
  if (at + names.size() > g_events.size()) return false;
  for (size_t i = 0; i < names.size(); ++i)
    if (g_events[at + i].what != names[i] || g_events[at + i].stream != stream ||
        g_events[at + i].n_nets != 1)
      return false;
  return true;
}

// every network's share of every optimizer launch / data-gradient launch, in order
static std::vector<const ReduceSeen*> reduce_nets() {
  std::vector<const ReduceSeen*> out;
  for (const Event* e : events_of("reduce"))
    for (int i = 0; i < e->n_nets; ++i) out.push_back(&e->reduce[i]);
  return out;
}
static std::vector<const ga_fused_dgrad_net*> dgrad_nets() {
  std::vector<const ga_fused_dgrad_net*> out;
  for (const Event* e : events_of("dgrad"))
    for (int i = 0; i < e->n_nets; ++i) out.push_back(&e->dgrad[i]);
  return out;
}

// the middle layer's regions (2: weights, 3: bias) of an optimizer launch: `splits`
// partials inside the slab workspace, nothing pre-summed
static void check_mid_regions(const ReduceSeen& r, Net& n, int64_t M) {
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

static void suite_fwd_dgrad() {
  begin_suite(false, true);
  void* const st = (void*)0x10;
  const std::vector<const char*> fused_seq = {"fwd_dgrad", "wgrad", "reduce"};
  const std::vector<const char*> old_seq = {"fused_fwd", "wgrad", "dgrad", "reduce"};
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
      CHECK(g_events.size() == steps * seq.size());
      if (g_events.size() != steps * seq.size()) {
        fprintf(stderr, "  on %d, %d -> %d x %d, mb %d:", on, c.in, c.h[0], c.h[1], (int)c.mb);
        for (const Event& l : g_events) fprintf(stderr, " %s", l.what.c_str());
        fprintf(stderr, "\n");
      }
      for (size_t k = 0; k < steps; ++k) CHECK(log_is(k * seq.size(), seq, st));
      CHECK(reduce_nets().size() == steps);
      CHECK(dgrad_nets().size() == (fused ? 0 : steps));
      CHECK(events_of("fwd_dgrad").size() == (fused ? steps : 0));
      const bool folds = ga_mlp_backward_splits(&net.d, c.mb) > 1;
      for (const ReduceSeen* r : reduce_nets()) {
        if (fused)
          check_mid_regions(*r, net, c.mb);
        else  // the slab sum rides in the data-gradient launch as before
          CHECK(r->presummed == (folds ? 0xcu : 0u));
      }
      for (const ga_fused_dgrad_net* g : dgrad_nets()) CHECK((g->sum_w.src != nullptr) == folds);
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
      CHECK(!g_events.empty() && g_events.back().what == "reduce");
      for (const Event& l : g_events) CHECK(l.what != "fwd_dgrad");
    }
  }
  // ---- the data-parallel step and phase 1 take the fused launch too: the all-reduce and
  //      the optimizer's own launch follow the optimizer launch's sum
  {
    ga_set_allreduce_hook([](void*, float*, int64_t, void*) { return 0; });
    const std::vector<const char*> dp_seq = {"fwd_dgrad", "wgrad", "reduce", "adam"};
    Net net(17, {256, 256}, 6, 1000, 500);
    ga_update_args a = net.args(1000, 500, 0);
    a.comm = (void*)1; a.world = 2; a.n_mb = 2; a.grad_scale = 0.5f;
    clear_log();
    CHECK(ga_update_epoch(&a, st) == 0);
    CHECK(g_events.size() == 8 && log_is(0, dp_seq, st) && log_is(4, dp_seq, st));
    for (const ReduceSeen* r : reduce_nets()) check_mid_regions(*r, net, 500);
    ga_set_allreduce_hook(nullptr);
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
      std::vector<Event> mine;
      for (const Event& l : g_events)
        if (l.stream == s) mine.push_back(l);
      CHECK(mine.size() == 6);
      for (size_t i = 0; i < mine.size() && i < 6; ++i)
        CHECK(mine[i].what == fused_seq[i % 3] && mine[i].n_nets == 1);
    }
    CHECK(g_events.size() == 12);
    for (const ReduceSeen* r : reduce_nets()) CHECK(r->presummed == 0u);
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
    CHECK(g_events.size() == 8);
    for (size_t i = 0; i < g_events.size() && i < 8; ++i)
      CHECK(g_events[i].what == old_seq[i % 4] && g_events[i].n_nets == 2);
    CHECK(reduce_nets().size() == 4);
    for (const ReduceSeen* r : reduce_nets()) CHECK(r->presummed == 0xcu);
    for (const ga_fused_dgrad_net* g : dgrad_nets()) CHECK(g->sum_w.src && g->sum_b.src);
    ga_set_merged_pair(0);
  }
}

int main(int argc, char** argv) {
  return run_suites({{"loops", suite_loops, "host loops ok"},
                     {"slab-sum", suite_slab_sum, "slab sum ok"},
                     {"fwd-dgrad", suite_fwd_dgrad, "fused fwd dgrad ok"}},
                    argc, argv);
}
