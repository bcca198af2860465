// Host-logic harness for the population's joint diagnostics
// (garage_amd/csrc/members_diag_host.cpp), built with -fsanitize=address,undefined on the
// CPU (`make asan-members-diag`) and linked with the per-layer dispatch it asks for the
// members' forward plans (garage_amd/csrc/mlp_layers.cpp).  The kernel side is this
// file's own: every function of the members' launch seam (members_diag.h) copies the table
// it is given -- "device" memory is host memory here -- and records its grid; the lone
// launch seam below mlp_layers.cpp (layer_plans.h) records the parameter struct of every
// lone launch.  Checked: each member's table entry against the struct the LONE entry
// point launches for the same arguments (memcmp: pointers, rows, strides, plan, grid),
// the kernel kinds members of different row counts take, the launch count, every
// member's stretch of the partials (disjoint, inside the allocation at the exact size
// ga_members_diag_partials_doubles returns), one table copy a call, every argument error,
// and that an error copies and launches nothing.
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/members_diag.h"
#include "harness.h"

// ---- the members' launch seam: copy the table, record the grid ---------------------------
struct MdCall {
  std::string what;
  int sub = 0;  // KV / the GEMM kind / categorical
  unsigned n = 0, gx = 0, gy = 0, lds = 0;
  std::vector<GemmParams> gemm;
  std::vector<MdSkinnyEntry> skinny;
  std::vector<MdPpoEntry> ppo;
  std::vector<MdCatEntry> cat;
  std::vector<MdNllEntry> nll;
  std::vector<MdKlEntry> kl;
  std::vector<PpoFinalizeParams> ppo_fin;
  std::vector<MdCatFinalize> cat_fin;
  std::vector<MdNllFinalize> nll_fin;
  std::vector<MdSum> sum;
  std::vector<MdEpisodes> eps;
};
static std::vector<MdCall> g_md;
static int g_fail_launch = -1;  // the index of the members launch that answers an error

template <class T>
static int md_record(const char* what, int sub, const T* table, unsigned n, unsigned gx,
                     unsigned gy, unsigned lds, std::vector<T> MdCall::*field) {
  if ((int)g_md.size() == g_fail_launch) {
    ga_set_error("%s: launch failed (harness)", what);
    g_md.push_back(MdCall());
    g_md.back().what = "failed";
    return GA_ERR_HIP;
  }
  MdCall c;
  c.what = what; c.sub = sub; c.n = n; c.gx = gx; c.gy = gy; c.lds = lds;
  (c.*field).assign(table, table + n);
  g_md.push_back(c);
  return GA_OK;
}
int md_launch_gemm_members(int kind, const GemmParams* t, unsigned n, unsigned blocks,
                           hipStream_t) {
  return md_record("gemm", kind, t, n, blocks, 1, 0, &MdCall::gemm);
}
int md_launch_skinny_fwd_members(int KV, const MdSkinnyEntry* t, unsigned n, unsigned gx,
                                 unsigned gy, unsigned lds, hipStream_t) {
  return md_record("skinny", KV, t, n, gx, gy, lds, &MdCall::skinny);
}
int md_launch_ppo_gaussian_members(const MdPpoEntry* t, unsigned n, unsigned blocks,
                                   hipStream_t) {
  return md_record("ppo", 0, t, n, blocks, 1, 0, &MdCall::ppo);
}
int md_launch_ppo_gaussian_finalize_members(const PpoFinalizeParams* t, unsigned n,
                                            hipStream_t) {
  return md_record("ppo_fin", 0, t, n, 1, 1, 0, &MdCall::ppo_fin);
}
int md_launch_ppo_categorical_members(const MdCatEntry* t, unsigned n, unsigned blocks,
                                      hipStream_t) {
  return md_record("cat", 0, t, n, blocks, 1, 0, &MdCall::cat);
}
int md_launch_ppo_categorical_finalize_members(const MdCatFinalize* t, unsigned n,
                                               hipStream_t) {
  return md_record("cat_fin", 0, t, n, 1, 1, 0, &MdCall::cat_fin);
}
int md_launch_nll_members(const MdNllEntry* t, unsigned n, unsigned blocks, hipStream_t) {
  return md_record("nll", 0, t, n, blocks, 1, 0, &MdCall::nll);
}
int md_launch_nll_finalize_members(const MdNllFinalize* t, unsigned n, hipStream_t) {
  return md_record("nll_fin", 0, t, n, 1, 1, 0, &MdCall::nll_fin);
}
int md_launch_kl_members(int categorical, const MdKlEntry* t, unsigned n, unsigned blocks,
                         hipStream_t) {
  return md_record("kl", categorical, t, n, blocks, 1, 0, &MdCall::kl);
}
int md_launch_sum_members(const MdSum* t, unsigned n, hipStream_t) {
  return md_record("sum", 0, t, n, 1, 1, 0, &MdCall::sum);
}
int md_launch_episodes_members(const MdEpisodes* t, unsigned n, unsigned blocks, hipStream_t) {
  return md_record("episodes", 0, t, n, blocks, 1, 0, &MdCall::eps);
}

// ---- the lone launch seam below mlp_layers.cpp: record the structs ----------------------
struct LoneCall {
  int kind;  // MdFwdKind
  GemmParams g;
  GemmPlan gp;
  GemmHeadPlan hp;
  SkinnyFwdPlan sp;
  SkinnyFwdParams s;
};
static std::vector<LoneCall> g_lone;
int ga_gemm_launch(const GemmPlan& plan, const GemmParams& p, hipStream_t) {
  LoneCall c = {};
  c.kind = MD_FWD_GEMM; c.g = p; c.gp = plan;
  g_lone.push_back(c);
  return 0;
}
int ga_gemm_head_launch(const GemmHeadPlan& plan, const GemmParams& p, hipStream_t) {
  LoneCall c = {};
  c.kind = MD_FWD_GEMM_HEAD; c.g = p; c.hp = plan;
  g_lone.push_back(c);
  return 0;
}
int ga_skinny_fwd_launch(const SkinnyFwdPlan& plan, const SkinnyFwdParams& p, hipStream_t) {
  LoneCall c = {};
  c.kind = MD_FWD_SKINNY; c.sp = plan; c.s = p;
  g_lone.push_back(c);
  return 0;
}
// (nothing here takes a backward pass, LayerNorm or a whole-network forward)
int ga_gemm_pair_launch(const GemmPairPlan&, const GemmParams&, const GemmParams&,
                        hipStream_t) { abort(); }
int ga_skinny_wgrad_launch(const SkinnyWgradPlan&, const SkinnyWgradParams&, hipStream_t) {
  abort();
}
int ga_ln_forward(const float*, int64_t, const int32_t*, int64_t, int, const float*,
                  const float*, float*, int64_t, float*, hipStream_t) { abort(); }
int ga_ln_backward(float*, int64_t, const float*, int64_t, const int32_t*, const float*,
                   int64_t, int, const float*, int, int, int, int, float*, float*, int64_t,
                   hipStream_t) { abort(); }
int ga_ln_jvp(const float*, int64_t, const float*, int64_t, const int32_t*, const float*,
              int64_t, int, const float*, const float*, const float*, float*, int64_t,
              hipStream_t) { abort(); }
static int g_members_ok = 1;
extern "C" {
int ga_fused_eval_supported(int, const int*) { return 0; }
int ga_fused_eval_forward(const float*, int64_t, const int32_t*, int64_t, const int*,
                          const float*, const float*, const float*, const float*, const float*,
                          const float*, float*, int64_t, hipStream_t) { abort(); }
int ga_mlp_forward_fused_f32(const ga_mlp_desc*, const float*, const float*, int64_t,
                             const int32_t*, int64_t, float*, float*, int64_t, ga_stream_t) {
  abort();
}
int ga_split_bf16_enabled(void) { return 0; }
int ga_split_bf16_gemm(void) { return 0; }
const uint16_t* ga_weight_planes(const float*, int64_t, int, int, int, hipStream_t) { abort(); }
// update_members.cpp's predicate (the narrow step's shapes), the kernel side's answer
int ga_update_members_supported(const ga_mlp_desc* d) {
  return g_members_ok && d && d->n_layers == 3 && d->hidden_act == 0 && d->output_act == 0 &&
         !d->layer_norm && d->dims[1] == d->dims[2] && (d->dims[1] == 32 || d->dims[1] == 64) &&
         d->dims[0] <= 32 && d->dims[3] <= 8;
}
}  // extern "C"

// ---- exactly-sized "device" buffers --------------------------------------------------------
template <class T>
struct Buf {
  T* p;
  size_t n;
  explicit Buf(int64_t count) : n((size_t)(count > 0 ? count : 1)) {
    void* v = nullptr;
    if (posix_memalign(&v, 16, sizeof(T) * n)) abort();
    memset(v, 0, sizeof(T) * n);
    p = (T*)v;
  }
  ~Buf() { free(p); }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  bool holds(const void* q, int64_t count) const {
    return (const char*)q >= (const char*)p &&
           (const char*)q + sizeof(T) * (size_t)count <= (const char*)(p + n);
  }
};

static int r4i(int v) { return (v + 3) & ~3; }

// the flat layout of garage_amd/engine.py
struct Net {
  ga_mlp_desc d;
  int64_t n_flat, act_width, ld_out;
  Net(int in, int hidden, int out) {
    memset(&d, 0, sizeof(d));
    const int dims[4] = {in, hidden, hidden, out};
    d.n_layers = 3;
    int64_t off = 4;
    for (int l = 0; l < 4; ++l) d.dims[l] = dims[l];
    for (int l = 0; l < 3; ++l) {
      d.w_off[l] = off; off += (int64_t)dims[l + 1] * r4i(dims[l]);
      d.b_off[l] = off; off += r4i(dims[l + 1]);
    }
    n_flat = off;
    act_width = 2 * r4i(hidden);
    ld_out = r4i(out);
  }
};

static void reset() {
  g_md.clear();
  g_lone.clear();
  g_copies.clear();
  g_error.clear();
  g_fail_launch = -1;
}

// ---- forward -------------------------------------------------------------------------------
// every table entry of the joint forward is the struct the lone entry launches
static void forward_case(int in, int hidden, int out, std::vector<int64_t> rows,
                         int want_launches) {
  Net net(in, hidden, out);
  const int64_t n = (int64_t)rows.size(), ldx = r4i(in) + 4;
  std::vector<Buf<float>*> params, X, acts, outs;
  std::vector<ga_member_forward> mem((size_t)n);
  for (int64_t m = 0; m < n; ++m) {
    params.push_back(new Buf<float>(net.n_flat));
    X.push_back(new Buf<float>(rows[(size_t)m] * ldx));
    acts.push_back(new Buf<float>(rows[(size_t)m] * net.act_width));
    outs.push_back(new Buf<float>(rows[(size_t)m] * net.ld_out));
    mem[(size_t)m] = {params.back()->p, X.back()->p, ldx, rows[(size_t)m], acts.back()->p,
                      outs.back()->p, net.ld_out};
  }
  reset();
  CHECK(ga_mlp_forward_members_f32(&net.d, mem.data(), n, nullptr) == 0);
  CHECK((int)g_md.size() == want_launches);
  CHECK(g_copies.size() == 1);  // one table copy a call
  CHECK(g_lone.empty());        // the plans were asked, nothing was launched alone
  const std::vector<MdCall> joint = g_md;
  // launches come layer by layer
  size_t n_entries = 0;
  for (const MdCall& c : joint) n_entries += c.n;
  size_t lone_total = 0;
  for (int64_t m = 0; m < n; ++m) {
    // the lone entry on the member's arguments, the workspace laid out for its rows
    ga_mlp_desc dd = net.d;
    dd.act_off[0] = 0;
    dd.act_off[1] = (int64_t)r4i(hidden) * rows[(size_t)m];
    g_lone.clear();
    const ga_member_forward& u = mem[(size_t)m];
    CHECK(ga_mlp_forward_f32(&dd, u.params, u.X, u.ldx, nullptr, u.rows, u.acts, u.out,
                             u.ldo, nullptr) == 0);
    lone_total += g_lone.size();
    for (const LoneCall& lc : g_lone) {
      // find the one table entry that writes the same output
      int found = 0;
      for (const MdCall& c : joint) {
        if (lc.kind == MD_FWD_SKINNY) {
          for (const MdSkinnyEntry& e : c.skinny) {
            if (e.p.Y != lc.s.Y) continue;
            ++found;
            CHECK(!memcmp(&e.p, &lc.s, sizeof(lc.s)));
            CHECK(e.gx == lc.sp.gx && e.gy == lc.sp.gy);
            CHECK(c.sub == lc.sp.KV && c.gx >= e.gx && c.gy >= e.gy &&
                  c.lds >= lc.sp.lds_bytes);
          }
        } else {
          for (const GemmParams& e : c.gemm) {
            if (e.C != lc.g.C || e.head_out != lc.g.head_out) continue;
            ++found;
            CHECK(!memcmp(&e, &lc.g, sizeof(lc.g)));
            CHECK(c.gx >= (unsigned)(e.gx * e.gy * e.gz));
            if (lc.kind == MD_FWD_GEMM_HEAD) {
              CHECK(c.sub == MD_GEMM_HEAD_64 && lc.hp.width == 64);
            } else {
              CHECK(c.sub == (lc.gp.tile == GT_128x32 ? MD_GEMM_128x32 : MD_GEMM_64x64));
              CHECK(lc.gp.tile == GT_128x32 || lc.gp.tile == GT_64x64);
            }
          }
        }
      }
      CHECK(found == 1);
    }
    // the member's outputs and activations lie inside its own buffers
    for (const MdCall& c : joint)
      for (const GemmParams& e : c.gemm) {
        if (!outs[(size_t)m]->holds(e.C, 1) && !acts[(size_t)m]->holds(e.C, 1)) continue;
        const Buf<float>* b = outs[(size_t)m]->holds(e.C, 1) ? outs[(size_t)m] : acts[(size_t)m];
        CHECK(b->holds(e.C, (int64_t)(e.M - 1) * e.c_rs + e.N));
        CHECK(e.M == rows[(size_t)m]);
      }
  }
  CHECK(lone_total == n_entries);  // nothing more, nothing less than the lone launches
  for (auto* b : params) delete b;
  for (auto* b : X) delete b;
  for (auto* b : acts) delete b;
  for (auto* b : outs) delete b;
}

static void suite_forward() {
  // hidden 64: the streaming first layer for all; the middle layer with the head where
  // rows % 64 == 0, else 64 x 64 tiles and the head on 128 x 32 tiles
  forward_case(4, 64, 2, {64, 100, 1}, 4);
  forward_case(32, 64, 8, {128, 192}, 2);
  forward_case(1, 64, 1, {1, 255, 256, 257, 1000}, 4);
  // hidden 32: 128 x 32 tiles for every layer
  forward_case(4, 32, 3, {1, 255, 256, 257, 1000}, 3);
  forward_case(11, 32, 1, {7}, 3);
}

// ---- losses, KL, episodes ---------------------------------------------------------------
static void check_partials(const std::vector<std::pair<const double*, int64_t>>& stretches,
                           const Buf<double>& part) {
  for (size_t i = 0; i < stretches.size(); ++i) {
    CHECK(part.holds(stretches[i].first, stretches[i].second));
    for (size_t j = i + 1; j < stretches.size(); ++j)
      CHECK(stretches[i].first + stretches[i].second <= stretches[j].first ||
            stretches[j].first + stretches[j].second <= stretches[i].first);
  }
}

static void suite_losses() {
  const std::vector<int64_t> rows = {1, 256, 257, 1000, 255};
  const int64_t n = (int64_t)rows.size();
  const int64_t need = ga_members_diag_partials_doubles(rows.data(), n);
  CHECK(need == 2 * (1 + 1 + 2 + 4 + 1));
  Buf<double> part(need);
  float dummy[8] = {0};
  double out64[16] = {0};
  float out32[16] = {0};
  for (int kind : {0, 2}) {
    ga_members_loss_args a = {};
    a.kind = kind; a.A = 3; a.algo = 0; a.ent_flags = 5; a.has_min = 1; a.min_log_std = -2.f;
    a.has_max = 1; a.max_log_std = 1.f; a.double_softmax = 1;
    std::vector<ga_member_loss> mem((size_t)n);
    for (int64_t m = 0; m < n; ++m)
      mem[(size_t)m] = {dummy + m, 4 + m, dummy, 4, dummy, dummy, dummy, rows[(size_t)m],
                        0.1f * (float)(m + 1), 0.01f * (float)(m + 1), out32 + m, out64 + m};
    reset();
    CHECK(ga_ppo_loss_members_f32(&a, mem.data(), n, part.p, need, nullptr) == 0);
    CHECK(g_md.size() == 2 && g_copies.size() == 1);
    CHECK(g_md[0].n == n && g_md[0].gx == 4);
    CHECK(g_md[1].n == 2);  // the members of 257 and 1000 rows
    std::vector<std::pair<const double*, int64_t>> st;
    for (int64_t m = 0; m < n; ++m) {
      const unsigned nb = (unsigned)ga_red_blocks(rows[(size_t)m]);
      if (kind == 0) {
        const MdPpoEntry& e = g_md[0].ppo[(size_t)m];
        CHECK(e.nb == nb && e.p.M == rows[(size_t)m] && e.p.mean == dummy + m &&
              e.p.ldm == 4 + m && e.p.lda == 4 && e.p.A == 3 && e.p.algo == 0);
        CHECK(e.p.clip == 0.1f * (float)(m + 1) && e.p.ent.coeff == 0.01f * (float)(m + 1));
        CHECK(e.p.ent.regularized == 1 && e.p.ent.softplus == 0 && e.p.ent.stop_grad == 1);
        CHECK(e.p.has_min == 1 && e.p.min_log_std == -2.f && e.p.max_log_std == 1.f);
        CHECK((e.p.loss_out == out32 + m) == (nb == 1) && (e.p.loss_out == nullptr) == (nb > 1));
        CHECK(!e.p.idx && !e.p.dmean && !e.p.ll_out && !e.p.grad_slab0 && !e.p.ticket);
        st.push_back({e.p.partials, 2 * (int64_t)nb});
      } else {
        const MdCatEntry& e = g_md[0].cat[(size_t)m];
        CHECK(e.nb == nb && e.p.M == rows[(size_t)m] && e.p.scores == dummy + m &&
              e.p.lds == 4 + m && e.p.double_softmax == 1 && e.p.ent_sum_out == out64 + m);
        CHECK((e.p.loss_out == out32 + m) == (nb == 1) && (e.p.loss_out == nullptr) == (nb > 1));
        CHECK(!e.p.idx && !e.p.dscores && !e.p.ll_out && !e.p.ent_out && !e.p.grad_slab0);
        st.push_back({e.p.partials, 2 * (int64_t)nb});
      }
    }
    check_partials(st, part);
    if (kind == 0) {
      CHECK(g_md[1].what == "ppo_fin");
      const PpoFinalizeParams& f = g_md[1].ppo_fin[1];
      CHECK(f.nblocks == 4 && f.M == 1000 && f.loss_out == out32 + 3 &&
            f.partials == g_md[0].ppo[3].p.partials && f.A == 3 && f.has_max == 1 &&
            !f.grad_slab0);
    } else {
      CHECK(g_md[1].what == "cat_fin");
      const MdCatFinalize& f = g_md[1].cat_fin[0];
      CHECK(f.nblocks == 2 && f.M == 257 && f.loss_out == out32 + 2 &&
            f.ent_sum_out == out64 + 2 && f.partials == g_md[0].cat[2].p.partials);
    }
    // one double short: refused, nothing copied or launched
    reset();
    CHECK(ga_ppo_loss_members_f32(&a, mem.data(), n, part.p, need - 1, nullptr) < 0);
    CHECK(g_md.empty() && g_copies.empty() && g_error.find("partials too small") != std::string::npos);
  }
  // members of at most 256 rows: one launch
  {
    ga_members_loss_args a = {};
    a.kind = 0; a.A = 1; a.algo = 1;
    ga_member_loss one = {dummy, 1, dummy, 1, nullptr, dummy, dummy, 256, 0.f, 0.f, out32, nullptr};
    reset();
    CHECK(ga_ppo_loss_members_f32(&a, &one, 1, part.p, 2, nullptr) == 0);
    CHECK(g_md.size() == 1 && g_md[0].ppo[0].p.loss_out == out32);
  }
  // value loss
  {
    std::vector<ga_member_nll> mem((size_t)n);
    for (int64_t m = 0; m < n; ++m)
      mem[(size_t)m] = {dummy + m, 1 + m, dummy, dummy, rows[(size_t)m], out32 + m};
    reset();
    CHECK(ga_gaussian_nll_members_f32(mem.data(), n, part.p, need, nullptr) == 0);
    CHECK(g_md.size() == 2 && g_copies.size() == 1 && g_md[0].gx == 4 && g_md[1].n == 2);
    std::vector<std::pair<const double*, int64_t>> st;
    for (int64_t m = 0; m < n; ++m) {
      const MdNllEntry& e = g_md[0].nll[(size_t)m];
      const unsigned nb = (unsigned)ga_red_blocks(rows[(size_t)m]);
      CHECK(e.nb == nb && e.p.v == dummy + m && e.p.ldv == 1 + m && e.p.M == rows[(size_t)m]);
      CHECK((e.p.loss_out == out32 + m) == (nb == 1) && !e.p.dv && !e.p.idx);
      st.push_back({e.p.partials, 2 * (int64_t)nb});
    }
    check_partials(st, part);
    CHECK(g_md[1].nll_fin[1].nblocks == 4 && g_md[1].nll_fin[1].loss_out == out32 + 3);
  }
  // KL: one double per block, always a second launch
  for (int cat : {0, 1}) {
    std::vector<ga_member_kl> mem((size_t)n);
    for (int64_t m = 0; m < n; ++m)
      mem[(size_t)m] = {dummy, dummy + 1, 4, rows[(size_t)m], 0.5f, 0.25f * (float)m, out64 + m};
    Buf<double> half(need / 2);
    reset();
    CHECK(ga_kl_members_f32(cat, 3, 1, mem.data(), n, half.p, need / 2, nullptr) == 0);
    CHECK(g_md.size() == 2 && g_copies.size() == 1 && g_md[0].sub == cat && g_md[0].gx == 4);
    CHECK(g_md[1].n == n);
    std::vector<std::pair<const double*, int64_t>> st;
    for (int64_t m = 0; m < n; ++m) {
      const MdKlEntry& e = g_md[0].kl[(size_t)m];
      CHECK(e.nb == (unsigned)ga_red_blocks(rows[(size_t)m]) && e.M == rows[(size_t)m] &&
            e.A == 3 && e.dbl == 1 && e.s_old == 0.5f && e.s_new == 0.25f * (float)m);
      const MdSum& q = g_md[1].sum[(size_t)m];
      CHECK(q.partials == e.partials && q.nblocks == (int)e.nb && q.out == out64 + m);
      st.push_back({e.partials, (int64_t)e.nb});
    }
    check_partials(st, half);
    reset();
    CHECK(ga_kl_members_f32(cat, 3, 1, mem.data(), n, half.p, need / 2 - 1, nullptr) < 0);
    CHECK(g_md.empty() && g_copies.empty());
  }
  // episodes
  {
    int64_t off[4] = {0, 2, 5, 9};
    uint8_t st[9] = {0};
    ga_member_episodes mem[2] = {{dummy, off, 3, dummy, st, out64}, {dummy, off, 300, dummy, st, out64}};
    reset();
    CHECK(ga_episode_stats_members_f32(mem, 2, 2, nullptr) == 0);
    CHECK(g_md.size() == 1 && g_copies.size() == 1 && g_md[0].gx == 2 && g_md[0].n == 2);
    CHECK(g_md[0].eps[0].n_eps == 3 && g_md[0].eps[1].terminal == 2 &&
          g_md[0].eps[0].step_types == st && g_md[0].eps[0].out == out64);
  }
}

// ---- every refusal comes before any copy or launch ------------------------------------------
#define REFUSED(call, text)                                                        \
  do {                                                                             \
    reset();                                                                       \
    CHECK((call) < 0);                                                             \
    CHECK(g_md.empty() && g_copies.empty() && g_lone.empty());                     \
    CHECK(g_error.find(text) != std::string::npos);                                \
  } while (0)

static void suite_errors() {
  Net net(4, 64, 2);
  Buf<float> params(net.n_flat), X(16 * 4), acts(16 * net.act_width), out(16 * net.ld_out);
  Buf<double> part(64);
  const ga_member_forward good = {params.p, X.p, 4, 16, acts.p, out.p, net.ld_out};
  std::vector<ga_member_forward> many(2049, good);
  ga_member_forward u = good;
  REFUSED(ga_mlp_forward_members_f32(nullptr, &good, 1, nullptr), "null pointer");
  REFUSED(ga_mlp_forward_members_f32(&net.d, nullptr, 1, nullptr), "null pointer");
  REFUSED(ga_mlp_forward_members_f32(&net.d, &good, 0, nullptr), "n_members must be");
  REFUSED(ga_mlp_forward_members_f32(&net.d, many.data(), 2049, nullptr), "n_members must be");
  u = good; u.rows = 0;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "bad rows");
  u = good; u.rows = 1ll << 31;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "bad rows");
  u = good; u.acts = nullptr;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "member 0: null pointer");
  u = good; u.ldx = 6;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "16-B aligned quads");
  u = good; u.X = X.p + 1;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "16-B aligned quads");
  u = good; u.ldo = 0;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &u, 1, nullptr), "16-B aligned quads");
  {
    // the second member is the bad one: the first is not launched either
    ga_member_forward two[2] = {good, good};
    two[1].out = nullptr;
    REFUSED(ga_mlp_forward_members_f32(&net.d, two, 2, nullptr), "member 1: null pointer");
  }
  g_members_ok = 0;
  REFUSED(ga_mlp_forward_members_f32(&net.d, &good, 1, nullptr), "unsupported network");
  g_members_ok = 1;
  Net wide(4, 128, 2);
  REFUSED(ga_mlp_forward_members_f32(&wide.d, &good, 1, nullptr), "unsupported network");
  // the whole-network forward is no per-layer launch, and the predicate says so beforehand
  CHECK(ga_mlp_forward_members_supported(&net.d) == 1);
  ga_set_fused_forward(1);
  REFUSED(ga_mlp_forward_members_f32(&net.d, &good, 1, nullptr), "ga_set_fused_forward");
  reset();
  CHECK(ga_mlp_forward_members_supported(&net.d) == 0);
  CHECK(g_error.find("ga_set_fused_forward") != std::string::npos);
  ga_set_fused_forward(0);
  CHECK(ga_mlp_forward_members_supported(&net.d) == 1);
  CHECK(ga_mlp_forward_members_supported(&wide.d) == 0);
  CHECK(ga_mlp_forward_members_supported(nullptr) == 0);
  CHECK(g_md.empty() && g_lone.empty());

  float f[4] = {0};
  double d[4] = {0};
  ga_members_loss_args a = {};
  a.kind = 0; a.A = 2; a.algo = 0;
  const ga_member_loss lgood = {f, 2, f, 2, f, f, f, 10, 0.2f, 0.f, f, d};
  ga_member_loss l = lgood;
  REFUSED(ga_ppo_loss_members_f32(nullptr, &lgood, 1, part.p, 64, nullptr), "null pointer");
  REFUSED(ga_ppo_loss_members_f32(&a, nullptr, 1, part.p, 64, nullptr), "null pointer");
  REFUSED(ga_ppo_loss_members_f32(&a, &lgood, 0, part.p, 64, nullptr), "n_members must be");
  REFUSED(ga_ppo_loss_members_f32(&a, &lgood, 1, nullptr, 64, nullptr), "partials must be");
  a.kind = 1;
  REFUSED(ga_ppo_loss_members_f32(&a, &lgood, 1, part.p, 64, nullptr), "kind must be");
  a.kind = 0; a.algo = 2;
  REFUSED(ga_ppo_loss_members_f32(&a, &lgood, 1, part.p, 64, nullptr), "algo must be");
  a.algo = 0; a.A = 9;
  REFUSED(ga_ppo_loss_members_f32(&a, &lgood, 1, part.p, 64, nullptr), "A must be");
  a.A = 2;
  l = lgood; l.old_ll = nullptr;
  REFUSED(ga_ppo_loss_members_f32(&a, &l, 1, part.p, 64, nullptr), "PPO needs old_ll");
  l = lgood; l.log_std = nullptr;
  REFUSED(ga_ppo_loss_members_f32(&a, &l, 1, part.p, 64, nullptr), "member 0: null pointer");
  l = lgood; l.rows = 0;
  REFUSED(ga_ppo_loss_members_f32(&a, &l, 1, part.p, 64, nullptr), "bad rows");
  l = lgood; l.ld = 1;
  REFUSED(ga_ppo_loss_members_f32(&a, &l, 1, part.p, 64, nullptr), "bad strides");
  l = lgood; l.lda = 1;
  REFUSED(ga_ppo_loss_members_f32(&a, &l, 1, part.p, 64, nullptr), "bad strides");

  const ga_member_nll ngood = {f, 1, f, f, 10, f};
  ga_member_nll nl = ngood;
  std::vector<ga_member_nll> nmany(1025, ngood);
  REFUSED(ga_gaussian_nll_members_f32(nullptr, 1, part.p, 64, nullptr), "null pointer");
  REFUSED(ga_gaussian_nll_members_f32(nmany.data(), 1025, part.p, 64, nullptr),
          "n_members must be");
  nl = ngood; nl.returns = nullptr;
  REFUSED(ga_gaussian_nll_members_f32(&nl, 1, part.p, 64, nullptr), "member 0: null pointer");
  nl = ngood; nl.rows = -1;
  REFUSED(ga_gaussian_nll_members_f32(&nl, 1, part.p, 64, nullptr), "bad rows");
  nl = ngood; nl.ldv = 0;
  REFUSED(ga_gaussian_nll_members_f32(&nl, 1, part.p, 64, nullptr), "bad strides");
  REFUSED(ga_gaussian_nll_members_f32(&ngood, 1, part.p, 1, nullptr), "partials too small");

  const ga_member_kl kgood = {f, f, 2, 10, 0.f, 0.f, d};
  ga_member_kl k = kgood;
  REFUSED(ga_kl_members_f32(0, 2, 0, nullptr, 1, part.p, 64, nullptr), "null pointer");
  REFUSED(ga_kl_members_f32(0, 0, 0, &kgood, 1, part.p, 64, nullptr), "A must be");
  k = kgood; k.kl_sum_out = nullptr;
  REFUSED(ga_kl_members_f32(0, 2, 0, &k, 1, part.p, 64, nullptr), "member 0: null pointer");
  k = kgood; k.rows = 0;
  REFUSED(ga_kl_members_f32(1, 2, 0, &k, 1, part.p, 64, nullptr), "bad rows");
  k = kgood; k.ld = 1;
  REFUSED(ga_kl_members_f32(1, 2, 0, &k, 1, part.p, 64, nullptr), "bad strides");

  int64_t off[2] = {0, 1};
  uint8_t st[1] = {0};
  const ga_member_episodes egood = {f, off, 1, f, st, d};
  ga_member_episodes e = egood;
  REFUSED(ga_episode_stats_members_f32(nullptr, 1, 2, nullptr), "null pointer");
  REFUSED(ga_episode_stats_members_f32(&egood, 1025, 2, nullptr), "n_members must be");
  e = egood; e.step_types = nullptr;
  REFUSED(ga_episode_stats_members_f32(&e, 1, 2, nullptr), "member 0: null pointer");
  e = egood; e.n_eps = 0;
  REFUSED(ga_episode_stats_members_f32(&e, 1, 2, nullptr), "bad n_eps");

  const int64_t bad_rows[2] = {5, 0};
  CHECK(ga_members_diag_partials_doubles(bad_rows, 2) == 0);
  CHECK(ga_members_diag_partials_doubles(nullptr, 2) == 0);
  CHECK(ga_members_diag_partials_doubles(bad_rows, 0) == 0);
  CHECK(ga_members_diag_partials_doubles(bad_rows, 1) == 2);

  // a launch that fails: the error comes back, the later launches are not made, the
  // tables' slot is still marked done
  reset();
  g_fail_launch = 1;
  const int recorded = g_events_recorded;
  CHECK(ga_mlp_forward_members_f32(&net.d, &good, 1, nullptr) == GA_ERR_HIP);
  CHECK(g_md.size() == 2 && g_md[1].what == "failed");
  CHECK(g_events_recorded == recorded + 1);
  reset();
  ga_members_diag_release();
}

int main(int argc, char** argv) {
  return run_suites({{"forward", suite_forward, "members diag forward ok"},
                     {"losses", suite_losses, "members diag losses ok"},
                     {"errors", suite_errors, "members diag errors ok"}},
                    argc, argv);
}
