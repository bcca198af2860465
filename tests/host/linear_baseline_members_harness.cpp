// Host-logic harness for the population's entry points of the linear feature baseline
// (garage_amd/csrc/linear_baseline_members_host.cpp), built with
// -fsanitize=address,undefined on the CPU (`make asan-linear-baseline-members`).  The three
// launches of the seam (linear_baseline_params.h) are replaced by recording fakes and the
// HIP runtime by harness.h's; "device" memory is exactly-sized host memory, and each fake
// walks the member table as its kernel would -- every workgroup of the flat grid finds its
// member through the prefix table and touches the first and the last byte it would reach --
// so that a grid, a prefix, a stretch of the workspace or a table size that is off trips
// the sanitizer.  The checks are about the host's own work: every refusal precedes the
// first copy and launch, the grids and prefix tables of uneven members (a member beyond
// LB_MAX_BLOCKS slabs included), the workspace bound, one table copy and one event a call.
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/linear_baseline_params.h"
#include "harness.h"

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "fake"; }
}

// ---- what the fakes record -----------------------------------------------------
struct GramLaunch {
  LinGramMembersParams p;
  std::vector<LinGramMemberDev> table;
  unsigned blocks, lds;
};
struct PredictLaunch {
  LinPredictMembersParams p;
  std::vector<LinPredictMemberDev> table;
  unsigned blocks;
};
static std::vector<GramLaunch> g_gram, g_reduce;
static std::vector<PredictLaunch> g_predict;
static hipStream_t g_stream_seen = nullptr;

static void touch(const void* p, int64_t at) {
  volatile char c = static_cast<const char*>(p)[at];
  (void)c;
}
static void touch_batch(const float* obs, int64_t ldo, int obs_dim, const int64_t* ep_off,
                        int64_t n_eps, int64_t S) {
  touch(obs, 0);
  touch(obs, ((S - 1) * ldo + obs_dim) * 4 - 1);
  touch(ep_off, 0);
  touch(ep_off, (n_eps + 1) * 8 - 1);
}
// the kernels' search: the last member whose first workgroup is not beyond `block`
template <class Member>
static int member_of(const Member* members, int n, int64_t block) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)members[mid].block0 <= block) lo = mid; else hi = mid;
  }
  return lo;
}

void lb_launch_gram_members(const LinGramMembersParams& p, unsigned blocks, unsigned lds_bytes,
                            hipStream_t stream) {
  CHECK(g_copies.size() == 1);  // the table is on the "device" before the launch
  GramLaunch l{p, {}, blocks, lds_bytes};
  for (int m = 0; m < p.n_members; ++m) l.table.push_back(p.members[m]);
  g_gram.push_back(l);
  g_stream_seen = stream;
  std::vector<int> seen(p.n_members, 0);
  int64_t slabs_done = 0, slabs = 0;
  for (unsigned b = 0; b < blocks; ++b) {
    const int m = member_of(p.members, p.n_members, b);
    const LinGramMemberDev& t = p.members[m];
    const int rel = (int)b - t.block0;
    CHECK(rel >= 0 && rel < t.n_blocks);
    ++seen[m];
    // the slabs this workgroup takes: rel, rel + n_blocks, ..
    for (int64_t slab = rel; slab < t.n_slabs; slab += t.n_blocks) {
      const int64_t row0 = slab * LB_SLAB_ROWS;
      CHECK(row0 < t.S);
      const int64_t last = row0 + LB_SLAB_ROWS < t.S ? row0 + LB_SLAB_ROWS - 1 : t.S - 1;
      touch(t.obs, (row0 * t.ldo) * 4);
      touch(t.obs, (last * t.ldo + p.obs_dim) * 4 - 1);
      touch(t.returns, row0 * 4);
      touch(t.returns, last * 4 + 3);
      ++slabs_done;
    }
    touch(t.partials, (int64_t)rel * p.block_doubles * 8);
    touch(t.partials, (int64_t)(rel + 1) * p.block_doubles * 8 - 1);
  }
  for (int m = 0; m < p.n_members; ++m) {
    const LinGramMemberDev& t = p.members[m];
    CHECK(seen[m] == t.n_blocks);  // every workgroup of the member, no other
    touch_batch(t.obs, t.ldo, p.obs_dim, t.ep_off, t.n_eps, t.S);
    slabs += t.n_slabs;
  }
  CHECK(slabs_done == slabs);  // every slab of every member exactly once
  CHECK(p.tpw * LB_WAVES >= p.NT && p.tpw >= 1 && p.tpw <= LB_MAX_TPW);
  CHECK(p.chunk_rows == 8 || p.chunk_rows == 16 || p.chunk_rows == 32);
  CHECK(lds_bytes <= LB_LDS_BUDGET);
  CHECK(16 * p.T <= LB_THREADS && 16 * p.T >= p.F && 16 * (p.T - 1) < p.F);
}
void lb_launch_gram_reduce_members(const LinGramMembersParams& p, unsigned blocks,
                                   hipStream_t stream) {
  CHECK(g_gram.size() == g_reduce.size() + 1);  // after the Gram pass, on the stream
  CHECK(stream == g_stream_seen);
  GramLaunch l{p, {}, blocks, 0};
  g_reduce.push_back(l);
  for (int m = 0; m < p.n_members; ++m) {  // (row m of the grid)
    const LinGramMemberDev& t = p.members[m];
    touch(t.partials, (int64_t)t.n_blocks * p.block_doubles * 8 - 1);
    touch(t.gram, 0);
    touch(t.gram, (int64_t)p.F * p.F * 8 - 1);
    touch(t.rhs, 0);
    touch(t.rhs, (int64_t)p.F * 8 - 1);
  }
  CHECK((int64_t)blocks * LB_REDUCE_THREADS >= p.block_doubles);
  CHECK((int64_t)(blocks - 1) * LB_REDUCE_THREADS < p.block_doubles);
}
void lb_launch_predict_members(const LinPredictMembersParams& p, unsigned blocks,
                               hipStream_t stream) {
  CHECK(g_copies.size() == 1);
  PredictLaunch l{p, {}, blocks};
  for (int m = 0; m < p.n_members; ++m) l.table.push_back(p.members[m]);
  g_predict.push_back(l);
  g_stream_seen = stream;
  // the first and the last workgroup of every member (the grids are large)
  int64_t total = 0;
  for (int m = 0; m < p.n_members; ++m) {
    const LinPredictMemberDev& t = p.members[m];
    const int64_t n = (t.S + LB_PREDICT_THREADS - 1) / LB_PREDICT_THREADS;
    CHECK(t.block0 == total);
    CHECK(member_of(p.members, p.n_members, t.block0) == m);
    CHECK(member_of(p.members, p.n_members, t.block0 + n - 1) == m);
    total += n;
    touch_batch(t.obs, t.ldo, p.obs_dim, t.ep_off, t.n_eps, t.S);
    if (t.coeffs) touch(t.coeffs, (2 * p.obs_dim + 4) * 8 - 1);
    touch(t.values, 0);
    touch(t.values, ((t.S - 1) * t.ldv + 1) * 4 - 1);
  }
  CHECK(total == (int64_t)blocks);
}

static void reset() {
  ga_linear_members_release();  // every call allocates its table afresh
  g_gram.clear(); g_reduce.clear(); g_predict.clear(); g_error.clear();
  g_host_allocs.clear(); g_dev_allocs.clear(); g_copies.clear();
  g_events_recorded = 0;
  g_log.clear();
  g_stream_seen = nullptr;
}

// ---- a population over exactly-sized buffers ---------------------------------------------
struct Pop {
  int obs_dim = 17;
  std::vector<int64_t> S, ldo, ldv, n_eps;
  std::vector<ga_linear_gram_member> gram;
  std::vector<ga_linear_predict_member> pred;
  double* workspace = nullptr;
  int64_t workspace_doubles = 0;
  bool null_members = false;
  std::vector<void*> owned;
  template <class T>
  T* make(int64_t n) {
    void* p = malloc((size_t)(n > 0 ? n : 1) * sizeof(T));
    owned.push_back(p);
    return static_cast<T*>(p);
  }
  Pop(int obs_dim_, std::vector<int64_t> S_) : obs_dim(obs_dim_), S(S_) {
    const int F = 2 * obs_dim + 4;
    for (size_t m = 0; m < S.size(); ++m) {
      ldo.push_back(obs_dim + (int64_t)(m % 3));  // some wider than obs_dim
      ldv.push_back(1 + (int64_t)(m % 2));
      n_eps.push_back(S[m] < 3 ? 1 : 3);
      ga_linear_gram_member g;
      g.obs = make<float>((S[m] - 1) * ldo[m] + obs_dim);  // the last row has no padding
      g.ldo = ldo[m];
      g.ep_off = make<int64_t>(n_eps[m] + 1);
      g.n_eps = n_eps[m]; g.S = S[m];
      g.returns = make<float>(S[m]);
      g.gram = make<double>((int64_t)F * F);
      g.rhs = make<double>(F);
      gram.push_back(g);
      ga_linear_predict_member q;
      q.obs = g.obs; q.ldo = g.ldo; q.ep_off = g.ep_off; q.n_eps = g.n_eps; q.S = g.S;
      q.coeffs = m % 4 == 3 ? nullptr : make<double>(F);  // (a member not fitted yet)
      q.values = make<float>((S[m] - 1) * ldv[m] + 1);
      q.ldv = ldv[m];
      pred.push_back(q);
    }
    workspace_doubles =
        ga_linear_gram_members_workspace_doubles(obs_dim, (int64_t)S.size(), S.data());
    workspace = make<double>(workspace_doubles > 0 ? workspace_doubles : 1);
  }
  int gram_run() {
    return ga_linear_features_gram_members_f64(null_members ? nullptr : gram.data(),
                                               (int64_t)gram.size(), obs_dim,
                                               workspace, workspace_doubles,
                                               (ga_stream_t)0x40);
  }
  int predict_run() {
    return ga_linear_features_predict_members_f32(null_members ? nullptr : pred.data(),
                                                  (int64_t)pred.size(), obs_dim,
                                                  (ga_stream_t)0x40);
  }
  ~Pop() { for (void* p : owned) free(p); }
};

// the Gram pass of members of S rows: want_blocks[m] workgroups each
static void check_gram(int obs_dim, std::vector<int64_t> S, std::vector<int> want_blocks,
                       int64_t block_doubles) {
  reset();
  Pop pop(obs_dim, S);
  const int n = (int)S.size();
  int64_t total = 0;
  for (int b : want_blocks) total += b;
  CHECK(pop.workspace_doubles == total * block_doubles);
  CHECK(pop.gram_run() == 0);
  CHECK(g_gram.size() == 1 && g_reduce.size() == 1 && g_predict.empty());
  if (g_gram.size() != 1 || g_reduce.size() != 1) return;
  // one table: one pinned and one device allocation of exactly its bytes, one copy, one event
  const size_t bytes = n * sizeof(LinGramMemberDev);
  CHECK(g_host_allocs.size() == 1 && g_host_allocs[0] == bytes);
  CHECK(g_dev_allocs.size() == 1 && g_dev_allocs[0] == bytes);
  CHECK(g_copies.size() == 1 && g_copies[0] == bytes);
  CHECK(g_events_recorded == 1);
  CHECK(g_stream_seen == (hipStream_t)0x40);
  const GramLaunch& l = g_gram[0];
  CHECK(l.blocks == (unsigned)total && l.p.n_members == n && l.p.obs_dim == obs_dim);
  CHECK(l.p.block_doubles == block_doubles && l.p.F == 2 * obs_dim + 4);
  CHECK(l.lds == lb_gram_lds_bytes(obs_dim, l.p.chunk_rows));
  CHECK(g_reduce[0].blocks == (unsigned)((block_doubles + 255) / 256));
  CHECK(g_reduce[0].p.members == l.p.members);
  int64_t block0 = 0;
  for (int m = 0; m < n; ++m) {
    const LinGramMemberDev& t = l.table[m];
    const ga_linear_gram_member& u = pop.gram[m];
    CHECK(t.obs == u.obs && t.ldo == u.ldo && t.ep_off == u.ep_off && t.n_eps == u.n_eps);
    CHECK(t.S == u.S && t.returns == u.returns && t.gram == u.gram && t.rhs == u.rhs);
    CHECK(t.n_blocks == want_blocks[m] && t.block0 == block0);
    CHECK(t.n_slabs == (S[m] + 2047) / 2048);
    CHECK(t.partials == pop.workspace + block0 * block_doubles);  // the members' stretches
    block0 += t.n_blocks;                                         // neither overlap nor gap
  }
}

static void check_predict(int obs_dim, std::vector<int64_t> S, unsigned blocks) {
  reset();
  Pop pop(obs_dim, S);
  const int n = (int)S.size();
  CHECK(pop.predict_run() == 0);
  CHECK(g_predict.size() == 1 && g_gram.empty() && g_reduce.empty());
  if (g_predict.size() != 1) return;
  const size_t bytes = n * sizeof(LinPredictMemberDev);
  CHECK(g_host_allocs.size() == 1 && g_host_allocs[0] == bytes);
  CHECK(g_copies.size() == 1 && g_copies[0] == bytes);
  CHECK(g_events_recorded == 1);
  CHECK(g_predict[0].blocks == blocks && g_predict[0].p.n_members == n);
  CHECK(g_predict[0].p.obs_dim == obs_dim);
  for (int m = 0; m < n; ++m) {
    const LinPredictMemberDev& t = g_predict[0].table[m];
    const ga_linear_predict_member& u = pop.pred[m];
    CHECK(t.obs == u.obs && t.ldo == u.ldo && t.ep_off == u.ep_off && t.n_eps == u.n_eps);
    CHECK(t.S == u.S && t.coeffs == u.coeffs && t.values == u.values && t.ldv == u.ldv);
  }
}

template <class F>
static void refused(const char* what, bool gram, F&& spoil) {
  reset();
  Pop pop(17, {100, 2049, 7, 300});
  spoil(pop);
  const int rc = gram ? pop.gram_run() : pop.predict_run();
  const bool ok = rc < 0 && !g_error.empty() && g_gram.empty() && g_reduce.empty() &&
                  g_predict.empty() && g_copies.empty() && g_events_recorded == 0;
  if (!ok)
    fprintf(stderr, "%s not refused: %s (rc %d, '%s')\n", gram ? "gram" : "predict", what, rc,
            g_error.c_str());
  CHECK(ok);
}
template <class F>
static void both_refused(const char* what, F&& spoil) {
  refused(what, true, spoil);
  refused(what, false, spoil);
}
template <class T>
static T* off4(T* p) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 4);
}

int main() {
  {
    const int64_t S[3] = {100, 2049, 1};
    CHECK(ga_linear_gram_members_workspace_doubles(17, 3, S) == 4 * 1584);
    CHECK(ga_linear_gram_members_workspace_doubles(0, 3, S) == -1);
    CHECK(ga_linear_gram_members_workspace_doubles(129, 3, S) == -1);
    CHECK(ga_linear_gram_members_workspace_doubles(17, 0, S) == -1);
    CHECK(ga_linear_gram_members_workspace_doubles(17, 1025, S) == -1);
    CHECK(ga_linear_gram_members_workspace_doubles(17, 3, nullptr) == -1);
    const int64_t bad[2] = {5, 0}, big[2] = {5, 1ll << 31};
    CHECK(ga_linear_gram_members_workspace_doubles(17, 2, bad) == -1);
    CHECK(ga_linear_gram_members_workspace_doubles(17, 2, big) == -1);
  }
  //         obs   members' rows                 their workgroups     block doubles
  check_gram(1, {1}, {1}, 272);
  check_gram(2, {2047, 2048, 2049}, {1, 1, 2}, 272);
  check_gram(1, {1, 1, 2}, {1, 1, 1}, 272);
  check_gram(17, {100, 2049, 7, 6145, 1}, {1, 2, 1, 4, 1}, 1584);
  check_gram(128, {100, 100, 37, 9}, {1, 1, 1, 1}, 39440);
  // a member beyond the cap of a lone grid (workgroup 0 of its 1024 takes slabs 0 and
  // 1024) between two small ones: its stride is its own 1024, not the grid's 1026
  check_gram(1, {5, 2048ll * 1024 + 1, 5}, {1, 1024, 1}, 272);
  {
    std::vector<int64_t> S(1024, 3);  // the most members
    std::vector<int> blocks(1024, 1);
    S[1023] = 4097; blocks[1023] = 3;
    check_gram(4, S, blocks, 272);
  }

  check_predict(17, {1}, 1);
  check_predict(17, {256, 257, 1, 1000}, 1 + 2 + 1 + 4);
  check_predict(128, {1000, 3}, 4 + 1);
  check_predict(1, {5, 2048ll * 1024 + 1, 5}, 1 + 8193 + 1);

  both_refused("null members", [](Pop& p) { p.null_members = true; });
  both_refused("null obs", [](Pop& p) { p.gram[2].obs = nullptr; p.pred[2].obs = nullptr; });
  both_refused("null ep_off", [](Pop& p) {
    p.gram[3].ep_off = nullptr; p.pred[3].ep_off = nullptr;
  });
  both_refused("obs_dim 0", [](Pop& p) { p.obs_dim = 0; });
  both_refused("obs_dim 129", [](Pop& p) { p.obs_dim = 129; });
  both_refused("ldo < obs_dim", [](Pop& p) { p.gram[1].ldo = 16; p.pred[1].ldo = 16; });
  both_refused("S = 0", [](Pop& p) { p.gram[0].S = 0; p.pred[0].S = 0; });
  both_refused("S = 2^31", [](Pop& p) { p.gram[3].S = 1ll << 31; p.pred[3].S = 1ll << 31; });
  both_refused("n_eps = 0", [](Pop& p) { p.gram[1].n_eps = 0; p.pred[1].n_eps = 0; });
  both_refused("n_eps > S", [](Pop& p) { p.gram[2].n_eps = 8; p.pred[2].n_eps = 8; });
  refused("null returns", true, [](Pop& p) { p.gram[1].returns = nullptr; });
  refused("null gram", true, [](Pop& p) { p.gram[3].gram = nullptr; });
  refused("null rhs", true, [](Pop& p) { p.gram[0].rhs = nullptr; });
  refused("null workspace", true, [](Pop& p) { p.workspace = nullptr; });
  refused("misaligned gram", true, [](Pop& p) { p.gram[2].gram = off4(p.gram[2].gram); });
  refused("misaligned rhs", true, [](Pop& p) { p.gram[2].rhs = off4(p.gram[2].rhs); });
  refused("misaligned workspace", true, [](Pop& p) { p.workspace = off4(p.workspace); });
  refused("small workspace", true, [](Pop& p) { p.workspace_doubles -= 1; });
  refused("null values", false, [](Pop& p) { p.pred[1].values = nullptr; });
  refused("misaligned coeffs", false, [](Pop& p) { p.pred[0].coeffs = off4(p.pred[0].coeffs); });
  refused("ldv = 0", false, [](Pop& p) { p.pred[2].ldv = 0; });
  // n_members outside 1 .. 1024 (the arrays are not looked at)
  {
    reset();
    Pop pop(17, {100});
    CHECK(ga_linear_features_gram_members_f64(pop.gram.data(), 0, 17, pop.workspace,
                                              pop.workspace_doubles, nullptr) < 0);
    CHECK(ga_linear_features_gram_members_f64(pop.gram.data(), 1025, 17, pop.workspace,
                                              pop.workspace_doubles, nullptr) < 0);
    CHECK(ga_linear_features_predict_members_f32(pop.pred.data(), 0, 17, nullptr) < 0);
    CHECK(ga_linear_features_predict_members_f32(pop.pred.data(), 1025, 17, nullptr) < 0);
    CHECK(g_copies.empty() && g_gram.empty() && g_predict.empty());
  }
  // more workgroups than one grid holds: 1024 members of 2^31 - 1 rows each
  {
    reset();
    Pop pop(1, {100});
    std::vector<ga_linear_predict_member> many(1024, pop.pred[0]);
    for (auto& u : many) { u.S = (1ll << 31) - 1; u.n_eps = 1; }
    CHECK(ga_linear_features_predict_members_f32(many.data(), 1024, 1, nullptr) < 0);
    CHECK(g_copies.empty() && g_predict.empty() && !g_error.empty());
  }
  reset();
  return finish("linear baseline members ok");
}
