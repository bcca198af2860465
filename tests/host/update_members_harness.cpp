// Host-logic harness for the population's epoch loop (garage_amd/csrc/update_members.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-members`).  The two
// launches of a step and the HIP runtime calls the loop makes are replaced by fakes:
// "device" memory is exactly-sized host memory, a copy happens at once, and each fake
// launch walks what its kernel would touch -- the ids of every active member's step,
// its tiles' shares inside the partials buffer, its Adam constants, its loss slot -- so
// that an extent that is off by one trips the sanitizer.  The checks are about the
// loop's own arithmetic: which ids form member m's step k, which members are active in
// which step, the Adam table, the launch count of a pass, the tables' sizes, and that
// nothing is launched after a refusal.
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/members_step.h"
#include "../../garage_amd/csrc/shape_rules.h"
#include "harness.h"

// ---- what the fakes record -----------------------------------------------------
struct StepRecord {
  int64_t k, max_tiles;
  std::vector<int> active;        // members with rows in this step
  std::vector<int64_t> rows;      // ... and how many
  std::vector<long long> id_sum;  // ... and the sum of their ids
};
static std::vector<StepRecord> g_train, g_reduce;
// the host's view of the pass under test (for the reduce fake's Adam check)
static const ga_update_members_args* g_args = nullptr;

// ---- kernel-side fakes (the shape rules: csrc/shape_rules.h) ----------------------------------
extern "C" {
static int64_t rows_of(const GaMemberDev& m, int64_t mb, int64_t k) {
  if (k >= m.n_steps) return 0;
  return k == m.n_steps - 1 ? m.last_M : mb;
}

int ga_members_train_step(const GaMembersShared* sh, const GaMemberDev* table, int64_t k,
                          int64_t max_tiles, hipStream_t) {
  StepRecord r;
  r.k = k; r.max_tiles = max_tiles;
  for (int m = 0; m < sh->n_members; ++m) {
    const GaMemberDev& t = table[m];
    const int64_t M = rows_of(t, sh->mb, k);
    if (M <= 0) continue;
    long long sum = 0;
    for (int64_t i = 0; i < M; ++i) sum += t.perm ? t.perm[k * sh->mb + i] : i;
    const int64_t tiles = ga_fused_tiles(M);
    CHECK(tiles <= max_tiles);
    for (int64_t tile = 0; tile < tiles; ++tile) {  // what a tile writes
      for (int64_t e = 0; e < sh->stride; ++e) t.part[tile * sh->stride + e] = 1.f;
      t.lpart[2 * tile] = 1.0; t.lpart[2 * tile + 1] = 1.0;
    }
    CHECK(t.inv_last == 1.f / (float)t.last_M);
    CHECK(t.n_steps == 1 || t.inv_full == 1.f / (float)sh->mb);
    r.active.push_back(m); r.rows.push_back(M); r.id_sum.push_back(sum);
  }
  g_train.push_back(r);
  return 0;
}

int ga_members_reduce_adam(const GaMembersShared* sh, const GaMemberDev* table,
                           const GaAdam* adam, int64_t k, int64_t max_tiles, hipStream_t) {
  StepRecord r;
  r.k = k; r.max_tiles = max_tiles;
  for (int m = 0; m < sh->n_members; ++m) {
    const GaAdam got = adam[m];  // (every slot of the step's row is readable)
    const GaMemberDev& t = table[m];
    const int64_t M = rows_of(t, sh->mb, k);
    if (M <= 0) continue;
    const ga_member_update& u = g_args->members_host[m];
    const GaAdam want =
        ga_adam_coeffs(u.lr, g_args->beta1, g_args->beta2, g_args->eps, u.step0 + k + 1);
    CHECK(memcmp(&got, &want, sizeof(GaAdam)) == 0);
    if (t.losses) t.losses[k] = (float)M;
    r.active.push_back(m); r.rows.push_back(M);
  }
  g_reduce.push_back(r);
  return 0;
}
}  // extern "C"

// ---- a pass over exactly-sized buffers ------------------------------------------------
static const int64_t kS[5] = {130, 64, 200, 1, 65};
static const int64_t kStep0[5] = {0, 7, 1000, 3, 1};

static ga_mlp_desc make_desc(int in_w, int H, int out_w) {
  ga_mlp_desc d;
  memset(&d, 0, sizeof(d));
  d.n_layers = 3;
  d.dims[0] = in_w; d.dims[1] = H; d.dims[2] = H; d.dims[3] = out_w;
  int64_t off = 4;
  for (int l = 0; l < 3; ++l) {
    d.w_off[l] = off; off += (int64_t)d.dims[l + 1] * ((d.dims[l] + 3) & ~3);
    d.b_off[l] = off; off += (d.dims[l + 1] + 3) & ~3;
  }
  return d;
}

struct Pass {
  ga_mlp_desc desc;
  ga_update_members_args a;
  std::vector<ga_member_update> mem;
  std::vector<int32_t*> perms;
  std::vector<float*> losses;
  float* partials = nullptr;
  float* flat = nullptr;   // stands for every float operand that is only passed on
  Pass(int n, int64_t mb, int kind) {
    desc = make_desc(4, 64, kind == 1 ? 1 : 2);
    memset(&a, 0, sizeof(a));
    a.desc = &desc; a.kind = kind; a.algo = 0; a.learn_std = 1;
    a.beta1 = 0.9; a.beta2 = 0.999; a.eps = 1e-8; a.mb = mb; a.n_members = n;
    flat = static_cast<float*>(aligned_alloc(16, 64));
    mem.resize(n);
    int64_t max_rows = 0;
    for (int m = 0; m < n; ++m) {
      ga_member_update& u = mem[m];
      memset(&u, 0, sizeof(u));
      u.params = u.grads = u.exp_avg = u.exp_avg_sq = flat;
      u.X = flat; u.ldx = 4; u.S = kS[m];
      int32_t* perm = static_cast<int32_t*>(malloc(sizeof(int32_t) * u.S));  // exactly S
      for (int64_t i = 0; i < u.S; ++i) perm[i] = (int32_t)((i * 7 + m) % u.S);
      perms.push_back(perm);
      u.perm = perm;
      u.actions = flat; u.lda = 4; u.old_ll = flat; u.adv = flat; u.returns = flat;
      u.step0 = kStep0[m]; u.lr = 1e-3 * (m + 1); u.clip = 0.2f;
      const int64_t steps = mb == 0 ? 1 : (u.S + mb - 1) / mb;
      float* l = static_cast<float*>(malloc(sizeof(float) * steps));  // exactly n_steps
      losses.push_back(l);
      u.losses = l;
      const int64_t rows = mb == 0 || u.S < mb ? u.S : mb;
      if (rows > max_rows) max_rows = rows;
    }
    a.members_host = mem.data();
    a.partials_floats = ga_update_members_partials_floats(&desc, n, max_rows);
    partials = static_cast<float*>(aligned_alloc(16, sizeof(float) * a.partials_floats));
    a.partials = partials;
  }
  ~Pass() {
    for (int32_t* p : perms) free(p);
    for (float* l : losses) free(l);
    free(partials);
    free(flat);
  }
};

static void reset() {
  ga_update_members_release();  // every pass allocates its tables afresh
  g_train.clear(); g_reduce.clear();
  g_host_allocs.clear(); g_dev_allocs.clear(); g_copies.clear();
  g_events_recorded = 0;
  g_log.clear();
  g_error.clear();
}

static void check_pass(int n, int64_t mb) {
  reset();
  Pass p(n, mb, 2);
  g_args = &p.a;
  int64_t largest = 0;  // rows of the largest minibatch of any member
  for (int m = 0; m < n; ++m) {
    const int64_t rows = mb == 0 || kS[m] < mb ? kS[m] : mb;
    if (rows > largest) largest = rows;
  }
  CHECK(p.a.partials_floats ==
        n * ga_fused_tiles(largest) * (4 + ga_narrow_step_stride(4, 64)));
  const int rc = ga_update_epoch_members(&p.a, nullptr);
  CHECK(rc == 0);
  int64_t steps[5], n_steps = 0;
  for (int m = 0; m < n; ++m) {
    steps[m] = mb == 0 ? 1 : (kS[m] + mb - 1) / mb;
    if (steps[m] > n_steps) n_steps = steps[m];
  }
  if (mb == 64 && n == 5) {
    const int64_t want[5] = {3, 1, 4, 1, 2};
    for (int m = 0; m < 5; ++m) CHECK(steps[m] == want[m]);
  }
  // the launch count of a pass: one pair per step of the longest member
  CHECK((int64_t)g_train.size() == n_steps && (int64_t)g_reduce.size() == n_steps);
  CHECK(g_events_recorded == 1);
  // the tables: one pinned and one device allocation of exactly the two tables' bytes,
  // one copy of both
  const size_t table_bytes = n * sizeof(GaMemberDev);
  const size_t adam_bytes = n_steps * n * sizeof(GaAdam);
  CHECK(g_host_allocs.size() == 1 && g_host_allocs[0] == table_bytes + adam_bytes);
  CHECK(g_dev_allocs.size() == 1 && g_dev_allocs[0] == table_bytes + adam_bytes);
  CHECK(g_copies.size() == 1 && g_copies[0] == table_bytes + adam_bytes);
  for (int64_t k = 0; k < n_steps; ++k) {
    const StepRecord& t = g_train[k];
    const StepRecord& r = g_reduce[k];
    CHECK(t.k == k && r.k == k);
    std::vector<int> active;
    int64_t max_rows = 0;
    for (int m = 0; m < n; ++m) {
      if (k >= steps[m]) continue;
      active.push_back(m);
      const int64_t lo = k * mb, hi = mb == 0 || lo + mb > kS[m] ? kS[m] : lo + mb;
      long long sum = 0;
      for (int64_t i = lo; i < hi; ++i) sum += p.perms[m][i];
      const size_t at = active.size() - 1;
      CHECK(at < t.active.size() && t.active[at] == m);
      CHECK(at < t.rows.size() && t.rows[at] == hi - lo);
      CHECK(at < t.id_sum.size() && t.id_sum[at] == sum);
      CHECK(p.losses[m][k] == (float)(hi - lo));
      if (hi - lo > max_rows) max_rows = hi - lo;
    }
    CHECK(t.active == active && r.active == active);
    CHECK(t.max_tiles == ga_fused_tiles(max_rows) && r.max_tiles == t.max_tiles);
  }
}

// a pass with one thing wrong: refused, with a message, before anything is launched
template <class F>
static void check_refused(const char* what, F&& spoil) {
  reset();
  Pass p(5, 64, 0);
  g_args = &p.a;
  const ga_update_members_args* args = &p.a;
  spoil(p, &args);
  const int rc = ga_update_epoch_members(args, nullptr);
  const bool refused = rc < 0 && !g_error.empty() && g_train.empty() && g_reduce.empty() &&
                       g_copies.empty();
  if (!refused) fprintf(stderr, "not refused: %s (rc %d, '%s')\n", what, rc, g_error.c_str());
  CHECK(refused);
}

// A slot is allocated to grow and when the device changes, never to shrink: eight
// passes fill the ring, the next eight (one step fewer, then the same again) allocate
// nothing, a longer pass grows its slot to exactly its size.
static void check_slot_reuse() {
  reset();
  g_device = 0;
  const size_t big = 5 * sizeof(GaMemberDev) + 4 * 5 * sizeof(GaAdam);  // mb = 64
  const size_t small = 5 * sizeof(GaMemberDev) + 2 * 5 * sizeof(GaAdam);  // mb = 100
  for (int i = 0; i < 8; ++i) {
    Pass p(5, 100, 2);
    g_args = &p.a;
    CHECK(ga_update_epoch_members(&p.a, nullptr) == 0);
  }
  CHECK(g_host_allocs.size() == 8 && g_dev_allocs.size() == 8);
  for (size_t b : g_host_allocs) CHECK(b == small);
  for (int i = 0; i < 8; ++i) {
    Pass p(5, i % 2 ? 100 : 0, 2);  // as many steps, or fewer
    g_args = &p.a;
    CHECK(ga_update_epoch_members(&p.a, nullptr) == 0);
  }
  CHECK(g_host_allocs.size() == 8 && g_dev_allocs.size() == 8);
  {
    Pass p(5, 64, 2);  // more steps: this slot grows
    g_args = &p.a;
    CHECK(ga_update_epoch_members(&p.a, nullptr) == 0);
  }
  CHECK(g_host_allocs.size() == 9 && g_host_allocs.back() == big);
  CHECK(g_dev_allocs.size() == 9 && g_dev_allocs.back() == big);
  g_device = 1;  // another device: the slot's memory is of no use there
  {
    Pass p(5, 0, 2);
    g_args = &p.a;
    CHECK(ga_update_epoch_members(&p.a, nullptr) == 0);
  }
  CHECK(g_host_allocs.size() == 10 && g_dev_allocs.size() == 10);
  g_device = 0;
  reset();
}

int main() {
  check_slot_reuse();
  for (int64_t mb : {(int64_t)0, (int64_t)64, (int64_t)100}) {
    check_pass(5, mb);
    check_pass(1, mb);
    check_pass(3, mb);
  }
  typedef const ga_update_members_args** Args;
  check_refused("null args", [](Pass&, Args a) { *a = nullptr; });
  check_refused("null desc", [](Pass& p, Args) { p.a.desc = nullptr; });
  check_refused("null members", [](Pass& p, Args) { p.a.members_host = nullptr; });
  check_refused("null partials", [](Pass& p, Args) { p.a.partials = nullptr; });
  check_refused("null params", [](Pass& p, Args) { p.mem[2].params = nullptr; });
  check_refused("null moments", [](Pass& p, Args) { p.mem[4].exp_avg_sq = nullptr; });
  check_refused("null X", [](Pass& p, Args) { p.mem[0].X = nullptr; });
  check_refused("null perm", [](Pass& p, Args) { p.mem[1].perm = nullptr; });
  check_refused("null adv", [](Pass& p, Args) { p.mem[3].adv = nullptr; });
  check_refused("null returns", [](Pass& p, Args) { p.a.kind = 1; p.mem[3].returns = nullptr; });
  check_refused("no members", [](Pass& p, Args) { p.a.n_members = 0; });
  check_refused("too many members", [](Pass& p, Args) { p.a.n_members = 1025; });
  check_refused("H = 128", [](Pass& p, Args) { p.desc.dims[1] = p.desc.dims[2] = 128; });
  check_refused("relu", [](Pass& p, Args) { p.desc.hidden_act = 1; });
  check_refused("output act", [](Pass& p, Args) { p.desc.output_act = 1; });
  check_refused("layer norm", [](Pass& p, Args) { p.desc.layer_norm = 1; });
  check_refused("misaligned params", [](Pass& p, Args) { p.mem[1].params = p.flat + 1; });
  check_refused("misaligned grads", [](Pass& p, Args) { p.mem[1].grads = p.flat + 2; });
  check_refused("ldx", [](Pass& p, Args) { p.mem[2].ldx = 5; });
  check_refused("lda", [](Pass& p, Args) { p.mem[2].lda = 3; });
  check_refused("misaligned partials", [](Pass& p, Args) { p.a.partials = p.partials + 1; });
  check_refused("S = 0", [](Pass& p, Args) { p.mem[3].S = 0; });
  check_refused("mb < 0", [](Pass& p, Args) { p.a.mb = -1; });
  check_refused("small partials", [](Pass& p, Args) { p.a.partials_floats -= 1; });
  check_refused("kind 3", [](Pass& p, Args) { p.a.kind = 3; });
  check_refused("kind -1", [](Pass& p, Args) { p.a.kind = -1; });
  check_refused("algo 2", [](Pass& p, Args) { p.a.algo = 2; });
  check_refused("step0 < 0", [](Pass& p, Args) { p.mem[0].step0 = -1; });
  reset();
  return finish("members loop ok");
}
