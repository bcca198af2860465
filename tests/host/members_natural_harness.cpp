// Host-logic harness for the population's natural-gradient step
// (garage_amd/csrc/members_natural_host.cpp), built with -fsanitize=address,undefined on
// the CPU (`make asan-members-natural`).  The launch seam and the HIP runtime calls are
// fakes: "device" memory is exactly-sized host memory, a copy happens at once, and each
// fake launch records its mode and walks what its kernel would touch of every member's
// stretch of the workspace, so that an extent that is off by one trips the sanitizer.
// The checks: the launch sequence of a solve, a product and a backtrack round, the
// table's contents, the workspace's size and layout, nothing copied or launched after a
// refusal.
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/members_natural.h"
#include "../../garage_amd/csrc/shape_rules.h"
#include "harness.h"

// ---- what the fakes record ------------------------------------------------------------
struct Launch {
  char what;  // 'n' natural pass, 'c' cg, 'f' eval finish, 'r' restore
  int mode, vec_sel, respect_done;
};
static std::vector<Launch> g_launches;
static std::vector<GaNaturalDev> g_table;  // the table of the last launch

static void touch(const GaNaturalShared* sh, const GaNaturalDev* table, bool heads) {
  g_table.assign(table, table + sh->n_members);
  for (int m = 0; m < sh->n_members; ++m) {
    const GaNaturalDev& t = table[m];
    const int shares = ga_natural_shares(t.S);
    for (int v = 0; v < NG_VECS; ++v)
      for (int64_t i = 0; i < sh->n_flat; ++i) t.vectors[v * sh->vec_stride + i] = 1.f;
    for (int s = 0; s < NG_SCALARS; ++s) t.scalars[s] = 1.0;
    for (int s = 0; s < shares; ++s) {
      t.lpart[2 * s] = t.lpart[2 * s + 1] = 1.0;
      for (int64_t e = 0; e < sh->stride; ++e) t.part[s * sh->stride + e] = 1.f;
    }
    if (heads)
      for (int64_t e = 0; e < (int64_t)t.S * NS_HN; ++e) t.heads[e] = 1.f;
  }
}

static int record(char what, const GaNaturalShared* sh, const GaNaturalDev* table, int mode) {
  g_launches.push_back({what, mode, sh->vec_sel, sh->respect_done});
  touch(sh, table, what == 'n');
  if (what == 'f')
    for (int m = 0; m < sh->n_members; ++m) table[m].result[0] = table[m].result[1] = 1.0;
  return 0;
}
extern "C" {
int ga_members_natural_launch(const GaNaturalShared* sh, const GaNaturalDev* t, int mode,
                              hipStream_t) { return record('n', sh, t, mode); }
int ga_members_cg_launch(const GaNaturalShared* sh, const GaNaturalDev* t, int mode,
                         hipStream_t) { return record('c', sh, t, mode); }
int ga_members_candidate_launch(const GaNaturalShared* sh, const GaNaturalDev* t,
                                hipStream_t) { return record('r', sh, t, 0); }
int ga_members_eval_finish_launch(const GaNaturalShared* sh, const GaNaturalDev* t,
                                  hipStream_t) { return record('f', sh, t, 0); }
}  // extern "C"

// ---- a call over exactly-sized buffers ------------------------------------------------
static const int64_t kS[3] = {1094, 65, 1};

struct Call {
  ga_mlp_desc desc;
  ga_members_natural_args a;
  std::vector<ga_member_natural> mem;
  int64_t n_flat = 0, layout[5];
  float* ws = nullptr;
  double* result = nullptr;
  float* flat = nullptr;  // stands for every operand that is only passed on
  explicit Call(int n) {
    memset(&desc, 0, sizeof(desc));
    desc.n_layers = 3;
    desc.dims[0] = 17; desc.dims[1] = desc.dims[2] = 64; desc.dims[3] = 6;
    int64_t off = 4;
    for (int l = 0; l < 3; ++l) {
      desc.w_off[l] = off; off += (int64_t)desc.dims[l + 1] * ((desc.dims[l] + 3) & ~3);
      desc.b_off[l] = off; off += (desc.dims[l + 1] + 3) & ~3;
    }
    n_flat = off;
    memset(&a, 0, sizeof(a));
    a.desc = &desc; a.n_flat = n_flat; a.kind = 0; a.learn_std = 1; a.cg_iters = 10;
    a.n_members = n;
    flat = static_cast<float*>(aligned_alloc(16, 64));
    mem.resize(n);
    int64_t rows[3];
    for (int m = 0; m < n; ++m) {
      ga_member_natural& u = mem[m];
      memset(&u, 0, sizeof(u));
      u.params = flat; u.X = flat; u.ldx = 20; u.S = rows[m] = kS[m];
      u.actions = flat; u.lda = 8; u.old_ll = flat; u.adv = flat;
      u.max_constraint_value = 0.01 * (m + 1); u.hvp_reg_coeff = 1e-5;
      u.backtrack_ratio = 0.8; u.ent_coeff = 0.5f * m;
      u.vec = flat; u.out = flat;
    }
    a.members_host = mem.data();
    a.workspace_floats = ga_members_natural_floats(&desc, n_flat, n, rows, layout);
    ws = static_cast<float*>(aligned_alloc(16, sizeof(float) * a.workspace_floats));
    a.workspace = ws;
    result = static_cast<double*>(malloc(sizeof(double) * 2 * n));  // exactly [n][2]
    a.result = result;
  }
  ~Call() { free(ws); free(result); free(flat); }
};

static void reset() {
  ga_members_natural_release();
  g_launches.clear(); g_table.clear();
  g_host_allocs.clear(); g_dev_allocs.clear(); g_copies.clear();
  g_events_recorded = 0;
  g_error.clear();
}

static void check_solve(int n) {
  reset();
  Call c(n);
  // the workspace: vectors, scalars, sums, shares, the members' head rows -- exactly
  const int64_t stride = ga_narrow_step_stride(17, 64);
  int64_t rows = 0;
  for (int m = 0; m < n; ++m) rows += kS[m];
  CHECK(c.n_flat % 4 == 0);
  CHECK(c.a.workspace_floats == NG_VECS * n * c.n_flat + 2 * NG_SCALARS * n +
                                    4 * NG_SHARES * n + n * NG_SHARES * stride + rows * NS_HN);
  CHECK(c.layout[0] == 0 && c.layout[1] == NG_VECS * n * c.n_flat);
  CHECK(ga_members_natural_solve(&c.a, nullptr) == 0);
  // 2 (cg_iters + 1) + 2 launches: gradient, begin, 10 x (product of p, step), product of
  // x, finish
  CHECK(g_launches.size() == 24);
  for (size_t i = 0; i < g_launches.size(); ++i) {
    const Launch& l = g_launches[i];
    CHECK(l.what == (i % 2 ? 'c' : 'n'));
    const bool cg = i >= 2 && i < 22;
    if (i % 2 == 0) {
      CHECK(l.mode == (i == 0 ? NG_MODE_GRAD : NG_MODE_FVP));
      if (i > 0) CHECK(l.vec_sel == (cg ? NG_P : NG_X) && l.respect_done == (cg ? 1 : 0));
    } else {
      CHECK(l.mode == (i == 1 ? NG_CG_BEGIN : (cg ? NG_CG_STEP : NG_CG_FINISH)));
    }
  }
  // one pinned and one device allocation of exactly the table's bytes, one copy, one event
  const size_t bytes = n * sizeof(GaNaturalDev);
  CHECK(g_host_allocs.size() == 1 && g_host_allocs[0] == bytes);
  CHECK(g_dev_allocs.size() == 1 && g_dev_allocs[0] == bytes);
  CHECK(g_copies.size() == 1 && g_copies[0] == bytes);
  CHECK(g_events_recorded == 1);
  // the table
  CHECK((int)g_table.size() == n);
  int64_t head_rows = 0;
  for (int m = 0; m < n; ++m) {
    const GaNaturalDev& t = g_table[m];
    CHECK(t.S == kS[m] && t.inv_S == 1.f / (float)kS[m]);
    CHECK(t.delta == (float)(0.01 * (m + 1)) && t.reg == 1e-5f && t.ent_coeff == 0.5f * m);
    CHECK(t.vectors == c.ws + m * c.n_flat);
    CHECK(t.scalars == reinterpret_cast<double*>(c.ws + c.layout[1]) + NG_SCALARS * m);
    CHECK(t.lpart == reinterpret_cast<double*>(c.ws + c.layout[2]) + 2 * NG_SHARES * m);
    CHECK(t.part == c.ws + c.layout[3] + m * NG_SHARES * stride);
    CHECK(t.heads == c.ws + c.layout[4] + head_rows * NS_HN);
    CHECK(t.result == c.result + 2 * m);
    head_rows += kS[m];
  }
  // the split is a function of S alone
  CHECK(ga_natural_shares(1094) == 16 && ga_natural_shares(65) == 2 &&
        ga_natural_shares(1) == 1 && ga_natural_shares(64 * 16) == 16);
}

static void check_product_and_rounds() {
  reset();
  Call c(3);
  CHECK(ga_members_natural_fvp(&c.a, nullptr) == 0);
  CHECK(g_launches.size() == 2 && g_launches[0].what == 'n' &&
        g_launches[0].mode == NG_MODE_FVP && g_launches[0].vec_sel == -1 &&
        g_launches[0].respect_done == 0 && g_launches[1].what == 'c' &&
        g_launches[1].mode == NG_CG_PRODUCT);
  g_launches.clear();
  c.mem[1].state = NG_ACCEPTED;
  CHECK(ga_members_natural_candidates(&c.a, 2, nullptr) == 0);
  CHECK(g_launches.size() == 2 && g_launches[0].what == 'n' &&
        g_launches[0].mode == NG_MODE_EVAL && g_launches[1].what == 'f');
  CHECK(g_table[0].neg_ratio == (float)-(0.8 * 0.8) && g_table[1].state == NG_ACCEPTED);
  g_launches.clear();
  c.mem[0].state = NG_REJECTED; c.mem[2].state = NG_ACCEPTED;
  CHECK(ga_members_natural_candidates(&c.a, 3, nullptr) == 0);
  CHECK(g_launches.size() == 1 && g_launches[0].what == 'r');
  g_launches.clear();
  c.mem[2].state = NG_SEARCHING;
  CHECK(ga_members_natural_candidates(&c.a, 3, nullptr) == 0);
  CHECK(g_launches.size() == 3 && g_launches[2].what == 'r');
}

typedef const ga_members_natural_args** Args;
// a call with one thing wrong: refused, with a message, before anything is copied or launched
template <class F>
static void check_refused(const char* what, int entry, F&& spoil) {
  reset();
  Call c(3);
  const ga_members_natural_args* args = &c.a;
  int64_t k = 1;
  spoil(c, &args, &k);
  const int rc = entry == 0   ? ga_members_natural_solve(args, nullptr)
                 : entry == 1 ? ga_members_natural_fvp(args, nullptr)
                              : ga_members_natural_candidates(args, k, nullptr);
  const bool refused = rc < 0 && !g_error.empty() && g_launches.empty() && g_copies.empty();
  if (!refused) fprintf(stderr, "not refused: %s (rc %d, '%s')\n", what, rc, g_error.c_str());
  CHECK(refused);
}

#define REFUSE(what, entry, body) \
  check_refused(what, entry, [](Call& c, Args a, int64_t* k) { (void)c; (void)a; (void)k; body; })
int main() {
  for (int n : {1, 2, 3}) check_solve(n);
  check_product_and_rounds();
  for (int e = 0; e < 3; ++e) {
    REFUSE("null args", e, *a = nullptr);
    REFUSE("null desc", e, c.a.desc = nullptr);
    REFUSE("null members", e, c.a.members_host = nullptr);
    REFUSE("null workspace", e, c.a.workspace = nullptr);
    REFUSE("null params", e, c.mem[1].params = nullptr);
    REFUSE("null X", e, c.mem[2].X = nullptr);
    REFUSE("no members", e, c.a.n_members = 0);
    REFUSE("too many", e, c.a.n_members = 1025);
    REFUSE("H = 128", e, c.desc.dims[1] = c.desc.dims[2] = 128);
    REFUSE("relu", e, c.desc.hidden_act = 1);
    REFUSE("layer norm", e, c.desc.layer_norm = 1);
    REFUSE("kind 1", e, c.a.kind = 1);
    REFUSE("offset", e, c.desc.w_off[1] += 2);
    REFUSE("n_flat", e, c.a.n_flat -= 4);
    REFUSE("misaligned params", e, c.mem[0].params = c.flat + 1);
    REFUSE("misaligned workspace", e, c.a.workspace = c.ws + 1);
    REFUSE("ldx", e, c.mem[2].ldx = 18);
    REFUSE("S = 0", e, c.mem[1].S = 0);
    REFUSE("small workspace", e, c.a.workspace_floats -= 1);
    REFUSE("reg < 0", e, c.mem[1].hvp_reg_coeff = -1.0);
  }
  for (int e : {0, 2}) {
    REFUSE("null adv", e, c.mem[0].adv = nullptr);
    REFUSE("null old_ll", e, c.mem[0].old_ll = nullptr);
    REFUSE("lda", e, c.mem[2].lda = 6);
    REFUSE("delta", e, c.mem[2].max_constraint_value = 0.0);
  }
  REFUSE("cg_iters", 0, c.a.cg_iters = -1);
  REFUSE("null vec", 1, c.mem[1].vec = nullptr);
  REFUSE("null out", 1, c.mem[1].out = nullptr);
  REFUSE("null result", 2, c.a.result = nullptr);
  REFUSE("ratio", 2, c.mem[0].backtrack_ratio = 1.5);
  REFUSE("state", 2, c.mem[0].state = 3);
  REFUSE("k < 0", 2, *k = -1);
  reset();
  return finish("members natural ok");
}
