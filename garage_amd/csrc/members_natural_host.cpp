// The natural-gradient (TRPO) step of a POPULATION of narrow networks, enqueued from C++.
//
// A lone TRPO learner pays a chain of per-layer launches and a host wait per
// conjugate-gradient iteration.  Here every pass over the batch is one launch for all
// members (members_natural.hip) and the recurrence's scalars stay on the device, so a
// whole solve is 2 (cg_iters + 1) + 2 launches whatever the member count, with no host
// wait inside: the member table is built in pinned host memory, uploaded once per call
// (table_slots.h) and read by the launches that follow on the caller's stream.  A
// translation unit of its own behind a launch seam (members_natural.h), so that the CPU
// harness under tests/host builds it against fakes of the kernel side.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "internal.h"
#include "members_natural.h"
#include "table_slots.h"

namespace {

constexpr int64_t MAX_MEMBERS = 1024;
constexpr int64_t ROWS_LIMIT = 1ll << 31;
constexpr int64_t FLAT_LIMIT = 1ll << 20;

int64_t r4(int64_t v) { return (v + 3) & ~(int64_t)3; }

GaTableRing g_ring;

bool shape_ok(const ga_mlp_desc* d) {
  if (!d || d->n_layers != 3) return false;
  if (d->hidden_act != 0 || d->output_act != 0 || d->layer_norm) return false;
  // (<= NS_IN_OVERLAY inputs always; up to NS_IN_MAX, the wide kernel of
  // members_natural.hip, where the caller has asked for the range: ga_set_narrow_wide)
  return ga_narrow_overlay_supported(3, d->dims) != 0 ||
         (ga_narrow_wide_on() && ga_narrow_wide_supported(3, d->dims) != 0);
}

// The workspace, in floats from its start: the members' vectors [NG_VECS][n][round4(n_flat)],
// their scalars [n][NG_SCALARS] doubles, their workgroups' sums [n][NG_SHARES][2] doubles,
// their gradient shares [n][NG_SHARES][stride], then member after member its saved head
// outputs [S_m][NS_HN].
struct Layout {
  int64_t vectors, scalars, lpart, part, heads, total;
};
Layout layout_of(const ga_mlp_desc* d, int64_t n_flat, int64_t n, int64_t rows_total) {
  Layout l;
  l.vectors = 0;
  l.scalars = l.vectors + (int64_t)NG_VECS * n * r4(n_flat);
  l.lpart = l.scalars + 2 * (int64_t)NG_SCALARS * n;
  l.part = l.lpart + 2 * 2 * (int64_t)NG_SHARES * n;
  l.heads = l.part + n * NG_SHARES * ga_narrow_step_stride(d->dims[0], d->dims[1]);
  l.total = l.heads + rows_total * NS_HN;
  return l;
}

bool flat_ok(const ga_mlp_desc* d, int64_t n_flat) {
  if (n_flat < 4 || n_flat > FLAT_LIMIT) return false;
  for (int l = 0; l < 3; ++l) {
    if (d->w_off[l] < 4 || d->w_off[l] % 4 || d->b_off[l] < 4 || d->b_off[l] % 4) return false;
    if (d->w_off[l] + (int64_t)d->dims[l + 1] * r4(d->dims[l]) > n_flat) return false;
    if (d->b_off[l] + d->dims[l + 1] > n_flat) return false;
  }
  return true;
}

enum Entry { SOLVE, FVP, CANDIDATES };

int check_args(const ga_members_natural_args* a, Entry entry, const char* who) {
  GA_REQUIRE(a && a->desc && a->members_host && a->workspace, "%s: null pointer", who);
  GA_REQUIRE(a->n_members >= 1 && a->n_members <= MAX_MEMBERS, "%s: n_members must be 1 .. %lld",
             who, (long long)MAX_MEMBERS);
  const ga_mlp_desc* d = a->desc;
  GA_REQUIRE(shape_ok(d),
             "%s: unsupported network (two equal tanh hidden layers of 32 or 64 units, <= 32 "
             "inputs, <= 128 inputs under ga_set_narrow_wide(1), <= 8 linear outputs, no "
             "layer norm; tanh whatever ga_set_narrow_acts says)", who);
  GA_REQUIRE(a->kind == 0 || a->kind == 2,
             "%s: kind must be 0 (Gaussian) or 2 (categorical)", who);
  GA_REQUIRE(flat_ok(d, a->n_flat),
             "%s: parameter offsets must be quads from 4 up inside n_flat", who);
  GA_REQUIRE(ga_aligned16(a->workspace), "%s: workspace must be 16-B aligned", who);
  if (entry == SOLVE)
    GA_REQUIRE(a->cg_iters >= 0 && a->cg_iters <= 1000, "%s: cg_iters must be 0 .. 1000", who);
  if (entry == CANDIDATES) GA_REQUIRE(a->result, "%s: null pointer (result)", who);
  const int A = d->dims[3];
  int64_t rows_total = 0;
  for (int64_t m = 0; m < a->n_members; ++m) {
    const ga_member_natural& u = a->members_host[m];
    GA_REQUIRE(u.params && u.X, "%s: member %lld: null pointer", who, (long long)m);
    GA_REQUIRE(u.S >= 1 && u.S < ROWS_LIMIT, "%s: member %lld: bad S", who, (long long)m);
    GA_REQUIRE(ga_aligned16(u.params) && ga_aligned16(u.X) && u.ldx % 4 == 0 &&
                   u.ldx >= r4(d->dims[0]),
               "%s: member %lld: operands must be 16-B aligned quads", who, (long long)m);
    if (entry == FVP) {
      GA_REQUIRE(u.vec && u.out, "%s: member %lld: null pointer (vec, out)", who, (long long)m);
      GA_REQUIRE(ga_aligned16(u.vec) && ga_aligned16(u.out),
                 "%s: member %lld: operands must be 16-B aligned quads", who, (long long)m);
    } else {
      GA_REQUIRE(u.actions && u.adv && u.old_ll,
                 "%s: member %lld: null pointer (batch arrays)", who, (long long)m);
      GA_REQUIRE(a->kind == 2 ? u.lda >= 1
                              : (u.lda % 4 == 0 && ga_aligned16(u.actions) && u.lda >= r4(A)),
                 "%s: member %lld: actions must be 16-B aligned quads", who, (long long)m);
      GA_REQUIRE(u.max_constraint_value > 0.0 && isfinite(u.max_constraint_value),
                 "%s: member %lld: max_constraint_value must be positive", who, (long long)m);
    }
    GA_REQUIRE(u.hvp_reg_coeff >= 0.0 && isfinite(u.hvp_reg_coeff),
               "%s: member %lld: hvp_reg_coeff must not be negative", who, (long long)m);
    if (entry == CANDIDATES) {
      GA_REQUIRE(u.backtrack_ratio > 0.0 && u.backtrack_ratio <= 1.0,
                 "%s: member %lld: backtrack_ratio must be in (0, 1]", who, (long long)m);
      GA_REQUIRE(u.state >= NG_SEARCHING && u.state <= NG_REJECTED,
                 "%s: member %lld: state must be 0 .. 2", who, (long long)m);
    }
    rows_total += u.S;
  }
  const Layout l = layout_of(d, a->n_flat, a->n_members, rows_total);
  GA_REQUIRE(a->workspace_floats >= l.total, "%s: workspace too small (%lld floats, %lld needed)",
             who, (long long)a->workspace_floats, (long long)l.total);
  return GA_OK;
}

// The shared struct and the device table of one call, then `launches(sh, table_dev)`.
template <class F>
int enqueue(const ga_members_natural_args* a, double ratio_k, const char* who,
            hipStream_t stream, F&& launches) {
  const ga_mlp_desc* d = a->desc;
  const int64_t n = a->n_members;
  GaNaturalShared sh;
  memset(&sh, 0, sizeof(sh));
  for (int l = 0; l < 3; ++l) { sh.w_off[l] = d->w_off[l]; sh.b_off[l] = d->b_off[l]; }
  sh.in_w = d->dims[0]; sh.H = d->dims[1]; sh.out_w = d->dims[3];
  sh.kind = a->kind; sh.ent_flags = a->ent_flags;
  sh.has_min = a->has_min; sh.has_max = a->has_max;
  sh.min_log_std = a->min_log_std; sh.max_log_std = a->max_log_std;
  sh.double_softmax = a->double_softmax; sh.zero_slot0 = !a->learn_std;
  sh.stride = ga_narrow_step_stride(sh.in_w, sh.H);
  sh.n_flat = a->n_flat;
  sh.vec_stride = n * r4(a->n_flat);
  sh.n_members = (int32_t)n;
  sh.vec_sel = -1;

  int64_t rows_total = 0;
  for (int64_t m = 0; m < n; ++m) rows_total += a->members_host[m].S;
  const Layout lay = layout_of(d, a->n_flat, n, rows_total);
  const size_t table_bytes = (size_t)n * sizeof(GaNaturalDev);
  std::lock_guard<std::mutex> lock(g_ring.mu);
  GaTableSlot* slot = g_ring.take(table_bytes);
  if (!slot) {
    ga_set_error("%s: cannot allocate the member table", who);
    return GA_ERR_HIP;
  }
  GaNaturalDev* table = static_cast<GaNaturalDev*>(slot->host);
  memset(table, 0, table_bytes);
  float* ws = a->workspace;
  int64_t head_rows = 0;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_natural& u = a->members_host[m];
    GaNaturalDev& t = table[m];
    t.params = u.params; t.X = u.X; t.ldx = u.ldx;
    t.actions = u.actions; t.lda = u.lda; t.old_ll = u.old_ll; t.adv = u.adv;
    t.vec = u.vec; t.out = u.out;
    t.vectors = ws + lay.vectors + m * r4(a->n_flat);
    t.scalars = reinterpret_cast<double*>(ws + lay.scalars) + NG_SCALARS * m;
    t.lpart = reinterpret_cast<double*>(ws + lay.lpart) + 2 * NG_SHARES * m;
    t.part = ws + lay.part + m * NG_SHARES * sh.stride;
    t.heads = ws + lay.heads + head_rows * NS_HN;
    head_rows += u.S;
    t.result = a->result ? a->result + 2 * m : nullptr;
    t.S = (int32_t)u.S; t.state = u.state;
    t.inv_S = 1.f / (float)u.S;
    t.ent_coeff = u.ent_coeff;
    t.delta = (float)u.max_constraint_value; t.reg = (float)u.hvp_reg_coeff;
    t.neg_ratio = (float)(-pow(u.backtrack_ratio, ratio_k));  // (read by MODE_EVAL only)
  }
  const GaNaturalDev* table_dev = static_cast<const GaNaturalDev*>(slot->dev);
  int rc = GA_OK;
  if (!GaTableRing::upload(slot, table_bytes, stream)) {
    ga_set_error("%s: table upload failed", who);
    rc = GA_ERR_HIP;
  }
  if (!rc) rc = launches(sh, table_dev);
  if (!GaTableRing::mark_done(slot, stream) && !rc) {
    ga_set_error("%s: hipEventRecord failed", who);
    rc = GA_ERR_HIP;
  }
  return rc;
}

}  // namespace

extern "C" int ga_members_natural_supported(const ga_mlp_desc* d) { return shape_ok(d) ? 1 : 0; }

extern "C" int64_t ga_members_natural_floats(const ga_mlp_desc* d, int64_t n_flat,
                                             int64_t n_members, const int64_t* rows,
                                             int64_t* layout) {
  if (!shape_ok(d) || !rows || n_members < 1 || n_members > MAX_MEMBERS ||
      !flat_ok(d, n_flat))
    return 0;
  int64_t rows_total = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    if (rows[m] < 1 || rows[m] >= ROWS_LIMIT) return 0;
    rows_total += rows[m];
  }
  const Layout l = layout_of(d, n_flat, n_members, rows_total);
  if (layout) {
    layout[0] = l.vectors; layout[1] = l.scalars; layout[2] = l.lpart; layout[3] = l.part;
    layout[4] = l.heads;
  }
  return l.total;
}

extern "C" void ga_members_natural_release(void) { g_ring.release(); }

extern "C" int ga_members_natural_solve(const ga_members_natural_args* a, ga_stream_t stream_) {
  static const char* who = "ga_members_natural_solve";
  int rc = check_args(a, SOLVE, who);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int cg_iters = a->cg_iters;
  return enqueue(a, 0.0, who, stream, [&](GaNaturalShared& sh, const GaNaturalDev* table) {
    int r = ga_members_natural_launch(&sh, table, NG_MODE_GRAD, stream);
    if (!r) r = ga_members_cg_launch(&sh, table, NG_CG_BEGIN, stream);
    sh.vec_sel = NG_P; sh.respect_done = 1;
    for (int it = 0; it < cg_iters && !r; ++it) {
      r = ga_members_natural_launch(&sh, table, NG_MODE_FVP, stream);
      if (!r) r = ga_members_cg_launch(&sh, table, NG_CG_STEP, stream);
    }
    sh.vec_sel = NG_X; sh.respect_done = 0;
    if (!r) r = ga_members_natural_launch(&sh, table, NG_MODE_FVP, stream);
    if (!r) r = ga_members_cg_launch(&sh, table, NG_CG_FINISH, stream);
    return r;
  });
}

extern "C" int ga_members_natural_fvp(const ga_members_natural_args* a, ga_stream_t stream_) {
  static const char* who = "ga_members_natural_fvp";
  int rc = check_args(a, FVP, who);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  return enqueue(a, 0.0, who, stream, [&](GaNaturalShared& sh, const GaNaturalDev* table) {
    int r = ga_members_natural_launch(&sh, table, NG_MODE_FVP, stream);
    if (!r) r = ga_members_cg_launch(&sh, table, NG_CG_PRODUCT, stream);
    return r;
  });
}

extern "C" int ga_members_natural_candidates(const ga_members_natural_args* a, int64_t k,
                                             ga_stream_t stream_) {
  static const char* who = "ga_members_natural_candidates";
  int rc = check_args(a, CANDIDATES, who);
  if (rc) return rc;
  GA_REQUIRE(k >= 0 && k <= 1000, "%s: k must be 0 .. 1000", who);
  hipStream_t stream = (hipStream_t)stream_;
  bool searching = false, rejected = false;
  for (int64_t m = 0; m < a->n_members; ++m) {
    searching |= a->members_host[m].state == NG_SEARCHING;
    rejected |= a->members_host[m].state == NG_REJECTED;
  }
  return enqueue(a, (double)k, who, stream, [&](GaNaturalShared& sh, const GaNaturalDev* table) {
    int r = GA_OK;
    if (searching) {
      r = ga_members_natural_launch(&sh, table, NG_MODE_EVAL, stream);
      if (!r) r = ga_members_eval_finish_launch(&sh, table, stream);
    }
    if (rejected && !r) r = ga_members_candidate_launch(&sh, table, stream);
    return r;
  });
}
