// One optimisation pass of a POPULATION of narrow networks, enqueued from C++.
//
// ga_update_epoch walks the minibatches of one network's pass, two launches per step on
// the narrow path.  A population of such networks trained member after member pays
// those two launches per member; this loop walks step k of EVERY member at once
// (members_step.hip): the member table and the per-step Adam constants are built in
// pinned host memory, uploaded once per pass (one copy: they lie back to back), and
// max_m n_steps_m pairs of launches follow on the caller's stream.  A translation unit of its own: update.cpp is linked
// into CPU harnesses that fake every entry point it calls.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "internal.h"
#include "fused_train.h"
#include "members_step.h"
#include "table_slots.h"

namespace {

constexpr int64_t MAX_MEMBERS = 1024;
constexpr int64_t ROWS_LIMIT = 1ll << 31;

int64_t r4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// floats of one member's share of `partials`: [tiles][2] doubles of loss sums, then
// [tiles][ga_narrow_step_stride] gradient shares (update.cpp's narrow layout)
int64_t member_floats(const ga_mlp_desc* d, int64_t max_rows) {
  const int64_t tiles = ga_fused_tiles(max_rows);
  return 4 * tiles + tiles * ga_narrow_step_stride(d->dims[0], d->dims[1]);
}

// The tables of one pass go through a ring of pinned / device slots (table_slots.h): the
// one place where this entry point may block its caller.
GaTableRing g_ring;

int64_t member_steps(int64_t S, int64_t mb) { return mb == 0 ? 1 : (S + mb - 1) / mb; }

int check_args(const ga_update_members_args* a) {
  GA_REQUIRE(a && a->desc && a->members_host && a->partials,
             "ga_update_epoch_members: null pointer");
  GA_REQUIRE(a->n_members >= 1 && a->n_members <= MAX_MEMBERS,
             "ga_update_epoch_members: n_members must be 1 .. %lld", (long long)MAX_MEMBERS);
  const ga_mlp_desc* d = a->desc;
  GA_REQUIRE(ga_update_members_supported(d),
             "ga_update_epoch_members: unsupported network (two equal tanh hidden layers "
             "of 32 or 64 units, <= 32 inputs, <= 8 linear outputs, no layer norm)");
  GA_REQUIRE(a->kind >= 0 && a->kind <= 2, "ga_update_epoch_members: kind must be 0 .. 2");
  GA_REQUIRE(a->algo == 0 || a->algo == 1, "ga_update_epoch_members: algo must be 0 or 1");
  GA_REQUIRE(a->mb >= 0 && a->mb < ROWS_LIMIT, "ga_update_epoch_members: bad mb");
  for (int l = 0; l < 3; ++l)
    GA_REQUIRE(d->w_off[l] >= 4 && d->w_off[l] % 4 == 0 && d->b_off[l] >= 4 &&
                   d->b_off[l] % 4 == 0,
               "ga_update_epoch_members: parameter offsets must be quads from 4 up");
  GA_REQUIRE(ga_aligned16(a->partials),
             "ga_update_epoch_members: partials must be 16-B aligned");
  const int A = d->dims[3];
  int64_t max_rows = 0;
  for (int64_t m = 0; m < a->n_members; ++m) {
    const ga_member_update& u = a->members_host[m];
    GA_REQUIRE(u.params && u.grads && u.exp_avg && u.exp_avg_sq && u.X,
               "ga_update_epoch_members: member %lld: null pointer", (long long)m);
    GA_REQUIRE(u.S >= 1 && u.S < ROWS_LIMIT, "ga_update_epoch_members: member %lld: bad S",
               (long long)m);
    GA_REQUIRE(u.step0 >= 0, "ga_update_epoch_members: member %lld: bad step0",
               (long long)m);
    GA_REQUIRE(u.perm || a->mb == 0,
               "ga_update_epoch_members: member %lld: null pointer (perm)", (long long)m);
    GA_REQUIRE(ga_aligned16(u.params) && ga_aligned16(u.grads) && ga_aligned16(u.exp_avg) &&
                   ga_aligned16(u.exp_avg_sq) && ga_aligned16(u.X) && u.ldx % 4 == 0 &&
                   u.ldx >= r4(d->dims[0]),
               "ga_update_epoch_members: member %lld: operands must be 16-B aligned quads",
               (long long)m);
    if (a->kind == 1) {
      GA_REQUIRE(u.returns, "ga_update_epoch_members: member %lld: null pointer (returns)",
                 (long long)m);
    } else {
      GA_REQUIRE(u.actions && u.adv && (a->algo == 1 || u.old_ll),
                 "ga_update_epoch_members: member %lld: null pointer (minibatch arrays)",
                 (long long)m);
      GA_REQUIRE(a->kind == 2 ? u.lda >= 1
                              : (u.lda % 4 == 0 && ga_aligned16(u.actions) && u.lda >= r4(A)),
                 "ga_update_epoch_members: member %lld: actions must be 16-B aligned quads",
                 (long long)m);
    }
    const int64_t rows = a->mb == 0 || u.S < a->mb ? u.S : a->mb;
    if (rows > max_rows) max_rows = rows;
  }
  const int64_t need = ga_update_members_partials_floats(d, a->n_members, max_rows);
  GA_REQUIRE(need > 0 && a->partials_floats >= need,
             "ga_update_epoch_members: partials too small (%lld floats, %lld needed)",
             (long long)a->partials_floats, (long long)need);
  return GA_OK;
}

}  // namespace

extern "C" int ga_update_members_supported(const ga_mlp_desc* d) {
  if (!d || d->n_layers != 3) return 0;
  if (d->hidden_act != 0 || d->output_act != 0 || d->layer_norm) return 0;
  return ga_narrow_step_supported(3, d->dims) ? 1 : 0;
}

extern "C" int64_t ga_update_members_partials_floats(const ga_mlp_desc* d, int64_t n_members,
                                                     int64_t max_rows) {
  if (!ga_update_members_supported(d) || n_members < 1 || n_members > MAX_MEMBERS ||
      max_rows < 1 || max_rows >= ROWS_LIMIT)
    return 0;
  return n_members * member_floats(d, max_rows);
}

// frees the table slots (tests; the library otherwise keeps them for its lifetime)
extern "C" void ga_update_members_release(void) {
  g_ring.release();
}

extern "C" int ga_update_epoch_members(const ga_update_members_args* a,
                                       ga_stream_t stream_) {
  int rc = check_args(a);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const ga_mlp_desc* d = a->desc;
  const int64_t n = a->n_members, mb = a->mb;
  int64_t n_steps = 0, max_rows = 0;
  for (int64_t m = 0; m < n; ++m) {
    const int64_t S = a->members_host[m].S, steps = member_steps(S, mb);
    const int64_t rows = mb == 0 || S < mb ? S : mb;
    if (steps > n_steps) n_steps = steps;
    if (rows > max_rows) max_rows = rows;
  }
  const int64_t per_member = member_floats(d, max_rows);
  const int64_t tiles = ga_fused_tiles(max_rows);

  GaMembersShared sh;
  memset(&sh, 0, sizeof(sh));
  for (int l = 0; l < 3; ++l) { sh.w_off[l] = d->w_off[l]; sh.b_off[l] = d->b_off[l]; }
  sh.in_w = d->dims[0]; sh.H = d->dims[1]; sh.out_w = d->dims[3];
  sh.kind = a->kind; sh.algo = a->algo; sh.ent_flags = a->ent_flags;
  sh.has_min = a->has_min; sh.has_max = a->has_max;
  sh.min_log_std = a->min_log_std; sh.max_log_std = a->max_log_std;
  sh.double_softmax = a->double_softmax; sh.zero_slot0 = !a->learn_std;
  sh.stride = ga_narrow_step_stride(sh.in_w, sh.H);
  sh.mb = mb; sh.n_members = (int32_t)n;

  // [n] members, then [n_steps][n] Adam constants
  const size_t table_bytes = (size_t)n * sizeof(GaMemberDev);
  const size_t adam_bytes = (size_t)(n_steps * n) * sizeof(GaAdam);
  std::lock_guard<std::mutex> lock(g_ring.mu);
  GaTableSlot* slot = g_ring.take(table_bytes + adam_bytes);
  if (!slot) {
    ga_set_error("ga_update_epoch_members: cannot allocate the member tables");
    return GA_ERR_HIP;
  }
  GaMemberDev* table = static_cast<GaMemberDev*>(slot->host);
  GaAdam* adam = reinterpret_cast<GaAdam*>(static_cast<char*>(slot->host) + table_bytes);
  memset(slot->host, 0, table_bytes + adam_bytes);
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_update& u = a->members_host[m];
    GaMemberDev& t = table[m];
    t.params = u.params; t.grads = u.grads; t.exp_avg = u.exp_avg;
    t.exp_avg_sq = u.exp_avg_sq;
    t.X = u.X; t.ldx = u.ldx; t.actions = u.actions; t.lda = u.lda; t.old_ll = u.old_ll;
    t.adv = u.adv; t.returns = u.returns; t.perm = u.perm;
    float* base = a->partials + m * per_member;
    t.lpart = reinterpret_cast<double*>(base);
    t.part = base + 4 * tiles;
    t.losses = u.losses;
    const int64_t steps = member_steps(u.S, mb);
    const int64_t last = u.S - (steps - 1) * mb;
    t.n_steps = (int32_t)steps; t.last_M = (int32_t)last;
    t.inv_full = mb > 0 ? 1.f / (float)mb : 0.f;
    t.inv_last = 1.f / (float)last;
    t.clip = u.clip; t.ent_coeff = u.ent_coeff;
    for (int64_t k = 0; k < steps; ++k)
      adam[k * n + m] = ga_adam_coeffs(u.lr, a->beta1, a->beta2, a->eps, u.step0 + k + 1);
  }
  GaMemberDev* table_dev = static_cast<GaMemberDev*>(slot->dev);
  GaAdam* adam_dev = reinterpret_cast<GaAdam*>(static_cast<char*>(slot->dev) + table_bytes);
  // from the first copy on the stream may read the slot: whatever happens after it, the
  // event goes behind what was enqueued and the slot counts as in flight
  // (the two tables lie back to back in both memories: one copy carries both)
  if (!GaTableRing::upload(slot, table_bytes + adam_bytes, stream)) {
    ga_set_error("ga_update_epoch_members: table upload failed");
    rc = GA_ERR_HIP;
  }
  for (int64_t k = 0; k < n_steps && !rc; ++k) {
    // tiles of the largest minibatch any member has in step k
    int64_t rows_k = 0;
    for (int64_t m = 0; m < n; ++m) {
      if (k >= table[m].n_steps) continue;
      const int64_t rows = k == table[m].n_steps - 1 ? table[m].last_M : mb;
      if (rows > rows_k) rows_k = rows;
    }
    const int64_t tiles_k = ga_fused_tiles(rows_k);
    rc = ga_members_train_step(&sh, table_dev, k, tiles_k, stream);
    if (!rc)
      rc = ga_members_reduce_adam(&sh, table_dev, adam_dev + k * n, k, tiles_k, stream);
  }
  if (!GaTableRing::mark_done(slot, stream)) {
    if (!rc) {
      ga_set_error("ga_update_epoch_members: hipEventRecord failed");
      rc = GA_ERR_HIP;
    }
  }
  return rc;
}
