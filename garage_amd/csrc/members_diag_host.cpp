// The diagnostics passes of a POPULATION of narrow networks in joint launches: the host
// side of every ga_*_members_f32 entry point of include/garage_amd.h's "diagnostics of a
// population" section -- argument checks, each member's table entries (the parameter
// structs its lone launch would get, its own grid, its own stretch of the partials), one
// asynchronous copy of the tables per call and a fixed number of launches whatever the
// member count.  Host C++ only: the launches go through the seam of members_diag.h, so
// that this file builds for the CPU harness under tests/host (members_diag_harness.cpp).
//
// The forward pass does not restate which kernel a layer takes: it asks mlp_layers.cpp for
// the steps ga_mlp_forward_f32 would launch for every member (ga_mlp_forward_steps) and
// groups equal kernels of equal layers into one table each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "internal.h"
#include "members_diag.h"
#include "table_slots.h"

namespace {

constexpr int64_t MAX_MEMBERS = 1024;
constexpr int64_t ROWS_LIMIT = 1ll << 31;

int64_t r4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// the tables of a call go through a ring of pinned / device slots (table_slots.h)
GaTableRing g_ring;

// Tables of one call, laid out back to back in one slot (16-byte aligned each)
struct TableLayout {
  size_t bytes = 0;
  size_t add(size_t n) {
    const size_t at = bytes;
    bytes += (n + 15) & ~(size_t)15;
    return at;
  }
};

// Takes a slot of `bytes`, lets `fill(host base)` write the tables, uploads them and runs
// `launch(device base)`; the slot is marked done behind whatever was enqueued.
template <class Fill, class Launch>
int with_tables(const char* who, size_t bytes, hipStream_t stream, Fill&& fill,
                Launch&& launch) {
  std::lock_guard<std::mutex> lock(g_ring.mu);
  GaTableSlot* slot = g_ring.take(bytes);
  if (!slot) {
    ga_set_error("%s: cannot allocate the member tables", who);
    return GA_ERR_HIP;
  }
  memset(slot->host, 0, bytes);
  fill(static_cast<char*>(slot->host));
  int rc = GA_OK;
  if (!GaTableRing::upload(slot, bytes, stream)) {
    ga_set_error("%s: table upload failed", who);
    rc = GA_ERR_HIP;
  }
  if (!rc) rc = launch(static_cast<char*>(slot->dev));
  if (!GaTableRing::mark_done(slot, stream) && !rc) {
    ga_set_error("%s: hipEventRecord failed", who);
    rc = GA_ERR_HIP;
  }
  return rc;
}

int check_count(const char* who, const void* members, int64_t n, int64_t most) {
  GA_REQUIRE(members, "%s: null pointer", who);
  GA_REQUIRE(n >= 1 && n <= most, "%s: n_members must be 1 .. %lld", who, (long long)most);
  return GA_OK;
}

// every member's stretch of `partials`: per doubles per block of its own grid
int partials_offsets(const char* who, const std::vector<int64_t>& rows, int per,
                     const double* partials, int64_t partials_doubles,
                     std::vector<int64_t>* off) {
  int64_t need = 0;
  off->clear();
  for (int64_t r : rows) {
    off->push_back(need);
    need += (int64_t)per * ga_red_blocks(r);
  }
  GA_REQUIRE(partials && (reinterpret_cast<uintptr_t>(partials) & 7u) == 0,
             "%s: partials must be an 8-byte aligned pointer", who);
  GA_REQUIRE(partials_doubles >= need, "%s: partials too small (%lld doubles, %lld needed)",
             who, (long long)partials_doubles, (long long)need);
  return GA_OK;
}

}  // namespace

extern "C" int64_t ga_members_diag_partials_doubles(const int64_t* rows, int64_t n_members) {
  if (!rows || n_members < 1 || n_members > 2 * MAX_MEMBERS) return 0;
  int64_t need = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    if (rows[m] < 1 || rows[m] >= ROWS_LIMIT) return 0;
    need += 2 * (int64_t)ga_red_blocks(rows[m]);
  }
  return need;
}

// frees the table slots (tests; the library otherwise keeps them for its lifetime)
extern "C" void ga_members_diag_release(void) { g_ring.release(); }

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
// Would ga_mlp_forward_members_f32 take this network under the switches as they stand?
// The plans of a 64-row and of a one-row entry are asked (on both sides of the head
// fusion's row rule) with a pointer that is never read.
extern "C" int ga_mlp_forward_members_supported(const ga_mlp_desc* d) {
  alignas(16) static float nowhere[4];
  if (!d || !ga_update_members_supported(d)) {
    ga_set_error("ga_mlp_forward_members_supported: unsupported network");
    return 0;
  }
  for (int64_t rows : {(int64_t)64, (int64_t)1}) {
    ga_mlp_desc dd = *d;
    dd.act_off[0] = 0;
    dd.act_off[1] = r4(d->dims[1]) * rows;
    GaForwardStep steps[8];
    int ns = 0;
    if (ga_mlp_forward_steps(&dd, nowhere, nowhere, r4(d->dims[0]), nullptr, rows, nowhere,
                             nowhere, r4(d->dims[3]), steps, &ns))
      return 0;  // (ga_last_error says why)
    for (int i = 0; i < ns; ++i) {
      const GaForwardStep& st = steps[i];
      const bool ok =
          st.kind == MD_FWD_SKINNY
              ? (st.sp.w_kc && st.sp.epi == 0 && st.sp.KV >= 1 && st.sp.KV <= 8)
              : (st.kind == MD_FWD_GEMM_HEAD
                     ? st.hp.width == 64
                     : (st.gp.tile == GT_128x32 || st.gp.tile == GT_64x64));
      if (!ok) {
        ga_set_error("ga_mlp_forward_members_supported: layer %d takes a kernel that has no "
                     "members instantiation under the current switches", st.layer);
        return 0;
      }
    }
  }
  return 1;
}

extern "C" int ga_mlp_forward_members_f32(const ga_mlp_desc* d, const ga_member_forward* members,
                                          int64_t n, ga_stream_t stream_) {
  const char* who = "ga_mlp_forward_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(d, "%s: null pointer", who);
  int rc = check_count(who, members, n, 2 * MAX_MEMBERS);
  if (rc) return rc;
  GA_REQUIRE(ga_update_members_supported(d),
             "%s: unsupported network (two equal tanh hidden layers of 32 or 64 units, <= 32 "
             "inputs, <= 8 linear outputs, no layer norm)", who);
  const int L = d->n_layers;  // 3
  // per layer: the streaming kernel's entries, and one GEMM table per instantiation
  std::vector<MdSkinnyEntry> skinny[3];
  int skinny_kv[3] = {0, 0, 0};
  unsigned skinny_lds[3] = {0, 0, 0};
  std::vector<GemmParams> gemm[3][MD_GEMM_KINDS];
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_forward& u = members[m];
    GA_REQUIRE(u.params && u.X && u.acts && u.out, "%s: member %lld: null pointer", who,
               (long long)m);
    GA_REQUIRE(u.rows >= 1 && u.rows < ROWS_LIMIT, "%s: member %lld: bad rows", who,
               (long long)m);
    GA_REQUIRE(ga_aligned16(u.params) && ga_aligned16(u.X) && ga_aligned16(u.acts) &&
                   ga_aligned16(u.out) && u.ldx % 4 == 0 && u.ldx >= r4(d->dims[0]) &&
                   u.ldo % 4 == 0 && u.ldo >= r4(d->dims[L]),
               "%s: member %lld: operands must be 16-B aligned quads", who, (long long)m);
    // the member's activations: layer l's block at (widths below it) * rows, the layout of
    // ga_mlp_forward_f32's workspace at a capacity of exactly `rows`
    ga_mlp_desc dd = *d;
    int64_t aoff = 0;
    for (int l = 0; l + 1 < L; ++l) {
      dd.act_off[l] = aoff * u.rows;
      aoff += r4(d->dims[l + 1]);
    }
    GaForwardStep steps[8];
    int ns = 0;
    rc = ga_mlp_forward_steps(&dd, u.params, u.X, u.ldx, nullptr, u.rows, u.acts, u.out,
                              u.ldo, steps, &ns);
    if (rc) return rc;
    for (int i = 0; i < ns; ++i) {
      const GaForwardStep& st = steps[i];
      GA_REQUIRE(st.layer >= 0 && st.layer < 3, "%s: member %lld: layer %d", who,
                 (long long)m, st.layer);
      if (st.kind == MD_FWD_SKINNY) {
        GA_REQUIRE(st.sp.w_kc && st.sp.epi == 0 && st.sp.KV >= 1 && st.sp.KV <= 8 &&
                       (skinny_kv[st.layer] == 0 || skinny_kv[st.layer] == st.sp.KV),
                   "%s: member %lld: streaming forward not instantiated", who, (long long)m);
        skinny_kv[st.layer] = st.sp.KV;
        if (st.sp.lds_bytes > skinny_lds[st.layer]) skinny_lds[st.layer] = st.sp.lds_bytes;
        MdSkinnyEntry e;
        e.p = st.s; e.gx = st.sp.gx; e.gy = st.sp.gy;
        skinny[st.layer].push_back(e);
      } else if (st.kind == MD_FWD_GEMM_HEAD) {
        GA_REQUIRE(st.hp.width == 64 && st.hp.threads == 256,
                   "%s: member %lld: head GEMM of width %d not instantiated", who,
                   (long long)m, st.hp.width);
        gemm[st.layer][MD_GEMM_HEAD_64].push_back(st.g);
      } else {
        GA_REQUIRE(st.gp.tile == GT_128x32 || st.gp.tile == GT_64x64,
                   "%s: member %lld: GEMM tile %d not instantiated", who, (long long)m,
                   (int)st.gp.tile);
        gemm[st.layer][st.gp.tile == GT_128x32 ? MD_GEMM_128x32 : MD_GEMM_64x64].push_back(
            st.g);
      }
    }
  }
  TableLayout lay;
  size_t sk_at[3], g_at[3][MD_GEMM_KINDS];
  for (int l = 0; l < 3; ++l) {
    sk_at[l] = lay.add(skinny[l].size() * sizeof(MdSkinnyEntry));
    for (int k = 0; k < MD_GEMM_KINDS; ++k)
      g_at[l][k] = lay.add(gemm[l][k].size() * sizeof(GemmParams));
  }
  return with_tables(
      who, lay.bytes, stream,
      [&](char* host) {
        for (int l = 0; l < 3; ++l) {
          if (!skinny[l].empty())
            memcpy(host + sk_at[l], skinny[l].data(), skinny[l].size() * sizeof(MdSkinnyEntry));
          for (int k = 0; k < MD_GEMM_KINDS; ++k)
            if (!gemm[l][k].empty())
              memcpy(host + g_at[l][k], gemm[l][k].data(),
                     gemm[l][k].size() * sizeof(GemmParams));
        }
      },
      [&](char* dev) {
        // layer by layer: an entry's layer l reads what its layer l - 1 wrote
        for (int l = 0; l < 3; ++l) {
          if (!skinny[l].empty()) {
            unsigned gx = 0, gy = 0;
            for (const MdSkinnyEntry& e : skinny[l]) {
              if (e.gx > gx) gx = e.gx;
              if (e.gy > gy) gy = e.gy;
            }
            const int r = md_launch_skinny_fwd_members(
                skinny_kv[l], reinterpret_cast<const MdSkinnyEntry*>(dev + sk_at[l]),
                (unsigned)skinny[l].size(), gx, gy, skinny_lds[l], stream);
            if (r) return r;
          }
          for (int k = 0; k < MD_GEMM_KINDS; ++k) {
            if (gemm[l][k].empty()) continue;
            unsigned blocks = 0;
            for (const GemmParams& p : gemm[l][k]) {
              const unsigned b = (unsigned)(p.gx * p.gy * p.gz);
              if (b > blocks) blocks = b;
            }
            const int r = md_launch_gemm_members(
                k, reinterpret_cast<const GemmParams*>(dev + g_at[l][k]),
                (unsigned)gemm[l][k].size(), blocks, stream);
            if (r) return r;
          }
        }
        return (int)GA_OK;
      });
}

// ---------------------------------------------------------------------------------------
// policy loss
// ---------------------------------------------------------------------------------------
extern "C" int ga_ppo_loss_members_f32(const ga_members_loss_args* a,
                                       const ga_member_loss* members, int64_t n,
                                       double* partials, int64_t partials_doubles,
                                       ga_stream_t stream_) {
  const char* who = "ga_ppo_loss_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(a, "%s: null pointer", who);
  int rc = check_count(who, members, n, 2 * MAX_MEMBERS);
  if (rc) return rc;
  GA_REQUIRE(a->kind == 0 || a->kind == 2, "%s: kind must be 0 (Gaussian) or 2 (categorical)",
             who);
  GA_REQUIRE(a->algo == 0 || a->algo == 1, "%s: algo must be 0 or 1", who);
  GA_REQUIRE(a->A >= 1 && a->A <= 8, "%s: A must be 1 .. 8", who);
  const bool cat = a->kind == 2;
  std::vector<int64_t> rows;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_loss& u = members[m];
    GA_REQUIRE(u.head && u.actions && u.adv && u.loss_out && (cat || u.log_std),
               "%s: member %lld: null pointer", who, (long long)m);
    GA_REQUIRE(a->algo == 1 || u.old_ll, "%s: member %lld: PPO needs old_ll", who,
               (long long)m);
    GA_REQUIRE(u.rows >= 1 && u.rows < ROWS_LIMIT, "%s: member %lld: bad rows", who,
               (long long)m);
    GA_REQUIRE(u.ld >= a->A && u.lda >= (cat ? 1 : a->A), "%s: member %lld: bad strides", who,
               (long long)m);
    rows.push_back(u.rows);
  }
  std::vector<int64_t> off;
  rc = partials_offsets(who, rows, 2, partials, partials_doubles, &off);
  if (rc) return rc;
  int64_t n_multi = 0;
  unsigned blocks = 1;
  for (int64_t r : rows) {
    const unsigned nb = (unsigned)ga_red_blocks(r);
    n_multi += nb > 1;
    if (nb > blocks) blocks = nb;
  }
  TableLayout lay;
  const size_t row_at = lay.add((size_t)n * (cat ? sizeof(MdCatEntry) : sizeof(MdPpoEntry)));
  const size_t fin_at =
      lay.add((size_t)n_multi * (cat ? sizeof(MdCatFinalize) : sizeof(PpoFinalizeParams)));
  return with_tables(
      who, lay.bytes, stream,
      [&](char* host) {
        int64_t f = 0;
        for (int64_t m = 0; m < n; ++m) {
          const ga_member_loss& u = members[m];
          const unsigned nb = (unsigned)ga_red_blocks(u.rows);
          double* part = partials + off[m];
          if (cat) {
            MdCatEntry& e = reinterpret_cast<MdCatEntry*>(host + row_at)[m];
            CatLossParams& p = e.p;
            p.scores = u.head; p.lds = u.ld; p.actions = u.actions; p.lda = u.lda;
            p.old_ll = u.old_ll; p.adv = u.adv; p.idx = nullptr; p.M = u.rows; p.A = a->A;
            p.double_softmax = a->double_softmax; p.algo = a->algo; p.clip = u.clip;
            p.ent = lr_ent(u.ent_coeff, a->ent_flags);
            p.partials = part; p.ent_sum_out = u.ent_sum_out;
            p.loss_out = nb == 1 ? u.loss_out : nullptr;
            e.nb = nb;
            if (nb > 1) {
              MdCatFinalize& q = reinterpret_cast<MdCatFinalize*>(host + fin_at)[f++];
              q.partials = part; q.nblocks = (int)nb; q.M = u.rows; q.loss_out = u.loss_out;
              q.ent_sum_out = u.ent_sum_out;
            }
          } else {
            MdPpoEntry& e = reinterpret_cast<MdPpoEntry*>(host + row_at)[m];
            PpoLossParams& p = e.p;
            p.mean = u.head; p.ldm = u.ld; p.actions = u.actions; p.lda = u.lda;
            p.old_ll = u.old_ll; p.adv = u.adv; p.idx = nullptr; p.log_std = u.log_std;
            p.min_log_std = a->min_log_std; p.has_min = a->has_min;
            p.max_log_std = a->max_log_std; p.has_max = a->has_max; p.M = u.rows; p.A = a->A;
            p.algo = a->algo; p.clip = u.clip; p.ent = lr_ent(u.ent_coeff, a->ent_flags);
            p.partials = part;
            p.loss_out = nb == 1 ? u.loss_out : nullptr;
            e.nb = nb;
            if (nb > 1) {
              PpoFinalizeParams& q = reinterpret_cast<PpoFinalizeParams*>(host + fin_at)[f++];
              q.partials = part; q.nblocks = (int)nb; q.log_std = u.log_std;
              q.min_log_std = a->min_log_std; q.max_log_std = a->max_log_std;
              q.has_min = a->has_min; q.has_max = a->has_max; q.M = u.rows; q.A = a->A;
              q.ent = p.ent; q.loss_out = u.loss_out;
            }
          }
        }
      },
      [&](char* dev) {
        int r = cat ? md_launch_ppo_categorical_members(
                          reinterpret_cast<const MdCatEntry*>(dev + row_at), (unsigned)n, blocks,
                          stream)
                    : md_launch_ppo_gaussian_members(
                          reinterpret_cast<const MdPpoEntry*>(dev + row_at), (unsigned)n, blocks,
                          stream);
        if (r || n_multi == 0) return r;
        return cat ? md_launch_ppo_categorical_finalize_members(
                         reinterpret_cast<const MdCatFinalize*>(dev + fin_at),
                         (unsigned)n_multi, stream)
                   : md_launch_ppo_gaussian_finalize_members(
                         reinterpret_cast<const PpoFinalizeParams*>(dev + fin_at),
                         (unsigned)n_multi, stream);
      });
}

// ---------------------------------------------------------------------------------------
// value loss
// ---------------------------------------------------------------------------------------
extern "C" int ga_gaussian_nll_members_f32(const ga_member_nll* members, int64_t n,
                                           double* partials, int64_t partials_doubles,
                                           ga_stream_t stream_) {
  const char* who = "ga_gaussian_nll_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_count(who, members, n, MAX_MEMBERS);
  if (rc) return rc;
  std::vector<int64_t> rows;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_nll& u = members[m];
    GA_REQUIRE(u.v && u.returns && u.log_std && u.loss_out, "%s: member %lld: null pointer",
               who, (long long)m);
    GA_REQUIRE(u.rows >= 1 && u.rows < ROWS_LIMIT, "%s: member %lld: bad rows", who,
               (long long)m);
    GA_REQUIRE(u.ldv >= 1, "%s: member %lld: bad strides", who, (long long)m);
    rows.push_back(u.rows);
  }
  std::vector<int64_t> off;
  rc = partials_offsets(who, rows, 2, partials, partials_doubles, &off);
  if (rc) return rc;
  int64_t n_multi = 0;
  unsigned blocks = 1;
  for (int64_t r : rows) {
    const unsigned nb = (unsigned)ga_red_blocks(r);
    n_multi += nb > 1;
    if (nb > blocks) blocks = nb;
  }
  TableLayout lay;
  const size_t row_at = lay.add((size_t)n * sizeof(MdNllEntry));
  const size_t fin_at = lay.add((size_t)n_multi * sizeof(MdNllFinalize));
  return with_tables(
      who, lay.bytes, stream,
      [&](char* host) {
        int64_t f = 0;
        for (int64_t m = 0; m < n; ++m) {
          const ga_member_nll& u = members[m];
          const unsigned nb = (unsigned)ga_red_blocks(u.rows);
          MdNllEntry& e = reinterpret_cast<MdNllEntry*>(host + row_at)[m];
          e.p.v = u.v; e.p.ldv = u.ldv; e.p.returns = u.returns; e.p.idx = nullptr;
          e.p.log_std = u.log_std; e.p.M = u.rows; e.p.partials = partials + off[m];
          e.p.loss_out = nb == 1 ? u.loss_out : nullptr;
          e.nb = nb;
          if (nb > 1) {
            MdNllFinalize& q = reinterpret_cast<MdNllFinalize*>(host + fin_at)[f++];
            q.partials = partials + off[m]; q.nblocks = (int)nb; q.M = u.rows;
            q.loss_out = u.loss_out;
          }
        }
      },
      [&](char* dev) {
        const int r = md_launch_nll_members(reinterpret_cast<const MdNllEntry*>(dev + row_at),
                                            (unsigned)n, blocks, stream);
        if (r || n_multi == 0) return r;
        return md_launch_nll_finalize_members(
            reinterpret_cast<const MdNllFinalize*>(dev + fin_at), (unsigned)n_multi, stream);
      });
}

// ---------------------------------------------------------------------------------------
// KL
// ---------------------------------------------------------------------------------------
extern "C" int ga_kl_members_f32(int categorical, int A, int double_softmax,
                                 const ga_member_kl* members, int64_t n, double* partials,
                                 int64_t partials_doubles, ga_stream_t stream_) {
  const char* who = "ga_kl_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_count(who, members, n, 2 * MAX_MEMBERS);
  if (rc) return rc;
  GA_REQUIRE(A >= 1 && A <= 8, "%s: A must be 1 .. 8", who);
  std::vector<int64_t> rows;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_kl& u = members[m];
    GA_REQUIRE(u.head_old && u.head_new && u.kl_sum_out, "%s: member %lld: null pointer", who,
               (long long)m);
    GA_REQUIRE(u.rows >= 1 && u.rows < ROWS_LIMIT, "%s: member %lld: bad rows", who,
               (long long)m);
    GA_REQUIRE(u.ld >= A, "%s: member %lld: bad strides", who, (long long)m);
    rows.push_back(u.rows);
  }
  std::vector<int64_t> off;
  rc = partials_offsets(who, rows, 1, partials, partials_doubles, &off);
  if (rc) return rc;
  unsigned blocks = 1;
  for (int64_t r : rows)
    if ((unsigned)ga_red_blocks(r) > blocks) blocks = (unsigned)ga_red_blocks(r);
  TableLayout lay;
  const size_t row_at = lay.add((size_t)n * sizeof(MdKlEntry));
  const size_t sum_at = lay.add((size_t)n * sizeof(MdSum));
  return with_tables(
      who, lay.bytes, stream,
      [&](char* host) {
        for (int64_t m = 0; m < n; ++m) {
          const ga_member_kl& u = members[m];
          MdKlEntry& e = reinterpret_cast<MdKlEntry*>(host + row_at)[m];
          e.head_old = u.head_old; e.head_new = u.head_new; e.ld = u.ld; e.M = u.rows;
          e.A = A; e.dbl = double_softmax; e.s_old = u.log_std_old; e.s_new = u.log_std_new;
          e.partials = partials + off[m]; e.nb = (unsigned)ga_red_blocks(u.rows);
          MdSum& q = reinterpret_cast<MdSum*>(host + sum_at)[m];
          q.partials = e.partials; q.nblocks = (int)e.nb; q.out = u.kl_sum_out;
        }
      },
      [&](char* dev) {
        const int r = md_launch_kl_members(categorical != 0,
                                           reinterpret_cast<const MdKlEntry*>(dev + row_at),
                                           (unsigned)n, blocks, stream);
        if (r) return r;
        // (as the lone entries: every member's sum is a second launch, one block or many)
        return md_launch_sum_members(reinterpret_cast<const MdSum*>(dev + sum_at), (unsigned)n,
                                     stream);
      });
}

// ---------------------------------------------------------------------------------------
// log_performance
// ---------------------------------------------------------------------------------------
extern "C" int ga_episode_stats_members_f32(const ga_member_episodes* members, int64_t n,
                                            int terminal, ga_stream_t stream_) {
  const char* who = "ga_episode_stats_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_count(who, members, n, MAX_MEMBERS);
  if (rc) return rc;
  int64_t most = 0;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_episodes& u = members[m];
    GA_REQUIRE(u.rewards && u.ep_off && u.returns && u.step_types && u.out,
               "%s: member %lld: null pointer", who, (long long)m);
    GA_REQUIRE(u.n_eps >= 1 && u.n_eps < ROWS_LIMIT, "%s: member %lld: bad n_eps", who,
               (long long)m);
    if (u.n_eps > most) most = u.n_eps;
  }
  TableLayout lay;
  const size_t at = lay.add((size_t)n * sizeof(MdEpisodes));
  return with_tables(
      who, lay.bytes, stream,
      [&](char* host) {
        for (int64_t m = 0; m < n; ++m) {
          const ga_member_episodes& u = members[m];
          MdEpisodes& e = reinterpret_cast<MdEpisodes*>(host + at)[m];
          e.rewards = u.rewards; e.ep_off = u.ep_off; e.n_eps = u.n_eps;
          e.returns = u.returns; e.step_types = u.step_types; e.terminal = terminal;
          e.out = u.out;
        }
      },
      [&](char* dev) {
        return md_launch_episodes_members(reinterpret_cast<const MdEpisodes*>(dev + at),
                                          (unsigned)n, (unsigned)ga_ceil_div(most, 256),
                                          stream);
      });
}
