// Every member's returns, advantages and advantage normalisation in one launch: the host
// side of ga_advantages_members_f32 -- argument checks, each member's table entry (the
// parameter struct its lone ga_gae_scan_f32 launch would get, by the ONE rule of
// gae_scan_params.h), one asynchronous copy of the table and one launch whatever the
// member count.  Nothing falls back to per-member launches.  Host C++ only: the launch
// goes through the seam of members_advantage.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "internal.h"
#include "members_advantage.h"
#include "table_slots.h"

namespace {
constexpr int64_t MAX_MEMBERS = 1024;
// the table of a call goes through a ring of pinned / device slots (table_slots.h)
GaTableRing g_ring;
}  // namespace

extern "C" int ga_advantages_members_f32(const ga_member_advantage* members, int64_t n,
                                         int max_episode_length, double discount,
                                         double gae_lambda, int center, int positive,
                                         ga_stream_t stream_) {
  const char* who = "ga_advantages_members_f32";
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(members, "%s: null pointer", who);
  GA_REQUIRE(n >= 1 && n <= MAX_MEMBERS, "%s: n_members must be 1 .. %lld", who,
             (long long)MAX_MEMBERS);
  GA_REQUIRE(max_episode_length >= 1, "%s: max_episode_length < 1", who);
  int64_t most = 0;
  double steps = 0.0;
  for (int64_t m = 0; m < n; ++m) {
    const ga_member_advantage& u = members[m];
    GA_REQUIRE(u.rewards && u.values && u.adv && u.ret && u.stats,
               "%s: member %lld: null pointer", who, (long long)m);
    GA_REQUIRE((reinterpret_cast<uintptr_t>(u.stats) & 7u) == 0,
               "%s: member %lld: stats must be 8-byte aligned", who, (long long)m);
    GA_REQUIRE(u.n_rows >= 1 && u.T >= 1, "%s: member %lld: S < 1 (n_rows %lld, T %lld)", who,
               (long long)m, (long long)u.n_rows, (long long)u.T);
    int64_t S = u.T;  // packed: T carries the total step count, as ga_gae_scan_f32's
    if (!u.offsets) {
      GA_REQUIRE(u.ld >= u.T, "%s: member %lld: ld (%lld) < T (%lld)", who, (long long)m,
                 (long long)u.ld, (long long)u.T);
      GA_REQUIRE(u.T <= MA_MAX_STEPS && u.n_rows <= MA_MAX_STEPS,
                 "%s: member %lld: S > MA_MAX_STEPS (%d)", who, (long long)m, MA_MAX_STEPS);
      S = u.n_rows * u.T;
    } else {
      GA_REQUIRE(u.max_len >= 1 && u.max_len <= u.T,
                 "%s: member %lld: max_len must be 1 .. T with offsets", who, (long long)m);
      GA_REQUIRE(u.n_rows <= u.T, "%s: member %lld: more rows than steps", who, (long long)m);
    }
    GA_REQUIRE(S <= MA_MAX_STEPS, "%s: member %lld: S (%lld) > MA_MAX_STEPS (%d)", who,
               (long long)m, (long long)S, MA_MAX_STEPS);
    if (S > most) most = S;
    steps += (double)S;
  }
  const size_t bytes = (size_t)n * sizeof(MaEntry);
  return ga_with_tables(
      g_ring, who, bytes, stream,
      [&](char* host) {
        MaEntry* table = reinterpret_cast<MaEntry*>(host);
        for (int64_t m = 0; m < n; ++m) {
          const ga_member_advantage& u = members[m];
          MaEntry& e = table[m];
          GaScanPlan plan;
          memset(&plan, 0, sizeof(plan));
          // (mode 1, no per-step bonus, no tail flags; v0 is read on the device)
          ga_gae_scan_plan(u.rewards, u.values, nullptr, nullptr, u.offsets, u.n_rows, u.T,
                           u.ld, u.offsets ? u.max_len : u.T, 1, max_episode_length, discount,
                           gae_lambda, 0.0, u.bonus_const, u.adv, u.ret, &plan);
          e.kernel = plan.kernel;
          e.waves = plan.waves;
          e.S = u.offsets ? u.T : u.n_rows * u.T;
          e.flags = (center ? MA_CENTER : 0) | (positive ? MA_POSITIVE : 0) |
                    ((u.offsets || u.ld == u.T) ? MA_PACKED : 0);
          e.v0 = u.v0;
          e.adv = u.adv;
          e.stats = u.stats;
          e.g = plan.p;
          e.r = plan.f;
        }
      },
      [&](char* dev) {
        return ma_launch_advantage_members(reinterpret_cast<const MaEntry*>(dev), (unsigned)n,
                                           (unsigned)(4 * ((most + 3) & ~(int64_t)3)),
                                           16.0 * steps, stream);
      });
}
