// The host side of the linear feature baseline for a POPULATION: every member's Gram pass
// in one launch (and one reduce launch), every member's predictions in one launch.  A file
// of its own beside linear_baseline_host.cpp, whose checks (linear_baseline_checks.h) and
// shape rules (linear_baseline_params.h) it shares: it stages a table, and so calls the HIP
// runtime and three more functions of the launch seam, which the lone entries' harness does
// not fake.  Host C++ only; tests/host/linear_baseline_members_harness.cpp builds it for
// the CPU.
//
//   ga_linear_features_gram_members_f64     featmat.T.dot(featmat), featmat.T.dot(returns)
//                                           of LinearFeatureBaseline.fit for n_members
//                                           baselines (np/baselines/
//                                           linear_feature_baseline.py:43-58,68-75)
//   ga_linear_features_predict_members_f32  _features(path).dot(self._coeffs) of predict
//                                           (linear_feature_baseline.py:91-93), n_members
//                                           whole batches
//
// The member table -- pointers, sizes and each member's first workgroup -- is built in
// pinned host memory and uploaded once per call through the ring of table_slots.h, as
// ga_update_epoch_members' tables are.
#include <string.h>

#include <mutex>

#include "common.h"
#include "linear_baseline_checks.h"
#include "linear_baseline_params.h"
#include "table_slots.h"

namespace {

constexpr int64_t MAX_MEMBERS = 1024;

GaTableRing g_ring;  // both entry points' tables

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// "<entry>: member <m>" for the checks' messages
struct Who {
  char text[96];
  Who(const char* entry, int64_t m) {
    snprintf(text, sizeof(text), "%s: member %lld", entry, (long long)m);
  }
};

}  // namespace

extern "C" int64_t ga_linear_gram_members_workspace_doubles(int obs_dim, int64_t n_members,
                                                            const int64_t* S) {
  if (obs_dim < 1 || obs_dim > LB_MAX_OBS || !S || n_members < 1 ||
      n_members > MAX_MEMBERS)
    return -1;
  int64_t blocks = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    if (S[m] < 1 || S[m] >= (1ll << 31)) return -1;
    blocks += lb_gram_blocks(S[m]);
  }
  return blocks * lb_block_doubles(obs_dim);
}

extern "C" void ga_linear_members_release(void) { g_ring.release(); }

extern "C" int ga_linear_features_gram_members_f64(const ga_linear_gram_member* members_host,
                                                   int64_t n_members, int obs_dim,
                                                   double* workspace,
                                                   int64_t workspace_doubles,
                                                   ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* entry = "ga_linear_features_gram_members_f64";
  GA_REQUIRE(members_host && workspace, "%s: null pointer", entry);
  GA_REQUIRE(n_members >= 1 && n_members <= MAX_MEMBERS, "%s: n_members must be 1 .. %lld",
             entry, (long long)MAX_MEMBERS);
  GA_REQUIRE(aligned8(workspace), "%s: workspace must be 8-byte aligned", entry);
  int64_t blocks = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    const ga_linear_gram_member& u = members_host[m];
    const Who who(entry, m);
    if (int rc = lb_batch_refused(who.text, u.obs, u.ldo, obs_dim, u.ep_off, u.n_eps, u.S))
      return rc;
    GA_REQUIRE(u.returns && u.gram && u.rhs, "%s: null pointer", who.text);
    GA_REQUIRE(aligned8(u.gram) && aligned8(u.rhs), "%s: gram and rhs must be 8-byte aligned",
               who.text);
    blocks += lb_gram_blocks(u.S);
  }
  const int64_t block_doubles = lb_block_doubles(obs_dim);
  GA_REQUIRE(workspace_doubles >= blocks * block_doubles,
             "%s: workspace too small (%lld doubles, %lld needed)", entry,
             (long long)workspace_doubles, (long long)(blocks * block_doubles));

  const size_t bytes = (size_t)n_members * sizeof(LinGramMemberDev);
  std::lock_guard<std::mutex> lock(g_ring.mu);
  GaTableSlot* slot = g_ring.take(bytes);
  if (!slot) {
    ga_set_error("%s: cannot allocate the member table", entry);
    return GA_ERR_HIP;
  }
  LinGramMemberDev* table = static_cast<LinGramMemberDev*>(slot->host);
  memset(table, 0, bytes);
  int64_t block0 = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    const ga_linear_gram_member& u = members_host[m];
    LinGramMemberDev& t = table[m];
    t.obs = u.obs; t.ldo = u.ldo; t.ep_off = u.ep_off; t.n_eps = u.n_eps; t.S = u.S;
    t.returns = u.returns; t.gram = u.gram; t.rhs = u.rhs;
    t.partials = workspace + block0 * block_doubles;
    t.n_slabs = lb_slabs(u.S);
    t.block0 = (int32_t)block0;
    t.n_blocks = lb_gram_blocks(u.S);
    block0 += t.n_blocks;
  }
  LinGramMembersParams p;
  p.members = static_cast<const LinGramMemberDev*>(slot->dev);
  p.n_members = (int)n_members; p.obs_dim = obs_dim; p.block_doubles = block_doubles;
  p.F = lb_features(obs_dim); p.T = lb_tiles(obs_dim); p.NT = lb_upper_tiles(obs_dim);
  p.tpw = lb_tiles_per_wave(obs_dim); p.chunk_rows = lb_chunk_rows(obs_dim);
  int rc = GA_OK;
  if (!GaTableRing::upload(slot, bytes, stream)) {
    ga_set_error("%s: table upload failed", entry);
    rc = GA_ERR_HIP;
  }
  if (!rc) {
    lb_launch_gram_members(p, (unsigned)blocks, lb_gram_lds_bytes(obs_dim, p.chunk_rows),
                           stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
      lb_launch_gram_reduce_members(
          p, (unsigned)ga_ceil_div(block_doubles, LB_REDUCE_THREADS), stream);
      e = hipGetLastError();
    }
    if (e != hipSuccess) {
      ga_set_error("%s: launch failed: %s", entry, hipGetErrorString(e));
      rc = GA_ERR_HIP;
    }
  }
  if (!GaTableRing::mark_done(slot, stream) && !rc) {
    ga_set_error("%s: hipEventRecord failed", entry);
    rc = GA_ERR_HIP;
  }
  return rc;
}

extern "C" int ga_linear_features_predict_members_f32(
    const ga_linear_predict_member* members_host, int64_t n_members, int obs_dim,
    ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* entry = "ga_linear_features_predict_members_f32";
  GA_REQUIRE(members_host, "%s: null pointer", entry);
  GA_REQUIRE(n_members >= 1 && n_members <= MAX_MEMBERS, "%s: n_members must be 1 .. %lld",
             entry, (long long)MAX_MEMBERS);
  int64_t blocks = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    const ga_linear_predict_member& u = members_host[m];
    const Who who(entry, m);
    if (int rc = lb_batch_refused(who.text, u.obs, u.ldo, obs_dim, u.ep_off, u.n_eps, u.S))
      return rc;
    GA_REQUIRE(u.values, "%s: null pointer", who.text);
    GA_REQUIRE(aligned8(u.coeffs), "%s: coeffs must be 8-byte aligned", who.text);
    GA_REQUIRE(u.ldv >= 1, "%s: ldv %lld < 1", who.text, (long long)u.ldv);
    blocks += ga_ceil_div(u.S, LB_PREDICT_THREADS);
  }
  GA_REQUIRE(blocks < (1ll << 31), "%s: %lld workgroups: the members' samples exceed one grid",
             entry, (long long)blocks);

  const size_t bytes = (size_t)n_members * sizeof(LinPredictMemberDev);
  std::lock_guard<std::mutex> lock(g_ring.mu);
  GaTableSlot* slot = g_ring.take(bytes);
  if (!slot) {
    ga_set_error("%s: cannot allocate the member table", entry);
    return GA_ERR_HIP;
  }
  LinPredictMemberDev* table = static_cast<LinPredictMemberDev*>(slot->host);
  memset(table, 0, bytes);
  int64_t block0 = 0;
  for (int64_t m = 0; m < n_members; ++m) {
    const ga_linear_predict_member& u = members_host[m];
    LinPredictMemberDev& t = table[m];
    t.obs = u.obs; t.ldo = u.ldo; t.ep_off = u.ep_off; t.n_eps = u.n_eps; t.S = u.S;
    t.coeffs = u.coeffs; t.values = u.values; t.ldv = u.ldv;
    t.block0 = block0;
    block0 += ga_ceil_div(u.S, LB_PREDICT_THREADS);
  }
  LinPredictMembersParams p;
  p.members = static_cast<const LinPredictMemberDev*>(slot->dev);
  p.n_members = (int)n_members; p.obs_dim = obs_dim;
  int rc = GA_OK;
  if (!GaTableRing::upload(slot, bytes, stream)) {
    ga_set_error("%s: table upload failed", entry);
    rc = GA_ERR_HIP;
  }
  if (!rc) {
    lb_launch_predict_members(p, (unsigned)blocks, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      ga_set_error("%s: launch failed: %s", entry, hipGetErrorString(e));
      rc = GA_ERR_HIP;
    }
  }
  if (!GaTableRing::mark_done(slot, stream) && !rc) {
    ga_set_error("%s: hipEventRecord failed", entry);
    rc = GA_ERR_HIP;
  }
  return rc;
}
