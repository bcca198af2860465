// The host side of the linear feature baseline's device solve: argument checks, the member
// table and the grid of ONE launch that solves every member's F x F system
// (linear_solve.hip).  A file of its own beside linear_baseline_members_host.cpp, with a
// seam of its own (linear_solve_params.h).  Host C++ only.
//
//   ga_linear_solve_members_f64   np.linalg.lstsq(featmat.T.dot(featmat) + reg_coeff *
//                                 identity, featmat.T.dot(returns)) and the retry loop
//                                 around it, of LinearFeatureBaseline.fit
//                                 (np/baselines/linear_feature_baseline.py:70-79), for
//                                 n_members baselines
//
// The member table is built in pinned host memory and uploaded once per call through the
// ring of table_slots.h, as the Gram and predict entries' tables are.
#include <math.h>
#include <string.h>

#include "common.h"
#include "linear_solve_params.h"
#include "table_slots.h"

namespace {

constexpr int64_t MAX_MEMBERS = 1024;

GaTableRing g_ring;

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" int64_t ga_linear_solve_workspace_doubles(int obs_dim, int64_t n_members) {
  if (!ga_linear_features_supported(obs_dim) || n_members < 1 || n_members > MAX_MEMBERS)
    return -1;
  return n_members * ls_member_doubles(obs_dim);
}

extern "C" int ga_linear_solve_members_f64(const ga_linear_solve_member* members_host,
                                           int64_t n_members, int obs_dim, double* workspace,
                                           int64_t workspace_doubles, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* entry = "ga_linear_solve_members_f64";
  GA_REQUIRE(members_host && workspace, "%s: null pointer", entry);
  GA_REQUIRE(n_members >= 1 && n_members <= MAX_MEMBERS, "%s: n_members must be 1 .. %lld",
             entry, (long long)MAX_MEMBERS);
  GA_REQUIRE(ga_linear_features_supported(obs_dim), "%s: obs_dim %d outside 1 .. 128", entry,
             obs_dim);
  GA_REQUIRE(aligned8(workspace), "%s: workspace must be 8-byte aligned", entry);
  for (int64_t m = 0; m < n_members; ++m) {
    const ga_linear_solve_member& u = members_host[m];
    GA_REQUIRE(u.gram && u.rhs && u.coeffs && u.status, "%s: member %lld: null pointer", entry,
               (long long)m);
    GA_REQUIRE(aligned8(u.gram) && aligned8(u.rhs) && aligned8(u.coeffs),
               "%s: member %lld: gram, rhs and coeffs must be 8-byte aligned", entry,
               (long long)m);
    GA_REQUIRE(((uintptr_t)u.status & 3) == 0, "%s: member %lld: status must be 4-byte aligned",
               entry, (long long)m);
    GA_REQUIRE(isfinite(u.reg_coeff) && u.reg_coeff >= 0.0,
               "%s: member %lld: reg_coeff must be finite and >= 0", entry, (long long)m);
  }
  const int64_t member_doubles = ls_member_doubles(obs_dim);
  GA_REQUIRE(workspace_doubles >= n_members * member_doubles,
             "%s: workspace too small (%lld doubles, %lld needed)", entry,
             (long long)workspace_doubles, (long long)(n_members * member_doubles));

  return ga_with_tables(
      g_ring, entry, (size_t)n_members * sizeof(LinSolveMemberDev), stream,
      [&](char* host) {
        LinSolveMemberDev* table = reinterpret_cast<LinSolveMemberDev*>(host);
        for (int64_t m = 0; m < n_members; ++m) {
          const ga_linear_solve_member& u = members_host[m];
          LinSolveMemberDev& t = table[m];
          t.gram = u.gram; t.rhs = u.rhs; t.reg_coeff = u.reg_coeff;
          t.coeffs = u.coeffs; t.status = u.status;
          t.factor = workspace + m * member_doubles;
        }
      },
      [&](char* dev) {
        LinSolveParams p;
        p.members = reinterpret_cast<const LinSolveMemberDev*>(dev);
        p.n_members = (int)n_members;
        p.F = ls_features(obs_dim); p.T = ls_tiles(obs_dim);
        ls_launch_solve_members(p, (unsigned)n_members, stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
          ga_set_error("%s: launch failed: %s", entry, hipGetErrorString(e));
          return GA_ERR_HIP;
        }
        return GA_OK;
      });
}
