// The host side of the linear feature baseline's kernels (linear_baseline.hip): every
// extern "C" entry point -- its argument checks, the kernels' parameter structs, the grids
// and the Gram pass's instantiation and LDS size.  Host C++ only: the launches go through
// the seam of linear_baseline_params.h, so that this file builds for the CPU harness under
// tests/host (linear_baseline_harness.cpp) too.
//
//   ga_linear_features_gram_f64     featmat.T.dot(featmat) and featmat.T.dot(returns) of
//                                   LinearFeatureBaseline.fit with _features' rows
//                                   (np/baselines/linear_feature_baseline.py:43-58,68-75)
//   ga_linear_features_predict_f32  _features(path).dot(self._coeffs) of predict
//                                   (linear_feature_baseline.py:91-93), a whole batch
// (a population's entries, every member in one launch: linear_baseline_members_host.cpp)
#include "common.h"
#include "linear_baseline_checks.h"
#include "linear_baseline_params.h"

extern "C" int ga_linear_features_supported(int obs_dim) {
  return obs_dim >= 1 && obs_dim <= LB_MAX_OBS;
}

extern "C" int64_t ga_linear_gram_workspace_doubles(int obs_dim, int64_t S) {
  if (!ga_linear_features_supported(obs_dim) || S < 1 || S >= (1ll << 31)) return -1;
  return lb_gram_blocks(S) * lb_block_doubles(obs_dim);
}

extern "C" int ga_linear_features_gram_f64(const float* obs, int64_t ldo, int obs_dim,
                                           const int64_t* ep_off, int64_t n_eps, int64_t S,
                                           const float* returns, double* gram, double* rhs,
                                           double* workspace, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "ga_linear_features_gram_f64";
  if (int rc = lb_batch_refused(who, obs, ldo, obs_dim, ep_off, n_eps, S)) return rc;
  GA_REQUIRE(returns && gram && rhs && workspace, "%s: null pointer", who);
  GA_REQUIRE(((uintptr_t)gram & 7) == 0 && ((uintptr_t)rhs & 7) == 0 &&
                 ((uintptr_t)workspace & 7) == 0,
             "%s: gram, rhs and workspace must be 8-byte aligned", who);
  LinGramParams p;
  p.obs = obs; p.ldo = ldo; p.obs_dim = obs_dim; p.ep_off = ep_off; p.n_eps = n_eps;
  p.S = S; p.returns = returns; p.partials = workspace;
  p.block_doubles = lb_block_doubles(obs_dim); p.n_slabs = lb_slabs(S);
  p.F = lb_features(obs_dim); p.T = lb_tiles(obs_dim); p.NT = lb_upper_tiles(obs_dim);
  p.tpw = lb_tiles_per_wave(obs_dim); p.chunk_rows = lb_chunk_rows(obs_dim);
  const int blocks = lb_gram_blocks(S);
  lb_launch_gram(p, (unsigned)blocks, lb_gram_lds_bytes(obs_dim, p.chunk_rows), stream);
  GA_CHECK_LAUNCH("linear_features_gram");
  LinReduceParams r;
  r.partials = workspace; r.n_blocks = blocks; r.block_doubles = p.block_doubles;
  r.F = p.F; r.T = p.T; r.NT = p.NT; r.gram = gram; r.rhs = rhs;
  lb_launch_gram_reduce(r, (unsigned)ga_ceil_div(p.block_doubles, LB_REDUCE_THREADS), stream);
  GA_CHECK_LAUNCH("linear_features_gram_reduce");
  return GA_OK;
}

extern "C" int ga_linear_features_predict_f32(const float* obs, int64_t ldo, int obs_dim,
                                              const int64_t* ep_off, int64_t n_eps, int64_t S,
                                              const double* coeffs, float* values,
                                              int64_t ldv, ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* who = "ga_linear_features_predict_f32";
  if (int rc = lb_batch_refused(who, obs, ldo, obs_dim, ep_off, n_eps, S)) return rc;
  GA_REQUIRE(coeffs && values, "%s: null pointer", who);
  GA_REQUIRE(((uintptr_t)coeffs & 7) == 0, "%s: coeffs must be 8-byte aligned", who);
  GA_REQUIRE(ldv >= 1, "%s: ldv %lld < 1", who, (long long)ldv);
  LinPredictParams p;
  p.obs = obs; p.ldo = ldo; p.obs_dim = obs_dim; p.ep_off = ep_off; p.n_eps = n_eps;
  p.S = S; p.coeffs = coeffs; p.values = values; p.ldv = ldv;
  lb_launch_predict(p, (unsigned)ga_ceil_div(S, LB_PREDICT_THREADS), stream);
  GA_CHECK_LAUNCH("linear_features_predict");
  return GA_OK;
}
