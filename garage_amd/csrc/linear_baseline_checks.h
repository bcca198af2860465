// What every pass of the linear feature baseline asks of a batch, stated once for the lone
// entries (linear_baseline_host.cpp) and the population's (linear_baseline_members_host.cpp).
// Host C++ only.
#pragma once
#include "common.h"
#include "linear_baseline_params.h"

// `who` names the entry point (and, in a population, the member)
inline int lb_batch_refused(const char* who, const float* obs, int64_t ldo, int obs_dim,
                            const int64_t* ep_off, int64_t n_eps, int64_t S) {
  GA_REQUIRE(obs && ep_off, "%s: null pointer", who);
  GA_REQUIRE(obs_dim >= 1 && obs_dim <= LB_MAX_OBS,
             "%s: obs_dim %d outside 1 .. %d", who, obs_dim, LB_MAX_OBS);
  GA_REQUIRE(ldo >= obs_dim, "%s: ldo %lld < obs_dim %d", who, (long long)ldo, obs_dim);
  GA_REQUIRE(S >= 1 && S < (1ll << 31), "%s: S %lld outside 1 .. 2^31 - 1", who,
             (long long)S);
  GA_REQUIRE(n_eps >= 1 && n_eps <= S, "%s: n_eps %lld outside 1 .. S", who,
             (long long)n_eps);
  return GA_OK;
}
