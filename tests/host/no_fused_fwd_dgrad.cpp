// For the host harnesses that pin the two-launch sequence of a fused optimizer step
// (update_loop_harness.cpp, slab_sum_harness.cpp): a kernel side without the fused
// forward + data-gradient instantiation.  update.cpp asks, is told "no" and never makes
// the launch.
#include <stdio.h>
#include <stdlib.h>

#include "../../garage_amd/csrc/fused_train.h"

extern "C" {
int ga_fused_fwd_dgrad_supported(int, int, int) { return 0; }
int ga_fused_fwd_dgrad(const ga_fused_fwd_net*, const ga_fused_dgrad_net*, int64_t, int, int,
                       hipStream_t) {
  fprintf(stderr, "ga_fused_fwd_dgrad launched although it is not supported\n");
  abort();
}
}
