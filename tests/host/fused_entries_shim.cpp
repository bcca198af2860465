// The forward + loss and data-gradient entry points of a fused optimizer step
// (fused_train.h) are not part of the C ABI: ga_update_epoch* is what callers see, and it
// lays H1, dZ2 and the weights out at the layers' widths.  The kernels take every leading
// dimension from their caller, though, and multiply it into their addresses.  This file is
// linked with the library's own objects into a second shared object
// (garage_amd/_C/libgarage_amd_fused_entries.so, Makefile) that exports ONE wrapper, so
// that tests/test_fused_entries_strides_gpu.py can run the entries on buffers whose rows
// lie further apart than they are wide.  Nothing here is part of the product.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/fused_train.h"

#define SHIM_API extern "C" __attribute__((visibility("default")))

// One network (two hidden tanh layers of `width` units, first layer in the kernel) on M
// rows: fused != 0: ga_fused_fwd_dgrad; 0: ga_fused_fwd_head_loss, then
// ga_fused_dgrad_wgrad0 on what it wrote.  kind 0 (Gaussian policy, PPO objective, clip
// 0.2): actions / old_ll / adv; kind 1 (value function): returns.  W2 [width][ldw] is the
// forward's weight matrix and the data gradient's.  -> the entry point's return code.
SHIM_API int ga_test_fused_fwd_and_dgrad(
    int fused, int64_t M, int width, int in_w, int A, int kind, const float* X, int64_t ldx,
    const int32_t* idx, const float* W1, const float* b1, float* H1, int64_t ldh,
    const float* W2, int64_t ldw, const float* b2, const float* Wh, int64_t head_ldw,
    const float* bh, const float* log_std, const float* actions, int64_t lda,
    const float* old_ll, const float* adv, const float* returns, float* dZ2, int64_t lddz,
    float* hpart, double* lpart, float* wpart, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ga_fused_loss_args la;
  memset(&la, 0, sizeof(la));
  la.kind = kind; la.actions = actions; la.lda = lda; la.old_ll = old_ll; la.adv = adv;
  la.returns = returns; la.idx = idx; la.log_std = log_std; la.A = A; la.algo = 0;
  la.clip = 0.2f;
  ga_fused_first_layer fl;
  memset(&fl, 0, sizeof(fl));
  fl.X = X; fl.ldx = ldx; fl.W = W1; fl.b = b1; fl.in_w = in_w; fl.H = H1; fl.ldh = ldh;
  ga_fused_fwd_net fw;
  memset(&fw, 0, sizeof(fw));
  fw.W = W2; fw.ldw = ldw; fw.bias = b2; fw.head_W = Wh; fw.head_ldw = head_ldw;
  fw.head_bias = bh; fw.loss = &la; fw.dZ = dZ2; fw.lddz = lddz; fw.hpart = hpart;
  fw.lpart = lpart; fw.first = &fl;
  ga_fused_dgrad_net g;
  memset(&g, 0, sizeof(g));
  g.dZ2 = dZ2; g.lddz = lddz; g.W2 = W2; g.ldw = ldw; g.H1 = H1; g.ldh = ldh; g.X = X;
  g.ldx = ldx; g.idx = idx; g.wpart = wpart;
  if (fused) return ga_fused_fwd_dgrad(&fw, &g, M, width, width, stream);
  const int rc = ga_fused_fwd_head_loss(&fw, 1, M, width, width, stream);
  if (rc) return rc;
  return ga_fused_dgrad_wgrad0(&g, 1, M, width, width, in_w, stream);
}

SHIM_API int ga_test_fused_fwd_dgrad_supported(int width, int in_w) {
  return ga_fused_fwd_dgrad_supported(width, width, in_w);
}
