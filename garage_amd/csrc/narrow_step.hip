// One optimizer step's forward + loss + backward of a NARROW network in one launch
// (gfx950): two tanh hidden layers of equal width H = 32 or 64, <= 32 inputs,
// <= 8 outputs -- the CartPole-class networks of BASELINE.json configs[0-1]
// (MLP(32,32), MLP(64,64)) at minibatches of any size.
//
// At these widths every weight of the network fits in LDS many times over (18 KB at
// H = 64), so a workgroup takes 64 rows of the minibatch through the WHOLE step --
// gather, both hidden layers, head, loss row by row with its gradient seed
// (loss_rows.h: torch/algos/ppo.py:96-132, vpg.py:434-454,
// gaussian_mlp_value_function.py:81-98), both data gradients, all three weight
// gradients -- with the activations of its rows never leaving the CU, and writes
// only its share of the gradient (a few KB).  reduce_regions_adam_kernel
// (fused_train.hip) then sums the shares in a fixed order, finishes the loss and
// applies Adam: two launches per optimizer step of VPG._train_policy /
// _train_value_function (vpg.py:250-293) instead of five (fused kernels) or ten
// (per-layer kernels), each of which was latency bound at these shapes.
//
// All products with K >= 32 run on v_mfma_f32_32x32x2_f32 from LDS operands (one
// 32x32 tile per wave at H = 64); sums over the 64 rows of a tile are taken in a
// fixed order, so results are bitwise reproducible; they agree with the other
// paths to rounding.
#include "common.h"
#include <hip/hip_ext.h>

#include "prof.h"

#include "fused_train.h"
#include "loss_rows.h"
#include "narrow_body.h"

namespace {

template <int H, int NS_LDX>
__global__ __launch_bounds__(NS_THREADS, NS_LDX <= 20 ? 2 : 1) void narrow_train_kernel(
    NarrowParams p) {
  narrow_train_body<H, NS_LDX>(p, blockIdx.x);
}

}  // namespace

static long long* g_ns_dbg = nullptr;
// developer hook: phase timestamps (100 MHz wall clock) of workgroup 0 of the most
// recent launch -- first call arms it, second call reads 16 values back
extern "C" int ga_narrow_step_debug(long long* host_out16) {
  if (!g_ns_dbg) {
    if (hipMalloc(&g_ns_dbg, 16 * sizeof(long long)) != hipSuccess) return -1;
    (void)hipMemset(g_ns_dbg, 0, 16 * sizeof(long long));
    return 1;
  }
  (void)hipDeviceSynchronize();
  return hipMemcpy(host_out16, g_ns_dbg, 16 * sizeof(long long), hipMemcpyDeviceToHost) ==
                 hipSuccess ? 0 : -1;
}

// (ga_narrow_step_supported, ga_narrow_step_stride: shape_rules.h)

extern "C" int ga_narrow_train_step(const float* params, const int64_t* w_off,
                                    const int64_t* b_off, int in_w, int H, int out_w,
                                    const float* X, int64_t ldx, int64_t M,
                                    const ga_fused_loss_args* loss, float* part,
                                    double* lpart, hipStream_t stream) {
  GA_REQUIRE(params && w_off && b_off && X && loss && part && lpart,
             "ga_narrow_train_step: null pointer");
  const int dims[4] = {in_w, H, H, out_w};
  GA_REQUIRE(ga_narrow_step_supported(3, dims) && M >= 1 && M < (1ll << 31),
             "ga_narrow_train_step: unsupported shape");
  GA_REQUIRE(ga_aligned16(params) && ga_aligned16(X) && ga_aligned16(part) &&
                 ldx % 4 == 0 && ldx >= ((in_w + 3) & ~3) && w_off[0] % 4 == 0 &&
                 w_off[1] % 4 == 0 && w_off[2] % 4 == 0,
             "ga_narrow_train_step: operands must be 16-B aligned quads");
  GA_REQUIRE(loss->kind == 1 ? loss->returns != nullptr
                             : (loss->actions && loss->adv &&
                                (loss->algo == 1 || loss->old_ll) &&
                                (loss->kind == 2 ||
                                 (loss->lda % 4 == 0 && ga_aligned16(loss->actions) &&
                                  loss->lda >= ((loss->A + 3) & ~3)))),
             "ga_narrow_train_step: missing / misaligned minibatch arrays");
  GA_REQUIRE(loss->kind == 2 || loss->log_std, "ga_narrow_train_step: log_std");
  GA_REQUIRE(loss->algo == 0 || loss->algo == 1, "ga_narrow_train_step: algo");
  NarrowParams p;
  memset(&p, 0, sizeof(p));
  p.params = params;
  for (int l = 0; l < 3; ++l) { p.w_off[l] = w_off[l]; p.b_off[l] = b_off[l]; }
  p.in_w = in_w; p.out_w = out_w; p.M = (int)M; p.X = X; p.ldx = ldx;
  p.loss = loss_args(loss, M);
  p.part = part; p.stride = ga_narrow_step_stride(in_w, H); p.lpart = lpart;
  p.dbg = g_ns_dbg;
  const dim3 grid((unsigned)ga_fused_tiles(M));
  // algorithmic flops: forward + both backward products of every layer
  const double flops =
      6.0 * (double)M * ((double)in_w * H + (double)H * H + (double)H * out_w);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_NARROW_STEP, flops, &e0, &e1);
#define GA_NARROW_LAUNCH(HH, LL)                                                      \
  hipExtLaunchKernelGGL((narrow_train_kernel<HH, LL>), grid, dim3(NS_THREADS), 0, stream, \
                        e0, e1, 0, p)
  const int ldx_s = in_w <= 8 ? 12 : (in_w <= 16 ? 20 : 36);
  if (H == 64) {
    if (ldx_s == 12) GA_NARROW_LAUNCH(64, 12);
    else if (ldx_s == 20) GA_NARROW_LAUNCH(64, 20);
    else GA_NARROW_LAUNCH(64, 36);
  } else {
    if (ldx_s == 12) GA_NARROW_LAUNCH(32, 12);
    else if (ldx_s == 20) GA_NARROW_LAUNCH(32, 20);
    else GA_NARROW_LAUNCH(32, 36);
  }
#undef GA_NARROW_LAUNCH
  GA_CHECK_LAUNCH("narrow_train");
  return GA_OK;
}
