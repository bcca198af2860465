// Fused kernels of one optimizer step (gfx950): the streaming passes around the
// MFMA GEMMs of VPG._train_policy / _train_value_function (torch/algos/vpg.py
// :250-293) folded into the GEMMs' epilogues, so that the activation of the last
// hidden layer, its data gradient's narrow products and the data gradient of the
// first hidden layer never travel through HBM.
//
//   fwd_head_loss_kernel   last hidden layer  H = tanh(A W^T + b)  on 64-row tiles
//       that span the layer's whole width (64, 128 or 256 units), then -- on the
//       staged rows, before anything leaves the CU -- the head layer (<= 8
//       outputs: torch/modules/multi_headed_mlp_module.py:136-151), the loss row
//       by row with its gradient seed (loss_rows.h: ppo.py:96-132, vpg.py:434-454,
//       gaussian_mlp_value_function.py:81-98), the data gradient of this layer
//       dZ = (dout W_head) (1 - H^2) and this workgroup's share of the head's
//       weight / bias gradient  dW_head = dout^T H.  Written: dZ [M x width] and a
//       few KB of partial sums per workgroup.  H itself is never stored.
//       Replaces: head GEMM, loss kernel, loss finalize, head weight-gradient +
//       data-gradient streaming kernel (4 launches, 2 passes over [M x width]).
//       L1 instantiation (two hidden layers, <= 32 inputs): the layer below is the
//       network's first layer and its output -- this GEMM's A operand -- is
//       produced in the kernel, 32 columns at a time, on v_mfma_f32_16x16x4_f32
//       (and written once for the backward pass); the B fragments then come
//       straight from L2 and the k-loop has one barrier per step.  Replaces the
//       first-layer streaming launch and a read of [M x width].
//
//   dgrad_wgrad0_kernel    data gradient into the FIRST hidden layer
//       dZ1 = (dZ2 W2) (1 - H1^2)  on 64-row tiles spanning H1's whole width, then
//       this workgroup's share of the first layer's weight and bias gradient
//       dW1 = dZ1^T X (a [width x 64] x [64 x 32] MFMA product per tile),
//       db1 = 1^T dZ1  (X: <= 32 observation columns, gathered).
//       dZ1 is never stored.  Replaces the first-layer weight-gradient streaming
//       kernel and one [M x width] store + load.
//       On the side (two hidden layers, more than one split; ga_set_slab_sum_in_dgrad):
//       the launch sums the split-K slabs of the MIDDLE layer's weight gradient, which
//       the GEMM one launch earlier on the same stream wrote, over their partial 0 --
//       one group of four partials per k-step, in the optimizer kernel's own order
//       (FtSlabSummer) -- so that the optimizer launch reads one partial of them.
//
//   fwd_dgrad_kernel       the two kernels above as ONE launch (one network, two
//       hidden layers of the same width, first layer in the kernel; the default for
//       such steps, ga_set_fused_fwd_dgrad): a workgroup runs both bodies on its 64
//       rows and dZ2 stays in LDS between them as the data gradient's A operand.  dZ2
//       is still written once, for the middle layer's weight-gradient GEMM, which then
//       runs AFTER this launch: its slabs are summed by the optimizer launch.
//
//   reduce_regions_adam_kernel   the optimizer step over per-region partial sums
//       (split-K slabs of the weight-gradient GEMMs, per-workgroup partials of
//       the two kernels above), each element summed in a fixed tree by 16 shares
//       of a workgroup (ft_share_run and its neighbours: one definition for this
//       kernel and the slab sum of dgrad_wgrad0_kernel; a region that launch has
//       summed already is read as one partial); one extra block finishes the loss (batch sums -> loss
//       value, log-std gradient) and steps the log-std slot.
//       torch.optim.Adam arithmetic as in losses.hip.
//
// Everything is exact fp32 on v_mfma_f32_32x32x2_f32 with fixed summation orders
// (bitwise reproducible run to run); orders differ from the unfused kernels, so
// the two paths agree to rounding, not bit for bit.
//
// Device code and, at the end, the launch seam only.  The entry points -- argument
// checks, kernel choice, grids, the weight-plane cache -- are host C++,
// fused_train_host.cpp; the parameter structs it fills are fused_params.h's.
#include "common.h"
#include <hip/hip_ext.h>
#include <type_traits>

#include "gemm_core.h"
#include "loss_rows.h"
#include "reduce_trees.h"
#include "fused_train.h"
#include "fused_params.h"

// ---- Audit (round 3) of out-of-range lanes / idle waves (the class of the round-2
// small_step fault).  Clamped loads whose value is masked afterwards: gathered row
// ids idx[min(m, M - 1)] (fused forward prologue, wave 0's sample, data gradient's
// observation quads and H1 quads), first-layer inputs X[..][min(k, in_w - 1)], the
// data gradient's observation quad min(e % 8, ld0 / 4 - 1), everything inside
// gemm_mainloop (TileLoader clamps rows and the last k vector).  Guarded loads: W1 /
// b1 staging (e < K * ld0 / 4, e < K), weight fragments (row wn0 + l31 < BN = the
// layer's width, k < K since K % 32 == 0), head weights and bias (j < A), bias
// columns (< BN).  Stores of rows >= M are predicated; per-tile partials are sized by
// ga_update_partials_floats (tests/host/update_loop_harness.cpp, check 9).
// The accesses that go through a buffer descriptor (GaBuffer, common.h: W2 and W
// fragments, the H1 spill, the fused epilogue's dZ stores) reach the addresses they
// reached as global accesses and keep the guards above; the descriptor's extent is exact.
namespace {

// (FT_ROWS = 64 rows per workgroup tile, FT_W1_FLOATS: shape_rules.h; the parameter
// structs: fused_params.h)

// FT_STAMP: timestamp i of workgroup 8; FT_MARK: slot (0 start, 1 end of the k-loop,
// 2 end) of EVERY workgroup, behind the 16 values of workgroup 8: the skew of a launch
#define FT_STAMP(i) \
  if (p.dbg && ft_tile == 8 && threadIdx.x == 0) p.dbg[i] = wall_clock64()
#define FT_MARK(slot) \
  if (p.dbg && threadIdx.x == 0) p.dbg[16 + 3 * ft_tile + (slot)] = wall_clock64()

typedef const __attribute__((address_space(4))) float* ft_uniform_ptr;
typedef float ft_f32x4 __attribute__((ext_vector_type(4)));

#ifdef GA_SPLIT_NO_SETPRIO
#define FT_SPLIT_PRIO(x)
#else
#define FT_SPLIT_PRIO(x) __builtin_amdgcn_s_setprio(x)
#endif

// MFMAs of one 32-deep k-step on k-contiguous LDS tiles (gemm_core.h: the
// A_KC = B_KC = true case of gemm_mainloop's body)
template <int TM, int TN>
__device__ __forceinline__ void ft_kstep(const float* As, const float* Bs,
                                         f32x16 (&acc)[TM][TN], int wm0, int wn0,
                                         int lane) {
  constexpr int LDK = BK + PAD;
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int g = 0; g < BK / 8; ++g) {
    float a[TM][4], b[TN][4];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(As + (wm0 + 32 * i + l31) * LDK +
                                                        8 * g + 4 * half);
      a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(Bs + (wn0 + 32 * j + l31) * LDK +
                                                        8 * g + 4 * half);
      b[j][0] = v.x; b[j][1] = v.y; b[j][2] = v.z; b[j][3] = v.w;
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] =
              __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  }
}

// The B fragments of dgrad_kloop_staged (W2 [K = BN][ldb], n-contiguous): lane (l31, half)
// feeds B(k, n = wn0 + 32 j + l31), k = 32 s + 8 g + 4 half + q -- four dword loads per
// group, straight from L2 (every workgroup reads all of W2).  A struct of its own because
// fwd_dgrad_kernel issues the first step's loads from inside the forward body's epilogue.
template <int BN, int TN>
struct FtW2Frags {
  float bn[TN][BK / 8][4];
  // wave-uniform base + one 32-bit lane offset (rows k < K = BN, columns < BN <= ldb)
  uint32_t ldb, woff;
#ifdef GA_FT_NO_BUFFER_ADDR
  const float* B;
#else
  // W2 as a buffer (GaBuffer, common.h) of BN rows, the last one BN floats long: the lane's
  // byte offset is one register for the whole loop, a load's row (32 s + 8 g + q) * ldb is
  // scalar arithmetic and the column block an immediate -- no vector instruction per load
  GaBuffer w2;
#endif
  __device__ __forceinline__ FtW2Frags(const DgradWgrad0Params& p, const int wn0)
      : ldb((uint32_t)p.g.ldb),
#ifdef GA_FT_NO_BUFFER_ADDR
        B(p.g.B)
#else
        w2(p.g.B, 4u * ((uint32_t)(BN - 1) * (uint32_t)p.g.ldb + (uint32_t)BN))
#endif
  {
    const int lane = threadIdx.x & 63;
    woff = (uint32_t)(4 * (lane >> 5)) * ldb + (uint32_t)(wn0 + (lane & 31));
  }
  __device__ __forceinline__ void fetch_group(int s, int g) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#ifdef GA_FT_NO_BUFFER_ADDR
        bn[j][g][q] = B[woff + (uint32_t)(32 * s + 8 * g + q) * ldb + (uint32_t)(32 * j)];
#else
        bn[j][g][q] = w2.load(4u * woff + (uint32_t)(128 * j),
                              4u * (uint32_t)(32 * s + 8 * g + q) * ldb);
#endif
  }
  __device__ __forceinline__ void fetch_step0() {
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) fetch_group(0, g);
  }
};

template <int NT>
__device__ __forceinline__ void dgrad_load_x(const DgradWgrad0Params& p, const int ft_tile,
                                             float4 (&xq)[2]);

// The loads of the data-gradient body that fwd_dgrad_kernel has in flight when that body
// begins: the observation quads (behind a load of their gathered row numbers, which they
// wait for) and the first k-step's W2 fragments.
template <int BN, int TN, int NT>
struct FtDgradLoads {
  const DgradWgrad0Params& p;
  const int ft_tile;
  FtW2Frags<BN, TN> w;
  float4 xq[2];
  __device__ __forceinline__ FtDgradLoads(const DgradWgrad0Params& p_, const int tile,
                                          const int wn0)
      : p(p_), ft_tile(tile), w(p_, wn0) {}
  __device__ __forceinline__ void issue() {
    dgrad_load_x<NT>(p, ft_tile, xq);
    w.fetch_step0();
  }
};

// What fwd_head_loss_body<FUSE> leaves behind for the data-gradient body
struct FtFusedLds {
  float* stage;  // [64][BN + 4]: dZ of the tile's rows, rows >= M exact zeros
  float* aux;    // 2048 floats, free once E5 is done
};

// (two 512-thread workgroups per CU need <= 128 registers: the second bound is waves
// per SIMD)
// EVAL (with L1): the whole MLP for its outputs only -- no H1 spill, and after the
// head outputs (E3) the rows go to p.eval_out and the workgroup is done
// (mlp_eval_forward_kernel: the full-batch passes around an update, baselines /
// old log-likelihoods / LossBefore / LossAfter / KL, need no activation in memory).
// KSC > 0 (with L1): round4(inputs) / 4 is the compile-time constant KSC and the
// k-loop is the software-pipelined one (see "pipelined k-loop" below); 0: any width,
// the plain loop.
// ft_tile / ft_tiles: this workgroup's 64-row tile and the number of tiles of ITS
// network's minibatch (a pair launch carries the tiles of two networks in one grid)
// FUSE (with L1, training): the data-gradient body runs behind this one in the same
// workgroup (fwd_dgrad_kernel).  The stage then ends up holding every dZ quad over the H
// quad it was computed from: the stage is the data gradient's A operand.  E5 comes first
// and keeps its quads in registers (the accumulators are dead), so that the tile's 64 KB
// of dZ stores drain under E6, which still reads the staged H; behind a barrier the kept
// quads go over the stage.  The data gradient's first loads (`dgl`: observation rows,
// the first k-step's W2 fragments) are requested IN FRONT of the dZ stores: the memory
// counter retires in order, and behind them the gathered rows' wait and the k-loop's first
// MFMAs would wait for the stores as well.  (GA_FT_NO_EARLY_DZ: E6, a barrier, then E5
// writing global memory and the stage; those loads behind that.)
// `keep` receives the workgroup's LDS.
template <int BN, int WAVES_M, int WAVES_N, bool L1, bool EVAL, int KSC = 0,
          bool SPLIT = false, bool FUSE = false>
__device__ __forceinline__ void fwd_head_loss_body(const FwdLossParams& p,
                                                   const int ft_tile,
                                                   const int ft_tiles,
                                                   FtFusedLds* keep = nullptr,
                                                   FtDgradLoads<BN, BN / WAVES_N / 32,
                                                                64 * WAVES_M * WAVES_N>* dgl =
                                                       nullptr) {
  static_assert(L1 || !EVAL, "the evaluation forward computes the first layer itself");
  static_assert(!FUSE || (L1 && !EVAL && !SPLIT),
                "the fused data gradient: exact fp32 training step, first layer in the kernel");
  static_assert(L1 || KSC == 0, "KSC belongs to the first-layer producer");
  static_assert(!SPLIT || (L1 && KSC == 0 && WAVES_M * WAVES_N == 8),
                "the split-operand loop: first layer in the kernel, 8 waves");
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int WM = FT_ROWS / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int LDK = BK + PAD;
  constexpr int A_FLOATS = FT_ROWS * LDK, B_FLOATS = BN * LDK;
  constexpr int LDC = BN + 4;
  constexpr int STAGE_FLOATS = FT_ROWS * LDC;
  constexpr int TILE_FLOATS =
      A_FLOATS + B_FLOATS > STAGE_FLOATS ? A_FLOATS + B_FLOATS : STAGE_FLOATS;
  constexpr int SEGS = NT / 64, CPS = BN / SEGS, HN = 8;
  constexpr int PL = SEGS < 4 ? SEGS : 4;
  constexpr int AUX_FLOATS = PL * 64 * HN > HN * BN ? PL * 64 * HN : HN * BN;
  static_assert(SEGS <= 2 * PL, "two reduction steps");
  static_assert((FT_ROWS * (BN / 4)) % NT == 0, "whole quads per thread");
  // L1: the first layer's weights sit behind the operand tiles for the k-loop -- in
  // the part of the epilogue stage the tiles leave free (all 20 KB of it at
  // BN = 256), plus EXTRA floats where that is not enough
  constexpr int SLACK = TILE_FLOATS - 2 * A_FLOATS;
  constexpr int EXTRA = (L1 && FT_W1_FLOATS > SLACK) ? FT_W1_FLOATS - SLACK : 0;
  __shared__ __attribute__((aligned(16))) float lds[TILE_FLOATS + EXTRA + AUX_FLOATS];
  __shared__ __attribute__((aligned(16))) float outl[FT_ROWS * HN];
  __shared__ __attribute__((aligned(16))) float doutl[FT_ROWS * HN];
  float* stage = lds;
  float* aux = lds + TILE_FLOATS + EXTRA;  // head partial planes, later W_head [8][BN]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WAVES_N) * WM;
  const int wn0 = (wave % WAVES_N) * WN;
  const int m0 = ft_tile * FT_ROWS;
  const int M = p.g.M;
  const LossRowArgs& L = p.loss;

  FT_STAMP(0);
  FT_MARK(0);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if constexpr (L1) {
    // ---- k-loop with the A operand produced in place:
    //   As(chunk c) = tanh(X_tile W1[32 c .. 32 c + 31]^T + b1) as 8 sub-tiles of
    //   16 x 16 on v_mfma_f32_16x16x4_f32 (lane l: A[l % 16][k = l / 16],
    //   B[k = l / 16][l % 16], D[row 4 (l / 16) + reg][col l % 16]); the wave's
    //   observation values stay in registers for the whole kernel, W1 / b1 in LDS.
    constexpr int NSUB = 8 / (NT / 64);  // sub-tiles per wave: 1 (8 waves) or 2
    const int K = p.g.K, in_w = p.l1_in;
    const int ld0 = (in_w + 3) & ~3, KS = ld0 / 4;
    // two buffers for the produced A chunks; the B fragments never pass through LDS
    auto As2 = [&](int i) { return lds + (i & 1) * A_FLOATS; };
    // (SPLIT: two buffers of three bf16 planes instead)
    constexpr int OPER_FLOATS = SPLIT ? 2 * FT_ABUF_B / 4 : 2 * A_FLOATS;
    float* w1s = lds + OPER_FLOATS;
    float* b1s = aux;
    static_assert(OPER_FLOATS + FT_W1_FLOATS <= TILE_FLOATS + EXTRA, "W1 fits");
    const int r16 = lane & 15, g4 = lane >> 4;
    const int half = lane >> 5, l31 = lane & 31;
    const int rt = wave & 3;  // row sub-tile (the same for both sub-tiles of a wave)
    // prologue: the gathered row number first (the observation loads depend on it),
    // W1 / b1 / the first B fragments in flight behind it
    const int xm = m0 + 16 * rt + r16;
    const int xmc = min(xm, M - 1);
    const int64_t xsrc = L.idx ? (int64_t)L.idx[xmc] : (int64_t)xmc;
    // B fragments of a 32-deep step: lane (l31, half) feeds B(k, n = wn0 + 32 j + l31),
    // k = 32 s + 8 g + 4 half + q -- one 16-B load per group, straight from memory
    // (every workgroup reads all of W: it stays in L2), one step ahead
    const float* Wb = p.g.B + (int64_t)(wn0 + l31) * p.g.ldb + 4 * half;
    float4 bn[TN][4];
    auto fetch_b = [&](int s) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          bn[j][g] = *reinterpret_cast<const float4*>(Wb + (int64_t)(32 * j) * p.g.ldb +
                                                      32 * s + 8 * g);
    };
    if constexpr (!SPLIT) fetch_b(0);
    float xa[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = 4 * s + g4;
      xa[s] = p.l1_X[xsrc * p.l1_ldx + min(k, in_w - 1)];
      xa[s] = (k < in_w && xm < M) ? xa[s] : 0.f;
    }
    for (int e = tid; e < K * KS; e += NT)
      reinterpret_cast<float4*>(w1s)[e] = reinterpret_cast<const float4*>(p.l1_W)[e];
    for (int e = tid; e < K; e += NT) b1s[e] = p.l1_b[e];
    // the 16 x 16 sub-tiles of chunk c (two accumulation chains per sub-tile), bias +
    // tanh, into the operand buffer of the chunk
    auto produce = [&](int c) {
      float* As = As2(c);
#pragma unroll
      for (int u = 0; u < NSUB; ++u) {
        const int ct = (wave + (NT / 64) * u) >> 2;
        const float* wrow = w1s + (32 * c + 16 * ct + r16) * ld0 + g4;
        ft_f32x4 e4 = {0.f, 0.f, 0.f, 0.f}, o4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; s += 2) {
          if (s < KS)
            e4 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wrow[4 * s], e4, 0, 0, 0);
          if (s + 1 < KS)
            o4 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s + 1], wrow[4 * s + 4], o4, 0,
                                                      0, 0);
        }
        const float b = b1s[32 * c + 16 * ct + r16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          As[(16 * rt + 4 * g4 + r) * LDK + 16 * ct + r16] = tanh_fast(e4[r] + o4[r] + b);
      }
    };
    // H1 goes to memory from the finished operand buffer: 16-B pieces, 128 B per row
    auto spill = [&](int c) {
      const float* As = As2(c);
#pragma unroll
      for (int q = 0; q < FT_ROWS * (BK / 4) / NT; ++q) {
        const int e = tid + NT * q;
        const int row = e / (BK / 4), c4 = e % (BK / 4);
        const float4 v = *reinterpret_cast<const float4*>(As + row * LDK + 4 * c4);
        if (m0 + row < M)
          *reinterpret_cast<float4*>(p.l1_H + (int64_t)(m0 + row) * p.l1_ldh + 32 * c +
                                     4 * c4) = v;
      }
    };
    const int nk = K / BK;
    __syncthreads();  // W1 / b1 staged
    if constexpr (SPLIT) {
      // ---- split-operand k-loop (see ft_split3).  The first-layer producer runs its
      // 16x16x4 products TRANSPOSED (A = W1 rows, B = observation rows: the same
      // products in the same order), so that a lane holds four consecutive units k of
      // one batch row: split, packed along k and written as 8 bytes per plane; H1 goes
      // to memory from the same registers.  The W planes come straight from L2 as
      // fragments (lane (n, half): 8 consecutive k), one step ahead, refilled in place.
      static_assert(NSUB == 1, "one 16 x 16 sub-tile per wave and chunk");
      char* apl = reinterpret_cast<char*>(lds);
      const int ct = wave >> 2;
      const bool full = m0 + FT_ROWS <= M;
      float* h1_row = p.l1_H + (int64_t)(m0 + 16 * rt + r16) * p.l1_ldh + 16 * ct + 4 * g4;
      const bool h1_ok = full || m0 + 16 * rt + r16 < M;
      auto produce_split = [&](int c) {
        const float* wrow = w1s + (32 * c + 16 * ct + r16) * ld0 + g4;
        ft_f32x4 e4 = {0.f, 0.f, 0.f, 0.f}, o4 = {0.f, 0.f, 0.f, 0.f};
        // (at most 20 inputs on this path: five groups of four, as in the loop below)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const float w = wrow[4 * min(k, KS - 1)], x = k < KS ? xa[k] : 0.f;
          if (k & 1)
            o4 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x, o4, 0, 0, 0);
          else
            e4 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, x, e4, 0, 0, 0);
        }
        const float4 bq = *reinterpret_cast<const float4*>(b1s + 32 * c + 16 * ct + 4 * g4);
        const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
        float hv[4];
        uint32_t hi[2], mid[2], lo[2];
#pragma unroll
        for (int r = 0; r < 4; ++r) hv[r] = tanh_fast(e4[r] + o4[r] + bb[r]);
        ft_split3_pair(hv[0], hv[1], hi[0], mid[0], lo[0]);
        ft_split3_pair(hv[2], hv[3], hi[1], mid[1], lo[1]);
        char* dst = apl + (c & 1) * FT_ABUF_B + (16 * rt + r16) * FT_PLANE_ROW_B +
                    (16 * ct + 4 * g4) * 2;
        *reinterpret_cast<uint2*>(dst) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(dst + FT_PLANE_B) = make_uint2(mid[0], mid[1]);
        *reinterpret_cast<uint2*>(dst + 2 * FT_PLANE_B) = make_uint2(lo[0], lo[1]);
        if constexpr (!EVAL) {
          if (h1_ok)
            *reinterpret_cast<float4*>(h1_row + 32 * c) =
                make_float4(hv[0], hv[1], hv[2], hv[3]);
        }
      };
      // W fragments of step s, group g (16 k), plane pl (split_planes_kernel's order)
      const uint16_t* wpl = p.bplanes + ((wn0 / 32) * 64 + lane) * 8;
      ft_u32x4 bw[TN][2][3];
      auto fetch_planes = [&](int s, int g) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            bw[j][g][pl] = *reinterpret_cast<const ft_u32x4*>(
                wpl + pl * p.bplane_stride + ((2 * s + g) * (BN / 32) + j) * 512);
      };
      fetch_planes(0, 0);
      fetch_planes(0, 1);
      produce_split(0);
      __syncthreads();
      FT_STAMP(1);
      // One step = 24 MFMAs (2 groups of 16 k x 2 row blocks x 6 products), the row
      // blocks alternating so that consecutive MFMAs never wait for each other's
      // accumulator; the producer of the NEXT chunk is cut into pieces issued between
      // them (the order is pinned: the pieces are chains of dependent instructions,
      // each placed where its inputs have had an MFMA or more of time to arrive).
#define FT_SB __builtin_amdgcn_sched_barrier(0)
      // The producer is itself pipelined across steps: step s runs bias + tanh + split
      // + LDS write of chunk s + 1 on first-layer products that step s - 1 issued (e4 /
      // o4 live across the barrier), and issues the products of chunk s + 2 at its end:
      // nothing in a step waits for something the same step started, except the A
      // fragments of the step itself.
      ft_f32x4 e4 = {0.f, 0.f, 0.f, 0.f}, o4 = {0.f, 0.f, 0.f, 0.f};
      auto first_layer = [&](int c, const float (&wv)[5]) {
        e4 = ft_f32x4{0.f, 0.f, 0.f, 0.f};
        o4 = ft_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const float x = k < KS ? xa[k] : 0.f;
          if (k & 1)
            o4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[k], x, o4, 0, 0, 0);
          else
            e4 = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[k], x, e4, 0, 0, 0);
        }
      };
      auto first_layer_weights = [&](int c, float (&wv)[5]) {
        // (KS <= 5 on this path: the host checks it; slots beyond KS read a valid
        // address and multiply a zero)
        const float* wrow = w1s + (32 * c + 16 * ct + r16) * ld0 + g4;
#pragma unroll
        for (int k = 0; k < 5; ++k) wv[k] = wrow[4 * min(k, KS - 1)];
      };
      if (nk > 1) {
        float wv[5];
        first_layer_weights(1, wv);
        first_layer(1, wv);
      }
      auto step = [&](int s, auto more_tag, auto more2_tag) {
        constexpr bool MORE = decltype(more_tag)::value;    // chunk s + 1 exists
        constexpr bool MORE2 = decltype(more2_tag)::value;  // chunk s + 2 exists
        const char* Ab = apl + (s & 1) * FT_ABUF_B;
        const char* arow = Ab + (wm0 + l31) * FT_PLANE_ROW_B + 16 * half;
        ft_u32x4 af[2][TM][3];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            af[0][i][pl] = *reinterpret_cast<const ft_u32x4*>(
                arow + pl * FT_PLANE_B + 32 * i * FT_PLANE_ROW_B);
        float wv[5];
        float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MORE)
          bq = *reinterpret_cast<const float4*>(b1s + 32 * (s + 1) + 16 * ct + 4 * g4);
        FT_SB;
        // ga_tanh (common.h) in four stages over the four values: the same operations
        // in the same order per value, a stage's four chains independent of each other
        float tc[4], ex[4], dn[4], rc[4], hv[4];
        uint32_t hi[2], mid[2], lo[2];
        auto side = [&](int t) {
          if constexpr (MORE) {
            if (t == 1) {
              const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float t2 = 2.f * (e4[r] + o4[r] + bb[r]);
                tc[r] = t2 > 80.f ? 80.f : t2;
              }
            } else if (t == 3) {
#pragma unroll
              for (int r = 0; r < 4; ++r) ex[r] = __expf(tc[r]);
            } else if (t == 5) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                dn[r] = ex[r] + 1.f;
                rc[r] = __builtin_amdgcn_rcpf(dn[r]);
              }
            } else if (t == 7) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float rr = fmaf(fmaf(-dn[r], rc[r], 1.f), rc[r], rc[r]);
                hv[r] = fmaf(-2.f, rr, 1.f);
              }
            } else if (t == 9) {
              ft_split3_pair(hv[0], hv[1], hi[0], mid[0], lo[0]);
            } else if (t == 10) {
              ft_split3_pair(hv[2], hv[3], hi[1], mid[1], lo[1]);
            } else if (t == 12) {
              char* dst = apl + ((s + 1) & 1) * FT_ABUF_B + (16 * rt + r16) * FT_PLANE_ROW_B +
                          (16 * ct + 4 * g4) * 2;
              *reinterpret_cast<uint2*>(dst) = make_uint2(hi[0], hi[1]);
              *reinterpret_cast<uint2*>(dst + FT_PLANE_B) = make_uint2(mid[0], mid[1]);
              *reinterpret_cast<uint2*>(dst + 2 * FT_PLANE_B) = make_uint2(lo[0], lo[1]);
            } else if (t == 13) {
              if constexpr (!EVAL) {
                if (h1_ok)
                  *reinterpret_cast<float4*>(h1_row + 32 * (s + 1)) =
                      make_float4(hv[0], hv[1], hv[2], hv[3]);
              }
            }
          }
          if constexpr (MORE2) {
            if (t == 11) first_layer_weights(s + 2, wv);
            if (t == 15) first_layer(s + 2, wv);
          }
        };
        FT_SPLIT_PRIO(1);
#pragma unroll
        for (int slot = 0; slot < 24; ++slot) {
          const int g = slot / 12, t = (slot % 12) / 2, i = slot % 2;
          // products small to large, the A planes released early:
          // (lo,hi) (mid,mid) (mid,hi) (hi,lo) (hi,mid) (hi,hi)
          const int pa = t == 0 ? 2 : (t == 1 || t == 2) ? 1 : 0;
          const int pb = t == 3 ? 2 : (t == 1 || t == 4) ? 1 : 0;
#ifdef GA_ABL_NOMFMA
          acc[i][0][slot & 15] += __uint_as_float(af[g][i][pa][0] ^ bw[0][g][pb][0]);
#else
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              __builtin_bit_cast(ft_bf16x8, af[g][i][pa]),
              __builtin_bit_cast(ft_bf16x8, bw[0][g][pb]), acc[i][0], 0, 0, 0);
#endif
          FT_SB;
          // the second group's A planes, each as late as its first use allows (the
          // first group's planes die in the order lo, mid, hi)
          if (slot == 6 || slot == 8 || slot == 11) {
            const int pl = slot == 6 ? 2 : slot == 8 ? 1 : 0;
#pragma unroll
            for (int ii = 0; ii < TM; ++ii)
              af[1][ii][pl] = *reinterpret_cast<const ft_u32x4*>(
                  arow + pl * FT_PLANE_B + 32 * ii * FT_PLANE_ROW_B + 32);
          }
#ifndef GA_ABL_NOFETCH
          if constexpr (MORE) {
            if (slot == 11) fetch_planes(s + 1, 0);
            if (slot == 23) fetch_planes(s + 1, 1);
          }
#endif
#ifndef GA_ABL_NOPRODUCE
          side(slot);
#endif
          FT_SB;
        }
        FT_SPLIT_PRIO(0);
#ifndef GA_ABL_NOBARRIER
        __syncthreads();
#endif
      };
#undef FT_SB
      static_assert(TN == 1 && TM == 2, "the slot list is written for a 64 x 32 wave tile");
      for (int s = 0; s + 2 < nk; ++s) step(s, std::true_type{}, std::true_type{});
      if (nk > 1) step(nk - 2, std::true_type{}, std::false_type{});
      step(nk - 1, std::false_type{}, std::false_type{});
    } else {
    produce(0);
    __syncthreads();
    FT_STAMP(1);
    if constexpr (KSC > 0) {
      // ---- pipelined k-loop.  The plain loop below runs a step as [produce chunk
      // s + 1: LDS reads -> 16x16x4 MFMAs -> tanh -> LDS writes] THEN [the step's 32
      // MFMAs]: while a wave produces it feeds the matrix pipe nothing, and right
      // after a barrier all waves of the workgroup produce at once -- a workgroup
      // alone on its CU keeps the pipe busy about half the time.  Here every piece
      // of the producer (and the H1 spill, and the next step's B fragments) is issued
      // BETWEEN the step's MFMAs: LDS / memory latencies and the producer's dependent
      // chains then no longer stall the wave's MFMA issue.  (Vector instructions do NOT
      // execute in an fp32 MFMA's shadow on this chip -- tools/mfma_valu_overlap.hip: the
      // fp32 MFMA runs on the vector ALU's lanes; the interleave saves stalls, not issue
      // time.)  The order below is pinned with sched_barrier(0);
      // the number of first-layer k groups is the compile-time KSC so that the
      // producer has no branches.  Same arithmetic in the same order per output
      // element as the plain loop: bit-identical results.
      constexpr int SLOTS = (BK / 8) * 4 * TN;  // one slot = TM MFMAs
      constexpr int SPQ = FT_ROWS * (BK / 4) / NT;
      constexpr int LD0 = 4 * KSC;
      // wave-uniform 64-bit bases + 32-bit lane offsets (one address register each)
      const uint32_t wb_off = (uint32_t)(wn0 + l31) * (uint32_t)p.g.ldb + 4u * half;
      float* h1_tile = p.l1_H + (int64_t)m0 * p.l1_ldh;
#ifndef GA_FT_NO_BUFFER_ADDR
      // the same as buffers (GaBuffer, common.h): W [BN][ldb] with K floats in its last
      // row, and this tile's rows of H1 (K floats in the last one that exists).  A lane's
      // byte offsets are computed here, once; the k-step enters as a scalar offset
      const GaBuffer wbuf(p.g.B, 4u * ((uint32_t)(BN - 1) * (uint32_t)p.g.ldb + (uint32_t)K));
      const GaBuffer h1buf(h1_tile, 4u * ((uint32_t)(min(FT_ROWS, M - m0) - 1) *
                                              (uint32_t)p.l1_ldh + (uint32_t)K));
      const uint32_t wb_off_b = 4u * wb_off;
      uint32_t sp_off_b[SPQ];
#pragma unroll
      for (int q = 0; q < SPQ; ++q) {
        const int e = tid + NT * q;
        sp_off_b[q] = 4u * ((uint32_t)(e / (BK / 4)) * (uint32_t)p.l1_ldh +
                            (uint32_t)(4 * (e % (BK / 4))));
      }
#endif
#define FT_SB __builtin_amdgcn_sched_barrier(0)
      auto step = [&](int s, auto more_tag, auto full_tag) {
        constexpr bool MORE = decltype(more_tag)::value;
        constexpr bool FULL = decltype(full_tag)::value;
        const float* As = As2(s);
        float* An = As2(s + 1);
        // (the B fragments of group g live in bn[.][g]; as soon as the group's MFMAs
        // are issued the same registers receive the next step's group g -- a whole
        // step of latency budget, no second register set, no copies)
        // -- the step's loads: A fragments of group 0 first (the MFMAs wait for
        //    them), then the producer's weights and the spill's quads
        float4 af[2][TM];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          af[0][i] = *reinterpret_cast<const float4*>(As + (wm0 + 32 * i + l31) * LDK +
                                                      4 * half);
        float wv[NSUB][KSC], bv[NSUB];
        if constexpr (MORE) {
#pragma unroll
          for (int u = 0; u < NSUB; ++u) {
            const int ct = (wave + (NT / 64) * u) >> 2;
            const float* wrow = w1s + (32 * (s + 1) + 16 * ct + r16) * LD0 + g4;
#pragma unroll
            for (int k = 0; k < KSC; ++k) wv[u][k] = wrow[4 * k];
            bv[u] = b1s[32 * (s + 1) + 16 * ct + r16];
          }
        }
        float4 sp[SPQ];
        if constexpr (!EVAL) {
#pragma unroll
          for (int q = 0; q < SPQ; ++q) {
            const int e = tid + NT * q;
            sp[q] = *reinterpret_cast<const float4*>(As + (e / (BK / 4)) * LDK +
                                                     4 * (e % (BK / 4)));
          }
        }
        FT_SB;
        ft_f32x4 e4[NSUB], o4[NSUB];
        float hv[NSUB][4];
        // what goes between the MFMAs: task t of the list
        //   0 .. NSUB-1          16x16x4 MFMAs of sub-tile t (two chains)
        //   NSUB                 H1 spill stores
        //   NSUB+1 .. +4 NSUB    one tanh each
        //   then NSUB            LDS writes of a finished sub-tile
        auto side = [&](int t) {
          if (t < NSUB) {
            if constexpr (MORE) {
              const int u = t;
              e4[u] = ft_f32x4{0.f, 0.f, 0.f, 0.f};
              o4[u] = ft_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int k = 0; k < KSC; k += 2) {
                e4[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k], wv[u][k], e4[u], 0, 0, 0);
                if (k + 1 < KSC)
                  o4[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[k + 1], wv[u][k + 1],
                                                               o4[u], 0, 0, 0);
              }
            }
          } else if (t == NSUB) {
            if constexpr (!EVAL) {
#pragma unroll
              for (int q = 0; q < SPQ; ++q) {
                const int e = tid + NT * q;
                const int row = e / (BK / 4), c4 = e % (BK / 4);
#ifdef GA_FT_NO_BUFFER_ADDR
                if (FULL || m0 + row < M)
                  *reinterpret_cast<float4*>(
                      h1_tile + ((uint32_t)row * (uint32_t)p.l1_ldh +
                                 (uint32_t)(32 * s + 4 * c4))) = sp[q];
#else
                (void)c4;
                if (FULL || m0 + row < M) h1buf.store4(sp[q], sp_off_b[q], 128u * (uint32_t)s);
#endif
              }
            }
          } else if (t < NSUB + 1 + 4 * NSUB) {
            if constexpr (MORE) {
              const int u = (t - NSUB - 1) / 4, r = (t - NSUB - 1) % 4;
              hv[u][r] = tanh_fast(e4[u][r] + o4[u][r] + bv[u]);
            }
          } else if (t < 2 * NSUB + 1 + 4 * NSUB) {
            if constexpr (MORE) {
              const int u = t - (NSUB + 1 + 4 * NSUB);
              const int ct = (wave + (NT / 64) * u) >> 2;
#pragma unroll
              for (int r = 0; r < 4; ++r)
                An[(16 * rt + 4 * g4 + r) * LDK + 16 * ct + r16] = hv[u][r];
            }
          }
        };
        constexpr int TASKS = 2 * NSUB + 1 + 4 * NSUB;
        static_assert(TASKS + 2 <= SLOTS, "a slot for every side task");
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int slot = 0; slot < SLOTS; ++slot) {
          const int g = slot / (4 * TN), q = (slot / TN) % 4, j = slot % TN;
          {
            const float4 bq = bn[j][g];
            const float bb = q == 0 ? bq.x : q == 1 ? bq.y : q == 2 ? bq.z : bq.w;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
              const float4 aq = af[g & 1][i];
              const float aa = q == 0 ? aq.x : q == 1 ? aq.y : q == 2 ? aq.z : aq.w;
#ifdef GA_ABL_NOMFMA
              acc[i][j][slot & 15] += aa * bb;
#else
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa, bb, acc[i][j], 0, 0, 0);
#endif
            }
          }
          FT_SB;
          // the next group's A fragments: issued at the start of this group
          if (slot % (4 * TN) == 0 && g + 1 < BK / 8) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
              af[(g + 1) & 1][i] = *reinterpret_cast<const float4*>(
                  As + (wm0 + 32 * i + l31) * LDK + 8 * (g + 1) + 4 * half);
          }
#ifndef GA_ABL_NOFETCH
          // this group's B registers are free: the next step's group g goes there
          if constexpr (MORE) {
            if (slot % (4 * TN) == 4 * TN - 1) {
#pragma unroll
              for (int jj = 0; jj < TN; ++jj)
#ifdef GA_FT_NO_BUFFER_ADDR
                bn[jj][g] = *reinterpret_cast<const float4*>(
                    p.g.B + (wb_off + (uint32_t)(32 * jj) * (uint32_t)p.g.ldb +
                             (uint32_t)(32 * (s + 1) + 8 * g)));
#else
                bn[jj][g] = wbuf.load4(wb_off_b + (uint32_t)(32 * g),
                                       4u * ((uint32_t)(32 * jj) * (uint32_t)p.g.ldb +
                                             (uint32_t)(32 * (s + 1))));
#endif
            }
          }
#endif
          // side tasks from slot 1 on, one per slot
#ifdef GA_ABL_NOPRODUCE
          if (slot - 1 == NSUB) side(slot - 1);
#elif defined(GA_ABL_NOSPILL)
          if (slot >= 1 && slot - 1 < TASKS && slot - 1 != NSUB) side(slot - 1);
#else
          if (slot >= 1 && slot - 1 < TASKS) side(slot - 1);
#endif
          FT_SB;
        }
        __builtin_amdgcn_s_setprio(0);
#ifndef GA_ABL_NOBARRIER
        __syncthreads();
#endif
      };
#undef FT_SB
      const bool full = m0 + FT_ROWS <= M;
      if (full) {
        for (int s = 0; s + 1 < nk; ++s) step(s, std::true_type{}, std::true_type{});
        step(nk - 1, std::false_type{}, std::true_type{});
      } else {
        for (int s = 0; s + 1 < nk; ++s) step(s, std::true_type{}, std::false_type{});
        step(nk - 1, std::false_type{}, std::false_type{});
      }
    } else {
#ifdef GA_FT_LOOP_STAMPS
    // developer build: shader-clock ticks thread 0 of every workgroup spends in the
    // parts of a k-step, summed over the loop (tools/fused_fwd_phases.py)
    long long c_mma = 0, c_bar1 = 0, c_store = 0, c_bar2 = 0;
#define FT_TICK(acc_, t_) { const long long n_ = clock64(); acc_ += n_ - t_; t_ = n_; }
#else
#define FT_TICK(acc_, t_)
#endif
    // step s: MFMAs on chunk buffer s % 2 with the B fragments fetched during step
    // s - 1; chunk s + 1 is produced into the other buffer (last read in step s - 1);
    // ONE barrier per step
    for (int s = 0; s < nk; ++s) {
      const bool more = s + 1 < nk;
#ifdef GA_FT_LOOP_STAMPS
      long long tk = clock64();
#endif
      float4 bc[TN][4];
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) bc[j][g] = bn[j][g];
      if (more) fetch_b(s + 1);
      if constexpr (!EVAL) spill(s);
      if (more) produce(s + 1);
      FT_TICK(c_store, tk);
      const float* As = As2(s);
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) {
        float a[TM][4];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const float4 v = *reinterpret_cast<const float4*>(As + (wm0 + 32 * i + l31) * LDK +
                                                            8 * g + 4 * half);
          a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
        }
        float b[TN][4];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          b[j][0] = bc[j][g].x; b[j][1] = bc[j][g].y; b[j][2] = bc[j][g].z; b[j][3] = bc[j][g].w;
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], b[j][q], acc[i][j],
                                                               0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
      FT_TICK(c_mma, tk);
      __syncthreads();
      FT_TICK(c_bar1, tk);
    }
#ifdef GA_FT_LOOP_STAMPS
    if (p.dbg && tid == 0) {
      long long* o = p.dbg + 16 + 3 * 4096 + 4 * ft_tile;
      o[0] = c_mma; o[1] = c_bar1; o[2] = c_store; o[3] = c_bar2;
    }
#endif
    }  // plain loop
    }  // exact fp32 loops
  } else {
    float csum = 0.f;
    const bool full = m0 + FT_ROWS <= M;
    if (full)
      gemm_mainloop<FT_ROWS, BN, WAVES_M, WAVES_N, true, true, BK, true>(
          p.g, lds, acc, csum, false, m0, 0, 0, p.g.K, wm0, wn0);
    else
      gemm_mainloop<FT_ROWS, BN, WAVES_M, WAVES_N, true, true, BK, false>(
          p.g, lds, acc, csum, false, m0, 0, 0, p.g.K, wm0, wn0);
  }

  FT_STAMP(2);
  FT_MARK(1);
  // this lane's output columns' biases (used when the accumulators are staged;
  // fetched here rather than before the k-loop: one register less live through it)
  float bcol[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) bcol[j] = p.g.bias[wn0 + 32 * j + (lane & 31)];
  // the sample of this lane's row (wave 0 computes the loss rows): loads issued
  // here, consumed three barriers later
  float act[8];
  float adv = 0.f, old_ll = 0.f, ret = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) act[j] = 0.f;
  const bool live = m0 + lane < M;
  if (!EVAL && wave == 0) {
    const int m = min(m0 + lane, M - 1);
    const int64_t src = L.idx ? (int64_t)L.idx[m] : (int64_t)m;
    if (L.kind == 1) {
      ret = L.returns[src];
    } else {
      adv = L.adv[src];
      if (L.algo != 1) old_ll = L.old_ll[src];
      const float* arow = L.actions + src * L.lda;
      if (L.kind == 2) {
        act[0] = arow[0];
      } else {
        // action rows are padded to a multiple of 4 floats (16-B aligned)
        const float4 a0 = *reinterpret_cast<const float4*>(arow);
        act[0] = a0.x; act[1] = a0.y; act[2] = a0.z; act[3] = a0.w;
        if (L.A > 4) {
          const float4 a1 = *reinterpret_cast<const float4*>(arow + 4);
          act[4] = a1.x; act[5] = a1.y; act[6] = a1.z; act[7] = a1.w;
        }
      }
    }
  }


  // ---- E1 + E2: H = tanh(accumulators + bias) -> staged rows [64][BN + 4], kept in
  //      the stage only (the activation is applied on the way in: one LDS round
  //      trip and one barrier less than staging first)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float b = bcol[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        stage[rr * LDC + wn0 + 32 * j + (lane & 31)] = tanh_fast(acc[i][j][r] + b);
      }
    }
  FT_STAMP(3);
  __syncthreads();
  FT_STAMP(4);
  // ---- E3: head outputs of the 64 rows (lane = row, wave = a column segment whose
  //      weights are wave-uniform: scalar loads, v_fmac with an SGPR operand)
  {
    const int row = lane, seg = wave;
    float4 h[CPS / 4];
#pragma unroll
    for (int i = 0; i < CPS / 4; ++i)
      h[i] = *reinterpret_cast<const float4*>(stage + row * LDC + seg * CPS + 4 * i);
    float a[HN];
#pragma unroll
    for (int j = 0; j < HN; ++j) {
      a[j] = 0.f;
      if (j < L.A) {
        ft_uniform_ptr w =
            (ft_uniform_ptr)(uintptr_t)(p.head_W + (int64_t)j * p.head_ldw + seg * CPS);
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < CPS / 4; ++i) {
          s0 = fmaf(h[i].x, w[4 * i + 0], s0);
          s1 = fmaf(h[i].y, w[4 * i + 1], s1);
          s0 = fmaf(h[i].z, w[4 * i + 2], s0);
          s1 = fmaf(h[i].w, w[4 * i + 3], s1);
        }
        a[j] = s0 + s1;
      }
    }
    float* mine = aux + ((seg % PL) * 64 + row) * HN;
    if (seg < PL) {
      *reinterpret_cast<float4*>(mine) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(mine + 4) = make_float4(a[4], a[5], a[6], a[7]);
    }
    __syncthreads();
    if (SEGS > PL) {
      if (seg >= PL) {
        float4 lo = *reinterpret_cast<const float4*>(mine);
        float4 hi = *reinterpret_cast<const float4*>(mine + 4);
        lo.x += a[0]; lo.y += a[1]; lo.z += a[2]; lo.w += a[3];
        hi.x += a[4]; hi.y += a[5]; hi.z += a[6]; hi.w += a[7];
        *reinterpret_cast<float4*>(mine) = lo;
        *reinterpret_cast<float4*>(mine + 4) = hi;
      }
      __syncthreads();
    }
    for (int o = tid; o < 64 * HN; o += NT) {
      const int j = o % HN;
      float s = 0.f;
      if (j < L.A) {
        s = p.head_bias[j];
#pragma unroll
        for (int w = 0; w < PL; ++w) s += aux[w * 64 * HN + o];
      }
      outl[o] = s;
      if constexpr (EVAL) {
        const int row = o / HN;
        if (j < L.A && m0 + row < M)
          p.eval_out[(int64_t)(m0 + row) * p.eval_ldo + j] = s;
      }
    }
  }
  if constexpr (EVAL) return;
  __syncthreads();
  FT_STAMP(5);
  // ---- E4: wave 0: the loss rows (d(loss)/d(head output) -> doutl, batch-sum
  //      shares -> lpart); the other waves stage W_head [8][BN] over the planes
  if (wave == 0) {
    float s = 0.f, inv_var = 1.f;
    if (L.kind != 2) {
      s = *L.log_std;
      if (L.kind == 0)
        s = ga_log_std(s, L.has_min, L.min_log_std, L.has_max, L.max_log_std, nullptr);
      inv_var = expf(-2.f * s);
    }
    float out[8], dout[8];
    const float4 o0 = *reinterpret_cast<const float4*>(outl + lane * HN);
    const float4 o1 = *reinterpret_cast<const float4*>(outl + lane * HN + 4);
    out[0] = o0.x; out[1] = o0.y; out[2] = o0.z; out[3] = o0.w;
    out[4] = o1.x; out[5] = o1.y; out[6] = o1.z; out[7] = o1.w;
    double second = 0.0;
    double first = lr_row(L, s, inv_var, out, act, adv, old_ll, ret, dout, &second);
    if (!live) {
      first = 0.0; second = 0.0;
#pragma unroll
      for (int j = 0; j < 8; ++j) dout[j] = 0.f;
    }
    *reinterpret_cast<float4*>(doutl + lane * HN) =
        make_float4(dout[0], dout[1], dout[2], dout[3]);
    *reinterpret_cast<float4*>(doutl + lane * HN + 4) =
        make_float4(dout[4], dout[5], dout[6], dout[7]);
    first = ga_wave_sum(first);
    second = ga_wave_sum(second);
    if (lane == 0) {
      p.lpart[2 * ft_tile + 0] = first;
      p.lpart[2 * ft_tile + 1] = second;
    }
  } else {
    for (int e = tid - 64; e < HN * (BN / 4); e += NT - 64) {
      const int j = e / (BN / 4), c4 = e % (BN / 4);
      float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < L.A)
        w = *reinterpret_cast<const float4*>(p.head_W + (int64_t)j * p.head_ldw + 4 * c4);
      *reinterpret_cast<float4*>(aux + j * BN + 4 * c4) = w;
    }
  }
  __syncthreads();
  FT_STAMP(6);
  // E5 and E6 both read only the staged H and dout: the second half of the grid takes
  // them in the other order, so that the dZ stores of the whole grid (33 MB, every
  // workgroup of the single generation reaching them within a microsecond of the
  // others) spread over twice the window, and the two workgroups of a CU do not
  // contend for the same unit at the same time
  // E5 / E6 take only the head rows that exist (j < A; JN = 1, 4 or 8 compiled): rows
  // of W_head and entries of dout beyond A are zero and add nothing -- the value
  // function's head has ONE row, 7 of 8 products were multiplications by zero
  constexpr int QN = FT_ROWS * (BN / 4) / NT;  // column quads per thread
  auto phase_dz = [&](auto jn_tag, float4* zk) {
  // ---- E5: dZ = (dout W_head) (1 - H^2) -> global (the only [M x BN] store).  A
  //      thread's column quad is the same for all its rows: its W_head values are
  //      read once
  constexpr int JN = decltype(jn_tag)::value;
  static_assert(NT % (BN / 4) == 0, "one column quad per thread");
  float4 w8[JN];
#pragma unroll
  for (int j = 0; j < JN; ++j)
    w8[j] = *reinterpret_cast<const float4*>(aux + j * BN + 4 * (tid % (BN / 4)));
#pragma unroll
  for (int q = 0; q < QN; ++q) {
    const int e = tid + NT * q;
    const int rr = e / (BN / 4), c4 = e % (BN / 4);
    const float4 h = *reinterpret_cast<const float4*>(stage + rr * LDC + 4 * c4);
    const float4 d0 = *reinterpret_cast<const float4*>(doutl + rr * HN);
    float4 d1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (JN > 4) d1 = *reinterpret_cast<const float4*>(doutl + rr * HN + 4);
    const float dd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      z.x = fmaf(dd[j], w8[j].x, z.x); z.y = fmaf(dd[j], w8[j].y, z.y);
      z.z = fmaf(dd[j], w8[j].z, z.z); z.w = fmaf(dd[j], w8[j].w, z.w);
    }
    z.x *= (1.f - h.x * h.x); z.y *= (1.f - h.y * h.y);
    z.z *= (1.f - h.z * h.z); z.w *= (1.f - h.w * h.w);
#ifndef GA_FT_NO_BUFFER_ADDR
    if constexpr (FUSE) {
      // the tile's rows of dZ as a buffer (GaBuffer, common.h; BN floats in the last row
      // that exists): a thread's rows lie NT / (BN / 4) apart, a scalar offset (the
      // descriptor and the lane offset are the same for every q: computed once)
      const GaBuffer dzbuf(p.dZ + (int64_t)m0 * p.lddz,
                           4u * ((uint32_t)(min(FT_ROWS, M - m0) - 1) * (uint32_t)p.lddz +
                                 (uint32_t)BN));
      const uint32_t dz_off = 4u * ((uint32_t)(tid / (BN / 4)) * (uint32_t)p.lddz +
                                    (uint32_t)(4 * (tid % (BN / 4))));
      if (m0 + rr < M)
        dzbuf.store4(z, dz_off, 4u * (uint32_t)((NT / (BN / 4)) * q) * (uint32_t)p.lddz);
    } else
#endif
    if (m0 + rr < M)
      *reinterpret_cast<float4*>(p.dZ + (int64_t)(m0 + rr) * p.lddz + 4 * c4) = z;
    if constexpr (FUSE) {
      // same thread, same address as the H quad above.  Rows beyond M: dout is zero
      // there, but 0 * w is not zero for every w -- the operand gets the zeros the
      // tile loader of the two-launch path gives it
      if (m0 + rr >= M) z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (zk)
        zk[q] = z;
      else
        *reinterpret_cast<float4*>(stage + rr * LDC + 4 * c4) = z;
    }
  }
  };
  auto phase_head_grad = [&](auto jn_tag) {
  // ---- E6: this workgroup's share of dW_head[j][c] = sum_r dout[r][j] H[r][c]
  //      (rows beyond M carry dout = 0) and of db_head
  {
    constexpr int JN = decltype(jn_tag)::value;
    constexpr int GROUPS = NT / BN, JPG = HN / GROUPS;
    const int c = tid % BN, j0 = (tid / BN) * JPG;
    float g[JPG];
#pragma unroll
    for (int jj = 0; jj < JPG; ++jj) g[jj] = 0.f;
    // (j0 is wave-uniform: a whole wave skips the rows its group does not have; within
    // a group `jj < JN` may keep a zero row or two -- they add exact zeros)
    if (j0 < JN) {
      for (int r = 0; r < FT_ROWS; ++r) {
        const float h = stage[r * LDC + c];
#pragma unroll
        for (int jj = 0; jj < JPG; ++jj)
          if (jj < JN) g[jj] = fmaf(doutl[r * HN + j0 + jj], h, g[jj]);
      }
    }
    float* hp = p.hpart + (int64_t)ft_tile * (HN * BN + HN);
#pragma unroll
    for (int jj = 0; jj < JPG; ++jj) hp[(j0 + jj) * BN + c] = g[jj];
    if (tid < HN) {
      float b = 0.f;
      for (int r = 0; r < FT_ROWS; ++r) b += doutl[r * HN + tid];
      hp[HN * BN + tid] = b;
    }
  }
  };
  auto two_phases = [&](auto jn_tag) {
    if constexpr (FUSE) {
#ifdef GA_FT_NO_EARLY_DZ
      // E6 reads the staged H that E5 overwrites
      phase_head_grad(jn_tag);
      FT_STAMP(7);
      __syncthreads();
      phase_dz(jn_tag, nullptr);
      dgl->issue();
#else
      // E5 with its quads kept, E6 on the H that is still staged, then the quads over it
      float4 zk[QN];
      dgl->issue();
      phase_dz(jn_tag, zk);
      FT_STAMP(7);
      phase_head_grad(jn_tag);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < QN; ++q) {
        const int e = tid + NT * q;
        *reinterpret_cast<float4*>(stage + (e / (BN / 4)) * LDC + 4 * (e % (BN / 4))) = zk[q];
      }
#endif
    } else if (ft_tile >= (ft_tiles + 1) / 2) {
      phase_head_grad(jn_tag);
      FT_STAMP(7);
      phase_dz(jn_tag, nullptr);
    } else {
      phase_dz(jn_tag, nullptr);
      FT_STAMP(7);
      phase_head_grad(jn_tag);
    }
  };
  if (L.A == 1)
    two_phases(std::integral_constant<int, 1>{});
  else if (L.A <= 4)
    two_phases(std::integral_constant<int, 4>{});
  else
    two_phases(std::integral_constant<int, 8>{});
  FT_STAMP(8);
  FT_MARK(2);
  if constexpr (FUSE) {
    static_assert(AUX_FLOATS >= FT_ROWS * 32, "the observation rows fit in aux");
    keep->stage = stage;
    keep->aux = aux;
  }
}

template <int BN, int WAVES_M, int WAVES_N, bool L1 = false, int KSC = 0>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void fwd_head_loss_kernel(
    FwdLossParams p) {
  fwd_head_loss_body<BN, WAVES_M, WAVES_N, L1, false, KSC>(p, (int)blockIdx.x,
                                                           (int)gridDim.x);
}

// (FwdLossPair, fused_params.h: the same step of TWO networks in one grid)
template <int BN, int WAVES_M, int WAVES_N, int KSC>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void fwd_head_loss_pair_kernel(
    FwdLossPair pp) {
  const int tile = (int)(blockIdx.x >> 1), tiles = (int)(gridDim.x >> 1);
  if (blockIdx.x & 1)
    fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, false, KSC>(pp.b, tile, tiles);
  else
    fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, false, KSC>(pp.a, tile, tiles);
}

template <int BN, int WAVES_M, int WAVES_N, int KSC = 0>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void mlp_eval_forward_kernel(
    FwdLossParams p) {
  fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, true, KSC>(p, (int)blockIdx.x,
                                                            (int)gridDim.x);
}

// the split-operand instantiation (opt-in; 256 units, first layer in the kernel)
template <int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 4) void fwd_head_loss_split_kernel(
    FwdLossParams p) {
  fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, false, 0, true>(p, (int)blockIdx.x,
                                                                  (int)gridDim.x);
}

template <int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 4) void mlp_eval_forward_split_kernel(
    FwdLossParams p) {
  fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, true, 0, true>(p, (int)blockIdx.x,
                                                                 (int)gridDim.x);
}

// A weight matrix W [rows][ld] as the B operand B(k, n) of the split-operand loops,
// three bf16 planes in FRAGMENT order: plane pl at out + pl * N * Kc; within a plane the
// 16-byte fragment of lane l = (n % 32) + 32 * ((k / 8) % 2) of the 32-column block
// n / 32 for the 16-deep k group k / 16 sits at ((k / 16) * (N / 32) + n / 32) * 64 + l
// (in units of 8 bf16): one wave's load instruction reads 1 KB of consecutive bytes.
//   fwd: B(k, n) = W[n * ld + k]   (N = rows, Kc = cols: n = unit of this layer)
//   bwd: B(k, n) = W[k * ld + n]   (N = cols, Kc = rows: n = unit of the layer below)
// BWD_ONLY = false: blocks [0, half) write fwd, [half, 2 half) write bwd.
template <bool BWD_ONLY>
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ W,
                                                           int64_t ld, int rows, int cols,
                                                           uint32_t* __restrict__ fwd,
                                                           uint32_t* __restrict__ bwd) {
  // one thread per PAIR of consecutive k (one dword of every plane); both dimensions
  // are padded to multiples of 32 in the planes, the padding is zero
  const int rows_p = (rows + 31) & ~31, cols_p = (cols + 31) & ~31;
  const int64_t pairs = (int64_t)rows_p * cols_p / 2;
  const int64_t half_blocks = (pairs + 255) / 256;
  const bool T = BWD_ONLY || (int64_t)blockIdx.x >= half_blocks;
  const int64_t e =
      ((int64_t)blockIdx.x - ((T && !BWD_ONLY) ? half_blocks : 0)) * 256 + threadIdx.x;
  if (e >= pairs) return;
  const int N = T ? cols_p : rows_p;
  // e enumerates the OUTPUT order (contiguous writes; the reads of bwd are strided:
  // a few 100 K elements, nothing to optimise)
  const int kk = 2 * (int)(e & 3);
  const int l = (int)((e >> 2) & 63);
  const int64_t blk = e >> 8;
  const int nb = (int)(blk % (N / 32)), kg = (int)(blk / (N / 32));
  const int n = 32 * nb + (l & 31);
  const int k = 16 * kg + 8 * (l >> 5) + kk;
  // W row / column of the two elements
  const int r0 = T ? k : n, c0 = T ? n : k;
  const int r1 = T ? k + 1 : n, c1 = T ? n : k + 1;
  const float x0 = (r0 < rows && c0 < cols) ? W[(int64_t)r0 * ld + c0] : 0.f;
  const float x1 = (r1 < rows && c1 < cols) ? W[(int64_t)r1 * ld + c1] : 0.f;
  uint32_t hi, mid, lo;
  ft_split3_pair(x0, x1, hi, mid, lo);
  uint32_t* out = T ? bwd : fwd;
  out[e] = hi;
  out[pairs + e] = mid;
  out[2 * pairs + e] = lo;
}

// (the sum of one parameter quad's partials -- ft_share_run and its neighbours -- is
// in reduce_trees.h: reduce_members_adam_kernel of members_step.hip runs it too)

// (FtSlabSum: fused_params.h)

// The other lane of a lane pair (l ^ 1), as a DPP operand: no LDS round trip
__device__ __forceinline__ float ft_pair_swap(float x) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float4 ft_pair_swap(const float4& v) {
  return make_float4(ft_pair_swap(v.x), ft_pair_swap(v.y), ft_pair_swap(v.z),
                     ft_pair_swap(v.w));
}

// The quads of FtSlabSum are spread evenly over the launch's workgroups; a workgroup
// takes its quads 8 * (NT / 64) at a time (a pass): wave w the 8 quads from 8 w on,
// lane l quad (l % 16) / 2 and share l / 16 (four shares, no wave-shares).  A STEP is
// one group of four partials per share (or the run's last one to three): issue() puts
// its loads in flight, consume() adds them; the last step of a pass lets the shares
// meet and the lane of share 0 -- the one that read partial 0 -- writes the sum over
// it.  The two lanes of a pair hold the same share of the same quad and load HALF a
// group each (lane bit 0 = 0: v0, v1; 1: v2, v3: eight registers in flight per lane
// instead of sixteen); (v0 + v1) and (v2 + v3) cross the pair, and both lanes carry
// the same accumulator.
// No other workgroup reads or writes that quad's partials.  gemm_mainloop runs one
// step per k-step (the loads land under the MFMAs); drain() runs what is left.
// Every load is unconditional: quads are clamped to the workgroup's last one, partials
// to the last one, and what a clamped lane loaded is not used.
// IN_LOOP = false: everything in drain().
template <int NT, bool IN_LOOP>
struct FtSlabSummer {
  static constexpr int QPW = 8;               // quads per wave and pass
  static constexpr int QPP = QPW * (NT / 64);  // quads per pass
  const FtSlabSum& S;
  int wave, lane;
  int chunk, steps, q_end, pass_base, j;
  int in_loop;    // steps of the first pass that gemm_mainloop still runs
  bool fast;      // every share's run is whole groups of four
  bool busy;      // this workgroup has a pass under way
  bool wave_on;   // ... and this wave has quads in it
  uint32_t sb;    // bytes between partials
  // bytes from S.base to this lane's quad; fast: to the first partial this lane
  // loads (share 0, lane bit 0 = 0: partial 0 either way)
  uint32_t voff;
  float4 acc, v[2];

  __device__ __forceinline__ FtSlabSummer(const FtSlabSum& S_, int tile) : S(S_) {
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    lane = threadIdx.x & 63;
    busy = wave_on = false;
    in_loop = 0;
    if (S.n_part <= 0) return;
    const int nq = S.nq[0] + S.nq[1];
    const int per = (nq + S.tiles - 1) / S.tiles;
    chunk = (S.n_part + 3) / 4;
    fast = S.n_part == 4 * chunk && chunk % 4 == 0;
    steps = (chunk + 3) / 4;
    sb = (uint32_t)S.stride * 4u;
    // (tile * per < 2^31: tile < tiles and per <= nq / tiles + 1)
    pass_base = min(nq, tile * per);
    q_end = min(nq, pass_base + per);
    start_pass();
    in_loop = (IN_LOOP && fast && wave_on) ? steps : 0;
  }
  __device__ __forceinline__ int lane_quad() const {
    return pass_base + QPW * wave + ((lane & 15) >> 1);
  }
  __device__ __forceinline__ void start_pass() {
    busy = pass_base < q_end;
    wave_on = pass_base + QPW * wave < q_end;
    j = 0;
    if (!wave_on) return;
    const int qc = min(lane_quad(), q_end - 1);  // (its own quads only)
    const uint32_t qoff = qc < S.nq[0] ? S.off[0] + 4u * (uint32_t)qc
                                       : S.off[1] + 4u * (uint32_t)(qc - S.nq[0]);
    voff = 4u * qoff +
           (fast ? (uint32_t)((lane >> 4) * chunk + 2 * (lane & 1)) * sb : 0u);
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // gemm_mainloop's side work: steps of whole groups of the workgroup's FIRST pass --
  // two loads and twelve additions per step and nothing else in the loop (beside an
  // fp32 MFMA every vector instruction costs its full issue time); ragged steps (three
  // times the registers), the end of the pass and further passes wait for drain()
  __device__ __forceinline__ void issue() {
    if (IN_LOOP && in_loop > 0) issue_step<true>();
  }
  __device__ __forceinline__ void consume() {
    if (IN_LOOP && in_loop > 0) {
      add_step<true>();
      --in_loop;
    }
  }
  template <bool FAST>
  __device__ __forceinline__ void issue_step() {
    if (FAST) {
      // a wave-uniform base per load (scalar registers) and one 32-bit lane offset: no
      // vector address arithmetic
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t uo = __builtin_amdgcn_readfirstlane((uint32_t)(4 * j + i) * sb);
        const char* bi = reinterpret_cast<const char*>(S.base) + uo;
        v[i] = *reinterpret_cast<const float4*>(bi + voff);
      }
    } else {
      const char* b = reinterpret_cast<const char*>(S.base);
      const int k = (lane >> 4) * chunk + 4 * j + 2 * (lane & 1);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        v[i] = *reinterpret_cast<const float4*>(
            b + (voff + (uint32_t)min(k + i, S.n_part - 1) * sb));
    }
  }
  template <bool FAST>
  __device__ __forceinline__ void add_step() {
    if (FAST) {
      // this lane's half (v0 + v1) or (v2 + v3), then the pair's other half: the two
      // lanes add the same two values, (v0 + v1) + (v2 + v3)
      const float4 h = make_float4(v[0].x + v[1].x, v[0].y + v[1].y, v[0].z + v[1].z,
                                   v[0].w + v[1].w);
      const float4 o = ft_pair_swap(h);
      acc.x += h.x + o.x; acc.y += h.y + o.y; acc.z += h.z + o.z; acc.w += h.w + o.w;
    } else {
      const bool hi = lane & 1;
      const float4 o0 = ft_pair_swap(v[0]), o1 = ft_pair_swap(v[1]);
      const float4 v0 = hi ? o0 : v[0], v1 = hi ? o1 : v[1];
      const float4 v2 = hi ? v[0] : o0, v3 = hi ? v[1] : o1;
      const int p0 = (lane >> 4) * chunk, p1 = min(S.n_part, p0 + chunk);
      const int k = p0 + 4 * j;
      if (k + 4 <= p1) {
        ft_sum_group4(acc, v0, v1, v2, v3);
      } else {
        if (k < p1) ft_sum_single(acc, v0);
        if (k + 1 < p1) ft_sum_single(acc, v1);
        if (k + 2 < p1) ft_sum_single(acc, v2);
      }
    }
    ++j;
  }
  __device__ __forceinline__ void drain() {
    in_loop = 0;
    while (busy) {
      if (wave_on) {
        if (fast) {
          while (j < steps) {
            issue_step<true>();
            add_step<true>();
          }
        } else {
          while (j < steps) {
            issue_step<false>();
            add_step<false>();
          }
        }
        float g[4] = {acc.x, acc.y, acc.z, acc.w};
        ft_lane_shares_meet(g, 16);
        if (lane < 16 && !(lane & 1) && lane_quad() < q_end)
          *reinterpret_cast<float4*>(reinterpret_cast<char*>(S.base) + voff) =
              make_float4(g[0], g[1], g[2], g[3]);
      }
      pass_base += QPP;
      start_pass();
    }
  }
};

// ---------------------------------------------------------------------------
constexpr int FT_LDXS = 32;  // staged observation rows: 32 floats (zero beyond in_w)

// The workgroup's observation rows, two quads per thread: loads issued in front of the
// k-loop, staged behind it (dgrad_wgrad0_tail)
template <int NT>
__device__ __forceinline__ void dgrad_load_x(const DgradWgrad0Params& p, const int ft_tile,
                                             float4 (&xq)[2]) {
  static_assert(FT_ROWS * (FT_LDXS / 4) <= 2 * NT, "at most two quads of X per thread");
  const int tid = threadIdx.x;
  const int m0 = ft_tile * FT_ROWS;
  const int M = p.g.M;
  const int ld0 = (p.in_w + 3) & ~3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + NT * i;
    const int rr = min(e / (FT_LDXS / 4), FT_ROWS - 1);
    const int q = min(e % (FT_LDXS / 4), ld0 / 4 - 1);
    const int m = min(m0 + rr, M - 1);
    const int64_t src = p.idx ? (int64_t)p.idx[m] : (int64_t)m;
    xq[i] = *reinterpret_cast<const float4*>(p.X + src * p.ldx + 4 * q);
  }
}

// The data-gradient k-loop on an A operand that is ALREADY in LDS: `stage` holds the
// tile's 64 rows of dZ2 [64][BN + 4], k-contiguous (fwd_head_loss_body<FUSE> left them
// there; K = BN), so the loop loads no A, stores nothing to LDS and has no barrier.
// A fragments: one 16-B read per row block and group of four MFMAs (BN + 4 has the
// residue of BK + PAD mod 32: gemm_mainloop's conflict-free pattern).  B fragments:
// FtW2Frags, one step ahead (the caller has requested step 0's), refilled in place as
// soon as the group's MFMAs are issued.  MFMAs per accumulator in gemm_mainloop's order
// (s, g, q): the same bits as dgrad_wgrad0_body's loop.
template <int BN, int TM, int TN>
__device__ __forceinline__ void dgrad_kloop_staged(const float* stage, FtW2Frags<BN, TN>& w,
                                                   f32x16 (&acc)[TM][TN], const int wm0) {
  constexpr int LDC = BN + 4;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const float* arow = stage + (wm0 + l31) * LDC + 4 * half;
  constexpr int nk = BN / BK;
#pragma unroll
  for (int s = 0; s < nk; ++s) {
    const bool more = s + 1 < nk;
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
      float a[TM][4];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const float4 v =
            *reinterpret_cast<const float4*>(arow + 32 * i * LDC + 32 * s + 8 * g);
        a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][q], w.bn[j][g][q], acc[i][j],
                                                             0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      if (more) w.fetch_group(s + 1, g);
    }
  }
}

template <int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void dgrad_wgrad0_tail(
    const DgradWgrad0Params& p, const int ft_tile,
    f32x16 (&acc)[FT_ROWS / WAVES_M / 32][BN / WAVES_N / 32], const float4 (&xq)[2],
    float* stage, float* xs);

template <int BN, int WAVES_M, int WAVES_N, bool SPLIT = false>
__device__ __forceinline__ void dgrad_wgrad0_body(const DgradWgrad0Params& p,
                                                  const int ft_tile) {
  static_assert(!SPLIT || (BN == 256 && WAVES_M == 1 && WAVES_N == 8),
                "the split-operand loop is written for the 256-unit, 8-wave tile");
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int WM = FT_ROWS / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int LDK = BK + PAD, LDB_S = BN + PAD;
  constexpr int A_FLOATS = FT_ROWS * LDK, B_FLOATS = BK * LDB_S;
  constexpr int LDC = BN + 4;
  constexpr int STAGE_FLOATS = FT_ROWS * LDC;
  constexpr int TILE_FLOATS =
      A_FLOATS + B_FLOATS > STAGE_FLOATS ? A_FLOATS + B_FLOATS : STAGE_FLOATS;
  __shared__ __attribute__((aligned(16))) float lds[TILE_FLOATS];
  __shared__ __attribute__((aligned(16))) float xs[FT_ROWS * FT_LDXS];
  float* stage = lds;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WAVES_N) * WM;
  const int wn0 = (wave % WAVES_N) * WN;
  const int m0 = ft_tile * FT_ROWS;
  const int M = p.g.M;

  FT_STAMP(0);
  FT_MARK(0);
  // the workgroup's observation rows: loads issued now, staged after the k-loop
  float4 xq[2];
  dgrad_load_x<NT>(p, ft_tile, xq);

  // the slab sum: one step per k-step of the plain loop, the rest (all of it beside the
  // hand-scheduled split-operand loop, and at 64 units, where the steps' registers
  // would cost the kernel a wave per SIMD) behind the loop
  FtSlabSummer<NT, (!SPLIT && BN > 64)> slab(p.sum, ft_tile);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  // (measured and not kept for this k-loop, see DESIGN.md section 5: B fragments
  // straight from L2 with the dZ2 tile double buffered in LDS and one barrier per
  // step -- 52.8 us; no LDS and no barrier at all, every wave fetching its own A and
  // B fragments -- 62.1 us; against 50.9 us for the two-barrier loop below.  Both
  // were measured in THIS kernel, where dZ2 comes from memory and has to be staged.
  // Where it is in LDS already -- fwd_dgrad_kernel, behind the forward body of the same
  // tile -- the B-from-L2 loop needs no A loads, no LDS stores and no barrier
  // (dgrad_kloop_staged), and the one launch takes 98.2 us against 54.5 + 52.6 for
  // the two: DESIGN.md section 9 item 3, profiles/r05_notes.md)
  if constexpr (SPLIT) {
    // ---- split-operand k-loop (see ft_split3): the dZ2 tile is fetched as one 16-B
    // quad per thread and 32-deep step, TWO steps ahead (it comes from HBM), split and
    // written to three bf16 LDS planes one step ahead; the W2 planes come straight
    // from L2 in fragment order, one step ahead, refilled in place; 24 MFMAs per step
    // and wave, one barrier.
    static_assert(TM == 2 && TN == 1 && NT == 512, "the slot list below");
    char* apl = reinterpret_cast<char*>(lds);
    const int half = lane >> 5, l31 = lane & 31;
    const int K = p.g.K, nk = K / BK;  // (K % 32 == 0: the host checks)
    const int qrow = tid >> 3, qq = tid & 7;
    const bool row_ok = m0 + qrow < M;
    const float* arow_g = p.g.A + (int64_t)min(m0 + qrow, M - 1) * p.g.lda + 4 * qq;
    auto load_quad = [&](int s) { return *reinterpret_cast<const float4*>(arow_g + 32 * s); };
    auto store_quad = [&](int s, float4 v) {
      if (!row_ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
      uint32_t hi[2], mid[2], lo[2];
      ft_split3_pair(v.x, v.y, hi[0], mid[0], lo[0]);
      ft_split3_pair(v.z, v.w, hi[1], mid[1], lo[1]);
      char* dst = apl + (s & 1) * FT_ABUF_B + qrow * FT_PLANE_ROW_B + qq * 8;
      *reinterpret_cast<uint2*>(dst) = make_uint2(hi[0], hi[1]);
      *reinterpret_cast<uint2*>(dst + FT_PLANE_B) = make_uint2(mid[0], mid[1]);
      *reinterpret_cast<uint2*>(dst + 2 * FT_PLANE_B) = make_uint2(lo[0], lo[1]);
    };
    const uint16_t* wpl = p.bplanes + ((wn0 / 32) * 64 + lane) * 8;
    ft_u32x4 bw[2][3];
    auto fetch_planes = [&](int s, int g) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        bw[g][pl] = *reinterpret_cast<const ft_u32x4*>(
            wpl + pl * p.bplane_stride + ((2 * s + g) * (BN / 32)) * 512);
    };
    fetch_planes(0, 0);
    fetch_planes(0, 1);
    float4 qc = load_quad(0);
    float4 qn = nk > 1 ? load_quad(1) : qc;
    store_quad(0, qc);
    qc = qn;
    __syncthreads();
#define FT_SB __builtin_amdgcn_sched_barrier(0)
    for (int s = 0; s < nk; ++s) {
      const bool more = s + 1 < nk;
      const char* arow = apl + (s & 1) * FT_ABUF_B + (wm0 + l31) * FT_PLANE_ROW_B + 16 * half;
      ft_u32x4 af[2][TM][3];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          af[0][i][pl] = *reinterpret_cast<const ft_u32x4*>(arow + pl * FT_PLANE_B +
                                                            32 * i * FT_PLANE_ROW_B);
      if (s + 2 < nk) qn = load_quad(s + 2);
      FT_SB;
      FT_SPLIT_PRIO(1);
#pragma unroll
      for (int slot = 0; slot < 24; ++slot) {
        const int g = slot / 12, t = (slot % 12) / 2, i = slot % 2;
        const int pa = t == 0 ? 2 : (t == 1 || t == 2) ? 1 : 0;
        const int pb = t == 3 ? 2 : (t == 1 || t == 4) ? 1 : 0;
#ifdef GA_DABL_NOMFMA
        acc[i][0][slot & 15] += __uint_as_float(af[g][i][pa][0] ^ bw[g][pb][0]);
#else
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            __builtin_bit_cast(ft_bf16x8, af[g][i][pa]),
            __builtin_bit_cast(ft_bf16x8, bw[g][pb]), acc[i][0], 0, 0, 0);
#endif
        FT_SB;
        if (slot == 6 || slot == 8 || slot == 11) {
          const int pl = slot == 6 ? 2 : slot == 8 ? 1 : 0;
#pragma unroll
          for (int ii = 0; ii < TM; ++ii)
            af[1][ii][pl] = *reinterpret_cast<const ft_u32x4*>(
                arow + pl * FT_PLANE_B + 32 * ii * FT_PLANE_ROW_B + 32);
        }
        if (more) {
#ifndef GA_DABL_NOSTORE
          if (slot == 2) store_quad(s + 1, qc);
#endif
#ifndef GA_DABL_NOFETCH
          if (slot == 11) fetch_planes(s + 1, 0);
          if (slot == 23) fetch_planes(s + 1, 1);
#endif
        }
        FT_SB;
      }
      FT_SPLIT_PRIO(0);
      qc = qn;
      __syncthreads();
    }
#undef FT_SB
  } else {
    float csum = 0.f;
    const bool full = m0 + FT_ROWS <= M;
    if (full)
      gemm_mainloop<FT_ROWS, BN, WAVES_M, WAVES_N, true, false, BK, true>(
          p.g, lds, acc, csum, false, m0, 0, 0, p.g.K, wm0, wn0, slab);
    else
      gemm_mainloop<FT_ROWS, BN, WAVES_M, WAVES_N, true, false, BK, false>(
          p.g, lds, acc, csum, false, m0, 0, 0, p.g.K, wm0, wn0, slab);
  }
  slab.drain();
  FT_STAMP(1);
  FT_MARK(1);
  dgrad_wgrad0_tail<BN, WAVES_M, WAVES_N>(p, ft_tile, acc, xq, stage, xs);
}

// Behind the data-gradient k-loop: the accumulators (dZ2 W2 of the tile) times the
// slope of H1 -> dZ1 in `stage`, then this workgroup's shares of dW1 and db1.  Nobody
// reads `stage` or `xs` ([64][32] floats) any more when this is called.
template <int BN, int WAVES_M, int WAVES_N>
__device__ __forceinline__ void dgrad_wgrad0_tail(
    const DgradWgrad0Params& p, const int ft_tile,
    f32x16 (&acc)[FT_ROWS / WAVES_M / 32][BN / WAVES_N / 32], const float4 (&xq)[2],
    float* stage, float* xs) {
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int WM = FT_ROWS / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int LDC = BN + 4;
  constexpr int LDXS = FT_LDXS;
  static_assert((FT_ROWS * (BN / 4)) % NT == 0, "whole quads per thread");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WAVES_N) * WM;
  const int wn0 = (wave % WAVES_N) * WN;
  const int m0 = ft_tile * FT_ROWS;
  const int M = p.g.M;
  const int ld0 = (p.in_w + 3) & ~3;

  // H1 of this thread's quads: in flight while the accumulators are staged
  float4 hq[FT_ROWS * (BN / 4) / NT];
#pragma unroll
  for (int q = 0; q < FT_ROWS * (BN / 4) / NT; ++q) {
    const int e = tid + NT * q;
    const int rr = e / (BN / 4), c4 = e % (BN / 4);
    const int m = min(m0 + rr, M - 1);
    hq[q] = *reinterpret_cast<const float4*>(p.H + (int64_t)m * p.ldh + 4 * c4);
  }
  FT_STAMP(6);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        stage[rr * LDC + wn0 + 32 * j + (lane & 31)] = acc[i][j][r];
      }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + NT * i;
    if (e < FT_ROWS * (LDXS / 4)) {
      const int rr = e / (LDXS / 4), q = e % (LDXS / 4);
      float4 x = xq[i];
      const bool row_ok = m0 + rr < M;
      x.x = (row_ok && 4 * q + 0 < p.in_w) ? x.x : 0.f;
      x.y = (row_ok && 4 * q + 1 < p.in_w) ? x.y : 0.f;
      x.z = (row_ok && 4 * q + 2 < p.in_w) ? x.z : 0.f;
      x.w = (row_ok && 4 * q + 3 < p.in_w) ? x.w : 0.f;
      *reinterpret_cast<float4*>(xs + rr * LDXS + 4 * q) = x;
    }
  }
  __syncthreads();
  FT_STAMP(2);
  // dZ1 = (dZ2 W2) (1 - H1^2), kept in the stage only (rows beyond M are zero: their
  // dZ2 rows were masked by the loader)
#pragma unroll
  for (int q = 0; q < FT_ROWS * (BN / 4) / NT; ++q) {
    const int e = tid + NT * q;
    const int rr = e / (BN / 4), c4 = e % (BN / 4);
    const float4 h = hq[q];
    float4 v = *reinterpret_cast<const float4*>(stage + rr * LDC + 4 * c4);
    v.x *= (1.f - h.x * h.x); v.y *= (1.f - h.y * h.y);
    v.z *= (1.f - h.z * h.z); v.w *= (1.f - h.w * h.w);
    *reinterpret_cast<float4*>(stage + rr * LDC + 4 * c4) = v;
  }
  __syncthreads();
  FT_STAMP(3);
  // this workgroup's share of dW1[n][k] = sum_r dZ1[r][n] X[r][k] on the matrix
  // cores -- [BN x 64] (dZ1^T, read down the staged columns) x [64 x 32] (the staged
  // observation rows), one 32-row tile of dW1 per wave, two accumulation chains --
  // and of db1[n] (column sums of dZ1)
  {
    const int half = lane >> 5, l31 = lane & 31;
    float* wp = p.wpart + (int64_t)ft_tile * ((int64_t)BN * ld0 + BN);
    for (int t = wave; t < BN / 32; t += NT / 64) {
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
      for (int g = 0; g < FT_ROWS / 8; ++g) {
        float a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 8 * g + 4 * half + q;
          a[q] = stage[r * LDC + 32 * t + l31];
          b[q] = xs[r * LDXS + l31];
        }
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc1, 0, 0, 0);
      }
      if (l31 < ld0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
          wp[(int64_t)n * ld0 + l31] = acc0[r] + acc1[r];
        }
      }
    }
    if (tid < BN) {
      float b = 0.f;
#pragma unroll 8
      for (int r = 0; r < FT_ROWS; ++r) b += stage[r * LDC + tid];
      wp[(int64_t)BN * ld0 + tid] = b;
    }
  }
  FT_STAMP(4);
  FT_MARK(2);
}

template <int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void dgrad_wgrad0_kernel(
    DgradWgrad0Params p) {
  dgrad_wgrad0_body<BN, WAVES_M, WAVES_N>(p, (int)blockIdx.x);
}

template <int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 4) void dgrad_wgrad0_split_kernel(
    DgradWgrad0Params p) {
  dgrad_wgrad0_body<BN, WAVES_M, WAVES_N, true>(p, (int)blockIdx.x);
}

// two networks in one grid (see fwd_head_loss_pair_kernel)
template <int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void dgrad_wgrad0_pair_kernel(
    DgradWgrad0Pair pp) {
  const int tile = (int)(blockIdx.x >> 1);
  if (blockIdx.x & 1)
    dgrad_wgrad0_body<BN, WAVES_M, WAVES_N>(pp.b, tile);
  else
    dgrad_wgrad0_body<BN, WAVES_M, WAVES_N>(pp.a, tile);
}

// The forward + loss body and the data-gradient body of the SAME 64-row tile in one
// workgroup (two hidden layers of equal width, first layer in the kernel, exact fp32).
// Workgroup t of dgrad_wgrad0_kernel reads back exactly the dZ2 rows workgroup t of
// fwd_head_loss_kernel stored, restages them 32 columns at a time behind two barriers a
// step, gathers the observation rows again and pays a second launch ramp, prologue and
// drain.  Here dZ2 stays in the stage as the k-contiguous A operand
// (dgrad_kloop_staged) and the rest of the data-gradient body follows unchanged.  dZ2
// still goes to memory once: the middle layer's weight-gradient GEMM reads it -- AFTER
// this launch, so its split-K slabs cannot be summed here (DgradWgrad0Params::sum is
// unused) and the optimizer launch sums them.  Same arithmetic in the same order per
// element as the two launches: the same bits.
// LDS: what the forward body has (the observation rows go to its aux block).
template <int BN, int WAVES_M, int WAVES_N, int KSC>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N,
                             WAVES_M * WAVES_N == 8 ? 4 : 2) void fwd_dgrad_kernel(
    FwdDgradParams pp) {
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int WM = FT_ROWS / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  const int ft_tile = (int)blockIdx.x;
  FtFusedLds l;
  const DgradWgrad0Params& p = pp.d;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm0 = (wave / WAVES_N) * WM;
  const int wn0 = (wave % WAVES_N) * WN;
  FtDgradLoads<BN, TN, NT> dgl(p, ft_tile, wn0);
  fwd_head_loss_body<BN, WAVES_M, WAVES_N, true, false, KSC, false, true>(
      pp.f, ft_tile, (int)gridDim.x, &l, &dgl);
  FT_STAMP(0);
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  __syncthreads();  // dZ2 is in the stage
  FT_STAMP(5);
  dgrad_kloop_staged<BN>(l.stage, dgl.w, acc, wm0);
  FT_STAMP(1);
  // The tail overwrites the stage (every wave read all of it) and reads H1 from
  // memory, where other threads of this workgroup stored it during the forward k-loop.
  // A workgroup-scope release / acquire pair around the barrier is enough for that: the
  // workgroup sits on one CU, so stores and loads go through the same vector L1, and
  // the loads are the first this launch makes of those lines (an H1 row is a whole
  // number of lines that belong to this tile alone) -- no stale copy can be there.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  dgrad_wgrad0_tail<BN, WAVES_M, WAVES_N>(p, ft_tile, acc, dgl.xq, l.stage, l.aux);
}

// ---------------------------------------------------------------------------
// (FtRegion, FtNet, ReduceRegionsParams: fused_params.h)
__global__ __launch_bounds__(256) void reduce_regions_adam_kernel(ReduceRegionsParams p) {
  // A short launch on its chain's critical path that usually lands beside the other
  // chain's GEMM-class kernel (traced: 17-57 us there against 11 us alone): its waves
  // go first on the CU.  Interleaved A/B on one box: C3 9.13 -> 9.80 M env-steps/s.
  __builtin_amdgcn_s_setprio(3);
  if ((int64_t)blockIdx.x >= p.n_virtual) {
    // ---- the loss scalars and the log-std slot (flat index 0) of one network, one
    //      wave
    if (threadIdx.x >= 64) return;
    const FtNet& N = p.net[(int64_t)blockIdx.x - p.n_virtual];
    double first = 0.0, second = 0.0;
    for (int b = threadIdx.x; b < N.n_lpart; b += 64) {
      first += N.lpart[2 * b + 0];
      second += N.lpart[2 * b + 1];
    }
    first = ga_wave_sum(first);
    second = ga_wave_sum(second);
    if (threadIdx.x != 0) return;
    float loss, dls;
    lr_finish(N.loss, first, second, N.M, &loss, &dls);
    if (N.loss_out) *N.loss_out = loss;
    float g = N.zero_slot0 ? 0.f : dls * N.scale;
    N.grads[0] = g;
    if (N.do_adam) {
      float pp = N.a.p[0], mm = N.a.m[0], vv = N.a.v[0];
      ga_adam_update(N.a.c, g, pp, mm, vv);
      N.a.p[0] = pp; N.a.m[0] = mm; N.a.v[0] = vv;
    }
    return;
  }
  // A workgroup = Q adjacent quads of one region x 4 (64 / Q) shares of the partials:
  // lane l holds quad l % Q and lane-share l / Q, wave w the wave-share w; a share
  // sums a contiguous run of partials with four independent 16-B loads in flight.
  // Q = 64 (whole 1-KB rows per load instruction, 4 shares) for regions of up to 128
  // partials -- the split-K slabs --, Q = 16 (256-B segments, 16 shares) for the
  // small regions with one partial per 64-row tile.  The lane-shares meet in a
  // butterfly, the wave-shares in LDS, both fixed trees (ft_share_run and its
  // neighbours above).
  __shared__ float4 wsum[4][64];
  const int64_t b = blockIdx.x;
  int ri = 0;
#pragma unroll 1
  for (int k = 1; k < p.n_regions; ++k)
    if (b >= p.r[k].vbeg) ri = k;
  const FtRegion& R = p.r[ri];
  const FtNet& N = p.net[R.net];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float g[4];
  int64_t e4;  // this lane's quad
  if (R.pre) {
    // partial 0 already holds the sum of the region's partials (the data-gradient
    // launch ran the tree above on them): the region as one of n_part = 1, in which
    // shares 1 .. 3 contribute exact zeros -- a quad per thread, nothing to meet
    e4 = (b - R.vbeg) * 256 + threadIdx.x;
    if (4 * e4 >= R.n) return;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    ft_wave_shares_meet(g, ft_share_run(R.src + 4 * e4, R.stride, 0, 1), zero, zero, zero);
  } else {
    const int Q = R.quads;  // 64 or 16
    const int lwc = 64 / Q;
    const int q = lane % Q, lw = lane / Q;
    const int way = lwc * wv + lw;
    e4 = (b - R.vbeg) * Q + q;
    const bool on = 4 * e4 < R.n;
    const int shares = 4 * lwc;
    const int chunk = (R.n_part + shares - 1) / shares;
    const int p0 = way * chunk, p1 = min(R.n_part, p0 + chunk);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) acc = ft_share_run(R.src + 4 * e4, R.stride, p0, p1);
    g[0] = acc.x; g[1] = acc.y; g[2] = acc.z; g[3] = acc.w;
    ft_lane_shares_meet(g, Q);
    if (lw == 0) wsum[wv][q] = make_float4(g[0], g[1], g[2], g[3]);
    __syncthreads();
    if ((int)threadIdx.x >= Q || !on) return;
    ft_wave_shares_meet(g, wsum[0][q], wsum[1][q], wsum[2][q], wsum[3][q]);
  }
  const int64_t i = R.beg + 4 * e4;
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] *= N.scale;
  *reinterpret_cast<float4*>(N.grads + i) = make_float4(g[0], g[1], g[2], g[3]);
  if (N.do_adam) {
    float4 p4 = *reinterpret_cast<float4*>(N.a.p + i);
    float4 m4 = *reinterpret_cast<float4*>(N.a.m + i);
    float4 v4 = *reinterpret_cast<float4*>(N.a.v + i);
    float pp[4] = {p4.x, p4.y, p4.z, p4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w},
          vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) ga_adam_update(N.a.c, g[j], pp[j], mm[j], vv[j]);
    *reinterpret_cast<float4*>(N.a.p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
    *reinterpret_cast<float4*>(N.a.m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
    *reinterpret_cast<float4*>(N.a.v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    if (N.pl_fwd && i >= N.pl_beg && i < N.pl_beg + (int64_t)N.pl_rows * N.pl_cols) {
      // this quad = W[n][k .. k + 3]; the layout of split_planes_kernel (rows and cols
      // are multiples of 32 here)
      const int64_t e0 = i - N.pl_beg;
      const int n = (int)(e0 / N.pl_cols), k = (int)(e0 % N.pl_cols);
      const int64_t total = (int64_t)N.pl_rows * N.pl_cols;
      uint32_t hi[2], mid[2], lo[2];
      ft_split3_pair(pp[0], pp[1], hi[0], mid[0], lo[0]);
      ft_split3_pair(pp[2], pp[3], hi[1], mid[1], lo[1]);
      {  // forward operand: B(k, n) = W[n][k], pairs along k: two adjacent dwords
        const int64_t blk = (int64_t)(k >> 4) * (N.pl_rows / 32) + (n >> 5);
        const int l = (n & 31) + 32 * ((k >> 3) & 1);
        uint32_t* o = N.pl_fwd + (blk * 64 + l) * 4 + ((k & 7) >> 1);
        *reinterpret_cast<uint2*>(o) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(o + total / 2) = make_uint2(mid[0], mid[1]);
        *reinterpret_cast<uint2*>(o + total) = make_uint2(lo[0], lo[1]);
      }
      {  // data-gradient operand: B(kk = n, nn = k): single bf16 values, 8 per fragment
        uint16_t* b16 = reinterpret_cast<uint16_t*>(N.pl_bwd);
        const uint32_t h4[4] = {hi[0] & 0xffffu, hi[0] >> 16, hi[1] & 0xffffu, hi[1] >> 16};
        const uint32_t m4[4] = {mid[0] & 0xffffu, mid[0] >> 16, mid[1] & 0xffffu,
                                mid[1] >> 16};
        const uint32_t l4[4] = {lo[0] & 0xffffu, lo[0] >> 16, lo[1] & 0xffffu, lo[1] >> 16};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int nn = k + j;
          const int64_t blk = (int64_t)(n >> 4) * (N.pl_cols / 32) + (nn >> 5);
          const int l = (nn & 31) + 32 * ((n >> 3) & 1);
          const int64_t o = (blk * 64 + l) * 8 + (n & 7);
          b16[o] = (uint16_t)h4[j];
          b16[total + o] = (uint16_t)m4[j];
          b16[2 * total + o] = (uint16_t)l4[j];
        }
      }
    }
  }
}

// developer hook (tools/): a register-only MFMA loop on `stream`, mode 1 =
// v_mfma_f32_32x32x16_bf16, 2 = v_mfma_f32_32x32x2_f32 -- a co-resident load with no
// memory traffic at all
__global__ __launch_bounds__(512, 4) void mfma_burn_kernel(int mode, int iters, float* sink) {
  f32x16 acc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  ft_bf16x8 a8, b8;
#pragma unroll
  for (int i = 0; i < 8; ++i) { a8[i] = (__bf16)(0.01f * (threadIdx.x + i)); b8[i] = (__bf16)(0.02f * i); }
  const float af = 0.01f * threadIdx.x, bf = 0.5f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (mode == 1)
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, b8, acc[c], 0, 0, 0);
      else
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc[c], 0, 0, 0);
    }
  }
  if (acc[0][0] + acc[1][0] == 12345.f) sink[0] = 1.f;
}

}  // namespace

// ---- the launch seam (fused_params.h).  The host side (fused_train_host.cpp) has checked
// the arguments, filled the parameter structs, chosen the variant and sized the grid;
// these functions do nothing but instantiate and launch.
#define FT_LAUNCH(threads, arg, ...) \
  hipExtLaunchKernelGGL((__VA_ARGS__), dim3(blocks), dim3(threads), 0, stream, e0, e1, 0, arg)

void ft_launch_fwd_loss(const FwdLossParams& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                        hipEvent_t e1, hipStream_t stream) {
  if (v.l1 && v.width == 64)
    FT_LAUNCH(256, p, fwd_head_loss_kernel<64, 2, 2, true>);
  else if (v.l1 && v.width == 128)
    FT_LAUNCH(256, p, fwd_head_loss_kernel<128, 1, 4, true>);
  else if (v.l1 && v.split)
    FT_LAUNCH(512, p, fwd_head_loss_split_kernel<256, 1, 8>);
  else if (v.l1 && v.ksc == 5)
    FT_LAUNCH(512, p, fwd_head_loss_kernel<256, 1, 8, true, 5>);
  else if (v.l1)
    FT_LAUNCH(512, p, fwd_head_loss_kernel<256, 1, 8, true>);
  else if (v.width == 64)
    FT_LAUNCH(256, p, fwd_head_loss_kernel<64, 2, 2>);
  else if (v.width == 128)
    FT_LAUNCH(256, p, fwd_head_loss_kernel<128, 1, 4>);
  else
    FT_LAUNCH(512, p, fwd_head_loss_kernel<256, 1, 8>);
}

void ft_launch_fwd_loss_pair(const FwdLossPair& pp, FtVariant v, unsigned blocks,
                             hipEvent_t e0, hipEvent_t e1, hipStream_t stream) {
  if (v.ksc == 5)
    FT_LAUNCH(512, pp, fwd_head_loss_pair_kernel<256, 1, 8, 5>);
  else
    FT_LAUNCH(512, pp, fwd_head_loss_pair_kernel<256, 1, 8, 0>);
}

void ft_launch_eval_forward(const FwdLossParams& p, FtVariant v, unsigned blocks,
                            hipEvent_t e0, hipEvent_t e1, hipStream_t stream) {
  if (v.width == 64)
    FT_LAUNCH(256, p, mlp_eval_forward_kernel<64, 2, 2>);
  else if (v.width == 128)
    FT_LAUNCH(256, p, mlp_eval_forward_kernel<128, 1, 4>);
  else if (v.split)
    FT_LAUNCH(512, p, mlp_eval_forward_split_kernel<256, 1, 8>);
  else if (v.ksc == 5)
    FT_LAUNCH(512, p, mlp_eval_forward_kernel<256, 1, 8, 5>);
  else
    FT_LAUNCH(512, p, mlp_eval_forward_kernel<256, 1, 8>);
}

void ft_launch_dgrad(const DgradWgrad0Params& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                     hipEvent_t e1, hipStream_t stream) {
  if (v.width == 64)
    FT_LAUNCH(256, p, dgrad_wgrad0_kernel<64, 2, 2>);
  else if (v.width == 128)
    FT_LAUNCH(256, p, dgrad_wgrad0_kernel<128, 1, 4>);
  else if (v.split)
    FT_LAUNCH(512, p, dgrad_wgrad0_split_kernel<256, 1, 8>);
  else
    FT_LAUNCH(512, p, dgrad_wgrad0_kernel<256, 1, 8>);
}

void ft_launch_dgrad_pair(const DgradWgrad0Pair& pp, FtVariant, unsigned blocks,
                          hipEvent_t e0, hipEvent_t e1, hipStream_t stream) {
  FT_LAUNCH(512, pp, dgrad_wgrad0_pair_kernel<256, 1, 8>);
}

void ft_launch_fwd_dgrad(const FwdDgradParams& pp, FtVariant v, unsigned blocks,
                         hipEvent_t e0, hipEvent_t e1, hipStream_t stream) {
  if (v.width == 64)
    FT_LAUNCH(256, pp, fwd_dgrad_kernel<64, 2, 2, 0>);
  else if (v.width == 128)
    FT_LAUNCH(256, pp, fwd_dgrad_kernel<128, 1, 4, 0>);
  else if (v.ksc == 5)
    FT_LAUNCH(512, pp, fwd_dgrad_kernel<256, 1, 8, 5>);
  else
    FT_LAUNCH(512, pp, fwd_dgrad_kernel<256, 1, 8, 0>);
}
#undef FT_LAUNCH

void ft_launch_reduce_regions(const ReduceRegionsParams& p, unsigned blocks,
                              hipStream_t stream) {
  hipLaunchKernelGGL(reduce_regions_adam_kernel, dim3(blocks), dim3(256), 0, stream, p);
}

void ft_launch_split_planes(bool bwd_only, unsigned blocks, const float* W, int64_t ld,
                            int rows, int cols, uint32_t* fwd, uint32_t* bwd,
                            hipStream_t stream) {
  if (bwd_only)
    hipLaunchKernelGGL(split_planes_kernel<true>, dim3(blocks), dim3(256), 0, stream, W, ld,
                       rows, cols, fwd, bwd);
  else
    hipLaunchKernelGGL(split_planes_kernel<false>, dim3(blocks), dim3(256), 0, stream, W,
                       ld, rows, cols, fwd, bwd);
}

void ft_launch_mfma_burn(int mode, int iters, int blocks, float* sink, hipStream_t stream) {
  hipLaunchKernelGGL(mfma_burn_kernel, dim3(blocks), dim3(512), 0, stream, mode, iters, sink);
}
