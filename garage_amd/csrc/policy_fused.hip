// Fused rollout step: MLP policy forward + action head in ONE launch.
//
// Replaces, per vectorised step of VecWorker.step_episode
// (sampler/vec_worker.py:176-204), the chain
//   StochasticPolicy.get_actions -> GaussianMLPModule.forward -> MLP layers ->
//   dist.sample()  (torch/policies/stochastic_policy.py:46-89,
//   torch/modules/gaussian_mlp_module.py:158-192, multi_headed_mlp_module.py:136-151)
// and the per-env appends of observations / actions / agent_info.
//
// One workgroup (4 waves) owns 16 envs for the whole network (n = 4096: 256
// workgroups, one per CU): the activations of those rows never leave the CU (two
// [16][H+4] fp32 tiles in LDS, ping / pong between layers), the weights stream from
// L2 through a double-buffered [N][32+4] LDS stage in 32-wide k chunks (16-B loads,
// branch free), hidden layers run on v_mfma_f32_16x16x4_f32 (wave w owns the
// 16-column tiles w, w + 4, ...; means agree with the per-layer path to rounding),
// the narrow output layer is a 16-lane VALU dot product, and the head (Gaussian:
// mean + std * noise; categorical: inverse CDF) writes the action and the rollout
// buffers.  Layer inputs up to 256 (C2, C3) run in policy_step_fused_kernel<WIDTH = 256>,
// up to 512 (C5) in its WIDTH = 512 instantiations; wider nets use the per-layer path.
// Every network option of ga_mlp_desc runs here: the tanh / linear-output network in
// the kernels it always had (GEN = false), any other hidden_act / output_act (0 .. 6)
// and layer_norm in a second set of instantiations (GEN = true) whose epilogues
// apply gemm_core.h's activations to the same sums and which normalise each hidden
// layer's input rows in LDS (ln_rows_w, lnorm.hip's formula).
// The parameters describe the network as NetDev and the head as HeadDev
// (rollout_params.h; filled by rollout_host.cpp), the struct the per-layer head kernel takes.
// With a device env (synthetic, PointEnv, GridWorldEnv, MultiEnvWrapper over PointEnv,
// CartPole, Pendulum, the inverted double pendulum, Acrobot, MountainCar: a template
// parameter of the kernel) the
// thread that sampled an env's action
// also steps it, and a whole rollout is ONE launch with the weights resident on the CU (see the kernel).
#include <type_traits>

#include "common.h"

#include "gemm_core.h"  // act_apply / act_forward_code: the per-layer epilogue's own
#include "rollout_dev.h"

// ---- Audit of out-of-range lanes / idle waves in the step kernel (one body for every
// WIDTH) and the training forward.  A hidden layer's weights are fetched per panel of
// up to 256 output columns: panel base W + n0 * ldw, rows = min(N - n0, 256) >= 1 rows
// of W left in it (n0 = 0 and rows = N at WIDTH = 256 and in the training forward).
// Clamped loads (value discarded by the matching store's mask): WeightStage::load --
// nrow = min(f >> 3, rows - 1), k = min(k0 + 4 (f & 7), last vector of the row); its
// store zeroes nrow >= rows and k >= K.
// Guarded loads: the register-resident second layer (ncol < N && k < K, a 16-B read
// at k <= ld - 4); biases (ncol < rows at bias[n0 + ncol]; resident: ncol <
// dims[l + 1], tid < dims[L]); the output layer's [N][ld] block (e < N * ld / 4 <=
// 32 * WIDTH / 4 vectors, inside the two contiguous stages of 4608 vectors; resident:
// <= 2048 vectors at stage 1, which holds 2304);
// observations (env < n && c < in_w); noise rows (per env < n); row vectors (output
// layer, ln_rows_w) at k < K <= WIDTH or vector 0; LayerNorm gamma / beta: the resident
// copy element by element (tid < dims[l], zero beyond), the streamed 16-B reads only
// where the vector's first column k < dims[l] -- it ends at k + 3 < round4(dims[l]),
// the length the layout gives gamma and beta each -- and never for a row index: all
// 16 rows of the tile exist in LDS (rows of envs >= n hold zeros and normalise to
// beta; they are never stored).
// Guarded stores: the epilogue's at n0 + ncol < n_pad <= WIDTH < the row stride.
// Nothing is fetched from an index derived from a wave number alone.
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (shape_rules.h states them once, for the host side too)
constexpr int ROWS = PS_ROWS;       // envs per workgroup (one 16 x 16 MFMA tile of rows)
constexpr int HMAX = PS_HMAX;       // output columns per panel; widest layer of the
                                    // WIDTH = 256 kernels and the training forward
constexpr int LDACT = HMAX + 4;     // the training forward's activation row stride (floats)
constexpr int KC = PS_KC;           // k chunk
constexpr int LDW = KC + 4;         // weight stage row stride
constexpr int MAX_OUT = PS_MAX_OUT; // widest output head
constexpr int WMAX = PS_WMAX;       // widest layer input of the WIDTH = 512 step kernels

// (tanh_fast: gemm_core.h)

// gemm_core.h's act_apply / act_apply_more (forward codes 0 .. 6), the same
// expressions, one activation per instantiation and force-inlined: a call to the
// noinline act_apply_more from the rollout kernel, whose lanes hold 256 weight
// registers, costs 96 - 144 B of scratch per lane for the saves around it.
template <int ACT>
__device__ __forceinline__ float act_fwd(float v) {
  if constexpr (ACT == 1) return tanh_fast(v);
  else if constexpr (ACT == 2) return fmaxf(v, 0.f);
  else if constexpr (ACT == 3) return 1.f / (1.f + expf(-v));
  else if constexpr (ACT == 4) return v > 0.f ? v : expm1f(v);
  else if constexpr (ACT == 5) return v > 0.f ? v : 0.01f * v;
  else if constexpr (ACT == 6) return v > 20.f ? v : log1pf(expf(v));
  else return v;
}
// f(integral_constant<forward code>) behind a wave-uniform switch
template <class F>
__device__ __forceinline__ void act_dispatch(int act, F&& f) {
  switch (act) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

// (NetDev, FusedParams<Env>, ENV_STEP_RESCALE, TrainFwdParams: rollout_params.h)

#define PS_STAMP(i) \
  if (p.dbg && blockIdx.x == 0 && threadIdx.x == 0 && sidx == p.n_steps / 2) \
    p.dbg[(i) + (RES ? 16 : 0)] = wall_clock64()

// Stage W[:, k0 : k0 + 32] of a [N][ldw] weight matrix (N <= HMAX rows: a panel):
// registers -> LDS, by a workgroup of NTHREADS.
template <int NTHREADS>
struct WeightStage {
  static constexpr int NV = HMAX * KC / 4 / NTHREADS;  // vectors per thread: 8 or 4
  float4 regs[NV];

  __device__ __forceinline__ void load(const float* __restrict__ W, int ldw, int N,
                                       int K, int k0) {
    const int last = max(((K + 3) & ~3) - 4, 0);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = threadIdx.x + NTHREADS * i;
      const int nrow = min(f >> 3, N - 1);
      const int k = min(k0 + 4 * (f & 7), last);
      regs[i] = *reinterpret_cast<const float4*>(W + (int64_t)nrow * ldw + k);
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ stage, int N, int K,
                                        int k0) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int f = threadIdx.x + NTHREADS * i;
      const int nrow = f >> 3;
      const int k = 4 * (f & 7);
      float4 v = regs[i];
      const bool ok = nrow < N;
      v.x = (ok && k0 + k + 0 < K) ? v.x : 0.f;
      v.y = (ok && k0 + k + 1 < K) ? v.y : 0.f;
      v.z = (ok && k0 + k + 2 < K) ? v.z : 0.f;
      v.w = (ok && k0 + k + 3 < K) ? v.w : 0.f;
      *reinterpret_cast<float4*>(stage + nrow * LDW + k) = v;
    }
  }
};

// Butterfly sum over 16 consecutive lanes (xor 1, 2, 4, 8) on DPP lane permutes:
// after the first two stages a quad holds one value, after the third a half row, so
// the mirrored (half) row supplies what lane ^ 4 / lane ^ 8 holds -- the same
// additions, in the same order, as four shuffles.
__device__ __forceinline__ float sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
           __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
           __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
           __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(
           __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
  return v;
}

// layer_normalization: LayerNorm of the 16 x D input tile of a hidden layer, in
// place in LDS, by lnorm.hip:ln_fwd_kernel's formula (two-pass mean and biased
// variance, eps 1e-5, y = (x - mean) * rstd * gamma + beta).  16 lanes per row, each
// lane the 16-B vectors at k = 4 part + 64 i; the columns D <= k < round4(D) stay 0
// (they are the layer's k padding).  gamma / beta: [round4(D)] floats each, in LDS
// (RES) or in the parameter buffer; a vector is read only where its first column
// k < D, and it ends inside the round4(D) floats the layout gives either row.
constexpr float LN_EPS = 1e-5f;
// (WIDTH: the step kernel's -- the widest row the tile holds, its row stride
// WIDTH + 4: 4 or 8 vectors per lane)
template <int WIDTH>
__device__ __forceinline__ void ln_rows_w(float* __restrict__ tile, int D,
                                          const float* __restrict__ gamma,
                                          const float* __restrict__ beta) {
  const int r = threadIdx.x >> 4, part = threadIdx.x & 15;
  float* a = tile + r * (WIDTH + 4);
  // (branch free, as the output layer reads its rows: out-of-range vectors read
  // vector 0 and are selected away; the row stays in registers for the three passes)
  float4 x[WIDTH / 64];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < WIDTH / 64; ++i) {
    const int k = part * 4 + 64 * i;
    float4 v = *reinterpret_cast<const float4*>(a + (k < D ? k : 0));
    v.x = k < D ? v.x : 0.f;
    v.y = k + 1 < D ? v.y : 0.f;
    v.z = k + 2 < D ? v.z : 0.f;
    v.w = k + 3 < D ? v.w : 0.f;
    x[i] = v;
    s += (v.x + v.y) + (v.z + v.w);
  }
  const float mean = sum16(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < WIDTH / 64; ++i) {
    const int k = part * 4 + 64 * i;
    const float d0 = k < D ? x[i].x - mean : 0.f;
    const float d1 = k + 1 < D ? x[i].y - mean : 0.f;
    const float d2 = k + 2 < D ? x[i].z - mean : 0.f;
    const float d3 = k + 3 < D ? x[i].w - mean : 0.f;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = 1.f / sqrtf(sum16(q) / (float)D + LN_EPS);
#pragma unroll
  for (int i = 0; i < WIDTH / 64; ++i) {
    const int k = part * 4 + 64 * i;
    if (k < D) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + k);
      const float4 b = *reinterpret_cast<const float4*>(beta + k);
      float4 y;
      y.x = (x[i].x - mean) * rstd * g.x + b.x;
      y.y = k + 1 < D ? (x[i].y - mean) * rstd * g.y + b.y : 0.f;
      y.z = k + 2 < D ? (x[i].z - mean) * rstd * g.z + b.z : 0.f;
      y.w = k + 3 < D ? (x[i].w - mean) * rstd * g.w + b.w : 0.f;
      *reinterpret_cast<float4*>(a + k) = y;
    }
  }
}
// (RES && GEN kernels only: a function-scope array, so that the LDS layout of every
// other instantiation is what it was)
__device__ __forceinline__ float* ln_resident_store() {
  __shared__ __attribute__((aligned(16))) float g[2][2][HMAX];
  return &g[0][0][0];
}

// The hidden layers run on v_mfma_f32_16x16x4_f32 (lane l: A[row l % 16][slot l / 16],
// B[slot l / 16][col l % 16], D[row 4 (l / 16) + reg][col l % 16]); wave w owns the
// 16-column tiles w, w + 4, w + 8, w + 12 of a layer's outputs.  Within a 16-deep
// group MFMA q gives slot kq the element k = 16 G + 4 kq + q, so A and B fragments
// are one 16-B read per lane and group.
constexpr int TPW = HMAX / 64;  // tiles per wave

// One 32-deep chunk with the B fragments in a staged [N][LDW] chunk.
//   A: act + (l % 16) * (WIDTH + 4) + 32 * chunk + 4 * (l / 16)
//   B: stage + (16 * wave + l % 16) * LDW + 4 * (l / 16)
template <int NT>
__device__ __forceinline__ void staged_chunk(const float* __restrict__ A,
                                             const float* __restrict__ B,
                                             f32x4 (&acc)[TPW]) {
#pragma unroll
  for (int G = 0; G < KC / 16; ++G) {
    const float4 av = *reinterpret_cast<const float4*>(A + 16 * G);
    const float a4[4] = {av.x, av.y, av.z, av.w};
    float b4[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float4 bv = *reinterpret_cast<const float4*>(B + 64 * t * LDW + 16 * G);
      b4[t][0] = bv.x; b4[t][1] = bv.y; b4[t][2] = bv.z; b4[t][3] = bv.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q], b4[t][q], acc[t], 0, 0, 0);
  }
}

// NG groups of 16 k of a hidden layer whose B operands sit in registers
// (wreg[t][4 G + q] = W[16 (wave + 4 t) + l % 16][16 G + 4 (l / 16) + q]).
template <int NG, int NT>
__device__ __forceinline__ void resident_layer(const float* __restrict__ A,
                                               const float (&wreg)[TPW][HMAX / 4],
                                               f32x4 (&acc)[TPW]) {
#pragma unroll
  for (int G = 0; G < NG; ++G) {
    const float4 av = *reinterpret_cast<const float4*>(A + 16 * G);
    const float a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q], wreg[t][4 * G + q], acc[t],
                                                      0, 0, 0);
  }
}
template <int NT>
__device__ __forceinline__ void resident_layer_k(const float* __restrict__ A, int K,
                                                 const float (&wreg)[TPW][HMAX / 4],
                                                 f32x4 (&acc)[TPW]) {
  // (straight-line per depth: a branch per k group would make the compiler move the
  // accumulators at every join; the tiles are zero beyond K)
  if (K <= 64) resident_layer<4, NT>(A, wreg, acc);
  else if (K <= 128) resident_layer<8, NT>(A, wreg, acc);
  else resident_layer<16, NT>(A, wreg, acc);
}

// The step kernel.  WIDTH is the widest layer input it takes and sizes the two
// activation tiles ([16][WIDTH + 4]) and the row registers of the output layer and
// the LayerNorm (WIDTH / 64 vectors per lane): HMAX = 256 (109 056 B of LDS) or
// WMAX = 512 (C5: MLP(512, 512, 512); 141 824 B, one workgroup per CU).  The weight
// stage is 2 x [HMAX][32 + 4] at either width: a layer's output columns come in
// panels of HMAX, per panel the k loop (32-wide chunks, ascending, one order per
// accumulator; wave w owns the panel's tiles w, w + 4, ...) and an epilogue that
// writes bias + activation into the other tile at the panel's column offset.  At
// WIDTH = HMAX a layer is one panel at offset 0 and the panel loop compiles away.
// The output layer's [N][ldw] block (up to 32 x 512 floats = 64 KB) goes to LDS across
// the two stages, which are contiguous; every wave is past a barrier behind its last
// stage read by then.
// RES (WIDTH = HMAX only: a 512 x 512 fp32 layer is 1 MB; a whole rollout in one
// launch, observations no wider than one k chunk, one or two hidden layers): the
// weights stay on the CU for all the steps -- the first layer's chunk in stage 0, the
// output layer's rows in stage 1, and the second hidden layer's [N][K] matrix in
// REGISTERS (each lane holds the 4 x 64 B operands its MFMAs consume: 256 of the 512
// registers a wave has at one wave per SIMD), so that layer runs without a barrier
// or a weight fetch.  Same k order per accumulator as the streamed loop:
// bit-identical.
// GEN = false is the tanh / linear-output / no-LayerNorm network.  GEN = true takes
// hidden_act, output_act and layer_norm from the descriptor, every branch on them
// wave-uniform: the epilogues apply gemm_core.h's activations to the same sums, and a
// LayerNorm (ln_rows_w) normalises each hidden layer's input tile in LDS first --
// gamma / beta resident on the CU next to obias in the RES variant.
template <int WIDTH, bool RES, class Env, bool GEN>
__global__ __launch_bounds__(256) void policy_step_fused_kernel(FusedParams<Env> p) {
  static_assert(WIDTH == HMAX || WIDTH == WMAX, "activation tile width");
  static_assert(!RES || WIDTH == HMAX, "resident weights: layer inputs up to HMAX");
  constexpr bool PANELS = WIDTH > HMAX;  // a layer's outputs can need a second panel
  constexpr int LDA = WIDTH + 4;       // activation tile row stride (floats)
  constexpr int STAGE = HMAX * LDW;
  __shared__ __attribute__((aligned(16))) float act[2][ROWS * LDA];
  __shared__ __attribute__((aligned(16))) float wst[2 * STAGE];
  __shared__ float head[ROWS][MAX_OUT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  const int L = p.net.n_layers;
  // This workgroup's parameter vector: member blockIdx.x / wg_per_member of a
  // population launch, p.params itself at member_stride 0.  The member's offset is
  // computed once (wave-uniform, one SGPR); every read of a parameter goes through
  // params(), which adds it to p.params behind an empty asm.  Without that the compiler
  // hoists a 64-bit base, and addresses derived from it, out of the step loop into
  // SGPRs the streamed kernels do not have (106 in use, hundreds of lane spills): that
  // form measured 0.9 % below the parent at (512, 512, 512), this one 3 % above
  // (DESIGN.md section 7).
  const int member_off =
      (int)(blockIdx.x / (unsigned)p.wg_per_member) * p.member_stride;
  auto params = [&]() -> const float* {
    int off = member_off;
    asm volatile("" : "+s"(off));
    return p.params + off;
  };
  // The action rescale's bounds, scale and scratch rows wait in LDS, and its branch
  // reads a bit of env_step, which every step reads anyway: held in SGPRs across the
  // step loop (as a test of p.es.nm.act_low holds them) they are lane spills whose
  // reloads every rollout pays in every step, rescale or not.  Thread 0 writes them
  // and the env threads read them behind a step's barriers.
  __shared__ ga_rollout::NormParams rescale;
  if (tid == 0 && (p.env_step & ENV_STEP_RESCALE)) rescale = p.es.nm;
  float wreg[TPW][HMAX / 4];
  float bias_r[2][TPW];  // RES: hidden biases of this lane's columns
#pragma unroll
  for (int t = 0; t < TPW; ++t) bias_r[0][t] = bias_r[1][t] = 0.f;
  __shared__ float obias[MAX_OUT];
  if constexpr (RES) {
    for (int l = 0; l < L - 1; ++l)
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int ncol = 16 * (wave + 4 * t) + r16;
        const float b = ncol < p.net.dims[l + 1] ? params()[p.net.b_off[l] + ncol] : 0.f;
        if (l == 0) bias_r[0][t] = b;
        else bias_r[1][t] = b;
      }
    if (tid < p.net.dims[L]) obias[tid] = params()[p.net.b_off[L - 1] + tid];
    // (the register-resident layer multiplies whole tiles: no stale columns)
    for (int e = tid; e < ROWS * LDA; e += 256) act[0][e] = act[1][e] = 0.f;
    {
      const int K = p.net.dims[0], N = p.net.dims[1];
      WeightStage<256> ws;
      ws.load(params() + p.net.w_off[0], (K + 3) & ~3, N, K, 0);
      ws.store(wst, N, K, 0);
    }
    if (L == 3) {
      const int K = p.net.dims[1], N = p.net.dims[2];
      const int ldw = (K + 3) & ~3;
      const float* W = params() + p.net.w_off[1];
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int ncol = 16 * (wave + 4 * t) + r16;
#pragma unroll
        for (int G = 0; G < HMAX / 16; ++G) {
          const int k = 16 * G + 4 * kq;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ncol < N && k < K) {
            v = *reinterpret_cast<const float4*>(W + (int64_t)ncol * ldw + k);
            if (k + 1 >= K) v.y = 0.f;
            if (k + 2 >= K) v.z = 0.f;
            if (k + 3 >= K) v.w = 0.f;
          }
          wreg[t][4 * G + 0] = v.x; wreg[t][4 * G + 1] = v.y;
          wreg[t][4 * G + 2] = v.z; wreg[t][4 * G + 3] = v.w;
        }
      }
    }
    {
      const int K = p.net.dims[L - 1], N = p.net.dims[L];
      const int ldw = (K + 3) & ~3;
      const float* W = params() + p.net.w_off[L - 1];
      for (int e = tid; e < N * (ldw / 4); e += 256)
        reinterpret_cast<float4*>(wst + STAGE)[e] = reinterpret_cast<const float4*>(W)[e];
    }
    if constexpr (GEN) {
      // gamma / beta of the (at most two) normalised layer inputs: [l][2][HMAX]
      // (constant indices: a dynamically indexed ln_off[l] is fetched as a whole
      // 16-register tuple)
      if (p.layer_norm) {
        float* lnp = ln_resident_store();
        if (L >= 2) {
          const int D = p.net.dims[0], ldn = (D + 3) & ~3;
          const float* g = params() + p.ln_off[0];
          lnp[0 * HMAX + tid] = tid < D ? g[tid] : 0.f;
          lnp[1 * HMAX + tid] = tid < D ? g[ldn + tid] : 0.f;
        }
        if (L == 3) {
          const int D = p.net.dims[1], ldn = (D + 3) & ~3;
          const float* g = params() + p.ln_off[1];
          lnp[2 * HMAX + tid] = tid < D ? g[tid] : 0.f;
          lnp[3 * HMAX + tid] = tid < D ? g[ldn + tid] : 0.f;
        }
      }
    }
    __syncthreads();
  }
  for (int sidx = 0; sidx < p.n_steps; ++sidx) {
  // this step's column, Philox counter and observation buffers (they swap roles
  // every step)
  ga_rollout::HeadDev hd = p.hd;
  hd.col = p.hd.col + sidx;
  hd.step = p.hd.step + (uint32_t)sidx;
  const bool odd = sidx & 1;
  const float* obs = odd ? p.es.seen_next : p.hd.obs;
  ga_rollout::EnvStepArgsT<Env> es = p.es;
  if (p.env_step) {
    es.p.col = hd.col;
    es.seen_next = odd ? const_cast<float*>(p.hd.obs) : p.es.seen_next;
    es.p.next_obs = es.seen_next;
    if (p.es.raw_next != p.es.seen_next) {  // NormalizedEnv: the env's own rows
      es.raw_obs = odd ? p.es.raw_next : p.es.raw_obs;
      es.raw_next = odd ? const_cast<float*>(p.es.raw_obs) : p.es.raw_next;
    } else {
      es.raw_obs = obs;
      es.raw_next = es.seen_next;
    }
  }

  // ---- observations -> act[0] (zero padded to a multiple of the k chunk) and
  //      into the rollout buffer (the list append of vec_worker.py:188)
  PS_STAMP(0);
  const int in_w = p.net.dims[0];
  const int in_pad = (in_w + KC - 1) / KC * KC;
  for (int e = tid; e < ROWS * in_pad; e += 256) {
    const int r = e / in_pad, c = e % in_pad;
    const int64_t env = row0 + r;
    float v = 0.f;
    if (env < hd.n && c < in_w) {
      v = obs[env * hd.ldo + c];
      hd.obs_buf[(env * hd.Tcap + hd.col) * hd.ldo + c] = v;
    }
    act[0][r * LDA + c] = v;
  }
  // the env threads fetch what their env's step will read now, behind the network
  decltype(ga_rollout::env_prefetch(es, 0)) pre;
  if (p.env_step && tid < ROWS && row0 + tid < hd.n)
    pre = ga_rollout::env_prefetch(es, row0 + tid);
  __syncthreads();
  PS_STAMP(1);

  // ---- hidden layers on the matrix cores
  int cur = 0;
  for (int l = 0; l < L - 1; ++l) {
    const int K = p.net.dims[l], N = p.net.dims[l + 1];
    const int ldw = (K + 3) & ~3;
    const float* W = params() + p.net.w_off[l];
    const float* bias = params() + p.net.b_off[l];
    const int nk = (K + KC - 1) / KC;
    const int n_pad = (N + KC - 1) / KC * KC;
    if constexpr (GEN) {
      // LayerNorm of this layer's input rows, in place (obs_buf already holds the
      // raw observations); gamma / beta are [ldw] floats each
      if (p.layer_norm) {
        if constexpr (RES)
          ln_rows_w<WIDTH>(act[cur], K, ln_resident_store() + (2 * l) * HMAX,
                           ln_resident_store() + (2 * l + 1) * HMAX);
        else
          ln_rows_w<WIDTH>(act[cur], K, params() + p.ln_off[l],
                           params() + p.ln_off[l] + ldw);
        __syncthreads();
      }
    }
    const float* Arow = act[cur] + r16 * LDA + 4 * kq;
    float* out = act[cur ^ 1];
    // one panel of (up to) HMAX output columns at a time: a single pass at n0 = 0
    // unless PANELS
    for (int n0 = 0; n0 < (PANELS ? n_pad : 1); n0 += HMAX) {
      // the rows of W and the (padded) columns left in this panel: 1 <= rows, since
      // n_pad - N < KC and n0 is a multiple of HMAX
      const int rows = PANELS ? min(N - n0, HMAX) : N;
      const int cols = PANELS ? min(n_pad - n0, HMAX) : n_pad;
      // this wave's tiles: the panel's columns 16 (wave + 4 t); a narrow panel is one
      // tile per wave
      const bool wave_on = 16 * wave < cols;
      const bool one_tile = cols <= 64;
      f32x4 acc[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = 0.f;
      if constexpr (RES) {
        if (wave_on) {
          if (l == 0) {
            const float* B = wst + (16 * wave + r16) * LDW + 4 * kq;
            if (one_tile) staged_chunk<1>(Arow, B, acc);
            else staged_chunk<TPW>(Arow, B, acc);
          } else {
            if (one_tile) resident_layer_k<1>(Arow, K, wreg, acc);
            else resident_layer_k<TPW>(Arow, K, wreg, acc);
          }
        }
      } else {
        // streamed weights, double buffered (every wave is past the barrier behind
        // the previous panel's last chunk)
        const float* Wp = W + (int64_t)n0 * ldw;
        WeightStage<256> ws;
        ws.load(Wp, ldw, rows, K, 0);
        ws.store(wst, rows, K, 0);
        __syncthreads();
        for (int s = 0; s < nk; ++s) {
          const bool more = s + 1 < nk;
          if (more) ws.load(Wp, ldw, rows, K, (s + 1) * KC);
          if (wave_on) {
            const float* B = wst + (s & 1) * STAGE + (16 * wave + r16) * LDW + 4 * kq;
            if (one_tile) staged_chunk<1>(Arow + s * KC, B, acc);
            else staged_chunk<TPW>(Arow + s * KC, B, acc);
          }
          if (more) ws.store(wst + ((s + 1) & 1) * STAGE, rows, K, (s + 1) * KC);
          __syncthreads();
        }
      }
      // bias + activation -> the other tile at the panel's offset (zero padded to the
      // k chunk), one copy per activation behind a wave-uniform switch.  The columns
      // N <= n0 + ncol < n_pad are 0, not f(0): they are the next layer's k padding.
      auto epilogue = [&](auto code) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          if (t == 0 || !one_tile) {
            const int ncol = 16 * (wave + 4 * t) + r16;
            const float bv = RES ? (l == 0 ? bias_r[0][t] : bias_r[1][t])
                                 : (ncol < rows ? bias[n0 + ncol] : 0.f);
            // (straight-line: f of every element, then one guarded run of stores)
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float th = act_fwd<decltype(code)::value>(acc[t][r] + bv);
              v[r] = ncol < rows ? th : 0.f;
            }
            if (n0 + ncol < n_pad) {
#pragma unroll
              for (int r = 0; r < 4; ++r) out[(4 * kq + r) * LDA + n0 + ncol] = v[r];
            }
          }
        }
      };
      if (wave_on) {
        if constexpr (GEN) act_dispatch(act_forward_code(p.hidden_act), epilogue);
        else epilogue(std::integral_constant<int, 1>{});  // tanh
      }
    }  // panels
    (void)nk; (void)W;
    __syncthreads();
    cur ^= 1;
    PS_STAMP(2 + l);
  }

  // ---- narrow output layer: its [N][ldw] block goes to LDS once (N <= 32,
  //      ldw <= WIDTH: inside the two stages); 16 lanes per row hold their k slice of
  //      the row in registers and dot it with every output
  {
    const int K = p.net.dims[L - 1], N = p.net.dims[L];
    const int ldw = (K + 3) & ~3;
    const float* W = params() + p.net.w_off[L - 1];
    const float* bias = params() + p.net.b_off[L - 1];
    float* wo = wst + (RES ? STAGE : 0);
    if constexpr (!RES)
      for (int e = tid; e < N * (ldw / 4); e += 256)
        reinterpret_cast<float4*>(wo)[e] = reinterpret_cast<const float4*>(W)[e];
    const int r = tid >> 4, part = tid & 15;
    const float* a = act[cur] + r * LDA;
    // (branch free: out-of-range slices read slice 0 and are selected away, so the
    // LDS reads of a row go out together instead of one latency after another)
    float4 xr[WIDTH / 64];
#pragma unroll
    for (int i = 0; i < WIDTH / 64; ++i) {
      const int k = part * 4 + 64 * i;
      float4 v = *reinterpret_cast<const float4*>(a + (k < K ? k : 0));
      v.x = k < K ? v.x : 0.f;
      v.y = k + 1 < K ? v.y : 0.f;
      v.z = k + 2 < K ? v.z : 0.f;
      v.w = k + 3 < K ? v.w : 0.f;
      xr[i] = v;
    }
    __syncthreads();
    for (int o = 0; o < N; ++o) {
      const float* w = wo + o * ldw + part * 4;
      float4 wv[WIDTH / 64];
#pragma unroll
      for (int i = 0; i < WIDTH / 64; ++i)
        wv[i] = *reinterpret_cast<const float4*>(
            w + (part * 4 + 64 * i < ldw ? 64 * i : 0));
      float sum = 0.f;
#pragma unroll
      for (int i = 0; i < WIDTH / 64; ++i) {
        const float t = sum + (xr[i].x * wv[i].x + xr[i].y * wv[i].y +
                               xr[i].z * wv[i].z + xr[i].w * wv[i].w);
        sum = part * 4 + 64 * i < ldw ? t : sum;
      }
      sum = sum16(sum);
      if (part == 0) {
        const float z = sum + (RES ? obias[o] : bias[o]);
        if constexpr (GEN)
          act_dispatch(p.output_act, [&](auto code) {
            head[r][o] = act_fwd<decltype(code)::value>(z);
          });
        else
          head[r][o] = z;
      }
    }
  }
  __syncthreads();
  PS_STAMP(10);

  // ---- action head and env step: one thread per env (rollout_dev.h's head_one at this
  //      sub-step's column and Philox step; the env steps from the action row it wrote)
  int ended_len = 0;
  if (tid < ROWS) {
    const int64_t env = row0 + tid;
    if (env < hd.n) {
      ga_rollout::head_one(hd, head[tid], p.net.dims[L], params(), env);
      if (p.env_step) {
        const float* act_row = hd.action + env * hd.lda;
        // NormalizedEnv.step (normalized_env.py:90-114): the wrapped env steps on the
        // rescaled, clipped row, written to the scratch as the rescale launch writes
        // it; the action buffer and act_buf keep the policy's own.  (Through memory:
        // a register row indexed by j would spill for A up to MAX_OUT.)
        if (p.env_step & ENV_STEP_RESCALE) {
          float* scaled = rescale.scaled_action + env * rescale.scaled_ld;
          ga_rollout::action_rescale_row(act_row, rescale.act_low, rescale.act_high,
                                         rescale.expected_action_scale, p.net.dims[L],
                                         scaled);
          act_row = scaled;
        }
        ended_len = ga_rollout::env_step_one(es, env, pre, act_row);
      }
    }
  }
  // (episode counts of the step: a wave-aggregated integer atomic; the envs of a
  // workgroup all sit in wave 0)
  if (p.env_step && wave == 0) ga_rollout::record_counts(es.p, ended_len);
  PS_STAMP(11);
  // the next step reads what the env threads just wrote (same workgroup: one CU,
  // one L1) and reuses the LDS tiles
  if (sidx + 1 < p.n_steps) __syncthreads();
  }  // steps
}

// ---- the same network, training forward ---------------------------------------
// All layers of one minibatch forward in one launch: 8 waves own 32 (gathered)
// rows; hidden activations go to LDS for the next layer AND to HBM for the
// backward pass; the narrow output layer is a 16-lane VALU dot.  Replaces the
// three per-layer GEMM launches of ga_mlp_forward_f32 (the activations' HBM
// read between layers disappears, the weights come from L2).
constexpr int TROWS = PS_TRAIN_ROWS;  // rows per workgroup of the training forward

__global__ __launch_bounds__(512) void mlp_train_fwd_fused_kernel(TrainFwdParams p) {
  // 64 rows x 8 waves: wave (ri, cj) owns rows [32 ri, 32 ri + 32) and columns
  // [64 cj, 64 cj + 64).  One activation tile, updated IN PLACE: a layer's
  // outputs wait in the accumulators until every wave has finished reading the
  // inputs, so LDS holds 64 rows (66.5 KB) + two weight stages (74 KB) and each
  // weight chunk fetched from L2 is amortised over 64 rows (32 MFMAs per wave per
  // chunk = ~1.7 us per SIMD, enough to cover the fetch of the next chunk).
  constexpr int NT = 512;
  __shared__ __attribute__((aligned(16))) float act[TROWS * LDACT];
  __shared__ __attribute__((aligned(16))) float wst[2][HMAX * LDW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int ri = wave >> 2, cj = wave & 3;
  const int64_t row0 = (int64_t)blockIdx.x * TROWS;
  const int L = p.net.n_layers;

  const int in_w = p.net.dims[0];
  const int in_pad = (in_w + KC - 1) / KC * KC;
  for (int e = tid; e < TROWS * in_pad; e += NT) {
    const int r = e / in_pad, c = e % in_pad;
    const int64_t m = row0 + r;
    float v = 0.f;
    if (m < p.M && c < in_w) {
      const int64_t src = p.idx ? (int64_t)p.idx[m] : m;
      v = p.X[src * p.ldx + c];
    }
    act[r * LDACT + c] = v;
  }
  __syncthreads();

  for (int l = 0; l < L - 1; ++l) {
    const int K = p.net.dims[l], N = p.net.dims[l + 1];
    const int ldw = (K + 3) & ~3;
    const int ldh = (N + 3) & ~3;
    const float* W = p.params + p.net.w_off[l];
    const float* bias = p.params + p.net.b_off[l];
    float* gact = p.acts + p.act_off[l];
    const int nk = (K + KC - 1) / KC;
    const int n0 = cj * 64;
    const bool wave_on = n0 < N;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    WeightStage<NT> ws;  // 256 x 32 floats = 2048 vectors, 4 per thread
    ws.load(W, ldw, N, K, 0);
    ws.store(wst[0], N, K, 0);
    __syncthreads();
    for (int s = 0; s < nk; ++s) {
      const bool more = s + 1 < nk;
      if (more) ws.load(W, ldw, N, K, (s + 1) * KC);
      if (wave_on) {
        const float* A = act + (32 * ri + l31) * LDACT + s * KC;
        const float* B = wst[s & 1] + (n0 + l31) * LDW;
#pragma unroll
        for (int g = 0; g < KC / 8; ++g) {
          const float4 av = *reinterpret_cast<const float4*>(A + 8 * g + 4 * half);
          const float4 b0 = *reinterpret_cast<const float4*>(B + 8 * g + 4 * half);
          const float4 b1 =
              *reinterpret_cast<const float4*>(B + 32 * LDW + 8 * g + 4 * half);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc[1], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc[1], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b0.z, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b1.z, acc[1], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b0.w, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b1.w, acc[1], 0, 0, 0);
        }
      }
      if (more) ws.store(wst[(s + 1) & 1], N, K, (s + 1) * KC);
      __syncthreads();
    }
    // every wave is past its last read of `act`: overwrite it with this layer
    const int n_pad = (N + KC - 1) / KC * KC;
    if (wave_on) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ncol = n0 + 32 * j + l31;
        const float bv = ncol < N ? bias[ncol] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = 32 * ri + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float v = ncol < N ? tanh_fast(acc[j][r] + bv) : 0.f;
          if (ncol < n_pad) act[m * LDACT + ncol] = v;
          if (ncol < N && row0 + m < p.M) gact[(row0 + m) * ldh + ncol] = v;
        }
      }
    }
    __syncthreads();
  }

  // narrow output layer: its weights go to LDS once, then 8 lanes per row
  {
    const int K = p.net.dims[L - 1], N = p.net.dims[L];
    const int ldw = (K + 3) & ~3;
    const float* W = p.params + p.net.w_off[L - 1];
    const float* bias = p.params + p.net.b_off[L - 1];
    float* wo = wst[0];  // [N][ldw] fits: N <= 32, ldw <= 256
    for (int e = tid; e < N * (ldw / 4); e += NT)
      reinterpret_cast<float4*>(wo)[e] = reinterpret_cast<const float4*>(W)[e];
    __syncthreads();
    const int r = tid >> 3, part = tid & 7;
    const float* a = act + r * LDACT;
    for (int o = 0; o < N; ++o) {
      const float* w = wo + o * ldw;
      float sum = 0.f;
      for (int k = part * 4; k < K; k += 32) {
        const float4 wv = *reinterpret_cast<const float4*>(w + k);
        const float4 xv = *reinterpret_cast<const float4*>(a + k);
        sum += xv.x * wv.x;
        if (k + 1 < K) sum += xv.y * wv.y;
        if (k + 2 < K) sum += xv.z * wv.z;
        if (k + 3 < K) sum += xv.w * wv.w;
      }
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 4, 64);
      if (part == 0 && row0 + r < p.M) p.out[(row0 + r) * p.ldo + o] = sum + bias[o];
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// The launch seam (rollout_params.h): instantiate and launch, nothing else.  The
// checks, the parameters, the choice of the variant and the grid are rollout_host.cpp's.
// ---------------------------------------------------------------------------
template <int WIDTH, bool RES, class Env>
static void step_kernel_launch(bool general, dim3 grid, hipStream_t stream,
                               const FusedParams<Env>& p) {
  if (general)
    hipLaunchKernelGGL((policy_step_fused_kernel<WIDTH, RES, Env, true>), grid, dim3(256),
                       0, stream, p);
  else
    hipLaunchKernelGGL((policy_step_fused_kernel<WIDTH, RES, Env, false>), grid, dim3(256),
                       0, stream, p);
}

template <class Env>
void ps_launch_policy_step(const FusedParams<Env>& p, PsVariant v, unsigned blocks,
                           hipStream_t stream) {
  const dim3 grid(blocks);
  if (v.width == WMAX) step_kernel_launch<WMAX, false>(v.general, grid, stream, p);
  else if (v.resident) step_kernel_launch<HMAX, true>(v.general, grid, stream, p);
  else step_kernel_launch<HMAX, false>(v.general, grid, stream, p);
}
#define GA_POLICY_STEP_OF(GaEnv, ...)                                                    \
  template void ps_launch_policy_step(const FusedParams<ga_env_dev_t<GaEnv>>&, PsVariant, \
                                      unsigned, hipStream_t);
GA_ENV_KINDS(GA_POLICY_STEP_OF)
#undef GA_POLICY_STEP_OF

void ps_launch_train_forward(const TrainFwdParams& p, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL(mlp_train_fwd_fused_kernel, dim3(blocks), dim3(512), 0, stream, p);
}

// (internal.h: what ga_rollout_env_steps asks before it sends a rescaled rollout to
// ga_policy_env_step_fused_f32.  A link-time answer: the loop's harness fakes it.)
extern "C" int ga_policy_env_step_rescales(void) { return 1; }
