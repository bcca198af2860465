// The natural-gradient (TRPO) step of a POPULATION of narrow networks (gfx950): every
// pass over a member's whole batch -- the surrogate's gradient, a Fisher-vector product
// A v = J^T M J v + reg v, a line-search candidate's loss and KL -- is ONE launch for all
// members, and the conjugate-gradient state lives on the device.
//   narrow_natural_members_kernel<H, NS_LDX, MODE>
//       grid (NG_SHARES, n_members).  A workgroup stages its member's weights (and, for a
//       product, the tangent v in the same flat layout) into LDS ONCE and then walks a
//       contiguous run of 64-row tiles: forward, tangent forward, metric seed, backward,
//       with no activation, tangent or seed ever leaving LDS.  The gradient shares stay
//       in registers across the tiles (dW2 in the MFMA accumulators, one 32 x 32 tile a
//       wave at most; dW1, dW_head and the biases in per-thread fp32 registers) and are
//       written once, when the run is finished: at most NG_SHARES shares per member
//       whatever its row count.  The run of a workgroup is a function of the member's row
//       count alone, so a member gets the same bits whatever the population around it.
//   narrow_natural_wide_kernel<H, NS_LDX, MODE>   the same pass at 33 .. 128 inputs
//       (NS_LDX = 68, 132): the same grid, run and shares on 32-row tiles, with the
//       tangent's accumulations on waves of their own and dW1 in MFMA accumulators (its
//       layout is stated above it).
//   members_cg_kernel   one workgroup per member: sums the member's shares in share order
//       and advances its conjugate-gradient recurrence (dots in fp64, fixed order; the
//       scalars stay on the device), or finishes the step direction and its length.
//   members_eval_finish_kernel / members_candidate_kernel   a candidate's loss and KL
//       from its workgroups' sums; `prev` back into a rejected member.
// Bounds: every global load sits behind its own test (rows under m0 + r < S, observation
// quads under 4 q < ld0, weights by loops over the layer's own sizes), rows past S
// contribute exact zeros (their seed is zero), workgroups past a member's share count and
// the workgroups of a finished or settled member return before touching memory.
#include "common.h"

#include "prof.h"

#include "fused_train.h"
#include "loss_rows.h"
#include "members_natural.h"
#include "narrow_body.h"

namespace {

struct NaturalParams {
  GaNaturalShared sh;
  const GaNaturalDev* table;
};

// LDS of a workgroup, in floats.  The forward / backward tiles of the narrow step with
// the first layer's weights in a buffer of their own (they are read for every tile),
// then what a product adds: the tangent's three weight blocks and biases, T2 and the
// head's tangent.  T1 lives in the dZ2 buffer: it is dead after T2's pre-activation and
// dZ2 is written in the backward phases.
template <int H, int NS_LDX, int MODE>
struct NaturalLds {
  static constexpr int LDH = H + 4;
  static constexpr int TILE = NS_ROWS * LDH;
  static constexpr int XS = 0;
  static constexpr int W1 = XS + NS_ROWS * NS_LDX;
  static constexpr int W2 = W1 + H * NS_LDX;
  static constexpr int WH = W2 + H * LDH;
  static constexpr int H1 = WH + NS_HN * H;
  static constexpr int H2 = H1 + TILE;    // later dZ1
  static constexpr int DZ2 = H2 + TILE;   // MODE_FVP: T1 until P2 is done
  static constexpr int OUT = DZ2 + TILE;
  static constexpr int DOUT = OUT + NS_ROWS * NS_HN;
  static constexpr int BIAS = DOUT + NS_ROWS * NS_HN;  // b1 [H], b2 [H], b_head [8]
  static constexpr int BASE_END = BIAS + 2 * H + NS_HN;
  static constexpr int V1 = BASE_END;
  static constexpr int V2 = V1 + H * NS_LDX;
  static constexpr int VH = V2 + H * LDH;
  static constexpr int T2 = VH + NS_HN * H;
  static constexpr int TOUT = T2 + TILE;
  static constexpr int VBIAS = TOUT + NS_ROWS * NS_HN;
  static constexpr int FVP_END = VBIAS + 2 * H + NS_HN;
  static constexpr int TOTAL = MODE == NG_MODE_FVP ? FVP_END : BASE_END;
  static_assert(TOTAL * 4 <= 160 * 1024, "a workgroup's tiles must fit the CU's 160 KB of LDS");
  static_assert(W1 % 4 == 0 && W2 % 4 == 0 && WH % 4 == 0 && H1 % 4 == 0 && H2 % 4 == 0 &&
                    DZ2 % 4 == 0 && OUT % 4 == 0 && DOUT % 4 == 0 && BIAS % 4 == 0 &&
                    V1 % 4 == 0 && V2 % 4 == 0 && VH % 4 == 0 && T2 % 4 == 0 &&
                    TOUT % 4 == 0 && VBIAS % 4 == 0,
                "16-B LDS accesses");
};

// a line-search candidate's parameter: prev - ratio^k descent, one rounding per operation
// (what `prev - ratio * descent` gives in fp32 outside the kernel)
__device__ __forceinline__ float ng_compose(float prev, float neg_ratio, float descent) {
#pragma clang fp contract(off)
  const float t = neg_ratio * descent;
  return prev + t;
}

// Where a pass reads a member's parameters: the member's own, or (MODE_EVAL) the
// candidate composed from the saved parameters and the descent step.
template <int MODE>
struct NgSource {
  const float* a;
  const float* d;
  float neg_ratio;
  __device__ __forceinline__ float at(int64_t i) const {
    return MODE == NG_MODE_EVAL ? ng_compose(a[i], neg_ratio, d[i]) : a[i];
  }
  __device__ __forceinline__ float4 at4(int64_t i) const {
    float4 v = *reinterpret_cast<const float4*>(a + i);
    if (MODE == NG_MODE_EVAL) {
      const float4 s = *reinterpret_cast<const float4*>(d + i);
      v.x = ng_compose(v.x, neg_ratio, s.x); v.y = ng_compose(v.y, neg_ratio, s.y);
      v.z = ng_compose(v.z, neg_ratio, s.z); v.w = ng_compose(v.w, neg_ratio, s.w);
    }
    return v;
  }
};

// the tangent of a product: NaNs of the finished step direction count as zeros
// (torch.nan_to_num in ConjugateGradientOptimizer.step)
struct NgTangent {
  const float* v;
  bool scrub;
  __device__ __forceinline__ float fix(float x) const { return scrub && x != x ? 0.f : x; }
  __device__ __forceinline__ float at(int64_t i) const { return fix(v[i]); }
  __device__ __forceinline__ float4 at4(int64_t i) const {
    float4 x = *reinterpret_cast<const float4*>(v + i);
    x.x = fix(x.x); x.y = fix(x.y); x.z = fix(x.z); x.w = fix(x.w);
    return x;
  }
};

// the three weight blocks and biases of a flat vector -> LDS (zero padded)
template <int H, int NS_LDX, class Src>
__device__ __forceinline__ void ng_stage(const Src& src, const GaNaturalShared& sh, float* w1,
                                         float* w2, float* wh, float* bias) {
  constexpr int LDH = H + 4;
  const int tid = threadIdx.x;
  const int ld0 = (sh.in_w + 3) & ~3, A = sh.out_w;
  for (int e = tid; e < H * (NS_LDX / 4); e += NS_THREADS) {
    const int n = e / (NS_LDX / 4), q = e % (NS_LDX / 4);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * q < ld0) w = src.at4(sh.w_off[0] + (int64_t)n * ld0 + 4 * q);
    *reinterpret_cast<float4*>(w1 + n * NS_LDX + 4 * q) = w;
  }
  for (int e = tid; e < H * (H / 4); e += NS_THREADS) {
    const int n = e / (H / 4), q = e % (H / 4);
    *reinterpret_cast<float4*>(w2 + n * LDH + 4 * q) =
        src.at4(sh.w_off[1] + (int64_t)n * H + 4 * q);
  }
  for (int e = tid; e < NS_HN * (H / 4); e += NS_THREADS) {
    const int j = e / (H / 4), q = e % (H / 4);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < A) w = src.at4(sh.w_off[2] + (int64_t)j * H + 4 * q);
    *reinterpret_cast<float4*>(wh + j * H + 4 * q) = w;
  }
  if (tid < H) {
    bias[tid] = src.at(sh.b_off[0] + tid);
    bias[H + tid] = src.at(sh.b_off[1] + tid);
  }
  if (tid < NS_HN) bias[2 * H + tid] = tid < A ? src.at(sh.b_off[2] + tid) : 0.f;
}

template <int H, int NS_LDX, int MODE>
__global__ __launch_bounds__(NS_THREADS, 1) void narrow_natural_members_kernel(
    NaturalParams q) {
  typedef NaturalLds<H, NS_LDX, MODE> Lds;
  constexpr int LDH = Lds::LDH;
  constexpr int CT = H / 32;   // column tiles of a hidden layer
  constexpr int QW = H / 4;    // hidden columns per wave in P5
  constexpr bool FVP = MODE == NG_MODE_FVP, EVAL = MODE == NG_MODE_EVAL,
                 GRAD = MODE == NG_MODE_GRAD;
  __shared__ __attribute__((aligned(16))) float lds[Lds::TOTAL];

  const GaNaturalShared& sh = q.sh;
  const GaNaturalDev& m = q.table[blockIdx.y];
  const int S = m.S;
  const int tiles = (S + NS_ROWS - 1) / NS_ROWS;
  const int shares = tiles < NG_SHARES ? tiles : NG_SHARES;
  const int g = blockIdx.x;
  if (g >= shares) return;
  if (EVAL && m.state != NG_SEARCHING) return;
  if (FVP && sh.respect_done && m.scalars[NG_DONE] != 0.0) return;

  float* xs = lds + Lds::XS;
  float* w1s = lds + Lds::W1;
  float* w2s = lds + Lds::W2;
  float* whs = lds + Lds::WH;
  float* h1 = lds + Lds::H1;
  float* h2 = lds + Lds::H2;
  float* dz2 = lds + Lds::DZ2;
  float* outl = lds + Lds::OUT;
  float* doutl = lds + Lds::DOUT;
  float* b1s = lds + Lds::BIAS;
  float* b2s = b1s + H;
  float* bhs = b2s + H;
  // (only a product's instantiation has these)
  float* v1s = lds + (FVP ? Lds::V1 : 0);
  float* v2s = lds + (FVP ? Lds::V2 : 0);
  float* vhs = lds + (FVP ? Lds::VH : 0);
  float* t1 = dz2;
  float* t2 = lds + (FVP ? Lds::T2 : 0);
  float* toutl = lds + (FVP ? Lds::TOUT : 0);
  float* vb1s = lds + (FVP ? Lds::VBIAS : 0);
  float* vb2s = vb1s + H;
  float* vbhs = vb2s + H;

  const int tid = threadIdx.x;
  const int lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int in_w = sh.in_w, A = sh.out_w;
  const int ld0 = (in_w + 3) & ~3;
  const int K1 = (in_w + 7) & ~7;  // first-layer reduction length, zero padded

  // ---- once: the member's weights (and the tangent) -> LDS
  NgSource<MODE> src;
  src.a = EVAL ? m.vectors + NG_PREV * sh.vec_stride : m.params;
  src.d = m.vectors + NG_DESCENT * sh.vec_stride;
  src.neg_ratio = m.neg_ratio;
  ng_stage<H, NS_LDX>(src, sh, w1s, w2s, whs, b1s);
  if (FVP) {
    NgTangent tv;
    tv.v = sh.vec_sel >= 0 ? m.vectors + sh.vec_sel * sh.vec_stride : m.vec;
    tv.scrub = sh.vec_sel == NG_X;
    ng_stage<H, NS_LDX>(tv, sh, v1s, v2s, vhs, vb1s);
  }
  // a candidate's parameters go to the member's own vector too: its first workgroup
  // stores them (the others read `prev` and `descent` only)
  if (EVAL && g == 0)
    for (int64_t i = tid; i < sh.n_flat; i += NS_THREADS) m.params[i] = src.at(i);

  // the log-std and what the rows' arithmetic derives from it
  float s = 0.f, inv_var = 1.f, seed_scale = 0.f, var_ratio = 1.f, inv_std_new = 1.f;
  if (sh.kind == 0) {
    s = ga_log_std(src.at(0), sh.has_min, sh.min_log_std, sh.has_max, sh.max_log_std,
                   nullptr);
    inv_var = expf(-2.f * s);
    seed_scale = expf(-2.f * s) / (float)S;
    if (EVAL) {
      const float s_old = ga_log_std(src.a[0], sh.has_min, sh.min_log_std, sh.has_max,
                                     sh.max_log_std, nullptr);
      const float ratio = expf(s_old - s);
      var_ratio = ratio * ratio;
      inv_std_new = expf(-s);
    }
  }
  LossRowArgs L;
  L.kind = sh.kind; L.actions = m.actions; L.lda = m.lda; L.old_ll = m.old_ll;
  L.adv = m.adv; L.returns = nullptr; L.idx = nullptr; L.log_std = nullptr;
  L.has_min = sh.has_min; L.has_max = sh.has_max; L.min_log_std = sh.min_log_std;
  L.max_log_std = sh.max_log_std; L.A = A; L.algo = 2; L.clip = 0.f;
  L.ent = lr_ent(m.ent_coeff, sh.ent_flags);
  L.double_softmax = sh.double_softmax;
  L.invM = m.inv_S;

  // tile of this wave in the 2 x CT tilings below (H = 32: waves 2, 3 idle there)
  const int tri = wave & 1, tcj = wave >> 1;
  const bool tile_on = tcj < CT;

  // ---- the shares this workgroup carries across its tiles
  constexpr int GROUPS = NS_THREADS / H, JPG = NS_HN / GROUPS;
  constexpr int MAXQ = (NS_LDX - 4) / 4, QN = (MAXQ + GROUPS - 1) / GROUPS;
  ns_f32x16 gW2;
#pragma unroll
  for (int i = 0; i < 16; ++i) gW2[i] = 0.f;
  float4 gW1[QN];
#pragma unroll
  for (int i = 0; i < QN; ++i) gW1[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  float gWh[JPG];
#pragma unroll
  for (int i = 0; i < JPG; ++i) gWh[i] = 0.f;
  float gb1 = 0.f, gb2 = 0.f, gbh = 0.f;
  double sum0 = 0.0, sum1 = 0.0;  // wave 0: the rows' two batch sums

  const int t_begin = (int)(((int64_t)g * tiles) / shares);
  const int t_end = (int)(((int64_t)(g + 1) * tiles) / shares);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int m0 = tile * NS_ROWS;
    const bool live = m0 + lane < S;
    // ---- the sample of this lane's row (wave 0 computes the rows' loss arithmetic)
    float act[8];
    float adv = 0.f, old_ll = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) act[j] = 0.f;
    if (!FVP && wave == 0 && live) {
      const int64_t row = m0 + lane;
      adv = m.adv[row];
      old_ll = m.old_ll[row];
      const float* arow = m.actions + row * m.lda;
      if (sh.kind == 2) {
        act[0] = arow[0];
      } else {
        const float4 a0 = *reinterpret_cast<const float4*>(arow);
        act[0] = a0.x; act[1] = a0.y; act[2] = a0.z; act[3] = a0.w;
        if (A > 4) {
          const float4 a1 = *reinterpret_cast<const float4*>(arow + 4);
          act[4] = a1.x; act[5] = a1.y; act[6] = a1.z; act[7] = a1.w;
        }
      }
    }
    // ---- P0: the tile's observations (zero padded)
    for (int e = tid; e < NS_ROWS * (NS_LDX / 4); e += NS_THREADS) {
      const int rr = e / (NS_LDX / 4), qq = e % (NS_LDX / 4);
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + rr < S && 4 * qq < ld0) {
        x = *reinterpret_cast<const float4*>(m.X + (int64_t)(m0 + rr) * m.ldx + 4 * qq);
        x.x = (4 * qq + 0 < in_w) ? x.x : 0.f;
        x.y = (4 * qq + 1 < in_w) ? x.y : 0.f;
        x.z = (4 * qq + 2 < in_w) ? x.z : 0.f;
        x.w = (4 * qq + 3 < in_w) ? x.w : 0.f;
      }
      *reinterpret_cast<float4*>(xs + rr * NS_LDX + 4 * qq) = x;
    }
    __syncthreads();
    // ---- P1: H1 = tanh(X W1^T + b1), T1 = (X V1^T + vb1) (1 - H1^2)
    if (tile_on) {
      const float* xa = xs + 32 * tri * NS_LDX;
      const ns_f32x16 acc =
          ns_tile<true, true>(xa, NS_LDX, w1s + 32 * tcj * NS_LDX, NS_LDX, K1, lane);
      ns_f32x16 tacc = acc;
      if (FVP) tacc = ns_tile<true, true>(xa, NS_LDX, v1s + 32 * tcj * NS_LDX, NS_LDX, K1, lane);
      const int col = 32 * tcj + l31;
      const float b = b1s[col];
      const float vb = FVP ? vb1s[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * tri + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float h = ns_tanh(acc[r] + b);
        h1[row * LDH + col] = h;
        if (FVP) t1[row * LDH + col] = (tacc[r] + vb) * (1.f - h * h);
      }
    }
    __syncthreads();
    // ---- P2: H2 = tanh(H1 W2^T + b2), T2 = (T1 W2^T + H1 V2^T + vb2) (1 - H2^2)
    if (tile_on) {
      const float* ha = h1 + 32 * tri * LDH;
      const ns_f32x16 acc = ns_tile<true, true>(ha, LDH, w2s + 32 * tcj * LDH, LDH, H, lane);
      const int col = 32 * tcj + l31;
      const float b = b2s[col];
      if (FVP) {
        // two accumulations, summed in this order
        const ns_f32x16 ta =
            ns_tile<true, true>(t1 + 32 * tri * LDH, LDH, w2s + 32 * tcj * LDH, LDH, H, lane);
        const ns_f32x16 tb = ns_tile<true, true>(ha, LDH, v2s + 32 * tcj * LDH, LDH, H, lane);
        const float vb = vb2s[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * tri + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float h = ns_tanh(acc[r] + b);
          h2[row * LDH + col] = h;
          t2[row * LDH + col] = ((ta[r] + tb[r]) + vb) * (1.f - h * h);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * tri + (r & 3) + 8 * (r >> 2) + 4 * half;
          h2[row * LDH + col] = ns_tanh(acc[r] + b);
        }
      }
    }
    __syncthreads();  // (every read of T1 is done: its buffer is dZ2 from P5 on)
    // ---- P3: head outputs and their tangent on the vector lanes (lane = row, wave = a
    // pair of outputs): out = H2 Wh^T + bh, tout = T2 Wh^T + H2 Vh^T + vbh
    {
      const int j0 = 2 * wave;
      float o0 = bhs[j0], o1 = bhs[j0 + 1];
      float u0 = FVP ? vbhs[j0] : 0.f, u1 = FVP ? vbhs[j0 + 1] : 0.f;
#pragma unroll 4
      for (int k = 0; k < H; k += 4) {
        const float4 h = *reinterpret_cast<const float4*>(h2 + lane * LDH + k);
        const float4 wa = *reinterpret_cast<const float4*>(whs + j0 * H + k);
        const float4 wb = *reinterpret_cast<const float4*>(whs + (j0 + 1) * H + k);
        o0 = fmaf(h.x, wa.x, o0); o0 = fmaf(h.y, wa.y, o0);
        o0 = fmaf(h.z, wa.z, o0); o0 = fmaf(h.w, wa.w, o0);
        o1 = fmaf(h.x, wb.x, o1); o1 = fmaf(h.y, wb.y, o1);
        o1 = fmaf(h.z, wb.z, o1); o1 = fmaf(h.w, wb.w, o1);
        if (FVP) {
          const float4 t = *reinterpret_cast<const float4*>(t2 + lane * LDH + k);
          const float4 va = *reinterpret_cast<const float4*>(vhs + j0 * H + k);
          const float4 vb = *reinterpret_cast<const float4*>(vhs + (j0 + 1) * H + k);
          u0 = fmaf(t.x, wa.x, u0); u0 = fmaf(t.y, wa.y, u0);
          u0 = fmaf(t.z, wa.z, u0); u0 = fmaf(t.w, wa.w, u0);
          u0 = fmaf(h.x, va.x, u0); u0 = fmaf(h.y, va.y, u0);
          u0 = fmaf(h.z, va.z, u0); u0 = fmaf(h.w, va.w, u0);
          u1 = fmaf(t.x, wb.x, u1); u1 = fmaf(t.y, wb.y, u1);
          u1 = fmaf(t.z, wb.z, u1); u1 = fmaf(t.w, wb.w, u1);
          u1 = fmaf(h.x, vb.x, u1); u1 = fmaf(h.y, vb.y, u1);
          u1 = fmaf(h.z, vb.z, u1); u1 = fmaf(h.w, vb.w, u1);
        }
      }
      outl[lane * NS_HN + j0] = o0;
      outl[lane * NS_HN + j0 + 1] = o1;
      if (FVP) {
        toutl[lane * NS_HN + j0] = u0;
        toutl[lane * NS_HN + j0 + 1] = u1;
      }
    }
    __syncthreads();
    // ---- P4: the rows' loss arithmetic (wave 0, lane = row)
    if (wave == 0) {
      float out[8], dout[8];
      const float4 o0 = *reinterpret_cast<const float4*>(outl + lane * NS_HN);
      const float4 o1 = *reinterpret_cast<const float4*>(outl + lane * NS_HN + 4);
      out[0] = o0.x; out[1] = o0.y; out[2] = o0.z; out[3] = o0.w;
      out[4] = o1.x; out[5] = o1.y; out[6] = o1.z; out[7] = o1.w;
#pragma unroll
      for (int j = 0; j < 8; ++j) dout[j] = 0.f;
      if (FVP) {
        float tout[8];
        const float4 u0 = *reinterpret_cast<const float4*>(toutl + lane * NS_HN);
        const float4 u1 = *reinterpret_cast<const float4*>(toutl + lane * NS_HN + 4);
        tout[0] = u0.x; tout[1] = u0.y; tout[2] = u0.z; tout[3] = u0.w;
        tout[4] = u1.x; tout[5] = u1.y; tout[6] = u1.z; tout[7] = u1.w;
        if (sh.kind == 0)
          lr_fisher_seed_gauss_row(A, seed_scale, tout, dout);
        else
          lr_fisher_seed_cat_row(A, sh.double_softmax, m.inv_S, out, tout, dout);
      } else {
        double second = 0.0;
        double first = lr_row(L, s, inv_var, out, act, adv, old_ll, 0.f, dout, &second);
        if (GRAD && live) {
          // the head outputs of the step's starting point (the KL's "old" side)
          float* hrow = m.heads + (int64_t)(m0 + lane) * NS_HN;
          *reinterpret_cast<float4*>(hrow) = o0;
          *reinterpret_cast<float4*>(hrow + 4) = o1;
        }
        if (EVAL) {
          float kl = 0.f;
          if (live) {
            const float* hrow = m.heads + (int64_t)(m0 + lane) * NS_HN;
            const float4 p0 = *reinterpret_cast<const float4*>(hrow);
            const float4 p1 = *reinterpret_cast<const float4*>(hrow + 4);
            const float old[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            kl = sh.kind == 0 ? lr_kl_gauss_row(A, var_ratio, inv_std_new, old, out)
                              : lr_kl_cat_row(A, sh.double_softmax, old, out);
          }
          second = (double)kl;
        }
        if (live) {
          sum0 += first;
          sum1 += second;
        }
      }
      if (!live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dout[j] = 0.f;
      }
      if (!EVAL) {
        *reinterpret_cast<float4*>(doutl + lane * NS_HN) =
            make_float4(dout[0], dout[1], dout[2], dout[3]);
        *reinterpret_cast<float4*>(doutl + lane * NS_HN + 4) =
            make_float4(dout[4], dout[5], dout[6], dout[7]);
      }
    }
    if (EVAL) continue;  // (two barriers lie between this P4 and the next tile's P3)
    __syncthreads();
    // ---- P5: dZ2 = (dout W_head) (1 - H2^2)   (lane = row, wave = column quarter)
    {
      const float4 d0 = *reinterpret_cast<const float4*>(doutl + lane * NS_HN);
      const float4 d1 = *reinterpret_cast<const float4*>(doutl + lane * NS_HN + 4);
      const float dd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int i = 0; i < QW / 4; ++i) {
        const int c = wave * QW + 4 * i;
        const float4 h = *reinterpret_cast<const float4*>(h2 + lane * LDH + c);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < NS_HN; ++j) {
          const float4 w = *reinterpret_cast<const float4*>(whs + j * H + c);
          z.x = fmaf(dd[j], w.x, z.x); z.y = fmaf(dd[j], w.y, z.y);
          z.z = fmaf(dd[j], w.z, z.z); z.w = fmaf(dd[j], w.w, z.w);
        }
        z.x *= (1.f - h.x * h.x); z.y *= (1.f - h.y * h.y);
        z.z *= (1.f - h.z * h.z); z.w *= (1.f - h.w * h.w);
        *reinterpret_cast<float4*>(dz2 + lane * LDH + c) = z;
      }
    }
    // ---- P6: head weight / bias gradient, into this thread's registers
    {
      const int c = tid % H, j0 = (tid / H) * JPG;
      for (int r = 0; r < NS_ROWS; ++r) {
        const float h = h2[r * LDH + c];
#pragma unroll
        for (int jj = 0; jj < JPG; ++jj)
          gWh[jj] = fmaf(doutl[r * NS_HN + j0 + jj], h, gWh[jj]);
      }
      if (tid < NS_HN)
        for (int r = 0; r < NS_ROWS; ++r) gbh += doutl[r * NS_HN + tid];
    }
    __syncthreads();  // dz2 complete; every read of h2 done
    // ---- P7: dW2[n][k] += sum_r dZ2[r][n] H1[r][k]   (CT x CT tiles, one a wave at most)
    if (wave < CT * CT) {
      const int tn = wave / CT, tk = wave % CT;
      const ns_f32x16 acc =
          ns_tile<false, false>(dz2 + 32 * tn, LDH, h1 + 32 * tk, LDH, NS_ROWS, lane);
#pragma unroll
      for (int i = 0; i < 16; ++i) gW2[i] += acc[i];
    }
    // ---- P8: dZ1 = (dZ2 W2) (1 - H1^2) -> the h2 buffer
    if (tile_on) {
      const ns_f32x16 acc = ns_tile<true, false>(dz2 + 32 * tri * LDH, LDH, w2s + 32 * tcj,
                                                 LDH, H, lane);
      const int col = 32 * tcj + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * tri + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float h = h1[row * LDH + col];
        h2[row * LDH + col] = acc[r] * (1.f - h * h);
      }
    }
    // bias gradient of layer 2 (column sums of dZ2)
    if (tid >= NS_THREADS - H) {
      const int n = tid - (NS_THREADS - H);
      for (int r = 0; r < NS_ROWS; ++r) gb2 += dz2[r * LDH + n];
    }
    __syncthreads();
    // ---- P9: dW1[n][k] += sum_r dZ1[r][n] X[r][k], db1
    {
      const int n = tid % H, g0 = tid / H;
#pragma unroll
      for (int qi = 0; qi < QN; ++qi) {
        const int qq = g0 + qi * GROUPS;
        if (4 * qq < ld0) {
          float4 gg = gW1[qi];
          for (int r = 0; r < NS_ROWS; ++r) {
            const float d = h2[r * LDH + n];
            const float4 x = *reinterpret_cast<const float4*>(xs + r * NS_LDX + 4 * qq);
            gg.x = fmaf(d, x.x, gg.x); gg.y = fmaf(d, x.y, gg.y);
            gg.z = fmaf(d, x.z, gg.z); gg.w = fmaf(d, x.w, gg.w);
          }
          gW1[qi] = gg;
        }
      }
      if (tid >= NS_THREADS - H) {
        const int nn = tid - (NS_THREADS - H);
        for (int r = 0; r < NS_ROWS; ++r) gb1 += h2[r * LDH + nn];
      }
    }
    __syncthreads();  // xs, h1, h2 are free for the next tile
  }

  // ---- once: this workgroup's sums and its share
  if (!FVP && wave == 0) {
    sum0 = ga_wave_sum(sum0);
    sum1 = ga_wave_sum(sum1);
    if (lane == 0) {
      m.lpart[2 * g + 0] = sum0;
      m.lpart[2 * g + 1] = sum1;
    }
  }
  if (EVAL) return;
  float* part = m.part + (int64_t)g * sh.stride;
  float* pW1 = part;
  float* pb1 = pW1 + (int64_t)H * ld0;
  float* pW2 = pb1 + H;
  float* pb2 = pW2 + (int64_t)H * H;
  float* pWh = pb2 + H;
  float* pbh = pWh + NS_HN * H;
  {
    const int n = tid % H, g0 = tid / H;
#pragma unroll
    for (int qi = 0; qi < QN; ++qi) {
      const int qq = g0 + qi * GROUPS;
      if (4 * qq < ld0) *reinterpret_cast<float4*>(pW1 + (int64_t)n * ld0 + 4 * qq) = gW1[qi];
    }
    const int c = tid % H, j0 = (tid / H) * JPG;
#pragma unroll
    for (int jj = 0; jj < JPG; ++jj) pWh[(j0 + jj) * H + c] = gWh[jj];
    if (tid < NS_HN) pbh[tid] = gbh;
    if (tid >= NS_THREADS - H) {
      pb1[tid - (NS_THREADS - H)] = gb1;
      pb2[tid - (NS_THREADS - H)] = gb2;
    }
  }
  if (wave < CT * CT) {
    const int tn = wave / CT, tk = wave % CT;
    const int k = 32 * tk + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = 32 * tn + (r & 3) + 8 * (r >> 2) + 4 * half;
      pW2[n * H + k] = gW2[r];
    }
  }
}

// ---- the WIDE instantiations: NS_LDX = 68 and 132 (33 .. 64 and 65 .. 128 inputs) ----
// The kernel above does not stretch: a product at H = 64 would need 168 000 B of LDS at
// NS_LDX = 68 and 217 152 B at 132, and its per-thread dW1 shares 32 registers and 64 x 8
// LDS quads per tile and thread.  narrow_natural_wide_kernel keeps the contract (grid,
// staging once, one share per workgroup, a run that is a function of S alone: the same
// 64-row tiles, walked as two halves) with a layout of its own:
//  * 32-ROW tiles in every mode.  Resident: W1, W2, the head and the biases, and for a
//    product V1, V2, the tangent's head and biases.  Per tile: X [32][NS_LDX], H1, H2
//    (later dZ1), dZ2 (T1 until P2 is done) and for a product T2, each [32][H + 4], and
//    the head buffers [32][8].  NaturalWideLds states the sum: 162 368 B at most.
//  * 32 rows are ONE row block of the 32 x 32 MFMA tiles, so a hidden layer has H / 32
//    output tiles for four waves.  In P1 and P2 of a product waves 0, 1 take the primal
//    accumulations and waves 2, 3 the tangent's.  The tangent waves store the
//    pre-activation's tangent U (without the (1 - h^2) factor, whose h the other waves
//    are still computing); the factor is applied where U is read next, after the barrier:
//    in P2's A operand (ng_tile_tangent) for T1, in P3 for T2.
//  * dW1 [H][<= 128] is H / 32 x NS_LDX / 32 tiles of dZ1^T X on the matrix cores, kept
//    in MFMA accumulators across the run (at most two a wave) like dW2, and scattered
//    into the share's [H][round4(in_w)] once.  X is staged zero padded up to column
//    NS_LDX - 4, so the columns in_w .. round4(in_w) are exact zeros and no column past
//    them is stored.
constexpr int NW_ROWS = 32;

template <int H, int NS_LDX, int MODE>
struct NaturalWideLds {
  static constexpr int LDH = H + 4;
  static constexpr int TILE = NW_ROWS * LDH;
  static constexpr int HEAD = NW_ROWS * NS_HN;
  static constexpr int WEIGHTS = H * NS_LDX + H * LDH + NS_HN * H + 2 * H + NS_HN;
  static constexpr int W1 = 0;
  static constexpr int W2 = W1 + H * NS_LDX;
  static constexpr int WH = W2 + H * LDH;
  static constexpr int BIAS = WH + NS_HN * H;  // b1 [H], b2 [H], b_head [8]
  static constexpr int XS = W1 + WEIGHTS;
  static constexpr int H1 = XS + NW_ROWS * NS_LDX;
  static constexpr int H2 = H1 + TILE;    // later dZ1
  static constexpr int DZ2 = H2 + TILE;   // MODE_FVP: U1 until P2 is done
  static constexpr int OUT = DZ2 + TILE;
  static constexpr int DOUT = OUT + HEAD;
  static constexpr int BASE_END = DOUT + HEAD;
  static constexpr int V1 = BASE_END;     // the tangent in the weights' layout
  static constexpr int V2 = V1 + H * NS_LDX;
  static constexpr int VH = V2 + H * LDH;
  static constexpr int VBIAS = VH + NS_HN * H;
  static constexpr int T2 = V1 + WEIGHTS;
  static constexpr int TOUT = T2 + TILE;
  static constexpr int FVP_END = TOUT + HEAD;
  static constexpr int TOTAL = MODE == NG_MODE_FVP ? FVP_END : BASE_END;
  static_assert(NS_LDX % 32 == 4 && NS_LDX > NS_IN_OVERLAY + 4, "whole 32-column tiles + 4");
  static_assert(TOTAL * 4 <= 160 * 1024, "a workgroup's tiles must fit the CU's 160 KB of LDS");
  static_assert(WEIGHTS % 4 == 0 && TILE % 4 == 0 && (NW_ROWS * NS_LDX) % 4 == 0,
                "16-B LDS accesses");
};

// ns_tile<true, true> whose A operand is a tangent still without its tanh factor:
// A(i, k) = U[i * lda + k] (1 - Hh[i * lda + k]^2)
__device__ __forceinline__ ns_f32x16 ng_tile_tangent(const float* U, const float* Hh, int lda,
                                                     const float* B, int ldb, int K, int lane) {
  const int l31 = lane & 31, half = lane >> 5;
  ns_f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  for (int g = 0; g < K / 8; ++g) {
    const int k0 = 8 * g + 4 * half;
    const float4 u = *reinterpret_cast<const float4*>(U + l31 * lda + k0);
    const float4 h = *reinterpret_cast<const float4*>(Hh + l31 * lda + k0);
    const float4 b = *reinterpret_cast<const float4*>(B + l31 * ldb + k0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(u.x * (1.f - h.x * h.x), b.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(u.y * (1.f - h.y * h.y), b.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(u.z * (1.f - h.z * h.z), b.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(u.w * (1.f - h.w * h.w), b.w, acc1, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] += acc1[i];
  return acc0;
}

template <int H, int NS_LDX, int MODE>
__global__ __launch_bounds__(NS_THREADS, 1) void narrow_natural_wide_kernel(NaturalParams q) {
  typedef NaturalWideLds<H, NS_LDX, MODE> Lds;
  constexpr int LDH = Lds::LDH, ROWS = NW_ROWS;
  constexpr int CT = H / 32;                  // column tiles of a hidden layer
  constexpr int KTMAX = (NS_LDX - 4) / 32;    // 32-column tiles of the staged observations
  constexpr int NACC = (CT * KTMAX + 3) / 4;  // dW1 tiles a wave carries
  constexpr int QW = H / 8;                   // hidden columns per thread in P5
  constexpr bool FVP = MODE == NG_MODE_FVP, EVAL = MODE == NG_MODE_EVAL,
                 GRAD = MODE == NG_MODE_GRAD;
  __shared__ __attribute__((aligned(16))) float lds[Lds::TOTAL];

  const GaNaturalShared& sh = q.sh;
  const GaNaturalDev& m = q.table[blockIdx.y];
  const int S = m.S;
  const int tiles = (S + NS_ROWS - 1) / NS_ROWS;  // (the 64-row tiles of ga_natural_tiles)
  const int shares = tiles < NG_SHARES ? tiles : NG_SHARES;
  const int g = blockIdx.x;
  if (g >= shares) return;
  if (EVAL && m.state != NG_SEARCHING) return;
  if (FVP && sh.respect_done && m.scalars[NG_DONE] != 0.0) return;

  float* xs = lds + Lds::XS;
  float* w1s = lds + Lds::W1;
  float* w2s = lds + Lds::W2;
  float* whs = lds + Lds::WH;
  float* h1 = lds + Lds::H1;
  float* h2 = lds + Lds::H2;
  float* dz2 = lds + Lds::DZ2;
  float* outl = lds + Lds::OUT;
  float* doutl = lds + Lds::DOUT;
  float* b1s = lds + Lds::BIAS;
  float* b2s = b1s + H;
  float* bhs = b2s + H;
  // (only a product's instantiation has these)
  float* v1s = lds + (FVP ? Lds::V1 : 0);
  float* v2s = lds + (FVP ? Lds::V2 : 0);
  float* vhs = lds + (FVP ? Lds::VH : 0);
  float* u1 = dz2;
  float* u2 = lds + (FVP ? Lds::T2 : 0);
  float* toutl = lds + (FVP ? Lds::TOUT : 0);
  float* vb1s = lds + (FVP ? Lds::VBIAS : 0);
  float* vb2s = vb1s + H;
  float* vbhs = vb2s + H;

  const int tid = threadIdx.x;
  const int lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int in_w = sh.in_w, A = sh.out_w;
  const int ld0 = (in_w + 3) & ~3;
  const int K1 = (in_w + 7) & ~7;   // first-layer reduction length, zero padded
  const int KT = (ld0 + 31) >> 5;   // 32-column tiles of dW1 that hold a column < ld0

  // ---- once: the member's weights (and the tangent) -> LDS
  NgSource<MODE> src;
  src.a = EVAL ? m.vectors + NG_PREV * sh.vec_stride : m.params;
  src.d = m.vectors + NG_DESCENT * sh.vec_stride;
  src.neg_ratio = m.neg_ratio;
  ng_stage<H, NS_LDX>(src, sh, w1s, w2s, whs, b1s);
  if (FVP) {
    NgTangent tv;
    tv.v = sh.vec_sel >= 0 ? m.vectors + sh.vec_sel * sh.vec_stride : m.vec;
    tv.scrub = sh.vec_sel == NG_X;
    ng_stage<H, NS_LDX>(tv, sh, v1s, v2s, vhs, vb1s);
  }
  if (EVAL && g == 0)
    for (int64_t i = tid; i < sh.n_flat; i += NS_THREADS) m.params[i] = src.at(i);

  // the log-std and what the rows' arithmetic derives from it
  float s = 0.f, inv_var = 1.f, seed_scale = 0.f, var_ratio = 1.f, inv_std_new = 1.f;
  if (sh.kind == 0) {
    s = ga_log_std(src.at(0), sh.has_min, sh.min_log_std, sh.has_max, sh.max_log_std,
                   nullptr);
    inv_var = expf(-2.f * s);
    seed_scale = expf(-2.f * s) / (float)S;
    if (EVAL) {
      const float s_old = ga_log_std(src.a[0], sh.has_min, sh.min_log_std, sh.has_max,
                                     sh.max_log_std, nullptr);
      const float ratio = expf(s_old - s);
      var_ratio = ratio * ratio;
      inv_std_new = expf(-s);
    }
  }
  LossRowArgs L;
  L.kind = sh.kind; L.actions = m.actions; L.lda = m.lda; L.old_ll = m.old_ll;
  L.adv = m.adv; L.returns = nullptr; L.idx = nullptr; L.log_std = nullptr;
  L.has_min = sh.has_min; L.has_max = sh.has_max; L.min_log_std = sh.min_log_std;
  L.max_log_std = sh.max_log_std; L.A = A; L.algo = 2; L.clip = 0.f;
  L.ent = lr_ent(m.ent_coeff, sh.ent_flags);
  L.double_softmax = sh.double_softmax;
  L.invM = m.inv_S;

  // P1, P2: waves 0, 1 the primal column tiles, waves 2, 3 the tangent's
  const int tcj = wave & 1;
  const bool primal_on = wave < 2 && tcj < CT, tangent_on = FVP && wave >= 2 && tcj < CT;
  // the rows' arithmetic: the first 32 lanes of wave 0
  const bool rows_on = wave == 0 && lane < ROWS;

  // ---- the shares this workgroup carries across its tiles
  constexpr int GROUPS = NS_THREADS / H, JPG = NS_HN / GROUPS;
  ns_f32x16 gW2, gW1[NACC];
#pragma unroll
  for (int i = 0; i < 16; ++i) gW2[i] = 0.f;
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int i = 0; i < 16; ++i) gW1[a][i] = 0.f;
  float gWh[JPG];
#pragma unroll
  for (int i = 0; i < JPG; ++i) gWh[i] = 0.f;
  float gb1 = 0.f, gb2 = 0.f, gbh = 0.f;
  double sum0 = 0.0, sum1 = 0.0;  // wave 0: the rows' two batch sums

  // the rows of this workgroup's 64-row tiles, 32 at a time
  const int64_t t_begin = ((int64_t)g * tiles) / shares;
  const int64_t t_end = ((int64_t)(g + 1) * tiles) / shares;
  const int r_end = (int)(t_end * NS_ROWS < (int64_t)S ? t_end * NS_ROWS : (int64_t)S);
  for (int m0 = (int)(t_begin * NS_ROWS); m0 < r_end; m0 += ROWS) {
    const bool live = rows_on && m0 + lane < S;
    // ---- the sample of this lane's row
    float act[8];
    float adv = 0.f, old_ll = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) act[j] = 0.f;
    if (!FVP && live) {
      const int64_t row = m0 + lane;
      adv = m.adv[row];
      old_ll = m.old_ll[row];
      const float* arow = m.actions + row * m.lda;
      if (sh.kind == 2) {
        act[0] = arow[0];
      } else {
        const float4 a0 = *reinterpret_cast<const float4*>(arow);
        act[0] = a0.x; act[1] = a0.y; act[2] = a0.z; act[3] = a0.w;
        if (A > 4) {
          const float4 a1 = *reinterpret_cast<const float4*>(arow + 4);
          act[4] = a1.x; act[5] = a1.y; act[6] = a1.z; act[7] = a1.w;
        }
      }
    }
    // ---- P0: the tile's observations (zero padded)
    for (int e = tid; e < ROWS * (NS_LDX / 4); e += NS_THREADS) {
      const int rr = e / (NS_LDX / 4), qq = e % (NS_LDX / 4);
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + rr < S && 4 * qq < ld0) {
        x = *reinterpret_cast<const float4*>(m.X + (int64_t)(m0 + rr) * m.ldx + 4 * qq);
        x.x = (4 * qq + 0 < in_w) ? x.x : 0.f;
        x.y = (4 * qq + 1 < in_w) ? x.y : 0.f;
        x.z = (4 * qq + 2 < in_w) ? x.z : 0.f;
        x.w = (4 * qq + 3 < in_w) ? x.w : 0.f;
      }
      *reinterpret_cast<float4*>(xs + rr * NS_LDX + 4 * qq) = x;
    }
    __syncthreads();
    // ---- P1: H1 = tanh(X W1^T + b1) | U1 = X V1^T + vb1
    if (primal_on || tangent_on) {
      const ns_f32x16 acc = ns_tile<true, true>(
          xs, NS_LDX, (tangent_on ? v1s : w1s) + 32 * tcj * NS_LDX, NS_LDX, K1, lane);
      const int col = 32 * tcj + l31;
      const float b = tangent_on ? vb1s[col] : b1s[col];
      float* dst = tangent_on ? u1 : h1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        dst[row * LDH + col] = tangent_on ? acc[r] + b : ns_tanh(acc[r] + b);
      }
    }
    __syncthreads();
    // ---- P2: H2 = tanh(H1 W2^T + b2) | U2 = T1 W2^T + H1 V2^T + vb2, T1 = U1 (1 - H1^2)
    if (primal_on) {
      const ns_f32x16 acc = ns_tile<true, true>(h1, LDH, w2s + 32 * tcj * LDH, LDH, H, lane);
      const int col = 32 * tcj + l31;
      const float b = b2s[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        h2[row * LDH + col] = ns_tanh(acc[r] + b);
      }
    } else if (tangent_on) {
      // two accumulations, summed in this order
      const ns_f32x16 ta = ng_tile_tangent(u1, h1, LDH, w2s + 32 * tcj * LDH, LDH, H, lane);
      const ns_f32x16 tb = ns_tile<true, true>(h1, LDH, v2s + 32 * tcj * LDH, LDH, H, lane);
      const int col = 32 * tcj + l31;
      const float vb = vb2s[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        u2[row * LDH + col] = (ta[r] + tb[r]) + vb;
      }
    }
    __syncthreads();  // (every read of U1 is done: its buffer is dZ2 from P5 on)
    // ---- P3: head outputs and their tangent on the vector lanes (thread = row x output):
    // out = H2 Wh^T + bh, tout = T2 Wh^T + H2 Vh^T + vbh, T2 = U2 (1 - H2^2)
    {
      const int row = tid & 31, j = tid >> 5;
      float o = bhs[j];
      float u = FVP ? vbhs[j] : 0.f;
#pragma unroll 4
      for (int k = 0; k < H; k += 4) {
        const float4 h = *reinterpret_cast<const float4*>(h2 + row * LDH + k);
        const float4 w = *reinterpret_cast<const float4*>(whs + j * H + k);
        o = fmaf(h.x, w.x, o); o = fmaf(h.y, w.y, o);
        o = fmaf(h.z, w.z, o); o = fmaf(h.w, w.w, o);
        if (FVP) {
          float4 t = *reinterpret_cast<const float4*>(u2 + row * LDH + k);
          const float4 v = *reinterpret_cast<const float4*>(vhs + j * H + k);
          t.x *= (1.f - h.x * h.x); t.y *= (1.f - h.y * h.y);
          t.z *= (1.f - h.z * h.z); t.w *= (1.f - h.w * h.w);
          u = fmaf(t.x, w.x, u); u = fmaf(t.y, w.y, u);
          u = fmaf(t.z, w.z, u); u = fmaf(t.w, w.w, u);
          u = fmaf(h.x, v.x, u); u = fmaf(h.y, v.y, u);
          u = fmaf(h.z, v.z, u); u = fmaf(h.w, v.w, u);
        }
      }
      outl[row * NS_HN + j] = o;
      if (FVP) toutl[row * NS_HN + j] = u;
    }
    __syncthreads();
    // ---- P4: the rows' loss arithmetic (wave 0, lane = row)
    if (rows_on) {
      float out[8], dout[8];
      const float4 o0 = *reinterpret_cast<const float4*>(outl + lane * NS_HN);
      const float4 o1 = *reinterpret_cast<const float4*>(outl + lane * NS_HN + 4);
      out[0] = o0.x; out[1] = o0.y; out[2] = o0.z; out[3] = o0.w;
      out[4] = o1.x; out[5] = o1.y; out[6] = o1.z; out[7] = o1.w;
#pragma unroll
      for (int j = 0; j < 8; ++j) dout[j] = 0.f;
      if (FVP) {
        float tout[8];
        const float4 u0 = *reinterpret_cast<const float4*>(toutl + lane * NS_HN);
        const float4 u1q = *reinterpret_cast<const float4*>(toutl + lane * NS_HN + 4);
        tout[0] = u0.x; tout[1] = u0.y; tout[2] = u0.z; tout[3] = u0.w;
        tout[4] = u1q.x; tout[5] = u1q.y; tout[6] = u1q.z; tout[7] = u1q.w;
        if (sh.kind == 0)
          lr_fisher_seed_gauss_row(A, seed_scale, tout, dout);
        else
          lr_fisher_seed_cat_row(A, sh.double_softmax, m.inv_S, out, tout, dout);
      } else {
        double second = 0.0;
        double first = lr_row(L, s, inv_var, out, act, adv, old_ll, 0.f, dout, &second);
        if (GRAD && live) {
          // the head outputs of the step's starting point (the KL's "old" side)
          float* hrow = m.heads + (int64_t)(m0 + lane) * NS_HN;
          *reinterpret_cast<float4*>(hrow) = o0;
          *reinterpret_cast<float4*>(hrow + 4) = o1;
        }
        if (EVAL) {
          float kl = 0.f;
          if (live) {
            const float* hrow = m.heads + (int64_t)(m0 + lane) * NS_HN;
            const float4 p0 = *reinterpret_cast<const float4*>(hrow);
            const float4 p1 = *reinterpret_cast<const float4*>(hrow + 4);
            const float old[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            kl = sh.kind == 0 ? lr_kl_gauss_row(A, var_ratio, inv_std_new, old, out)
                              : lr_kl_cat_row(A, sh.double_softmax, old, out);
          }
          second = (double)kl;
        }
        if (live) {
          sum0 += first;
          sum1 += second;
        }
      }
      if (!live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dout[j] = 0.f;
      }
      if (!EVAL) {
        *reinterpret_cast<float4*>(doutl + lane * NS_HN) =
            make_float4(dout[0], dout[1], dout[2], dout[3]);
        *reinterpret_cast<float4*>(doutl + lane * NS_HN + 4) =
            make_float4(dout[4], dout[5], dout[6], dout[7]);
      }
    }
    if (EVAL) continue;  // (two barriers lie between this P4 and the next tile's P3)
    __syncthreads();
    // ---- P5: dZ2 = (dout W_head) (1 - H2^2)   (thread = row x an eighth of the columns)
    {
      const int row = tid & 31, c0 = (tid >> 5) * QW;
      const float4 d0 = *reinterpret_cast<const float4*>(doutl + row * NS_HN);
      const float4 d1 = *reinterpret_cast<const float4*>(doutl + row * NS_HN + 4);
      const float dd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
      for (int i = 0; i < QW / 4; ++i) {
        const int c = c0 + 4 * i;
        const float4 h = *reinterpret_cast<const float4*>(h2 + row * LDH + c);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < NS_HN; ++j) {
          const float4 w = *reinterpret_cast<const float4*>(whs + j * H + c);
          z.x = fmaf(dd[j], w.x, z.x); z.y = fmaf(dd[j], w.y, z.y);
          z.z = fmaf(dd[j], w.z, z.z); z.w = fmaf(dd[j], w.w, z.w);
        }
        z.x *= (1.f - h.x * h.x); z.y *= (1.f - h.y * h.y);
        z.z *= (1.f - h.z * h.z); z.w *= (1.f - h.w * h.w);
        *reinterpret_cast<float4*>(dz2 + row * LDH + c) = z;
      }
    }
    // ---- P6: head weight / bias gradient, into this thread's registers
    {
      const int c = tid % H, j0 = (tid / H) * JPG;
      for (int r = 0; r < ROWS; ++r) {
        const float h = h2[r * LDH + c];
#pragma unroll
        for (int jj = 0; jj < JPG; ++jj)
          gWh[jj] = fmaf(doutl[r * NS_HN + j0 + jj], h, gWh[jj]);
      }
      if (tid < NS_HN)
        for (int r = 0; r < ROWS; ++r) gbh += doutl[r * NS_HN + tid];
    }
    __syncthreads();  // dz2 complete; every read of h2 done
    // ---- P7: dW2[n][k] += sum_r dZ2[r][n] H1[r][k]   (CT x CT tiles, one a wave at most)
    if (wave < CT * CT) {
      const int tn = wave / CT, tk = wave % CT;
      const ns_f32x16 acc =
          ns_tile<false, false>(dz2 + 32 * tn, LDH, h1 + 32 * tk, LDH, ROWS, lane);
#pragma unroll
      for (int i = 0; i < 16; ++i) gW2[i] += acc[i];
    }
    // ---- P8: dZ1 = (dZ2 W2) (1 - H1^2) -> the h2 buffer   (wave = column tile)
    if (wave < CT) {
      const ns_f32x16 acc = ns_tile<true, false>(dz2, LDH, w2s + 32 * wave, LDH, H, lane);
      const int col = 32 * wave + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        const float h = h1[row * LDH + col];
        h2[row * LDH + col] = acc[r] * (1.f - h * h);
      }
    }
    // bias gradient of layer 2 (column sums of dZ2)
    if (tid >= NS_THREADS - H) {
      const int n = tid - (NS_THREADS - H);
      for (int r = 0; r < ROWS; ++r) gb2 += dz2[r * LDH + n];
    }
    __syncthreads();
    // ---- P9: dW1[n][k] += sum_r dZ1[r][n] X[r][k] (CT x KTMAX tiles, NACC a wave), db1
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
      const int t = wave + 4 * a, tn = t / KTMAX, tk = t % KTMAX;
      if (t < CT * KTMAX && tk < KT) {
        const ns_f32x16 acc =
            ns_tile<false, false>(h2 + 32 * tn, LDH, xs + 32 * tk, NS_LDX, ROWS, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) gW1[a][i] += acc[i];
      }
    }
    if (tid >= NS_THREADS - H) {
      const int nn = tid - (NS_THREADS - H);
      for (int r = 0; r < ROWS; ++r) gb1 += h2[r * LDH + nn];
    }
    __syncthreads();  // xs, h1, h2 are free for the next tile
  }

  // ---- once: this workgroup's sums and its share
  if (!FVP && wave == 0) {
    sum0 = ga_wave_sum(sum0);
    sum1 = ga_wave_sum(sum1);
    if (lane == 0) {
      m.lpart[2 * g + 0] = sum0;
      m.lpart[2 * g + 1] = sum1;
    }
  }
  if (EVAL) return;
  float* part = m.part + (int64_t)g * sh.stride;
  float* pW1 = part;
  float* pb1 = pW1 + (int64_t)H * ld0;
  float* pW2 = pb1 + H;
  float* pb2 = pW2 + (int64_t)H * H;
  float* pWh = pb2 + H;
  float* pbh = pWh + NS_HN * H;
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    const int t = wave + 4 * a, tn = t / KTMAX, tk = t % KTMAX;
    const int k = 32 * tk + l31;
    if (t < CT * KTMAX && k < ld0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = 32 * tn + (r & 3) + 8 * (r >> 2) + 4 * half;
        pW1[(int64_t)n * ld0 + k] = gW1[a][r];
      }
    }
  }
  {
    const int c = tid % H, j0 = (tid / H) * JPG;
#pragma unroll
    for (int jj = 0; jj < JPG; ++jj) pWh[(j0 + jj) * H + c] = gWh[jj];
    if (tid < NS_HN) pbh[tid] = gbh;
    if (tid >= NS_THREADS - H) {
      pb1[tid - (NS_THREADS - H)] = gb1;
      pb2[tid - (NS_THREADS - H)] = gb2;
    }
  }
  if (wave < CT * CT) {
    const int tn = wave / CT, tk = wave % CT;
    const int k = 32 * tk + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = 32 * tn + (r & 3) + 8 * (r >> 2) + 4 * half;
      pW2[n * H + k] = gW2[r];
    }
  }
}

// ---- the conjugate-gradient state of a member, one workgroup ------------------------
constexpr int CG_THREADS = 256;
constexpr int CG_REGIONS = 6;
// The six regions of a narrow network's flat vector (W1 | b1 | W2 | b2 | head rows | head
// bias): flat range [beg, beg + n) and where a share holds it.  Whatever lies between
// them (slot 0 .. 3, padding) is no parameter: its gradient is zero.
struct CgRegion {
  int64_t beg, n, src;
};
struct CgParams {
  GaNaturalShared sh;
  const GaNaturalDev* table;
  int mode;
  CgRegion r[CG_REGIONS];
};

__device__ __forceinline__ int ng_share_count(int S) {
  const int tiles = (S + NS_ROWS - 1) / NS_ROWS;
  return tiles < NG_SHARES ? tiles : NG_SHARES;
}

// element i of the member's shares, summed in share order (0 outside the regions)
__device__ __forceinline__ float cg_share_sum(const CgParams& p, const GaNaturalDev& m,
                                              int shares, int64_t i) {
  int64_t src = -1;
#pragma unroll
  for (int k = 0; k < CG_REGIONS; ++k)
    if (i >= p.r[k].beg && i < p.r[k].beg + p.r[k].n) src = p.r[k].src + (i - p.r[k].beg);
  if (src < 0) return 0.f;
  float acc = 0.f;
  for (int s = 0; s < shares; ++s) acc += m.part[(int64_t)s * p.sh.stride + src];
  return acc;
}

// a . b with fp64 accumulation in a fixed order; every thread gets the result
__device__ __forceinline__ double cg_dot(const float* a, const float* b, int64_t n,
                                         double* red) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += CG_THREADS) s += (double)a[i] * (double)b[i];
  s = ga_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const double r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}

// z = A v of the shares of the product's pass: J^T M J v summed in share order, the
// log-std block in slot 0 (2 A chain^2 v[0] for a Gaussian head with a learned std, 0
// otherwise: TRPO._fisher_vector_product), plus reg v.  scrub: NaNs of v count as zeros.
__device__ __forceinline__ void cg_product(const CgParams& p, const GaNaturalDev& m,
                                           int shares, const float* v, float* z,
                                           bool scrub) {
  float slot0 = 0.f;
  if (p.sh.kind == 0 && !p.sh.zero_slot0) {
    float chain;
    ga_log_std(m.params[0], p.sh.has_min, p.sh.min_log_std, p.sh.has_max, p.sh.max_log_std,
               &chain);
    slot0 = (float)(2.0 * (double)p.sh.out_w * (double)chain * (double)chain);
  }
  for (int64_t i = threadIdx.x; i < p.sh.n_flat; i += CG_THREADS) {
    float vi = v[i];
    if (scrub && vi != vi) vi = 0.f;
    const float acc = i == 0 ? vi * slot0 : cg_share_sum(p, m, shares, i);
    z[i] = fmaf(m.reg, vi, acc);
  }
}

// A thread reads and writes the elements i = threadIdx.x + 256 k of every vector only,
// so the vectors need no barrier between the phases; the dots bring their own.
__global__ __launch_bounds__(CG_THREADS) void members_cg_kernel(CgParams p) {
  __shared__ double red[4];
  const GaNaturalDev& m = p.table[blockIdx.x];
  const int64_t n = p.sh.n_flat, vs = p.sh.vec_stride;
  const int shares = ng_share_count(m.S);
  float* vb = m.vectors + NG_GRAD * vs;
  float* vx = m.vectors + NG_X * vs;
  float* vr = m.vectors + NG_R * vs;
  float* vp = m.vectors + NG_P * vs;
  float* vz = m.vectors + NG_Z * vs;
  const int tid = threadIdx.x;
  if (p.mode == NG_CG_PRODUCT) {
    cg_product(p, m, shares, m.vec, m.out, false);
    return;
  }
  if (p.mode == NG_CG_BEGIN) {
    // the surrogate's loss and the log-std slot from the workgroups' sums, in share order
    double first = 0.0, second = 0.0;
    for (int s = 0; s < shares; ++s) {
      first += m.lpart[2 * s + 0];
      second += m.lpart[2 * s + 1];
    }
    LossRowArgs L;
    L.kind = p.sh.kind; L.log_std = m.params; L.has_min = p.sh.has_min;
    L.has_max = p.sh.has_max; L.min_log_std = p.sh.min_log_std;
    L.max_log_std = p.sh.max_log_std; L.A = p.sh.out_w; L.algo = 2;
    L.ent = lr_ent(m.ent_coeff, p.sh.ent_flags);
    float loss, dls;
    lr_finish(L, first, second, m.S, &loss, &dls);
    if (p.sh.kind != 0 || p.sh.zero_slot0) dls = 0.f;
    for (int64_t i = tid; i < n; i += CG_THREADS) {
      const float b = i == 0 ? dls : cg_share_sum(p, m, shares, i);
      vb[i] = b; vx[i] = 0.f; vr[i] = b; vp[i] = b;
    }
    const double rdotr = cg_dot(vr, vr, n, red);
    if (tid == 0) {
      m.scalars[NG_RDOTR] = rdotr;
      m.scalars[NG_LOSS_BEFORE] = (double)loss;
      m.scalars[NG_DONE] = 0.0;
      m.scalars[NG_ITERS] = 0.0;
      m.scalars[NG_SAS] = 0.0;
      m.scalars[NG_STEP] = 0.0;
    }
    return;
  }
  if (p.mode == NG_CG_STEP) {
    if (m.scalars[NG_DONE] != 0.0) return;  // finished: left as it is
    const double rdotr = m.scalars[NG_RDOTR];
    cg_product(p, m, shares, vp, vz, false);
    const float v = (float)(rdotr / cg_dot(vp, vz, n, red));
    for (int64_t i = tid; i < n; i += CG_THREADS) {
      vx[i] = fmaf(v, vp[i], vx[i]);
      vr[i] = fmaf(-v, vz[i], vr[i]);
    }
    const double newrdotr = cg_dot(vr, vr, n, red);
    const float mu = (float)(newrdotr / rdotr);
    for (int64_t i = tid; i < n; i += CG_THREADS) vp[i] = fmaf(mu, vp[i], vr[i]);
    if (tid == 0) {
      m.scalars[NG_RDOTR] = newrdotr;
      m.scalars[NG_ITERS] += 1.0;
      if (newrdotr < 1e-10) m.scalars[NG_DONE] = 1.0;
    }
    return;
  }
  // NG_CG_FINISH: after the product of x
  for (int64_t i = tid; i < n; i += CG_THREADS) {
    const float x = vx[i];
    if (x != x) vx[i] = 0.f;  // torch.nan_to_num(x, nan=0, posinf=inf, neginf=-inf)
  }
  cg_product(p, m, shares, vx, vz, false);
  const double sAs = cg_dot(vx, vz, n, red);
  double step = sqrt(2.0 * (double)m.delta * (1.0 / (sAs + 1e-8)));
  if (step != step) step = 1.0;
  const float stepf = (float)step;
  float* vd = m.vectors + NG_DESCENT * vs;
  float* vprev = m.vectors + NG_PREV * vs;
  for (int64_t i = tid; i < n; i += CG_THREADS) {
    vd[i] = vx[i] * stepf;
    vprev[i] = m.params[i];
  }
  if (tid == 0) {
    m.scalars[NG_SAS] = sAs;
    m.scalars[NG_STEP] = step;
  }
}

// a searching member's candidate: loss and KL from its workgroups' sums, in share order
__global__ __launch_bounds__(64) void members_eval_finish_kernel(NaturalParams q) {
  const GaNaturalDev& m = q.table[blockIdx.x];
  if (m.state != NG_SEARCHING || threadIdx.x != 0) return;
  const int shares = ng_share_count(m.S);
  double first = 0.0, kl = 0.0;
  for (int s = 0; s < shares; ++s) {
    first += m.lpart[2 * s + 0];
    kl += m.lpart[2 * s + 1];
  }
  LossRowArgs L;
  L.kind = q.sh.kind; L.log_std = m.params; L.has_min = q.sh.has_min;
  L.has_max = q.sh.has_max; L.min_log_std = q.sh.min_log_std;
  L.max_log_std = q.sh.max_log_std; L.A = q.sh.out_w; L.algo = 2;
  L.ent = lr_ent(m.ent_coeff, q.sh.ent_flags);
  float loss, dls;
  lr_finish(L, first, 0.0, m.S, &loss, &dls);
  m.result[0] = (double)loss;
  m.result[1] = kl / (double)m.S;
}

// the saved parameters back into the members the line search rejected
__global__ __launch_bounds__(CG_THREADS) void members_candidate_kernel(NaturalParams q) {
  const GaNaturalDev& m = q.table[blockIdx.x];
  if (m.state != NG_REJECTED) return;
  const float* prev = m.vectors + NG_PREV * q.sh.vec_stride;
  for (int64_t i = threadIdx.x; i < q.sh.n_flat; i += CG_THREADS) m.params[i] = prev[i];
}

int ng_check(const GaNaturalShared* sh, const GaNaturalDev* table_dev, const char* who) {
  GA_REQUIRE(sh && table_dev, "%s: null pointer", who);
  const int dims[4] = {sh->in_w, sh->H, sh->H, sh->out_w};
  GA_REQUIRE(ga_narrow_step_supported(3, dims) && sh->n_members >= 1 &&
                 sh->n_members <= 65535 && sh->n_flat >= 4 &&
                 sh->stride == ga_narrow_step_stride(sh->in_w, sh->H),
             "%s: unsupported shape", who);
  return GA_OK;
}

}  // namespace

extern "C" int ga_members_natural_launch(const GaNaturalShared* sh,
                                         const GaNaturalDev* table_dev, int mode,
                                         hipStream_t stream) {
  int rc = ng_check(sh, table_dev, "ga_members_natural_launch");
  if (rc) return rc;
  GA_REQUIRE(mode >= NG_MODE_GRAD && mode <= NG_MODE_EVAL,
             "ga_members_natural_launch: unknown mode");
  NaturalParams q;
  memset(&q, 0, sizeof(q));
  q.sh = *sh; q.table = table_dev;
  const dim3 grid((unsigned)NG_SHARES, (unsigned)sh->n_members);
  ga_prof_count(GA_PROF_MEMBERS_STEP);
#define GA_NATURAL_LAUNCH(KERNEL, HH, LL, MM) \
  hipLaunchKernelGGL((KERNEL<HH, LL, MM>), grid, dim3(NS_THREADS), 0, stream, q)
#define GA_NATURAL_MODES(KERNEL, HH, LL)                                          \
  do {                                                                            \
    if (mode == NG_MODE_GRAD) GA_NATURAL_LAUNCH(KERNEL, HH, LL, NG_MODE_GRAD);    \
    else if (mode == NG_MODE_FVP) GA_NATURAL_LAUNCH(KERNEL, HH, LL, NG_MODE_FVP); \
    else GA_NATURAL_LAUNCH(KERNEL, HH, LL, NG_MODE_EVAL);                         \
  } while (0)
  const int ldx_s = ga_narrow_ldx(sh->in_w);
  if (ldx_s > NS_IN_OVERLAY + 4) {
    // 33 .. 128 inputs: the wide kernel (32-row tiles, dW1 on the matrix cores)
    ga_prof_count_narrow_wide();
    if (sh->H == 64) {
      if (ldx_s == 68) GA_NATURAL_MODES(narrow_natural_wide_kernel, 64, 68);
      else GA_NATURAL_MODES(narrow_natural_wide_kernel, 64, 132);
    } else {
      if (ldx_s == 68) GA_NATURAL_MODES(narrow_natural_wide_kernel, 32, 68);
      else GA_NATURAL_MODES(narrow_natural_wide_kernel, 32, 132);
    }
  } else if (sh->H == 64) {
    if (ldx_s == 12) GA_NATURAL_MODES(narrow_natural_members_kernel, 64, 12);
    else if (ldx_s == 20) GA_NATURAL_MODES(narrow_natural_members_kernel, 64, 20);
    else GA_NATURAL_MODES(narrow_natural_members_kernel, 64, 36);
  } else {
    if (ldx_s == 12) GA_NATURAL_MODES(narrow_natural_members_kernel, 32, 12);
    else if (ldx_s == 20) GA_NATURAL_MODES(narrow_natural_members_kernel, 32, 20);
    else GA_NATURAL_MODES(narrow_natural_members_kernel, 32, 36);
  }
#undef GA_NATURAL_MODES
#undef GA_NATURAL_LAUNCH
  GA_CHECK_LAUNCH("narrow_natural_members");
  return GA_OK;
}

extern "C" int ga_members_cg_launch(const GaNaturalShared* sh, const GaNaturalDev* table_dev,
                                    int mode, hipStream_t stream) {
  int rc = ng_check(sh, table_dev, "ga_members_cg_launch");
  if (rc) return rc;
  GA_REQUIRE(mode >= NG_CG_BEGIN && mode <= NG_CG_PRODUCT, "ga_members_cg_launch: unknown mode");
  CgParams p;
  memset(&p, 0, sizeof(p));
  p.sh = *sh; p.table = table_dev; p.mode = mode;
  // a share's layout (ga_narrow_step_stride): dW1 [H][ld0], db1, dW2 [H][H], db2,
  // dW_head [8][H], db_head [8]
  const int H = sh->H, A = sh->out_w;
  const int64_t ld0 = (sh->in_w + 3) & ~3;
  const int64_t n[CG_REGIONS] = {H * ld0, H, (int64_t)H * H, H, (int64_t)A * H, A};
  const int64_t held[CG_REGIONS] = {H * ld0, H, (int64_t)H * H, H, (int64_t)NS_HN * H, NS_HN};
  int64_t src = 0;
  for (int k = 0; k < CG_REGIONS; ++k) {
    p.r[k].beg = k % 2 ? sh->b_off[k / 2] : sh->w_off[k / 2];
    p.r[k].n = n[k];
    p.r[k].src = src;
    GA_REQUIRE(p.r[k].beg >= 4 && p.r[k].beg + p.r[k].n <= sh->n_flat,
               "ga_members_cg_launch: bad region");
    src += held[k];
  }
  ga_prof_count(GA_PROF_MEMBERS_STEP);
  hipLaunchKernelGGL(members_cg_kernel, dim3((unsigned)sh->n_members), dim3(CG_THREADS), 0,
                     stream, p);
  GA_CHECK_LAUNCH("members_cg");
  return GA_OK;
}

extern "C" int ga_members_candidate_launch(const GaNaturalShared* sh,
                                           const GaNaturalDev* table_dev,
                                           hipStream_t stream) {
  int rc = ng_check(sh, table_dev, "ga_members_candidate_launch");
  if (rc) return rc;
  NaturalParams q;
  memset(&q, 0, sizeof(q));
  q.sh = *sh; q.table = table_dev;
  ga_prof_count(GA_PROF_MEMBERS_STEP);
  hipLaunchKernelGGL(members_candidate_kernel, dim3((unsigned)sh->n_members),
                     dim3(CG_THREADS), 0, stream, q);
  GA_CHECK_LAUNCH("members_candidate");
  return GA_OK;
}

extern "C" int ga_members_eval_finish_launch(const GaNaturalShared* sh,
                                             const GaNaturalDev* table_dev,
                                             hipStream_t stream) {
  int rc = ng_check(sh, table_dev, "ga_members_eval_finish_launch");
  if (rc) return rc;
  NaturalParams q;
  memset(&q, 0, sizeof(q));
  q.sh = *sh; q.table = table_dev;
  ga_prof_count(GA_PROF_MEMBERS_STEP);
  hipLaunchKernelGGL(members_eval_finish_kernel, dim3((unsigned)sh->n_members), dim3(64), 0,
                     stream, q);
  GA_CHECK_LAUNCH("members_eval_finish");
  return GA_OK;
}
