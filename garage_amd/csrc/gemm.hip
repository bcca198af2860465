// fp32 MFMA GEMM family for the MLP policy / value networks (gfx950).
//
// One LDS-tiled kernel, C(m,n) = epi(sum_k A(m,k) * B(k,n)), instantiated for
// the three products an MLP layer needs (reference: nn.Linear forward/backward
// inside torch/modules/multi_headed_mlp_module.py:136-151, driven by
// torch/algos/vpg.py:250-293):
//   forward      Y  = act(X W^T + b)          A, B both k-contiguous
//   data grad    dX = (dY W) * (1 - H^2)      A k-contiguous, B n-contiguous
//   weight grad  dW = dY^T X (+ db = 1^T dY)  A, B both "row"-contiguous,
//                                             split-K over the batch into slabs
// Arithmetic is exact fp32 on v_mfma_f32_32x32x2_f32 (the parity bar is 1e-5 on
// losses, so no reduced-precision operands).  Every matrix this file touches
// has a leading dimension that is a multiple of 4 floats and a 16-B aligned
// base (garage_amd pads obs / weights / activations accordingly), so all
// global traffic is 16-B vector loads; ragged edges are masked, not branched.
//
// Operand tiles keep their memory orientation in LDS.  A k-contiguous operand is
// stored [BR][BK + 4] (one ds_write_b128 per loaded vector) and feeds four MFMAs
// from one ds_read_b128: lane l of a 32x32x2 MFMA holds row l & 31 and, in MFMA q
// of group g, k = 8g + 4(l >> 5) + q -- any k <-> slot map is valid as long as A
// and B agree.  A row-contiguous operand is stored [BK][BR + 4] and read with one
// ds_read_b32 per MFMA under the same map.  The +4 floats keep rows 16-B aligned
// and the 32-lane reads of an instruction on distinct banks (SQ_LDS_BANK_CONFLICT
// = 0 by PMC).  Tile shapes: 128x128 (8 waves, two workgroups per CU), 64x64 for
// 33..64-wide outputs, 128x32 for narrow ones; the products with a dimension
// <= 32 that stream a whole activation matrix go to skinny.hip instead.
#include "common.h"
#include <hip/hip_ext.h>

#include "prof.h"

#include "gemm_core.h"
#include "layer_plans.h"
#include "members_diag.h"

namespace {

// The narrow layer on 64 staged rows: lane = row, wave = a segment of CPS columns,
// whose weights are wave-uniform and come through the scalar cache (constant
// address space), so the inner product is v_fmac with an SGPR operand and LDS is
// read once per element; the waves' partial sums meet in `hp` and are added in a
// fixed order.
template <int NT_ALL, int BN, int LDC>
__device__ __forceinline__ void head_on_staged_rows(const GemmParams& p,
                                                    const float* stage, float* hp,
                                                    int n0, int m_base) {
  typedef const __attribute__((address_space(4))) float* uniform_ptr;
  constexpr int SEGS = NT_ALL / 64, CPS = BN / SEGS, HN = 8;
  const int row = threadIdx.x & 63;
  const int seg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float4 h[CPS / 4];
#pragma unroll
  for (int i = 0; i < CPS / 4; ++i)
    h[i] = *reinterpret_cast<const float4*>(stage + row * LDC + seg * CPS + 4 * i);
  float a[HN];
#pragma unroll
  for (int j = 0; j < HN; ++j) {
    a[j] = 0.f;
    if (j < p.head_n) {
      uniform_ptr w = (uniform_ptr)(uintptr_t)(p.head_W + (int64_t)j * p.head_ldw + n0 +
                                               seg * CPS);
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
  // hp holds PL planes: waves PL.. add theirs onto plane (wave - PL) in a second step
  constexpr int PL = SEGS < 4 ? SEGS : 4;
  static_assert(SEGS <= 2 * PL, "two reduction steps");
  float* mine = hp + ((seg % PL) * 64 + row) * HN;
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
  for (int o = threadIdx.x; o < 64 * HN; o += NT_ALL) {
    const int r = o / HN, j = o % HN;
    if (j < p.head_n) {
      float s = p.head_bias ? p.head_bias[j] : 0.f;
#pragma unroll
      for (int w = 0; w < PL; ++w) s += hp[(w * 64 + r) * HN + j];
      p.head_out[(int64_t)(m_base + r) * p.head_ld + j] = s;
    }
  }
}

// Split-operand k-loop of a 128 x 128 tile (opt-in, gemm_core.h: ft_split3_pair): the A
// operand -- k-contiguous rows of activations -- is fetched as two 16-B quads per thread
// and 32-deep step, two steps ahead, split into three bf16 planes in LDS one step ahead
// (two buffers); the B operand -- a weight matrix -- comes as fragments straight from
// its planes in L2 (p.bplanes), one step ahead, refilled in place; 24 MFMAs per step
// and wave (v_mfma_f32_32x32x16_bf16), one barrier.  K % 4 == 0; rows beyond M and k
// beyond K are zero in the planes.
__device__ __forceinline__ void gemm_mainloop_split(const GemmParams& p, float* lds,
                                                    f32x16 (&acc)[2][1], int m0, int n0,
                                                    int wm0, int wn0) {
  constexpr int PLANE_B = 128 * FT_PLANE_ROW_B, ABUF_B = 3 * PLANE_B;
  char* apl = reinterpret_cast<char*>(lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int K = p.K, nk = (K + 31) / 32;
  const int qq = tid & 7;
  const float* arow[2];
  bool row_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (tid >> 3) + 64 * i;
    const int m = min(m0 + r, p.M - 1);
    const int64_t line = p.a_idx ? (int64_t)p.a_idx[m] : (int64_t)m;
    arow[i] = p.A + line * p.lda;
    row_ok[i] = m0 + r < p.M;
  }
  auto load_quads = [&](int s, float4 (&v)[2]) {
    const int kq = min(32 * s + 4 * qq, K - 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] = *reinterpret_cast<const float4*>(arow[i] + kq);
  };
  auto store_quads = [&](int s, const float4 (&v)[2]) {
    const bool k_ok = 32 * s + 4 * qq < K;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float4 x = v[i];
      if (!row_ok[i] || !k_ok) x = make_float4(0.f, 0.f, 0.f, 0.f);
      uint32_t hi[2], mid[2], lo[2];
      ft_split3_pair(x.x, x.y, hi[0], mid[0], lo[0]);
      ft_split3_pair(x.z, x.w, hi[1], mid[1], lo[1]);
      char* dst = apl + (s & 1) * ABUF_B + ((tid >> 3) + 64 * i) * FT_PLANE_ROW_B + qq * 8;
      *reinterpret_cast<uint2*>(dst) = make_uint2(hi[0], hi[1]);
      *reinterpret_cast<uint2*>(dst + PLANE_B) = make_uint2(mid[0], mid[1]);
      *reinterpret_cast<uint2*>(dst + 2 * PLANE_B) = make_uint2(lo[0], lo[1]);
    }
  };
  const uint16_t* wpl = p.bplanes + (((n0 + wn0) / 32) * 64 + lane) * 8;
  ft_u32x4 bw[2][3];
  auto fetch_planes = [&](int s, int g) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      bw[g][pl] = *reinterpret_cast<const ft_u32x4*>(
          wpl + pl * p.bplane_stride + (int64_t)((2 * s + g) * p.bplane_nblk) * 512);
  };
  if (nk <= 0) return;
  fetch_planes(0, 0);
  fetch_planes(0, 1);
  float4 qc[2], qn[2];
  load_quads(0, qc);
  if (nk > 1) load_quads(1, qn);
  store_quads(0, qc);
  qc[0] = qn[0]; qc[1] = qn[1];
  __syncthreads();
#define GS_SB __builtin_amdgcn_sched_barrier(0)
  for (int s = 0; s < nk; ++s) {
    const bool more = s + 1 < nk;
    const char* arow_l =
        apl + (s & 1) * ABUF_B + (wm0 + l31) * FT_PLANE_ROW_B + 16 * half;
    ft_u32x4 af[2][2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        af[0][i][pl] = *reinterpret_cast<const ft_u32x4*>(arow_l + pl * PLANE_B +
                                                          32 * i * FT_PLANE_ROW_B);
#ifndef GA_GABL_NOLOAD
    if (s + 2 < nk) load_quads(s + 2, qn);
#endif
    GS_SB;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int slot = 0; slot < 24; ++slot) {
      const int g = slot / 12, t = (slot % 12) / 2, i = slot % 2;
      const int pa = t == 0 ? 2 : (t == 1 || t == 2) ? 1 : 0;
      const int pb = t == 3 ? 2 : (t == 1 || t == 4) ? 1 : 0;
#ifdef GA_GABL_NOMFMA
      acc[i][0][slot & 15] += __uint_as_float(af[g][i][pa][0] ^ bw[g][pb][0]);
#else
      acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          __builtin_bit_cast(ft_bf16x8, af[g][i][pa]),
          __builtin_bit_cast(ft_bf16x8, bw[g][pb]), acc[i][0], 0, 0, 0);
#endif
      GS_SB;
      if (slot == 6 || slot == 8 || slot == 11) {
        const int pl = slot == 6 ? 2 : slot == 8 ? 1 : 0;
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
          af[1][ii][pl] = *reinterpret_cast<const ft_u32x4*>(
              arow_l + pl * PLANE_B + 32 * ii * FT_PLANE_ROW_B + 32);
      }
      if (more) {
#ifndef GA_GABL_NOSTORE
        if (slot == 2) store_quads(s + 1, qc);
#endif
#ifndef GA_GABL_NOFETCH
        if (slot == 11) fetch_planes(s + 1, 0);
        if (slot == 23) fetch_planes(s + 1, 1);
#endif
      }
      GS_SB;
    }
    __builtin_amdgcn_s_setprio(0);
    qc[0] = qn[0]; qc[1] = qn[1];
    __syncthreads();
  }
#undef GS_SB
}

// bid: the workgroup's linear id within ITS problem (a pair launch carries two)
// SPLIT: the opt-in split-operand k-loop above (128 x 128 tiles, A_KC, weights as planes)
// PIPE: interior tiles take the software-pipelined two-stage k-loop
// (gemm_core.h: gemm_mainloop_pipe) -- for tile shapes with few waves per SIMD
template <int BM, int BN, int WAVES_M, int WAVES_N, bool A_KC, bool B_KC, int BKT,
          bool HEAD, bool SPLIT = false, bool PIPE = false>
__device__ __forceinline__ void gemm_f32_body(const GemmParams& p, const int bid) {
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 32, TN = WN / 32;
  // row-contiguous operands: [BK][BR + PAD]; k-contiguous ones: [BR][BK + PAD]
  constexpr int LDA_S = BM + PAD, LDB_S = BN + PAD, LDK = BKT + PAD;
  constexpr int A_FLOATS = A_KC ? BM * LDK : BKT * LDA_S;
  constexpr int B_FLOATS = B_KC ? BN * LDK : BKT * LDB_S;
  // (the epilogue stages 64 output rows in the same memory)
  constexpr int STAGE_FLOATS = (BM % 64 == 0) ? 64 * (BN + 4) : 0;
  constexpr int OPERAND_FLOATS = (PIPE ? 2 : 1) * (A_FLOATS + B_FLOATS);
  constexpr int TILE_FLOATS = OPERAND_FLOATS > STAGE_FLOATS ? OPERAND_FLOATS : STAGE_FLOATS;
  // HEAD: + the waves' partial head sums, [<= 4 planes][64 rows][8]
  constexpr int HEAD_PLANES = WAVES_M * WAVES_N < 4 ? WAVES_M * WAVES_N : 4;
  // (SPLIT: two buffers of three bf16 planes of the 128-row A tile)
  constexpr int SPLIT_FLOATS = SPLIT ? 2 * 3 * 128 * FT_PLANE_ROW_B / 4 : 0;
  constexpr int LDS_FLOATS = (TILE_FLOATS > SPLIT_FLOATS ? TILE_FLOATS : SPLIT_FLOATS) +
                             (HEAD ? HEAD_PLANES * 64 * 8 : 0);
  static_assert(!SPLIT || (BM == 128 && BN == 128 && WAVES_M == 2 && WAVES_N == 4 && A_KC &&
                           !HEAD),
                "the split-operand loop: 128 x 128 tiles, 8 waves, k-contiguous A");
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm0 = (wave / WAVES_N) * WM;
  const int wn0 = (wave % WAVES_N) * WN;
  // logical block from the linear id (XCD-aware order, common.h): with one split
  // the n blocks of an m block share its A tile; with split-K every block of a
  // split shares the split's A and B rows
  int bx, by, bz;
  if (p.gz == 1) {
    ga_xcd_group(bid, p.gx, p.gy, &bx, &by);
    bz = 0;
  } else {
    int mem;
    ga_xcd_group(bid, p.gz, p.gx * p.gy, &bz, &mem);
    bx = mem % p.gx;
    by = mem / p.gx;
  }
  const int m0 = bx * BM;
  const int n0 = by * BN;
  const int split = bz;
  const int kbeg = split * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float csum = 0.f;  // colsum accumulator (threads < BM or < BN)
  const bool do_colsum =
      p.colsum != nullptr &&
      (p.colsum_of_b ? (bx == 0) : (by == 0));

  // interior workgroups (every one at the C3 shapes, all but the last row / column
  // block and the last split otherwise) take the mask-free loader
  const bool full = (m0 + BM <= p.M) && (n0 + BN <= p.N) && kend > kbeg;
  if constexpr (SPLIT) {
    gemm_mainloop_split(p, lds, acc, m0, n0, wm0, wn0);
    __syncthreads();  // (the epilogue stages output rows over the planes)
  } else if (PIPE && full && !do_colsum)
    gemm_mainloop_pipe<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BKT>(p, lds, acc, m0, n0, kbeg,
                                                                  kend, wm0, wn0);
  else if (full)
    gemm_mainloop<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BKT, true>(
        p, lds, acc, csum, do_colsum, m0, n0, kbeg, kend, wm0, wn0);
  else
    gemm_mainloop<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BKT, false>(
        p, lds, acc, csum, do_colsum, m0, n0, kbeg, kend, wm0, wn0);

  // ---- epilogue: D(row, col): col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* Cout = p.C + (int64_t)split * p.c_split_stride;
#ifndef GA_NO_TR_EPILOGUE
  // Interior tiles of a row-major C go through LDS, 64 rows at a time in the
  // operand stages that are free now: a lane then owns 4
  // adjacent columns of a row, so stores (and the H / C loads of the fused
  // epilogues) are 16-B accesses and a wave instruction covers two whole 512-B
  // row segments instead of two 128-B ones.
  constexpr int NT_ALL = 64 * WAVES_M * WAVES_N;
  constexpr bool TR_OK = BM % 64 == 0 && (64 * (BN / 4)) % NT_ALL == 0;
  // (PIPE: the host has checked the layout conditions -- gemm_pipe_ok -- and N is a
  // multiple of BN; the last row block may be ragged and guards its rows below.  The
  // per-element path at the end is not instantiated: its loops stay rolled at 16
  // accumulator tiles and the accumulators would then live in scratch memory.)
  if (PIPE || (TR_OK && full && p.c_cs == 1 && (p.c_rs & 3) == 0 &&
      (reinterpret_cast<uintptr_t>(Cout) & 15u) == 0 &&
      (!p.H || ((p.ldh & 3) == 0 && (reinterpret_cast<uintptr_t>(p.H) & 15u) == 0)) &&
      (!p.bias || (reinterpret_cast<uintptr_t>(p.bias) & 15u) == 0))) {
    constexpr int LDC = BN + 4;
    for (int hrow = 0; hrow < BM; hrow += 64) {
      // (a wave's rows may span more than one 64-row pass: WM = 128 in the
      // one-wave-per-SIMD A/B instantiation)
      if (wm0 < hrow + 64 && wm0 + WM > hrow) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int rr =
                  wm0 - hrow + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
              if (rr >= 0 && rr < 64)
                lds[rr * LDC + wn0 + 32 * j + (lane & 31)] = acc[i][j][r];
            }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < (TR_OK ? 64 * (BN / 4) / NT_ALL : 0); ++q) {
        const int idx = threadIdx.x + NT_ALL * q;
        const int rr = idx / (BN / 4), c4 = idx % (BN / 4);
        const int m = m0 + hrow + rr, n = n0 + 4 * c4;
        if (PIPE && m >= p.M) continue;
        float4 v = *reinterpret_cast<const float4*>(lds + rr * LDC + 4 * c4);
        float* dst = Cout + (int64_t)m * p.c_rs + n;
        if (p.accum) {
          const float4 o = *reinterpret_cast<const float4*>(dst);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (p.epi == EPI_BIAS_ACT) {
          if (p.bias) {
            const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
            v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
          }
          if (p.act) {
            v.x = act_apply(v.x, p.act); v.y = act_apply(v.y, p.act);
            v.z = act_apply(v.z, p.act); v.w = act_apply(v.w, p.act);
          }
        }
        if ((p.epi == EPI_BIAS_ACT && p.H) || p.epi == EPI_MUL_DTANH) {
          const float4 h =
              *reinterpret_cast<const float4*>(p.H + (int64_t)m * p.ldh + n);
          v.x *= act_slope(h.x, p.hact); v.y *= act_slope(h.y, p.hact);
          v.z *= act_slope(h.z, p.hact); v.w *= act_slope(h.w, p.hact);
        }
        *reinterpret_cast<float4*>(dst) = v;
        if constexpr (HEAD) *reinterpret_cast<float4*>(lds + rr * LDC + 4 * c4) = v;
      }
      __syncthreads();
      if constexpr (HEAD) {
        head_on_staged_rows<NT_ALL, BN, LDC>(p, lds, lds + TILE_FLOATS, n0, m0 + hrow);
        __syncthreads();
      }
    }
    if (do_colsum) {
      const int W = p.colsum_of_b ? BN : BM;
      const int base = p.colsum_of_b ? n0 : m0;
      const int lim = p.colsum_of_b ? p.N : p.M;
      if ((int)threadIdx.x < W && base + (int)threadIdx.x < lim)
        p.colsum[(int64_t)split * p.colsum_split_stride + base + threadIdx.x] = csum;
    }
    return;
  }
#endif
  if constexpr (!PIPE) {
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn0 + 32 * j + (lane & 31);
      if (n >= p.N) continue;
      float bias = 0.f;
      if (p.epi == EPI_BIAS_ACT && p.bias) bias = p.bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= p.M) continue;
        float v = acc[i][j][r];
        if (p.accum) v += Cout[(int64_t)m * p.c_rs + (int64_t)n * p.c_cs];
        if (p.epi == EPI_BIAS_ACT) {
          v += bias;
          v = act_apply(v, p.act);
          if (p.H) {
            const float h = p.H[(int64_t)m * p.ldh + n];
            v *= act_slope(h, p.hact);
          }
        } else if (p.epi == EPI_MUL_DTANH) {
          const float h = p.H[(int64_t)m * p.ldh + n];
          v *= act_slope(h, p.hact);
        }
        Cout[(int64_t)m * p.c_rs + (int64_t)n * p.c_cs] = v;
      }
    }
  }
  if (do_colsum) {
    const int W = p.colsum_of_b ? BN : BM;
    const int base = p.colsum_of_b ? n0 : m0;
    const int lim = p.colsum_of_b ? p.N : p.M;
    if ((int)threadIdx.x < W && base + (int)threadIdx.x < lim)
      p.colsum[(int64_t)split * p.colsum_split_stride + base + threadIdx.x] = csum;
  }
  }  // !PIPE
}

template <int BM, int BN, int WAVES_M, int WAVES_N, bool A_KC, bool B_KC,
          int BKT = BK, bool HEAD = false>
#ifdef GA_GEMM_WAVES_PER_EU  // A/B builds (tools/build_variants.sh)
__attribute__((amdgpu_waves_per_eu(GA_GEMM_WAVES_PER_EU, 8)))
#endif
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_f32_kernel(
    GemmParams p) {
  gemm_f32_body<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BKT, HEAD>(p, (int)blockIdx.x);
}

// The forward product (both operands k-contiguous) of every entry of a device table in one
// grid (members_diag.h): entry blockIdx.y, whose own 1-D grid the launch's x covers or
// exceeds.  The same body as gemm_f32_kernel's, so the same bits per entry.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool HEAD>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_f32_members_kernel(
    const GemmParams* table) {
  const GemmParams p = table[blockIdx.y];
  if ((int)blockIdx.x >= p.gx * p.gy * p.gz) return;
  gemm_f32_body<BM, BN, WAVES_M, WAVES_N, true, true, BK, HEAD>(p, (int)blockIdx.x);
}

// 256 x 256 tiles, 4 waves of 128 x 128: one wave per SIMD, pipelined k-loop
template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_pipe_kernel(GemmParams p) {
  gemm_f32_body<256, 256, 2, 2, A_KC, B_KC, BK, false, false, true>(p, (int)blockIdx.x);
}

__global__ __launch_bounds__(512, 4) void gemm_kc_split_kernel(GemmParams p) {
  gemm_f32_body<128, 128, 2, 4, true, true, BK, false, true>(p, (int)blockIdx.x);
}

// Two problems of the same shape in one grid (GemmPair, gemm_params.h)
template <int BM, int BN, int WAVES_M, int WAVES_N, bool A_KC, bool B_KC>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_f32_pair_kernel(
    GemmPair pp) {
  const int bid = (int)(blockIdx.x >> 1);
  if (blockIdx.x & 1)
    gemm_f32_body<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BK, false>(pp.b, bid);
  else
    gemm_f32_body<BM, BN, WAVES_M, WAVES_N, A_KC, B_KC, BK, false>(pp.a, bid);
}

// ---- split-operand weight-gradient GEMM (opt-in, see ft_split3 in gemm_core.h):
// C[m][n] = sum_k A(m, k) B(k, n) with BOTH operands row-contiguous in memory
// (A(m, k) = A[k * lda + m]: k is the minibatch row).  v_mfma_f32_32x32x16_bf16 wants
// 8 consecutive k per lane, so the loader pairs two consecutive rows: a thread loads
// the same 16-B column quad of rows 2 t and 2 t + 1, splits the eight values and
// writes, per plane, the four (row 2 t, row 2 t + 1) bf16 pairs as ONE 16-B LDS store
// into [pair][column] dwords; a fragment is then four ds_read_b32 down the pairs.
// 128 x 128 tiles, 8 waves (2 x 4, 64 x 32 each), 16 rows per step, operands fetched
// three steps ahead (they come from HBM), double-buffered planes, one barrier per
// step.  Interior shapes only (the host checks): M, N multiples of 128, no gathers.
constexpr int NTS_LD = 136;                  // dwords per pair row: 128 + 8 (the two lane
                                             // halves read rows 4 apart: 32 banks apart)
constexpr int NTS_PLANE = 8 * NTS_LD;        // dwords per plane of a 16-row step
constexpr int NTS_OPER = 3 * NTS_PLANE;      // hi, mid, lo
constexpr int NTS_BUF = 2 * NTS_OPER;        // A and B

__global__ __launch_bounds__(512, 4) void gemm_nt_split_kernel(GemmParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[2 * NTS_BUF];
  __shared__ __attribute__((aligned(16))) float cs_lds[8 * 128];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / 4) * 64, wn0 = (wave % 4) * 32;
  int bz, mem;
  ga_xcd_group((int)blockIdx.x, p.gz, p.gx * p.gy, &bz, &mem);
  const int bx = mem % p.gx, by = mem / p.gx;
  const int m0 = bx * 128, n0 = by * 128;
  const int kbeg = bz * p.k_per_split, kend = min(p.K, kbeg + p.k_per_split);
  const int nk = (kend - kbeg + 15) / 16;

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // loader: threads 0 .. 255 take A, 256 .. 511 take B; pair pi of the step, quad c4
  const bool isb = tid >= 256;
  const int lt = tid & 255, pi = lt >> 5, c4 = lt & 31;
  const float* src = isb ? p.B + n0 + 4 * c4 : p.A + m0 + 4 * c4;
  const int64_t ld = isb ? p.ldb : p.lda;
  uint32_t* dst0 = lds + (isb ? NTS_OPER : 0) + pi * NTS_LD + 4 * c4;
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load2 = [&](int s, float4& v0, float4& v1) {
    const int r0 = kbeg + 16 * s + 2 * pi;
    v0 = *reinterpret_cast<const float4*>(src + (int64_t)min(r0, p.K - 1) * ld);
    v1 = *reinterpret_cast<const float4*>(src + (int64_t)min(r0 + 1, p.K - 1) * ld);
    if (r0 >= kend) v0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + 1 >= kend) v1 = make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store2 = [&](int s, const float4& v0, const float4& v1) {
    const float a[4] = {v0.x, v0.y, v0.z, v0.w}, b[4] = {v1.x, v1.y, v1.z, v1.w};
    uint32_t h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ft_split3_pair(a[j], b[j], h[j], m[j], l[j]);
    uint32_t* d = dst0 + (s & 1) * NTS_BUF;
    *reinterpret_cast<uint4*>(d) = make_uint4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<uint4*>(d + NTS_PLANE) = make_uint4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<uint4*>(d + 2 * NTS_PLANE) = make_uint4(l[0], l[1], l[2], l[3]);
    if (!isb) {
      csum.x += v0.x + v1.x; csum.y += v0.y + v1.y;
      csum.z += v0.z + v1.z; csum.w += v0.w + v1.w;
    }
  };
  // three steps in flight
  float4 q0[3], q1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    q0[d] = make_float4(0.f, 0.f, 0.f, 0.f);
    q1[d] = q0[d];
    if (d < nk) load2(d, q0[d], q1[d]);
  }
  if (nk > 0) store2(0, q0[0], q1[0]);
  __syncthreads();

  const int half = lane >> 5, l31 = lane & 31;
  // fragment rows: pairs 4 half .. 4 half + 3 of the step
  const uint32_t* fa = lds + 4 * half * NTS_LD + wm0 + l31;
  const uint32_t* fb = lds + NTS_OPER + 4 * half * NTS_LD + wn0 + l31;
  auto frag = [&](const uint32_t* base, int pl) {
    ft_u32x4 v;
    v[0] = base[pl * NTS_PLANE];
    v[1] = base[pl * NTS_PLANE + NTS_LD];
    v[2] = base[pl * NTS_PLANE + 2 * NTS_LD];
    v[3] = base[pl * NTS_PLANE + 3 * NTS_LD];
    return __builtin_bit_cast(ft_bf16x8, v);
  };
#pragma unroll 1
  for (int s0 = 0; s0 < nk; s0 += 3) {
    // (unrolled by the depth of the prefetch ring so that its registers are static)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int s = s0 + d;
      if (s < nk) {
        const uint32_t* ab = fa + (s & 1) * NTS_BUF;
        const uint32_t* bb = fb + (s & 1) * NTS_BUF;
        ft_bf16x8 a[2][3], b[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          a[0][pl] = frag(ab, pl);
          a[1][pl] = frag(ab + 32, pl);
          b[pl] = frag(bb, pl);
        }
        // the quads of step s + 1 are in registers since two steps ago: split them
        // into the other buffer while this step's MFMAs run, then refill the slot
        // with step s + 3
        __builtin_amdgcn_s_setprio(1);
        ft_mfma6(a[0], b, acc[0]);
        ft_mfma6(a[1], b, acc[1]);
        __builtin_amdgcn_s_setprio(0);
        if (s + 1 < nk) store2(s + 1, q0[(d + 1) % 3], q1[(d + 1) % 3]);
        if (s + 3 < nk) load2(s + 3, q0[d], q1[d]);
        __syncthreads();
      }
    }
  }

  // ---- epilogue: the slab of this split; bias-gradient column sums of A
  float* Cout = p.C + (int64_t)bz * p.c_split_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half;
      Cout[(int64_t)m * p.c_rs + (int64_t)(n0 + wn0 + l31) * p.c_cs] = acc[i][r];
    }
  if (p.colsum != nullptr && by == 0) {
    if (!isb) *reinterpret_cast<float4*>(cs_lds + pi * 128 + 4 * c4) = csum;
    __syncthreads();
    if (tid < 128) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t += cs_lds[k * 128 + tid];
      p.colsum[(int64_t)bz * p.colsum_split_stride + m0 + tid] = t;
    }
  }
}

// ---- weight-gradient GEMM, interior row-major shapes (layer_plans.h: ga_gemm_paired_ok).
// gemm_f32_kernel<128, 128, 2, 4, false, false> again -- the same tiles, slabs, k order
// per output element and column sums, so the same bits -- with the vector instructions
// this case does not need taken out of the wave's instruction stream (beside an fp32 MFMA
// every one of them is matrix time).  Three items, each with an A/B
// macro that restores the parent's form (tools/build_variants.sh):
//   * paired columns (GA_GEMM_NO_PAIRED_COLS): waves are 4 (m) x 2 (n) and own 32 x 64
//     outputs; lane l31 of accumulator block j holds column wn0 + 2 l31 + j, so the two B
//     values of a lane for one k are neighbours in the [k][BN + PAD] image and come with
//     ONE ds_read_b64 (8-B aligned: LDB_S and wn0 are even; 32 lanes cover 64 consecutive
//     dwords).  8 LDS reads per 8 MFMAs instead of 12.
//   * direct stores (GA_GEMM_NO_DIRECT_STORE; needs the paired columns): a lane holds
//     C[m][n] and C[m][n + 1] -- one 8-B store per accumulator register, a 256-B run per
//     half wave, no LDS staging and none of its four barriers.
//   * buffer addressing (GA_GEMM_NO_BUFFER_ADDR): the tile loads and the slab stores go
//     through GaBuffer (common.h) -- one lane offset per operand computed in front of the
//     loop, the k-step and the store's row as scalar offsets.  The descriptors' extents are
//     exact; every clamp and mask of the ragged last k-step stays.
// The last k-step is masked only where it is partial (the parent masks it always).
#ifdef GA_GEMM_NO_PAIRED_COLS
constexpr bool RR_PAIRED = false;
#else
constexpr bool RR_PAIRED = true;
#endif
#ifdef GA_GEMM_NO_DIRECT_STORE
constexpr bool RR_DIRECT = false;
#else
constexpr bool RR_DIRECT = RR_PAIRED;
#endif
#ifdef GA_GEMM_NO_BUFFER_ADDR
constexpr bool RR_BUF = false;
#else
constexpr bool RR_BUF = true;
#endif

// One [BK][128] tile of a row-major operand, two 16-B vectors per thread: rows
// tid / 32 and tid / 32 + 16 of the k-step, columns 4 (tid % 32) ..
struct RrLoader {
  float4 regs[2];
  GaBuffer buf;
  uint32_t voff;        // RR_BUF: the lane's byte offset in the slab's rows of the tile
  const float* ptr[2];  // !RR_BUF: the lane's two vectors of the slab's first k-step
  int64_t ld;
  int rows;             // of the slab

  // base: the operand at (kbeg, first column of the tile)
  __device__ __forceinline__ RrLoader(const float* base, int64_t ld_, int rows_)
      : buf(base, rows_ > 0 ? 4u * ((uint32_t)(rows_ - 1) * (uint32_t)ld_ + 128u) : 0u),
        ld(ld_), rows(rows_) {
    const int tid = threadIdx.x;
    voff = 4u * ((uint32_t)(tid >> 5) * (uint32_t)ld_ + 4u * (tid & 31));
#pragma unroll
    for (int i = 0; i < 2; ++i) ptr[i] = base + (int64_t)((tid >> 5) + 16 * i) * ld_ + 4 * (tid & 31);
  }
  // krel: the k-step's first row within the slab
  __device__ __forceinline__ void load(int krel) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (RR_BUF)
        regs[i] = buf.load4(voff, 4u * (uint32_t)(krel + 16 * i) * (uint32_t)ld);
      else
        regs[i] = *reinterpret_cast<const float4*>(ptr[i] + (int64_t)krel * ld);
    }
  }
  // a partial k-step: rows beyond the slab are clamped into it here and zeroed by store()
  __device__ __forceinline__ void load_partial(int krel) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = min(krel + (tid >> 5) + 16 * i, rows - 1);  // (rows >= 1 here)
      if (RR_BUF)
        regs[i] = buf.load4(4u * ((uint32_t)row * (uint32_t)ld + 4u * (tid & 31)), 0u);
      else
        regs[i] = *reinterpret_cast<const float4*>(ptr[0] + (int64_t)(row - (tid >> 5)) * ld);
    }
  }
  __device__ __forceinline__ void store(float* tile, int krel, bool masked) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = (tid >> 5) + 16 * i;
      float4 v = regs[i];
      if (masked && krel + k >= rows) v = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(tile + k * (128 + PAD) + 4 * (tid & 31)) = v;
    }
  }
};

__global__ __launch_bounds__(512) void gemm_rr_paired_kernel(GemmParams p) {
  constexpr int BM = 128, BN = 128, NT_ALL = 512;
  constexpr int LDA_S = BM + PAD, LDB_S = BN + PAD, A_FLOATS = BK * LDA_S;
  constexpr int WAVES_N = RR_PAIRED ? 2 : 4;
  constexpr int WM = RR_PAIRED ? 32 : 64, WN = RR_PAIRED ? 64 : 32;
  // the operand tiles; the staged epilogue's 64 rows of BN + 4 are the same size (the
  // parent's footprint: the two update chains' workgroups co-reside on a CU)
  __shared__ __attribute__((aligned(16))) float lds[BK * (LDA_S + LDB_S)];
  static_assert(BK * (LDA_S + LDB_S) >= 64 * (BN + 4), "the epilogue's stage");

  const int tid = threadIdx.x, lane = tid & 63;
  const int half = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
  int bx, by, bz;  // (the parent's order, gemm_f32_body)
  if (p.gz == 1) {
    ga_xcd_group((int)blockIdx.x, p.gx, p.gy, &bx, &by);
    bz = 0;
  } else {
    int mem;
    ga_xcd_group((int)blockIdx.x, p.gz, p.gx * p.gy, &bz, &mem);
    bx = mem % p.gx;
    by = mem / p.gx;
  }
  const int m0 = bx * BM, n0 = by * BN;
  const int kbeg = bz * p.k_per_split, kend = min(p.K, kbeg + p.k_per_split);
  const int rows = max(kend - kbeg, 0);
  const int nk = (rows + BK - 1) / BK;
  const bool partial = (rows % BK) != 0;  // the last k-step is masked

  // acc[t]: RR_PAIRED columns wn0 + 2 l31 + t, else rows wm0 + 32 t ..
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float csum = 0.f;
  const bool do_colsum = p.colsum != nullptr && (p.colsum_of_b ? (bx == 0) : (by == 0));

  float* As = lds;
  float* Bs = lds + A_FLOATS;
  RrLoader la(p.A + (int64_t)kbeg * p.lda + m0, p.lda, rows);
  RrLoader lb(p.B + (int64_t)kbeg * p.ldb + n0, p.ldb, rows);
  if (nk > 0) {
    const bool t0 = partial && nk == 1;
    if (t0) {
      la.load_partial(0);
      lb.load_partial(0);
    } else {
      la.load(0);
      lb.load(0);
    }
    la.store(As, 0, t0);
    lb.store(Bs, 0, t0);
  }
  __syncthreads();

  // lane half h feeds k = 8 g + 4 h + q to MFMA q of group g (gemm_core.h: gemm_mainloop)
  const float* fa = As + 4 * half * LDA_S + wm0 + l31;
  const float* fb = Bs + 4 * half * LDB_S + wn0 + (RR_PAIRED ? 2 : 1) * l31;
  for (int s = 0; s < nk; ++s) {
    const bool more = s + 1 < nk;
    const bool tail = partial && s + 2 == nk;  // the tile being fetched is the partial one
    if (more) {
      if (tail) {
        la.load_partial((s + 1) * BK);
        lb.load_partial((s + 1) * BK);
      } else {
        la.load((s + 1) * BK);
        lb.load((s + 1) * BK);
      }
    }
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) {
      float a[2][4], b[2][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[0][q] = fa[(8 * g + q) * LDA_S];
        if (RR_PAIRED) {
          const float2 v = *reinterpret_cast<const float2*>(fb + (8 * g + q) * LDB_S);
          b[0][q] = v.x;
          b[1][q] = v.y;
        } else {
          a[1][q] = fa[(8 * g + q) * LDA_S + 32];
          b[0][q] = fb[(8 * g + q) * LDB_S];
        }
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[RR_PAIRED ? 0 : t][q],
                                                        b[RR_PAIRED ? t : 0][q], acc[t], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    if (do_colsum) {
      const float* T = p.colsum_of_b ? Bs : As;
      if (tid < 128) {
#pragma unroll 8
        for (int k = 0; k < BK; ++k) csum += T[k * LDA_S + tid];
      }
    }
    __syncthreads();
    if (more) {
      la.store(As, (s + 1) * BK, tail);
      lb.store(Bs, (s + 1) * BK, tail);
      __syncthreads();
    }
  }

  // ---- epilogue: the slab of this split.  D(row, col): col = lane & 31,
  // row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* Ctile = p.C + (int64_t)bz * p.c_split_stride + (int64_t)m0 * p.c_rs + n0;
  const GaBuffer cbuf(Ctile, 4u * ((uint32_t)(BM - 1) * (uint32_t)p.c_rs + BN));
  if constexpr (RR_DIRECT) {
    const uint32_t voff = 4u * ((uint32_t)(wm0 + 4 * half) * (uint32_t)p.c_rs + wn0 + 2 * l31);
    float* dst = Ctile + (int64_t)(wm0 + 4 * half) * p.c_rs + wn0 + 2 * l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2);
      if (RR_BUF)
        cbuf.store2(acc[0][r], acc[1][r], voff, 4u * (uint32_t)row * (uint32_t)p.c_rs);
      else
        *reinterpret_cast<float2*>(dst + (int64_t)row * p.c_rs) = make_float2(acc[0][r], acc[1][r]);
    }
  } else {
    // the parent's: through LDS, 64 rows at a time, 16-B stores of whole row segments
    constexpr int LDC = BN + 4;
    for (int hrow = 0; hrow < BM; hrow += 64) {
      if (wm0 < hrow + 64 && wm0 + WM > hrow) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rr = wm0 - hrow + (RR_PAIRED ? 0 : 32 * t) + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int cc = wn0 + (RR_PAIRED ? 2 * l31 + t : l31);
            if (rr >= 0 && rr < 64) lds[rr * LDC + cc] = acc[t][r];
          }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 64 * (BN / 4) / NT_ALL; ++q) {
        const int rr = (tid >> 5) + 16 * q, c4 = tid & 31;
        const float4 v = *reinterpret_cast<const float4*>(lds + rr * LDC + 4 * c4);
        if (RR_BUF)
          cbuf.store4(v, 4u * ((uint32_t)(tid >> 5) * (uint32_t)p.c_rs + 4u * c4),
                      4u * (uint32_t)(hrow + 16 * q) * (uint32_t)p.c_rs);
        else
          *reinterpret_cast<float4*>(Ctile + (int64_t)(hrow + rr) * p.c_rs + 4 * c4) = v;
      }
      __syncthreads();
    }
  }
  if (do_colsum && tid < 128)
    p.colsum[(int64_t)bz * p.colsum_split_stride + (p.colsum_of_b ? n0 : m0) + tid] = csum;
}

// ---------------------------------------------------------------------------
// The launch seam (layer_plans.h): which tile, which grid and which k range is the
// plan's word, and `p` arrives with them filled in; here the plan's enum becomes an
// instantiation.
// ---------------------------------------------------------------------------
// launches of gemm_rr_paired_kernel since the library was loaded (kind 2 times and counts
// the weight-gradient GEMM whichever kernel it takes; tests ask which one it was)
int64_t g_paired_launches = 0;

template <bool A_KC, bool B_KC>
int launch_gemm(const GemmPlan& plan, const GemmParams& p, hipStream_t stream) {
  const dim3 grid((unsigned)(p.gx * p.gy * p.gz)), block((unsigned)plan.threads);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(plan.prof_kind, plan.work, &e0, &e1);
  switch (plan.tile) {
    case GT_SMALL_M:
      hipExtLaunchKernelGGL((gemm_f32_kernel<64, 64, 2, 2, A_KC, B_KC, 128>), grid, block, 0,
                            stream, e0, e1, 0, p);
      break;
    case GT_128x32:
      hipExtLaunchKernelGGL((gemm_f32_kernel<128, 32, 4, 1, A_KC, B_KC>), grid, block, 0,
                            stream, e0, e1, 0, p);
      break;
    case GT_64x64:
      hipExtLaunchKernelGGL((gemm_f32_kernel<64, 64, 2, 2, A_KC, B_KC>), grid, block, 0,
                            stream, e0, e1, 0, p);
      break;
    case GT_KC_SPLIT:
      hipExtLaunchKernelGGL(gemm_kc_split_kernel, grid, block, 0, stream, e0, e1, 0, p);
      break;
    case GT_NT_SPLIT:
      hipExtLaunchKernelGGL(gemm_nt_split_kernel, grid, block, 0, stream, e0, e1, 0, p);
      break;
    case GT_128x128:
      if (plan.paired_cols) {  // (the plan has checked the orientation and the layout)
        ++g_paired_launches;
        hipExtLaunchKernelGGL(gemm_rr_paired_kernel, grid, block, 0, stream, e0, e1, 0, p);
        break;
      }
#ifdef GA_GEMM_BIG_TILE  // A/B builds: 4-wave workgroups with 128-row wave tiles
      // 1: 256 x 256 tiles, waves of 128 x 128 (one per SIMD); 2: 256 x 128, waves of 128 x 64
      if (p.gz == 1 && p.M >= 4096 && p.N % 256 == 0) {
        constexpr int TBN = GA_GEMM_BIG_TILE == 2 ? 128 : 256;
        GemmParams q = p;
        q.gx = (int)ga_ceil_div(p.M, 256); q.gy = p.N / TBN;
        dim3 g2((unsigned)(q.gx * q.gy));
        const bool pipe_ok = !p.colsum && p.c_cs == 1 && (p.c_rs & 3) == 0 && ga_aligned16(p.C) &&
                             (!p.H || ((p.ldh & 3) == 0 && ga_aligned16(p.H))) &&
                             (!p.bias || ga_aligned16(p.bias)) && !p.accum &&
                             p.K % BK == 0 && !p.a_idx && !p.b_idx;
        if (GA_GEMM_BIG_TILE == 3 && pipe_ok)
          hipExtLaunchKernelGGL((gemm_f32_pipe_kernel<A_KC, B_KC>), g2, dim3(256), 0, stream,
                                e0, e1, 0, q);
        else
          hipExtLaunchKernelGGL((gemm_f32_kernel<256, TBN, 2, 2, A_KC, B_KC>), g2, dim3(256),
                                0, stream, e0, e1, 0, q);
        GA_CHECK_LAUNCH("gemm_f32 (256-row tiles)");
        return GA_OK;
      }
#endif
#ifdef GA_GEMM_BIG_BKT  // A/B builds (tools/build_variants.sh): k-tile depth of this shape
      hipExtLaunchKernelGGL((gemm_f32_kernel<128, 128, 2, 4, A_KC, B_KC, GA_GEMM_BIG_BKT>),
                            grid, block, 0, stream, e0, e1, 0, p);
#else
      hipExtLaunchKernelGGL((gemm_f32_kernel<128, 128, 2, 4, A_KC, B_KC>), grid, block, 0,
                            stream, e0, e1, 0, p);
#endif
      break;
  }
  GA_CHECK_LAUNCH("gemm_f32");
  return GA_OK;
}

}  // namespace

extern "C" int64_t ga_wgrad_paired_launches(void) { return g_paired_launches; }

int ga_gemm_launch(const GemmPlan& plan, const GemmParams& p, hipStream_t stream) {
  if (plan.a_kc && plan.b_kc) return launch_gemm<true, true>(plan, p, stream);
  if (plan.a_kc) return launch_gemm<true, false>(plan, p, stream);
  return launch_gemm<false, false>(plan, p, stream);
}

int ga_gemm_head_launch(const GemmHeadPlan& plan, const GemmParams& p, hipStream_t stream) {
  const dim3 grid((unsigned)p.gx), block((unsigned)plan.threads);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_GEMM_NT_128, plan.work, &e0, &e1);
  if (plan.width == 64)
    hipExtLaunchKernelGGL((gemm_f32_kernel<64, 64, 2, 2, true, true, BK, true>), grid, block,
                          0, stream, e0, e1, 0, p);
  else if (plan.width == 128)
    hipExtLaunchKernelGGL((gemm_f32_kernel<64, 128, 1, 4, true, true, BK, true>), grid, block,
                          0, stream, e0, e1, 0, p);
  else
    hipExtLaunchKernelGGL((gemm_f32_kernel<64, 256, 1, 8, true, true, BK, true>), grid, block,
                          0, stream, e0, e1, 0, p);
  GA_CHECK_LAUNCH("gemm_f32 (+head)");
  return GA_OK;
}

int md_launch_gemm_members(int kind, const GemmParams* table, unsigned n, unsigned blocks,
                           hipStream_t stream) {
  // (counted as one launch of the lone kernel's kind, never timed)
  ga_prof_count(kind == MD_GEMM_128x32 ? GA_PROF_GEMM_NT_256 : GA_PROF_GEMM_NT_128);
  const dim3 grid(blocks, n), block(256);
  switch (kind) {
    case MD_GEMM_128x32:
      hipLaunchKernelGGL((gemm_f32_members_kernel<128, 32, 4, 1, false>), grid, block, 0,
                         stream, table);
      break;
    case MD_GEMM_64x64:
      hipLaunchKernelGGL((gemm_f32_members_kernel<64, 64, 2, 2, false>), grid, block, 0, stream,
                         table);
      break;
    case MD_GEMM_HEAD_64:
      hipLaunchKernelGGL((gemm_f32_members_kernel<64, 64, 2, 2, true>), grid, block, 0, stream,
                         table);
      break;
    default:
      ga_set_error("gemm_f32_members: kind %d not instantiated", kind);
      return GA_ERR_ARG;
  }
  GA_CHECK_LAUNCH("gemm_f32_members");
  return GA_OK;
}

int ga_gemm_pair_launch(const GemmPairPlan& plan, const GemmParams& a, const GemmParams& b,
                        hipStream_t stream) {
  GemmPair pp;
  pp.a = a;
  pp.b = b;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ga_prof_events(GA_PROF_GEMM_TN_128, plan.work, &e0, &e1);
  ga_prof_count(GA_PROF_GEMM_TN_128);
  const dim3 grid((unsigned)(2 * plan.gx * plan.gy * plan.gz));
  hipExtLaunchKernelGGL((gemm_f32_pair_kernel<128, 128, 2, 4, false, false>), grid,
                        dim3(512), 0, stream, e0, e1, 0, pp);
  GA_CHECK_LAUNCH("gemm_f32_pair");
  return GA_OK;
}

namespace {
__global__ __launch_bounds__(256) void act_slope_mul_kernel(float* dout, int64_t ldd,
                                                            const float* out, int64_t ldo,
                                                            int64_t M, int N, int act) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * N) return;
  const int64_t i = e / N;
  const int j = (int)(e % N);
  const float o = out[i * ldo + j];
  dout[i * ldd + j] *= act_slope_fwd(o, act);  // (forward codes, gemm_core.h)
}
}  // namespace

extern "C" int ga_act_slope_mul_f32(float* dout, int64_t ldd, const float* out,
                                    int64_t ldo, int64_t M, int N, int act,
                                    ga_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GA_REQUIRE(dout && out && M >= 0 && N >= 1 && ldd >= N && ldo >= N && act >= 0 &&
                 act <= 6,
             "ga_act_slope_mul_f32: bad arguments");
  if (M == 0 || act == 0) return GA_OK;
  hipLaunchKernelGGL(act_slope_mul_kernel, dim3((unsigned)ga_ceil_div(M * N, 256)),
                     dim3(256), 0, stream, dout, ldd, out, ldo, M, N, act);
  GA_CHECK_LAUNCH("act_slope_mul");
  return GA_OK;
}
