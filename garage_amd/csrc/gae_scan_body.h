// The row arithmetic of the returns / GAE(lambda) scan, written ONCE for the kernels that
// run it: gae_scan_kernel / gae_scan_rows_kernel (gae_scan.hip), where a wave of the grid
// takes its rows and the advantages go to HBM, and members_advantage_kernel
// (members_advantage.hip), where the waves of ONE workgroup walk a member's rows and the
// advantages stay in LDS for the normalisation.  A body takes the wave index the lone
// launch would have, the value of the all-zero observation (v0: a kernel argument of the
// lone kernels, a device scalar of the member's) and a sink for the advantages; the
// returns always go to HBM.
// Device code only.
#pragma once
#include "common.h"
#include "gae_scan_params.h"

namespace {

struct Pair {
  double d;  // decay applied to the carry coming from the right
  double x;  // value when that carry is 0
};

__device__ __forceinline__ double shfl_down_d(double v, int o, int width) {
  return __shfl_down(v, o, width);
}

// The advantages of the lone kernels: to HBM where the returns go.  A sink gets the row,
// the row's first float (`start`) and the step index inside the row.
struct AdvToHbm {
  float* adv;
  __device__ __forceinline__ void quad(int64_t, int64_t start, int64_t i, float a0, float a1,
                                       float a2, float a3) const {
    *reinterpret_cast<float4*>(adv + start + i) = make_float4(a0, a1, a2, a3);
  }
  __device__ __forceinline__ void one(int64_t, int64_t start, int64_t i, float a) const {
    adv[start + i] = a;
  }
};

// Carry entering an episode of length L from its zero-padded tail (Q2).
__device__ double padded_tail_carry(const ScanParams& p, double v0, int L, double* boot) {
  const int m = p.P - L;
  if (m <= 0) {
    *boot = 0.0;
    return 0.0;
  }
  *boot = v0;
  const double pad_delta = p.bonus_const + (p.gamma - 1.0) * v0;
  double cm1 = 1.0, base = p.c;  // c^(m-1) by squaring: cheap in registers
  for (int e = m - 1; e > 0; e >>= 1) {
    if (e & 1) cm1 *= base;
    base *= base;
  }
  const double geo = (p.c == 1.0) ? (double)(m - 1) : (1.0 - cm1) / (1.0 - p.c);
  return pad_delta * geo + cm1 * (p.bonus_const - v0);
}

// The general kernel's wave: 64 / lpr rows, each walked chunk by chunk from the right.
template <bool VEC, class AdvSink>
__device__ __forceinline__ void gae_scan_wave(const ScanParams& p, double v0, int64_t wave,
                                              int lane, const AdvSink& sink) {
  const int lpr = p.lpr;
  const int rows_per_wave = 64 / lpr;
  const int sub = lane & (lpr - 1);
  const int64_t row = wave * rows_per_wave + lane / lpr;
  const bool row_ok = row < p.n_rows;

  int64_t start = 0, len = 0;
  if (row_ok) {
    if (p.offsets) {
      start = p.offsets[row];
      len = p.offsets[row + 1] - start;
    } else {
      start = row * p.ld;
      len = p.T;
    }
  }
  // 16-B accesses need the row to start on a 4-float boundary (always true for
  // the padded layout, true for packed batches of fixed-length episodes).
  const bool vec_row = (start & 3) == 0;
  const int C = 4 * lpr;
  int nchunks = (int)((len + C - 1) / C);
  int maxchunks = nchunks;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    maxchunks = max(maxchunks, __shfl_xor(maxchunks, o, 64));

  double carry_a = 0.0, carry_g = 0.0, vnext_chunk = 0.0;

  for (int k = maxchunks - 1; k >= 0; --k) {
    const bool active = k < nchunks;
    const int64_t i0 = (int64_t)k * C + 4 * sub;  // first step of this lane
    float r[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    int tl[4] = {0, 0, 0, 0};
    const bool full = active && (i0 + 3 < len);
    if (VEC && vec_row && full) {
      const float4 r4 = *reinterpret_cast<const float4*>(p.rew + start + i0);
      const float4 v4 = *reinterpret_cast<const float4*>(p.val + start + i0);
      r[0] = r4.x; r[1] = r4.y; r[2] = r4.z; r[3] = r4.w;
      v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
      if (p.bonus) {
        const float4 b4 = *reinterpret_cast<const float4*>(p.bonus + start + i0);
        b[0] = b4.x; b[1] = b4.y; b[2] = b4.z; b[3] = b4.w;
      }
      if (p.mode == 0) {
        const ushort4 t4 = *reinterpret_cast<const ushort4*>(p.tail + start + i0);
        tl[0] = t4.x; tl[1] = t4.y; tl[2] = t4.z; tl[3] = t4.w;
      }
    } else if (active) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < len) {
          r[j] = p.rew[start + i0 + j];
          v[j] = p.val[start + i0 + j];
          if (p.bonus) b[j] = p.bonus[start + i0 + j];
          if (p.mode == 0) tl[j] = p.tail[start + i0 + j];
        }
      }
    }
    if (p.mode == 1 && active) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j == len - 1) tl[j] = (int)len;
    }

    // V of the step to the right of this lane's last step.
    double vright = shfl_down_d((double)v[0], 1, lpr);
    if (sub == lpr - 1) vright = vnext_chunk;

    // Per-step affine maps  y_t = x_t + d_t * y_{t+1}; d_t is one of three
    // values, so only the offsets are kept in (fp64) registers.
    double xa[4];
    int kind[4];  // 0: beyond the row (identity), 1: episode end, 2: ordinary
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const bool valid = active && (i0 + j < len);
      const double vn = (j == 3) ? vright : (double)v[j + 1];
      const double rb = (double)r[j] + p.bonus_const + (double)b[j];
      if (!valid) {
        xa[j] = 0.0;
        kind[j] = 0;
      } else if (tl[j] > 0) {
        double boot;
        const double c0 = padded_tail_carry(p, v0, tl[j], &boot);
        xa[j] = rb + p.gamma * boot - (double)v[j] + p.c * c0;
        kind[j] = 1;
      } else {
        xa[j] = rb + p.gamma * vn - (double)v[j];
        kind[j] = 2;
      }
    }
    // Compose the lane's four maps (right to left).
    Pair A = {1.0, 0.0}, G = {1.0, 0.0};
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const double da = kind[j] == 2 ? p.c : (kind[j] == 1 ? 0.0 : 1.0);
      const double dg = kind[j] == 2 ? p.gamma_ret : (kind[j] == 1 ? 0.0 : 1.0);
      A.x = xa[j] + da * A.x;
      A.d = da * A.d;
      G.x = (double)r[j] + dg * G.x;
      G.d = dg * G.d;
    }
    // Inclusive suffix scan over the row group.
    for (int o = 1; o < lpr; o <<= 1) {
      const double ad = shfl_down_d(A.d, o, lpr), ax = shfl_down_d(A.x, o, lpr);
      const double gd = shfl_down_d(G.d, o, lpr), gx = shfl_down_d(G.x, o, lpr);
      if (sub + o < lpr) {
        A.x = A.x + A.d * ax;
        A.d = A.d * ad;
        G.x = G.x + G.d * gx;
        G.d = G.d * gd;
      }
    }
    // Carry entering this lane from its right neighbour's suffix.
    double nad = shfl_down_d(A.d, 1, lpr), nax = shfl_down_d(A.x, 1, lpr);
    double ngd = shfl_down_d(G.d, 1, lpr), ngx = shfl_down_d(G.x, 1, lpr);
    double ya = carry_a, yg = carry_g;
    if (sub + 1 < lpr) {
      ya = nax + nad * carry_a;
      yg = ngx + ngd * carry_g;
    }
    float oa[4], og[4];
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      const double da = kind[j] == 2 ? p.c : (kind[j] == 1 ? 0.0 : 1.0);
      const double dg = kind[j] == 2 ? p.gamma_ret : (kind[j] == 1 ? 0.0 : 1.0);
      ya = xa[j] + da * ya;
      yg = (double)r[j] + dg * yg;
      oa[j] = (float)ya;
      og[j] = (float)yg;
    }
    if (VEC && vec_row && full) {
      sink.quad(row, start, i0, oa[0], oa[1], oa[2], oa[3]);
      *reinterpret_cast<float4*>(p.ret + start + i0) =
          make_float4(og[0], og[1], og[2], og[3]);
    } else if (active) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < len) {
          sink.one(row, start, i0 + j, oa[j]);
          p.ret[start + i0 + j] = og[j];
        }
      }
    }
    // Group-uniform carries for the chunk to the left.
    const double ca = __shfl(ya, 0, lpr), cg = __shfl(yg, 0, lpr);
    const double cv = __shfl((double)v[0], 0, lpr);
    if (active) {
      carry_a = ca;
      carry_g = cg;
      vnext_chunk = cv;
    }
  }
}

// The whole-episode kernel's wave.  NQ = quads (4 steps) per lane: 1 (up to 256 steps per
// 64-lane row group) or 2 (8 steps per lane: half the lanes, waves and shuffle steps per
// row)
template <int NQ, class AdvSink>
__device__ __forceinline__ void gae_scan_rows_wave(const RowsScanParams& p, double v0,
                                                   int64_t wave, int lane,
                                                   const AdvSink& sink) {
  constexpr int NS = 4 * NQ;
  const int lpr = p.lpr;
  const int sub = lane & (lpr - 1);
  const int64_t row = wave * (64 / lpr) + lane / lpr;
  const bool row_ok = row < p.n_rows;
  int64_t start = 0;
  int len = 0;
  if (row_ok) {
    if (p.offsets) {
      start = p.offsets[row];
      len = (int)(p.offsets[row + 1] - start);
    } else {
      start = row * p.ld;
      len = (int)p.T;
    }
  }
  const int i0 = NS * sub;
  const int nv = max(0, min(NS, len - i0));  // valid steps of this lane
  float rf[NS], vf[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) { rf[j] = 0.f; vf[j] = 0.f; }
  const bool vec = nv == NS && ((start + i0) & 3) == 0;
  if (vec) {
    float4 r4[NQ], v4[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      r4[q] = *reinterpret_cast<const float4*>(p.rew + start + i0 + 4 * q);
      v4[q] = *reinterpret_cast<const float4*>(p.val + start + i0 + 4 * q);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      rf[4 * q + 0] = r4[q].x; rf[4 * q + 1] = r4[q].y;
      rf[4 * q + 2] = r4[q].z; rf[4 * q + 3] = r4[q].w;
      vf[4 * q + 0] = v4[q].x; vf[4 * q + 1] = v4[q].y;
      vf[4 * q + 2] = v4[q].z; vf[4 * q + 3] = v4[q].w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (j < nv) {
        rf[j] = p.rew[start + i0 + j];
        vf[j] = p.val[start + i0 + j];
      }
    }
  }
  float vr = __shfl_down(vf[0], 1, lpr);
  if (sub == lpr - 1) vr = 0.f;
  // the row's last step: what the padded tail hands it (only that lane computes)
  double end_add = 0.0;
  const bool has_end = nv > 0 && i0 + nv == len;
  if (has_end) {
    const int m = p.P - len;
    if (m > 0) {
      const double pad_delta = p.bonus_const + (p.gamma - 1.0) * v0;
      double cm1 = 1.0, base = p.c;
      for (int e = m - 1; e > 0; e >>= 1) {
        if (e & 1) cm1 *= base;
        base *= base;
      }
      const double geo =
          (p.c == 1.0) ? (double)(m - 1) : (1.0 - cm1) / (1.0 - p.c);
      const double c0 = pad_delta * geo + cm1 * (p.bonus_const - v0);
      end_add = p.gamma * v0 + p.c * c0;
    }
  }
  double r[NS], xa[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    r[j] = (double)rf[j];
    const bool valid = j < nv;
    const bool last = has_end && j == nv - 1;
    const double vn =
        last ? 0.0 : (double)(j == NS - 1 ? vr : vf[j < NS - 1 ? j + 1 : NS - 1]);
    xa[j] = valid ? (r[j] + p.bonus_const) + p.gamma * vn - (double)vf[j] +
                        (last ? end_add : 0.0)
                  : 0.0;
    if (!valid) r[j] = 0.0;
  }
  double ax = xa[NS - 1], gx = r[NS - 1];
#pragma unroll
  for (int j = NS - 2; j >= 0; --j) {
    ax = xa[j] + p.c * ax;
    gx = r[j] + p.gamma_ret * gx;
  }
  // steps right of the row's end are zero maps with zero offsets: a lane that
  // holds the end must not pass anything on from them (they are zero already)
  int s = 0;
  for (int o = 1; o < lpr; o <<= 1, ++s) {
    const double nax = shfl_down_d(ax, o, lpr), ngx = shfl_down_d(gx, o, lpr);
    if (sub + o < lpr) {
      ax = ax + p.cpow[s] * nax;
      gx = gx + p.gpow[s] * ngx;
    }
  }
  double ya = shfl_down_d(ax, 1, lpr), yg = shfl_down_d(gx, 1, lpr);
  if (sub + 1 >= lpr) {
    ya = 0.0;
    yg = 0.0;
  }
  float oa[NS], og[NS];
#pragma unroll
  for (int j = NS - 1; j >= 0; --j) {
    ya = xa[j] + p.c * ya;
    yg = r[j] + p.gamma_ret * yg;
    oa[j] = (float)ya;
    og[j] = (float)yg;
  }
  if (vec) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      sink.quad(row, start, i0 + 4 * q, oa[4 * q], oa[4 * q + 1], oa[4 * q + 2],
                oa[4 * q + 3]);
      *reinterpret_cast<float4*>(p.ret + start + i0 + 4 * q) =
          make_float4(og[4 * q], og[4 * q + 1], og[4 * q + 2], og[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (j < nv) {
        sink.one(row, start, i0 + j, oa[j]);
        p.ret[start + i0 + j] = og[j];
      }
    }
  }
}

}  // namespace
