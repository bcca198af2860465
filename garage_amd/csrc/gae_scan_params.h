// What the host says to the returns / GAE(lambda) scan kernels (gae_scan_body.h), and the
// ONE rule that picks the kernel for a set of arguments: ga_gae_scan_f32 (gae_scan.hip)
// launches what it names, ga_advantages_members_f32 (members_advantage_host.cpp) writes it
// into every member's table entry, so a member's rows take the arithmetic its lone launch
// would.  Host C++ only (no device code).  Not part of the C ABI.
#pragma once
#include <stdint.h>

#include "common.h"

struct ScanParams {
  const float* rew;
  const float* val;
  const float* bonus;      // optional per-step reward bonus (entropy 'max')
  const uint16_t* tail;    // mode 0: episode length at episode ends, else 0
  const int64_t* offsets;  // optional row starts (n_rows + 1), else row * ld
  int64_t n_rows, T, ld;
  int lpr;                 // lanes per row
  int mode;                // 0: tail flags, 1: row == one episode
  int P;                   // env_spec.max_episode_length (padding length)
  double gamma, c;         // fp32-rounded discount, discount * gae_lambda
  double gamma_ret;        // discount as the float64 lfilter sees it
  double v0;               // V(zero observation): content of padded baselines
  double bonus_const;      // constant reward bonus, padded cells included
  float* adv;
  float* ret;
};

struct RowsScanParams {
  const float* rew;
  const float* val;
  const int64_t* offsets;  // n_rows + 1 row starts, or null: row * ld, length T
  int64_t n_rows, T, ld;
  int lpr, P;
  double gamma, c, gamma_ret, bonus_const, v0;
  double cpow[6], gpow[6];
  float* adv;
  float* ret;
};

enum GaScanKernel {
  GS_GENERAL = 0,      // gae_scan_kernel<false>
  GS_GENERAL_VEC = 1,  // gae_scan_kernel<true>
  GS_ROWS_1 = 2,       // gae_scan_rows_kernel<1>
  GS_ROWS_2 = 3,       // gae_scan_rows_kernel<2>
};

struct GaScanPlan {
  int kernel;       // GaScanKernel
  int64_t waves;    // waves of the lone launch that hold rows (four to a workgroup)
  ScanParams p;     // GS_GENERAL, GS_GENERAL_VEC
  RowsScanParams f; // GS_ROWS_1, GS_ROWS_2
};

// gae_scan.hip: the developer switches (ga_set_gae_fixed_fast_path,
// ga_set_gae_rows_steps_per_lane) as they stand
int ga_gae_fixed_fast_path(void);
int ga_gae_rows_steps_per_lane(void);

// The kernel and its parameters for checked arguments (n_rows >= 1, max_len >= 1; without
// offsets max_len == T).
inline void ga_gae_scan_plan(const float* rewards, const float* values, const float* bonus,
                             const uint16_t* tail, const int64_t* offsets, int64_t n_rows,
                             int64_t T, int64_t ld, int64_t max_len, int mode,
                             int max_episode_length, double discount, double gae_lambda,
                             double v0, float bonus_const, float* adv, float* ret,
                             GaScanPlan* out) {
  int lpr = 1;
  while (lpr < 64 && (int64_t)lpr * 4 < max_len) lpr <<= 1;

  ScanParams& p = out->p;
  p.rew = rewards; p.val = values; p.bonus = bonus; p.tail = tail;
  p.offsets = offsets; p.n_rows = n_rows; p.T = T; p.ld = ld; p.lpr = lpr;
  p.mode = mode; p.P = max_episode_length;
  // gamma * lambda is formed in fp32 like the reference's filter seed
  // (torch.full(..., discount * gae_lambda, dtype=float), torch/_functions.py:75)
  // and the deltas use the fp32-rounded discount (vpg.py:166 -> :80), while the
  // returns come from a float64 lfilter (np/_functions.py:127).
  p.gamma = (double)(float)discount;
  p.gamma_ret = discount;
  p.c = (double)(float)(discount * gae_lambda);
  p.v0 = v0; p.bonus_const = (double)bonus_const;
  p.adv = adv; p.ret = ret;
  out->waves = ga_ceil_div(n_rows, 64 / lpr);

  const bool aligned = ga_aligned16(rewards) && ga_aligned16(values) &&
                       ga_aligned16(adv) && ga_aligned16(ret) &&
                       (!bonus || ga_aligned16(bonus));
  // whole-episode rows of at most 256 steps: the constant-decay kernel (its lanes
  // decide on 16-B accesses from the step index alone, so the bases must be aligned)
  if (ga_gae_fixed_fast_path() && mode == 1 && !bonus && max_len <= 256 && aligned) {
    const int nq = (ga_gae_rows_steps_per_lane() == 8 && max_len > 4) ? 2 : 1;
    int flpr = 1;
    while (flpr < 64 && (int64_t)flpr * 4 * nq < max_len) flpr <<= 1;
    RowsScanParams& f = out->f;
    f.rew = rewards; f.val = values; f.offsets = offsets; f.n_rows = n_rows; f.T = T;
    f.ld = ld; f.lpr = flpr; f.P = max_episode_length; f.gamma = p.gamma; f.c = p.c;
    f.gamma_ret = p.gamma_ret; f.bonus_const = p.bonus_const; f.v0 = p.v0;
    f.adv = adv; f.ret = ret;
    // decay over one lane's steps, then squared per scan step
    double cd = 1.0, gd = 1.0;
    for (int k = 0; k < 4 * nq; ++k) {
      cd *= p.c;
      gd *= discount;
    }
    for (int k = 0; k < 6; ++k) {
      f.cpow[k] = cd;
      f.gpow[k] = gd;
      cd *= cd;
      gd *= gd;
    }
    out->kernel = nq == 2 ? GS_ROWS_2 : GS_ROWS_1;
    out->waves = ga_ceil_div(n_rows, 64 / flpr);
    return;
  }
  const bool vec = (offsets || ld % 4 == 0) && aligned &&
                   (!tail || (reinterpret_cast<uintptr_t>(tail) & 7u) == 0);
  out->kernel = vec ? GS_GENERAL_VEC : GS_GENERAL;
}
