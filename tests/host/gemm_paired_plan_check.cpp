// Which weight-gradient products take gemm_rr_paired_kernel: the rule of
// layer_plans.h (ga_gemm_paired_ok, GemmPlan::paired_cols) against a literal table, one
// refused product per condition, on the CPU (`make paired-plan-check`, AddressSanitizer +
// UBSan).  Whatever the flag says, tile, grid, threads, k_per_split and the profiling kind
// are those of gemm_f32_kernel<128, 128, 2, 4, false, false>.  No pointer is dereferenced.
#include <cstdio>
#include <cstdlib>

#include "../../garage_amd/csrc/layer_plans.h"

namespace {
alignas(16) float g_a[8], g_b[8], g_c[8];
int32_t g_idx[4];
int g_failures = 0;

// dW = dZ^T H: out_w x in_w from `rows` rows in slabs of `kps`
GemmParams wgrad(int out_w, int in_w, int rows, int kps) {
  GemmParams p = {};
  p.A = g_a; p.lda = out_w;
  p.B = g_b; p.ldb = in_w;
  p.C = g_c; p.c_rs = in_w; p.c_cs = 1;
  p.M = out_w; p.N = in_w; p.K = rows;
  p.epi = EPI_PLAIN;
  p.k_per_split = kps;
  p.c_split_stride = 4 + (int64_t)out_w * in_w + out_w;
  p.colsum = g_c; p.colsum_split_stride = p.c_split_stride;
  return p;
}

const GemmSwitches kOn = {false, false, false, true};
const GemmSwitches kOff = {false, false, false, false};

void expect(const char* what, const GemmParams& p, int a_kc, int b_kc, int splits,
            const GemmSwitches& sw, bool paired, GemmTile tile = GT_128x128) {
  const GemmPlan g = ga_gemm_plan(p, a_kc, b_kc, splits, sw);
  bool ok = g.paired_cols == paired && g.tile == tile;
  if (tile == GT_128x128)
    ok = ok && g.gx == (p.M + 127) / 128 && g.gy == (p.N + 127) / 128 && g.gz == splits &&
         g.threads == 512 && g.k_per_split == p.k_per_split &&
         g.prof_kind == GA_PROF_GEMM_NT_128 + ((a_kc && b_kc) ? 0 : (a_kc ? 1 : 2));
  if (!ok) {
    std::printf("FAILED %s: paired %d (want %d) tile %d grid %d %d %d threads %d kps %d\n",
                what, (int)g.paired_cols, (int)paired, (int)g.tile, g.gx, g.gy, g.gz,
                g.threads, g.k_per_split);
    ++g_failures;
  }
}
}  // namespace

int main() {
  // ---- taken
  expect("the bench's middle layer", wgrad(256, 256, 32768, 256), 0, 0, 128, kOn, true);
  expect("512-wide layers", wgrad(512, 512, 65536, 1024), 0, 0, 64, kOn, true);
  expect("one tile, one slab", wgrad(128, 128, 256, 256), 0, 0, 1, kOn, true);
  expect("ragged last slab", wgrad(256, 128, 520, 192), 0, 0, 3, kOn, true);
  expect("three row tiles", wgrad(384, 128, 512, 256), 0, 0, 2, kOn, true);
  {
    GemmParams p = wgrad(256, 256, 4096, 256);
    p.lda = 260; p.ldb = 264; p.c_rs = 258; p.c_split_stride = 70000;
    expect("leading dimensions beyond the widths", p, 0, 0, 16, kOn, true);
    p.colsum = nullptr;
    expect("no column sums", p, 0, 0, 16, kOn, true);
    p.lda = (1ll << 22) - 4;  // 256 rows of it: just below 2^32, beyond 2^31
    expect("slab rows beyond 2^31 bytes", p, 0, 0, 16, kOn, false);
    p.lda = (1ll << 21) - 4; p.k_per_split = 224;
    expect("slab rows just inside 2^31 bytes", p, 0, 0, 19, kOn, true);
  }
  // ---- the switch
  expect("switch off", wgrad(256, 256, 32768, 256), 0, 0, 128, kOff, false);
  // ---- refused, one condition each
  const GemmParams base = wgrad(256, 256, 4096, 256);
  GemmParams p = base;
  expect("forward orientation", p, 1, 1, 1, kOn, false);
  expect("data-gradient orientation", p, 1, 0, 1, kOn, false);
  p = base; p.a_idx = g_idx;
  expect("gathered A", p, 0, 0, 16, kOn, false);
  p = base; p.b_idx = g_idx;
  expect("gathered B", p, 0, 0, 16, kOn, false);
  p = base; p.epi = EPI_BIAS_ACT;
  expect("bias + activation epilogue", p, 0, 0, 16, kOn, false);
  p = base; p.epi = EPI_MUL_DTANH; p.H = g_a; p.ldh = 256;
  expect("slope epilogue", p, 0, 0, 16, kOn, false);
  p = base; p.accum = 1;
  expect("accumulating", p, 0, 0, 16, kOn, false);
  p = base; p.H = g_a;
  expect("H set", p, 0, 0, 16, kOn, false);
  p = base; p.bias = g_a;
  expect("bias set", p, 0, 0, 16, kOn, false);
  p = base; p.head_W = g_a;
  expect("head set", p, 0, 0, 16, kOn, false);
  expect("M no multiple of 128", wgrad(192, 128, 512, 256), 0, 0, 2, kOn, false);
  expect("N no multiple of 128", wgrad(256, 192, 512, 256), 0, 0, 2, kOn, false);
  expect("N = 130 (padded rows)", wgrad(256, 130, 512, 256), 0, 0, 2, kOn, false);
  p = base; p.c_rs = 1; p.c_cs = 256;
  expect("column-major C", p, 0, 0, 16, kOn, false);
  p = base; p.c_rs = 257;
  expect("odd leading dimension of C", p, 0, 0, 16, kOn, false);
  p = base; p.C = g_c + 1;
  expect("C at 4 B beyond 8", p, 0, 0, 16, kOn, false);
  p = base; p.C = g_c + 2;
  expect("C 8-B aligned", p, 0, 0, 16, kOn, true);
  p = base; p.c_split_stride += 1;
  expect("odd slab stride", p, 0, 0, 16, kOn, false);
  p = base; p.lda = 258;
  expect("lda no multiple of 4", p, 0, 0, 16, kOn, false);
  p = base; p.A = g_a + 1;
  expect("A not 16-B aligned", p, 0, 0, 16, kOn, false);
  p = base; p.ldb = 1ll << 22;
  expect("ldb of 2^22 floats", p, 0, 0, 16, kOn, false);
  p = base; p.c_rs = 1ll << 22;
  expect("c_rs of 2^22 floats", p, 0, 0, 16, kOn, false);
  // ---- the arms in front of the 128 x 128 tile keep their products
  {
    const GemmSwitches small_m = {true, false, false, true};
    expect("one slab with the small-M tiles on", wgrad(128, 128, 256, 256), 0, 0, 1, small_m,
           false, GT_SMALL_M);
    const GemmSwitches split = {false, false, true, true};
    expect("split-operand weight gradient", base, 0, 0, 16, split, false, GT_NT_SPLIT);
    expect("64-wide", wgrad(128, 64, 512, 256), 0, 0, 2, kOn, false, GT_64x64);
  }
  if (g_failures) {
    std::printf("%d failed\n", g_failures);
    return 1;
  }
  std::printf("paired plan ok\n");
  return 0;
}
