// Host-logic harness for the per-layer MLP dispatch (garage_amd/csrc/mlp_layers.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-mlp`).  The dispatch and
// the plans it asks (garage_amd/csrc/layer_plans.h: which kernel takes a product, with
// which grid) are the library's own; every launch below them -- the five entries of the
// launch seam, the LayerNorm passes, the one-launch forwards -- is replaced by a fake
// that records the call and never dereferences a device pointer.  Instead each fake
// works out the extent its kernel would reach (operand rows x ld through the gather's
// largest index, C through its strides and splits, column sums, bias, H, the head
// operands, the weight planes, LayerNorm statistics) and checks it against the
// exactly-sized heap buffer the pointer came from, and checks that the plan's grid covers
// the product with its tile.  A miss is a failure.  The checks are about the dispatch's
// own arithmetic: where a layer's operands sit in the flat layouts (built the way
// garage_amd/engine.py builds them), which kernel a layer takes by default, with each
// developer switch flipped and at shapes a kernel refuses, that ga_wgrad_mid and
// ga_mlp_backward_range_f32 describe the middle layer's weight gradient alike, and the
// plans themselves against literal tables with both sides of every boundary.
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/layer_plans.h"
#include "../../garage_amd/csrc/internal.h"
#include "harness.h"

// ---- "device" buffers: exactly-sized heap blocks, known to the fakes -------------
struct Region {
  const char* lo;
  const char* hi;
};
static std::vector<Region> g_regions;
static int g_extent_errors = 0;

template <class T>
struct Buf {
  T* p;
  explicit Buf(int64_t n) {
    void* v = nullptr;
    const size_t bytes = sizeof(T) * (size_t)(n > 0 ? n : 1);
    if (posix_memalign(&v, 16, bytes)) abort();
    memset(v, 0, bytes);
    p = (T*)v;
    g_regions.push_back({(const char*)p, (const char*)p + bytes});
  }
  ~Buf() {
    for (size_t i = 0; i < g_regions.size(); ++i)
      if (g_regions[i].lo == (const char*)p) {
        g_regions.erase(g_regions.begin() + (long)i);
        break;
      }
    free(p);
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
};

// the kernel reads or writes `n` elements of `elem` bytes from `ptr` on
static void reach(const void* ptr, int64_t n, size_t elem, const char* what) {
  const char* p = (const char*)ptr;
  for (const Region& r : g_regions)
    if (p >= r.lo && p < r.hi) {
      if (n < 0 || p + (size_t)n * elem > r.hi) {
        fprintf(stderr, "extent: %s reaches %lld bytes past its buffer\n", what,
                (long long)(p + (size_t)n * elem - r.hi));
        ++g_extent_errors;
      }
      return;
    }
  fprintf(stderr, "extent: %s points into no buffer\n", what);
  ++g_extent_errors;
}
static void reach_f(const float* p, int64_t n, const char* what) { reach(p, n, 4, what); }
// `lines` memory lines of `span` valid floats (fetched as 16-B vectors), `ld` floats
// apart, through an optional gather of the line index
static void reach_lines(const float* base, int64_t ld, const int32_t* idx, int64_t lines,
                        int64_t span, const char* what) {
  int64_t last = lines - 1;
  if (idx) {
    reach(idx, lines, 4, "gather index");
    last = 0;
    for (int64_t i = 0; i < lines; ++i) last = idx[i] > last ? idx[i] : last;
  }
  if (ld < ((span + 3) & ~3)) {
    fprintf(stderr, "extent: %s: ld %lld below round4(%lld)\n", what, (long long)ld,
            (long long)span);
    ++g_extent_errors;
  }
  reach_f(base, last * ld + ((span + 3) & ~3), what);
}

// ---- the record -------------------------------------------------------------------
struct Call {
  std::string kind;
  GemmParams p;        // the GEMM launches
  int tile;            // ... and their plan's tile
  int splits;
  const float* C;      // what the launch writes first (slab, data gradient, output)
  const float* dz_out; // skinny_wgrad: the fused data gradient
  int want_dx;         // ln_bwd
};
static std::vector<Call> g_calls;
static Call& record(const char* kind) {
  Call c = {};
  c.kind = kind;
  g_calls.push_back(c);
  return g_calls.back();
}
static std::vector<std::string> kinds() {
  std::vector<std::string> k;
  for (auto& c : g_calls) k.push_back(c.kind);
  return k;
}
static int calls_of(const char* kind) {
  int n = 0;
  for (auto& c : g_calls) n += c.kind == kind;
  return n;
}

// (ga_policy_step_fused_supported answers g_policy_step_fused_ok: harness.h)
static int g_eval_ok = 1;
// the split-operand switches of fused_train_host.cpp
static int g_split_gemm = 0, g_split_wgrad = 0;

static void grid_error(const char* what) {
  fprintf(stderr, "extent: %s\n", what);
  ++g_extent_errors;
}

static void gemm_extents(const GemmParams& p, int a_kc, int b_kc, int splits) {
  if (p.k_per_split % BK != 0 || (int64_t)p.k_per_split * splits < p.K || p.M < 1 ||
      p.N < 1 || p.K < 1) {
    fprintf(stderr, "extent: k_per_split %d x %d splits against K %d\n", p.k_per_split,
            splits, p.K);
    ++g_extent_errors;
  }
  if (a_kc) reach_lines(p.A, p.lda, p.a_idx, p.M, p.K, "A");
  else reach_lines(p.A, p.lda, p.a_idx, p.K, p.M, "A (k lines)");
  if (b_kc) reach_lines(p.B, p.ldb, p.b_idx, p.N, p.K, "B");
  else reach_lines(p.B, p.ldb, p.b_idx, p.K, p.N, "B (k lines)");
  reach_f(p.C, (splits - 1) * p.c_split_stride + (p.M - 1) * p.c_rs + (p.N - 1) * p.c_cs + 1,
          "C");
  if (p.colsum)
    reach_f(p.colsum, (splits - 1) * p.colsum_split_stride + (p.colsum_of_b ? p.N : p.M),
            "colsum");
  if (p.epi == EPI_BIAS_ACT && p.bias) reach_f(p.bias, p.N, "bias");
  if (p.H) reach_f(p.H, (int64_t)(p.M - 1) * p.ldh + p.N, "H");
}
// gx x gy tiles of bm x bn cover M x N, none of them empty
static void grid_covers(const GemmParams& p, int bm, int bn) {
  if (p.gx < 1 || p.gy < 1 || (int64_t)p.gx * bm < p.M || (int64_t)(p.gx - 1) * bm >= p.M ||
      (int64_t)p.gy * bn < p.N || (int64_t)(p.gy - 1) * bn >= p.N)
    grid_error("the grid does not cover M x N with its tile");
}

// ---- fakes of gemm.hip's launch seam (layer_plans.h) -------------------------------
// (the tile shapes, as literals)
static const struct { int bm, bn, threads; } TILES[6] = {
    {64, 64, 256}, {128, 32, 256}, {64, 64, 256}, {128, 128, 512}, {128, 128, 512},
    {128, 128, 512}};
int ga_gemm_launch(const GemmPlan& plan, const GemmParams& p, hipStream_t) {
  char kind[16];
  snprintf(kind, sizeof(kind), "gemm%d%d", plan.a_kc, plan.b_kc);
  Call& c = record(kind);
  c.p = p; c.tile = plan.tile; c.splits = p.gz; c.C = p.C;
  if (p.gx != plan.gx || p.gy != plan.gy || p.gz != plan.gz || p.gz < 1 ||
      p.k_per_split != plan.k_per_split || plan.threads != TILES[plan.tile].threads)
    grid_error("GemmParams and its plan disagree");
  grid_covers(p, TILES[plan.tile].bm, TILES[plan.tile].bn);
  gemm_extents(p, plan.a_kc, plan.b_kc, p.gz);
  if (plan.tile == GT_NT_SPLIT && (p.M % 128 || p.N % 128 || p.a_idx || p.b_idx))
    grid_error("the split-operand weight gradient masks nothing");
  if ((plan.tile == GT_KC_SPLIT) != (p.bplanes != nullptr))
    grid_error("weight planes exactly for the split-operand k-loop");
  if (p.bplanes) {
    // fragments of every 32-column block the grid touches, every 16-deep k group
    const int64_t np = (p.N + 31) & ~31, kp = (p.K + 31) & ~31;
    if (p.bplane_nblk != np / 32 || p.bplane_stride != np * kp || p.gz != 1)
      grid_error("plane geometry");
    reach(p.bplanes, 3 * p.bplane_stride, 2, "weight planes");
  }
  return 0;
}
int ga_gemm_head_launch(const GemmHeadPlan& plan, const GemmParams& p, hipStream_t) {
  Call& c = record("gemm_head");
  c.p = p; c.splits = 1; c.C = p.C;
  if (!plan.taken || plan.width != p.N || p.gx != plan.gx || p.gy != 1 || p.gz != 1 ||
      (int64_t)p.gx * 64 != p.M || plan.threads != (p.N == 256 ? 512 : 256))
    grid_error("head launch: 64-row tiles over whole rows");
  gemm_extents(p, 1, 1, 1);
  reach_lines(p.head_W, p.head_ldw, nullptr, p.head_n, p.N, "head W");
  reach_f(p.head_bias, p.head_n, "head bias");
  reach_f(p.head_out, (int64_t)(p.M - 1) * p.head_ld + p.head_n, "head out");
  return 0;
}
int ga_gemm_pair_launch(const GemmPairPlan& plan, const GemmParams& a, const GemmParams& b,
                        hipStream_t) {
  for (const GemmParams* p : {&a, &b}) {
    Call& c = record("gemm_pair");
    c.p = *p; c.tile = GT_128x128; c.splits = p->gz; c.C = p->C;
    if (!plan.taken || p->gx != plan.gx || p->gy != plan.gy || p->gz != plan.gz)
      grid_error("pair launch: GemmParams and the plan disagree");
    grid_covers(*p, 128, 128);
    gemm_extents(*p, 0, 0, p->gz);
  }
  return 0;
}

// ---- skinny.hip's -------------------------------------------------------------------
int ga_skinny_fwd_launch(const SkinnyFwdPlan& plan, const SkinnyFwdParams& p, hipStream_t) {
  Call& c = record(plan.w_kc ? "skinny_fwd" : "skinny_dgrad");
  c.C = p.Y;
  const int n_rg = p.qpr > 0 ? 256 / p.qpr : 0;
  const int64_t rows_wg = (int64_t)n_rg * p.rows_per_thread;
  if (!plan.taken || p.qpr < 1 || 256 % p.qpr != 0 || p.qpr != plan.qpr ||
      p.rows_per_thread < 4 || p.rows_per_thread % 4 != 0 ||
      p.rows_per_thread != plan.rows_per_thread || plan.KV != (p.K + 3) / 4 || plan.KV > 8 ||
      plan.gx * rows_wg < p.M || (plan.gx - 1) * rows_wg >= p.M ||
      (int64_t)plan.gy * 4 * p.qpr < p.N || (int64_t)(plan.gy - 1) * 4 * p.qpr >= p.N ||
      plan.lds_bytes != rows_wg * plan.KV * 16 || plan.lds_bytes > 48 * 1024 ||
      plan.epi != (p.H ? 1 : 0) || plan.w_kc != (p.H == nullptr) || p.N % 4 != 0)
    grid_error("skinny forward: grid, rows per workgroup or LDS bytes");
  reach_lines(p.X, p.ldx, p.idx, p.M, p.K, "skinny X");
  if (plan.w_kc) reach_lines(p.W, p.ldw, nullptr, p.N, p.K, "skinny W");
  else reach_lines(p.W, p.ldw, nullptr, p.K, p.N, "skinny W (k lines)");
  if (p.bias) reach_f(p.bias, p.N, "skinny bias");
  if (p.H) reach_f(p.H, (int64_t)(p.M - 1) * p.ldh + p.N, "skinny H");
  reach_f(p.Y, (int64_t)(p.M - 1) * p.ldy + p.N, "skinny Y");
  return 0;
}
int ga_skinny_wgrad_launch(const SkinnyWgradPlan& plan, const SkinnyWgradParams& p,
                           hipStream_t) {
  Call& c = record(plan.variant == SWV_DZ ? "skinny_wgrad+dz" : "skinny_wgrad");
  c.C = p.C; c.dz_out = p.dz_out; c.splits = p.n_splits;
  if (!plan.taken || p.qpr < 1 || 256 % p.qpr != 0 || p.qpr > 16 || p.qpr != plan.qpr ||
      p.n_colblk != plan.n_colblk || (int64_t)p.n_colblk * 4 * p.qpr < p.wide ||
      (int64_t)(p.n_colblk - 1) * 4 * p.qpr >= p.wide ||
      plan.grid != (unsigned)(p.n_colblk * p.n_splits) || plan.NV != (p.NS + 3) / 4 ||
      plan.NV > 6 || (plan.variant == SWV_DZ) != (p.dz_out != nullptr) ||
      (plan.variant == SWV_DZ && (plan.NV > 4 || !p.Wn || !p.colsum_narrow)) ||
      (plan.variant == SWV_PLAIN) != (p.colsum_narrow == nullptr) || p.wide % 4 != 0)
    grid_error("skinny weight gradient: grid, column blocks or variant");
  if (p.rows_per_split % BK != 0 || (int64_t)p.rows_per_split * p.n_splits < p.rows)
    grid_error("skinny_wgrad rows_per_split");
  reach_lines(p.Wd, p.ldw, p.w_idx, p.rows, p.wide, "skinny wide");
  reach_lines(p.Nr, p.ldn, p.n_idx, p.rows, p.NS, "skinny narrow");
  const int64_t split_off = (p.n_splits - 1) * p.split_stride;
  reach_f(p.C, split_off + (p.wide - 1) * p.c_wide_stride + (p.NS - 1) * p.c_narrow_stride + 1,
          "skinny dW");
  if (p.colsum_wide) reach_f(p.colsum_wide, split_off + p.wide, "skinny colsum (wide)");
  if (p.colsum_narrow) reach_f(p.colsum_narrow, split_off + p.NS, "skinny colsum (narrow)");
  if (p.Wn) {
    reach_lines(p.Wn, p.ldwn, nullptr, p.NS, p.wide, "skinny head W");
    reach_f(p.dz_out, (int64_t)(p.rows - 1) * p.lddz + p.wide, "skinny dz out");
  }
  return 0;
}

// ---- lnorm.hip ----------------------------------------------------------------------
int ga_ln_forward(const float* X, int64_t ldx, const int32_t* idx, int64_t M, int D,
                  const float* gamma, const float* beta, float* Y, int64_t ldy, float* stats,
                  hipStream_t) {
  Call& c = record("ln_fwd");
  c.C = Y;
  reach_lines(X, ldx, idx, M, D, "ln X");
  reach_f(gamma, D, "gamma");
  reach_f(beta, D, "beta");
  reach_lines(Y, ldy, nullptr, M, D, "ln Y");
  reach_f(stats, 2 * M, "ln stats");
  return 0;
}
int ga_ln_backward(float* dY, int64_t ldd, const float* X, int64_t ldx, const int32_t* idx,
                   const float* stats, int64_t M, int D, const float* gamma, int want_dx, int,
                   int rows_per_split, int n_splits, float* dgamma, float* dbeta,
                   int64_t split_stride, hipStream_t) {
  Call& c = record("ln_bwd");
  c.C = dY; c.want_dx = want_dx; c.splits = n_splits;
  if (rows_per_split % BK != 0 || (int64_t)rows_per_split * n_splits < M) ++g_extent_errors;
  reach_lines(dY, ldd, nullptr, M, D, "ln dY");
  reach_lines(X, ldx, idx, M, D, "ln X");
  reach_f(stats, 2 * M, "ln stats");
  reach_f(gamma, D, "gamma");
  reach_f(dgamma, (n_splits - 1) * split_stride + D, "dgamma");
  reach_f(dbeta, (n_splits - 1) * split_stride + D, "dbeta");
  return 0;
}
int ga_ln_jvp(const float* tX, int64_t ldt, const float* X, int64_t ldx, const int32_t* idx,
              const float* stats, int64_t M, int D, const float* gamma, const float* tgamma,
              const float* tbeta, float* tY, int64_t ldy, hipStream_t) {
  Call& c = record("ln_jvp");
  c.C = tY;
  if (tX) reach_lines(tX, ldt, nullptr, M, D, "ln tX");
  reach_lines(X, ldx, idx, M, D, "ln X");
  reach_f(stats, 2 * M, "ln stats");
  reach_f(gamma, D, "gamma");
  reach_f(tgamma, D, "tgamma");
  reach_f(tbeta, D, "tbeta");
  reach_lines(tY, ldy, nullptr, M, D, "ln tY");
  return 0;
}

// ---- the one-launch forwards and the predicates ------------------------------------
extern "C" {
int ga_fused_eval_supported(int n_layers, const int*) { return g_eval_ok && n_layers == 3; }
int ga_fused_eval_forward(const float* X, int64_t ldx, const int32_t* idx, int64_t M,
                          const int* dims, const float* W1, const float* b1,
                          const float* W2, const float* b2, const float* Wh, const float* bh,
                          float* out, int64_t ldo, hipStream_t) {
  Call& c = record("eval_fwd");
  c.C = out;
  reach_lines(X, ldx, idx, M, dims[0], "eval X");
  reach_lines(W1, (dims[0] + 3) & ~3, nullptr, dims[1], dims[0], "eval W1");
  reach_lines(W2, (dims[1] + 3) & ~3, nullptr, dims[2], dims[1], "eval W2");
  reach_lines(Wh, (dims[2] + 3) & ~3, nullptr, dims[3], dims[2], "eval Wh");
  reach_f(b1, dims[1], "eval b1");
  reach_f(b2, dims[2], "eval b2");
  reach_f(bh, dims[3], "eval bh");
  reach_f(out, (M - 1) * ldo + dims[3], "eval out");
  return 0;
}
int ga_mlp_forward_fused_f32(const ga_mlp_desc*, const float*, const float*, int64_t,
                             const int32_t*, int64_t, float*, float* out, int64_t,
                             ga_stream_t) {
  record("fused_fwd").C = out;
  return 0;
}
int ga_split_bf16_enabled(void) { return g_split_wgrad; }
int ga_split_bf16_gemm(void) { return g_split_gemm; }
// three planes of round32(rows) x round32(cols) bf16, exactly
static std::vector<Buf<uint16_t>*> g_planes;
static int g_planes_bwd = -1;  // the orientation last asked for
const uint16_t* ga_weight_planes(const float* W, int64_t ld, int rows, int cols, int bwd,
                                 hipStream_t) {
  reach_lines(W, ld, nullptr, rows, cols, "planes W");
  g_planes_bwd = bwd;
  g_planes.push_back(new Buf<uint16_t>(3 * (int64_t)((rows + 31) & ~31) * ((cols + 31) & ~31)));
  return g_planes.back()->p;
}
}  // extern "C"
static void free_planes() {
  for (auto* b : g_planes) delete b;
  g_planes.clear();
}

// ---- networks: the flat layouts of garage_amd/engine.py ----------------------------
struct Net {
  ga_mlp_desc d;
  int L;
  int64_t n_flat, act_width, ld_out;
  int64_t act_row[8], lnx_row[8], lns_row[8];  // per-row offsets, times the capacity
  Net(std::vector<int> dims, int hidden_act = 0, int output_act = 0, int layer_norm = 0) {
    memset(&d, 0, sizeof(d));
    L = (int)dims.size() - 1;
    d.n_layers = L;
    d.hidden_act = hidden_act; d.output_act = output_act; d.layer_norm = layer_norm;
    for (int i = 0; i <= L; ++i) d.dims[i] = dims[(size_t)i];
    int64_t off = 4;
    for (int l = 0; l < L; ++l) {
      d.w_off[l] = off; off += (int64_t)dims[(size_t)l + 1] * round4(dims[(size_t)l]);
      d.b_off[l] = off; off += round4(dims[(size_t)l + 1]);
    }
    if (layer_norm)
      for (int l = 0; l + 1 < L; ++l) { d.ln_off[l] = off; off += 2 * round4(dims[(size_t)l]); }
    n_flat = off;
    int64_t a = 0;
    for (int l = 0; l + 1 < L; ++l) { act_row[l] = a; a += round4(dims[(size_t)l + 1]); }
    if (layer_norm) {
      for (int l = 0; l + 1 < L; ++l) { lnx_row[l] = a; a += round4(dims[(size_t)l]); }
      for (int l = 0; l + 1 < L; ++l) { lns_row[l] = a; a += 4; }
    }
    act_width = a;
    ld_out = round4(dims[(size_t)L]);
  }
  void set_capacity(int64_t cap) {
    for (int l = 0; l + 1 < L; ++l) {
      d.act_off[l] = act_row[l] * cap;
      if (d.layer_norm) { d.lnx_off[l] = lnx_row[l] * cap; d.lns_off[l] = lns_row[l] * cap; }
    }
  }
};

static const int X_ROWS = 97;

// one network at one batch: every buffer at exactly the size the Python side gives it
struct Case {
  Net& net;
  int64_t M, n_splits;
  Buf<float> params, tangent, X, acts, dacts, tacts, out, dout, tout, slabs;
  Buf<int32_t> idx;
  bool gather;
  int64_t ldx;
  Case(Net& n, int64_t M_, bool gather_, int64_t n_splits_)
      : net(n), M(M_), n_splits(n_splits_), params(n.n_flat), tangent(n.n_flat),
        X((gather_ ? X_ROWS : M_) * round4(n.d.dims[0])), acts(M_ * n.act_width),
        dacts(M_ * n.act_width), tacts(M_ * n.act_width), out(M_ * n.ld_out),
        dout(M_ * n.ld_out), tout(M_ * n.ld_out), slabs(n_splits_ * n.n_flat), idx(M_),
        gather(gather_), ldx(round4(n.d.dims[0])) {
    net.set_capacity(M);
    for (int64_t i = 0; i < M; ++i) idx.p[i] = (int32_t)((X_ROWS - 1 + 92 * i) % X_ROWS);
    idx.p[M - 1] = X_ROWS - 1;
  }
  const int32_t* rows() const { return gather ? idx.p : nullptr; }
  int forward(bool with_out = true, bool with_acts = true) {
    return ga_mlp_forward_f32(&net.d, params.p, X.p, ldx, rows(), M,
                              with_acts ? acts.p : nullptr, with_out ? out.p : nullptr,
                              net.ld_out, nullptr);
  }
  int backward() {
    return ga_mlp_backward_f32(&net.d, params.p, X.p, ldx, rows(), M, acts.p, dout.p,
                               net.ld_out, dacts.p, slabs.p, net.n_flat, n_splits, nullptr);
  }
  int backward_range(int l_start, int fused_first) {
    return ga_mlp_backward_range_f32(&net.d, params.p, X.p, ldx, rows(), M, acts.p, dout.p,
                                     net.ld_out, dacts.p, slabs.p, net.n_flat, n_splits,
                                     l_start, fused_first, nullptr);
  }
  int jvp() {
    return ga_mlp_jvp_f32(&net.d, params.p, tangent.p, X.p, ldx, rows(), M, acts.p, tacts.p,
                          tout.p, net.ld_out, nullptr);
  }
  // which layer's slab region / which hidden layer's data gradient a launch writes
  int slab_layer(const float* C) const {
    const int64_t off = C - slabs.p;
    if (C < slabs.p || off >= net.n_flat) return -1;
    int l = -1;
    for (int k = 0; k < net.L; ++k)
      if (off >= net.d.w_off[k]) l = k;
    return l;
  }
  int dgrad_layer(const float* C) const {
    for (int k = 0; k + 1 < net.L; ++k)
      if (C == dacts.p + net.d.act_off[k]) return k;
    return -1;
  }
};

#define SAME(f) (a.f == b.f)
static bool same_params(const GemmParams& a, const GemmParams& b) {
  return SAME(A) && SAME(lda) && SAME(a_idx) && SAME(B) && SAME(ldb) && SAME(b_idx) &&
         SAME(C) && SAME(c_rs) && SAME(c_cs) && SAME(M) && SAME(N) && SAME(K) && SAME(epi) &&
         SAME(bias) && SAME(act) && SAME(H) && SAME(ldh) && SAME(hact) && SAME(accum) &&
         SAME(k_per_split) && SAME(c_split_stride) && SAME(colsum) && SAME(colsum_of_b) &&
         SAME(colsum_split_stride) && SAME(gx) && SAME(gy) && SAME(gz) && SAME(head_W) &&
         SAME(head_ldw) && SAME(head_bias) && SAME(head_n) && SAME(head_out) &&
         SAME(head_ld) && SAME(bplanes) && SAME(bplane_stride) && SAME(bplane_nblk);
}
// two launches are the same launch
static bool same_call(const Call& a, const Call& b) {
  return a.kind == b.kind && same_params(a.p, b.p) && a.tile == b.tile &&
         a.splits == b.splits && a.C == b.C &&
         a.dz_out == b.dz_out && a.want_dx == b.want_dx;
}

typedef std::vector<std::string> Kinds;

static void reset_switches() {
  ga_set_fused_forward(0);
  ga_set_eval_forward(1);
  ga_set_fused_head_forward(1);
  ga_set_fused_head_dgrad(1);
  ga_set_skinny_kernels(1);
  ga_set_small_m_gemm(1);
  g_split_gemm = g_split_wgrad = 0;
  g_eval_ok = g_policy_step_fused_ok = 1;
}

// ---- the plans against literal tables (layer_plans.h) -------------------------------
// Every row is a situation and what the library does with it, written out as numbers;
// boundaries come in pairs, the last value one side, the first value on the other.
alignas(16) static float g_mem[64];  // aligned operands that are never read
static int32_t g_idx[4];

// which field of the product a row sets on top of its shape
enum Twist {
  T_NONE, T_A_IDX, T_B_IDX, T_ACCUM, T_COLSUM, T_COLSUM_OF_B, T_HEAD_W, T_C_CS, T_H, T_EPI_BIAS,
  T_EPI_PLAIN, T_ACT2, T_HACT1, T_HEAD_N9, T_HEAD_LDW, T_C_RS, T_C_UNALIGNED, T_NO_NSUM, T_DZ,
  T_CNS, T_CWS
};
static GemmParams product(int M, int N, int K, int kps, Twist t) {
  GemmParams p = {};
  p.A = g_mem; p.lda = round4(K); p.B = g_mem; p.ldb = round4(K);
  p.C = g_mem; p.c_rs = round4(N); p.c_cs = 1;
  p.M = M; p.N = N; p.K = K;
  p.epi = EPI_PLAIN;
  p.k_per_split = kps;
  switch (t) {
    case T_A_IDX: p.a_idx = g_idx; break;
    case T_B_IDX: p.b_idx = g_idx; break;
    case T_ACCUM: p.accum = 1; break;
    case T_COLSUM: p.colsum = g_mem; break;
    case T_COLSUM_OF_B: p.colsum = g_mem; p.colsum_of_b = 1; break;
    case T_HEAD_W: p.head_W = g_mem; break;
    case T_C_CS: p.c_cs = 2; break;
    case T_EPI_BIAS: p.epi = EPI_BIAS_ACT; break;
    default: break;
  }
  return p;
}

static void gemm_plan_table() {
  const int S = 1, G = 2, W = 4;  // switches: small-M, split-operand GEMM, ... weight gradient
  const struct {
    int M, N, K, kps, a_kc, b_kc, splits, sw;
    Twist twist;
    int tile, gx, gy, gz, k_per_split, threads, prof;
  } rows[] = {
      // N = 32 | 33 and 64 | 65 (K <= 64: no small-M tiles)
      {200, 32, 32, 32, 1, 1, 1, S, T_NONE, GT_128x32, 2, 1, 1, 32, 256, 3},
      {200, 33, 32, 32, 1, 1, 1, S, T_NONE, GT_64x64, 4, 1, 1, 32, 256, 0},
      {200, 64, 32, 32, 1, 0, 1, S, T_NONE, GT_64x64, 4, 1, 1, 32, 256, 1},
      {200, 65, 32, 32, 1, 0, 1, S, T_NONE, GT_128x128, 2, 1, 1, 32, 512, 1},
      {200, 32, 32, 32, 1, 0, 1, S, T_NONE, GT_128x32, 2, 1, 1, 32, 256, 4},
      {200, 20, 500, 128, 0, 0, 4, S, T_NONE, GT_128x32, 2, 1, 4, 128, 256, 5},
      // small-M: 128 | 129 tiles of 128 x 128
      {16384, 128, 256, 256, 1, 1, 1, S, T_NONE, GT_SMALL_M, 256, 2, 1, 256, 256, 0},
      {16385, 128, 256, 256, 1, 1, 1, S, T_NONE, GT_128x128, 129, 1, 1, 256, 512, 0},
      {8192, 256, 256, 256, 1, 0, 1, S, T_NONE, GT_SMALL_M, 128, 4, 1, 256, 256, 1},
      {8193, 256, 256, 256, 1, 0, 1, S, T_NONE, GT_128x128, 65, 2, 1, 256, 512, 1},
      // ... K = 64 | 65, and the 128-deep k step rounds k_per_split up
      {64, 256, 64, 64, 1, 1, 1, S, T_NONE, GT_128x128, 1, 2, 1, 64, 512, 0},
      {64, 256, 65, 96, 1, 1, 1, S, T_NONE, GT_SMALL_M, 1, 4, 1, 128, 256, 0},
      {64, 256, 200, 224, 1, 1, 1, S, T_NONE, GT_SMALL_M, 1, 4, 1, 256, 256, 0},
      // ... M = 4096 | 4097 rows for narrow outputs
      {4096, 8, 256, 256, 1, 1, 1, S, T_NONE, GT_SMALL_M, 64, 1, 1, 256, 256, 0},
      {4097, 8, 256, 256, 1, 1, 1, S, T_NONE, GT_128x32, 33, 1, 1, 256, 256, 3},
      // ... splits 1 | 2
      {256, 256, 512, 512, 0, 0, 1, S, T_NONE, GT_SMALL_M, 4, 4, 1, 512, 256, 2},
      {256, 256, 512, 256, 0, 0, 2, S, T_NONE, GT_128x128, 2, 2, 2, 256, 512, 2},
      // ... the switch on | off; before every other arm, the split-operand one too
      {64, 256, 65, 96, 1, 1, 1, 0, T_NONE, GT_128x128, 1, 2, 1, 96, 512, 0},
      {64, 48, 65, 96, 1, 1, 1, S, T_NONE, GT_SMALL_M, 1, 1, 1, 128, 256, 0},
      {64, 48, 65, 96, 1, 1, 1, 0, T_NONE, GT_64x64, 1, 1, 1, 96, 256, 0},
      {1024, 128, 128, 128, 1, 1, 1, S | G, T_NONE, GT_SMALL_M, 16, 2, 1, 128, 256, 0},
      {32768, 256, 256, 256, 1, 1, 1, S | G, T_NONE, GT_KC_SPLIT, 256, 2, 1, 256, 512, 0},
      // the split-operand forward / data gradient: M 1023 | 1024, N 127 | 128, K 127 | 128
      {1024, 128, 128, 128, 1, 1, 1, G, T_NONE, GT_KC_SPLIT, 8, 1, 1, 128, 512, 0},
      {1023, 128, 128, 128, 1, 1, 1, G, T_NONE, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 127, 128, 128, 1, 1, 1, G, T_NONE, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 127, 128, 1, 1, 1, G, T_NONE, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 124, 128, 1, 1, 1, G, T_NONE, GT_128x128, 8, 1, 1, 128, 512, 0},
      // ... K % 4; k_per_split is K rounded up to 32
      {1024, 128, 130, 160, 1, 1, 1, G, T_NONE, GT_128x128, 8, 1, 1, 160, 512, 0},
      {1024, 128, 132, 132, 1, 1, 1, G, T_NONE, GT_KC_SPLIT, 8, 1, 1, 160, 512, 0},
      // ... the data gradient too, never the weight gradient, one split, the switch
      {1024, 256, 128, 128, 1, 0, 1, G, T_NONE, GT_KC_SPLIT, 8, 2, 1, 128, 512, 1},
      {1024, 256, 128, 128, 0, 0, 1, G, T_NONE, GT_128x128, 8, 2, 1, 128, 512, 2},
      {1024, 128, 256, 128, 1, 1, 2, G, T_NONE, GT_128x128, 8, 1, 2, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, W, T_NONE, GT_128x128, 8, 1, 1, 128, 512, 0},
      // ... and each of b_idx, accum, colsum, head_W, c_cs refuses it (a_idx does not)
      {1024, 128, 128, 128, 1, 1, 1, G, T_A_IDX, GT_KC_SPLIT, 8, 1, 1, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, G, T_B_IDX, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, G, T_ACCUM, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, G, T_COLSUM, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, G, T_HEAD_W, GT_128x128, 8, 1, 1, 128, 512, 0},
      {1024, 128, 128, 128, 1, 1, 1, G, T_C_CS, GT_128x128, 8, 1, 1, 128, 512, 0},
      // the split-operand weight gradient: M % 128, N % 128, k_per_split % 16
      {256, 384, 32768, 256, 0, 0, 128, W, T_NONE, GT_NT_SPLIT, 2, 3, 128, 256, 512, 2},
      {257, 384, 32768, 256, 0, 0, 128, W, T_NONE, GT_128x128, 3, 3, 128, 256, 512, 2},
      {256, 383, 32768, 256, 0, 0, 128, W, T_NONE, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 264, 0, 0, 128, W, T_NONE, GT_128x128, 2, 3, 128, 264, 512, 2},
      {256, 384, 32768, 272, 0, 0, 128, W, T_NONE, GT_NT_SPLIT, 2, 3, 128, 272, 512, 2},
      // ... the gathers, the transposed bias gradient, the epilogue, accumulation, the
      // orientation and the switch
      {256, 384, 32768, 256, 0, 0, 128, W, T_A_IDX, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 0, 0, 128, W, T_B_IDX, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 0, 0, 128, W, T_COLSUM, GT_NT_SPLIT, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 0, 0, 128, W, T_COLSUM_OF_B, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 0, 0, 128, W, T_EPI_BIAS, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 0, 0, 128, W, T_ACCUM, GT_128x128, 2, 3, 128, 256, 512, 2},
      {256, 384, 32768, 256, 1, 0, 128, W, T_NONE, GT_128x128, 2, 3, 128, 256, 512, 1},
      {256, 384, 32768, 256, 0, 0, 128, G, T_NONE, GT_128x128, 2, 3, 128, 256, 512, 2},
  };
  int i = 0;
  for (const auto& r : rows) {
    const GemmParams p = product(r.M, r.N, r.K, r.kps, r.twist);
    const GemmSwitches sw = {(r.sw & S) != 0, (r.sw & G) != 0, (r.sw & W) != 0};
    const GemmPlan g = ga_gemm_plan(p, r.a_kc, r.b_kc, r.splits, sw);
    const bool ok = g.tile == r.tile && g.gx == r.gx && g.gy == r.gy && g.gz == r.gz &&
                    g.k_per_split == r.k_per_split && g.threads == r.threads &&
                    g.prof_kind == r.prof && g.a_kc == r.a_kc && g.b_kc == r.b_kc &&
                    g.work == 2.0 * r.M * r.N * r.K && g.planes == (r.tile == GT_KC_SPLIT);
    if (!ok)
      fprintf(stderr, "gemm plan row %d: tile %d grid %d x %d x %d k_per_split %d threads %d "
              "prof %d planes %d\n", i, g.tile, g.gx, g.gy, g.gz, g.k_per_split, g.threads,
              g.prof_kind, (int)g.planes);
    CHECK(ok);
    ++i;
  }
  // the weight planes: orientation and geometry (both sides padded to 32)
  const GemmSwitches split = {false, true, false};
  GemmPlan g = ga_gemm_plan(product(1024, 128, 128, 128, T_NONE), 1, 1, 1, split);
  CHECK(g.planes && g.planes_bwd == 0 && g.bplane_stride == 16384 && g.bplane_nblk == 4);
  g = ga_gemm_plan(product(1024, 256, 132, 160, T_NONE), 1, 0, 1, split);
  CHECK(g.planes && g.planes_bwd == 1 && g.bplane_stride == 256 * 160 && g.bplane_nblk == 8);
  g = ga_gemm_plan(product(1024, 130, 128, 128, T_NONE), 1, 1, 1, split);
  CHECK(g.planes && g.bplane_stride == 160 * 128 && g.bplane_nblk == 5 && g.gy == 2);
  GemmParams filled = product(1024, 130, 128, 128, T_NONE);
  ga_gemm_apply(g, &filled);
  CHECK(filled.gx == 8 && filled.gy == 2 && filled.gz == 1 && filled.k_per_split == 128 &&
        filled.bplane_stride == 160 * 128 && filled.bplane_nblk == 5 &&
        filled.bplanes == nullptr);
  // ... and through the dispatch: asked for in the product's orientation, before the launch
  g_split_gemm = 1;
  ga_set_small_m_gemm(0);
  {
    Buf<float> A(1024 * 128), B(128 * 128), C(1024 * 128);
    g_calls.clear();
    g_planes_bwd = -1;
    CHECK(ga_gemm_nt_f32(A.p, 128, B.p, 128, C.p, 128, 1024, 128, 128, nullptr) == 0);
    CHECK(g_calls.size() == 1 && g_calls[0].tile == GT_KC_SPLIT && g_planes_bwd == 0 &&
          g_planes.size() == 1 && g_calls[0].p.bplanes == g_planes[0]->p);
    free_planes();
  }
  g_split_gemm = 0;
  ga_set_small_m_gemm(1);

  // two products in one grid: one shape, gz >= 1
  GemmParams a = product(256, 256, 32768, 256, T_NONE), b = a;
  a.gz = b.gz = 128;
  GemmPairPlan pp = ga_gemm_pair_plan(a, b);
  CHECK(pp.taken && pp.gx == 2 && pp.gy == 2 && pp.gz == 128 &&
        pp.work == 4.0 * 256 * 256 * 32768);
  a.M = 257;
  pp = ga_gemm_pair_plan(a, b);
  CHECK(!pp.taken);
  b.M = 257;
  pp = ga_gemm_pair_plan(a, b);
  CHECK(pp.taken && pp.gx == 3);
  b.N = 255;
  CHECK(!ga_gemm_pair_plan(a, b).taken);
  b.N = 256; b.K = 1;
  CHECK(!ga_gemm_pair_plan(a, b).taken);
  b.K = a.K; b.gz = 127;
  CHECK(!ga_gemm_pair_plan(a, b).taken);
  a.gz = b.gz = 0;
  CHECK(!ga_gemm_pair_plan(a, b).taken);
  a.gz = b.gz = 1;
  CHECK(ga_gemm_pair_plan(a, b).taken);
}

static void head_plan_table() {
  const struct {
    int M, N, head_n;
    Twist twist;
    int taken, width, gx, threads;
  } rows[] = {
      // the widths with an instantiation against those without
      {64, 64, 2, T_NONE, 1, 64, 1, 256},
      {64, 128, 2, T_NONE, 1, 128, 1, 256},
      {64, 256, 2, T_NONE, 1, 256, 1, 512},
      {64, 32, 2, T_NONE, 0, 0, 0, 0},
      {64, 96, 2, T_NONE, 0, 0, 0, 0},
      {64, 512, 2, T_NONE, 0, 0, 0, 0},
      // whole 64-row tiles
      {63, 64, 2, T_NONE, 0, 0, 0, 0},
      {65, 64, 2, T_NONE, 0, 0, 0, 0},
      {128, 64, 2, T_NONE, 1, 64, 2, 256},
      {32768, 256, 6, T_NONE, 1, 256, 512, 512},
      // head_n 8 | 9, and 1 | 0
      {64, 128, 8, T_NONE, 1, 128, 1, 256},
      {64, 128, 9, T_NONE, 0, 0, 0, 0},
      {64, 128, 1, T_NONE, 1, 128, 1, 256},
      {64, 128, 0, T_NONE, 0, 0, 0, 0},
      // head_ldw % 4, c_rs % 4, an unaligned C
      {64, 128, 2, T_HEAD_LDW, 0, 0, 0, 0},
      {64, 128, 2, T_C_RS, 0, 0, 0, 0},
      {64, 128, 2, T_C_UNALIGNED, 0, 0, 0, 0},
      // each of H, accum, colsum set; another epilogue; a transposed C
      {64, 128, 2, T_H, 0, 0, 0, 0},
      {64, 128, 2, T_ACCUM, 0, 0, 0, 0},
      {64, 128, 2, T_COLSUM, 0, 0, 0, 0},
      {64, 128, 2, T_EPI_PLAIN, 0, 0, 0, 0},
      {64, 128, 2, T_C_CS, 0, 0, 0, 0},
  };
  int i = 0;
  for (const auto& r : rows) {
    GemmParams p = product(r.M, r.N, 17, 32, r.twist == T_H || r.twist == T_EPI_PLAIN ||
                                                    r.twist == T_C_RS ? T_NONE : r.twist);
    if (r.twist != T_EPI_PLAIN) p.epi = EPI_BIAS_ACT;
    p.bias = g_mem; p.act = 1;
    p.head_W = g_mem; p.head_ldw = r.twist == T_HEAD_LDW ? r.N + 2 : r.N;
    p.head_bias = g_mem; p.head_n = r.head_n; p.head_out = g_mem; p.head_ld = 12;
    if (r.twist == T_H) { p.H = g_mem; p.ldh = r.N; }
    if (r.twist == T_C_RS) p.c_rs = r.N + 2;
    if (r.twist == T_C_UNALIGNED) p.C = g_mem + 1;
    const GemmHeadPlan h = ga_gemm_head_plan(p);
    const bool ok = h.taken == (r.taken != 0) && h.width == r.width && h.gx == r.gx &&
                    h.threads == r.threads &&
                    (!h.taken || h.work == 2.0 * r.M * r.N * (17.0 + r.head_n));
    if (!ok)
      fprintf(stderr, "head plan row %d: taken %d width %d gx %d threads %d\n", i, (int)h.taken,
              h.width, h.gx, h.threads);
    CHECK(ok);
    ++i;
  }
}

static void skinny_fwd_plan_table() {
  const struct {
    int M, N, K, w_kc, enabled, rows_wg;
    Twist twist;
    int taken, KV, qpr, rows_per_thread, gx, gy, lds_bytes;
  } rows[] = {
      // K = 32 | 33
      {70, 64, 32, 1, 1, 32, T_NONE, 1, 8, 16, 4, 2, 1, 8192},
      {70, 64, 33, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 1, 1, 1, 32, T_NONE, 1, 1, 16, 4, 2, 1, 1024},
      {70, 64, 5, 1, 1, 32, T_NONE, 1, 2, 16, 4, 2, 1, 2048},
      // widths: a whole power-of-two row up to 256 floats, else whole 256-float blocks
      {70, 128, 4, 1, 1, 32, T_NONE, 1, 1, 32, 4, 3, 1, 512},
      {70, 256, 4, 1, 1, 32, T_NONE, 1, 1, 64, 8, 3, 1, 512},
      {70, 512, 4, 1, 1, 32, T_NONE, 1, 1, 64, 8, 3, 2, 512},
      {70, 768, 4, 1, 1, 32, T_NONE, 1, 1, 64, 8, 3, 3, 512},
      {70, 32, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 36, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 40, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 48, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 260, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 516, 4, 1, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      // the two products: k-contiguous weights without H, the others with tanh's H
      {70, 64, 4, 1, 1, 32, T_H, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 0, 1, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 0, 1, 32, T_H, 1, 1, 16, 4, 2, 1, 1024},
      {70, 64, 4, 0, 1, 32, T_HACT1, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 1, 1, 32, T_ACT2, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 1, 1, 32, T_EPI_PLAIN, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 1, 1, 32, T_ACCUM, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 1, 1, 32, T_C_UNALIGNED, 0, 0, 0, 0, 0, 0, 0},
      {70, 64, 4, 1, 1, 32, T_A_IDX, 1, 1, 16, 4, 2, 1, 1024},
      // the switch
      {70, 64, 4, 1, 0, 32, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      // rows per workgroup: halved while M < 256 of them, never below 32
      {32768, 64, 4, 1, 1, 128, T_NONE, 1, 1, 16, 8, 256, 1, 2048},
      {32767, 64, 4, 1, 1, 128, T_NONE, 1, 1, 16, 4, 512, 1, 1024},
      {16383, 64, 4, 1, 1, 128, T_NONE, 1, 1, 16, 4, 256, 1, 1024},
      {70, 64, 4, 1, 1, 64, T_NONE, 1, 1, 16, 4, 2, 1, 1024},
      // ... the 48 KiB of staged rows: 384 | 448 rows of 32 floats
      {131072, 64, 32, 1, 1, 384, T_NONE, 1, 8, 16, 24, 342, 1, 49152},
      {131072, 64, 32, 1, 1, 400, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {131072, 64, 32, 1, 1, 512, T_NONE, 0, 0, 0, 0, 0, 0, 0},
      {131072, 64, 16, 1, 1, 512, T_NONE, 1, 4, 16, 32, 256, 1, 32768},
  };
  int i = 0;
  for (const auto& r : rows) {
    GemmParams p = product(r.M, r.N, r.K, 32, r.twist == T_A_IDX || r.twist == T_ACCUM ? r.twist
                                                                                       : T_NONE);
    p.ldb = r.w_kc ? round4(r.K) : round4(r.N);
    p.epi = r.w_kc ? EPI_BIAS_ACT : EPI_MUL_DTANH;
    if (r.twist == T_EPI_PLAIN) p.epi = EPI_PLAIN;
    if (r.w_kc) { p.bias = g_mem; p.act = r.twist == T_ACT2 ? 2 : 1; }
    if (r.twist == T_H || r.twist == T_HACT1) {
      p.H = g_mem; p.ldh = round4(r.N); p.hact = r.twist == T_HACT1 ? 1 : 0;
    }
    if (r.twist == T_C_UNALIGNED) p.C = g_mem + 2;
    const SkinnyFwdPlan s = ga_skinny_fwd_plan(p, r.w_kc != 0, r.enabled != 0, r.rows_wg);
    bool ok = s.taken == (r.taken != 0);
    if (r.taken)
      ok = ok && s.KV == r.KV && s.qpr == r.qpr && s.rows_per_thread == r.rows_per_thread &&
           s.gx == (unsigned)r.gx && s.gy == (unsigned)r.gy &&
           s.lds_bytes == (unsigned)r.lds_bytes && s.w_kc == (r.w_kc != 0) &&
           s.epi == (r.w_kc ? 0 : 1) &&
           s.work == 4.0 * r.M * ((double)r.N * (r.w_kc ? 1 : 2) + r.K);
    if (!ok)
      fprintf(stderr, "skinny forward plan row %d: taken %d KV %d qpr %d rows_per_thread %d "
              "grid %u x %u lds %u\n", i, (int)s.taken, s.KV, s.qpr, s.rows_per_thread, s.gx,
              s.gy, s.lds_bytes);
    CHECK(ok);
    if (s.taken) {
      const SkinnyFwdParams q = ga_skinny_fwd_params(p, s);
      CHECK(q.X == p.A && q.ldx == p.lda && q.idx == p.a_idx && q.W == p.B && q.ldw == p.ldb &&
            q.bias == p.bias && q.H == p.H && q.ldh == p.ldh && q.Y == p.C && q.ldy == p.c_rs &&
            q.M == r.M && q.N == r.N && q.K == r.K && q.act == p.act && q.qpr == r.qpr &&
            q.rows_per_thread == r.rows_per_thread);
    }
    ++i;
  }
  // rows_wg defaults to 32
  const GemmParams p = product(32768, 64, 4, 32, T_EPI_BIAS);
  CHECK(ga_skinny_fwd_plan(p, true, true).rows_per_thread == 4 &&
        ga_skinny_fwd_plan(p, true, true).gx == 512);
}

static void skinny_wgrad_plan_table() {
  const struct {
    int wide, NS, enabled;
    Twist twist;
    int taken, variant, NV, qpr, n_colblk, grid;
  } rows[] = {
      // NS = 24 | 25
      {256, 24, 1, T_NONE, 1, SWV_NSUM, 6, 16, 4, 12},
      {256, 25, 1, T_NONE, 0, 0, 0, 0, 0, 0},
      {256, 1, 1, T_NONE, 1, SWV_NSUM, 1, 16, 4, 12},
      // ... 16 | 17 with the data gradient; without it, 17 is taken
      {256, 16, 1, T_DZ, 1, SWV_DZ, 4, 16, 4, 12},
      {256, 17, 1, T_DZ, 0, 0, 0, 0, 0, 0},
      {256, 17, 1, T_NONE, 1, SWV_NSUM, 5, 16, 4, 12},
      {256, 6, 1, T_DZ, 1, SWV_DZ, 2, 16, 4, 12},
      // the plain variant: no narrow column sums (the data gradient needs them)
      {256, 6, 1, T_NO_NSUM, 1, SWV_PLAIN, 2, 16, 4, 12},
      {256, 17, 1, T_NO_NSUM, 1, SWV_PLAIN, 5, 16, 4, 12},
      // widths: a whole power-of-two row up to 64 floats, else 64-float column blocks
      {64, 6, 1, T_NONE, 1, SWV_NSUM, 2, 16, 1, 3},
      {260, 6, 1, T_NONE, 1, SWV_NSUM, 2, 16, 5, 15},
      {36, 6, 1, T_NONE, 0, 0, 0, 0, 0, 0},
      {48, 6, 1, T_NONE, 0, 0, 0, 0, 0, 0},
      {32, 6, 1, T_NONE, 0, 0, 0, 0, 0, 0},
      {258, 6, 1, T_NONE, 0, 0, 0, 0, 0, 0},
      // C with the wide side contiguous: 16-B rows; otherwise element stores
      {256, 6, 1, T_CNS, 0, 0, 0, 0, 0, 0},
      {256, 6, 1, T_C_UNALIGNED, 0, 0, 0, 0, 0, 0},
      {256, 6, 1, T_CWS, 1, SWV_NSUM, 2, 16, 4, 12},
      // the switch
      {256, 6, 0, T_NONE, 0, 0, 0, 0, 0, 0},
  };
  int i = 0;
  for (const auto& r : rows) {
    SkinnyWgradParams p = {};
    p.Wd = g_mem; p.ldw = round4(r.wide); p.Nr = g_mem; p.ldn = round4(r.NS);
    p.rows = 70; p.wide = r.wide; p.NS = r.NS; p.rows_per_split = 32; p.n_splits = 3;
    p.C = g_mem; p.c_wide_stride = 1; p.c_narrow_stride = round4(r.wide);
    p.split_stride = 1000;
    p.colsum_narrow = g_mem;
    if (r.twist == T_NO_NSUM) { p.colsum_narrow = nullptr; p.colsum_wide = g_mem; }
    if (r.twist == T_DZ) { p.Wn = g_mem; p.ldwn = p.ldw; p.dz_out = g_mem; p.lddz = p.ldw; }
    if (r.twist == T_CNS) p.c_narrow_stride += 2;
    if (r.twist == T_C_UNALIGNED) p.C = g_mem + 1;
    if (r.twist == T_CWS) {  // (the first layer's orientation, at an odd address)
      p.c_wide_stride = round4(r.NS); p.c_narrow_stride = 1; p.C = g_mem + 1;
    }
    const SkinnyWgradPlan s = ga_skinny_wgrad_plan(p, r.enabled != 0);
    bool ok = s.taken == (r.taken != 0);
    if (r.taken)
      ok = ok && s.variant == r.variant && s.NV == r.NV && s.qpr == r.qpr &&
           s.n_colblk == r.n_colblk && s.grid == (unsigned)r.grid &&
           s.work == 4.0 * 70 * ((double)r.wide * (r.twist == T_DZ ? 2 : 1) + r.NS);
    if (!ok)
      fprintf(stderr, "skinny weight-gradient plan row %d: taken %d variant %d NV %d qpr %d "
              "n_colblk %d grid %u\n", i, (int)s.taken, (int)s.variant, s.NV, s.qpr,
              s.n_colblk, s.grid);
    CHECK(ok);
    ++i;
  }
  // the data gradient's own conditions: no gather of the wide side, aligned head weights
  SkinnyWgradParams p = {};
  p.Wd = g_mem; p.ldw = 256; p.Nr = g_mem; p.ldn = 8; p.rows = 70; p.wide = 256; p.NS = 6;
  p.rows_per_split = 32; p.n_splits = 3; p.C = g_mem; p.c_wide_stride = 1;
  p.c_narrow_stride = 256; p.split_stride = 1000; p.colsum_narrow = g_mem;
  p.Wn = g_mem; p.ldwn = 256; p.dz_out = g_mem; p.lddz = 256;
  CHECK(ga_skinny_wgrad_plan(p, true).variant == SWV_DZ);
  p.w_idx = g_idx;
  CHECK(!ga_skinny_wgrad_plan(p, true).taken);
  p.w_idx = nullptr; p.ldwn = 258;
  CHECK(!ga_skinny_wgrad_plan(p, true).taken);
  p.ldwn = 256; p.colsum_narrow = nullptr;
  CHECK(!ga_skinny_wgrad_plan(p, true).taken);
}

static void plan_tables() {
  gemm_plan_table();
  head_plan_table();
  skinny_fwd_plan_table();
  skinny_wgrad_plan_table();
}

int main() {
  Net one({5, 3});
  Net n64({4, 64, 64, 2});
  Net n256({17, 256, 256, 6});
  Net nln({11, 48, 40, 3}, /*relu*/ 1, /*tanh*/ 1, /*layer_norm*/ 1);
  Net n512({376, 512, 512, 512, 17});
  Net* nets[] = {&one, &n64, &n256, &nln, &n512};
  reset_switches();

  // 1. every launch of forward, backward and the tangent pass stays inside its
  //    buffers, with every streaming / fused kernel taking its shapes and with the
  //    tile kernel taking everything
  for (int tiles_only = 0; tiles_only < 2; ++tiles_only) {
    ga_set_skinny_kernels(!tiles_only);
    ga_set_fused_head_forward(tiles_only ? 0 : 2);
    for (Net* n : nets)
      for (int64_t M : {1, 70})
        for (int gather = 0; gather < 2; ++gather)
          for (int64_t n_splits : {1, 3}) {
            Case c(*n, M, gather != 0, n_splits);
            g_calls.clear();
            CHECK(c.forward() == 0);
            if (n->L >= 2) CHECK(c.forward(false) == 0);
            CHECK(c.backward() == 0);
            for (int l = 1; l < n->L; ++l) CHECK(c.backward_range(l, 1) == 0);
            CHECK(c.jvp() == 0);
            CHECK(!g_calls.empty());
            CHECK(calls_of("skinny_fwd") + calls_of("skinny_wgrad") + calls_of("skinny_wgrad+dz") +
                      calls_of("skinny_dgrad") + calls_of("gemm_head") == 0 || !tiles_only);
          }
  }
  CHECK(g_extent_errors == 0);
  reset_switches();

  // 1b. the same with the split-operand kernels switched on, at a batch they take: the
  //     weight planes come from ga_weight_planes and are exactly as large as the k-loop
  //     reads; the split-operand weight gradient gets interior shapes only
  g_split_gemm = g_split_wgrad = 1;
  for (int small_m = 0; small_m < 2; ++small_m) {
    ga_set_small_m_gemm(small_m);
    for (Net* n : {&n256, &n512}) {
      Case c(*n, 1024, true, 4);
      g_calls.clear();
      CHECK(c.forward() == 0);
      CHECK(c.backward() == 0);
      CHECK(c.jvp() == 0);
      int kc = 0, nt = 0;
      for (auto& k : g_calls) { kc += k.tile == GT_KC_SPLIT; nt += k.tile == GT_NT_SPLIT; }
      // (small-M tiles take these few-tile products first.  Without them, every product
      // with N, K >= 128 that does not accumulate: 1 forward, 1 data-gradient and 1
      // tangent product of the 256-wide net, 3 + 2 + 3 of the 512-wide one.  Every
      // wide x wide weight gradient whose sides are multiples of 128.)
      CHECK(kc == (small_m ? 0 : (n == &n256 ? 3 : 8)));
      CHECK(nt == n->L - 2);
      free_planes();
    }
  }
  CHECK(g_extent_errors == 0);
  reset_switches();

  // 2. which launcher a layer takes
  {
    // the streaming forward: K <= 32 < N with tanh / the identity; the last hidden layer
    // takes the head along when the batch is whole 64-row tiles
    Case c(n64, 128, true, 1);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm_head"}));  // head-fused: both layers done
    CHECK(g_calls[1].p.head_n == 2 && g_calls[1].p.head_out == c.out.p &&
          g_calls[1].p.head_W == c.params.p + n64.d.w_off[2] &&
          g_calls[1].C == c.acts.p + n64.d.act_off[1]);
    // M % 64 != 0, a shape the head launch does not take: the tile kernel, head dropped,
    // then the head
    Case c70(n64, 70, true, 1);
    g_calls.clear();
    CHECK(c70.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}));
    CHECK(g_calls[1].p.head_n == 0 && g_calls[1].p.head_W == c70.params.p + n64.d.w_off[2] &&
          g_calls[1].C == c70.acts.p + n64.d.act_off[1] && g_calls[2].C == c70.out.p);
    ga_set_fused_head_forward(0);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}));
    CHECK(g_calls[1].p.head_W == nullptr);
    ga_set_fused_head_forward(1);
    // a 48-wide first layer is no streaming shape (12 column quads): the tile kernel
    // takes the layer
    Net n48({4, 48, 64, 2});
    Case c48(n48, 128, true, 1);
    g_calls.clear();
    CHECK(c48.forward() == 0);
    CHECK((kinds() == Kinds{"gemm11", "gemm_head"}));
    CHECK(g_calls[0].p.a_idx == c48.idx.p && g_calls[0].p.K == 4 && g_calls[0].p.act == 1 &&
          g_calls[0].tile == GT_64x64);
    ga_set_skinny_kernels(0);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"gemm11", "gemm_head"}));
    CHECK(g_calls[0].p.a_idx == c.idx.p && g_calls[0].p.K == 4 && g_calls[0].p.act == 1);
    ga_set_skinny_kernels(1);
    // out == NULL stops below the head, and fuses no head
    g_calls.clear();
    CHECK(c.forward(false) == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11"}));
    CHECK(g_calls[1].p.head_W == nullptr && g_calls[1].C == c.acts.p + n64.d.act_off[1]);
    // an output activation: never head-fused
    Net n64t({4, 64, 64, 2}, 0, 1);
    Case ct(n64t, 128, false, 1);
    ga_set_fused_head_forward(2);
    g_calls.clear();
    CHECK(ct.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}) && g_calls[2].p.act == 1);
    ga_set_fused_head_forward(1);
    // a relu first layer of 11 inputs is no streaming shape
    Net relu({11, 64, 3}, 1);
    Case cr(relu, 128, false, 1);
    g_calls.clear();
    CHECK(cr.forward() == 0);
    CHECK((kinds() == Kinds{"gemm_head"}) && g_calls[0].p.act == 2);
    // ... nor is its head-fused launch one for a 48-wide layer
    Net relu48({11, 48, 3}, 1);
    Case cr48(relu48, 128, false, 1);
    g_calls.clear();
    CHECK(cr48.forward() == 0);
    CHECK((kinds() == Kinds{"gemm11", "gemm11"}) && g_calls[0].p.act == 2);
  }
  {
    // 256-wide: head-fused at mode 2 only
    Case c(n256, 128, false, 1);
    for (int mode = 0; mode <= 2; ++mode) {
      ga_set_fused_head_forward(mode);
      g_calls.clear();
      CHECK(c.forward() == 0);
      if (mode == 2) CHECK((kinds() == Kinds{"skinny_fwd", "gemm_head"}));
      else CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}));
    }
    ga_set_fused_head_forward(2);
    Net nln64({11, 64, 64, 3}, 0, 0, 1);
    Case cl(nln64, 128, false, 1);  // never with layer_norm
    g_calls.clear();
    CHECK(cl.forward() == 0);
    CHECK(calls_of("gemm_head") == 0 && g_calls.size() == 5);
    reset_switches();
    // the whole forward in one launch, on request
    ga_set_fused_forward(1);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"fused_fwd"}));
    g_policy_step_fused_ok = 0;
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK(calls_of("fused_fwd") == 0 && g_calls.size() == 3);
    reset_switches();
    // acts == NULL: the outputs-only forward when supported, else an error
    g_calls.clear();
    CHECK(c.forward(true, false) == 0);
    CHECK((kinds() == Kinds{"eval_fwd"}));
    g_calls.clear();
    ga_set_eval_forward(0);
    CHECK(c.forward(true, false) != 0 && g_calls.empty());
    CHECK(g_error == "ga_mlp_forward_f32: acts workspace needed");
    ga_set_eval_forward(1);
    g_eval_ok = 0;
    CHECK(c.forward(true, false) != 0 && g_calls.empty());
    g_eval_ok = 1;
    CHECK(c.forward(false, false) != 0 && g_calls.empty());
    Case c64(n64, 70, false, 1);  // 64-wide: the per-layer kernels
    CHECK(c64.forward(true, false) != 0 && g_calls.empty());
    Case c1(one, 70, false, 1);  // one layer needs no workspace
    CHECK(c1.forward(true, false) == 0);
    CHECK((kinds() == Kinds{"gemm11"}));
  }
  {
    // the head layer's streaming weight gradient, with and without the data gradient
    Case c(n256, 70, true, 3);
    const float* d1 = c.dacts.p + n256.d.act_off[1];
    const float* d0 = c.dacts.p + n256.d.act_off[0];
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad+dz", "gemm00", "gemm10", "skinny_wgrad"}));
    CHECK(g_calls[0].dz_out == d1 && g_calls[2].C == d0 && g_calls[2].p.H == c.acts.p &&
          g_calls[2].p.epi == EPI_MUL_DTANH && g_calls[1].splits == 3);
    {
      // a 17-wide head: no data gradient in the pass (16 narrow columns at most), so the
      // streaming weight gradient without it, then the data gradient on its own
      Net n17({17, 256, 256, 17});
      Case c17(n17, 70, true, 3);
      g_calls.clear();
      CHECK(c17.backward() == 0);
      CHECK((kinds() == Kinds{"skinny_wgrad", "skinny_dgrad", "gemm00", "gemm10",
                              "skinny_wgrad"}));
      CHECK(g_calls[0].C == c17.slabs.p + n17.d.w_off[2] && g_calls[0].dz_out == nullptr &&
            g_calls[1].C == c17.dacts.p + n17.d.act_off[1]);
    }
    ga_set_fused_head_dgrad(0);
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad", "skinny_dgrad", "gemm00", "gemm10",
                            "skinny_wgrad"}));
    {
      // 320-wide hidden layers: a streaming weight gradient (64-float column blocks) but
      // no streaming data gradient (no whole 256-float blocks): it falls to the tile
      // kernel too
      Net n320({17, 320, 320, 6});
      Case c3(n320, 70, true, 3);
      g_calls.clear();
      CHECK(c3.backward() == 0);
      CHECK((kinds() == Kinds{"skinny_wgrad", "gemm10", "gemm00", "gemm10", "skinny_wgrad"}));
      CHECK(g_calls[1].C == c3.dacts.p + n320.d.act_off[1] && g_calls[1].p.K == 6 &&
            g_calls[1].p.N == 320 && g_calls[1].p.A == c3.dout.p &&
            g_calls[1].p.H == c3.acts.p + n320.d.act_off[1]);
    }
    ga_set_fused_head_dgrad(1);
    {
      // 25 inputs and a 25-wide head: one narrow column more than the streaming weight
      // gradient takes, so the tile kernel takes both layers'
      Net n25({25, 256, 256, 25});
      Case c25(n25, 70, true, 3);
      g_calls.clear();
      CHECK(c25.backward() == 0);
      CHECK((kinds() == Kinds{"gemm00", "skinny_dgrad", "gemm00", "gemm10", "gemm00"}));
      // the head layer's transposed product: dW^T = in^T dz, bias gradient from B
      const GemmParams& h = g_calls[0].p;
      CHECK(h.M == 256 && h.N == 25 && h.c_rs == 1 && h.c_cs == 256 && h.colsum_of_b == 1 &&
            h.A == c25.acts.p + n25.d.act_off[1] && h.B == c25.dout.p && h.ldb == 28 &&
            h.C == c25.slabs.p + n25.d.w_off[2] && h.colsum == c25.slabs.p + n25.d.b_off[2]);
      // layer 0: narrow in, natural orientation, X through the gather as B's lines
      const GemmParams& f = g_calls[4].p;
      CHECK(f.M == 256 && f.N == 25 && f.c_rs == 28 && f.c_cs == 1 && f.colsum_of_b == 0 &&
            f.B == c25.X.p && f.b_idx == c25.idx.p && f.ldb == 28 && f.K == 70 &&
            f.k_per_split == 32 && g_calls[4].tile == GT_128x32);
    }
    ga_set_skinny_kernels(0);
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "gemm00", "gemm10", "gemm00"}));
    reset_switches();
    // both sides narrow: the transposed tile product; a narrow hidden layer's weight
    // gradient streams like the head's, with the data gradient up to 16 outputs ...
    Net narrow({40, 64, 16, 2});
    Case cn(narrow, 70, false, 1);
    g_calls.clear();
    CHECK(cn.backward() == 0);
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "skinny_wgrad+dz", "gemm00"}));
    // ... and without it up to 24
    Net narrow24({40, 64, 24, 2});
    Case cn24(narrow24, 70, false, 1);
    g_calls.clear();
    CHECK(cn24.backward() == 0);
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "skinny_wgrad", "skinny_dgrad", "gemm00"}));
  }

  // 3. ga_wgrad_mid's two descriptors are the ones ga_mlp_backward_range_f32 launches
  //    for layer 1 with fused_first = 1, grid and all, wherever that takes the 128 x 128
  //    tiles of the pair kernel (a one-split product of more than 64 rows takes the
  //    small-M tiles: same descriptor, another grid and k step)
  for (int64_t M : {70, 64})
    for (int64_t n_splits : {1, 3}) {
      Net na({17, 256, 256, 6}), nb({17, 256, 256, 1});
      Case a(na, M, false, n_splits), b(nb, M, true, n_splits);
      ga_wgrad_mid_net pair[2];
      Case* cs[2] = {&a, &b};
      for (int i = 0; i < 2; ++i) {
        const ga_mlp_desc& d = cs[i]->net.d;
        pair[i].dz = cs[i]->dacts.p + d.act_off[1];
        pair[i].in = cs[i]->acts.p + d.act_off[0];
        pair[i].slabs_w = cs[i]->slabs.p + d.w_off[1];
        pair[i].slabs_b = cs[i]->slabs.p + d.b_off[1];
        pair[i].slab_stride = cs[i]->net.n_flat;
      }
      g_calls.clear();
      CHECK(ga_wgrad_mid(pair, 2, M, n_splits, 256, 256, nullptr) == 0);
      CHECK((kinds() == Kinds{"gemm_pair", "gemm_pair"}));
      CHECK(a.backward_range(1, 1) == 0);
      CHECK(b.backward_range(1, 1) == 0);
      CHECK((kinds() == Kinds{"gemm_pair", "gemm_pair", "gemm00", "gemm00"}));
      if (g_calls.size() == 4) {
        const bool small_m = M == 70 && n_splits == 1;
        CHECK(g_calls[2].tile == (small_m ? GT_SMALL_M : GT_128x128) &&
              g_calls[3].tile == g_calls[2].tile);
        if (small_m)
          for (int i = 2; i < 4; ++i) {
            GemmParams& q = g_calls[(size_t)i].p;
            CHECK(q.gx == 4 && q.gy == 4 && q.k_per_split == 128);
            q.gx = q.gy = 2; q.k_per_split = 96;  // what the 128 x 128 tiles get
          }
        CHECK(same_params(g_calls[0].p, g_calls[2].p) && g_calls[0].splits == g_calls[2].splits);
        CHECK(same_params(g_calls[1].p, g_calls[3].p) && g_calls[1].splits == g_calls[3].splits);
        CHECK(!same_params(g_calls[0].p, g_calls[1].p));
        CHECK(g_calls[2].p.gz == n_splits && g_calls[2].p.M == 256 && g_calls[2].p.N == 256 &&
              g_calls[2].p.K == M && g_calls[2].p.colsum_of_b == 0);
      }
    }
  CHECK(ga_wgrad_mid(nullptr, 2, 70, 1, 256, 256, nullptr) != 0);

  // 4. l_start = L - 2, fused_first = 1: the full pass minus the head layer's launches,
  //    minus layer 0's, minus the data gradient into layer 0's output
  for (Net* n : {&n64, &n256, &n512})
    for (int dgrad_fusion = 0; dgrad_fusion < 2; ++dgrad_fusion) {
      ga_set_fused_head_dgrad(dgrad_fusion);
      Case c(*n, 70, true, 3);
      g_calls.clear();
      CHECK(c.backward() == 0);
      std::vector<Call> want;
      for (const Call& k : g_calls) {
        const int sl = c.slab_layer(k.C), dl = c.dgrad_layer(k.C);
        CHECK((sl >= 0) != (dl >= 0));
        const bool heads = sl == n->L - 1 || dl == n->L - 2;
        const bool first = sl == 0 || dl == 0;
        if (!heads && !first) want.push_back(k);
      }
      g_calls.clear();
      CHECK(c.backward_range(n->L - 2, 1) == 0);
      CHECK(g_calls.size() == want.size() && want.size() == (size_t)(2 * (n->L - 2) - 1));
      for (size_t i = 0; i < want.size() && i < g_calls.size(); ++i)
        CHECK(same_call(want[i], g_calls[i]));
    }
  reset_switches();

  // 5. LayerNorm: the norm in front of each hidden product; backward, the plain product
  //    first, then ga_ln_backward in place, want_dx = 0 only at layer 0
  {
    Case c(nln, 70, true, 3);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"ln_fwd", "gemm11", "ln_fwd", "gemm11", "gemm11"}));
    CHECK(g_calls[1].p.A == g_calls[0].C && g_calls[1].p.a_idx == nullptr &&
          g_calls[0].C == c.acts.p + nln.d.lnx_off[0] && g_calls[1].p.lda == 12 &&
          g_calls[3].p.A == g_calls[2].C && g_calls[3].p.lda == 48 &&
          g_calls[4].p.A == c.acts.p + nln.d.act_off[1] && g_calls[4].p.act == 1 &&
          g_calls[1].p.act == 2);
    g_calls.clear();
    CHECK(c.backward() == 0);
    // (40 and 48 floats are no whole power-of-two row: no streaming weight gradient)
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "gemm00", "gemm10", "ln_bwd", "gemm00", "gemm10",
                            "ln_bwd"}));
    CHECK(g_calls[1].p.epi == EPI_MUL_DTANH && g_calls[1].p.hact == 1);
    CHECK(g_calls[3].p.epi == EPI_PLAIN && g_calls[3].p.H == nullptr &&
          g_calls[4].C == g_calls[3].C && g_calls[4].want_dx == 1 &&
          g_calls[3].C == c.dacts.p + nln.d.act_off[0] &&
          g_calls[2].p.B == c.acts.p + nln.d.lnx_off[1]);
    CHECK(g_calls[6].p.epi == EPI_PLAIN && g_calls[7].C == g_calls[6].C &&
          g_calls[7].want_dx == 0 && g_calls[6].C == c.dacts.p + nln.d.lnx_off[0]);
    g_calls.clear();
    CHECK(c.jvp() == 0);
    CHECK((kinds() == Kinds{"ln_jvp", "gemm11", "gemm11", "ln_jvp", "gemm11", "gemm11",
                            "gemm11", "gemm11"}));
    CHECK(g_calls[1].p.B == c.tangent.p + nln.d.w_off[0] && g_calls[1].p.H == nullptr &&
          g_calls[2].p.B == c.params.p + nln.d.w_off[0] && g_calls[2].p.accum == 1 &&
          g_calls[2].p.A == g_calls[0].C && g_calls[2].p.H == c.acts.p &&
          g_calls[7].p.epi == EPI_PLAIN && g_calls[7].C == c.tout.p);
    // without LayerNorm the first layer's tangent is one product with the slope
    Case c2(n256, 70, true, 1);
    g_calls.clear();
    CHECK(c2.jvp() == 0);
    CHECK(g_calls.size() == 5 && g_calls[0].p.H == c2.acts.p && g_calls[0].p.hact == 0 &&
          g_calls[0].p.a_idx == c2.idx.p && g_calls[0].p.bias == c2.tangent.p + n256.d.b_off[0]);
  }
  CHECK(g_extent_errors == 0);

  // 6. argument errors launch nothing
  {
    Case c(n256, 70, false, 1);
    g_calls.clear();
    const ga_mlp_desc good = n256.d;
    float* const P = c.params.p; float* const X = c.X.p;
    auto fwd = [&](const ga_mlp_desc* d, const float* p, const float* x, int64_t ldx) {
      return ga_mlp_forward_f32(d, p, x, ldx, nullptr, 70, c.acts.p, c.out.p, 8, nullptr);
    };
    auto bwd = [&](const ga_mlp_desc* d, const float* p, float* slabs, int l_start, int ff,
                   const float* dout) {
      return ga_mlp_backward_range_f32(d, p, X, 20, nullptr, 70, c.acts.p, dout, 8,
                                       c.dacts.p, slabs, n256.n_flat, 1, l_start, ff, nullptr);
    };
    auto jvp = [&](const ga_mlp_desc* d, const float* t, int64_t ldx) {
      return ga_mlp_jvp_f32(d, P, t, X, ldx, nullptr, 70, c.acts.p, c.tacts.p, c.tout.p, 8,
                            nullptr);
    };
    CHECK(fwd(nullptr, P, X, 20) != 0 && g_error == "ga_mlp_forward_f32: null descriptor");
    CHECK(fwd(&good, nullptr, X, 20) != 0 && g_error == "ga_mlp_forward_f32: null pointer");
    CHECK(fwd(&good, P, nullptr, 20) != 0 && g_error == "ga_mlp_forward_f32: null pointer");
    CHECK(fwd(&good, P, X, 18) != 0 && g_error == "ga_mlp_forward_f32: ldx 18");
    CHECK(jvp(&good, c.tangent.p, 18) != 0 && g_error == "ga_mlp_jvp_f32: leading dimensions");
    CHECK(jvp(&good, nullptr, 20) != 0 && g_error == "ga_mlp_jvp_f32: null pointer");
    CHECK(bwd(&good, P, nullptr, 2, 0, c.dout.p) != 0 &&
          g_error == "ga_mlp_backward_f32: null pointer");
    CHECK(ga_mlp_backward_f32(nullptr, P, X, 20, nullptr, 70, c.acts.p, c.dout.p, 8, c.dacts.p,
                              c.slabs.p, n256.n_flat, 1, nullptr) != 0 &&
          g_error == "ga_mlp_backward_f32: null descriptor");
    CHECK(ga_mlp_backward_f32(&good, P, X, 18, nullptr, 70, c.acts.p, c.dout.p, 8, c.dacts.p,
                              c.slabs.p, n256.n_flat, 1, nullptr) != 0 &&
          g_error == "ga_mlp_backward_f32: strides must be multiples of 4");
    for (int bad_layers : {0, 9}) {
      ga_mlp_desc d = good;
      d.n_layers = bad_layers;
      char want[96];
      snprintf(want, sizeof(want), ": n_layers %d not in 1..8", bad_layers);
      CHECK(fwd(&d, P, X, 20) != 0 && g_error == std::string("ga_mlp_forward_f32") + want);
      CHECK(bwd(&d, P, c.slabs.p, 2, 0, c.dout.p) != 0 &&
            g_error == std::string("ga_mlp_backward_f32") + want);
      CHECK(jvp(&d, c.tangent.p, 20) != 0 && g_error == std::string("ga_mlp_jvp_f32") + want);
    }
    {
      ga_mlp_desc d = good;
      d.w_off[1] += 2;
      CHECK(fwd(&d, P, X, 20) != 0 &&
            g_error == "ga_mlp_forward_f32: offsets of layer 1 not 16-B aligned");
      d = good;
      d.act_off[1] += 1;
      CHECK(bwd(&d, P, c.slabs.p, 2, 0, c.dout.p) != 0 &&
            g_error == "ga_mlp_backward_f32: offsets of layer 1 not 16-B aligned");
      d = nln.d;
      d.ln_off[0] += 2;
      CHECK(fwd(&d, P, X, 20) != 0 &&
            g_error.find("layer normalisation of layer 0: unaligned offsets") !=
                std::string::npos);
    }
    // a bad layer range: past the net, the head without dout, fused_first at layer 0
    CHECK(bwd(&good, P, c.slabs.p, 3, 0, c.dout.p) != 0 &&
          g_error == "ga_mlp_backward_f32: bad layer range");
    CHECK(bwd(&good, P, c.slabs.p, -1, 0, c.dout.p) != 0);
    CHECK(bwd(&good, P, c.slabs.p, 2, 0, nullptr) != 0 &&
          g_error == "ga_mlp_backward_f32: bad layer range");
    CHECK(bwd(&good, P, c.slabs.p, 0, 1, c.dout.p) != 0 &&
          g_error == "ga_mlp_backward_f32: bad layer range");
    CHECK(bwd(&good, P + 1, c.slabs.p, 2, 0, c.dout.p) != 0 &&
          g_error == "ga_mlp_backward_f32: pointers must be 16-B aligned");
    CHECK(ga_gemm_nt_f32(nullptr, 4, X, 4, c.out.p, 4, 1, 1, 1, nullptr) != 0 &&
          g_error == "ga_gemm_nt_f32: null pointer");
    CHECK(g_calls.empty());
    CHECK(bwd(&good, P, c.slabs.p, 1, 0, nullptr) == 0 && !g_calls.empty());
  }

  // 7. the split count (environment unset, exact fp32 weight-gradient kernel)
  if (getenv("GARAGE_AMD_WGRAD_WORKGROUPS") == nullptr) {
    CHECK(ga_mlp_backward_splits(&n256.d, 32768) == 128);
    CHECK(ga_mlp_backward_splits(&n512.d, 65536) == 64);
    CHECK(ga_mlp_backward_splits(&n64.d, 4096) == 32);
    CHECK(ga_mlp_backward_splits(&n64.d, 64) == 1);
    for (Net* n : nets) CHECK(ga_mlp_backward_splits(&n->d, 1) == 1);
  } else {
    fprintf(stderr, "GARAGE_AMD_WGRAD_WORKGROUPS is set: unset it for this harness\n");
    ++g_failed;
  }

  plan_tables();

  if (g_extent_errors) fprintf(stderr, "%d extent error(s)\n", g_extent_errors);
  CHECK(g_extent_errors == 0);
  return finish("mlp layers ok");
}
