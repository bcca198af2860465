// Host-logic harness for the per-layer MLP dispatch (garage_amd/csrc/mlp_layers.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-mlp`).  Every launch
// the dispatch makes -- the three GEMM launch entries, the streaming kernels, the
// LayerNorm passes, the one-launch forwards -- is replaced by a fake that records the
// call and never dereferences a device pointer.  Instead each fake works out the
// extent its kernel would reach (operand rows x ld through the gather's largest
// index, C through its strides and splits, column sums, bias, H, the head operands,
// LayerNorm statistics) and checks it against the exactly-sized heap buffer the
// pointer came from.  A miss is a failure.  The checks are about the dispatch's own
// arithmetic: where a layer's operands sit in the flat layouts (built the way
// garage_amd/engine.py builds them), which kernel a layer takes by default and with
// each developer switch flipped, and that ga_wgrad_mid and
// ga_mlp_backward_range_f32 describe the middle layer's weight gradient alike.
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/gemm_params.h"
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

// what the fakes answer (0 launched, 1 shape not taken)
static int g_head_answer = 0, g_skinny_fwd_answer = 0, g_skinny_wgrad_answer = 0;
static int g_skinny_wgrad_refuse_dz = 0;
// (ga_policy_step_fused_supported answers g_policy_step_fused_ok: harness.h)
static int g_eval_ok = 1;

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

// ---- fakes of gemm.hip's launch entries -----------------------------------------
int ga_gemm_launch(const GemmParams* p, int a_kc, int b_kc, int splits, hipStream_t) {
  char kind[16];
  snprintf(kind, sizeof(kind), "gemm%d%d", a_kc, b_kc);
  Call& c = record(kind);
  c.p = *p; c.splits = splits; c.C = p->C;
  gemm_extents(*p, a_kc, b_kc, splits);
  return 0;
}
int ga_gemm_launch_with_head(const GemmParams* p, hipStream_t) {
  Call& c = record("gemm_head");
  c.p = *p; c.splits = 1; c.C = p->C;
  if (g_head_answer) return g_head_answer;
  gemm_extents(*p, 1, 1, 1);
  reach_lines(p->head_W, p->head_ldw, nullptr, p->head_n, p->N, "head W");
  reach_f(p->head_bias, p->head_n, "head bias");
  reach_f(p->head_out, (int64_t)(p->M - 1) * p->head_ld + p->head_n, "head out");
  return 0;
}
int ga_gemm_launch_pair(const GemmParams* a, const GemmParams* b, hipStream_t) {
  for (const GemmParams* p : {a, b}) {
    Call& c = record("gemm_pair");
    c.p = *p; c.splits = p->gz; c.C = p->C;
    gemm_extents(*p, 0, 0, p->gz);
  }
  return 0;
}

// ---- skinny.hip ---------------------------------------------------------------------
int ga_skinny_forward(const float* X, int64_t ldx, const int32_t* idx, const float* W,
                      int64_t ldw, bool w_kc, const float* bias, int, const float* H,
                      int64_t ldh, float* Y, int64_t ldy, int M, int N, int K, hipStream_t) {
  Call& c = record(w_kc ? "skinny_fwd" : "skinny_dgrad");
  c.C = Y;
  if (g_skinny_fwd_answer) return g_skinny_fwd_answer;
  reach_lines(X, ldx, idx, M, K, "skinny X");
  if (w_kc) reach_lines(W, ldw, nullptr, N, K, "skinny W");
  else reach_lines(W, ldw, nullptr, K, N, "skinny W (k lines)");
  if (bias) reach_f(bias, N, "skinny bias");
  if (H) reach_f(H, (int64_t)(M - 1) * ldh + N, "skinny H");
  reach_f(Y, (int64_t)(M - 1) * ldy + N, "skinny Y");
  return 0;
}
int ga_skinny_wgrad(const float* Wd, int64_t ldw, const int32_t* w_idx, const float* Nr,
                    int64_t ldn, const int32_t* n_idx, int rows, int wide, int NS,
                    int rows_per_split, int n_splits, float* C, int64_t c_wide_stride,
                    int64_t c_narrow_stride, int64_t split_stride, float* colsum_wide,
                    float* colsum_narrow, const float* Wn, int64_t ldwn, float* dz_out,
                    int64_t lddz, hipStream_t) {
  Call& c = record(Wn ? "skinny_wgrad+dz" : "skinny_wgrad");
  c.C = C; c.dz_out = dz_out; c.splits = n_splits;
  if (g_skinny_wgrad_answer) return g_skinny_wgrad_answer;
  if (Wn && g_skinny_wgrad_refuse_dz) return 1;
  if (rows_per_split % BK != 0 || (int64_t)rows_per_split * n_splits < rows) {
    fprintf(stderr, "extent: skinny_wgrad rows_per_split\n");
    ++g_extent_errors;
  }
  reach_lines(Wd, ldw, w_idx, rows, wide, "skinny wide");
  reach_lines(Nr, ldn, n_idx, rows, NS, "skinny narrow");
  const int64_t split_off = (n_splits - 1) * split_stride;
  reach_f(C, split_off + (wide - 1) * c_wide_stride + (NS - 1) * c_narrow_stride + 1,
          "skinny dW");
  if (colsum_wide) reach_f(colsum_wide, split_off + wide, "skinny colsum (wide)");
  if (colsum_narrow) reach_f(colsum_narrow, split_off + NS, "skinny colsum (narrow)");
  if (Wn) {
    reach_lines(Wn, ldwn, nullptr, NS, wide, "skinny head W");
    reach_f(dz_out, (int64_t)(rows - 1) * lddz + wide, "skinny dz out");
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
int ga_split_bf16_enabled(void) { return 0; }
}  // extern "C"

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
  return a.kind == b.kind && same_params(a.p, b.p) && a.splits == b.splits && a.C == b.C &&
         a.dz_out == b.dz_out && a.want_dx == b.want_dx;
}

typedef std::vector<std::string> Kinds;

static void reset_switches() {
  ga_set_fused_forward(0);
  ga_set_eval_forward(1);
  ga_set_fused_head_forward(1);
  ga_set_fused_head_dgrad(1);
  ga_set_skinny_kernels(1);
  g_head_answer = g_skinny_fwd_answer = g_skinny_wgrad_answer = 0;
  g_skinny_wgrad_refuse_dz = 0;
  g_eval_ok = g_policy_step_fused_ok = 1;
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

  // 2. which launcher a layer takes
  {
    // the streaming forward: K <= 32 < N with tanh / the identity
    Case c(n64, 70, true, 1);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm_head"}));  // head-fused: both layers done
    g_head_answer = 1;  // shape not taken: the tile kernel, head dropped, then the head
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm_head", "gemm11", "gemm11"}));
    CHECK(g_calls[2].p.head_n == 0 && g_calls[2].p.head_W == g_calls[1].p.head_W &&
          g_calls[1].p.head_n == 2 && g_calls[1].p.head_out == c.out.p &&
          g_calls[2].C == c.acts.p + n64.d.act_off[1] && g_calls[3].C == c.out.p);
    g_head_answer = 0;
    ga_set_fused_head_forward(0);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}));
    CHECK(g_calls[1].p.head_W == nullptr);
    ga_set_fused_head_forward(1);
    // a streaming fake that answers 1: the tile kernel takes the layer
    g_skinny_fwd_answer = 1;
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm_head"}));
    CHECK(g_calls[1].p.a_idx == c.idx.p && g_calls[1].p.K == 4 && g_calls[1].p.act == 1);
    g_skinny_fwd_answer = 0;
    ga_set_skinny_kernels(0);
    g_calls.clear();
    CHECK(c.forward() == 0);
    CHECK((kinds() == Kinds{"gemm11", "gemm_head"}));
    ga_set_skinny_kernels(1);
    // out == NULL stops below the head, and fuses no head
    g_calls.clear();
    CHECK(c.forward(false) == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11"}));
    CHECK(g_calls[1].p.head_W == nullptr && g_calls[1].C == c.acts.p + n64.d.act_off[1]);
    // an output activation: never head-fused
    Net n64t({4, 64, 64, 2}, 0, 1);
    Case ct(n64t, 70, false, 1);
    ga_set_fused_head_forward(2);
    g_calls.clear();
    CHECK(ct.forward() == 0);
    CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}) && g_calls[2].p.act == 1);
    ga_set_fused_head_forward(1);
    // a relu first layer of 11 inputs is no streaming shape
    Net relu({11, 48, 3}, 1);
    Case cr(relu, 70, false, 1);
    g_calls.clear();
    CHECK(cr.forward() == 0);
    CHECK((kinds() == Kinds{"gemm_head"}) && g_calls[0].p.act == 2);
  }
  {
    // 256-wide: head-fused at mode 2 only
    Case c(n256, 70, false, 1);
    for (int mode = 0; mode <= 2; ++mode) {
      ga_set_fused_head_forward(mode);
      g_calls.clear();
      CHECK(c.forward() == 0);
      if (mode == 2) CHECK((kinds() == Kinds{"skinny_fwd", "gemm_head"}));
      else CHECK((kinds() == Kinds{"skinny_fwd", "gemm11", "gemm11"}));
    }
    ga_set_fused_head_forward(2);
    Case cl(nln, 70, false, 1);  // never with layer_norm
    g_calls.clear();
    CHECK(cl.forward() == 0);
    CHECK(calls_of("gemm_head") == 0);
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
    g_skinny_wgrad_refuse_dz = 1;  // the retry without the data gradient
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad+dz", "skinny_wgrad", "skinny_dgrad", "gemm00",
                            "gemm10", "skinny_wgrad"}));
    CHECK(g_calls[0].C == g_calls[1].C && g_calls[2].C == d1);
    g_skinny_wgrad_refuse_dz = 0;
    ga_set_fused_head_dgrad(0);
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad", "skinny_dgrad", "gemm00", "gemm10",
                            "skinny_wgrad"}));
    g_skinny_fwd_answer = 1;  // the data gradient falls back to the tile kernel too
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad", "skinny_dgrad", "gemm10", "gemm00", "gemm10",
                            "skinny_wgrad"}));
    CHECK(g_calls[2].C == d1 && g_calls[2].p.K == 6 && g_calls[2].p.N == 256 &&
          g_calls[2].p.A == c.dout.p && g_calls[2].p.H == c.acts.p + n256.d.act_off[1]);
    g_skinny_fwd_answer = 0;
    ga_set_fused_head_dgrad(1);
    g_skinny_wgrad_answer = 1;  // the tile kernel takes what the streaming one refuses
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"skinny_wgrad+dz", "skinny_wgrad", "gemm00", "skinny_dgrad",
                            "gemm00", "gemm10", "skinny_wgrad", "gemm00"}));
    // the head layer's transposed product: dW^T = in^T dz, bias gradient from B
    const GemmParams& h = g_calls[2].p;
    CHECK(h.M == 256 && h.N == 6 && h.c_rs == 1 && h.c_cs == 256 && h.colsum_of_b == 1 &&
          h.A == c.acts.p + n256.d.act_off[1] && h.B == c.dout.p && h.ldb == 8 &&
          h.C == c.slabs.p + n256.d.w_off[2] && h.colsum == c.slabs.p + n256.d.b_off[2]);
    // layer 0: narrow in, natural orientation, X through the gather as B's lines
    const GemmParams& f = g_calls[7].p;
    CHECK(f.M == 256 && f.N == 17 && f.c_rs == 20 && f.c_cs == 1 && f.colsum_of_b == 0 &&
          f.B == c.X.p && f.b_idx == c.idx.p && f.ldb == 20 && f.K == 70 &&
          f.k_per_split == 32);
    g_skinny_wgrad_answer = 0;
    ga_set_skinny_kernels(0);
    g_calls.clear();
    CHECK(c.backward() == 0);
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "gemm00", "gemm10", "gemm00"}));
    reset_switches();
    // both sides narrow: the transposed tile product; a narrow hidden layer's weight
    // gradient streams like the head's
    Net narrow({40, 64, 24, 2});
    Case cn(narrow, 70, false, 1);
    g_calls.clear();
    CHECK(cn.backward() == 0);
    CHECK((kinds() == Kinds{"gemm00", "gemm10", "skinny_wgrad+dz", "gemm00"}));
  }

  // 3. ga_wgrad_mid's two descriptors are the ones ga_mlp_backward_range_f32 launches
  //    for layer 1 with fused_first = 1
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
    CHECK((kinds() == Kinds{"skinny_wgrad", "gemm10", "gemm00", "gemm10", "ln_bwd",
                            "skinny_wgrad", "gemm10", "ln_bwd"}));
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

  if (g_extent_errors) fprintf(stderr, "%d extent error(s)\n", g_extent_errors);
  CHECK(g_extent_errors == 0);
  return finish("mlp layers ok");
}
