// Host-logic harness for the host side of the stand-alone loss, statistics and optimizer
// kernels (garage_amd/csrc/losses_host.cpp), built with -fsanitize=address,undefined on
// the CPU (`make asan-losses-host`).  The launch seam of loss_params.h and the two HIP
// calls the file makes are replaced by fakes.  Every seam fake records its grid, stream
// and dynamic LDS bytes, keeps the parameter struct it was handed, and touches, through
// volatile pointers, the extent its kernel would reach in buffers of exactly the
// required size, so that a grid, a stride or a workspace offset that is off trips the
// sanitizer.  What is expected is written down as literals, not taken from the code's
// own formulas: the refusals and their messages (each before any launch), the grids,
// one launch or two, the ticket's place, the structs field by field, the head kernels'
// LDS bytes, the optimizer coefficients.
#include "../../garage_amd/csrc/loss_params.h"
#include "../../garage_amd/csrc/internal.h"
#include "harness.h"

#include <functional>

static_assert(RED_BLOCKS == 512 && HL_THREADS == 256 && FS_MAX_A == 32 &&
                  LS_DOT_THREADS == 1024 && ga_head_rows(1) == 4 && ga_head_rows(2) == 4 &&
                  ga_head_rows(4) == 4 && ga_head_rows(8) == 2,
              "the constants the cases below are written for");

// ---- "device" memory: exactly n elements, 16-byte aligned, zeroed, freed at exit ----------
static std::vector<void*> g_owned;
template <class T>
static T* dev(int64_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, (size_t)n * sizeof(T))) abort();
  memset(p, 0, (size_t)n * sizeof(T));
  g_owned.push_back(p);
  return static_cast<T*>(p);
}
static void free_all() {
  for (void* p : g_owned) free(p);
  g_owned.clear();
}
static double* workspace() { return dev<double>(1026); }  // 2 * 512 partials + 2

// ---- what the fakes record ----------------------------------------------------------------
struct Launch {
  std::string what;
  unsigned blocks, lds;
  int arg;  // `what` of the stats pair, nblocks of a finalize
};
static std::vector<Launch> g_launches;
static hipStream_t const S1 = (hipStream_t)0x100;
static PpoLossParams g_ppo;
static PpoFinalizeParams g_fin;
static CatLossParams g_cat;
static NllParams g_nll;
static AdamParams g_adam;
static OptParams g_opt;
static HeadLayer g_head;
static int64_t g_pool = 0;  // rows of the per-sample inputs (gathered through idx)
static volatile float g_sink;

static void record(const char* what, unsigned blocks, hipStream_t s, unsigned lds = 0,
                   int arg = 0) {
  g_launches.push_back(Launch{what, blocks, lds, arg});
  CHECK(s == S1);  // the caller's stream, every time
}
template <class T> static void rd(const T* p, int64_t i) {
  const volatile T* q = p;
  g_sink = (float)q[0] + (float)q[i];
}
// (through a volatile pointer: a plain self-assignment is removed before the sanitizer
// instruments it)
template <class T> static void wr(T* p, int64_t i) {
  volatile T* q = p;
  q[0] = q[0]; q[i] = q[i];
}
static void reset() { g_launches.clear(); g_error.clear(); }
static std::string names() {
  std::string s;
  for (auto& l : g_launches) s += (s.empty() ? "" : " ") + l.what;
  return s;
}

// the scalars of the batch, as a loss launch that finishes itself or a finalize writes them
static void touch_scalars(float* loss_out, float* grad_slab0, int64_t slab_stride,
                          int64_t n_splits) {
  wr(loss_out, 0);
  if (grad_slab0) wr(grad_slab0, (n_splits - 1) * slab_stride);
}
// the tail every two-phase loss kernel shares: partials, ticket, scalars
template <class P>
static void touch_reduction(const P& p, unsigned blocks) {
  if (blocks > 1 || !p.loss_out) wr(p.partials, 2 * (int64_t)blocks - 1);
  if (p.loss_out && blocks > 1) wr(p.ticket, 0);
  if (p.loss_out) touch_scalars(p.loss_out, p.grad_slab0, p.slab_stride, p.n_splits);
}
// blocks of 256 threads loop over the rows: every row is taken, and none twice at first
static void grid_covers(unsigned blocks, int64_t rows, int per_block) {
  CHECK(blocks >= 1 && blocks <= 512);
  CHECK((int64_t)blocks * per_block >= rows || blocks == 512);
  CHECK((int64_t)(blocks - 1) * per_block < rows);
}

// ---- the seam's fakes ---------------------------------------------------------------------
void ls_launch_ppo_gaussian_loss(const PpoLossParams& p, unsigned blocks, hipStream_t s) {
  record("ppo_gaussian_loss", blocks, s);
  g_ppo = p;
  grid_covers(blocks, p.M, 256);
  rd(p.mean, (p.M - 1) * p.ldm + p.A - 1);
  if (p.idx) rd(p.idx, p.M - 1);
  rd(p.actions, (g_pool - 1) * p.lda + p.A - 1);
  if (p.algo != 1) rd(p.old_ll, g_pool - 1);
  rd(p.adv, g_pool - 1); rd(p.log_std, 0);
  if (p.dmean) wr(p.dmean, (p.M - 1) * p.ldm + p.A - 1);
  if (p.ll_out) wr(p.ll_out, p.M - 1);
  touch_reduction(p, blocks);
}
void ls_launch_ppo_gaussian_finalize(const PpoFinalizeParams& f, hipStream_t s) {
  record("ppo_gaussian_finalize", 1, s, 0, f.nblocks);
  g_fin = f;
  rd(f.partials, 2 * (int64_t)f.nblocks - 1); rd(f.log_std, 0);
  touch_scalars(f.loss_out, f.grad_slab0, f.slab_stride, f.n_splits);
}
void ls_launch_ppo_categorical_loss(const CatLossParams& p, unsigned blocks, hipStream_t s) {
  record("ppo_categorical_loss", blocks, s);
  g_cat = p;
  grid_covers(blocks, p.M, 256);
  rd(p.scores, (p.M - 1) * p.lds + p.A - 1);
  if (p.idx) rd(p.idx, p.M - 1);
  rd(p.actions, (g_pool - 1) * p.lda);
  if (p.algo != 1) rd(p.old_ll, g_pool - 1);
  rd(p.adv, g_pool - 1);
  if (p.dscores) wr(p.dscores, (p.M - 1) * p.lds + p.A - 1);
  if (p.ll_out) wr(p.ll_out, p.M - 1);
  if (p.ent_out) wr(p.ent_out, p.M - 1);
  touch_reduction(p, blocks);
  if (p.loss_out && p.ent_sum_out) wr(p.ent_sum_out, 0);
}
struct CatFinalize {
  const double* partials; int nblocks; int64_t M; float* loss_out; double* ent_sum_out;
  float* grad_slab0; int64_t slab_stride, n_splits;
};
static CatFinalize g_cat_fin;
void ls_launch_ppo_categorical_finalize(const double* partials, int nblocks, int64_t M,
                                        float* loss_out, double* ent_sum_out,
                                        float* grad_slab0, int64_t slab_stride,
                                        int64_t n_splits, hipStream_t s) {
  record("ppo_categorical_finalize", 1, s, 0, nblocks);
  g_cat_fin = CatFinalize{partials, nblocks, M, loss_out, ent_sum_out, grad_slab0,
                          slab_stride, n_splits};
  rd(partials, 2 * (int64_t)nblocks - 1);
  if (ent_sum_out) wr(ent_sum_out, 0);
  touch_scalars(loss_out, grad_slab0, slab_stride, n_splits);
}
void ls_launch_gaussian_nll(const NllParams& p, unsigned blocks, hipStream_t s) {
  record("gaussian_nll", blocks, s);
  g_nll = p;
  grid_covers(blocks, p.M, 256);
  rd(p.v, (p.M - 1) * p.ldv);
  if (p.idx) rd(p.idx, p.M - 1);
  rd(p.returns, g_pool - 1); rd(p.log_std, 0);
  if (p.dv) wr(p.dv, (p.M - 1) * p.ldv);
  touch_reduction(p, blocks);
}
struct NllFinalize {
  const double* partials; int nblocks; int64_t M; float* loss_out; float* grad_slab0;
  int64_t slab_stride, n_splits;
};
static NllFinalize g_nll_fin;
void ls_launch_gaussian_nll_finalize(const double* partials, int nblocks, int64_t M,
                                     float* loss_out, float* grad_slab0, int64_t slab_stride,
                                     int64_t n_splits, hipStream_t s) {
  record("gaussian_nll_finalize", 1, s, 0, nblocks);
  g_nll_fin = NllFinalize{partials, nblocks, M, loss_out, grad_slab0, slab_stride, n_splits};
  rd(partials, 2 * (int64_t)nblocks - 1);
  touch_scalars(loss_out, grad_slab0, slab_stride, n_splits);
}
static void kl_touch(const float* a, const float* b, int64_t ld, int64_t M, int A,
                     double* partials, unsigned blocks) {
  grid_covers(blocks, M, 256);
  rd(a, (M - 1) * ld + A - 1); rd(b, (M - 1) * ld + A - 1);
  wr(partials, (int64_t)blocks - 1);
}
void ls_launch_categorical_kl(const float* sc_old, const float* sc_new, int64_t ld, int64_t M,
                              int A, int dbl, double* partials, unsigned blocks,
                              hipStream_t s) {
  record("categorical_kl", blocks, s, 0, dbl);
  kl_touch(sc_old, sc_new, ld, M, A, partials, blocks);
}
static float g_kl_s_old, g_kl_s_new;
void ls_launch_gaussian_kl(const float* mean_old, const float* mean_new, int64_t ld,
                           int64_t M, int A, float s_old, float s_new, double* partials,
                           unsigned blocks, hipStream_t s) {
  record("gaussian_kl", blocks, s);
  g_kl_s_old = s_old; g_kl_s_new = s_new;
  kl_touch(mean_old, mean_new, ld, M, A, partials, blocks);
}
void ls_launch_sum_partials(const double* partials, int nblocks, double* out, hipStream_t s) {
  record("sum_partials", 1, s, 0, nblocks);
  rd(partials, (int64_t)nblocks - 1);
  wr(out, 0);
}
// 64 float4 columns per block, every slab
static void slabs_touch(const float* slabs, int64_t n_splits, int64_t stride, int64_t n,
                        unsigned blocks) {
  CHECK((int64_t)blocks * 256 >= n && (int64_t)(blocks - 1) * 256 < n);
  rd(slabs, (n_splits - 1) * stride + n - 1);
}
static float g_scale;
void ls_launch_reduce_slabs(const float* slabs, int64_t n_splits, int64_t stride, int64_t n,
                            float* out, float scale, unsigned blocks, hipStream_t s) {
  record("reduce_slabs", blocks, s);
  g_scale = scale;
  slabs_touch(slabs, n_splits, stride, n, blocks);
  wr(out, n - 1);
}
static void adam_touch(const AdamParams& a) {
  wr(a.p, a.n - 1); rd(a.g, a.n - 1); wr(a.m, a.n - 1); wr(a.v, a.n - 1);
}
static int g_zero_slot0;
void ls_launch_reduce_adam(const float* slabs, int64_t n_splits, int64_t stride,
                           int zero_slot0, const AdamParams& a, float* grads, unsigned blocks,
                           hipStream_t s) {
  record("reduce_adam", blocks, s);
  g_adam = a; g_zero_slot0 = zero_slot0;
  CHECK(grads == a.g);
  slabs_touch(slabs, n_splits, stride, a.n, blocks);
  wr(grads, a.n - 1);
  adam_touch(a);
}
void ls_launch_adam(const AdamParams& a, unsigned blocks, hipStream_t s) {
  record("adam", blocks, s);
  g_adam = a;
  CHECK((int64_t)blocks * 256 >= a.n && (int64_t)(blocks - 1) * 256 < a.n);
  adam_touch(a);
}
void ls_launch_optimizer_step(const OptParams& a, unsigned blocks, hipStream_t s) {
  record("optimizer_step", blocks, s);
  g_opt = a;
  CHECK((int64_t)blocks * 256 >= a.n && (int64_t)(blocks - 1) * 256 < a.n);
  wr(a.p, a.n - 1); rd(a.g, a.n - 1);
  // the state each kind reaches (optimizer_step_kernel)
  if (a.kind == 1) {
    if (a.h1 != 0.f) wr(a.s1, a.n - 1);
  } else if (a.kind == 2) {
    wr(a.s1, a.n - 1);
    if (a.flags & 1) wr(a.s3, a.n - 1);
    if (a.h4 > 0.f) wr(a.s2, a.n - 1);
  } else {
    wr(a.s1, a.n - 1); wr(a.s2, a.n - 1);
    if (a.flags & 1) wr(a.s3, a.n - 1);
  }
}
void ls_launch_stats(int what, const float* x, int64_t n, double* stats, double* partials,
                     unsigned blocks, hipStream_t s) {
  record("stats", blocks, s, 0, what);
  grid_covers(blocks, n, 256);
  rd(x, n - 1); wr(partials, (int64_t)blocks - 1); wr(stats, 3);
}
void ls_launch_adv_center(float* x, int64_t n, const double* stats, float eps, unsigned blocks,
                          hipStream_t s) {
  record("adv_center", blocks, s);
  g_scale = eps;
  grid_covers(blocks, n, 256);
  wr(x, n - 1); rd(stats, 2);
}
void ls_launch_sub_scalar(float* x, int64_t n, const double* scalar, unsigned blocks,
                          hipStream_t s) {
  record("sub_scalar", blocks, s);
  grid_covers(blocks, n, 256);
  wr(x, n - 1); rd(scalar, 0);
}
void ls_launch_dot(const float* a, const float* b, int64_t n, double* out, unsigned blocks,
                   hipStream_t s) {
  record("dot", blocks, s);
  rd(a, n - 1); rd(b, n - 1); wr(out, 0);
}
static float g_alpha, g_beta;
void ls_launch_axpby(float alpha, const float* x, float beta, float* y, int64_t n,
                     unsigned blocks, hipStream_t s) {
  record("axpby", blocks, s);
  g_alpha = alpha; g_beta = beta;
  CHECK((int64_t)blocks * 256 >= n && (int64_t)(blocks - 1) * 256 < n);
  rd(x, n - 1); wr(y, n - 1);
}
void ls_launch_fisher_seed_gaussian(const float* tmean, int64_t ldt, int64_t M, int A,
                                    const float* log_std, int, float, int, float, float* dout,
                                    int64_t ldd, unsigned blocks, hipStream_t s) {
  record("fisher_seed_gaussian", blocks, s);
  CHECK((int64_t)blocks * 256 >= M && (int64_t)(blocks - 1) * 256 < M);
  rd(tmean, (M - 1) * ldt + A - 1); rd(log_std, 0);
  wr(dout, (M - 1) * ldd + ldd - 1);  // (the padding columns are written too)
}
void ls_launch_fisher_seed_categorical(const float* scores, int64_t lds, const float* tscores,
                                       int64_t ldt, int64_t M, int A, int, float* dout,
                                       int64_t ldd, unsigned blocks, hipStream_t s) {
  record("fisher_seed_categorical", blocks, s);
  CHECK((int64_t)blocks * 256 >= M && (int64_t)(blocks - 1) * 256 < M);
  CHECK(A <= 32);  // z, q, u of the kernel
  rd(scores, (M - 1) * lds + A - 1); rd(tscores, (M - 1) * ldt + A - 1);
  wr(dout, (M - 1) * ldd + ldd - 1);
}
// what a head kernel reaches of the layer: H's last row, W's last row, the outputs
static void head_touch(const HeadLayer& L, int64_t M, int A, unsigned blocks) {
  CHECK(L.K == 64 || L.K == 128 || L.K == 256 || L.K == 512);  // an instantiation exists
  grid_covers(blocks, M, 64);
  rd(L.H, (M - 1) * L.ldh + L.K - 1); rd(L.W, (int64_t)(A - 1) * L.ldw + L.K - 1);
  rd(L.bias, A - 1);
  if (L.out) wr(L.out, (M - 1) * L.ldo + A - 1);
}
void ls_launch_head_ppo_gaussian(const HeadLayer& L, const PpoLossParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t s) {
  record("head_ppo_gaussian", blocks, s, lds_bytes);
  g_head = L; g_ppo = p;
  head_touch(L, p.M, p.A, blocks);
  if (p.idx) rd(p.idx, p.M - 1);
  rd(p.actions, (g_pool - 1) * p.lda + p.A - 1);
  if (p.algo != 1) rd(p.old_ll, g_pool - 1);
  rd(p.adv, g_pool - 1); rd(p.log_std, 0);
  if (p.dmean) wr(p.dmean, (p.M - 1) * p.ldm + p.A - 1);
  if (p.ll_out) wr(p.ll_out, p.M - 1);
  wr(p.partials, 2 * (int64_t)blocks - 1);
}
void ls_launch_head_gaussian_nll(const HeadLayer& L, const NllParams& p, unsigned blocks,
                                 unsigned lds_bytes, hipStream_t s) {
  record("head_gaussian_nll", blocks, s, lds_bytes);
  g_head = L; g_nll = p;
  head_touch(L, p.M, 1, blocks);
  if (p.idx) rd(p.idx, p.M - 1);
  rd(p.returns, g_pool - 1); rd(p.log_std, 0);
  if (p.dv) wr(p.dv, (p.M - 1) * p.ldv);
  wr(p.partials, 2 * (int64_t)blocks - 1);
}

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "fake"; }
}

// ---- the arguments of the entry points, in buffers of exactly the required size -------------
static const int64_t N_SPLITS = 3, SLAB_STRIDE = 16;
static const ga_stream_t ST = (ga_stream_t)S1;

// what the Gaussian, the categorical and the head-Gaussian entry share
struct Policy {
  int64_t M, pool;
  int A;
  int64_t ld, lda;
  int algo = 0;
  float *head, *actions, *old_ll, *adv, *log_std, *seed, *ll, *loss, *slabs, *ent;
  double *ws, *ent_sum;
  int32_t* idx;
  Policy(int64_t M_, int A_, bool gather = false, bool categorical = false)
      : M(M_), pool(gather ? M_ + 37 : M_), A(A_), ld(A_ + 2), lda(A_ + 5) {
    const int aw = categorical ? 1 : A;
    head = dev<float>((M - 1) * ld + A); actions = dev<float>((pool - 1) * lda + aw);
    old_ll = dev<float>(pool); adv = dev<float>(pool); log_std = dev<float>(1);
    seed = dev<float>((M - 1) * ld + A); ll = dev<float>(M); ent = dev<float>(M);
    loss = dev<float>(1); slabs = dev<float>((N_SPLITS - 1) * SLAB_STRIDE + 1);
    ws = workspace(); ent_sum = dev<double>(1);
    idx = gather ? dev<int32_t>(M) : nullptr;
  }
  int gauss() {
    g_pool = pool;
    return ga_ppo_gaussian_loss_f32(head, ld, actions, lda, old_ll, adv, idx, log_std, 3,
                                    -1.5f, 1, 0.75f, M, A, algo, 0.25f, 0.02f, 5, seed, ll,
                                    loss, slabs, SLAB_STRIDE, N_SPLITS, ws, ST);
  }
  int cat() {
    g_pool = pool;
    return ga_ppo_categorical_loss_f32(head, ld, actions, lda, old_ll, adv, idx, M, A, 1, algo,
                                       0.25f, 0.02f, 5, seed, ll, ent, loss, ent_sum, slabs,
                                       SLAB_STRIDE, N_SPLITS, ws, ST);
  }
};
struct Value {
  int64_t M, pool, ldv = 3;
  float *v, *returns, *log_std, *dv, *loss, *slabs;
  double* ws;
  int32_t* idx;
  explicit Value(int64_t M_, bool gather = false) : M(M_), pool(gather ? M_ + 37 : M_) {
    v = dev<float>((M - 1) * ldv + 1); returns = dev<float>(pool); log_std = dev<float>(1);
    dv = dev<float>((M - 1) * ldv + 1); loss = dev<float>(1);
    slabs = dev<float>((N_SPLITS - 1) * SLAB_STRIDE + 1); ws = workspace();
    idx = gather ? dev<int32_t>(M) : nullptr;
  }
  int nll() {
    g_pool = pool;
    return ga_gaussian_nll_loss_f32(v, ldv, returns, idx, log_std, M, dv, loss, slabs,
                                    SLAB_STRIDE, N_SPLITS, ws, ST);
  }
};
// the head layer in front of a policy / value loss
struct Head {
  int K;
  int64_t ldh, ldw, ldo;
  float *H, *W, *bias, *out;
  Head(int64_t M, int A, int K_) : K(K_), ldh(K_ + 4), ldw(K_ + 8), ldo(A + 3) {
    H = dev<float>((M - 1) * ldh + K); W = dev<float>((int64_t)(A - 1) * ldw + K);
    bias = dev<float>(A); out = dev<float>((M - 1) * ldo + A);
  }
};
static int head_gauss(Policy& p, Head& h) {
  g_pool = p.pool;
  return ga_head_ppo_gaussian_loss_f32(h.H, h.ldh, h.W, h.ldw, h.bias, h.K, h.out, h.ldo,
                                       p.actions, p.lda, p.old_ll, p.adv, p.idx, p.log_std, 3,
                                       -1.5f, 1, 0.75f, p.M, p.A, p.algo, 0.25f, 0.02f, 5,
                                       p.seed, p.ld, p.ll, p.loss, p.slabs, SLAB_STRIDE,
                                       N_SPLITS, p.ws, ST);
}
// (the value head's W is one row: no stride)
static int head_nll(Value& v, Head& h) {
  g_pool = v.pool;
  return ga_head_gaussian_nll_loss_f32(h.H, h.ldh, h.W, h.bias, h.K, h.out, h.ldo, v.returns,
                                       v.idx, v.log_std, v.M, v.dv, v.ldv, v.loss, v.slabs,
                                       SLAB_STRIDE, N_SPLITS, v.ws, ST);
}

// ---- refusals: the return code, the message, and nothing launched ---------------------------
static void refused(const char* file, int line, int rc, const char* message) {
  if (rc != -1 || g_error != message || !g_launches.empty()) {
    fprintf(stderr, "FAILED %s:%d: rc %d, error '%s' (want '%s'), %zu launch(es)\n", file, line,
            rc, g_error.c_str(), message, g_launches.size());
    ++g_failed;
  }
  reset();
}
#define REFUSED(call, message)              \
  do {                                      \
    reset();                                \
    const int rc__ = (call);                \
    refused(__FILE__, __LINE__, rc__, message); \
  } while (0)
// `call` with `field` set to `value` for the call
#define WITH(field, value, call, message)   \
  do {                                      \
    auto saved__ = field;                   \
    field = value;                          \
    REFUSED(call, message);                 \
    field = saved__;                        \
  } while (0)

static void test_refusals() {
  {
    Policy p(300, 3);
    const char* null = "ga_ppo_gaussian_loss_f32: null pointer";
    WITH(p.head, nullptr, p.gauss(), null); WITH(p.actions, nullptr, p.gauss(), null);
    WITH(p.adv, nullptr, p.gauss(), null); WITH(p.log_std, nullptr, p.gauss(), null);
    WITH(p.loss, nullptr, p.gauss(), null); WITH(p.ws, nullptr, p.gauss(), null);
    WITH(p.old_ll, nullptr, p.gauss(), "ga_ppo_gaussian_loss_f32: PPO needs old_ll");
    p.algo = 2;
    WITH(p.old_ll, nullptr, p.gauss(), "ga_ppo_gaussian_loss_f32: PPO needs old_ll");
    p.algo = 0;
    const char* sizes = "ga_ppo_gaussian_loss_f32: bad sizes";
    WITH(p.M, 0, p.gauss(), sizes); WITH(p.A, 0, p.gauss(), sizes);
    WITH(p.ld, 2, p.gauss(), sizes); WITH(p.lda, 2, p.gauss(), sizes);
    // the null pointer is reported before the sizes
    p.M = 0;
    WITH(p.head, nullptr, p.gauss(), null);
    p.M = 300;
    // VPG does not read old_ll; the optional outputs may be absent
    reset();
    p.algo = 1; p.old_ll = nullptr; p.seed = nullptr; p.ll = nullptr; p.slabs = nullptr;
    CHECK(p.gauss() == 0 && names() == "ppo_gaussian_loss ppo_gaussian_finalize");
  }
  {
    Policy p(300, 3, false, true);
    const char* null = "ga_ppo_categorical_loss_f32: null pointer";
    WITH(p.head, nullptr, p.cat(), null); WITH(p.actions, nullptr, p.cat(), null);
    WITH(p.adv, nullptr, p.cat(), null); WITH(p.loss, nullptr, p.cat(), null);
    WITH(p.ws, nullptr, p.cat(), null);
    WITH(p.old_ll, nullptr, p.cat(), "ga_ppo_categorical_loss_f32: PPO needs old_ll");
    const char* sizes = "ga_ppo_categorical_loss_f32: bad sizes";
    WITH(p.M, 0, p.cat(), sizes); WITH(p.A, 0, p.cat(), sizes);
    WITH(p.ld, 2, p.cat(), sizes); WITH(p.lda, 0, p.cat(), sizes);
    reset();
    p.algo = 1; p.old_ll = nullptr; p.seed = nullptr; p.ll = nullptr; p.ent = nullptr;
    p.ent_sum = nullptr; p.slabs = nullptr;
    CHECK(p.cat() == 0 && names() == "ppo_categorical_loss ppo_categorical_finalize");
  }
  {
    Value v(300);
    const char* null = "ga_gaussian_nll_loss_f32: null pointer";
    WITH(v.v, nullptr, v.nll(), null); WITH(v.returns, nullptr, v.nll(), null);
    WITH(v.log_std, nullptr, v.nll(), null); WITH(v.loss, nullptr, v.nll(), null);
    WITH(v.ws, nullptr, v.nll(), null);
    WITH(v.M, 0, v.nll(), "ga_gaussian_nll_loss_f32: bad sizes");
    WITH(v.ldv, 0, v.nll(), "ga_gaussian_nll_loss_f32: bad sizes");
  }
  {  // the two KL sums
    const int64_t M = 300, ld = 5;
    const int A = 3;
    float *a = dev<float>((M - 1) * ld + A), *b = dev<float>((M - 1) * ld + A);
    double *out = dev<double>(1), *ws = workspace();
    const char* null = "ga_categorical_kl_f32: null pointer";
    REFUSED(ga_categorical_kl_f32(nullptr, b, ld, M, A, 1, out, ws, ST), null);
    REFUSED(ga_categorical_kl_f32(a, nullptr, ld, M, A, 1, out, ws, ST), null);
    REFUSED(ga_categorical_kl_f32(a, b, ld, M, A, 1, nullptr, ws, ST), null);
    REFUSED(ga_categorical_kl_f32(a, b, ld, M, A, 1, out, nullptr, ST), null);
    const char* sizes = "ga_categorical_kl_f32: bad sizes";
    REFUSED(ga_categorical_kl_f32(a, b, ld, 0, A, 1, out, ws, ST), sizes);
    REFUSED(ga_categorical_kl_f32(a, b, ld, M, 0, 1, out, ws, ST), sizes);
    REFUSED(ga_categorical_kl_f32(a, b, 2, M, A, 1, out, ws, ST), sizes);
    null = "ga_gaussian_kl_f32: null pointer";
    REFUSED(ga_gaussian_kl_f32(nullptr, b, ld, M, A, 0.f, 0.f, out, ws, ST), null);
    REFUSED(ga_gaussian_kl_f32(a, nullptr, ld, M, A, 0.f, 0.f, out, ws, ST), null);
    REFUSED(ga_gaussian_kl_f32(a, b, ld, M, A, 0.f, 0.f, nullptr, ws, ST), null);
    REFUSED(ga_gaussian_kl_f32(a, b, ld, M, A, 0.f, 0.f, out, nullptr, ST), null);
    sizes = "ga_gaussian_kl_f32: bad sizes";
    REFUSED(ga_gaussian_kl_f32(a, b, ld, 0, A, 0.f, 0.f, out, ws, ST), sizes);
    REFUSED(ga_gaussian_kl_f32(a, b, ld, M, 0, 0.f, 0.f, out, ws, ST), sizes);
    REFUSED(ga_gaussian_kl_f32(a, b, 2, M, A, 0.f, 0.f, out, ws, ST), sizes);
  }
  {  // slab reductions and the Adam steps: n % 4, stride % 4, 16-byte alignment
    const int64_t n = 520, stride = 524, ns = 3;
    float *slabs = dev<float>((ns - 1) * stride + n), *out = dev<float>(n + 4);
    float *p = dev<float>(n + 4), *g = dev<float>(n + 4), *m = dev<float>(n + 4),
          *v = dev<float>(n + 4);
    const char* null = "ga_reduce_slabs_f32: null pointer";
    REFUSED(ga_reduce_slabs_f32(nullptr, ns, stride, n, 1.f, out, ST), null);
    REFUSED(ga_reduce_slabs_f32(slabs, ns, stride, n, 1.f, nullptr, ST), null);
    const char* mult = "ga_reduce_slabs_f32: n and stride must be multiples of 4";
    REFUSED(ga_reduce_slabs_f32(slabs, ns, stride, 0, 1.f, out, ST), mult);
    REFUSED(ga_reduce_slabs_f32(slabs, ns, stride, n - 2, 1.f, out, ST), mult);
    REFUSED(ga_reduce_slabs_f32(slabs, ns, stride + 2, n, 1.f, out, ST), mult);
    REFUSED(ga_reduce_slabs_f32(slabs, 0, stride, n, 1.f, out, ST), mult);
    const char* align = "ga_reduce_slabs_f32: 16-B alignment required";
    REFUSED(ga_reduce_slabs_f32(slabs + 1, ns, stride, n, 1.f, out, ST), align);
    REFUSED(ga_reduce_slabs_f32(slabs, ns, stride, n, 1.f, out + 2, ST), align);

    auto ra = [&](const float* s, float* p_, float* g_, float* m_, float* v_, int64_t n_,
                  int64_t stride_, int64_t ns_, int64_t step) {
      return ga_reduce_adam_f32(s, ns_, stride_, p_, g_, m_, v_, n_, step, 1e-3, 0.9, 0.999,
                                1e-8, 0, ST);
    };
    null = "ga_reduce_adam_f32: null pointer";
    REFUSED(ra(nullptr, p, g, m, v, n, stride, ns, 1), null);
    REFUSED(ra(slabs, nullptr, g, m, v, n, stride, ns, 1), null);
    REFUSED(ra(slabs, p, nullptr, m, v, n, stride, ns, 1), null);
    REFUSED(ra(slabs, p, g, nullptr, v, n, stride, ns, 1), null);
    REFUSED(ra(slabs, p, g, m, nullptr, n, stride, ns, 1), null);
    const char* sizes = "ga_reduce_adam_f32: bad sizes";
    REFUSED(ra(slabs, p, g, m, v, 0, stride, ns, 1), sizes);
    REFUSED(ra(slabs, p, g, m, v, n - 1, stride, ns, 1), sizes);
    REFUSED(ra(slabs, p, g, m, v, n, stride + 1, ns, 1), sizes);
    REFUSED(ra(slabs, p, g, m, v, n, stride, 0, 1), sizes);
    REFUSED(ra(slabs, p, g, m, v, n, stride, ns, 0), sizes);
    align = "ga_reduce_adam_f32: 16-B alignment required";
    REFUSED(ra(slabs + 1, p, g, m, v, n, stride, ns, 1), align);
    REFUSED(ra(slabs, p + 1, g, m, v, n, stride, ns, 1), align);
    REFUSED(ra(slabs, p, g + 2, m, v, n, stride, ns, 1), align);
    REFUSED(ra(slabs, p, g, m + 3, v, n, stride, ns, 1), align);
    REFUSED(ra(slabs, p, g, m, v + 1, n, stride, ns, 1), align);

    null = "ga_adam_step_f32: null pointer";
    REFUSED(ga_adam_step_f32(nullptr, g, m, v, n, 1, 1e-3, 0.9, 0.999, 1e-8, ST), null);
    REFUSED(ga_adam_step_f32(p, nullptr, m, v, n, 1, 1e-3, 0.9, 0.999, 1e-8, ST), null);
    REFUSED(ga_adam_step_f32(p, g, nullptr, v, n, 1, 1e-3, 0.9, 0.999, 1e-8, ST), null);
    REFUSED(ga_adam_step_f32(p, g, m, nullptr, n, 1, 1e-3, 0.9, 0.999, 1e-8, ST), null);
    REFUSED(ga_adam_step_f32(p, g, m, v, 0, 1, 1e-3, 0.9, 0.999, 1e-8, ST),
            "ga_adam_step_f32: bad n / step");
    REFUSED(ga_adam_step_f32(p, g, m, v, n, 0, 1e-3, 0.9, 0.999, 1e-8, ST),
            "ga_adam_step_f32: bad n / step");

    // ga_optimizer_step_f32: kind outside 1 .. 3, and each kind's state buffers
    const double h[5] = {0.01, 0.9, 0.3, 1e-4, 0.5};
    float *s1 = m, *s2 = v, *s3 = out;
    null = "ga_optimizer_step_f32: null pointer";
    REFUSED(ga_optimizer_step_f32(1, nullptr, g, s1, s2, s3, n, 1, h, 0, ST), null);
    REFUSED(ga_optimizer_step_f32(1, p, nullptr, s1, s2, s3, n, 1, h, 0, ST), null);
    REFUSED(ga_optimizer_step_f32(1, p, g, s1, s2, s3, n, 1, nullptr, 0, ST), null);
    const char* bad = "ga_optimizer_step_f32: bad n / step / kind";
    REFUSED(ga_optimizer_step_f32(0, p, g, s1, s2, s3, n, 1, h, 0, ST), bad);
    REFUSED(ga_optimizer_step_f32(4, p, g, s1, s2, s3, n, 1, h, 0, ST), bad);
    REFUSED(ga_optimizer_step_f32(-1, p, g, s1, s2, s3, n, 1, h, 0, ST), bad);
    REFUSED(ga_optimizer_step_f32(1, p, g, s1, s2, s3, 0, 1, h, 0, ST), bad);
    REFUSED(ga_optimizer_step_f32(1, p, g, s1, s2, s3, n, 0, h, 0, ST), bad);
    REFUSED(ga_optimizer_step_f32(1, p, g, nullptr, s2, s3, n, 1, h, 0, ST),
            "ga_optimizer_step_f32: SGD momentum buffer");
    const char* rms = "ga_optimizer_step_f32: RMSprop state buffers";
    REFUSED(ga_optimizer_step_f32(2, p, g, nullptr, s2, s3, n, 1, h, 0, ST), rms);
    REFUSED(ga_optimizer_step_f32(2, p, g, s1, nullptr, s3, n, 1, h, 0, ST), rms);  // momentum
    REFUSED(ga_optimizer_step_f32(2, p, g, s1, s2, nullptr, n, 1, h, 1, ST), rms);  // centered
    const char* adam = "ga_optimizer_step_f32: Adam state buffers";
    REFUSED(ga_optimizer_step_f32(3, p, g, nullptr, s2, s3, n, 1, h, 0, ST), adam);
    REFUSED(ga_optimizer_step_f32(3, p, g, s1, nullptr, s3, n, 1, h, 0, ST), adam);
    REFUSED(ga_optimizer_step_f32(3, p, g, s1, s2, nullptr, n, 1, h, 1, ST), adam);  // amsgrad
    // ... and what each kind does not need may be absent
    const double h0[5] = {0.01, 0.0, 0.3, 1e-4, 0.0};
    reset();
    CHECK(ga_optimizer_step_f32(1, p, g, nullptr, nullptr, nullptr, n, 1, h0, 0, ST) == 0);
    CHECK(ga_optimizer_step_f32(2, p, g, s1, nullptr, nullptr, n, 1, h0, 0, ST) == 0);
    CHECK(ga_optimizer_step_f32(3, p, g, s1, s2, nullptr, n, 1, h, 2, ST) == 0);
    CHECK(names() == "optimizer_step optimizer_step optimizer_step");
  }
  {  // statistics and the vector ops
    const int64_t n = 300;
    float *x = dev<float>(n), *y = dev<float>(n);
    double *stats = dev<double>(4), *ws = workspace(), *out = dev<double>(1);
    const char* null = "ga_stats_f32: null pointer";
    REFUSED(ga_stats_f32(nullptr, n, 0, stats, ws, ST), null);
    REFUSED(ga_stats_f32(x, n, 0, nullptr, ws, ST), null);
    REFUSED(ga_stats_f32(x, n, 0, stats, nullptr, ST), null);
    REFUSED(ga_stats_f32(x, 0, 0, stats, ws, ST), "ga_stats_f32: bad arguments");
    REFUSED(ga_stats_f32(x, n, -1, stats, ws, ST), "ga_stats_f32: bad arguments");
    REFUSED(ga_stats_f32(x, n, 3, stats, ws, ST), "ga_stats_f32: bad arguments");
    const char* bad = "ga_adv_center_f32: bad arguments";
    REFUSED(ga_adv_center_f32(nullptr, n, stats, 1e-8f, ST), bad);
    REFUSED(ga_adv_center_f32(x, n, nullptr, 1e-8f, ST), bad);
    REFUSED(ga_adv_center_f32(x, 0, stats, 1e-8f, ST), bad);
    bad = "ga_sub_scalar_f32: bad arguments";
    REFUSED(ga_sub_scalar_f32(nullptr, n, out, ST), bad);
    REFUSED(ga_sub_scalar_f32(x, n, nullptr, ST), bad);
    REFUSED(ga_sub_scalar_f32(x, 0, out, ST), bad);
    bad = "ga_dot_f32: bad arguments";
    REFUSED(ga_dot_f32(nullptr, y, n, out, ST), bad); REFUSED(ga_dot_f32(x, nullptr, n, out, ST), bad);
    REFUSED(ga_dot_f32(x, y, n, nullptr, ST), bad); REFUSED(ga_dot_f32(x, y, 0, out, ST), bad);
    bad = "ga_axpby_f32: bad arguments";
    REFUSED(ga_axpby_f32(1.0, nullptr, 1.0, y, n, ST), bad);
    REFUSED(ga_axpby_f32(1.0, x, 1.0, nullptr, n, ST), bad);
    REFUSED(ga_axpby_f32(1.0, x, 1.0, y, 0, ST), bad);
  }
  {  // the Fisher seeds: A > FS_MAX_A is the categorical one's own limit
    const int64_t M = 300, ld = 36;
    float *a = dev<float>((M - 1) * ld + 33), *t = dev<float>((M - 1) * ld + 33),
          *d = dev<float>(M * ld), *ls = dev<float>(1);
    const char* bad = "ga_fisher_seed_gaussian_f32: bad arguments";
    REFUSED(ga_fisher_seed_gaussian_f32(nullptr, ld, M, 3, ls, 0, 0.f, 0, 0.f, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, ld, M, 3, nullptr, 0, 0.f, 0, 0.f, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, ld, M, 3, ls, 0, 0.f, 0, 0.f, nullptr, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, ld, 0, 3, ls, 0, 0.f, 0, 0.f, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, ld, M, 0, ls, 0, 0.f, 0, 0.f, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, 2, M, 3, ls, 0, 0.f, 0, 0.f, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_gaussian_f32(t, ld, M, 3, ls, 0, 0.f, 0, 0.f, d, 2, ST), bad);
    reset();
    CHECK(ga_fisher_seed_gaussian_f32(t, ld, M, 33, ls, 0, 0.f, 0, 0.f, d, ld, ST) == 0);
    bad = "ga_fisher_seed_categorical_f32: bad arguments";
    REFUSED(ga_fisher_seed_categorical_f32(nullptr, ld, t, ld, M, 3, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, nullptr, ld, M, 3, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, ld, M, 3, 1, nullptr, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, ld, 0, 3, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, ld, M, 0, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, ld, M, 33, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, 2, t, ld, M, 3, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, 2, M, 3, 1, d, ld, ST), bad);
    REFUSED(ga_fisher_seed_categorical_f32(a, ld, t, ld, M, 3, 1, d, 2, ST), bad);
    reset();
    CHECK(ga_fisher_seed_categorical_f32(a, ld, t, ld, M, 32, 1, d, ld, ST) == 0);
    CHECK(names() == "fisher_seed_categorical");
  }
  {  // the head entries
    Policy p(100, 3);
    Head h(100, 3, 128);
    const char* null = "ga_head_ppo_gaussian_loss_f32: null pointer";
    WITH(h.H, nullptr, head_gauss(p, h), null); WITH(h.W, nullptr, head_gauss(p, h), null);
    WITH(h.bias, nullptr, head_gauss(p, h), null);
    WITH(p.actions, nullptr, head_gauss(p, h), null); WITH(p.adv, nullptr, head_gauss(p, h), null);
    WITH(p.log_std, nullptr, head_gauss(p, h), null); WITH(p.loss, nullptr, head_gauss(p, h), null);
    WITH(p.ws, nullptr, head_gauss(p, h), null);
    WITH(h.K, 0, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 0");
    WITH(h.K, 32, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 32");
    WITH(h.K, 192, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 192");
    WITH(h.K, 320, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 320");
    WITH(h.K, 1024, head_gauss(p, h),
         "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 1024");
    WITH(p.A, 0, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 0 x 128");
    WITH(p.A, 65, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 65 x 128");
    // A * K * 4 > 60 KiB: 30 x 512 floats are 60 KiB exactly, the largest head at that width
    h.K = 512;
    WITH(p.A, 31, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 31 x 512");
    h.K = 128;
    // the head's shape is reported before old_ll, old_ll before the sizes
    p.old_ll = nullptr;
    WITH(h.K, 32, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: unsupported head 3 x 32");
    WITH(p.M, 0, head_gauss(p, h), "ga_head_ppo_gaussian_loss_f32: PPO needs old_ll");
    p.old_ll = p.adv;
    const char* sizes = "ga_head_ppo_gaussian_loss_f32: bad sizes / alignment";
    WITH(p.M, 0, head_gauss(p, h), sizes);
    WITH(h.ldh, 124, head_gauss(p, h), sizes); WITH(h.ldh, 130, head_gauss(p, h), sizes);
    WITH(h.ldw, 124, head_gauss(p, h), sizes); WITH(h.ldw, 130, head_gauss(p, h), sizes);
    WITH(p.lda, 2, head_gauss(p, h), sizes); WITH(p.ld, 2, head_gauss(p, h), sizes);
    WITH(h.ldo, 2, head_gauss(p, h), sizes);
    WITH(h.H, h.H + 1, head_gauss(p, h), sizes); WITH(h.W, h.W + 2, head_gauss(p, h), sizes);
    // without the optional outputs their strides are not looked at
    reset();
    p.seed = nullptr; p.ld = 0; h.out = nullptr; h.ldo = 0;
    CHECK(head_gauss(p, h) == 0 && names() == "head_ppo_gaussian ppo_gaussian_finalize");
    CHECK(ga_head_loss_supported(512, 30) == 1 && ga_head_loss_supported(512, 31) == 0 &&
          ga_head_loss_supported(256, 60) == 1 && ga_head_loss_supported(256, 61) == 0 &&
          ga_head_loss_supported(64, 64) == 1 && ga_head_loss_supported(64, 65) == 0 &&
          ga_head_loss_supported(96, 1) == 0);
  }
  {
    Value v(100);
    Head h(100, 1, 256);
    const char* null = "ga_head_gaussian_nll_loss_f32: null pointer";
    WITH(h.H, nullptr, head_nll(v, h), null); WITH(h.W, nullptr, head_nll(v, h), null);
    WITH(h.bias, nullptr, head_nll(v, h), null); WITH(v.returns, nullptr, head_nll(v, h), null);
    WITH(v.log_std, nullptr, head_nll(v, h), null); WITH(v.loss, nullptr, head_nll(v, h), null);
    WITH(v.ws, nullptr, head_nll(v, h), null);
    WITH(h.K, 32, head_nll(v, h), "ga_head_gaussian_nll_loss_f32: unsupported hidden width 32");
    WITH(h.K, 384, head_nll(v, h), "ga_head_gaussian_nll_loss_f32: unsupported hidden width 384");
    WITH(h.K, 1024, head_nll(v, h),
         "ga_head_gaussian_nll_loss_f32: unsupported hidden width 1024");
    const char* sizes = "ga_head_gaussian_nll_loss_f32: bad sizes / alignment";
    WITH(v.M, 0, head_nll(v, h), sizes);
    WITH(h.ldh, 252, head_nll(v, h), sizes); WITH(h.ldh, 258, head_nll(v, h), sizes);
    WITH(v.ldv, 0, head_nll(v, h), sizes); WITH(h.ldo, 0, head_nll(v, h), sizes);
    WITH(h.H, h.H + 3, head_nll(v, h), sizes); WITH(h.W, h.W + 1, head_nll(v, h), sizes);
  }
  free_all();
}

// ---- grids ------------------------------------------------------------------------------------
static void test_grids() {
  CHECK(ga_reduction_workspace_doubles() == 1026 && ga_reduction_partials_doubles() == 1024);
  // red_blocks, through every entry point that sizes its grid with it
  const int64_t rows[5] = {1, 256, 257, 131072, 131073};
  const unsigned want[5] = {1, 1, 2, 512, 512};
  for (int i = 0; i < 5; ++i) {
    const int64_t n = rows[i];
    float* x = dev<float>(n);
    double *stats = dev<double>(4), *ws = workspace(), *out = dev<double>(1);
    reset();
    CHECK(ga_stats_f32(x, n, 1, stats, ws, ST) == 0);
    CHECK(ga_adv_center_f32(x, n, stats, 1e-8f, ST) == 0);
    CHECK(ga_sub_scalar_f32(x, n, out, ST) == 0);
    CHECK(ga_gaussian_kl_f32(x, x, 1, n, 1, 0.25f, -0.5f, out, ws, ST) == 0);
    CHECK(ga_categorical_kl_f32(x, x, 1, n, 1, 1, out, ws, ST) == 0);
    CHECK(names() == "stats adv_center sub_scalar gaussian_kl sum_partials categorical_kl "
                     "sum_partials");
    if (g_launches.size() == 7) {
      for (int k : {0, 1, 2, 3, 5}) CHECK(g_launches[k].blocks == want[i]);
      CHECK(g_launches[4].arg == (int)want[i] && g_launches[6].arg == (int)want[i]);
      CHECK(g_launches[5].arg == 1);  // double_softmax
    }
    CHECK(g_kl_s_old == 0.25f && g_kl_s_new == -0.5f);
    Policy p(n, 1);
    Policy c(n, 3, false, true);
    Value v(n);
    reset();
    CHECK(p.gauss() == 0 && c.cat() == 0 && v.nll() == 0);
    int seen = 0;
    for (auto& l : g_launches)
      if (l.what == "ppo_gaussian_loss" || l.what == "ppo_categorical_loss" ||
          l.what == "gaussian_nll") {
        CHECK(l.blocks == want[i]);
        ++seen;
      }
    CHECK(seen == 3);
    free_all();
  }
  // ga_stats_f32 hands `what` through
  {
    float* x = dev<float>(300);
    double *stats = dev<double>(4), *ws = workspace();
    reset();
    for (int what = 0; what < 3; ++what) CHECK(ga_stats_f32(x, 300, what, stats, ws, ST) == 0);
    CHECK(g_launches.size() == 3);
    for (int what = 0; what < 3 && g_launches.size() == 3; ++what)
      CHECK(g_launches[what].arg == what && g_launches[what].blocks == 2);
  }
  // slab reductions: ceil(n / 4 / 64); the Adam and optimizer launches, axpby and the Fisher
  // seeds: ceil(n / 256); the dot product: one workgroup
  const int64_t ns[5] = {4, 256, 260, 1024, 72196};
  const unsigned blocks[5] = {1, 1, 2, 4, 283};
  for (int i = 0; i < 5; ++i) {
    const int64_t n = ns[i], stride = n + 8;
    float *slabs = dev<float>(2 * stride + n), *out = dev<float>(n), *p = dev<float>(n),
          *g = dev<float>(n), *m = dev<float>(n), *v = dev<float>(n), *ls = dev<float>(1);
    double* d = dev<double>(1);
    const double h[5] = {0.01, 0.9, 0.3, 1e-4, 0.5};
    reset();
    CHECK(ga_reduce_slabs_f32(slabs, 3, stride, n, 0.5f, out, ST) == 0 && g_scale == 0.5f);
    CHECK(ga_reduce_adam_f32(slabs, 3, stride, p, g, m, v, n, 2, 1e-3, 0.9, 0.999, 1e-8, 1,
                             ST) == 0 && g_zero_slot0 == 1);
    CHECK(ga_adam_step_f32(p, g, m, v, n, 2, 1e-3, 0.9, 0.999, 1e-8, ST) == 0);
    CHECK(ga_optimizer_step_f32(2, p, g, m, v, out, n, 2, h, 1, ST) == 0);
    CHECK(ga_axpby_f32(0.5, p, -2.0, g, n, ST) == 0 && g_alpha == 0.5f && g_beta == -2.f);
    CHECK(ga_fisher_seed_gaussian_f32(p, 1, n, 1, ls, 0, 0.f, 0, 0.f, g, 1, ST) == 0);
    CHECK(ga_fisher_seed_categorical_f32(p, 1, m, 1, n, 1, 0, g, 1, ST) == 0);
    CHECK(ga_dot_f32(p, g, n, d, ST) == 0);
    CHECK(names() == "reduce_slabs reduce_adam adam optimizer_step axpby fisher_seed_gaussian "
                     "fisher_seed_categorical dot");
    if (g_launches.size() == 8) {
      for (int k = 0; k < 7; ++k) CHECK(g_launches[k].blocks == blocks[i]);
      CHECK(g_launches[7].blocks == 1);
    }
    free_all();
  }
  // n = 1028: 257 quads -> 5 blocks of 64 quads, 1028 elements -> 5 blocks of 256
  {
    const int64_t n = 1028;
    float *slabs = dev<float>(n), *out = dev<float>(n);
    reset();
    CHECK(ga_reduce_slabs_f32(slabs, 1, n, n, 1.f, out, ST) == 0 && g_launches[0].blocks == 5);
    free_all();
  }
  // head_blocks: 64 rows per workgroup, at most 512 workgroups
  const int64_t hrows[5] = {1, 64, 65, 32768, 32769};
  const unsigned hwant[5] = {1, 1, 2, 512, 512};
  for (int i = 0; i < 5; ++i) {
    Policy p(hrows[i], 3);
    Value v(hrows[i]);
    Head hp(hrows[i], 3, 64), hv(hrows[i], 1, 512);
    reset();
    CHECK(head_gauss(p, hp) == 0 && head_nll(v, hv) == 0);
    CHECK(names() ==
          "head_ppo_gaussian ppo_gaussian_finalize head_gaussian_nll gaussian_nll_finalize");
    if (g_launches.size() == 4) {
      CHECK(g_launches[0].blocks == hwant[i] && g_launches[2].blocks == hwant[i]);
      CHECK(g_launches[1].arg == (int)hwant[i] && g_launches[3].arg == (int)hwant[i]);
    }
    free_all();
  }
}

// ---- one launch or two; the ticket; the structs field by field -----------------------------
static void ent_is(const LossEnt& e) {  // ent_coeff 0.02, ent_flags 5
  CHECK(e.coeff == 0.02f && e.regularized == 1 && e.softplus == 0 && e.stop_grad == 1);
}
static void gauss_rows_are(const PpoLossParams& q, const Policy& p) {
  CHECK(q.actions == p.actions && q.lda == p.lda && q.old_ll == p.old_ll && q.adv == p.adv &&
        q.idx == p.idx && q.log_std == p.log_std && q.min_log_std == -1.5f && q.has_min == 3 &&
        q.max_log_std == 0.75f && q.has_max == 1 && q.M == p.M && q.A == p.A &&
        q.algo == p.algo && q.clip == 0.25f && q.dmean == p.seed && q.ll_out == p.ll &&
        q.partials == p.ws);
  ent_is(q.ent);
}
static void gauss_finalize_is(const Policy& p, int nb) {
  const PpoFinalizeParams& f = g_fin;
  CHECK(f.partials == p.ws && f.nblocks == nb && f.log_std == p.log_std &&
        f.min_log_std == -1.5f && f.max_log_std == 0.75f && f.has_min == 3 && f.has_max == 1 &&
        f.M == p.M && f.A == p.A && f.loss_out == p.loss && f.grad_slab0 == p.slabs &&
        f.slab_stride == 16 && f.n_splits == 3);
  ent_is(f.ent);
}
// a plain loss launch under the plan: finishes itself (loss_out passed) or not
template <class P, class A>
static void plan_is(const P& q, const A& a, bool finishes) {
  CHECK(q.loss_out == (finishes ? a.loss : nullptr));
  CHECK(q.grad_slab0 == a.slabs && q.slab_stride == 16 && q.n_splits == 3);
  // the word at double 2 * 512 of the workspace
  CHECK((void*)q.ticket == (void*)(a.ws + 1024));
}

static void test_one_launch_or_two() {
  const int64_t rows[3] = {1, 257, 131073};
  const int nbs[3] = {1, 2, 512};
  for (int on = 0; on < 2; ++on) {
    CHECK(ga_set_one_launch_losses(on ? 7 : 0) == 0);
    for (int i = 0; i < 3; ++i) {
      const bool one = on || nbs[i] == 1;
      for (int gather = 0; gather < 2; ++gather) {
        Policy p(rows[i], 3, gather != 0);
        p.algo = gather ? 2 : 0;
        reset();
        CHECK(p.gauss() == 0);
        CHECK(names() == (one ? "ppo_gaussian_loss" : "ppo_gaussian_loss ppo_gaussian_finalize"));
        CHECK(g_launches[0].blocks == (unsigned)nbs[i]);
        CHECK(g_ppo.mean == p.head && g_ppo.ldm == p.ld);
        gauss_rows_are(g_ppo, p);
        plan_is(g_ppo, p, one);
        if (!one) gauss_finalize_is(p, nbs[i]);

        Policy c(rows[i], 3, gather != 0, true);
        reset();
        CHECK(c.cat() == 0);
        CHECK(names() ==
              (one ? "ppo_categorical_loss" : "ppo_categorical_loss ppo_categorical_finalize"));
        CHECK(g_launches[0].blocks == (unsigned)nbs[i]);
        const CatLossParams& q = g_cat;
        CHECK(q.scores == c.head && q.lds == c.ld && q.actions == c.actions && q.lda == c.lda &&
              q.old_ll == c.old_ll && q.adv == c.adv && q.idx == c.idx && q.M == c.M &&
              q.A == 3 && q.double_softmax == 1 && q.algo == 0 && q.clip == 0.25f &&
              q.dscores == c.seed && q.ll_out == c.ll && q.ent_out == c.ent &&
              q.partials == c.ws && q.ent_sum_out == c.ent_sum);
        ent_is(q.ent);
        plan_is(q, c, one);
        if (!one) {
          const CatFinalize& f = g_cat_fin;
          CHECK(f.partials == c.ws && f.nblocks == nbs[i] && f.M == c.M && f.loss_out == c.loss &&
                f.ent_sum_out == c.ent_sum && f.grad_slab0 == c.slabs && f.slab_stride == 16 &&
                f.n_splits == 3);
        }

        Value v(rows[i], gather != 0);
        reset();
        CHECK(v.nll() == 0);
        CHECK(names() == (one ? "gaussian_nll" : "gaussian_nll gaussian_nll_finalize"));
        CHECK(g_launches[0].blocks == (unsigned)nbs[i]);
        const NllParams& n = g_nll;
        CHECK(n.v == v.v && n.ldv == 3 && n.returns == v.returns && n.idx == v.idx &&
              n.log_std == v.log_std && n.M == v.M && n.dv == v.dv && n.partials == v.ws);
        plan_is(n, v, one);
        if (!one) {
          const NllFinalize& f = g_nll_fin;
          CHECK(f.partials == v.ws && f.nblocks == nbs[i] && f.M == v.M && f.loss_out == v.loss &&
                f.grad_slab0 == v.slabs && f.slab_stride == 16 && f.n_splits == 3);
        }
        free_all();
      }
    }
    // the head entries always run two launches, whatever the switch says: null ticket and
    // null slab fields in the first
    for (int64_t M : {1, 65, 1000}) {
      Policy p(M, 3, M == 1000);
      Head h(M, 3, 256);
      reset();
      CHECK(head_gauss(p, h) == 0);
      CHECK(names() == "head_ppo_gaussian ppo_gaussian_finalize");
      const PpoLossParams& q = g_ppo;
      CHECK(q.mean == nullptr && q.ldm == p.ld);  // (ldd: the seed's stride)
      gauss_rows_are(q, p);
      CHECK(!q.loss_out && !q.grad_slab0 && q.slab_stride == 0 && q.n_splits == 0 && !q.ticket);
      CHECK(g_head.H == h.H && g_head.ldh == h.ldh && g_head.W == h.W && g_head.ldw == h.ldw &&
            g_head.bias == h.bias && g_head.K == 256 && g_head.out == h.out &&
            g_head.ldo == h.ldo);
      gauss_finalize_is(p, (int)g_launches[0].blocks);

      Value v(M, M == 1000);
      Head hv(M, 1, 128);
      reset();
      CHECK(head_nll(v, hv) == 0);
      CHECK(names() == "head_gaussian_nll gaussian_nll_finalize");
      const NllParams& n = g_nll;
      CHECK(n.v == nullptr && n.ldv == v.ldv && n.returns == v.returns && n.idx == v.idx &&
            n.log_std == v.log_std && n.M == v.M && n.dv == v.dv && n.partials == v.ws);
      CHECK(!n.loss_out && !n.grad_slab0 && n.slab_stride == 0 && n.n_splits == 0 && !n.ticket);
      CHECK(g_head.H == hv.H && g_head.ldh == hv.ldh && g_head.W == hv.W &&
            g_head.ldw == 128 &&  // the value head's one row: ldw is the hidden width
            g_head.bias == hv.bias && g_head.K == 128 && g_head.out == hv.out &&
            g_head.ldo == hv.ldo);
      const NllFinalize& f = g_nll_fin;
      CHECK(f.partials == v.ws && f.nblocks == (int)g_launches[0].blocks && f.M == v.M &&
            f.loss_out == v.loss && f.grad_slab0 == v.slabs && f.slab_stride == 16 &&
            f.n_splits == 3);
      free_all();
    }
  }
  ga_set_one_launch_losses(0);
}

// ---- the head kernels' dynamic LDS ----------------------------------------------------------
// W [A][K], the bias [round4(A)], 16 groups x 4 rows x A row buffers, 4 bytes each
static void test_head_lds() {
  const int As[5] = {1, 3, 8, 29, 30}, Ks[5] = {64, 256, 512, 512, 512};
  const unsigned bytes[5] = {528, 3856, 18464, 66944, 69248};
  for (int i = 0; i < 5; ++i) {
    Policy p(70, As[i]);
    Head h(70, As[i], Ks[i]);
    reset();
    CHECK(head_gauss(p, h) == 0);
    CHECK(g_launches.size() == 2 && g_launches[0].lds == bytes[i] && g_launches[1].lds == 0);
    free_all();
  }
  const unsigned vbytes[4] = {528, 784, 1296, 2320};  // the value head: A = 1
  const int vK[4] = {64, 128, 256, 512};
  for (int i = 0; i < 4; ++i) {
    Value v(70);
    Head h(70, 1, vK[i]);
    reset();
    CHECK(head_nll(v, h) == 0);
    CHECK(g_launches.size() == 2 && g_launches[0].lds == vbytes[i]);
    free_all();
  }
}

// ---- the optimizer coefficients: formed in double, rounded once ------------------------------
static void test_coefficients() {
  const int64_t n = 8;
  float *p = dev<float>(n), *g = dev<float>(n), *s1 = dev<float>(n), *s2 = dev<float>(n),
        *s3 = dev<float>(n);
  // the float complements differ from the rounded double ones: what the literals tell apart
  CHECK(1.f - 0.999f != 0x1.0624dep-10f && 1.f - 0.9f != 0x1.99999ap-4f &&
        1.f - 0.99f != 0x1.47ae14p-7f);
  {  // AdamW with amsgrad at step 3: h = {lr, beta1, beta2, eps, weight_decay}
    const double h[5] = {0.001, 0.9, 0.999, 1e-8, 0.01};
    reset();
    CHECK(ga_optimizer_step_f32(3, p, g, s1, s2, s3, n, 3, h, 3, ST) == 0);
    const OptParams& a = g_opt;
    CHECK(a.p == p && a.g == g && a.s1 == s1 && a.s2 == s2 && a.s3 == s3 && a.n == n &&
          a.kind == 3 && a.flags == 3 && a.first == 0);
    CHECK(a.neg_lr == -0x1.0624dep-10f && a.h1 == 0x1.ccccccp-1f && a.h2 == 0x1.ff7ceep-1f &&
          a.h3 == 0x1.5798eep-27f && a.h4 == 0x1.47ae14p-7f);
    CHECK(a.w1 == 0x1.99999ap-4f);             // (float)(1.0 - 0.9)
    CHECK(a.w2 == 0x1.0624dep-10f);            // (float)(1.0 - 0.999)
    CHECK(a.decay == 0x1.fffebp-1f);           // (float)(1.0 - 0.001 * 0.01)
    CHECK(a.neg_step_size == -0x1.e3a918p-9f); // (float)(-(0.001 / (1.0 - 0.9^3)))
    CHECK(a.bc2_sqrt == 0x1.c07852p-5f);       // (float)sqrt(1.0 - 0.999^3)
    reset();
    CHECK(ga_optimizer_step_f32(3, p, g, s1, s2, nullptr, n, 1, h, 0, ST) == 0);
    CHECK(g_opt.first == 1 && g_opt.neg_step_size == -0x1.47ae14p-7f &&
          g_opt.bc2_sqrt == 0x1.030dc4p-5f && g_opt.flags == 0);
  }
  {  // SGD: h = {lr, momentum, dampening, weight_decay}
    const double h[5] = {0.01, 0.9, 0.3, 1e-4, 123.0};
    reset();
    CHECK(ga_optimizer_step_f32(1, p, g, s1, nullptr, nullptr, n, 1, h, 1, ST) == 0);
    const OptParams& a = g_opt;
    CHECK(a.kind == 1 && a.flags == 1 && a.first == 1 && a.s2 == nullptr && a.s3 == nullptr);
    CHECK(a.neg_lr == -0x1.47ae14p-7f && a.h1 == 0x1.ccccccp-1f && a.h2 == 0x1.333334p-2f &&
          a.h3 == 0x1.a36e2ep-14f);
    CHECK(a.w1 == 0x1.666666p-1f);  // (float)(1.0 - 0.3)
    CHECK(a.w2 == 0.f && a.decay == 0.f && a.neg_step_size == 0.f && a.bc2_sqrt == 0.f);
    reset();
    CHECK(ga_optimizer_step_f32(1, p, g, s1, nullptr, nullptr, n, 2, h, 0, ST) == 0);
    CHECK(g_opt.first == 0);
  }
  {  // RMSprop: h = {lr, alpha, eps, weight_decay, momentum}
    const double h[5] = {0.01, 0.99, 1e-8, 0.0, 0.5};
    reset();
    CHECK(ga_optimizer_step_f32(2, p, g, s1, s2, s3, n, 5, h, 1, ST) == 0);
    const OptParams& a = g_opt;
    CHECK(a.kind == 2 && a.flags == 1 && a.first == 0);
    CHECK(a.neg_lr == -0x1.47ae14p-7f && a.h1 == 0x1.fae148p-1f && a.h2 == 0x1.5798eep-27f &&
          a.h3 == 0.f && a.h4 == 0.5f);
    CHECK(a.w1 == 0x1.47ae14p-7f);  // (float)(1.0 - 0.99)
    CHECK(a.w2 == 0.f && a.decay == 0.f && a.neg_step_size == 0.f && a.bc2_sqrt == 0.f);
  }
  {  // the one AdamParams of ga_adam_step_f32 and ga_reduce_adam_f32: lr 2.5e-4, eps 1e-5, step 7
    float* slabs = dev<float>(n);
    for (int which = 0; which < 2; ++which) {
      reset();
      memset(&g_adam, 0, sizeof(g_adam));
      if (which == 0)
        CHECK(ga_adam_step_f32(p, g, s1, s2, n, 7, 2.5e-4, 0.9, 0.999, 1e-5, ST) == 0);
      else
        CHECK(ga_reduce_adam_f32(slabs, 1, n, p, g, s1, s2, n, 7, 2.5e-4, 0.9, 0.999, 1e-5, 0,
                                 ST) == 0);
      const AdamParams& a = g_adam;
      CHECK(a.p == p && a.g == g && a.m == s1 && a.v == s2 && a.n == n);
      CHECK(a.c.lerp_w == 0x1.99999ap-4f && a.c.beta2 == 0x1.ff7ceep-1f &&
            a.c.one_minus_beta2 == 0x1.0624dep-10f && a.c.neg_step_size == -0x1.f67a34p-12f &&
            a.c.bc2_sqrt == 0x1.562ebp-4f && a.c.eps == 0x1.4f8b58p-17f);
    }
  }
  free_all();
}

int main(int argc, char** argv) {
  return run_suites(
      {
          {"refusals", test_refusals, "losses host refusals ok"},
          {"grids", test_grids, "losses host grids ok"},
          {"launches", test_one_launch_or_two, "losses host launches ok"},
          {"head-lds", test_head_lds, "losses host head lds ok"},
          {"coefficients", test_coefficients, "losses host ok"},
      },
      argc, argv);
}
