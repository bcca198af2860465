// Host-logic harness for the linear feature baseline's entry points
// (garage_amd/csrc/linear_baseline_host.cpp), built with -fsanitize=address,undefined on the
// CPU (`make asan-linear-baseline`).  The three launches of the seam
// (linear_baseline_params.h) are replaced by recording fakes; "device" memory is
// exactly-sized host memory, and each fake touches the first and the last byte its kernel
// would reach in every array, so that a grid, a stride or a workspace size that is off trips
// the sanitizer.  The checks are about the host's own work: every refusal precedes the first
// launch, the grids cover S on both sides of a slab boundary and of the grid's cap, the
// workspace sizes, tiles per wave, chunk rows and LDS bytes against literals, the parameter
// structs field by field.
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/linear_baseline_params.h"
#include "harness.h"

extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "fake"; }
}

// ---- what the fakes record -----------------------------------------------------
struct GramLaunch {
  LinGramParams p;
  unsigned blocks, lds;
};
struct ReduceLaunch {
  LinReduceParams p;
  unsigned blocks;
};
struct PredictLaunch {
  LinPredictParams p;
  unsigned blocks;
};
static std::vector<GramLaunch> g_gram;
static std::vector<ReduceLaunch> g_reduce;
static std::vector<PredictLaunch> g_predict;
static hipStream_t g_stream_seen = nullptr;

// touches byte `at` of a buffer (the sanitizer checks it lies inside)
static void touch(const void* p, int64_t at) {
  volatile char c = static_cast<const char*>(p)[at];
  (void)c;
}
static void touch_batch(const float* obs, int64_t ldo, int obs_dim, const int64_t* ep_off,
                        int64_t n_eps, int64_t S) {
  touch(obs, 0);
  touch(obs, ((S - 1) * ldo + obs_dim) * 4 - 1);
  touch(ep_off, 0);
  touch(ep_off, (n_eps + 1) * 8 - 1);
}

void lb_launch_gram(const LinGramParams& p, unsigned blocks, unsigned lds_bytes,
                    hipStream_t stream) {
  CHECK(g_reduce.size() == g_gram.size());
  g_gram.push_back({p, blocks, lds_bytes});
  g_stream_seen = stream;
  touch_batch(p.obs, p.ldo, p.obs_dim, p.ep_off, p.n_eps, p.S);
  touch(p.returns, 0);
  touch(p.returns, p.S * 4 - 1);
  touch(p.partials, 0);
  touch(p.partials, (int64_t)blocks * p.block_doubles * 8 - 1);
  // every slab has a workgroup, and no workgroup is idle
  CHECK(blocks >= 1 && blocks <= LB_MAX_BLOCKS && (int64_t)blocks <= p.n_slabs);
  CHECK(p.n_slabs * LB_SLAB_ROWS >= p.S && (p.n_slabs - 1) * LB_SLAB_ROWS < p.S);
  CHECK((int64_t)blocks == p.n_slabs || blocks == LB_MAX_BLOCKS);
  // the waves' tiles cover the triangle
  CHECK(p.tpw * LB_WAVES >= p.NT && p.tpw >= 1 && p.tpw <= LB_MAX_TPW);
  CHECK(p.chunk_rows == 8 || p.chunk_rows == 16 || p.chunk_rows == 32);
  CHECK(lds_bytes <= LB_LDS_BUDGET);
  CHECK(16 * p.T <= LB_THREADS && 16 * p.T >= p.F && 16 * (p.T - 1) < p.F);
}
void lb_launch_gram_reduce(const LinReduceParams& p, unsigned blocks, hipStream_t stream) {
  CHECK(g_gram.size() == g_reduce.size() + 1);  // after the Gram pass, on the stream
  CHECK(stream == g_stream_seen);
  g_reduce.push_back({p, blocks});
  touch(p.partials, (int64_t)p.n_blocks * p.block_doubles * 8 - 1);
  touch(p.gram, 0);
  touch(p.gram, (int64_t)p.F * p.F * 8 - 1);
  touch(p.rhs, (int64_t)p.F * 8 - 1);
  CHECK((int64_t)blocks * LB_REDUCE_THREADS >= p.block_doubles);
  CHECK((int64_t)(blocks - 1) * LB_REDUCE_THREADS < p.block_doubles);
}
void lb_launch_predict(const LinPredictParams& p, unsigned blocks, hipStream_t stream) {
  g_predict.push_back({p, blocks});
  g_stream_seen = stream;
  touch_batch(p.obs, p.ldo, p.obs_dim, p.ep_off, p.n_eps, p.S);
  touch(p.coeffs, (2 * p.obs_dim + 4) * 8 - 1);
  touch(p.values, 0);
  touch(p.values, ((p.S - 1) * p.ldv + 1) * 4 - 1);
  CHECK((int64_t)blocks * LB_PREDICT_THREADS >= p.S);
  CHECK((int64_t)(blocks - 1) * LB_PREDICT_THREADS < p.S);
}

static void reset() {
  g_gram.clear(); g_reduce.clear(); g_predict.clear(); g_error.clear();
  g_stream_seen = nullptr;
}

// ---- a call over exactly-sized buffers -------------------------------------------------
struct Call {
  int obs_dim = 17;
  int64_t ldo = 20, n_eps = 3, S = 100, ldv = 1;
  float *obs = nullptr, *returns = nullptr, *values = nullptr;
  int64_t* ep_off = nullptr;
  double *gram = nullptr, *rhs = nullptr, *workspace = nullptr, *coeffs = nullptr;
  std::vector<void*> owned;
  template <class T>
  T* make(int64_t n) {
    void* p = malloc((size_t)(n > 0 ? n : 1) * sizeof(T));
    owned.push_back(p);
    return static_cast<T*>(p);
  }
  void alloc() {
    const int F = 2 * obs_dim + 4;
    obs = make<float>((S - 1) * ldo + obs_dim);  // the last row has no padding
    returns = make<float>(S);
    values = make<float>((S - 1) * ldv + 1);
    ep_off = make<int64_t>(n_eps + 1);
    gram = make<double>((int64_t)F * F);
    rhs = make<double>(F);
    coeffs = make<double>(F);
    const int64_t ws = ga_linear_gram_workspace_doubles(obs_dim, S);
    workspace = make<double>(ws > 0 ? ws : 1);
  }
  int gram_run() {
    return ga_linear_features_gram_f64(obs, ldo, obs_dim, ep_off, n_eps, S, returns, gram,
                                       rhs, workspace, (ga_stream_t)0x40);
  }
  int predict_run() {
    return ga_linear_features_predict_f32(obs, ldo, obs_dim, ep_off, n_eps, S, coeffs, values,
                                          ldv, (ga_stream_t)0x40);
  }
  ~Call() { for (void* p : owned) free(p); }
};

struct Want {
  int obs_dim;
  int64_t S;
  int F, T, NT, tpw, chunk_rows;
  unsigned lds;
  int64_t block_doubles, blocks, workspace;
};

static void check_gram(const Want& w, int64_t ldo) {
  reset();
  Call c;
  c.obs_dim = w.obs_dim; c.S = w.S; c.ldo = ldo; c.n_eps = w.S < 3 ? 1 : 3;
  CHECK(ga_linear_gram_workspace_doubles(w.obs_dim, w.S) == w.workspace);
  c.alloc();
  CHECK(c.gram_run() == 0);
  CHECK(g_gram.size() == 1 && g_reduce.size() == 1 && g_predict.empty());
  if (g_gram.size() != 1 || g_reduce.size() != 1) return;
  const LinGramParams& p = g_gram[0].p;
  CHECK(p.obs == c.obs && p.ldo == ldo && p.obs_dim == w.obs_dim && p.ep_off == c.ep_off);
  CHECK(p.n_eps == c.n_eps && p.S == w.S && p.returns == c.returns);
  CHECK(p.partials == c.workspace && p.block_doubles == w.block_doubles);
  CHECK(p.n_slabs == (w.S + 2047) / 2048);
  CHECK(p.F == w.F && p.T == w.T && p.NT == w.NT && p.tpw == w.tpw);
  CHECK(p.chunk_rows == w.chunk_rows);
  CHECK(g_gram[0].lds == w.lds && g_gram[0].blocks == (unsigned)w.blocks);
  CHECK(g_stream_seen == (hipStream_t)0x40);
  const LinReduceParams& r = g_reduce[0].p;
  CHECK(r.partials == c.workspace && r.n_blocks == (int)w.blocks);
  CHECK(r.block_doubles == w.block_doubles && r.F == w.F && r.T == w.T && r.NT == w.NT);
  CHECK(r.gram == c.gram && r.rhs == c.rhs);
  CHECK(g_reduce[0].blocks == (unsigned)((w.block_doubles + 255) / 256));
}

static void check_predict(int obs_dim, int64_t S, int64_t ldo, int64_t ldv, unsigned blocks) {
  reset();
  Call c;
  c.obs_dim = obs_dim; c.S = S; c.ldo = ldo; c.ldv = ldv; c.n_eps = 1;
  c.alloc();
  CHECK(c.predict_run() == 0);
  CHECK(g_predict.size() == 1 && g_gram.empty() && g_reduce.empty());
  if (g_predict.size() != 1) return;
  const LinPredictParams& p = g_predict[0].p;
  CHECK(p.obs == c.obs && p.ldo == ldo && p.obs_dim == obs_dim && p.ep_off == c.ep_off);
  CHECK(p.n_eps == 1 && p.S == S && p.coeffs == c.coeffs && p.values == c.values);
  CHECK(p.ldv == ldv && g_predict[0].blocks == blocks);
}

template <class F>
static void refused(const char* what, bool gram, F&& spoil) {
  reset();
  Call c;
  c.alloc();
  spoil(c);
  const int rc = gram ? c.gram_run() : c.predict_run();
  const bool ok = rc < 0 && !g_error.empty() && g_gram.empty() && g_reduce.empty() &&
                  g_predict.empty();
  if (!ok)
    fprintf(stderr, "%s not refused: %s (rc %d, '%s')\n", gram ? "gram" : "predict", what, rc,
            g_error.c_str());
  CHECK(ok);
}
// a refusal both entry points share
template <class F>
static void both_refused(const char* what, F&& spoil) {
  refused(what, true, spoil);
  refused(what, false, spoil);
}

int main() {
  CHECK(ga_linear_features_supported(0) == 0 && ga_linear_features_supported(1) == 1);
  CHECK(ga_linear_features_supported(128) == 1 && ga_linear_features_supported(129) == 0);
  CHECK(ga_linear_features_supported(-3) == 0);
  CHECK(ga_linear_gram_workspace_doubles(0, 10) == -1);
  CHECK(ga_linear_gram_workspace_doubles(129, 10) == -1);
  CHECK(ga_linear_gram_workspace_doubles(4, 0) == -1);
  CHECK(ga_linear_gram_workspace_doubles(4, 1ll << 31) == -1);

  //          obs      S    F   T   NT tpw rows  lds  block doubles blocks workspace
  check_gram({1, 1, 6, 1, 1, 1, 32, 18944, 272, 1, 272}, 1);
  check_gram({1, 2047, 6, 1, 1, 1, 32, 18944, 272, 1, 272}, 4);
  check_gram({1, 2048, 6, 1, 1, 1, 32, 18944, 272, 1, 272}, 4);
  check_gram({1, 2049, 6, 1, 1, 1, 32, 18944, 272, 2, 544}, 4);
  check_gram({17, 2049, 38, 3, 6, 1, 32, 35328, 1584, 2, 3168}, 20);
  check_gram({17, 1048576, 38, 3, 6, 1, 32, 35328, 1584, 512, 811008}, 20);
  check_gram({30, 100, 64, 4, 10, 2, 32, 43520, 2624, 1, 2624}, 32);
  check_gram({31, 100, 66, 5, 15, 2, 32, 51712, 3920, 1, 3920}, 32);
  check_gram({46, 100, 96, 6, 21, 3, 32, 59904, 5472, 1, 5472}, 48);
  check_gram({47, 100, 98, 7, 28, 4, 16, 38400, 7280, 1, 7280}, 48);
  check_gram({102, 100, 208, 13, 91, 12, 16, 62976, 23504, 1, 23504}, 104);
  check_gram({103, 100, 210, 14, 105, 14, 8, 37888, 27104, 1, 27104}, 104);
  check_gram({128, 262144, 260, 17, 153, 20, 8, 44032, 39440, 128, 5048320}, 128);
  // the grid's cap: 1024 slabs, and one row more (workgroup 0 takes slabs 0 and 1024)
  check_gram({1, 2097152, 6, 1, 1, 1, 32, 18944, 272, 1024, 278528}, 1);
  check_gram({1, 2097153, 6, 1, 1, 1, 32, 18944, 272, 1024, 278528}, 1);

  check_predict(17, 1, 20, 1, 1);
  check_predict(17, 256, 20, 1, 1);
  check_predict(17, 257, 20, 1, 2);
  check_predict(128, 1000, 128, 4, 4);
  check_predict(1, 1048576, 4, 1, 4096);

  both_refused("null obs", [](Call& c) { c.obs = nullptr; });
  both_refused("null ep_off", [](Call& c) { c.ep_off = nullptr; });
  both_refused("obs_dim 0", [](Call& c) { c.obs_dim = 0; });
  both_refused("obs_dim 129", [](Call& c) { c.obs_dim = 129; c.ldo = 132; });
  both_refused("ldo < obs_dim", [](Call& c) { c.ldo = 16; });
  both_refused("S = 0", [](Call& c) { c.S = 0; });
  both_refused("S = 2^31", [](Call& c) { c.S = 1ll << 31; });
  both_refused("n_eps = 0", [](Call& c) { c.n_eps = 0; });
  both_refused("n_eps > S", [](Call& c) { c.n_eps = c.S + 1; });
  refused("null returns", true, [](Call& c) { c.returns = nullptr; });
  refused("null gram", true, [](Call& c) { c.gram = nullptr; });
  refused("null rhs", true, [](Call& c) { c.rhs = nullptr; });
  refused("null workspace", true, [](Call& c) { c.workspace = nullptr; });
  refused("misaligned gram", true, [](Call& c) {
    c.gram = reinterpret_cast<double*>(reinterpret_cast<char*>(c.gram) + 4);
  });
  refused("misaligned rhs", true, [](Call& c) {
    c.rhs = reinterpret_cast<double*>(reinterpret_cast<char*>(c.rhs) + 4);
  });
  refused("misaligned workspace", true, [](Call& c) {
    c.workspace = reinterpret_cast<double*>(reinterpret_cast<char*>(c.workspace) + 4);
  });
  refused("null coeffs", false, [](Call& c) { c.coeffs = nullptr; });
  refused("null values", false, [](Call& c) { c.values = nullptr; });
  refused("misaligned coeffs", false, [](Call& c) {
    c.coeffs = reinterpret_cast<double*>(reinterpret_cast<char*>(c.coeffs) + 4);
  });
  refused("ldv = 0", false, [](Call& c) { c.ldv = 0; });
  reset();
  return finish("linear baseline ok");
}
