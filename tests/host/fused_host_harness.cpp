// Host-logic harness for the fused optimizer step's host side
// (garage_amd/csrc/fused_train_host.cpp), built with -fsanitize=address,undefined on the
// CPU (`make asan-fused-host`).  The launch seam of fused_params.h, the profiler entries
// and the HIP calls the file makes are replaced by fakes.  Every seam fake records the
// variant, the grid and its parameter structs, and touches exactly what its kernel would
// in buffers of exactly the documented size, so that a tile count, an offset or an extent
// that is off trips the sanitizer.  The checks are about the host's own work: which
// instantiation a launch runs (against a literal table), the grids, every refusal with
// its message and before any launch, the optimizer launch's virtual grid, the slab sum's
// 32-bit offsets, the weight-plane cache's state machine, the developer hooks' buffers.
// GARAGE_AMD_SPLIT_PARTS is read once per process: the program runs the variant table
// again in child processes for the masks 1, 2 and 8.
#include "../../garage_amd/csrc/fused_params.h"
#include "../../garage_amd/csrc/fused_train.h"
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/prof.h"
#include "harness.h"

static_assert(FT_ROWS == 64 && FT_W1_FLOATS == 5120 && FT_MAX_REGIONS == 16,
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
template <class T>
static T* plus4bytes(T* p) {
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 4);
}

// ---- what the fakes record ----------------------------------------------------------------
struct Launch {
  std::string what;
  FtVariant v;
  unsigned blocks;
  hipStream_t stream;
  bool timed;                 // got the pair of events ga_prof_events handed out
  FwdLossParams f[2];         // forward + loss, evaluation, forward + data gradient
  DgradWgrad0Params d[2];     // data gradient, forward + data gradient
  ReduceRegionsParams r;      // regions + Adam
  bool bwd_only;              // planes
};
static std::vector<Launch> g_launches;
static std::vector<int> g_prof_events, g_prof_counts;  // the kinds asked for
static char g_ev[2];
static std::vector<void*> g_memsets;                 // hipMemset's targets
static std::vector<size_t> g_sync_copies;            // hipMemcpy's sizes
static int g_syncs = 0;
static volatile float g_sink;

static Launch& record(const char* what, FtVariant v, unsigned blocks, hipEvent_t e0,
                      hipEvent_t e1, hipStream_t s) {
  Launch l = {};
  l.what = what; l.v = v; l.blocks = blocks; l.stream = s;
  l.timed = e0 == (hipEvent_t)&g_ev[0] && e1 == (hipEvent_t)&g_ev[1];
  g_launches.push_back(l);
  return g_launches.back();
}
static int launches_of(const char* what) {
  int n = 0;
  for (const Launch& l : g_launches) n += l.what == what;
  return n;
}
static void wr(float* p, int64_t n) { memset(p, 0, sizeof(float) * (size_t)n); }
static void rd(const void* p, int64_t bytes) {
  const char* c = static_cast<const char*>(p);
  char s = 0;
  for (int64_t i = 0; i < bytes; ++i) s ^= c[i];
  g_sink = s;
}

// ---- what the kernels touch ---------------------------------------------------------------
// forward + loss body on `tiles` tiles: lpart [tiles][2], hpart [tiles][8 width + 8], dZ
// rows < M, H1 (first layer in the kernel, training), the planes; EVAL: the outputs only
static void touch_fwd(const FwdLossParams& p, unsigned tiles, bool l1, bool eval,
                      bool split) {
  const int64_t M = p.g.M, N = p.g.N;
  CHECK((int64_t)tiles == ga_fused_tiles(M));
  if (split) rd(p.bplanes, 2 * 3 * p.bplane_stride);
  CHECK(split == (p.bplanes != nullptr));
  if (eval) {
    for (int64_t m = 0; m < M; ++m) wr(p.eval_out + m * p.eval_ldo, p.loss.A);
    return;
  }
  for (unsigned t = 0; t < tiles; ++t) {
    p.lpart[2 * t] = p.lpart[2 * t + 1] = 0.0;
    wr(p.hpart + t * (8 * N + 8), 8 * N + 8);
  }
  for (int64_t m = 0; m < M; ++m) {
    wr(p.dZ + m * p.lddz, N);
    if (l1) wr(p.l1_H + m * p.l1_ldh, p.g.K);
  }
}
// data-gradient body: wpart [tiles][width round4(in_w) + width]; every partial of every
// slab range read, partial 0 written
static void touch_dgrad(const DgradWgrad0Params& p, unsigned tiles, bool split) {
  CHECK((int64_t)tiles == ga_fused_tiles(p.g.M));
  const int64_t stride = (int64_t)p.g.N * round4(p.in_w) + p.g.N;
  for (unsigned t = 0; t < tiles; ++t) wr(p.wpart + t * stride, stride);
  if (split) rd(p.bplanes, 2 * 3 * p.bplane_stride);
  CHECK(split == (p.bplanes != nullptr));
  if (!p.sum.n_part) return;
  CHECK(p.sum.tiles == (int)tiles);
  for (int i = 0; i < 2; ++i)
    for (int k = 0; k < p.sum.n_part; ++k) {
      float* part = p.sum.base + p.sum.off[i] + k * p.sum.stride;
      rd(part, 16 * (int64_t)p.sum.nq[i]);
      if (k == 0) wr(part, 4 * (int64_t)p.sum.nq[i]);
    }
}

void ft_launch_fwd_loss(const FwdLossParams& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                        hipEvent_t e1, hipStream_t s) {
  record("fwd", v, blocks, e0, e1, s).f[0] = p;
  CHECK(v.width == p.g.N);
  touch_fwd(p, blocks, v.l1, false, v.split);
}
void ft_launch_fwd_loss_pair(const FwdLossPair& pp, FtVariant v, unsigned blocks,
                             hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
  Launch& l = record("fwd_pair", v, blocks, e0, e1, s);
  l.f[0] = pp.a; l.f[1] = pp.b;
  CHECK(blocks % 2 == 0 && v.width == 256 && v.l1 && !v.split);
  touch_fwd(pp.a, blocks / 2, true, false, false);
  touch_fwd(pp.b, blocks / 2, true, false, false);
}
void ft_launch_eval_forward(const FwdLossParams& p, FtVariant v, unsigned blocks,
                            hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
  record("eval", v, blocks, e0, e1, s).f[0] = p;
  CHECK(v.width == p.g.N && v.l1);
  touch_fwd(p, blocks, true, true, v.split);
}
void ft_launch_dgrad(const DgradWgrad0Params& p, FtVariant v, unsigned blocks, hipEvent_t e0,
                     hipEvent_t e1, hipStream_t s) {
  record("dgrad", v, blocks, e0, e1, s).d[0] = p;
  CHECK(v.width == p.g.N && !v.ksc);
  touch_dgrad(p, blocks, v.split);
}
void ft_launch_dgrad_pair(const DgradWgrad0Pair& pp, FtVariant v, unsigned blocks,
                          hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
  Launch& l = record("dgrad_pair", v, blocks, e0, e1, s);
  l.d[0] = pp.a; l.d[1] = pp.b;
  CHECK(blocks % 2 == 0 && v.width == 256 && !v.split && !v.ksc);
  touch_dgrad(pp.a, blocks / 2, false);
  touch_dgrad(pp.b, blocks / 2, false);
}
void ft_launch_fwd_dgrad(const FwdDgradParams& pp, FtVariant v, unsigned blocks,
                         hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
  Launch& l = record("fwd_dgrad", v, blocks, e0, e1, s);
  l.f[0] = pp.f; l.d[0] = pp.d;
  CHECK(v.width == pp.f.g.N && v.l1 && !v.split && !pp.d.sum.n_part);
  touch_fwd(pp.f, blocks, true, false, false);
  touch_dgrad(pp.d, blocks, false);
}
// Every partial of every region read (partial 0 only where pre-summed); [beg, beg + n) of
// the gradient, the parameters and both moments written; one more block per network
// reads its loss sums and steps slot 0; the planes rewritten where asked
void ft_launch_reduce_regions(const ReduceRegionsParams& p, unsigned blocks, hipStream_t s) {
  record("reduce", FtVariant{}, blocks, nullptr, nullptr, s).r = p;
  CHECK((int64_t)blocks == p.n_virtual + p.n_nets);
  for (int k = 0; k < p.n_regions; ++k) {
    const FtRegion& r = p.r[k];
    const FtNet& N = p.net[r.net];
    CHECK(r.n % 4 == 0 && r.net < p.n_nets);
    for (int part = 0; part < (r.pre ? 1 : r.n_part); ++part)
      rd(r.src + part * r.stride, 4 * r.n);
    wr(N.grads + r.beg, r.n);
    if (N.do_adam) { wr(N.a.p + r.beg, r.n); wr(N.a.m + r.beg, r.n); wr(N.a.v + r.beg, r.n); }
  }
  for (int i = 0; i < p.n_nets; ++i) {
    const FtNet& N = p.net[i];
    rd(N.lpart, 16 * (int64_t)N.n_lpart);
    N.grads[0] = 0.f;
    if (N.do_adam) N.a.p[0] = N.a.m[0] = N.a.v[0] = 0.f;
    if (N.loss_out) *N.loss_out = 1.f;
    if (N.pl_fwd) {
      const int64_t halves = 3 * (int64_t)N.pl_rows * N.pl_cols;
      memset(N.pl_fwd, 0, 2 * (size_t)halves);
      memset(N.pl_bwd, 0, 2 * (size_t)halves);
    }
  }
}
// (the product keeps its plane buffers for the life of the process, in a container that
// is destroyed at exit: they stay reachable from here, so that LeakSanitizer reports
// nothing but leaks)
static std::vector<void*>* g_plane_cache = new std::vector<void*>;
// three planes of round32(rows) round32(cols) halves per orientation
void ft_launch_split_planes(bool bwd_only, unsigned blocks, const float* W, int64_t ld,
                            int rows, int cols, uint32_t* fwd, uint32_t* bwd,
                            hipStream_t s) {
  record("planes", FtVariant{}, blocks, nullptr, nullptr, s).bwd_only = bwd_only;
  g_plane_cache->push_back(fwd);
  const int64_t pairs = (int64_t)((rows + 31) & ~31) * ((cols + 31) & ~31) / 2;
  const unsigned half = (unsigned)((pairs + 255) / 256);
  CHECK(blocks == half || (!bwd_only && blocks == 2 * half));
  rd(W, 4 * ((int64_t)(rows - 1) * ld + cols));
  if (!bwd_only) memset(fwd, 0, 4 * 3 * (size_t)pairs);
  if (bwd_only || blocks == 2 * half) memset(bwd, 0, 4 * 3 * (size_t)pairs);
  CHECK(bwd == fwd + 3 * pairs);  // the two orientations share one allocation
}
void ft_launch_mfma_burn(int mode, int iters, int blocks, float*, hipStream_t s) {
  record("burn", FtVariant{mode, iters, 0, 0}, (unsigned)blocks, nullptr, nullptr, s);
}

void ga_prof_events(int kind, double work, hipEvent_t* e0, hipEvent_t* e1) {
  CHECK(work > 0.0);
  g_prof_events.push_back(kind);
  *e0 = (hipEvent_t)&g_ev[0];
  *e1 = (hipEvent_t)&g_ev[1];
}
void ga_prof_count(int kind) { g_prof_counts.push_back(kind); }

extern "C" {
hipError_t hipMemset(void* p, int v, size_t bytes) {
  g_memsets.push_back(p);
  memset(p, v, bytes);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  g_sync_copies.push_back(bytes);
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { ++g_syncs; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "fake"; }
}

static void reset() {
  g_launches.clear(); g_prof_events.clear(); g_prof_counts.clear(); g_error.clear();
}
static hipStream_t const S1 = (hipStream_t)0x100, S2 = (hipStream_t)0x200;

// ---- one network's step over exactly-sized buffers -------------------------------------------
// Two hidden layers of K and `width` units, in_w inputs (0: the first layer is not in
// the kernel and the forward launch reads A [M][K]), a head of A outputs.  Inputs no
// fake reads are one quad long.
struct Step {
  int64_t M; int width, K, in_w, A;
  ga_fused_loss_args loss;
  ga_fused_first_layer fl;
  ga_fused_fwd_net fwd;
  ga_fused_dgrad_net dg;
  int dg_in_w;
  Step(int64_t M_, int width_, int K_, int in_w_, int A_ = 2, const float* W = nullptr)
      : M(M_), width(width_), K(K_), in_w(in_w_), A(A_) {
    const int64_t rows = M >= 1 && M < (1 << 20) ? M : 1, tiles = ga_fused_tiles(rows);
    dg_in_w = in_w ? in_w : 4;
    memset(&loss, 0, sizeof(loss)); memset(&fl, 0, sizeof(fl));
    memset(&fwd, 0, sizeof(fwd)); memset(&dg, 0, sizeof(dg));
    loss.kind = 0; loss.actions = dev<float>(4); loss.lda = (A + 3) & ~3;
    loss.old_ll = dev<float>(4); loss.adv = dev<float>(4); loss.returns = dev<float>(4);
    loss.log_std = dev<float>(4); loss.A = A; loss.algo = 0; loss.clip = 0.2f;
    fl.X = dev<float>(4); fl.ldx = (dg_in_w + 3) & ~3; fl.W = dev<float>(4);
    fl.b = dev<float>(4); fl.in_w = in_w; fl.ldh = K;
    fl.H = dev<float>((rows - 1) * fl.ldh + K);
    fwd.A = in_w ? nullptr : dev<float>(4); fwd.lda = K;
    fwd.W = W ? W : dev<float>((int64_t)width * K); fwd.ldw = K;
    fwd.bias = dev<float>(4);
    fwd.head_W = dev<float>(4); fwd.head_ldw = width; fwd.head_bias = dev<float>(4);
    fwd.loss = &loss; fwd.lddz = width;
    fwd.dZ = dev<float>((rows - 1) * fwd.lddz + width);
    fwd.hpart = dev<float>(tiles * (8 * width + 8));
    fwd.lpart = dev<double>(tiles * 2);
    fwd.first = in_w ? &fl : nullptr;
    // the data gradient of the same step: into the K units of the first hidden layer
    dg.dZ2 = fwd.dZ; dg.lddz = fwd.lddz; dg.W2 = fwd.W; dg.ldw = fwd.ldw;
    dg.H1 = fl.H; dg.ldh = fl.ldh; dg.X = fl.X; dg.ldx = fl.ldx; dg.idx = nullptr;
    dg.wpart = dev<float>(tiles * ((int64_t)K * ((dg_in_w + 3) & ~3) + K));
  }
  int run_fwd(hipStream_t s = S1) { return ga_fused_fwd_head_loss(&fwd, 1, M, width, K, s); }
  int run_dgrad(hipStream_t s = S1) {
    return ga_fused_dgrad_wgrad0(&dg, 1, M, K, width, dg_in_w, s);
  }
  int run_fwd_dgrad(hipStream_t s = S1) {
    return ga_fused_fwd_dgrad(&fwd, &dg, M, width, K, s);
  }
};

// the whole MLP for its outputs: out [M][ldo], A valid columns
struct Eval {
  int64_t M; int dims[4]; int64_t ldx, ldo;
  const float *X, *W1, *b1, *W2, *b2, *Wh, *bh; float* out; const int* dims_p;
  Eval(int64_t M_, int in_w, int K, int width, int A = 3) : M(M_), dims{in_w, K, width, A} {
    const int64_t rows = M >= 1 && M < (1 << 20) ? M : 1;
    ldx = (in_w + 3) & ~3; ldo = 5;
    X = dev<float>(4); W1 = dev<float>(4); b1 = dev<float>(4);
    W2 = dev<float>((int64_t)width * ((K + 3) & ~3)); b2 = dev<float>(4);
    Wh = dev<float>(4); bh = dev<float>(4);
    out = dev<float>((rows - 1) * ldo + A);
    dims_p = dims;
  }
  int run(hipStream_t s = S1) {
    return ga_fused_eval_forward(X, ldx, nullptr, M, dims_p, W1, b1, W2, b2, Wh, bh, out, ldo,
                                 s);
  }
};

// an optimizer launch over exactly-sized buffers: region k has n[k] elements in parts[k]
// partials at the given stride (0: round4(n)); a pre-summed region owns partial 0 only
struct Reduce {
  std::vector<ga_fused_region> regions;
  ga_fused_loss_args loss;
  ga_reduce_net net;
  Reduce(std::vector<int64_t> n, std::vector<int> parts, uint32_t presummed = 0,
         int64_t first_beg = 4, float* params = nullptr) {
    int64_t beg = first_beg;
    for (size_t k = 0; k < n.size(); ++k) {
      const int64_t n4 = (n[k] + 3) & ~(int64_t)3;
      const bool pre = (presummed >> k) & 1u;
      ga_fused_region r = {beg, n[k], dev<float>(((pre ? 1 : parts[k]) - 1) * n4 + n4), n4,
                           parts[k]};
      regions.push_back(r);
      beg += n4;
    }
    memset(&loss, 0, sizeof(loss)); memset(&net, 0, sizeof(net));
    loss.kind = 2; loss.A = 2; loss.algo = 1;
    net.regions = regions.data(); net.n_regions = (int)regions.size();
    net.params = params ? params : dev<float>(beg);
    net.grads = dev<float>(beg); net.exp_avg = dev<float>(beg);
    net.exp_avg_sq = dev<float>(beg);
    net.step = 1; net.lr = 1e-3; net.beta1 = 0.9; net.beta2 = 0.999; net.eps = 1e-8;
    net.scale = 1.f; net.do_adam = 1; net.n_lpart = 3; net.lpart = dev<double>(2 * 3);
    net.M = 100; net.loss = &loss; net.presummed = presummed;
  }
  int run(hipStream_t s = S1) { return ga_reduce_regions_adam(&net, 1, s); }
};

// `rc` is a refusal with this message, and nothing was launched
static void refused(const char* what, int rc, const char* message) {
  const bool ok = rc == -1 && g_error == message && g_launches.empty();
  if (!ok)
    fprintf(stderr, "not refused as expected: %s (rc %d, '%s', %zu launches)\n", what, rc,
            g_error.c_str(), g_launches.size());
  CHECK(ok);
  reset();
}
static void switches(int pipelined, int split) {
  ga_set_pipelined_kloop(pipelined);
  ga_set_split_bf16(split);
}

// ---- which instantiation a launch runs --------------------------------------------------
// One row per (family, networks, width, inputs; 0 = the first layer is not in the kernel),
// one letter per switch setting: p the plain k-loop, k the pipelined one (KSC = 5), s the
// split-operand one, x refused.  Settings: ga_set_pipelined_kloop 0 then 1, under each
// ga_set_split_bf16 0, then 1 with GARAGE_AMD_SPLIT_PARTS unset (all), 1, 2, 8.
// K is the width, except 128 units where the kernel computes a first layer of 24 inputs
// for a 256-wide layer (24 x 256 floats do not fit).
struct VariantRow {
  const char* family; int n_nets, width, in_w; const char* want;
};
static const VariantRow VARIANTS[] = {
    {"fwd", 1, 64, 0, "ppppp" "ppppp"},    {"fwd", 1, 64, 4, "ppppp" "ppppp"},
    {"fwd", 1, 64, 17, "ppppp" "ppppp"},   {"fwd", 1, 64, 20, "ppppp" "ppppp"},
    {"fwd", 1, 64, 24, "ppppp" "ppppp"},   {"fwd", 1, 128, 0, "ppppp" "ppppp"},
    {"fwd", 1, 128, 4, "ppppp" "ppppp"},   {"fwd", 1, 128, 17, "ppppp" "ppppp"},
    {"fwd", 1, 128, 20, "ppppp" "ppppp"},  {"fwd", 1, 128, 24, "ppppp" "ppppp"},
    {"fwd", 1, 256, 0, "ppppp" "ppppp"},   {"fwd", 1, 256, 4, "psspp" "psspp"},
    {"fwd", 1, 256, 17, "psspp" "ksskk"},  {"fwd", 1, 256, 20, "psspp" "ksskk"},
    {"fwd", 1, 256, 24, "ppppp" "ppppp"},
    {"fwd", 2, 256, 4, "ppppp" "ppppp"},   {"fwd", 2, 256, 17, "ppppp" "kkkkk"},
    {"fwd", 2, 256, 20, "ppppp" "kkkkk"},  {"fwd", 2, 256, 24, "ppppp" "ppppp"},
    {"eval", 1, 64, 4, "ppppp" "ppppp"},   {"eval", 1, 64, 17, "ppppp" "ppppp"},
    {"eval", 1, 64, 20, "ppppp" "ppppp"},  {"eval", 1, 64, 24, "ppppp" "ppppp"},
    {"eval", 1, 128, 4, "ppppp" "ppppp"},  {"eval", 1, 128, 17, "ppppp" "ppppp"},
    {"eval", 1, 128, 20, "ppppp" "ppppp"}, {"eval", 1, 128, 24, "ppppp" "ppppp"},
    {"eval", 1, 256, 4, "pspps" "pspps"},  {"eval", 1, 256, 17, "pspps" "kskks"},
    {"eval", 1, 256, 20, "pspps" "kskks"}, {"eval", 1, 256, 24, "ppppp" "ppppp"},
    {"dgrad", 1, 64, 4, "ppppp" "ppppp"},  {"dgrad", 1, 64, 24, "ppppp" "ppppp"},
    {"dgrad", 1, 128, 4, "ppppp" "ppppp"}, {"dgrad", 1, 128, 20, "ppppp" "ppppp"},
    {"dgrad", 1, 256, 4, "pspsp" "pspsp"}, {"dgrad", 1, 256, 17, "pspsp" "pspsp"},
    {"dgrad", 1, 256, 20, "pspsp" "pspsp"}, {"dgrad", 1, 256, 24, "pspsp" "pspsp"},
    {"dgrad", 2, 256, 4, "ppppp" "ppppp"}, {"dgrad", 2, 256, 20, "ppppp" "ppppp"},
    {"fwd_dgrad", 1, 64, 4, "pxxxx" "pxxxx"},   {"fwd_dgrad", 1, 64, 20, "pxxxx" "pxxxx"},
    {"fwd_dgrad", 1, 64, 24, "pxxxx" "pxxxx"},  {"fwd_dgrad", 1, 128, 17, "pxxxx" "pxxxx"},
    {"fwd_dgrad", 1, 128, 24, "pxxxx" "pxxxx"}, {"fwd_dgrad", 1, 256, 4, "pxxxx" "pxxxx"},
    {"fwd_dgrad", 1, 256, 17, "pxxxx" "kxxxx"}, {"fwd_dgrad", 1, 256, 20, "pxxxx" "kxxxx"},
};

// the column of VARIANTS this process can reach with the split mode on
static int parts_column() {
  const char* e = getenv("GARAGE_AMD_SPLIT_PARTS");
  if (!e) return 1;
  return atoi(e) == 1 ? 2 : (atoi(e) == 2 ? 3 : 4);
}

static void check_variant(const VariantRow& row, int pipelined, int split) {
  reset();
  switches(pipelined, split);
  const char want = row.want[5 * pipelined + (split ? parts_column() : 0)];
  const std::string fam = row.family;
  const int K = row.in_w == 24 && row.width == 256 && fam != "dgrad" ? 128 : row.width;
  const int64_t M = 65;
  int rc;
  std::string what = fam;
  if (fam == "eval") {
    Eval e(M, row.in_w, K, row.width);
    rc = e.run();
  } else if (row.n_nets == 1) {
    Step st(M, row.width, K, row.in_w);
    rc = fam == "fwd" ? st.run_fwd() : (fam == "dgrad" ? st.run_dgrad() : st.run_fwd_dgrad());
  } else {
    Step a(M, row.width, K, row.in_w), b(M, row.width, K, row.in_w, 1);
    what += "_pair";
    if (fam == "fwd") {
      const ga_fused_fwd_net nets[2] = {a.fwd, b.fwd};
      rc = ga_fused_fwd_head_loss(nets, 2, M, row.width, K, S1);
    } else {
      const ga_fused_dgrad_net nets[2] = {a.dg, b.dg};
      rc = ga_fused_dgrad_wgrad0(nets, 2, M, K, row.width, a.dg_in_w, S1);
    }
  }
  bool ok;
  if (want == 'x') {
    ok = rc == -1 && g_launches.empty() &&
         g_error == "ga_fused_fwd_dgrad: unsupported shape or mode";
  } else {
    const int planes = launches_of("planes");
    ok = rc == 0 && (int)g_launches.size() == 1 + planes && planes == (want == 's');
    if (ok) {
      const Launch& l = g_launches.back();
      const int l1 = fam == "dgrad" ? 0 : (fam == "fwd" ? row.in_w != 0 : 1);
      ok = l.what == what && l.v.width == (fam == "dgrad" ? K : row.width) && l.v.l1 == l1 &&
           l.v.ksc == (want == 'k' ? 5 : 0) && l.v.split == (want == 's') && l.timed &&
           l.blocks == (unsigned)(2 * row.n_nets);
    }
  }
  if (!ok)
    fprintf(stderr, "variant: %s nets=%d width=%d in=%d pipelined=%d split=%d: want '%c'\n",
            row.family, row.n_nets, row.width, row.in_w, pipelined, split, want);
  CHECK(ok);
  free_all();
}

static void suite_variants() {
  for (const VariantRow& row : VARIANTS)
    for (int pipelined = 0; pipelined < 2; ++pipelined)
      for (int split = 0; split < 2; ++split) check_variant(row, pipelined, split);
  switches(1, 0);
}

// ---- grids, profiler slots, the first layer's bound --------------------------------------
static void suite_grids() {
  switches(1, 0);
  const int64_t Ms[3] = {1, 64, 65};
  const unsigned tiles[3] = {1, 1, 2};
  for (int i = 0; i < 3; ++i) {
    reset();
    Step st(Ms[i], 256, 256, 4), other(Ms[i], 256, 256, 4, 1);
    Eval ev(Ms[i], 4, 64, 128);
    CHECK(st.run_fwd() == 0 && st.run_dgrad() == 0 && st.run_fwd_dgrad() == 0);
    CHECK(ev.run() == 0);
    const ga_fused_fwd_net f2[2] = {st.fwd, other.fwd};
    const ga_fused_dgrad_net d2[2] = {st.dg, other.dg};
    CHECK(ga_fused_fwd_head_loss(f2, 2, Ms[i], 256, 256, S2) == 0);
    CHECK(ga_fused_dgrad_wgrad0(d2, 2, Ms[i], 256, 256, 4, S2) == 0);
    CHECK(g_launches.size() == 6);
    if (g_launches.size() == 6) {
      for (int k = 0; k < 4; ++k)
        CHECK(g_launches[k].blocks == tiles[i] && g_launches[k].stream == S1);
      for (int k = 4; k < 6; ++k)
        CHECK(g_launches[k].blocks == 2 * tiles[i] && g_launches[k].stream == S2);
      CHECK(g_launches[4].what == "fwd_pair" && g_launches[5].what == "dgrad_pair");
      // the descriptors reach the kernels' structs
      const FwdLossParams& f = g_launches[0].f[0];
      CHECK(f.g.M == Ms[i] && f.g.N == 256 && f.g.K == 256 && f.g.B == st.fwd.W);
      CHECK(f.dZ == st.fwd.dZ && f.hpart == st.fwd.hpart && f.lpart == st.fwd.lpart);
      CHECK(f.l1_H == st.fl.H && f.l1_in == 4 && f.loss.A == 2);
      CHECK(f.loss.invM == 1.f / (float)Ms[i]);
      const DgradWgrad0Params& d = g_launches[1].d[0];
      CHECK(d.g.A == st.fwd.dZ && d.g.B == st.fwd.W && d.H == st.fl.H && d.in_w == 4);
      CHECK(d.wpart == st.dg.wpart && d.sum.n_part == 0);
      CHECK(g_launches[4].f[1].hpart == other.fwd.hpart && g_launches[4].f[1].loss.A == 1);
      CHECK(g_launches[5].d[1].wpart == other.dg.wpart);
    }
    // one timed dispatch each; the pair launches and the fused forward + data gradient
    // count the second network step
    const std::vector<int> ev_want = {GA_PROF_FUSED_FWD, GA_PROF_FUSED_DGRAD,
                                      GA_PROF_FUSED_FWD, GA_PROF_EVAL_FWD,
                                      GA_PROF_FUSED_FWD, GA_PROF_FUSED_DGRAD};
    const std::vector<int> count_want = {GA_PROF_FUSED_DGRAD, GA_PROF_FUSED_FWD,
                                         GA_PROF_FUSED_DGRAD};
    CHECK(g_prof_events == ev_want && g_prof_counts == count_want);
    free_all();
  }
  // the first layer's weights: K x round4(in_w) floats within FT_W1_FLOATS
  struct { int K, in_w; bool ok; } bound[4] = {
      {256, 20, true}, {256, 21, false}, {64, 32, true}, {48, 4, false}};
  for (auto& b : bound) {
    reset();
    Step st(3, 256, b.K, b.in_w);
    const int rc = st.run_fwd();
    if (b.ok) {
      CHECK(rc == 0 && g_launches.size() == 1);
      reset();
    } else {
      refused("first layer bound", rc, "ga_fused_fwd_head_loss: unsupported first layer");
    }
    free_all();
  }
  CHECK(ga_fused_first_layer_ok(20, 256) && !ga_fused_first_layer_ok(21, 256));
  CHECK(ga_fused_tiles(1) == 1 && ga_fused_tiles(64) == 1 && ga_fused_tiles(65) == 2);
  CHECK(ga_fused_fwd_dgrad_supported(256, 256, 20) && !ga_fused_fwd_dgrad_supported(256, 128, 4));
  const int dims_ok[4] = {20, 256, 256, 8}, dims_bad[4] = {20, 256, 256, 9};
  CHECK(ga_fused_eval_supported(3, dims_ok) && !ga_fused_eval_supported(3, dims_bad));
  CHECK(!ga_fused_eval_supported(2, dims_ok) && !ga_fused_eval_supported(3, nullptr));
  reset();
  CHECK(ga_debug_mfma_burn(1, 7, 5, nullptr, S2) == 0 && g_launches.size() == 1 &&
        g_launches[0].blocks == 5 && g_launches[0].v.width == 1 && g_launches[0].v.l1 == 7);
  reset();
}

// ---- every refusal, before any launch ------------------------------------------------------
#define FWD_REFUSED(msg, M, width, K, in_w, spoil)                                   \
  do {                                                                               \
    reset();                                                                         \
    Step st(M, width, K, in_w);                                                      \
    spoil;                                                                           \
    refused(#spoil, st.run_fwd(), "ga_fused_fwd_head_loss: " msg);                   \
    free_all();                                                                      \
  } while (0)
#define DGRAD_REFUSED(msg, M, spoil)                                                 \
  do {                                                                               \
    reset();                                                                         \
    Step st(M, 128, 128, 4);                                                         \
    spoil;                                                                           \
    refused(#spoil, st.run_dgrad(), "ga_fused_dgrad_wgrad0: " msg);                  \
    free_all();                                                                      \
  } while (0)
#define FWD_DGRAD_REFUSED(msg, spoil)                                                \
  do {                                                                               \
    reset();                                                                         \
    Step st(65, 128, 128, 4);                                                        \
    spoil;                                                                           \
    refused(#spoil, st.run_fwd_dgrad(), msg);                                        \
    free_all();                                                                      \
  } while (0)
#define EVAL_REFUSED(msg, M, in_w, K, width, A, spoil)                               \
  do {                                                                               \
    reset();                                                                         \
    Eval e(M, in_w, K, width, A);                                                    \
    spoil;                                                                           \
    refused(#spoil, e.run(), "ga_fused_eval_forward: " msg);                         \
    free_all();                                                                      \
  } while (0)
#define REDUCE_REFUSED(msg, spoil)                                                   \
  do {                                                                               \
    reset();                                                                         \
    Reduce r({8, 100}, {2, 3});                                                      \
    spoil;                                                                           \
    refused(#spoil, r.run(), "ga_reduce_regions_adam: " msg);                        \
    free_all();                                                                      \
  } while (0)

// two slab ranges of 8 and 16 elements in 3 partials 32 floats apart, in one workspace
static float* with_slabs(Step& st) {
  float* slabs = dev<float>(2 * 32 + 24);
  st.dg.sum_w = ga_slab_range{slabs, 8, 32, 3};
  st.dg.sum_b = ga_slab_range{slabs + 8, 16, 32, 3};
  return slabs;
}

static void suite_refusals() {
  switches(1, 0);
  const int64_t big = 1ll << 31;
  // ---- fwd_build
  FWD_REFUSED("null pointer", 5, 128, 64, 0, st.fwd.A = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.W = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.bias = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.head_W = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.head_bias = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.loss = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.dZ = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.hpart = nullptr);
  FWD_REFUSED("null pointer", 5, 128, 64, 4, st.fwd.lpart = nullptr);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.X = nullptr);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.W = nullptr);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.b = nullptr);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.H = nullptr);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.in_w = 0);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.in_w = 33);
  FWD_REFUSED("unsupported first layer", 5, 128, 288, 4, (void)0);  // more than 256 units
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 5, st.fl.ldx = 4);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.ldh = 66);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.ldh = 60);
  FWD_REFUSED("unsupported first layer", 5, 128, 64, 4, st.fl.W = plus4bytes(st.fl.W));
  FWD_REFUSED("unsupported shape", 5, 96, 64, 4, (void)0);
  FWD_REFUSED("unsupported shape", 0, 128, 64, 4, (void)0);
  FWD_REFUSED("unsupported shape", big, 128, 64, 4, (void)0);
  FWD_REFUSED("unsupported shape", 5, 128, 0, 0, (void)0);
  FWD_REFUSED("unsupported shape", 5, 128, 64, 4, st.loss.A = 0);
  FWD_REFUSED("unsupported shape", 5, 128, 64, 4, st.loss.A = 9);
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 0, st.fwd.lda = 66);
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4, st.fwd.ldw = 66);
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4, st.fwd.head_ldw = 130);
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4, st.fwd.lddz = 130);
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 0,
              st.fwd.A = plus4bytes(st.fwd.A));
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4,
              st.fl.H = plus4bytes(st.fl.H));
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4,
              st.fwd.W = plus4bytes(st.fwd.W));
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4,
              st.fwd.bias = plus4bytes(st.fwd.bias));
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4,
              st.fwd.head_W = plus4bytes(st.fwd.head_W));
  FWD_REFUSED("operands must be 16-B aligned quads", 5, 128, 64, 4,
              st.fwd.dZ = plus4bytes(st.fwd.dZ));
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4,
              (st.loss.kind = 1, st.loss.returns = nullptr));
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4,
              st.loss.actions = nullptr);
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4, st.loss.adv = nullptr);
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4,
              st.loss.old_ll = nullptr);
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4, st.loss.lda = 6);
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4,
              (st.loss.A = 5, st.loss.lda = 4));
  FWD_REFUSED("missing / misaligned minibatch arrays", 5, 128, 64, 4,
              st.loss.actions = plus4bytes(st.loss.actions));
  FWD_REFUSED("log_std", 5, 128, 64, 4, st.loss.log_std = nullptr);
  FWD_REFUSED("algo", 5, 128, 64, 4, st.loss.algo = 2);
  {  // what the same checks let through: VPG without old_ll, a value loss, a categorical one
    reset();
    Step st(5, 128, 64, 4);
    st.loss.algo = 1; st.loss.old_ll = nullptr;
    CHECK(st.run_fwd() == 0);
    st.loss.kind = 1; st.loss.actions = nullptr; st.loss.adv = nullptr; st.loss.A = 1;
    CHECK(st.run_fwd() == 0);
    st.loss.kind = 2; st.loss.actions = plus4bytes(dev<float>(4)); st.loss.adv = dev<float>(4);
    st.loss.lda = 1; st.loss.log_std = nullptr; st.loss.A = 3;
    CHECK(st.run_fwd() == 0 && g_launches.size() == 3);
    free_all();
  }
  // ---- ga_fused_fwd_head_loss
  reset();
  refused("nets = null", ga_fused_fwd_head_loss(nullptr, 1, 5, 128, 64, S1),
          "ga_fused_fwd_head_loss: one or two networks");
  {
    Step a(5, 256, 256, 4), b(5, 256, 256, 4), c(5, 256, 256, 8), d(5, 256, 256, 0);
    ga_fused_fwd_net nets[2] = {a.fwd, b.fwd};
    refused("three networks", ga_fused_fwd_head_loss(nets, 3, 5, 256, 256, S1),
            "ga_fused_fwd_head_loss: one or two networks");
    refused("no networks", ga_fused_fwd_head_loss(nets, 0, 5, 256, 256, S1),
            "ga_fused_fwd_head_loss: one or two networks");
    const char* pair_msg = "ga_fused_fwd_head_loss_pair: unsupported shapes";
    nets[1] = c.fwd;
    refused("pair: input widths", ga_fused_fwd_head_loss(nets, 2, 5, 256, 256, S1), pair_msg);
    nets[1] = d.fwd;
    refused("pair: second first", ga_fused_fwd_head_loss(nets, 2, 5, 256, 256, S1), pair_msg);
    nets[1] = a.fwd; nets[0] = d.fwd;
    refused("pair: first first", ga_fused_fwd_head_loss(nets, 2, 5, 256, 256, S1), pair_msg);
    Step e(5, 128, 128, 4), f(5, 128, 128, 4);
    ga_fused_fwd_net narrow[2] = {e.fwd, f.fwd};
    refused("pair: width 128", ga_fused_fwd_head_loss(narrow, 2, 5, 128, 128, S1), pair_msg);
    // the second network's descriptor is checked like the first one's
    nets[0] = a.fwd; nets[1] = b.fwd; nets[1].hpart = nullptr;
    refused("pair: null in the second", ga_fused_fwd_head_loss(nets, 2, 5, 256, 256, S1),
            "ga_fused_fwd_head_loss: null pointer");
    free_all();
  }
  // ---- ga_fused_eval_forward
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.X = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.dims_p = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.W1 = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.b1 = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.W2 = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.b2 = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.Wh = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.bh = nullptr);
  EVAL_REFUSED("null pointer", 5, 4, 64, 128, 3, e.out = nullptr);
  EVAL_REFUSED("unsupported shape", 5, 33, 64, 128, 3, (void)0);
  EVAL_REFUSED("unsupported shape", 5, 21, 256, 128, 3, (void)0);
  EVAL_REFUSED("unsupported shape", 5, 4, 288, 128, 3, (void)0);
  EVAL_REFUSED("unsupported shape", 5, 4, 64, 96, 3, (void)0);
  EVAL_REFUSED("unsupported shape", 5, 4, 64, 128, 0, (void)0);
  EVAL_REFUSED("unsupported shape", 5, 4, 64, 128, 9, (void)0);
  EVAL_REFUSED("bad sizes", 0, 4, 64, 128, 3, (void)0);
  EVAL_REFUSED("bad sizes", big, 4, 64, 128, 3, (void)0);
  EVAL_REFUSED("bad sizes", 5, 4, 64, 128, 3, e.ldx = 3);
  EVAL_REFUSED("bad sizes", 5, 4, 64, 128, 3, e.ldo = 2);
  EVAL_REFUSED("operands must be 16-B aligned", 5, 4, 64, 128, 3, e.W1 = plus4bytes(e.W1));
  EVAL_REFUSED("operands must be 16-B aligned", 5, 4, 64, 128, 3, e.W2 = plus4bytes(e.W2));
  EVAL_REFUSED("operands must be 16-B aligned", 5, 4, 64, 128, 3, e.b2 = plus4bytes(e.b2));
  EVAL_REFUSED("operands must be 16-B aligned", 5, 4, 64, 128, 3, e.Wh = plus4bytes(e.Wh));
  // ---- dgrad_build
  DGRAD_REFUSED("null pointer", 5, st.dg.dZ2 = nullptr);
  DGRAD_REFUSED("null pointer", 5, st.dg.W2 = nullptr);
  DGRAD_REFUSED("null pointer", 5, st.dg.H1 = nullptr);
  DGRAD_REFUSED("null pointer", 5, st.dg.X = nullptr);
  DGRAD_REFUSED("null pointer", 5, st.dg.wpart = nullptr);
  DGRAD_REFUSED("unsupported shape", 5, st.K = 96);
  DGRAD_REFUSED("unsupported shape", 0, (void)0);
  DGRAD_REFUSED("unsupported shape", big, (void)0);
  DGRAD_REFUSED("unsupported shape", 5, st.width = 0);
  DGRAD_REFUSED("unsupported shape", 5, st.dg_in_w = 0);
  DGRAD_REFUSED("unsupported shape", 5, (st.dg_in_w = 33, st.dg.ldx = 36));
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.lddz = 130);
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.ldw = 130);
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.ldh = 130);
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.ldx = 6);
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg_in_w = 5);  // ldx = 4 < 8
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.dZ2 = plus4bytes(st.dg.dZ2));
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.W2 = plus4bytes(st.dg.W2));
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.H1 = plus4bytes(st.dg.H1));
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5, st.dg.X = plus4bytes(st.dg.X));
  DGRAD_REFUSED("operands must be 16-B aligned quads", 5,
                st.dg.wpart = plus4bytes(st.dg.wpart));
#define SLABS with_slabs(st)
  DGRAD_REFUSED("bad slab range 0", 5, (SLABS, st.dg.sum_w.n = 6));
  DGRAD_REFUSED("bad slab range 0", 5, (SLABS, st.dg.sum_w.n = 0));
  DGRAD_REFUSED("bad slab range 1", 5, (SLABS, st.dg.sum_b.n = 18));
  DGRAD_REFUSED("bad slab range 0", 5, (SLABS, st.dg.sum_w.n_part = st.dg.sum_b.n_part = 0));
  DGRAD_REFUSED("bad slab range 1", 5, (SLABS, st.dg.sum_w.stride = st.dg.sum_b.stride = 12));
  DGRAD_REFUSED("bad slab range 0", 5, (SLABS, st.dg.sum_w.stride = st.dg.sum_b.stride = 34));
  DGRAD_REFUSED("bad slab range 0", 5, st.dg.sum_w.src = plus4bytes(SLABS));
  DGRAD_REFUSED("bad slab range 1", 5, (SLABS, st.dg.sum_b.stride = 36));  // unequal strides
  DGRAD_REFUSED("bad slab range 1", 5, (SLABS, st.dg.sum_b.n_part = 2));   // unequal n_part
  // (fabricated addresses: a refusal never dereferences them)
  DGRAD_REFUSED("slab ranges further apart than 2^30 floats", 5,
                (st.dg.sum_w = ga_slab_range{(float*)0x10000000000ull, 8, 32, 3},
                 st.dg.sum_b = ga_slab_range{(float*)0x10100000000ull, 16, 32, 3}));
  DGRAD_REFUSED("slab ranges further apart than 2^30 floats", 5,
                (st.dg.sum_b = ga_slab_range{(float*)0x10000000000ull, 8, 32, 3},
                 // (the upper range's 288 bytes end one quad too far)
                 st.dg.sum_w = ga_slab_range{(float*)(0x10100000000ull - 288 + 16), 8, 32, 3}));
  // ---- ga_fused_dgrad_wgrad0
  reset();
  refused("nets = null", ga_fused_dgrad_wgrad0(nullptr, 1, 5, 128, 128, 4, S1),
          "ga_fused_dgrad_wgrad0: one or two networks");
  {
    Step a(5, 128, 128, 4), b(5, 128, 128, 4);
    const ga_fused_dgrad_net nets[2] = {a.dg, b.dg};
    refused("three networks", ga_fused_dgrad_wgrad0(nets, 3, 5, 128, 128, 4, S1),
            "ga_fused_dgrad_wgrad0: one or two networks");
    refused("pair: width 128", ga_fused_dgrad_wgrad0(nets, 2, 5, 128, 128, 4, S1),
            "ga_fused_dgrad_wgrad0_pair: unsupported width");
    free_all();
  }
  // ---- ga_fused_fwd_dgrad
  reset();
  {
    Step st(65, 128, 128, 4);
    refused("fwd = null", ga_fused_fwd_dgrad(nullptr, &st.dg, 65, 128, 128, S1),
            "ga_fused_fwd_dgrad: null pointer");
    refused("dgrad = null", ga_fused_fwd_dgrad(&st.fwd, nullptr, 65, 128, 128, S1),
            "ga_fused_fwd_dgrad: null pointer");
    free_all();
  }
  FWD_DGRAD_REFUSED("ga_fused_fwd_dgrad: null pointer", st.fwd.first = nullptr);
  FWD_DGRAD_REFUSED("ga_fused_fwd_dgrad: null pointer", st.fwd.loss = nullptr);
  FWD_DGRAD_REFUSED("ga_fused_fwd_dgrad: unsupported shape or mode", st.K = 64);
  FWD_DGRAD_REFUSED("ga_fused_fwd_dgrad: unsupported shape or mode", st.fl.in_w = 33);
  const char* one_step = "ga_fused_fwd_dgrad: the two descriptors are not one step's";
  FWD_DGRAD_REFUSED(one_step, st.dg.dZ2 = dev<float>(4));
  FWD_DGRAD_REFUSED(one_step, st.dg.lddz += 4);
  FWD_DGRAD_REFUSED(one_step, st.dg.H1 = dev<float>(4));
  FWD_DGRAD_REFUSED(one_step, st.dg.ldh += 4);
  FWD_DGRAD_REFUSED(one_step, st.dg.X = dev<float>(4));
  FWD_DGRAD_REFUSED(one_step, st.dg.ldx += 4);
  FWD_DGRAD_REFUSED(one_step, st.dg.idx = dev<int32_t>(4));
  FWD_DGRAD_REFUSED(one_step, st.loss.idx = dev<int32_t>(4));
  FWD_DGRAD_REFUSED(one_step, (st.dg.sum_w = ga_slab_range{dev<float>(8), 8, 8, 1}));
  FWD_DGRAD_REFUSED(one_step, (st.dg.sum_b = ga_slab_range{dev<float>(8), 8, 8, 1}));
  // (both builders run behind them)
  FWD_DGRAD_REFUSED("ga_fused_fwd_head_loss: null pointer", st.fwd.hpart = nullptr);
  FWD_DGRAD_REFUSED("ga_fused_dgrad_wgrad0: null pointer", st.dg.wpart = nullptr);
  // ---- reduce_add_net, ga_reduce_regions_adam
  REDUCE_REFUSED("null pointer", r.net.regions = nullptr);
  REDUCE_REFUSED("null pointer", r.net.params = nullptr);
  REDUCE_REFUSED("null pointer", r.net.grads = nullptr);
  REDUCE_REFUSED("null pointer", r.net.exp_avg = nullptr);
  REDUCE_REFUSED("null pointer", r.net.exp_avg_sq = nullptr);
  REDUCE_REFUSED("null pointer", r.net.lpart = nullptr);
  REDUCE_REFUSED("null pointer", r.net.loss = nullptr);
  REDUCE_REFUSED("bad arguments", r.net.n_regions = 0);
  REDUCE_REFUSED("bad arguments", r.net.n_regions = FT_MAX_REGIONS + 1);
  REDUCE_REFUSED("bad arguments", r.net.step = 0);
  REDUCE_REFUSED("bad arguments", r.net.n_lpart = 0);
  REDUCE_REFUSED("bad arguments", r.net.presummed = 4);  // a bit beyond two regions
  REDUCE_REFUSED("bad region 0", r.regions[0].src = nullptr);
  REDUCE_REFUSED("bad region 1", r.regions[1].n = 0);
  REDUCE_REFUSED("bad region 1", r.regions[1].n_part = 0);
  REDUCE_REFUSED("bad region 0", r.regions[0].beg = 0);
  REDUCE_REFUSED("bad region 0", r.regions[0].beg = 6);
  REDUCE_REFUSED("bad region 1", r.regions[1].stride = 102);
  REDUCE_REFUSED("bad region 1", r.regions[1].src = plus4bytes(r.regions[1].src));
  reset();
  refused("nets = null", ga_reduce_regions_adam(nullptr, 1, S1),
          "ga_reduce_regions_adam: one or two networks");
  {
    Reduce a({8, 100}, {2, 3}), b({8}, {2});
    ga_reduce_net nets[2] = {a.net, b.net};
    refused("three networks", ga_reduce_regions_adam(nets, 3, S1),
            "ga_reduce_regions_adam: one or two networks");
    nets[1].pl_rows = 32; nets[1].pl_cols = 32;
    refused("two networks with pl_rows", ga_reduce_regions_adam(nets, 2, S1),
            "ga_reduce_regions_adam: no plane rewriting for two networks");
    // 16 regions fit, over both networks; 17 do not
    Reduce c(std::vector<int64_t>(9, 8), std::vector<int>(9, 1)),
        d(std::vector<int64_t>(7, 8), std::vector<int>(7, 1)),
        e(std::vector<int64_t>(8, 8), std::vector<int>(8, 1));
    ga_reduce_net full[2] = {c.net, d.net}, over[2] = {c.net, e.net};
    CHECK(ga_reduce_regions_adam(full, 2, S1) == 0 && g_launches.size() == 1 &&
          g_launches[0].r.n_regions == 16 && g_launches[0].blocks == 16 + 2);
    reset();
    refused("17 regions", ga_reduce_regions_adam(over, 2, S1),
            "ga_reduce_regions_adam: bad arguments");
    free_all();
  }
}

// ---- the optimizer launch's virtual grid, the slab sum's offsets ---------------------------
static void suite_layout() {
  switches(1, 0);
  reset();
  {
    // 1 element in 4 partials, 1000 in 128, 1000 in 129, 5000 pre-summed (of 3)
    Reduce r({1, 1000, 1000, 5000}, {4, 128, 129, 3}, 8u);
    CHECK(r.run(S2) == 0 && g_launches.size() == 1);
    const ReduceRegionsParams& p = g_launches[0].r;
    const int quads[4] = {64, 64, 16, 256};
    const int64_t vbeg[4] = {0, 1, 5, 21};       // + 1, + ceil(250 / 64), + ceil(250 / 16)
    const int64_t beg[4] = {4, 8, 1008, 2008}, n[4] = {4, 1000, 1000, 5000};
    CHECK(p.n_regions == 4 && p.n_nets == 1 && p.n_virtual == 26);  // + ceil(1250 / 256)
    CHECK(g_launches[0].blocks == 27 && g_launches[0].stream == S2);
    for (int k = 0; k < 4; ++k) {
      CHECK(p.r[k].quads == quads[k] && p.r[k].vbeg == vbeg[k] && p.r[k].beg == beg[k]);
      CHECK(p.r[k].n == n[k] && p.r[k].pre == (k == 3) && p.r[k].net == 0);
      CHECK(p.r[k].src == r.regions[k].src && p.r[k].stride == r.regions[k].stride);
      CHECK(p.r[k].n_part == r.regions[k].n_part);
    }
    const FtNet& N = p.net[0];
    CHECK(N.a.p == r.net.params && N.a.m == r.net.exp_avg && N.a.v == r.net.exp_avg_sq);
    CHECK(N.grads == r.net.grads && N.do_adam == 1 && N.n_lpart == 3 && N.M == 100);
    CHECK(N.pl_fwd == nullptr && N.pl_bwd == nullptr);
    const GaAdam want = ga_adam_coeffs(1e-3, 0.9, 0.999, 1e-8, 1);
    CHECK(memcmp(&N.a.c, &want, sizeof(want)) == 0);
    free_all();
  }
  reset();
  {  // two networks: the second one's regions follow, in its own buffers
    Reduce a({1000}, {200}), b({1}, {1});
    const ga_reduce_net nets[2] = {a.net, b.net};
    CHECK(ga_reduce_regions_adam(nets, 2, S1) == 0 && g_launches.size() == 1);
    const ReduceRegionsParams& p = g_launches[0].r;
    CHECK(p.n_regions == 2 && p.n_virtual == 17 && g_launches[0].blocks == 19);
    CHECK(p.r[0].quads == 16 && p.r[0].vbeg == 0 && p.r[0].net == 0);
    CHECK(p.r[1].quads == 64 && p.r[1].vbeg == 16 && p.r[1].net == 1 && p.r[1].n == 4);
    CHECK(p.net[1].grads == b.net.grads);
    free_all();
  }
  reset();
  {  // slab ranges: 256 and 16 elements in 3 partials 1024 floats apart, sum_b the lower
    Step st(65, 128, 128, 4);
    float* slabs = dev<float>(64 + 2 * 1024 + 256);
    st.dg.sum_w = ga_slab_range{slabs + 64, 256, 1024, 3};
    st.dg.sum_b = ga_slab_range{slabs + 16, 16, 1024, 3};
    CHECK(st.run_dgrad() == 0 && g_launches.size() == 1);
    const FtSlabSum& s = g_launches[0].d[0].sum;
    CHECK(s.base == slabs + 16 && s.off[0] == 48 && s.off[1] == 0);
    CHECK(s.nq[0] == 64 && s.nq[1] == 4 && s.stride == 1024 && s.n_part == 3 && s.tiles == 2);
    // one range alone, either one
    st.dg.sum_b = ga_slab_range{};
    CHECK(st.run_dgrad() == 0 && g_launches.size() == 2);
    const FtSlabSum& w = g_launches[1].d[0].sum;
    CHECK(w.base == slabs + 64 && w.off[0] == 0 && w.nq[0] == 64 && w.nq[1] == 0);
    st.dg.sum_w = ga_slab_range{};
    st.dg.sum_b = ga_slab_range{slabs + 16, 16, 1024, 3};
    CHECK(st.run_dgrad() == 0 && g_launches.size() == 3);
    const FtSlabSum& b = g_launches[2].d[0].sum;
    CHECK(b.base == slabs + 16 && b.off[1] == 0 && b.nq[0] == 0 && b.nq[1] == 4);
    free_all();
  }
  reset();
}

// ---- the weight-plane cache -------------------------------------------------------------------
static void suite_planes() {
  if (getenv("GARAGE_AMD_SPLIT_PARTS")) return;  // (every part of the split mode)
  switches(1, 1);
  ga_set_split_adam_planes(1);
  reset();
  // W [256][256] at flat index 8 of the parameters
  const int64_t pl_beg = 8, n_w = 256 * 256;
  float* params = dev<float>(pl_beg + n_w);
  const float* W = params + pl_beg;
  Step st(65, 256, 256, 4, 2, W);
  const unsigned half = 128;  // 256 x 256 / 2 pairs, 256 to a workgroup
  const size_t allocs = g_dev_allocs.size();
  // a step: the forward launch writes both orientations, the data gradient none
  CHECK(st.run_fwd(S1) == 0 && g_launches.size() == 2);
  CHECK(g_dev_allocs.size() == allocs + 1 && g_dev_allocs.back() == 6 * 256 * 256 * 2);
  CHECK(g_launches[0].what == "planes" && g_launches[0].blocks == 2 * half &&
        !g_launches[0].bwd_only && g_launches[0].stream == S1);
  const uint16_t* fwd_planes = g_launches[1].f[0].bplanes;
  CHECK(g_launches[1].f[0].bplane_stride == 256 * 256);
  CHECK(st.run_dgrad(S1) == 0 && g_launches.size() == 3 && g_launches[2].what == "dgrad");
  CHECK(g_launches[2].d[0].bplanes == fwd_planes + 3 * 256 * 256);
  CHECK(g_launches[2].d[0].bplane_stride == 256 * 256);
  // ... once: a second data-gradient launch recomputes
  CHECK(st.run_dgrad(S1) == 0 && g_launches.size() == 5 && g_launches[3].what == "planes" &&
        g_launches[3].bwd_only && g_launches[3].blocks == half);
  // the data gradient on another stream recomputes
  reset();
  CHECK(st.run_fwd(S1) == 0 && st.run_dgrad(S2) == 0 && g_launches.size() == 4);
  CHECK(g_launches[2].what == "planes" && g_launches[2].bwd_only &&
        g_launches[2].blocks == half && g_launches[2].stream == S2);
  CHECK(g_dev_allocs.size() == allocs + 1);  // the same buffer throughout
  // ga_weight_planes always recomputes, one orientation
  reset();
  CHECK(ga_weight_planes(W, 256, 256, 256, 0, S1) == fwd_planes);
  CHECK(ga_weight_planes(W, 256, 256, 256, 0, S1) == fwd_planes);
  CHECK(ga_weight_planes(W, 256, 256, 256, 1, S1) == fwd_planes + 3 * 256 * 256);
  CHECK(ga_weight_planes(W, 256, 256, 256, 1, S1) == fwd_planes + 3 * 256 * 256);
  CHECK(g_launches.size() == 4 && !g_launches[1].bwd_only && g_launches[3].bwd_only);
  for (const Launch& l : g_launches) CHECK(l.what == "planes" && l.blocks == half);
  // ... and leaves nothing for a data-gradient launch to reuse
  CHECK(st.run_fwd(S1) == 0 && ga_weight_planes(W, 256, 256, 256, 0, S1) == fwd_planes);
  reset();
  CHECK(st.run_dgrad(S1) == 0 && launches_of("planes") == 1);
  // ragged shapes are padded to multiples of 32: 6 x 64 x 32 halves, 1024 pairs
  reset();
  const float* ragged = dev<float>(33 * 8 - 3);
  CHECK(ga_weight_planes(ragged, 8, 33, 5, 0, S1) != nullptr);
  CHECK(g_dev_allocs.back() == 6 * 64 * 32 * 2 && g_launches[0].blocks == 4);
  // an optimizer launch with pl_rows rewrites both orientations: the next training
  // forward on that stream launches nothing
  Reduce opt({n_w}, {1}, 0, pl_beg, params);
  opt.net.pl_beg = pl_beg; opt.net.pl_rows = 256; opt.net.pl_cols = 256;
  auto optimizer_then_forward = [&](hipStream_t s_opt, hipStream_t s_fwd, bool between) {
    reset();
    CHECK(st.run_fwd(S1) == 0);
    reset();
    CHECK(opt.run(s_opt) == 0 && g_launches.size() == 1);
    const FtNet N = g_launches[0].r.net[0];
    if (between) ga_planes_epoch_begin();
    reset();
    CHECK(st.run_fwd(s_fwd) == 0);
    return std::make_pair(N, launches_of("planes"));
  };
  auto r = optimizer_then_forward(S1, S1, false);
  CHECK((const uint16_t*)r.first.pl_fwd == fwd_planes && r.first.pl_beg == pl_beg);
  CHECK((const uint16_t*)r.first.pl_bwd == fwd_planes + 3 * 256 * 256);
  CHECK(r.first.pl_rows == 256 && r.first.pl_cols == 256 && r.second == 0);
  CHECK(g_launches[0].f[0].bplanes == fwd_planes);
  // ... and the data gradient of THAT step still recomputes its orientation? No: the
  // forward marked it fresh, on its stream
  CHECK(st.run_dgrad(S1) == 0 && launches_of("planes") == 0);
  // on another stream the forward recomputes
  r = optimizer_then_forward(S1, S2, false);
  CHECK(r.first.pl_fwd != nullptr && r.second == 1);
  r = optimizer_then_forward(S2, S1, false);
  CHECK(r.first.pl_fwd != nullptr && r.second == 1);
  // after ga_planes_epoch_begin it recomputes
  r = optimizer_then_forward(S1, S1, true);
  CHECK(r.first.pl_fwd != nullptr && r.second == 1);
  // without Adam, with ragged planes or with the switch off nothing is rewritten
  opt.net.do_adam = 0;
  r = optimizer_then_forward(S1, S1, false);
  CHECK(r.first.pl_fwd == nullptr && r.first.pl_rows == 0 && r.second == 1);
  opt.net.do_adam = 1;
  ga_set_split_adam_planes(0);
  r = optimizer_then_forward(S1, S1, false);
  CHECK(r.first.pl_fwd == nullptr && r.second == 1);
  ga_set_split_adam_planes(1);
  r = optimizer_then_forward(S1, S1, false);
  CHECK(r.first.pl_fwd != nullptr && r.second == 0);
  // a matrix no forward launch has asked planes for: nothing to rewrite
  {
    float* other = dev<float>(pl_beg + n_w);
    Reduce fresh({n_w}, {1}, 0, pl_beg, other);
    fresh.net.pl_beg = pl_beg; fresh.net.pl_rows = 256; fresh.net.pl_cols = 256;
    reset();
    CHECK(fresh.run(S1) == 0 && g_launches[0].r.net[0].pl_fwd == nullptr);
  }
  // no memory: refused, nothing launched
  reset();
  g_hip_malloc_fails = true;
  {
    Step cold(65, 256, 256, 4);
    refused("forward planes", cold.run_fwd(),
            "ga_fused_fwd_head_loss: no memory for the weight planes");
    refused("data-gradient planes", cold.run_dgrad(),
            "ga_fused_dgrad_wgrad0: no memory for the weight planes");
    Eval e(65, 4, 256, 256);
    refused("evaluation planes", e.run(),
            "ga_fused_eval_forward: no memory for the weight planes");
    CHECK(ga_weight_planes(cold.fwd.W, 256, 256, 256, 0, S1) == nullptr);
    CHECK(g_launches.empty());
  }
  g_hip_malloc_fails = false;
  // the evaluation forward recomputes its orientation every time
  {
    reset();
    Eval e(65, 4, 256, 256);
    CHECK(e.run() == 0 && e.run() == 0 && g_launches.size() == 4);
    CHECK(g_launches[0].what == "planes" && g_launches[0].blocks == half &&
          !g_launches[0].bwd_only && g_launches[2].what == "planes");
    CHECK(g_launches[1].f[0].bplanes != nullptr && g_launches[1].f[0].bplane_stride == 65536);
  }
  switches(1, 0);
  reset();
  free_all();
}

// ---- the developer hooks' buffers ------------------------------------------------------------
// (last: once armed, the buffers stay for the life of the process)
static void suite_debug() {
  switches(1, 0);
  reset();
  long long out[3 * 8];
  const size_t bytes = (16 + 7 * 4096) * sizeof(long long);
  // not armed: the read-only hooks refuse, launches get no buffer
  CHECK(ga_fused_fwd_debug_loop(out, 2) == -1 && ga_fused_fwd_debug_skew(out, 2) == -1);
  CHECK(g_memsets.empty() && g_syncs == 0);
  {
    Step st(65, 64, 64, 4);
    CHECK(st.run_fwd() == 0 && st.run_dgrad() == 0 && st.run_fwd_dgrad() == 0);
    CHECK(g_launches.size() == 3 && !g_launches[0].f[0].dbg && !g_launches[1].d[0].dbg &&
          !g_launches[2].f[0].dbg && !g_launches[2].d[0].dbg);
    reset();
    free_all();
  }
  const size_t allocs = g_dev_allocs.size();
  CHECK(ga_fused_fwd_debug(out) == 1 && g_dev_allocs.size() == allocs + 1 &&
        g_dev_allocs.back() == bytes && g_memsets.size() == 1 && g_syncs == 0);
  long long* ft = static_cast<long long*>(g_memsets[0]);
  for (int i = 0; i < 16; ++i) ft[i] = 100 + i;
  CHECK(ga_fused_fwd_debug(out) == 0 && g_syncs == 1 && g_sync_copies.back() == 16 * 8 &&
        out[0] == 100 && out[15] == 115);
  ft[16 + 5] = 7;
  CHECK(ga_fused_fwd_debug_skew(out, 2) == 0 && g_sync_copies.back() == 6 * 8 && out[5] == 7);
  ft[16 + 3 * 4096 + 7] = 9;
  CHECK(ga_fused_fwd_debug_loop(out, 2) == 0 && g_sync_copies.back() == 8 * 8 && out[7] == 9);
  CHECK(ga_fused_fwd_debug_skew(out, 4096 + 1) == -1 && ga_fused_fwd_debug_loop(out, 0) == -1);
  CHECK(ga_fused_dgrad_debug(out, 1, 2) == 1 && g_dev_allocs.size() == allocs + 2 &&
        g_memsets.size() == 2);
  long long* dg = static_cast<long long*>(g_memsets[1]);
  dg[3] = 33; dg[16 + 4] = 44;
  CHECK(ga_fused_dgrad_debug(out, 0, 0) == 0 && g_sync_copies.back() == 16 * 8 && out[3] == 33);
  CHECK(ga_fused_dgrad_debug(out, 1, 2) == 0 && g_sync_copies.back() == 6 * 8 && out[4] == 44);
  CHECK(ga_fused_dgrad_debug(out, 1, 0) == -1 && ga_fused_dgrad_debug(out, 1, 4097) == -1);
  // which buffer a launch gets: single launches their family's, the fused forward + data
  // gradient both, pair launches and launches of more than 4096 tiles none
  {
    Step st(65, 256, 256, 4), other(65, 256, 256, 4);
    CHECK(st.run_fwd() == 0 && st.run_dgrad() == 0 && st.run_fwd_dgrad() == 0);
    const ga_fused_fwd_net f2[2] = {st.fwd, other.fwd};
    const ga_fused_dgrad_net d2[2] = {st.dg, other.dg};
    CHECK(ga_fused_fwd_head_loss(f2, 2, 65, 256, 256, S1) == 0);
    CHECK(ga_fused_dgrad_wgrad0(d2, 2, 65, 256, 256, 4, S1) == 0);
    Eval e(65, 4, 64, 64);
    CHECK(e.run() == 0 && g_launches.size() == 6);
    CHECK(g_launches[0].f[0].dbg == ft && g_launches[1].d[0].dbg == dg);
    CHECK(g_launches[2].f[0].dbg == ft && g_launches[2].d[0].dbg == dg);
    CHECK(!g_launches[3].f[0].dbg && !g_launches[3].f[1].dbg);
    CHECK(!g_launches[4].d[0].dbg && !g_launches[4].d[1].dbg && !g_launches[5].f[0].dbg);
    free_all();
  }
  {
    reset();
    const int64_t M = 4096 * 64, over = M + 1;
    Step at(M, 64, 64, 4), past(over, 64, 64, 4);
    CHECK(at.run_fwd() == 0 && past.run_fwd() == 0 && past.run_dgrad() == 0 &&
          past.run_fwd_dgrad() == 0 && g_launches.size() == 4);
    CHECK(g_launches[0].blocks == 4096 && g_launches[0].f[0].dbg == ft);
    CHECK(g_launches[1].blocks == 4097 && !g_launches[1].f[0].dbg && !g_launches[2].d[0].dbg);
    CHECK(!g_launches[3].f[0].dbg && !g_launches[3].d[0].dbg);
    free_all();
  }
  reset();
}

int main(int argc, char** argv) {
  const std::vector<Suite> suites = {
      {"variants", suite_variants, "fused host variants ok"},
      {"grids", suite_grids, "fused host grids ok"},
      {"refusals", suite_refusals, "fused host refusals ok"},
      {"layout", suite_layout, "fused host layout ok"},
      {"planes", suite_planes, "fused host planes ok"},
      {"debug", suite_debug, "fused host debug hooks ok"},
  };
  int rc = run_suites(suites, argc, argv);
  if (argc > 1 || getenv("GARAGE_AMD_SPLIT_PARTS")) return rc;
  // the variant table again under each mask of GARAGE_AMD_SPLIT_PARTS (read once per
  // process): fresh processes of this program
  for (const char* mask : {"1", "2", "8"}) {
    fflush(stdout);
    setenv("GARAGE_AMD_SPLIT_PARTS", mask, 1);
    const std::string cmd = std::string("'") + argv[0] + "' variants";
    if (system(cmd.c_str()) != 0) {
      fprintf(stderr, "variant table failed under GARAGE_AMD_SPLIT_PARTS=%s\n", mask);
      rc = 1;
    }
  }
  if (rc == 0) printf("fused host ok\n");
  return rc;
}
