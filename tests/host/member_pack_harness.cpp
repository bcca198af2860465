// Host-logic harness for a population's joint pack (garage_amd/csrc/member_pack_host.cpp),
// built with -fsanitize=address,undefined on the CPU (`make asan-member-pack`).  The three
// launches are replaced by recording fakes; "device" memory is exactly-sized host memory,
// and the gather's fake walks, per plane and path, the first and the last unit its kernel
// would touch on both sides, so that a row count, a unit count or a stride that is off
// trips the sanitizer.  The checks are about the host's own work: every refusal precedes
// the first launch, the plane table (path, units, rows), the grids' bounds, the
// launches of a pack.
#include "../../garage_amd/csrc/internal.h"
#include "../../garage_amd/csrc/member_pack.h"
#include "harness.h"

// ---- what the fakes record -----------------------------------------------------
static std::vector<GaPackIndexArgs> g_episodes, g_src;
static std::vector<int64_t> g_src_blocks, g_gather_blocks;
static std::vector<GaPackTable> g_tables;
static int64_t g_n_rows = 0, g_n_eps = 0;  // of the gather under test

extern "C" {
int ga_launch_member_episodes(const GaPackIndexArgs* a, hipStream_t) {
  g_episodes.push_back(*a);
  return 0;
}
int ga_launch_member_src(const GaPackIndexArgs* a, int64_t blocks_x, hipStream_t) {
  CHECK(g_episodes.size() == g_src.size() + 1);  // after the episodes, on the stream
  g_src.push_back(*a);
  g_src_blocks.push_back(blocks_x);
  return 0;
}

// touches byte `at` of a buffer (the sanitizer checks it lies inside)
static void touch(const void* p, int64_t at) {
  volatile char c = static_cast<const char*>(p)[at];
  (void)c;
}

int ga_launch_member_gather(const GaPackTable* t, int64_t blocks_x, hipStream_t) {
  g_tables.push_back(*t);
  g_gather_blocks.push_back(blocks_x);
  for (int i = 0; i < t->n_planes; ++i) {
    const GaPackPlaneDev& p = t->plane[i];
    CHECK(p.rows == (p.per_episode ? g_n_eps : g_n_rows));
    const int64_t es = p.elem_size, last = p.rows - 1;
    // the destination's extent: row 0 .. the last row's last element
    touch(p.dst, 0);
    touch(p.dst, (last * p.ld_dst + p.width) * es - 1);
    // a row of the source (cell 0): the harness' sources hold one row
    touch(p.src, 0);
    touch(p.src, (int64_t)p.width * es - 1);
    if (p.path == GA_PACK_QUADS) {
      CHECK(es == 4 && p.width % 4 == 0 && p.units == p.rows * (p.width / 4));
      CHECK(p.ld_src % 4 == 0 && p.ld_dst % 4 == 0);
      CHECK(((uintptr_t)p.src & 15) == 0 && ((uintptr_t)p.dst & 15) == 0);
    } else if (p.path == GA_PACK_SCALAR) {
      CHECK(p.width == 1 && p.ld_dst == 1 && p.units == (p.rows + 3) / 4);
      CHECK(((uintptr_t)p.dst & (4 * es - 1)) == 0);  // one store of four elements
    } else {
      CHECK(p.path == GA_PACK_ELEMS && p.units == p.rows * p.width);
    }
    // the index a unit reads
    if (p.per_episode) {
      touch(t->ep_env, 4 * p.rows - 1);
      touch(t->ep_end, 4 * p.rows - 1);
    } else {
      touch(t->src, 4 * p.rows - 1);
    }
    CHECK(blocks_x >= 1 && blocks_x <= 8192);
    CHECK(blocks_x * 256 >= p.units || blocks_x == 8192);
  }
  return 0;
}
}  // extern "C"

static void reset() {
  g_episodes.clear(); g_src.clear(); g_src_blocks.clear(); g_gather_blocks.clear();
  g_tables.clear(); g_error.clear();
}

// ---- the index ----------------------------------------------------------------------
struct IndexCall {
  int64_t n = 64, Tcap = 8, n_cols = 6, n_members = 2, max_eps = 5, max_samples = 40;
  std::vector<uint16_t> tail;
  std::vector<int32_t> progress, col_base, ep_env, ep_end, ep_len, src;
  std::vector<int64_t> ep_off, member_samples, member_off;
  const uint16_t* tail_p; int32_t* progress_p; int32_t* col_base_p; int32_t* ep_env_p;
  int32_t* ep_end_p; int32_t* ep_len_p; int64_t* ep_off_p; int64_t* samples_p;
  int64_t* off_p; int32_t* src_p;
  void alloc() {
    tail.resize(n * Tcap); progress.resize(3 * n_members);
    col_base.resize(n_members * Tcap); ep_env.resize(max_eps); ep_end.resize(max_eps);
    ep_len.resize(max_eps); src.resize(max_samples); ep_off.resize(max_eps + n_members);
    member_samples.resize(n_members); member_off.resize(n_members + 1);
    tail_p = tail.data(); progress_p = progress.data(); col_base_p = col_base.data();
    ep_env_p = ep_env.data(); ep_end_p = ep_end.data(); ep_len_p = ep_len.data();
    ep_off_p = ep_off.data(); samples_p = member_samples.data();
    off_p = member_off.data(); src_p = src.data();
  }
  int run() {
    return ga_member_pack_index(tail_p, n, Tcap, n_cols, n_members, progress_p,
                                col_base_p, max_eps, max_samples, ep_env_p, ep_end_p,
                                ep_len_p, ep_off_p, samples_p, off_p, src_p, nullptr);
  }
};

static void check_index(int64_t n, int64_t members, int64_t max_samples) {
  reset();
  IndexCall c;
  c.n = n; c.n_members = members; c.max_samples = max_samples;
  c.alloc();
  CHECK(c.run() == 0);
  CHECK(g_episodes.size() == 1 && g_src.size() == 1);
  const GaPackIndexArgs& a = g_src[0];
  CHECK(memcmp(&a, &g_episodes[0], sizeof(a)) == 0);
  CHECK(a.tail == c.tail_p && a.g == n / members && a.Tcap == c.Tcap);
  CHECK(a.n_cols == c.n_cols);
  CHECK(a.n_members == members && a.progress == c.progress_p && a.col_base == c.col_base_p);
  CHECK(a.max_eps == c.max_eps && a.max_samples == max_samples);
  CHECK(a.ep_env == c.ep_env_p && a.ep_end == c.ep_end_p && a.ep_len == c.ep_len_p);
  CHECK(a.ep_off == c.ep_off_p && a.member_samples == c.samples_p);
  CHECK(a.member_off == c.off_p && a.src == c.src_p);
  // a member's share of the rows, 256 to a workgroup, at most 4096 of them
  const int64_t share = (max_samples + members - 1) / members;
  const int64_t want = (share + 255) / 256;
  CHECK(g_src_blocks[0] == (want > 4096 ? 4096 : want) && g_src_blocks[0] >= 1);
}

template <class F>
static void index_refused(const char* what, F&& spoil) {
  reset();
  IndexCall c;
  c.alloc();
  spoil(c);
  const int rc = c.run();
  const bool refused = rc < 0 && !g_error.empty() && g_episodes.empty() && g_src.empty();
  if (!refused)
    fprintf(stderr, "index not refused: %s (rc %d, '%s')\n", what, rc, g_error.c_str());
  CHECK(refused);
}

// ---- the gather ----------------------------------------------------------------------
struct GatherCall {
  int64_t n_rows = 37, n_eps = 5, Tcap = 8;
  std::vector<ga_pack_plane> planes;
  std::vector<void*> owned;
  std::vector<int32_t> src, ep_env, ep_end;
  const int32_t* src_p; const int32_t* ep_env_p; const int32_t* ep_end_p;
  // a plane over exactly-sized buffers: one source row, `rows` destination rows
  void add(int elem, int width, int64_t ld, bool per_episode) {
    const int64_t rows = per_episode ? n_eps : n_rows;
    ga_pack_plane p;
    memset(&p, 0, sizeof(p));
    const size_t src_bytes = (size_t)width * elem;
    const size_t dst_bytes = (size_t)((rows - 1) * ld + width) * elem;
    void* s = aligned_alloc(16, (src_bytes + 15) / 16 * 16);
    void* d = aligned_alloc(16, (dst_bytes + 15) / 16 * 16);
    owned.push_back(s); owned.push_back(d);
    p.src = s; p.dst = d; p.ld_src = ld; p.ld_dst = ld; p.elem_size = elem;
    p.width = width; p.per_episode = per_episode;
    planes.push_back(p);
  }
  void index() {
    src.assign(n_rows, 0); ep_env.assign(n_eps > 0 ? n_eps : 1, 0);
    ep_end.assign(n_eps > 0 ? n_eps : 1, 0);
    src_p = src.data(); ep_env_p = ep_env.data(); ep_end_p = ep_end.data();
  }
  int run() {
    g_n_rows = n_rows; g_n_eps = n_eps;
    return ga_member_pack_gather(planes.data(), (int64_t)planes.size(), src_p, n_rows,
                                 ep_env_p, ep_end_p, n_eps, Tcap, nullptr);
  }
  ~GatherCall() { for (void* p : owned) free(p); }
};

// the planes of a batch: obs, actions, head, rewards, step types, lastobs, an env_info in
// sample rows and at the episodes' ends, plus shapes only the generic path takes
static void fill(GatherCall& g) {
  g.add(4, 4, 4, false);    // 0 obs: quads
  g.add(4, 12, 12, false);  // 1 three quads a row
  g.add(4, 8, 12, false);   // 2 a stride wider than the row
  g.add(4, 1, 1, false);    // 3 rewards: four rows a thread
  g.add(1, 1, 1, false);    // 4 step types
  g.add(4, 4, 4, true);     // 5 lastobs
  g.add(1, 1, 1, true);     // 6 an env_info at the episode's end
  g.add(4, 3, 3, false);    // 7 narrow 4-byte rows: by element
  g.add(1, 5, 8, false);    // 8 wide 1-byte rows: by element
  g.add(4, 1, 2, false);    // 9 width 1 with a stride: by element
}

static void check_gather(int64_t n_rows, int64_t n_eps) {
  reset();
  GatherCall g;
  g.n_rows = n_rows; g.n_eps = n_eps;
  fill(g);
  g.index();
  CHECK(g.run() == 0);
  CHECK(g_tables.size() == 1);
  const GaPackTable& t = g_tables[0];
  CHECK(t.n_planes == 10 && t.src == g.src_p && t.ep_env == g.ep_env_p);
  CHECK(t.ep_end == g.ep_end_p && t.Tcap == g.Tcap);
  const int want[10] = {GA_PACK_QUADS, GA_PACK_QUADS, GA_PACK_QUADS, GA_PACK_SCALAR,
                        GA_PACK_SCALAR, GA_PACK_QUADS, GA_PACK_SCALAR, GA_PACK_ELEMS,
                        GA_PACK_ELEMS, GA_PACK_ELEMS};
  int64_t most = 1;
  for (int i = 0; i < 10; ++i) {
    const GaPackPlaneDev& p = t.plane[i];
    CHECK(p.path == want[i]);
    CHECK(p.src == g.planes[i].src && p.dst == g.planes[i].dst);
    CHECK(p.ld_src == g.planes[i].ld_src && p.ld_dst == g.planes[i].ld_dst);
    CHECK(p.width == g.planes[i].width && p.elem_size == g.planes[i].elem_size);
    if (p.units > most) most = p.units;
  }
  const int64_t blocks = (most + 255) / 256;
  CHECK(g_gather_blocks[0] == (blocks > 8192 ? 8192 : blocks));
}

template <class F>
static void gather_refused(const char* what, F&& spoil) {
  reset();
  GatherCall g;
  fill(g);
  g.index();
  spoil(g);
  const int rc = g.run();
  const bool refused = rc < 0 && !g_error.empty() && g_tables.empty();
  if (!refused)
    fprintf(stderr, "gather not refused: %s (rc %d, '%s')\n", what, rc, g_error.c_str());
  CHECK(refused);
}

int main() {
  check_index(64, 2, 40);
  check_index(64, 1, 1);
  check_index(1024, 1024, 300000);
  check_index(64, 1, 5000000);  // the grid's cap
  index_refused("null tail", [](IndexCall& c) { c.tail_p = nullptr; });
  index_refused("null progress", [](IndexCall& c) { c.progress_p = nullptr; });
  index_refused("null col_base", [](IndexCall& c) { c.col_base_p = nullptr; });
  index_refused("null ep_env", [](IndexCall& c) { c.ep_env_p = nullptr; });
  index_refused("null ep_end", [](IndexCall& c) { c.ep_end_p = nullptr; });
  index_refused("null ep_len", [](IndexCall& c) { c.ep_len_p = nullptr; });
  index_refused("null ep_off", [](IndexCall& c) { c.ep_off_p = nullptr; });
  index_refused("null member_samples", [](IndexCall& c) { c.samples_p = nullptr; });
  index_refused("null member_off", [](IndexCall& c) { c.off_p = nullptr; });
  index_refused("null src", [](IndexCall& c) { c.src_p = nullptr; });
  index_refused("no members", [](IndexCall& c) { c.n_members = 0; });
  index_refused("1025 members", [](IndexCall& c) { c.n_members = 1025; c.n = 2050; });
  index_refused("3 members", [](IndexCall& c) { c.n_members = 3; });
  index_refused("n = 0", [](IndexCall& c) { c.n = 0; });
  index_refused("n_cols = 0", [](IndexCall& c) { c.n_cols = 0; });
  index_refused("n_cols > Tcap", [](IndexCall& c) { c.n_cols = c.Tcap + 1; });
  index_refused("2^31 cells", [](IndexCall& c) { c.n = 1 << 20; c.Tcap = 1 << 11; });
  index_refused("max_eps = 0", [](IndexCall& c) { c.max_eps = 0; });
  index_refused("max_samples = 0", [](IndexCall& c) { c.max_samples = 0; });
  index_refused("max_samples = 2^31", [](IndexCall& c) { c.max_samples = 1ll << 31; });

  check_gather(37, 5);
  check_gather(1, 1);
  check_gather(4, 3);
  check_gather(300000, 2000);
  {  // no episodes and no per-episode plane: fine
    reset();
    GatherCall g;
    g.n_eps = 0;
    g.add(4, 4, 4, false);
    g.add(1, 1, 1, false);
    g.index();
    g.ep_env_p = g.ep_end_p = nullptr;
    CHECK(g.run() == 0 && g_tables.size() == 1);
  }
  {  // a 1-byte destination that is not aligned to four: by element
    reset();
    GatherCall g;
    g.add(1, 1, 1, false);
    g.index();
    g.planes[0].dst = static_cast<char*>(g.planes[0].dst) + 1;
    g.n_rows -= 1;  // (the buffer holds one row fewer from there)
    g.index();
    CHECK(g.run() == 0 && g_tables.size() == 1 &&
          g_tables[0].plane[0].path == GA_PACK_ELEMS);
  }
  gather_refused("no planes", [](GatherCall& g) { g.planes.clear(); });
  gather_refused("null src", [](GatherCall& g) { g.src_p = nullptr; });
  gather_refused("null plane src", [](GatherCall& g) { g.planes[3].src = nullptr; });
  gather_refused("null plane dst", [](GatherCall& g) { g.planes[9].dst = nullptr; });
  gather_refused("null ep_env", [](GatherCall& g) { g.ep_env_p = nullptr; });
  gather_refused("null ep_end", [](GatherCall& g) { g.ep_end_p = nullptr; });
  gather_refused("n_eps = 0", [](GatherCall& g) { g.n_eps = 0; });
  gather_refused("n_eps < 0", [](GatherCall& g) { g.n_eps = -1; });
  gather_refused("17 planes", [](GatherCall& g) {
    while (g.planes.size() < 17) g.planes.push_back(g.planes[0]);
  });
  gather_refused("n_rows = 0", [](GatherCall& g) { g.n_rows = 0; });
  gather_refused("n_rows = 2^31", [](GatherCall& g) { g.n_rows = 1ll << 31; });
  gather_refused("Tcap = 0", [](GatherCall& g) { g.Tcap = 0; });
  gather_refused("elem 2", [](GatherCall& g) { g.planes[4].elem_size = 2; });
  gather_refused("elem 8", [](GatherCall& g) { g.planes[0].elem_size = 8; });
  gather_refused("width 0", [](GatherCall& g) { g.planes[7].width = 0; });
  gather_refused("ld_src < width", [](GatherCall& g) { g.planes[1].ld_src = 8; });
  gather_refused("ld_dst < width", [](GatherCall& g) { g.planes[1].ld_dst = 8; });
  gather_refused("width 6", [](GatherCall& g) { g.planes[2].width = 6; });
  gather_refused("ld_src 6", [](GatherCall& g) { g.planes[0].ld_src = 6; });
  gather_refused("ld_dst 5", [](GatherCall& g) { g.planes[0].ld_dst = 5; });
  gather_refused("misaligned src", [](GatherCall& g) {
    g.planes[0].src = static_cast<const char*>(g.planes[0].src) + 4;
  });
  gather_refused("misaligned dst", [](GatherCall& g) {
    g.planes[5].dst = static_cast<char*>(g.planes[5].dst) + 8;
  });
  reset();
  return finish("member pack ok");
}
