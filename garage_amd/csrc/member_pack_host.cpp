// A population's joint pack, host side: the argument checks of ga_member_pack_index /
// ga_member_pack_gather, the gather's plane table and the grids of the three launches
// (member_pack.hip).  Host C++ only: tests/host/member_pack_harness.cpp builds this
// file against fakes of the launches.
#include "member_pack.h"

extern "C" int ga_member_pack_index(const uint16_t* tail_buf, int64_t n, int64_t Tcap,
                                    int64_t n_cols, int64_t n_members,
                                    const int32_t* progress, const int32_t* col_base,
                                    int64_t max_eps, int64_t max_samples,
                                    int32_t* ep_env, int32_t* ep_end, int32_t* ep_len,
                                    int64_t* ep_off, int64_t* member_samples,
                                    int64_t* member_off, int32_t* src,
                                    ga_stream_t stream) {
  const char* who = "ga_member_pack_index";
  GA_REQUIRE(tail_buf && progress && col_base && ep_env && ep_end && ep_len && ep_off &&
                 member_samples && member_off && src,
             "%s: null pointer", who);
  // (the member offsets are one workgroup's scan, as ga_update_epoch_members' tables)
  GA_REQUIRE(n_members >= 1 && n_members <= 1024,
             "%s: n_members must be in 1..1024 (got %lld)", who, (long long)n_members);
  GA_REQUIRE(n > 0 && n % n_members == 0, "%s: %lld envs do not split into %lld members",
             who, (long long)n, (long long)n_members);
  GA_REQUIRE(n_cols >= 1 && n_cols <= Tcap,
             "%s: n_cols must be in 1..Tcap (got %lld, Tcap %lld)", who, (long long)n_cols,
             (long long)Tcap);
  GA_REQUIRE(n * Tcap < (1ll << 31),
             "%s: rollout buffers too large (%lld x %lld cells are addressed in int32)",
             who, (long long)n, (long long)Tcap);
  GA_REQUIRE(max_eps >= 1, "%s: max_eps must be at least 1 (got %lld)", who,
             (long long)max_eps);
  GA_REQUIRE(max_samples >= 1 && max_samples < (1ll << 31),
             "%s: max_samples must be in 1..2^31 - 1 (got %lld)", who,
             (long long)max_samples);
  GaPackIndexArgs a;
  a.tail = tail_buf; a.g = n / n_members; a.Tcap = Tcap; a.n_cols = (int32_t)n_cols;
  a.n_members = (int32_t)n_members;
  a.progress = progress; a.col_base = col_base; a.max_eps = max_eps;
  a.max_samples = max_samples; a.ep_env = ep_env; a.ep_end = ep_end; a.ep_len = ep_len;
  a.ep_off = ep_off; a.member_samples = member_samples; a.member_off = member_off;
  a.src = src;
  int rc = ga_launch_member_episodes(&a, (hipStream_t)stream);
  if (rc) return rc;
  // a member's rows are shared out 256 at a time; the kernel strides over what is left
  int64_t bx = ga_ceil_div(ga_ceil_div(max_samples, n_members), 256);
  if (bx > 4096) bx = 4096;
  return ga_launch_member_src(&a, bx, (hipStream_t)stream);
}

extern "C" int ga_member_pack_gather(const ga_pack_plane* planes, int64_t n_planes,
                                     const int32_t* src, int64_t n_rows,
                                     const int32_t* ep_env, const int32_t* ep_end,
                                     int64_t n_eps, int64_t Tcap, ga_stream_t stream) {
  const char* who = "ga_member_pack_gather";
  GA_REQUIRE(planes && src, "%s: null pointer", who);
  GA_REQUIRE(n_planes >= 1 && n_planes <= GA_PACK_MAX_PLANES,
             "%s: n_planes must be in 1..%d (got %lld)", who, GA_PACK_MAX_PLANES,
             (long long)n_planes);
  GA_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31),
             "%s: n_rows must be in 1..2^31 - 1 (got %lld)", who, (long long)n_rows);
  GA_REQUIRE(n_eps >= 0 && n_eps < (1ll << 31), "%s: bad n_eps %lld", who,
             (long long)n_eps);
  GA_REQUIRE(Tcap >= 1 && Tcap < (1ll << 31), "%s: Tcap must be in 1..2^31 - 1 (got %lld)",
             who, (long long)Tcap);
  GaPackTable t;
  memset(&t, 0, sizeof(t));
  t.src = src; t.ep_env = ep_env; t.ep_end = ep_end; t.Tcap = Tcap;
  t.n_planes = (int32_t)n_planes;
  int64_t most = 1;
  for (int64_t i = 0; i < n_planes; ++i) {
    const ga_pack_plane& p = planes[i];
    GA_REQUIRE(p.src && p.dst, "%s: null pointer in plane %lld", who, (long long)i);
    GA_REQUIRE(p.elem_size == 1 || p.elem_size == 4,
               "%s: plane %lld: elem_size must be 1 or 4 (got %d)", who, (long long)i,
               (int)p.elem_size);
    GA_REQUIRE(p.width >= 1 && p.ld_src >= p.width && p.ld_dst >= p.width,
               "%s: plane %lld: rows of %d elements with strides %lld / %lld", who,
               (long long)i, (int)p.width, (long long)p.ld_src, (long long)p.ld_dst);
    if (p.per_episode) {
      GA_REQUIRE(ep_env && ep_end, "%s: null pointer (plane %lld is per episode)", who,
                 (long long)i);
      GA_REQUIRE(n_eps >= 1, "%s: plane %lld is per episode and n_eps is 0", who,
                 (long long)i);
    }
    GaPackPlaneDev& d = t.plane[i];
    d.src = p.src; d.dst = p.dst; d.ld_src = p.ld_src; d.ld_dst = p.ld_dst;
    d.elem_size = p.elem_size; d.width = p.width; d.per_episode = p.per_episode != 0;
    d.rows = p.per_episode ? n_eps : n_rows;
    if (p.elem_size == 4 && p.width >= 4) {
      GA_REQUIRE(p.width % 4 == 0 && p.ld_src % 4 == 0 && p.ld_dst % 4 == 0 &&
                     ga_aligned16(p.src) && ga_aligned16(p.dst),
                 "%s: plane %lld: 4-byte rows of width >= 4 are copied as 16-byte "
                 "quads (width %d, strides %lld / %lld, pointers 16-byte aligned)", who,
                 (long long)i, (int)p.width, (long long)p.ld_src, (long long)p.ld_dst);
      d.path = GA_PACK_QUADS;
      d.units = d.rows * (p.width / 4);
    } else if (p.width == 1 && p.ld_dst == 1 &&
               (reinterpret_cast<uintptr_t>(p.dst) & (4u * p.elem_size - 1u)) == 0) {
      d.path = GA_PACK_SCALAR;  // four rows: one store of 4 elem_size bytes
      d.units = ga_ceil_div(d.rows, 4);
    } else {
      d.path = GA_PACK_ELEMS;
      d.units = d.rows * p.width;
    }
    if (d.units > most) most = d.units;
  }
  int64_t bx = ga_ceil_div(most, 256);
  if (bx > 8192) bx = 8192;
  return ga_launch_member_gather(&t, bx, (hipStream_t)stream);
}
