// gat_prep_units.h -- the host-side preparation of ONE unit (gat/Engine.pyx:543-565, hoisted to problem creation): the
// working segments, the rank table, the workspace's cumulated lengths, and the tables the placement kernels search -- the
// position grid, the 16-ary trees, the grid over the cumulated lengths -- plus the list samplers' own tables.  Plain host
// code: no context, no problem record, no runtime call, so every builder here runs (and is checked: tests/host/) without a
// device.  gat_prep.hip calls prepare_unit per unit on the host threads and deals out the offsets behind it.
#pragma once
#include <hip/hip_vector_types.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/gat_mi355.h"
#include "gat_types.h"
#include "gat_knobs.h"
#include "gat_samplers.h"

using gat::UnitDev;

// the samplers that draw a segment's length from the unit's histogram: only they are bound by nbuckets
inline bool sampler_draws_lengths(int32_t s) { return sampler_info(s) != nullptr && sampler_info(s)->draws_lengths; }

// SamplerCircular computes on 64-bit linear positions and never leaves the workspace, so a problem that only samples -- no
// annotation tracks, no isochore keys: nothing is counted or merged -- takes the whole uint32 range; whatever counts or merges
// compares coordinates as the reference's int32 lmin / lmax do and stays below 2^31
inline bool sampler_takes_wide_coordinates(const gat_problem_desc& d) {
  return d.sampler == GAT_SAMPLER_CIRCULAR && d.n_tracks == 0 && !d.merge_contigs;
}

// Lmax: the largest value length_draw (gat_annotator_steps.h) can return on a unit's rank table {0, the buckets of its
// hist_total working segments in ascending order}.  The rank drawn is 1 + [0, hist_total - 2] (the reference's
// randint(1, total_size) excludes total_size, gat/Engine.pyx:420; rank 1 when hist_total is 1), so the largest bucket
// that can be drawn is rank[hist_total - 1] -- the table's last entry is never drawn when it has two or more; the length
// is that bucket times the bucket size, plus the largest draw inside the bucket: with bucket > 1 a drawn length can
// exceed every segment of the unit.
inline uint64_t unit_lmax(const std::vector<uint32_t>& rank, uint32_t bucket) {
  if (rank.size() < 2) return 0;
  const size_t top = std::max<size_t>(1, rank.size() - 2);
  return (uint64_t)rank[top] * bucket + (bucket > 1 ? bucket - 1u : 0u);
}

// The placement domain of those samplers: a placed segment starts at ce - 1 at the latest (ce: the end of the workspace's
// last piece) and so ends at ce + Lmax - 1 at the most; that end has to stay a coordinate (< 2^31).  Beyond it the
// reference computes on wrapped int32 values ("The placement domain") and nothing is defined.
constexpr uint64_t kMaxCoordinate = 0x7fffffffull;
inline bool placement_in_domain(uint32_t last_ws_end, uint64_t lmax) { return (uint64_t)last_ws_end + lmax <= kMaxCoordinate + 1; }

// everything a unit needs by itself, in a record of its own; the offsets into the shared tables are dealt out in unit
// order behind it (gat_prep.hip: gather_unit_tables)
struct UnitPrep {
  int rc = 0;
  std::string err;
  bool active = false;
  std::vector<uint32_t> rank;          // rank 0 (never drawn) + the bucket indices in ascending order
  std::vector<uint2> ws;
  std::vector<uint32_t> cdf, tree_start, tree_cdf;
  std::vector<uint32_t> pgrid, cgrid;  // the grids of a fragmented workspace, header included (UnitDev::pgrid_off / cgrid_off)
  std::vector<uint4> shift;            // GAT_SAMPLER_SHIFT: two records per working segment (gat_problem::d_shift)
  std::vector<uint32_t> lens;          // GAT_SAMPLER_GLOBAL_PERMUTATION: the working lengths, W, its cumulated lengths, free
  std::vector<uint2> perm_w;
  std::vector<uint32_t> perm_cum;
  int64_t perm_free = 0;
  std::vector<uint2> circ_iv;          // GAT_SAMPLER_CIRCULAR: the working list in linear workspace coordinates {start, length}
  uint4 univ = {0u, 0u, 0u, 0u};       // GAT_SAMPLER_UNIVERSE: {k, m, c, invert} (universe_record)
  std::vector<uint4> lperm;            // GAT_SAMPLER_LOCAL_PERMUTATION: the active pieces, the sum and maximum of their n
  int64_t lperm_sum_n = 0, lperm_max_n = 0;
  int64_t nwork = 0;
  uint64_t lmax = 0;                   // unit_lmax of the rank table (the samplers that draw lengths)
  double cv2 = 0.0;
};

template <typename... Args>
inline void fail_unit(UnitPrep& R, int code, const char* fmt, Args... args) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, args...);
  R.rc = code; R.err = buf;
}

inline uint32_t host_overlap(const gat_segment* w, int64_t nw, uint32_t s, uint32_t e) {
  // bases of [s,e) inside the normalized list w
  uint32_t ov = 0;
  const gat_segment* it = std::lower_bound(w, w + nw, s, [](const gat_segment& a, uint32_t v) { return a.end <= v; });
  for (; it != w + nw && it->start < e; ++it) ov += std::min(e, it->end) - std::max(s, it->start);
  return ov;
}

// SamplerShift (gat/Engine.pyx:1063-1084): the window of every working segment -- [max(0, mid - area), max(0, mid + area)]
// in the reference's int32 lmax, the workspace segments overlapping it, truncated to it and normalized (empties dropped:
// gat/SegmentList.pyx:1186-1203).  Those are the workspace segments with end > window start and start < window end, a
// contiguous run [lo, hi]; only the run's first start and last end are clipped.  Two records per working segment.
inline void shift_windows(std::vector<uint4>& out, const gat_segment* us, int64_t nus, const gat_segment* uw, int64_t nuw,
                          const std::vector<uint32_t>& cdf, double radius, int32_t extension) {
  const double half_radius = radius / 2;
  for (int64_t i = 0; i < nus; ++i) {
    if (host_overlap(uw, nuw, us[i].start, us[i].end) == 0) continue;          // working = segments.filter(workspace)
    const uint32_t length = us[i].end - us[i].start;
    const uint32_t mid = us[i].start + length / 2u;
    const int32_t area = extension ? extension / 2 : (int32_t)(uint32_t)(uint64_t)std::floor((double)length * half_radius);
    const int32_t ws_start = std::max<int32_t>(0, (int32_t)(mid - (uint32_t)area));
    const int32_t ws_end = std::max<int32_t>(0, (int32_t)(mid + (uint32_t)area));
    const uint32_t s0 = (uint32_t)ws_start, e0 = (uint32_t)ws_end;
    const gat_segment* lo_it = std::upper_bound(uw, uw + nuw, s0, [](uint32_t v, const gat_segment& g) { return v < g.end; });
    const gat_segment* hi_it = std::lower_bound(uw, uw + nuw, e0, [](const gat_segment& g, uint32_t v) { return g.start < v; });
    const int64_t lo = lo_it - uw, hi = (hi_it - uw) - 1;                     // pieces lo..hi
    uint32_t k = 0, fs = 0, le = 0, sum = 0;
    if (hi >= lo && s0 < e0) {
      k = (uint32_t)(hi - lo + 1);
      fs = std::max(uw[lo].start, s0);
      le = std::min(uw[hi].end, e0);
      if (k == 1) sum = le - fs;
      else {
        sum = (uw[lo].end - fs) + (le - uw[hi].start) + (cdf[(size_t)hi - 1] - cdf[(size_t)lo]);   // (cdf: cumulated lengths - 1)
      }
    }
    out.push_back(make_uint4(length, k ? (uint32_t)lo : 0u, k, sum));
    out.push_back(make_uint4(fs, le, 0u, 0u));
  }
}

// SamplerGlobalPermutation (gat/Engine.pyx:1284-1299): working = segments.filter(workspace) (kept whole), W = the workspace
// extended by them and merge(0)ed (adjacent pieces united), free = W.sum() - sum(lengths).  Appends W and its cumulated
// lengths; returns free (negative: the reference's randint(0, free) raises).
inline int64_t permute_tables(std::vector<uint2>& w, std::vector<uint32_t>& cum, const gat_segment* us, int64_t nus,
                              const gat_segment* uw, int64_t nuw) {
  std::vector<uint2> all;
  int64_t total = 0;
  all.reserve((size_t)(nus + nuw));
  for (int64_t i = 0; i < nuw; ++i) all.push_back(make_uint2(uw[i].start, uw[i].end));
  for (int64_t i = 0; i < nus; ++i) {
    if (host_overlap(uw, nuw, us[i].start, us[i].end) == 0) continue;
    all.push_back(make_uint2(us[i].start, us[i].end));
    total += us[i].end - us[i].start;
  }
  std::stable_sort(all.begin(), all.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
  for (const uint2& p : all) {
    if (!w.empty() && p.x <= w.back().y) w.back().y = std::max(w.back().y, p.y);
    else w.push_back(p);
  }
  int64_t sum = 0;
  for (const uint2& p : w) { sum += p.y - p.x; cum.push_back((uint32_t)sum); }
  return sum - total;
}

// SamplerCircular (no counterpart in the reference; DESIGN.md section 5, "k_circular"): the working list -- the unit's
// segments cut to the workspace -- in LINEAR workspace coordinates: a base of piece j at genome position x has the linear
// position x minus the gaps before it, cum(j - 1) + (x - start_j).  Pieces that touch in linear coordinates are united, so a
// segment bridging a workspace gap is one interval; the workspace's own pieces stay apart, touching or not.  Appends the
// intervals {linear start, length}, sorted, disjoint and non-touching.  cdf: the cumulated lengths - 1 (UnitPrep::cdf).
inline void circular_intervals(std::vector<uint2>& out, const gat_segment* us, int64_t nus, const gat_segment* uw, int64_t nuw,
                               const std::vector<uint32_t>& cdf) {
  for (int64_t i = 0; i < nus; ++i) {
    const uint32_t s = us[i].start, e = us[i].end;
    const gat_segment* it = std::lower_bound(uw, uw + nuw, s, [](const gat_segment& a, uint32_t v) { return a.end <= v; });
    for (; it != uw + nuw && it->start < e; ++it) {
      const int64_t j = it - uw;
      const uint32_t gs = std::max(s, it->start), ge = std::min(e, it->end);
      const uint32_t ls = (j ? cdf[(size_t)j - 1] + 1u : 0u) + (gs - it->start);
      if (!out.empty() && out.back().x + out.back().y == ls) out.back().y += ge - gs;
      else out.push_back(make_uint2(ls, ge - gs));
    }
  }
}

// SamplerUniverse (no counterpart in the reference; DESIGN.md section 5, "k_universe"): the unit's workspace pieces are the
// candidates.  k: the pieces that share at least one base with a segment -- one merge walk of the (normalized) segments
// against the pieces; a segment over two pieces hits two, one outside the workspace none.
inline int64_t universe_hits(const gat_segment* us, int64_t nus, const gat_segment* uw, int64_t nuw) {
  int64_t k = 0, j = 0;                // j: the first piece no segment so far has hit or passed
  for (int64_t i = 0; i < nus; ++i) {
    while (j < nuw && uw[j].end <= us[i].start) ++j;
    for (; j < nuw && uw[j].start < us[i].end; ++j) ++k;
  }
  return k;
}

// ... the unit's record {k, m, c, invert}: Floyd's algorithm marks the smaller side, c = k pieces when 2k <= m, else the
// m - k that stay out (invert)
inline uint4 universe_record(int64_t k, int64_t m) {
  const bool invert = 2 * k > m;
  return make_uint4((uint32_t)k, (uint32_t)m, (uint32_t)(invert ? m - k : k), invert ? 1u : 0u);
}

// ... and the table of m mark bits k_universe keeps in LDS beside the generator's state, in whole wave steps of 64 words
// (2 048 pieces): the words a launch needs for a unit of m pieces, and the most pieces a context's LDS limit takes
inline int64_t universe_table_words(int64_t m) { return (m + 2047) / 2048 * 64; }
inline int64_t universe_max_pieces(int64_t max_lds) {
  return std::max<int64_t>(0, (max_lds - gat::kUniverseFixedLdsBytes) / 4 / 64) * 2048;
}
// the message of a unit that does not fit (empty: it fits)
inline std::string universe_refusal(int u, int64_t m, int64_t max_lds) {
  if (m <= universe_max_pieces(max_lds)) return std::string();
  char buf[256];
  snprintf(buf, sizeof(buf), "unit %d: SamplerUniverse: %lld workspace pieces, the mark table in LDS takes at most %lld", u,
           (long long)m, (long long)universe_max_pieces(max_lds));
  return buf;
}

// SamplerLocalPermutation (gat/Engine.pyx:1174-1188): per workspace piece (ws, we) the working segments are
// getOverlappingSegments' set (gat/SegmentList.pyx:952-983) -- from the last segment with start <= ws (the first one when
// there is none) on, every segment with start <= we, whether or not it reaches the piece --, a contiguous run of the
// unit's list.  work_start / work_end come out as 0 / we: min() and max() of the run's list (built with _add, normalized
// flag 0) fail their assertion inside a cpdef that cannot raise and return 0.  free = we - sum(lengths).  Appends one
// record {first, n, we, free} per piece with n > 0; returns the index of the first piece with free < 0 (the reference's
// randint(0, free) raises), -1 when there is none.  sum_n / max_n: the run lengths' sum and maximum.
inline int64_t local_permute_tables(std::vector<uint4>& pieces, int64_t& sum_n, int64_t& max_n, const gat_segment* us, int64_t nus,
                                    const gat_segment* uw, int64_t nuw) {
  std::vector<uint64_t> cum((size_t)nus + 1, 0);
  for (int64_t i = 0; i < nus; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + (us[i].end - us[i].start);
  auto starts_le = [&](uint32_t x) {                       // segments with start <= x
    int64_t lo = 0, hi = nus;
    while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (us[m].start <= x) lo = m + 1; else hi = m; }
    return lo;
  };
  int64_t bad = -1;
  sum_n = max_n = 0;
  for (int64_t k = 0; k < nuw; ++k) {
    const int64_t first = std::max<int64_t>(0, starts_le(uw[k].start) - 1), n = starts_le(uw[k].end) - first;
    if (n <= 0) continue;
    const int64_t free_len = (int64_t)uw[k].end - (int64_t)(cum[(size_t)(first + n)] - cum[(size_t)first]);
    if (free_len < 0 && bad < 0) bad = k;
    pieces.push_back(make_uint4((uint32_t)first, (uint32_t)n, uw[k].end, (uint32_t)std::max<int64_t>(free_len, 0)));
    sum_n += n;
    max_n = std::max(max_n, n);
  }
  return bad;
}

inline int32_t cap_for(const Knobs& kn, int64_t n) {
  int64_t c = n + n / 4 + 96;
  if (kn.test_small_caps) c = n / 2 + 8;      // tests: force the overflow / retry path
  c = (c + 63) / 64 * 64;
  return (int32_t)c;
}

// a unit's capacity before scaling (gat_problem::h_base_cap), by sampler; nall: the unit's segments, filtered or not
inline int64_t base_cap_for(int32_t sampler, const Knobs& kn, const UnitDev& U, const UnitPrep& R, int64_t nall) {
  switch (sampler) {
    case GAT_SAMPLER_SEGMENTS: return cap_for(kn, std::max<int64_t>(R.nwork, nall));
    // (a segment gives one piece, two where it wraps round its window -- more only in fragmented windows, which the overflow
    //  path takes)
    case GAT_SAMPLER_SHIFT: return cap_for(kn, 2 * R.nwork);
    // (every accepted segment covers a base of the workspace, so `remaining` bounds the list; expected are about as many
    //  segments as the unit has -- more where some of them lie outside the workspace, whose bases are sampled too: twice
    //  the unit's segments to begin with, the overflow path beyond)
    case GAT_SAMPLER_BRUTE_FORCE: return cap_for(kn, std::min<int64_t>(std::max<int32_t>(U.ltotal, 0), 2 * nall));
    // (exact: the lengths and the sorted points at the top of the region when the unit is too long for LDS, the pieces --
    //  at most n + |W| -- below them)
    case GAT_SAMPLER_GLOBAL_PERMUTATION: return 2 * R.nwork + (int64_t)R.perm_w.size();
    // (exact: two slots per working segment of every piece -- a segment gives one piece, two where it wraps; a piece of
    //  more working segments than LDS holds keeps its lengths and points at the top of the region)
    // (exact: an interval gives one piece and one more per border of the workspace or wrap it crosses, |W| over the list)
    case GAT_SAMPLER_CIRCULAR: return (int64_t)R.circ_iv.size() + (int64_t)R.ws.size();
    // (exact: k whole pieces, nothing united or cut)
    case GAT_SAMPLER_UNIVERSE: return (int64_t)R.univ.x;
    case GAT_SAMPLER_LOCAL_PERMUTATION: return 2 * R.lperm_sum_n + (R.lperm_max_n > 2048 ? 2 * R.lperm_max_n : 0);
    default: return cap_for(kn, R.nwork);
  }
}

// Fragmented workspaces (the reference's own test data: 6 600 - 21 000 workspace segments per contig).  A tree search is four
// dependent 64-byte node reads; the two questions asked of a workspace have cheaper answers:
// (a) "how many bases of [s, e) lie inside?" (SegmentList.intersect(workspace).sum(), gat/Engine.pyx:596-598): a grid over
//     the POSITIONS, entry c = the first segment whose end lies beyond c << shift -- the segments that can overlap [s, e)
//     are walked from entry s >> shift (one or two for segments shorter than the workspace's pieces).  About two cells
//     per segment, at most 2^16.  Header (kGridHeader words): {shift, cells, widest cell's span, 0}.
inline std::vector<uint32_t> build_position_grid(const gat_segment* uw, int64_t nuw) {
  const uint32_t top = uw[nuw - 1].end;                      // (coordinates are below 2^31)
  int shift = 0;
  int64_t want = 2 * nuw;
  if (want > 65536) want = 65536;
  while (((int64_t)top >> shift) + 1 > want) ++shift;
  const int64_t cells = ((int64_t)top >> shift) + 1;
  std::vector<uint32_t> grid((size_t)gat::kGridHeader + (size_t)cells + 1, 0u);
  grid[0] = (uint32_t)shift; grid[1] = (uint32_t)cells;
  int64_t j = 0;
  uint32_t span = 0, prev = 0;
  for (int64_t c = 0; c <= cells; ++c) {
    const uint64_t x = (uint64_t)c << shift;
    while (j < nuw && (uint64_t)uw[j].end <= x) ++j;
    grid[(size_t)gat::kGridHeader + (size_t)c] = (uint32_t)j;
    if (c > 0) span = std::max(span, (uint32_t)j - prev);
    prev = (uint32_t)j;
  }
  grid[(size_t)gat::kGridHeader + (size_t)cells] = (uint32_t)nuw;       // (a position beyond the last cell: nothing to walk)
  grid[2] = span;
  return grid;
}

// long workspaces: a 16-ary search tree (gat_device.h, WsTree) over ascending keys, level by level from the keys themselves
// up to one node, every level padded to whole nodes with `pad`
inline std::vector<uint32_t> build_ws_tree(std::vector<uint32_t> level, uint32_t pad) {
  std::vector<uint32_t> tree;
  for (;;) {
    const size_t n = level.size(), nodes = (n + 15) / 16;
    tree.insert(tree.end(), level.begin(), level.end());
    tree.insert(tree.end(), nodes * 16 - n, pad);
    if (n <= 16) break;
    std::vector<uint32_t> up(nodes);
    for (size_t j = 0; j < nodes; ++j) up[j] = level[std::min(16 * j + 15, n - 1)];   // largest key of node j
    level.swap(up);
  }
  return tree;
}

// (b) "which segment holds base p of the workspace?" (SegmentListSampler.sample, gat/Engine.pyx:299-305: searchsorted over
//     cdf[i] = cumulated length - 1 with cmpPosition): a grid over the CUMULATED lengths, g[c] = #{i : cdf[i] < c << shift},
//     and 16-bit keys cdf[i] & mask -- within a cell the high bits agree, so #{cdf < p} = g[c] + #{i in [g[c], g[c + 1]) :
//     key[i] < (p & mask)}.  2 bytes per segment + 2 per cell: k_place_grid keeps the image in LDS, where the trees (64 bytes
//     per node and level, in global memory) were four dependent L2 round trips for EVERY random number of a chunk.  shift
//     <= 16 (the keys), at most 65 535 segments (the entries), the widest cell at most 8 segments where the cells allow it.
//     Header: {shift, cells, widest cell's span, words of the image}.  cell_segs: segments per cell to begin with
//     (GAT_GRID_CELL_SEGS; refdata, k_place_grid with eight tiles: 2.2 ms at two, 2.6 at eight: the halving search over a
//     cell's span is LDS round trips on the lane's chain).  Needs 1 < tot <= 2^31 and nuw <= 65 535.
inline std::vector<uint32_t> build_cdf_grid(const std::vector<uint32_t>& cdf, int64_t nuw, uint32_t tot, int64_t cell_segs) {
  const uint32_t topc = tot - 1u;                             // the largest p
  auto cells_at = [&](int s) { return ((int64_t)topc >> s) + 1; };
  auto fill = [&](int s, std::vector<uint32_t>& g) {          // g[c] for c = 0 .. cells; returns the widest cell's span
    g.resize((size_t)cells_at(s) + 1);
    int64_t j = 0;
    uint32_t span = 0;
    for (size_t c = 0; c < g.size(); ++c) {
      const uint64_t x = (uint64_t)c << s;
      while (j < nuw && (uint64_t)cdf[(size_t)j] < x) ++j;
      g[c] = (uint32_t)j;
      if (c > 0) span = std::max(span, g[c] - g[c - 1]);
    }
    return span;
  };
  int shift = 16;
  while (shift > 0 && cells_at(shift) < nuw / cell_segs) --shift;
  std::vector<uint32_t> g;
  uint32_t span = fill(shift, g);
  // finer while some cell holds more than 8 segments and the image stays below 96 KB (24 K words)
  while (span > 8 && shift > 0 && (cells_at(shift - 1) + 2) / 2 + (nuw + 1) / 2 <= 24576) span = fill(--shift, g);
  const int64_t cells = cells_at(shift);
  const size_t gw = ((size_t)cells + 2) / 2, kw = ((size_t)nuw + 1) / 2;
  std::vector<uint32_t> grid((size_t)gat::kGridHeader + gw + kw, 0u);
  grid[0] = (uint32_t)shift; grid[1] = (uint32_t)cells; grid[2] = span; grid[3] = (uint32_t)(gw + kw);
  uint16_t* g16 = reinterpret_cast<uint16_t*>(grid.data() + gat::kGridHeader);
  for (int64_t c = 0; c <= cells; ++c) g16[c] = (uint16_t)g[(size_t)c];
  uint16_t* k16 = reinterpret_cast<uint16_t*>(grid.data() + gat::kGridHeader + gw);
  const uint32_t mask = (1u << shift) - 1u;
  for (int64_t i = 0; i < nuw; ++i) k16[i] = (uint16_t)(cdf[(size_t)i] & mask);
  return grid;
}

// what check_list (gat_prep.hip) reports, as a yes or no.  wide: coordinates up to 2^32 - 1 (sampler_takes_wide_coordinates)
inline bool list_is_normalized(const gat_segment* l, int64_t n, bool wide = false) {
  for (int64_t i = 0; i < n; ++i)
    if (l[i].start >= l[i].end || (!wide && l[i].end >= 0x80000000u) || (i > 0 && l[i - 1].end > l[i].start)) return false;
  return true;
}

// squared coefficient of variation of the lengths drawn
inline double length_cv2(const std::vector<uint32_t>& lens) {
  double m1 = 0, m2 = 0;
  for (uint32_t l : lens) { m1 += (double)l; m2 += (double)l * (double)l; }
  m1 /= (double)lens.size(); m2 /= (double)lens.size();
  return m1 > 0 ? std::max(0.0, m2 / (m1 * m1) - 1.0) : 0.0;
}

// Unit u of the desc: U's own fields (everything but the offsets and the slab region) and R.  A unit without segments or
// workspace, or none of whose segments is a working one, stays inactive with R.rc == 0.  R.rc == GAT_ERR_ASSERT with R.err
// "segment" / "workspace": a list is not normalized -- the caller words the message (check_list, in unit order).
inline void prepare_unit(const gat_problem_desc& d, const Knobs& kn, int u, UnitDev& U, UnitPrep& R) {
  const gat_segment* us = d.segs + d.seg_off[u];
  const int64_t nus = d.seg_off[u + 1] - d.seg_off[u];
  const gat_segment* uw = d.ws + d.ws_off[u];
  const int64_t nuw = d.ws_off[u + 1] - d.ws_off[u];
  if (nus == 0 || nuw == 0) return;
  const bool wide = sampler_takes_wide_coordinates(d);
  if (!list_is_normalized(us, nus, wide)) { R.rc = GAT_ERR_ASSERT; R.err = "segment"; return; }       // gat/Engine.pyx:535-536: both
  if (!list_is_normalized(uw, nuw, wide)) { R.rc = GAT_ERR_ASSERT; R.err = "workspace"; return; }     // lists normalized
  const bool local = d.sampler == GAT_SAMPLER_LOCAL_PERMUTATION;
  if (local) {
    // the unit is active when some piece has a working segment (the segment in front of a piece counts): not filter()'s rule
    const int64_t bad = local_permute_tables(R.lperm, R.lperm_sum_n, R.lperm_max_n, us, nus, uw, nuw);
    if (bad >= 0)
      return fail_unit(R, GAT_ERR_ASSERT, "unit %d: SamplerLocalPermutation: the working segments of workspace piece %lld [%u, %u) are longer "
                       "than [0, %u) (free length < 0): the reference's randint raises ValueError", u, (long long)bad, uw[bad].start, uw[bad].end, uw[bad].end);
    if (R.lperm.empty()) return;       // no piece draws: an empty list, no RNG use
  }
  // working = segments.filter(workspace); ltotal = working.intersect(workspace).sum()
  uint32_t ltotal = 0, maxlen = 0;
  int64_t nwork = 0;
  std::vector<uint32_t> lens;
  lens.reserve((size_t)nus);
  for (int64_t i = 0; i < nus; ++i) {
    // (SamplerLocalPermutation: the unit's list as it is, no overlap asked)
    const uint32_t ov = local ? 0u : host_overlap(uw, nuw, us[i].start, us[i].end);
    if (ov == 0 && !local) continue;
    ltotal += ov;
    const uint32_t l = us[i].end - us[i].start;
    lens.push_back(l);
    maxlen = std::max(maxlen, l);
    nwork++;
  }
  if (nwork == 0) return;              // sample() returns an empty list, no RNG use (gat/Engine.pyx:545-546)
  // getLengthDistribution (gat/SegmentList.pyx:1148-1184)
  int64_t bucket = d.bucket_size;
  if (bucket == 0) bucket = (int64_t)std::ceil((double)(int32_t)maxlen / (double)d.nbuckets);
  // the histogram over the buckets, cumulated, read as "rank r -> bucket": the bucket indices in ascending order (a sort
  // of the unit's lengths; a std::map insertion per segment was most of this stage: 0.8 of config 2's 1.2 ms)
  R.rank.reserve(lens.size() + 1);
  R.rank.push_back(0u);                           // rank 0 is never drawn (r >= 1, gat/Engine.pyx:419-422)
  for (uint32_t l : lens) {
    const int64_t i = ((int64_t)l + bucket - 1) / bucket;
    if (i >= d.nbuckets && sampler_draws_lengths(d.sampler))
      return fail_unit(R, GAT_ERR_VALUE, "unit %d: segment of length %u too large: increase nbuckets (%d) or bucket_size (%lld)",
                       u, l, d.nbuckets, (long long)bucket);
    R.rank.push_back((uint32_t)i);
  }
  std::sort(R.rank.begin() + 1, R.rank.end());                    // ranks (cum-count, cum] of a bucket hold it
  U.hist_total = (uint32_t)lens.size();
  U.bucket = (uint32_t)bucket;
  R.lmax = unit_lmax(R.rank, (uint32_t)bucket);
  if (sampler_draws_lengths(d.sampler) && !placement_in_domain(uw[nuw - 1].end, R.lmax))
    return fail_unit(R, GAT_ERR_ARG, "unit %d: workspace end %u + longest drawn length %llu - 1 > 2^31 - 1: a placed segment could end at "
                     "or beyond 2^31, where nothing is defined (limit: workspace end + Lmax - 1 <= 2147483647; Lmax = largest "
                     "bucket the histogram can draw x bucket_size %lld, + bucket_size - 1 when it is > 1)", u, uw[nuw - 1].end, (unsigned long long)R.lmax,
                     (long long)bucket);
  R.cv2 = length_cv2(lens);
  // SegmentListSampler(workspace) (gat/Engine.pyx:261-277)
  U.n_ws = (int32_t)nuw;
  uint32_t tot = 0;
  R.ws.reserve((size_t)nuw); R.cdf.reserve((size_t)nuw);
  for (int64_t i = 0; i < nuw; ++i) {
    tot += uw[i].end - uw[i].start;
    R.ws.push_back(make_uint2(uw[i].start, uw[i].end));
    R.cdf.push_back(tot - 1u);
  }
  U.ws_total = tot;
  U.tree_start_off = -1;
  U.tree_cdf_off = -1;
  if (nuw > ((int64_t)1 << (4 * gat::kWsTreeLevels)))
    return fail_unit(R, GAT_ERR_CAPACITY, "unit %d: %lld workspace segments (> %lld)", u, (long long)nuw, (long long)((int64_t)1 << (4 * gat::kWsTreeLevels)));
  // (k_permute_local reads its own tables: no grids, no trees; isochore problems: k_units_overlap asks every candidate's unit)
  if (!local && (nuw > gat::kWsTreeMin || (d.merge_contigs && nuw > 2))) R.pgrid = build_position_grid(uw, nuw);
  if (!local && nuw > gat::kWsTreeMin) {
    std::vector<uint32_t> starts((size_t)nuw);
    for (int64_t i = 0; i < nuw; ++i) starts[(size_t)i] = uw[i].start;
    R.tree_start = build_ws_tree(std::move(starts), 0xffffffffu);
    R.tree_cdf = build_ws_tree(R.cdf, 0x7fffffffu);
    if (nuw > gat::kPlaceWsLds && nuw <= 65535 && tot > 1u && tot <= 0x80000000u)
      R.cgrid = build_cdf_grid(R.cdf, nuw, tot, std::max<int64_t>(1, kn.grid_cell_segs));
  }
  U.ltotal = (int32_t)ltotal;
  if (d.sampler == GAT_SAMPLER_BRUTE_FORCE) {
    // remaining = segments.sum() (gat/Engine.pyx:830): ALL of the unit's segments, neither filtered nor intersected, the
    // uint32 sum (gat/SegmentList.pyx:1607) assigned to an int32
    uint32_t all = 0;
    for (int64_t i = 0; i < nus; ++i) all += us[i].end - us[i].start;
    U.ltotal = (int32_t)all;
  }
  U.n_target = (int32_t)nus;                       // SamplerSegments places len(segments) segments
  if (d.sampler == GAT_SAMPLER_SHIFT) shift_windows(R.shift, us, nus, uw, nuw, R.cdf, d.shift_radius, d.shift_extension);
  if (d.sampler == GAT_SAMPLER_GLOBAL_PERMUTATION) {
    R.perm_free = permute_tables(R.perm_w, R.perm_cum, us, nus, uw, nuw);
    if (R.perm_free < 0)
      return fail_unit(R, GAT_ERR_VALUE, "unit %d: SamplerGlobalPermutation: the working segments overlap (free length %lld < 0)",
                       u, (long long)R.perm_free);
  }
  if (local || d.sampler == GAT_SAMPLER_GLOBAL_PERMUTATION) R.lens = std::move(lens);
  R.nwork = local ? R.lperm_sum_n : nwork;       // (the launch order: the longest draw chain first)
  if (d.sampler == GAT_SAMPLER_CIRCULAR) {
    circular_intervals(R.circ_iv, us, nus, uw, nuw, R.cdf);
    U.hist_total = (uint32_t)R.circ_iv.size();   // (n: the intervals the kernel maps, at most the working segments' pieces)
    R.nwork = (int64_t)R.circ_iv.size();
  }
  if (d.sampler == GAT_SAMPLER_UNIVERSE) {
    R.univ = universe_record(universe_hits(us, nus, uw, nuw), nuw);
    U.hist_total = R.univ.x;                     // (k: the pieces of every list)
    R.nwork = (int64_t)R.univ.z + nuw / 64;      // (the launch order: the marks' chain and the table's words)
  }
  R.active = true;
}
