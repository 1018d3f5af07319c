// prep_units_check.cpp -- the table builders of gat_amd/csrc/gat_prep_units.h against their definitions, written here in
// plain loops.  Host only: tests/test_prep_units_host.py compiles it with the address and undefined-behaviour sanitizers
// and runs it; exit status 0 = every check held, else the failed checks are on stderr.
#include "gat_prep_units.h"
#include "gat_annotator_steps.h"

#include <random>

static int g_failed = 0;
static std::string g_case;

#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (++g_failed <= 40) {                                        \
        fprintf(stderr, "FAIL [%s] %s: ", g_case.c_str(), #cond);    \
        fprintf(stderr, __VA_ARGS__);                                \
        fprintf(stderr, "\n");                                       \
      }                                                              \
    }                                                                \
  } while (0)

// the workspace sizes at which the code takes another path
static const int kSizes[] = {1, 2, 3, 16, 17, 32, 33, 256, 257, 272, 4097, 20011};
enum Pattern { kEqual = 0, kShort = 1, kOneHuge = 2, kPatterns = 3 };
static const char* const kPatternName[] = {"equal", "1..3", "99%"};

// n pieces, ascending and disjoint (gaps of 0..3 bases: adjacent pieces are allowed in a normalized list)
static std::vector<gat_segment> make_workspace(int n, Pattern pat, std::mt19937& rng) {
  std::vector<uint32_t> len((size_t)n);
  uint64_t others = 0;
  for (int i = 0; i < n; ++i) {
    len[(size_t)i] = pat == kEqual ? 100u : 1u + rng() % 3u;
    others += len[(size_t)i];
  }
  if (pat == kOneHuge) {                                        // one piece holds 99 % of the bases
    const size_t big = (size_t)(rng() % (uint32_t)n);
    others -= len[big];
    len[big] = (uint32_t)std::max<uint64_t>(99u * others, 99u);
  }
  std::vector<gat_segment> w((size_t)n);
  uint32_t x = rng() % 50u;
  for (int i = 0; i < n; ++i) {
    w[(size_t)i].start = x;
    w[(size_t)i].end = x + len[(size_t)i];
    x = w[(size_t)i].end + rng() % 4u;
  }
  return w;
}

static void check_position_grid(const std::vector<gat_segment>& w) {
  const int64_t n = (int64_t)w.size();
  const int failed_before = g_failed;
  const std::vector<uint32_t> g = build_position_grid(w.data(), n);
  const uint32_t top = w.back().end;
  const int64_t want = std::min<int64_t>(2 * n, 65536);
  CHECK(g.size() > (size_t)gat::kGridHeader, "size %zu", g.size());
  const uint32_t shift = g[0];
  const int64_t cells = g[1];
  CHECK(shift < 32 && cells == ((int64_t)top >> shift) + 1, "shift %u cells %lld top %u", shift, (long long)cells, top);
  CHECK(cells <= want, "cells %lld > %lld", (long long)cells, (long long)want);
  CHECK(shift == 0 || ((int64_t)top >> (shift - 1)) + 1 > want, "shift %u is not the smallest", shift);
  CHECK(g[3] == 0u, "word 3 = %u", g[3]);
  CHECK(g.size() == (size_t)gat::kGridHeader + (size_t)cells + 1, "size %zu for %lld cells", g.size(), (long long)cells);
  if (g_failed != failed_before) return;                     // (the entries are where the header says)
  // entry c = #{pieces with end <= c << shift}: a piece counts from the first cell whose left edge reaches its end
  std::vector<uint32_t> first((size_t)cells + 2, 0u);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t c0 = ((uint64_t)w[(size_t)i].end + ((1ull << shift) - 1)) >> shift;
    first[(size_t)std::min<uint64_t>(c0, (uint64_t)cells + 1)] += 1u;
  }
  uint32_t count = 0, span = 0;
  const uint32_t* e = g.data() + gat::kGridHeader;
  for (int64_t c = 0; c < cells; ++c) {
    count += first[(size_t)c];
    CHECK(e[c] == count, "cell %lld: %u, want %u", (long long)c, e[c], count);
  }
  CHECK(e[cells] == (uint32_t)n, "last entry %u, want %lld", e[cells], (long long)n);
  for (int64_t c = 1; c <= cells; ++c) span = std::max(span, e[c] - e[c - 1]);
  CHECK(g[2] == span, "span %u, want %u", g[2], span);
}

static void check_tree(const std::vector<uint32_t>& keys, uint32_t pad, const char* what) {
  const std::vector<uint32_t> t = build_ws_tree(keys, pad);
  const int failed_before = g_failed;
  size_t off = 0, n = keys.size(), below_off = 0, below_n = 0;
  for (int level = 0;; ++level) {
    const size_t nodes = (n + 15) / 16;
    CHECK(off + nodes * 16 <= t.size(), "%s level %d: %zu words, the tree has %zu", what, level, off + nodes * 16, t.size());
    if (g_failed != failed_before) return;
    for (size_t j = 0; j < nodes * 16; ++j) {
      if (j >= n) { CHECK(t[off + j] == pad, "%s level %d pad %zu = %#x", what, level, j, t[off + j]); continue; }
      uint32_t want = 0;
      if (level == 0) want = keys[j];
      else for (size_t k = 16 * j; k < std::min(16 * j + 16, below_n); ++k) want = std::max(want, t[below_off + k]);   // its children
      CHECK(t[off + j] == want, "%s level %d node %zu = %u, want %u", what, level, j, t[off + j], want);
    }
    below_off = off; below_n = n;
    off += nodes * 16;
    if (n <= 16) break;
    n = nodes;
  }
  CHECK(off == t.size(), "%s: %zu words, want %zu", what, t.size(), off);
}

// the widest cell of a grid over the cumulated lengths with cells of 2^s: the fullest bin of cdf >> s
static uint32_t widest_cell(const std::vector<uint32_t>& cdf, int s) {
  std::vector<uint32_t> bin((size_t)(cdf.back() >> s) + 1, 0u);
  uint32_t widest = 0;
  for (uint32_t v : cdf) widest = std::max(widest, ++bin[(size_t)(v >> s)]);
  return widest;
}

// returns the refinement steps the builder took
static int check_cdf_grid(const std::vector<uint32_t>& cdf, int64_t cell_segs, std::mt19937& rng) {
  const int64_t n = (int64_t)cdf.size();
  const uint32_t tot = cdf.back() + 1u, topc = tot - 1u;
  const int failed_before = g_failed;
  const std::vector<uint32_t> grid = build_cdf_grid(cdf, n, tot, cell_segs);
  CHECK(grid.size() > (size_t)gat::kGridHeader, "size %zu", grid.size());
  const int shift = (int)grid[0];
  const int64_t cells = grid[1];
  CHECK(shift >= 0 && shift <= 16 && cells == ((int64_t)topc >> shift) + 1, "shift %d cells %lld", shift, (long long)cells);
  const size_t gw = ((size_t)cells + 2) / 2, kw = ((size_t)n + 1) / 2;
  CHECK(grid[3] == gw + kw && grid.size() == (size_t)gat::kGridHeader + gw + kw, "word 3 = %u, %zu words written, want %zu",
        grid[3], grid.size() - gat::kGridHeader, gw + kw);
  if (g_failed != failed_before) return 0;
  // where the refinement starts, and that it stopped where it should: widest cell <= 8, or no finer cells, or > 24 576 words
  int start = 16;
  while (start > 0 && ((int64_t)topc >> start) + 1 < n / cell_segs) --start;
  CHECK(shift <= start, "shift %d above the start %d", shift, start);
  CHECK(grid[2] == widest_cell(cdf, shift), "span %u, want %u", grid[2], widest_cell(cdf, shift));
  const int64_t words_finer = shift > 0 ? (((int64_t)topc >> (shift - 1)) + 1 + 2) / 2 + (n + 1) / 2 : 0;
  CHECK(grid[2] <= 8 || shift == 0 || words_finer > 24576, "stopped at span %u, shift %d, %lld words one finer", grid[2], shift, (long long)words_finer);
  for (int s = shift + 1; s <= start; ++s) CHECK(widest_cell(cdf, s) > 8, "refined beyond shift %d, whose widest cell is %u", s, widest_cell(cdf, s));
  // the look-up, for every cell boundary, its neighbours and a random sample: g[c] + #{keys of the cell < p & mask} = #{cdf < p}
  const uint16_t* g16 = reinterpret_cast<const uint16_t*>(grid.data() + gat::kGridHeader);
  const uint16_t* k16 = reinterpret_cast<const uint16_t*>(grid.data() + gat::kGridHeader + gw);
  const uint32_t mask = (1u << shift) - 1u;
  std::vector<uint32_t> ps;
  for (int64_t c = 0; c <= cells; ++c)
    for (int64_t dp = -1; dp <= 1; ++dp) {
      const int64_t p = (c << shift) + dp;
      if (p >= 0 && p < (int64_t)tot) ps.push_back((uint32_t)p);
    }
  for (int i = 0; i < 2000; ++i) ps.push_back((uint32_t)(rng() % tot));
  ps.push_back(topc);
  std::sort(ps.begin(), ps.end());
  size_t below = 0;                                              // #{cdf < p}, p ascending
  for (uint32_t p : ps) {
    while (below < (size_t)n && cdf[below] < p) ++below;
    const uint32_t c = p >> shift;
    uint32_t got = g16[c];
    CHECK(g16[c] <= g16[c + 1] && g16[c + 1] <= n, "cell %u: [%u, %u)", c, g16[c], g16[c + 1]);
    for (uint32_t i = g16[c]; i < g16[c + 1] && i < (uint32_t)n; ++i) got += k16[i] < (p & mask);
    CHECK(got == below, "p %u: %u, want %zu", p, got, below);
  }
  return start - shift;
}

static std::vector<uint32_t> cdf_of(const std::vector<gat_segment>& w) {
  std::vector<uint32_t> cdf;
  uint32_t tot = 0;
  for (const gat_segment& s : w) { tot += s.end - s.start; cdf.push_back(tot - 1u); }
  return cdf;
}

static uint32_t overlap(const std::vector<gat_segment>& w, const gat_segment& s) {
  uint32_t ov = 0;
  for (const gat_segment& p : w) if (p.start < s.end && s.start < p.end) ov += std::min(p.end, s.end) - std::max(p.start, s.start);
  return ov;
}

// one unit through prepare_unit: segments of 1..40 bases scattered over the workspace's extent and beyond it
static void check_prepare_unit(const std::vector<gat_segment>& w, int merge_contigs, std::mt19937& rng) {
  const int64_t nuw = (int64_t)w.size();
  std::vector<gat_segment> segs;
  const uint32_t extent = w.back().end + 200u;
  for (uint32_t x = rng() % 7u; x < extent && segs.size() < 300;) {
    const uint32_t l = 1u + rng() % 40u;
    segs.push_back(gat_segment{x, x + l});
    x += l + rng() % std::max(1u, extent / 150u);
  }
  // unit 0: those segments; unit 1: segments behind the workspace's end only (none is a working segment)
  std::vector<gat_segment> all_segs = segs, all_ws = w;
  all_segs.push_back(gat_segment{w.back().end + 5u, w.back().end + 9u});
  all_ws.insert(all_ws.end(), w.begin(), w.end());
  const int64_t seg_off[3] = {0, (int64_t)segs.size(), (int64_t)all_segs.size()}, ws_off[3] = {0, nuw, 2 * nuw};
  const int32_t unit_contig[2] = {0, 0};
  gat_problem_desc d = {};
  d.n_units = 2; d.segs = all_segs.data(); d.seg_off = seg_off; d.ws = all_ws.data(); d.ws_off = ws_off;
  d.unit_contig = unit_contig; d.n_contigs = 1; d.merge_contigs = merge_contigs; d.nbuckets = 100000; d.bucket_size = 3;
  d.sampler = GAT_SAMPLER_ANNOTATOR;
  const Knobs kn;
  {
    UnitDev U = {};
    UnitPrep R;
    prepare_unit(d, kn, 1, U, R);
    CHECK(R.rc == 0 && !R.active && R.rank.empty(), "a unit without working segments: rc %d active %d", R.rc, (int)R.active);
  }
  UnitDev U = {};
  UnitPrep R;
  prepare_unit(d, kn, 0, U, R);
  std::vector<uint32_t> want_rank(1, 0u);
  uint32_t ltotal = 0;
  for (const gat_segment& s : segs) {
    const uint32_t ov = overlap(w, s);
    if (ov == 0) continue;
    ltotal += ov;
    want_rank.push_back((s.end - s.start + 2u) / 3u);          // its bucket: ceil(length / bucket_size)
  }
  std::sort(want_rank.begin() + 1, want_rank.end());
  if (want_rank.size() == 1) { CHECK(R.rc == 0 && !R.active, "no working segment: rc %d active %d", R.rc, (int)R.active); return; }
  CHECK(R.rc == 0 && R.active, "rc %d (%s) active %d", R.rc, R.err.c_str(), (int)R.active);
  CHECK(R.rank == want_rank, "rank table of %zu entries, want %zu", R.rank.size(), want_rank.size());
  CHECK(U.hist_total == want_rank.size() - 1 && U.bucket == 3u && U.ltotal == (int32_t)ltotal && U.n_target == (int32_t)segs.size() &&
        R.nwork == (int64_t)want_rank.size() - 1, "hist_total %u bucket %u ltotal %d n_target %d", U.hist_total, U.bucket, U.ltotal, U.n_target);
  const std::vector<uint32_t> cdf = cdf_of(w);
  CHECK(R.cdf == cdf && U.ws_total == cdf.back() + 1u && U.n_ws == (int32_t)nuw, "cdf: ws_total %u n_ws %d", U.ws_total, U.n_ws);
  CHECK(R.ws.size() == w.size(), "ws: %zu entries", R.ws.size());
  for (size_t i = 0; i < R.ws.size() && i < w.size(); ++i) CHECK(R.ws[i].x == w[i].start && R.ws[i].y == w[i].end, "ws[%zu]", i);
  // which tables a workspace of this size gets (their contents: the checks of the builders)
  const bool want_pgrid = nuw > gat::kWsTreeMin || (merge_contigs && nuw > 2), want_trees = nuw > gat::kWsTreeMin;
  const bool want_cgrid = nuw > gat::kPlaceWsLds && nuw <= 65535 && cdf.back() > 0u;
  CHECK(R.pgrid.empty() == !want_pgrid && R.tree_start.empty() == !want_trees && R.tree_cdf.empty() == !want_trees &&
        R.cgrid.empty() == !want_cgrid, "tables: pgrid %zu trees %zu %zu cgrid %zu words", R.pgrid.size(), R.tree_start.size(),
        R.tree_cdf.size(), R.cgrid.size());
  if (want_pgrid) CHECK(R.pgrid == build_position_grid(w.data(), nuw), "pgrid is not build_position_grid's");
  if (want_trees) CHECK(R.tree_cdf == build_ws_tree(cdf, 0x7fffffffu), "tree_cdf is not build_ws_tree's");
  if (want_cgrid) CHECK(R.cgrid == build_cdf_grid(cdf, nuw, cdf.back() + 1u, 2), "cgrid is not build_cdf_grid's at two segments per cell");
}

// one unit (segments, workspace) through prepare_unit under a sampler kind and a bucket size
static void prepare_one(const std::vector<gat_segment>& segs, const std::vector<gat_segment>& w, int32_t sampler, uint32_t bucket_size,
                        UnitDev& U, UnitPrep& R) {
  const int64_t seg_off[2] = {0, (int64_t)segs.size()}, ws_off[2] = {0, (int64_t)w.size()};
  const int32_t unit_contig[1] = {0};
  gat_problem_desc d = {};
  d.n_units = 1; d.segs = segs.data(); d.seg_off = seg_off; d.ws = w.data(); d.ws_off = ws_off;
  d.unit_contig = unit_contig; d.n_contigs = 1; d.nbuckets = 100000; d.bucket_size = bucket_size; d.sampler = sampler;
  d.shift_radius = 2.0;
  const Knobs kn;
  prepare_unit(d, kn, 0, U, R);
}

// Lmax against the definition: the largest value length_draw returns over every rank and every draw inside the bucket
static void check_lmax() {
  const std::vector<std::vector<uint32_t>> length_sets = {
      {1u}, {4u, 4u, 4u, 4u}, {1u, 2u, 3u, 64u, 65u}, {7u, 130u, 129u, 128u}, {90u}, {40u, 48u, 41u}, {250001u, 3u}, {6350000u, 1u, 63u}};
  for (const std::vector<uint32_t>& lens : length_sets)
    for (uint32_t bucket_size : {0u, 1u, 3u, 64u}) {
      char name[96];
      snprintf(name, sizeof(name), "lmax: %zu lengths from %u, bucket_size %u", lens.size(), lens[0], bucket_size);
      g_case = name;
      std::vector<gat_segment> segs;
      uint32_t x = 10u, longest = 0u;
      for (uint32_t l : lens) { segs.push_back(gat_segment{x, x + l}); x += l + 5u; longest = std::max(longest, l); }
      const std::vector<gat_segment> w{{0u, x + 100u}};
      UnitDev U = {};
      UnitPrep R;
      prepare_one(segs, w, GAT_SAMPLER_ANNOTATOR, bucket_size, U, R);
      if (bucket_size && (longest + bucket_size - 1u) / bucket_size >= 100000u) {        // (beyond nbuckets: the reference's ValueError)
        CHECK(R.rc == GAT_ERR_VALUE, "a length beyond the buckets: rc %d", R.rc);
        continue;
      }
      CHECK(R.rc == 0 && R.active, "rc %d (%s)", R.rc, R.err.c_str());
      if (R.rc || !R.active) continue;
      const uint32_t want_bucket = bucket_size ? bucket_size : (uint32_t)std::ceil((double)longest / 100000.0);
      CHECK(U.bucket == want_bucket, "bucket %u, want %u", U.bucket, want_bucket);
      // every rank the first draw can name (1 + [0, hist_total - 2]; rank 1 alone for one segment), every second draw
      uint64_t brute = 0;
      const uint32_t last_d0 = U.hist_total > 1 ? U.hist_total - 2u : 0u;
      for (uint32_t d0 = 0; d0 <= last_d0; ++d0)
        for (uint32_t d1 = 0; d1 < std::max(U.bucket, 1u); ++d1) {
          int call = 0;
          const uint32_t got = gat::length_draw(U.hist_total, R.rank.data(), U.bucket, [&](uint32_t range) -> uint32_t {
            const bool first = call++ == 0 && U.hist_total > 1;
            CHECK((first ? d0 : d1) <= range, "draw beyond its range %u", range);
            return first ? d0 : d1;
          });
          brute = std::max<uint64_t>(brute, got);
        }
      CHECK(R.lmax == brute && unit_lmax(R.rank, U.bucket) == brute, "Lmax %llu, the largest length_draw %llu", (unsigned long long)R.lmax,
            (unsigned long long)brute);
      // ... which is the unit's second longest segment (its only one) rounded up to its bucket, plus the bucket's last base: the
      // reference's randint(1, total_size) never reaches the last rank
      std::vector<uint32_t> sorted = lens;
      std::sort(sorted.begin(), sorted.end());
      const uint64_t top = sorted.size() > 1 ? sorted[sorted.size() - 2] : sorted[0];
      const uint64_t want = (top + U.bucket - 1) / U.bucket * U.bucket + (U.bucket > 1 ? U.bucket - 1u : 0u);
      CHECK(brute == want, "largest draw %llu, want %llu", (unsigned long long)brute, (unsigned long long)want);
    }
}

// accept at the border (last workspace end + Lmax - 1 == 2^31 - 1), refuse one base further up: per sampler kind
static void check_domain() {
  const uint32_t T = 0x7fffffffu;
  const int32_t drawing[] = {GAT_SAMPLER_ANNOTATOR, GAT_SAMPLER_SEGMENTS, GAT_SAMPLER_BRUTE_FORCE};
  const int32_t others[] = {GAT_SAMPLER_SHIFT, GAT_SAMPLER_GLOBAL_PERMUTATION, GAT_SAMPLER_LOCAL_PERMUTATION};
  for (uint32_t bucket_size : {1u, 3u, 0u}) {
    // four segments of 4 bases (bucket 3: Lmax = 2 * 3 + 2 = 8; bucket 0 -> 1: Lmax 4), or one of 250 001 (bucket 0 -> 3)
    for (uint32_t seg_len : {4u, 250001u}) {
      if (bucket_size == 1u && seg_len > 99999u) continue;                                // (beyond nbuckets: another error)
      UnitDev U0 = {};
      UnitPrep R0;
      const uint32_t base = T - 2000000u;
      std::vector<gat_segment> segs;
      for (uint32_t i = 0; i < (seg_len == 4u ? 4u : 1u); ++i) segs.push_back(gat_segment{base + 10u * i, base + 10u * i + seg_len});
      prepare_one(segs, {{base, base + 300000u}}, GAT_SAMPLER_ANNOTATOR, bucket_size, U0, R0);
      const uint64_t lmax = R0.lmax;
      CHECK(R0.rc == 0 && lmax >= seg_len, "probe: rc %d Lmax %llu", R0.rc, (unsigned long long)lmax);
      const uint32_t ce_border = (uint32_t)((uint64_t)T - lmax + 1);                       // ce + Lmax - 1 == T
      for (uint32_t up : {0u, 1u}) {
        const uint32_t ce = ce_border + up;
        if (ce > T) continue;
        const std::vector<gat_segment> w{{base, base + 300000u}, {ce - 1u, ce}};
        char name[96];
        snprintf(name, sizeof(name), "domain: bucket_size %u segments of %u, last end border + %u", bucket_size, seg_len, up);
        g_case = name;
        for (int32_t s : drawing) {
          UnitDev U = {};
          UnitPrep R;
          prepare_one(segs, w, s, bucket_size, U, R);
          if (up == 0) CHECK(R.rc == 0 && R.active && R.lmax == lmax, "sampler %d at the border: rc %d (%s)", s, R.rc, R.err.c_str());
          else {
            char want_unit[32], want_end[32], want_lmax[32];
            snprintf(want_unit, sizeof(want_unit), "unit 0"); snprintf(want_end, sizeof(want_end), "%u", ce);
            snprintf(want_lmax, sizeof(want_lmax), "%llu", (unsigned long long)lmax);
            CHECK(R.rc == GAT_ERR_ARG && !R.active, "sampler %d one base past the border: rc %d active %d", s, R.rc, (int)R.active);
            CHECK(R.err.find(want_unit) != std::string::npos && R.err.find(want_end) != std::string::npos &&
                  R.err.find(want_lmax) != std::string::npos && R.err.find("2^31 - 1") != std::string::npos, "message: %s", R.err.c_str());
          }
        }
        for (int32_t s : others) {                             // their own rules: this one is not theirs
          UnitDev U = {};
          UnitPrep R;
          prepare_one(segs, w, s, bucket_size, U, R);
          CHECK(R.rc != GAT_ERR_ARG, "sampler %d: rc %d (%s)", s, R.rc, R.err.c_str());
        }
        // a unit without a working segment, or without a workspace, is not looked at
        UnitDev U = {};
        UnitPrep R;
        prepare_one({{5u, 9u}}, w, GAT_SAMPLER_ANNOTATOR, bucket_size, U, R);
        CHECK(R.rc == 0 && !R.active, "no working segment: rc %d active %d", R.rc, (int)R.active);
        UnitPrep R2;
        prepare_one(segs, {}, GAT_SAMPLER_ANNOTATOR, bucket_size, U, R2);
        CHECK(R2.rc == 0 && !R2.active, "no workspace: rc %d active %d", R2.rc, (int)R2.active);
      }
    }
  }
  // the helpers by themselves
  g_case = "domain helpers";
  CHECK(placement_in_domain(T, 1) && !placement_in_domain(T, 2) && placement_in_domain(T - 3u, 4) && !placement_in_domain(T - 3u, 5) &&
        placement_in_domain(1u, (uint64_t)T) && !placement_in_domain(2u, (uint64_t)T) && !placement_in_domain(T, 0xffffffffull * 3), "placement_in_domain");
  CHECK(unit_lmax({0u}, 5u) == 0 && unit_lmax({0u, 2u, 9u}, 1u) == 2 && unit_lmax({0u, 2u, 9u}, 4u) == 11 && unit_lmax({0u, 2u, 5u, 9u}, 4u) == 23 &&
        unit_lmax({0u, 9u}, 1u) == 9 && unit_lmax({0u, 0x7fffffffu}, 3u) == 3ull * 0x7fffffffull + 2, "unit_lmax");
}

int main() {
  check_lmax();
  check_domain();
  std::mt19937 rng(20240607u);
  int most_steps = 0;
  for (int n : kSizes)
    for (int pat = 0; pat < kPatterns; ++pat) {
      char name[64];
      snprintf(name, sizeof(name), "%d pieces, %s", n, kPatternName[pat]);
      g_case = name;
      const std::vector<gat_segment> w = make_workspace(n, (Pattern)pat, rng);
      const std::vector<uint32_t> cdf = cdf_of(w);
      std::vector<uint32_t> starts;
      for (const gat_segment& s : w) starts.push_back(s.start);
      check_position_grid(w);
      check_tree(starts, 0xffffffffu, "start tree");
      check_tree(cdf, 0x7fffffffu, "cdf tree");
      if (cdf.back() > 0u && n <= 65535)
        for (int64_t cell_segs : {2, 64}) {
          const int steps = check_cdf_grid(cdf, cell_segs, rng);
          if (n > 20000) most_steps = std::max(most_steps, steps);
        }
      check_prepare_unit(w, 0, rng);
      check_prepare_unit(w, 1, rng);
    }
  g_case = "20011 pieces";
  CHECK(most_steps >= 3, "the refinement loop took at most %d steps", most_steps);
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("prep_units_check: ok\n");
  return 0;
}
