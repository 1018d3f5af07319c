// annotator_steps_check.cpp -- the plain steps of SamplerAnnotator.sample's loop (gat_amd/csrc/gat_annotator_steps.h) against
// independent restatements: the unit's seed and the placement of one segment in 64-bit (128-bit) arithmetic, the length draw
// against a scripted stream, the consolidation's bookkeeping case by case, and trim_ends against a model that takes one base
// at a time off a std::vector.  Host only: tests/test_annotator_steps_host.py compiles it with the address and
// undefined-behaviour sanitizers and runs it; exit status 0 = every check held, else the failed checks are on stderr.
#include "gat_annotator_steps.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <random>
#include <vector>

static int g_failed = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++g_failed <= 40) {                             \
        fprintf(stderr, "FAIL %s: ", #cond);              \
        fprintf(stderr, __VA_ARGS__);                     \
        fprintf(stderr, "\n");                            \
      }                                                   \
    }                                                     \
  } while (0)

// ---- unit_stream_seed: (seed + sample * n_units + unit) mod 2^32, the sample counted from the run's first

static void check_seed(uint32_t seed, int64_t sample_begin, int64_t sidx, int32_t n_units, int32_t u) {
  const unsigned __int128 wide = (unsigned __int128)seed + (unsigned __int128)(sample_begin + sidx) * (unsigned __int128)n_units + (unsigned __int128)u;
  const uint32_t want = (uint32_t)(wide & 0xffffffffu);
  const uint32_t got = gat::unit_stream_seed(seed, sample_begin, sidx, n_units, u);
  CHECK(got == want, "seed %u begin %lld sidx %lld units %d unit %d: %u, want %u", seed, (long long)sample_begin, (long long)sidx, n_units, u, got, want);
}

static void check_seeds() {
  const uint32_t seeds[] = {0u, 1u, 42u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  const int64_t begins[] = {0, 1, 63, 64, 0xffffffffll, 0x100000000ll, (1ll << 40) + 12345, (1ll << 52) - 1, (1ll << 62)};
  const int64_t sidxs[] = {0, 1, 63, 64, 12499};
  const int32_t units[] = {1, 2, 24, 1000, 65535, 1 << 20};
  for (uint32_t s : seeds)
    for (int64_t b : begins)
      for (int64_t i : sidxs)
        for (int32_t n : units) {
          check_seed(s, b, i, n, 0);
          check_seed(s, b, i, n, n - 1);
        }
  // wrap-around: the sum passes 2^32 by one, the product passes 2^64
  check_seed(0xffffffffu, 0, 0, 1, 1);
  check_seed(0xfffffff0u, 0, 1, 16, 0);
  check_seed(1u, (1ll << 62), 3, 1 << 20, 7);
  // ... and how a run is cut into batches does not matter
  CHECK(gat::unit_stream_seed(7u, 0, 1000, 24, 5) == gat::unit_stream_seed(7u, 936, 64, 24, 5), "batch cut");
  std::mt19937_64 g(1);
  for (int t = 0; t < 20000; ++t)
    check_seed((uint32_t)g(), (int64_t)(g() >> 2), (int64_t)(g() % 100000), (int32_t)(g() % 1000000) + 1, (int32_t)(g() % 1000000));
}

// ---- the placement of one segment

// piece [cs, ce), the piece in front ends at prev_end (has_prev), a segment of `length`; every offset in `offsets`
static void check_place(int64_t cs, int64_t ce, bool has_prev, int64_t prev_end, int64_t length, bool all_offsets) {
  int64_t ss = cs - length + 1;
  if (has_prev) ss = std::max(ss, prev_end);
  const int64_t range = ce - 1 - ss;
  const gat::PlaceRange pr = gat::place_range((uint32_t)cs, (uint32_t)ce, has_prev ? (int32_t)prev_end : gat::kNoPieceInFront, (int32_t)length);
  CHECK((int64_t)pr.sampling_start == ss && (int64_t)pr.range == range && range >= 0,
        "piece [%lld, %lld) prev %d %lld length %lld: start %d range %u, want %lld %lld", (long long)cs, (long long)ce, (int)has_prev,
        (long long)prev_end, (long long)length, pr.sampling_start, pr.range, (long long)ss, (long long)range);
  std::vector<int64_t> offsets;
  constexpr int64_t kEdge = 4096;
  if (all_offsets && range <= 4 * kEdge) for (int64_t o = 0; o <= range; ++o) offsets.push_back(o);
  else if (all_offsets) {
    // a range of up to 2^31 offsets: the first and the last 4 096, the 4 096 around q == 0 (where the start clamps) and
    // 4 096 spread evenly -- the placement is piecewise linear in the offset with its kinks at those three places
    for (int64_t o = 0; o < kEdge; ++o) { offsets.push_back(o); offsets.push_back(range - o); }
    for (int64_t o = std::max<int64_t>(0, -ss - kEdge / 2); o <= std::min(range, -ss + kEdge / 2); ++o) offsets.push_back(o);
    for (int64_t i = 1; i < kEdge; ++i) offsets.push_back((int64_t)((unsigned __int128)range * (unsigned)i / kEdge));
  }
  else offsets = {0, range / 3, range / 2, range > 0 ? range - 1 : 0, range};
  for (int64_t o : offsets) {
    const int64_t q = ss + o;
    const int64_t start = std::max<int64_t>(0, q), end = q + length;
    const int64_t overlap = std::max<int64_t>(0, std::min(ce, end) - std::max(cs, start));
    const gat::Placed x = gat::place_at((uint32_t)cs, (uint32_t)ce, (int32_t)q, (int32_t)length);
    CHECK((int64_t)x.start == start && (int64_t)x.end == end && (int64_t)x.overlap == overlap,
          "piece [%lld, %lld) q %lld length %lld: [%u, %u) overlap %d, want [%lld, %lld) %lld", (long long)cs, (long long)ce, (long long)q,
          (long long)length, x.start, x.end, x.overlap, (long long)start, (long long)end, (long long)overlap);
    // (what the loop relies on: a placed segment overlaps its piece, and only q < 0 is clamped)
    CHECK(x.overlap >= 1, "piece [%lld, %lld) q %lld length %lld: no overlap", (long long)cs, (long long)ce, (long long)q, (long long)length);
    CHECK(q >= 0 || (x.start == 0 && (int64_t)x.end == q + length), "q %lld < 0: the start clamps, the end does not", (long long)q);
  }
}

static void check_placements() {
  // exhaustive small: first piece (no clamp), every end of a piece in front up to the piece's start, length 1 upwards
  for (int64_t cs = 0; cs <= 6; ++cs)
    for (int64_t ce = cs + 1; ce <= cs + 6; ++ce)
      for (int64_t length = 1; length <= 9; ++length) {
        check_place(cs, ce, false, 0, length, true);
        for (int64_t pe = 0; pe <= cs; ++pe) check_place(cs, ce, true, pe, length, true);
      }
  // q < 0: a long segment over a piece near the origin
  check_place(2, 10, false, 0, 50, true);
  check_place(0, 1, false, 0, 1, true);
  // the piece in front ends above start - length + 1, and exactly at it
  check_place(1000, 1100, true, 990, 64, true);
  check_place(1000, 1100, true, 1000 - 64 + 1, 64, true);
  check_place(1000, 1100, true, 1000, 64, true);
  // coordinates up to 2^31 - 1 (the reference's int32: the segment's end stays within it)
  const int64_t top = INT32_MAX;
  check_place(top - 100, top - 50, false, 0, 51, true);
  check_place(top - 1, top, true, top - 1, 1, true);
  check_place(top - 1000, top - 1, true, top - 5000, 2, false);
  check_place(0, top - 1, false, 0, 2, false);
  check_place(5, top - 10, true, 3, 11, false);
  // the exact border of the placement domain: ce + length - 1 == 2^31 - 1, so the last offset's segment ends AT 2^31 - 1
  // (gat_problem_create refuses a unit one base further up).  Every offset (for a range beyond 16 384: both ends, the
  // clamp at q == 0 and a spread); the piece first in its workspace, and behind a piece that ends at its start, one base
  // before, exactly at cs - length + 1, and further down than the segment reaches
  for (int64_t length : {(int64_t)1, (int64_t)2, (int64_t)64, (int64_t)1 << 30}) {
    const int64_t ce = top - length + 1;
    for (int64_t width : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)1000}) {
      const int64_t cs = ce - width;
      check_place(cs, ce, false, 0, length, true);
      for (int64_t pe : {cs, cs - 1, cs - length + 1, cs - length, cs - length - 7, (int64_t)0, (int64_t)1})
        if (pe >= 0 && pe <= cs) check_place(cs, ce, true, pe, length, true);
    }
    // ... and the piece from near 0 up to the border: q < 0 at the low offsets, the end at 2^31 - 1 at the last
    check_place(0, ce, false, 0, length, true);
    check_place(5, ce, false, 0, length, true);
    check_place(5, ce, true, 3, length, true);
  }
  // q < 0 on a piece near 0 under a length near 2^30 (the start clamps to 0, the end does not)
  for (int64_t length : {((int64_t)1 << 30) - 1, (int64_t)1 << 30, ((int64_t)1 << 30) + 1}) {
    check_place(0, 1, false, 0, length, true);
    check_place(3, 20, false, 0, length, true);
    check_place(3, 20, true, 2, length, true);
    check_place(7, top - length + 1, false, 0, length, true);
  }
  std::mt19937_64 g(2);
  for (int t = 0; t < 200000; ++t) {
    const int64_t length = 1 + (int64_t)(g() % (t % 2 ? 100000 : 60));
    const int64_t span = top - length;                                  // ce + length - 1 <= 2^31 - 1
    const int64_t ce = 1 + (int64_t)(g() % (uint64_t)span);
    const int64_t cs = (t % 3 == 0) ? std::max<int64_t>(0, ce - 1 - (int64_t)(g() % 100)) : (int64_t)(g() % (uint64_t)ce);
    const bool has_prev = (g() & 1) != 0 && cs > 0;
    const int64_t pe = has_prev ? ((g() & 1) ? cs - (int64_t)(g() % (uint64_t)std::min<int64_t>(cs, 2 * length)) : (int64_t)(g() % (uint64_t)(cs + 1))) : 0;
    check_place(cs, ce, has_prev, pe, length, false);
  }
}

// ---- the length draw: which ranges it asks for, in which order, and what it makes of the answers

static void check_length_draw() {
  const std::vector<uint32_t> rank_len{0u, 3u, 3u, 7u, 20u, 20u, 21u};       // [0] is never read: ranks start at 1
  for (uint32_t hist_total = 0; hist_total <= 6; ++hist_total)
    for (uint32_t bucket : {1u, 2u, 10u})
      for (uint32_t d0 = 0; d0 + 2 <= std::max(hist_total, 2u); ++d0)
        for (uint32_t d1 = 0; d1 < bucket; ++d1) {
          std::vector<uint32_t> asked;
          const uint32_t answers[2] = {d0, d1};
          const uint32_t got = gat::length_draw(hist_total, rank_len.data(), bucket, [&](uint32_t range) -> uint32_t {
            asked.push_back(range);
            return hist_total > 1 ? answers[asked.size() - 1] : d1;
          });
          std::vector<uint32_t> want_asked;
          if (hist_total > 1) want_asked.push_back(hist_total - 2u);
          if (bucket > 1) want_asked.push_back(bucket - 1u);
          const uint32_t rank = hist_total > 1 ? 1u + d0 : 1u;
          const uint32_t want = rank_len[rank] * bucket + (bucket > 1 ? d1 : 0u);
          CHECK(asked == want_asked, "hist_total %u bucket %u: %zu draws", hist_total, bucket, asked.size());
          CHECK(got == want, "hist_total %u bucket %u draws %u %u: %u, want %u", hist_total, bucket, d0, d1, got, want);
        }
}

// ---- the consolidation's bookkeeping and the loop's test

static void check_bookkeeping() {
  {  // progress: what is left changed -- it is taken over, the count of unsuccessful rounds stays
    int32_t tr = 1000; int nuns = 3;
    CHECK(gat::consolidate_progress(400, tr, nuns) && tr == 400 && nuns == 3, "progress: %d %d", tr, nuns);
    CHECK(gat::consolidate_progress(-7, tr, nuns) && tr == -7 && nuns == 3, "overshoot: %d %d", tr, nuns);
  }
  {  // no progress: counted, and the loop ends with the twentieth round
    int32_t tr = 55; int nuns = 0;
    for (int round = 1; round <= 20; ++round) {
      const bool on = gat::consolidate_progress(55, tr, nuns);
      CHECK(tr == 55 && nuns == round, "round %d: %d %d", round, tr, nuns);
      CHECK(on == (round < 20), "round %d: goes on %d", round, (int)on);
    }
    CHECK(gat::kMaxUnsuccessful == 20, "the reference's twenty rounds");
  }
  {  // nothing left: the loop ends at once, whatever the count
    int32_t tr = 12; int nuns = 0;
    CHECK(!gat::consolidate_progress(0, tr, nuns) && tr == 0 && nuns == 0, "remaining 0: %d %d", tr, nuns);
    int32_t tr0 = 0; int n0 = 5;
    CHECK(!gat::consolidate_progress(0, tr0, n0) && tr0 == 0 && n0 == 6, "remaining 0 twice: %d %d", tr0, n0);
  }
}

// ---- trim_ends

struct Seg { uint32_t x, y; };

static bool in_ws(const std::vector<Seg>& ws, uint32_t b) {
  for (const Seg& w : ws) if (b >= w.x && b < w.y) return true;
  return false;
}

// one base at a time: the element at hand loses its first (forward) or last base; when it is used up and bases are still to
// go it becomes the [0, 0) placeholder and the walk moves on, round the list's end
static void model_trim(std::vector<Seg>& L, int k, int64_t s, bool forward, const std::vector<Seg>& ws, uint32_t& removed, int& last) {
  const int n = (int)L.size();
  int idx = k;
  removed = 0;
  last = -1;
  auto step = [&]() { if (forward) { if (++idx == n) idx = 0; } else { if (--idx < 0) idx = n - 1; } };
  while (s > 0) {
    Seg& e = L[(size_t)idx];
    if (e.x == e.y) { e = {0u, 0u}; step(); continue; }
    const uint32_t b = forward ? e.x : e.y - 1u;
    if (forward) e.x++; else e.y--;
    if (in_ws(ws, b)) removed++;
    s--;
    last = idx;
    if (s > 0 && e.x == e.y) { e = {0u, 0u}; step(); }
  }
}

static void check_trim(const std::vector<Seg>& L0, int k, int32_t s, bool forward, const std::vector<Seg>& ws, const char* what) {
  std::vector<Seg> want = L0;
  uint32_t want_removed; int want_last;
  model_trim(want, k, s, forward, ws, want_removed, want_last);
  std::vector<uint2> got(L0.size());                                 // exactly n elements: an index beyond them is the sanitizer's
  for (size_t i = 0; i < L0.size(); ++i) got[i] = make_uint2(L0[i].x, L0[i].y);
  int bad_index = 0;
  const gat::TrimWalk r = gat::trim_ends_walk((int)got.size(), k, s, forward,
      [&](int i) -> uint2& { if (i < 0 || i >= (int)got.size()) { ++bad_index; i = 0; } return got[(size_t)i]; },
      [&](uint32_t a, uint32_t b) -> uint32_t {
        uint32_t ov = 0;
        for (const Seg& w : ws) { const uint32_t lo = std::max(a, w.x), hi = std::min(b, w.y); ov += hi > lo ? hi - lo : 0u; }
        return ov;
      });
  bool same = true;
  for (size_t i = 0; i < L0.size(); ++i) same = same && got[i].x == want[i].x && got[i].y == want[i].y;
  CHECK(bad_index == 0, "%s: n %zu k %d s %d forward %d: %d indices out of the list", what, L0.size(), k, s, (int)forward, bad_index);
  CHECK(same, "%s: n %zu k %d s %d forward %d: the list differs", what, L0.size(), k, s, (int)forward);
  CHECK(r.removed == want_removed, "%s: n %zu k %d s %d forward %d: removed %u, want %u", what, L0.size(), k, s, (int)forward, r.removed, want_removed);
  CHECK(r.last == want_last, "%s: n %zu k %d s %d forward %d: last %d, want %d", what, L0.size(), k, s, (int)forward, r.last, want_last);
}

// every start element, both directions, every s the caller may ask for (the list holds more than s bases)
static void check_trim_all(const std::vector<Seg>& L, const std::vector<Seg>& ws, const char* what) {
  int64_t total = 0;
  for (const Seg& e : L) total += e.y - e.x;
  for (int k = 0; k < (int)L.size(); ++k)
    for (int32_t s = 1; s < total; ++s)
      for (int f = 0; f < 2; ++f) check_trim(L, k, s, f != 0, ws, what);
  check_trim(L, 0, 0, true, ws, what);                               // (nothing to take: nothing touched, last -1)
}

static void check_trims() {
  const std::vector<Seg> ws_all{{0u, 1000u}}, ws_frag{{2u, 5u}, {9u, 10u}, {14u, 30u}}, ws_none{};
  // n = 1
  check_trim_all({{10u, 20u}}, ws_all, "n 1");
  check_trim_all({{3u, 12u}}, ws_frag, "n 1, fragmented workspace");
  // s equal to an element's length / spanning several / wrapping past either end: every (k, s, direction) of these lists
  check_trim_all({{0u, 4u}, {6u, 9u}, {12u, 13u}, {15u, 22u}}, ws_all, "four elements");
  check_trim_all({{0u, 4u}, {6u, 9u}, {12u, 13u}, {15u, 22u}}, ws_frag, "four elements, fragmented workspace");
  check_trim_all({{1u, 2u}, {3u, 4u}, {5u, 6u}, {7u, 8u}, {9u, 10u}}, ws_none, "unit elements, no workspace");
  // [0, 0) placeholders on the way (what an earlier trim left), at the ends and in a row
  check_trim_all({{0u, 0u}, {6u, 9u}, {0u, 0u}, {0u, 0u}, {15u, 22u}, {0u, 0u}}, ws_frag, "placeholders");
  check_trim_all({{2u, 7u}, {0u, 0u}, {11u, 12u}}, ws_all, "placeholder in the middle");
  // ... and an empty element that is not [0, 0) (a trim that ended exactly at an element's end leaves [y, y))
  check_trim_all({{2u, 7u}, {9u, 9u}, {11u, 15u}}, ws_all, "empty element");
  // exhaustive small: up to four elements of 0..3 bases with gaps of 1..2
  for (int n = 1; n <= 4; ++n) {
    const int combos = 1 << (3 * n);                                 // per element: 2 bits length, 1 bit gap
    for (int c = 0; c < combos; ++c) {
      std::vector<Seg> L;
      uint32_t pos = 1;
      for (int i = 0; i < n; ++i) {
        const uint32_t len = (uint32_t)((c >> (3 * i)) & 3), gap = 1u + (uint32_t)((c >> (3 * i + 2)) & 1);
        L.push_back(len ? Seg{pos, pos + len} : Seg{0u, 0u});
        pos += len + gap;
      }
      check_trim_all(L, ws_frag, "small");
    }
  }
  // seeded fuzz: longer lists, coordinates up to 2^31 - 1
  std::mt19937_64 g(3);
  for (int t = 0; t < 3000; ++t) {
    const int n = 1 + (int)(g() % 40);
    std::vector<Seg> L, ws;
    uint32_t pos = (t % 4 == 0) ? (uint32_t)INT32_MAX - 4000u : (uint32_t)(g() % 1000);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t len = (g() % 5 == 0) ? 0u : 1u + (uint32_t)(g() % 30);
      L.push_back(len ? Seg{pos, pos + len} : Seg{0u, 0u});
      if (g() % 3) ws.push_back({pos + (uint32_t)(g() % 4), pos + len + (uint32_t)(g() % 3)});
      total += len;
      pos += len + 3u + (uint32_t)(g() % 20);                          // (the workspace pieces stay apart: a normalized list)
    }
    if (total < 2) continue;
    for (int rep = 0; rep < 8; ++rep) {
      const int k = rep == 0 ? 0 : rep == 1 ? n - 1 : (int)(g() % (uint64_t)n);
      const int32_t s = 1 + (int32_t)(g() % (uint64_t)(total - 1));
      check_trim(L, k, s, (rep & 1) != 0, ws, "fuzz");
      check_trim(L, k, s, (rep & 1) == 0, ws, "fuzz");
    }
  }
}

int main() {
  check_seeds();
  check_placements();
  check_length_draw();
  check_bookkeeping();
  check_trims();
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("annotator_steps_check: all checks held\n");
  return 0;
}
