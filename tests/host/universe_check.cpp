// universe_check.cpp -- SamplerUniverse's host side (gat_amd/csrc/gat_prep_units.h: universe_hits, universe_record, prepare_unit,
// base_cap_for, universe_refusal) on hand-made units and against a base-by-base definition on random ones.  Host only:
// tests/test_universe_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit status 0 =
// every check held, else the failed checks are on stderr.
#include "gat_prep_units.h"

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

typedef std::vector<gat_segment> List;

static gat_segment seg(uint32_t s, uint32_t e) { gat_segment g; g.start = s; g.end = e; return g; }

// one unit through prepare_unit
static void prepare_one(const List& segs, const List& w, UnitDev& U, UnitPrep& R) {
  const int64_t seg_off[2] = {0, (int64_t)segs.size()}, ws_off[2] = {0, (int64_t)w.size()};
  const int32_t unit_contig[1] = {0};
  gat_problem_desc d = {};
  d.n_units = 1; d.segs = segs.data(); d.seg_off = seg_off; d.ws = w.data(); d.ws_off = ws_off;
  d.unit_contig = unit_contig; d.n_contigs = 1; d.nbuckets = 100000; d.bucket_size = 1; d.sampler = GAT_SAMPLER_UNIVERSE;
  const Knobs kn;
  prepare_unit(d, kn, 0, U, R);
}

static bool record_is(const uint4& r, uint32_t k, uint32_t m, uint32_t c, uint32_t invert) {
  return r.x == k && r.y == m && r.z == c && r.w == invert;
}

static void check_records() {
  g_case = "records";
  CHECK(record_is(universe_record(0, 5), 0u, 5u, 0u, 0u), "k 0");
  CHECK(record_is(universe_record(5, 5), 5u, 5u, 0u, 1u), "k m");
  CHECK(record_is(universe_record(1, 1), 1u, 1u, 0u, 1u), "m 1");
  CHECK(record_is(universe_record(3, 6), 3u, 6u, 3u, 0u), "2k == m");
  CHECK(record_is(universe_record(4, 7), 4u, 7u, 3u, 1u), "2k == m + 1");
  CHECK(record_is(universe_record(3, 7), 3u, 7u, 3u, 0u), "2k == m - 1");
  for (int64_t m = 0; m < 40; ++m)
    for (int64_t k = 0; k <= m; ++k) {
      const uint4 r = universe_record(k, m);
      CHECK(2 * (int64_t)r.z <= m && (int64_t)r.z == std::min(k, m - k) && (r.w != 0u) == (2 * k > m), "k %lld m %lld", (long long)k, (long long)m);
    }
}

static void check_hand_made() {
  const Knobs kn;
  const List w = {seg(0, 10), seg(10, 20), seg(30, 40)};
  {
    g_case = "a segment over two touching pieces hits two";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(5, 15)}, w, U, R);
    CHECK(R.rc == 0 && R.active, "rc %d active %d", R.rc, (int)R.active);
    CHECK(record_is(R.univ, 2u, 3u, 1u, 1u), "record %u %u %u %u", R.univ.x, R.univ.y, R.univ.z, R.univ.w);
    CHECK(R.ws.size() == 3 && U.n_ws == 3 && U.hist_total == 2u, "|W| %zu n_ws %d hist_total %u", R.ws.size(), U.n_ws, U.hist_total);
    CHECK(base_cap_for(GAT_SAMPLER_UNIVERSE, kn, U, R, 1) == 2, "capacity %lld", (long long)base_cap_for(GAT_SAMPLER_UNIVERSE, kn, U, R, 1));
  }
  {
    g_case = "three segments in one piece, one outside";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(1, 2), seg(3, 4), seg(5, 6), seg(22, 28)}, w, U, R);
    CHECK(R.active && record_is(R.univ, 1u, 3u, 1u, 0u), "record %u %u %u %u", R.univ.x, R.univ.y, R.univ.z, R.univ.w);
    CHECK(base_cap_for(GAT_SAMPLER_UNIVERSE, kn, U, R, 4) == 1, "capacity");
  }
  {
    g_case = "every piece hit";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(9, 31)}, w, U, R);
    CHECK(R.active && record_is(R.univ, 3u, 3u, 0u, 1u), "record %u %u %u %u", R.univ.x, R.univ.y, R.univ.z, R.univ.w);
    CHECK(base_cap_for(GAT_SAMPLER_UNIVERSE, kn, U, R, 1) == 3, "capacity");
  }
  {
    g_case = "segments in the gap and beyond: no hit piece, the unit is inactive";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(20, 30), seg(50, 60)}, w, U, R);
    CHECK(R.rc == 0 && !R.active, "rc %d active %d", R.rc, (int)R.active);
    CHECK(universe_hits(nullptr, 0, w.data(), 3) == 0, "no segments");
  }
  {
    g_case = "one piece";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(90, 200)}, {seg(100, 110)}, U, R);
    CHECK(R.active && record_is(R.univ, 1u, 1u, 0u, 1u), "record %u %u %u %u", R.univ.x, R.univ.y, R.univ.z, R.univ.w);
  }
}

// random units against the definition: a piece is hit when one of its bases lies in a segment
static void check_random(std::mt19937& rng) {
  int spanning = 0;
  for (int it = 0; it < 600; ++it) {
    g_case = "random unit " + std::to_string(it);
    List w, segs;
    uint32_t x = rng() % 4u;
    const int nw = 1 + (int)(rng() % 9u);
    for (int j = 0; j < nw; ++j) {
      const uint32_t ln = 1u + rng() % 12u;
      w.push_back(seg(x, x + ln));
      x += ln + (rng() % 3u ? rng() % 5u : 0u);
    }
    const uint32_t top = w.back().end + 6u;
    uint32_t s = rng() % 5u;
    while (s < top) {
      const uint32_t ln = 1u + rng() % 14u;
      segs.push_back(seg(s, s + ln));
      s += ln + rng() % 16u;
    }
    int64_t want = 0;
    for (const gat_segment& p : w) {
      bool hit = false;
      for (uint32_t g = p.start; g < p.end; ++g)
        for (const gat_segment& q : segs) hit = hit || (q.start <= g && g < q.end);
      want += hit;
    }
    for (const gat_segment& q : segs) {
      int n = 0;
      for (const gat_segment& p : w) n += p.start < q.end && q.start < p.end;
      spanning += n > 1;
    }
    CHECK(universe_hits(segs.data(), (int64_t)segs.size(), w.data(), nw) == want, "k %lld, %lld wanted",
          (long long)universe_hits(segs.data(), (int64_t)segs.size(), w.data(), nw), (long long)want);
    UnitDev U = {};
    UnitPrep R;
    prepare_one(segs, w, U, R);
    CHECK(R.rc == 0, "rc %d (%s)", R.rc, R.err.c_str());
    CHECK(R.active == (want > 0), "active %d, k %lld", (int)R.active, (long long)want);
    if (!R.active) continue;
    const uint4 r = universe_record(want, nw);
    CHECK(record_is(R.univ, r.x, r.y, r.z, r.w), "record %u %u %u %u", R.univ.x, R.univ.y, R.univ.z, R.univ.w);
    const Knobs kn;
    CHECK(base_cap_for(GAT_SAMPLER_UNIVERSE, kn, U, R, (int64_t)segs.size()) == want, "capacity");
    CHECK(U.hist_total == (uint32_t)want && U.n_ws == nw, "hist_total %u n_ws %d", U.hist_total, U.n_ws);
  }
  g_case = "random units";
  CHECK(spanning > 100, "%d segments over several pieces", spanning);
}

// the mark table: whole wave steps of 64 words beside the generator's 2 560 bytes
static void check_table_and_refusal() {
  g_case = "mark table";
  CHECK(universe_table_words(1) == 64 && universe_table_words(2048) == 64 && universe_table_words(2049) == 128, "words");
  CHECK(universe_table_words(0) == 0 && universe_table_words(4097) == 192, "words");
  const int64_t lds = 160 * 1024;
  const int64_t most = universe_max_pieces(lds);
  CHECK(most == 1290240, "%lld pieces", (long long)most);
  CHECK(gat::kUniverseFixedLdsBytes + universe_table_words(most) * 4 <= lds, "the largest table fits");
  CHECK(gat::kUniverseFixedLdsBytes + universe_table_words(most + 1) * 4 > lds, "one piece more does not");
  CHECK(universe_max_pieces(64 * 1024) == 503808 && universe_max_pieces(2560) == 0 && universe_max_pieces(0) == 0, "other limits");
  CHECK(universe_refusal(3, most, lds).empty() && universe_refusal(3, 1, lds).empty(), "fits");
  const std::string msg = universe_refusal(3, most + 1, lds);
  CHECK(msg.find("unit 3") != std::string::npos && msg.find("SamplerUniverse") != std::string::npos &&
        msg.find("1290241 workspace pieces") != std::string::npos && msg.find("at most 1290240") != std::string::npos, "%s", msg.c_str());
}

int main() {
  check_records();
  check_hand_made();
  std::mt19937 rng(20240628u);
  check_random(rng);
  check_table_and_refusal();
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  else printf("universe_check: all checks held\n");
  return g_failed ? 1 : 0;
}
