// circular_check.cpp -- SamplerCircular's host side (gat_amd/csrc/gat_prep_units.h: circular_intervals, prepare_unit, base_cap_for)
// on hand-made units and against a base-by-base definition on random ones.  Host only: tests/test_circular_host.py compiles
// it with the address and undefined-behaviour sanitizers and runs it; exit status 0 = every check held, else the failed
// checks are on stderr.
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
typedef std::vector<std::pair<uint32_t, uint32_t>> Pairs;          // {linear start, length}

static gat_segment seg(uint32_t s, uint32_t e) { gat_segment g; g.start = s; g.end = e; return g; }

// one unit through prepare_unit as a problem without tracks (n_tracks 0) or with one
static void prepare_one(const List& segs, const List& w, int32_t n_tracks, UnitDev& U, UnitPrep& R) {
  const int64_t seg_off[2] = {0, (int64_t)segs.size()}, ws_off[2] = {0, (int64_t)w.size()};
  const int32_t unit_contig[1] = {0};
  gat_problem_desc d = {};
  d.n_units = 1; d.segs = segs.data(); d.seg_off = seg_off; d.ws = w.data(); d.ws_off = ws_off;
  d.unit_contig = unit_contig; d.n_contigs = 1; d.nbuckets = 100000; d.bucket_size = 1; d.sampler = GAT_SAMPLER_CIRCULAR;
  d.n_tracks = n_tracks;
  const Knobs kn;
  prepare_unit(d, kn, 0, U, R);
}

static Pairs intervals_of(const UnitPrep& R) {
  Pairs p;
  for (const uint2& v : R.circ_iv) p.push_back(std::make_pair(v.x, v.y));
  return p;
}

static void check_hand_made() {
  const Knobs kn;
  {
    g_case = "bridging a gap, hanging over the edge";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(5, 25), seg(38, 50)}, {seg(0, 10), seg(20, 40)}, 0, U, R);
    CHECK(R.rc == 0 && R.active, "rc %d active %d", R.rc, (int)R.active);
    CHECK((intervals_of(R) == Pairs{{5u, 10u}, {28u, 2u}}), "%zu intervals", R.circ_iv.size());
    CHECK(U.hist_total == 2u && R.nwork == 2, "n %u nwork %lld", U.hist_total, (long long)R.nwork);
    CHECK(U.n_ws == 2 && U.ws_total == 30u, "|W| %d Wsum %u", U.n_ws, U.ws_total);
    CHECK(base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 2) == 4, "capacity %lld", (long long)base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 2));
  }
  {
    g_case = "touching workspace pieces stay two";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(5, 15)}, {seg(0, 10), seg(10, 20)}, 0, U, R);
    CHECK(R.ws.size() == 2 && R.cdf == (std::vector<uint32_t>{9u, 19u}), "%zu pieces", R.ws.size());
    CHECK((intervals_of(R) == Pairs{{5u, 10u}}), "%zu intervals", R.circ_iv.size());
    CHECK(base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 1) == 3, "capacity %lld", (long long)base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 1));
  }
  {
    g_case = "segments that touch in linear coordinates are united";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(6, 12), seg(18, 24), seg(30, 31)}, {seg(0, 10), seg(20, 40)}, 0, U, R);
    CHECK((intervals_of(R) == Pairs{{6u, 8u}, {20u, 1u}}), "%zu intervals", R.circ_iv.size());
    CHECK(U.hist_total == 2u, "n %u", U.hist_total);
  }
  {
    g_case = "one piece filled by one segment";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(90, 200)}, {seg(100, 110)}, 0, U, R);
    CHECK((intervals_of(R) == Pairs{{0u, 10u}}), "%zu intervals", R.circ_iv.size());
    CHECK(base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 1) == 2, "capacity %lld", (long long)base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, 1));
  }
  {
    g_case = "no working segment";
    UnitDev U = {};
    UnitPrep R;
    prepare_one({seg(50, 60), seg(70, 71)}, {seg(0, 10), seg(61, 70)}, 0, U, R);
    CHECK(R.rc == 0 && !R.active && R.circ_iv.empty(), "rc %d active %d", R.rc, (int)R.active);
  }
  {
    g_case = "coordinates beyond 2^31";
    UnitDev U = {};
    UnitPrep R;
    const List segs = {seg(10u, 20u), seg(2999999990u, 3000000000u)}, w = {seg(0u, 3000000000u)};
    prepare_one(segs, w, 0, U, R);
    CHECK(R.rc == 0 && R.active && U.ws_total == 3000000000u, "rc %d active %d Wsum %u", R.rc, (int)R.active, U.ws_total);
    CHECK((intervals_of(R) == Pairs{{10u, 10u}, {2999999990u, 10u}}), "%zu intervals", R.circ_iv.size());
    UnitDev U1 = {};
    UnitPrep R1;
    prepare_one(segs, w, 1, U1, R1);                       // (a problem that counts stays below 2^31)
    CHECK(R1.rc == GAT_ERR_ASSERT && !R1.active, "rc %d active %d", R1.rc, (int)R1.active);
  }
}

// random units against the definition: base x of the genome is a working base when a segment and a workspace piece hold it;
// the intervals are the maximal runs of working bases in linear order
static void check_random(std::mt19937& rng) {
  for (int it = 0; it < 400; ++it) {
    g_case = "random unit " + std::to_string(it);
    List w, segs;
    uint32_t x = rng() % 4u;
    const int nw = 1 + (int)(rng() % 6u);
    for (int j = 0; j < nw; ++j) {
      const uint32_t ln = 1u + rng() % 12u;
      w.push_back(seg(x, x + ln));
      x += ln + (rng() % 3u ? rng() % 5u : 0u);
    }
    const uint32_t top = w.back().end + 6u;
    uint32_t s = rng() % 5u;
    while (s < top) {
      const uint32_t ln = 1u + rng() % 9u;
      segs.push_back(seg(s, s + ln));
      s += ln + rng() % 8u;
    }
    Pairs want;
    uint32_t lin = 0;
    bool prev = false;
    for (const gat_segment& p : w)
      for (uint32_t g = p.start; g < p.end; ++g, ++lin) {
        bool in = false;
        for (const gat_segment& q : segs) in = in || (q.start <= g && g < q.end);
        if (in && prev) want.back().second++;
        else if (in) want.push_back(std::make_pair(lin, 1u));
        prev = in;
      }
    UnitDev U = {};
    UnitPrep R;
    prepare_one(segs, w, 0, U, R);
    CHECK(R.rc == 0, "rc %d (%s)", R.rc, R.err.c_str());
    CHECK(R.active == !want.empty(), "active %d, %zu intervals wanted", (int)R.active, want.size());
    if (!R.active) continue;
    CHECK(intervals_of(R) == want, "%zu intervals, %zu wanted", R.circ_iv.size(), want.size());
    CHECK(U.hist_total == (uint32_t)want.size() && U.ws_total == lin, "n %u Wsum %u", U.hist_total, U.ws_total);
    const Knobs kn;
    CHECK(base_cap_for(GAT_SAMPLER_CIRCULAR, kn, U, R, (int64_t)segs.size()) == (int64_t)want.size() + nw, "capacity");
  }
}

int main() {
  check_hand_made();
  std::mt19937 rng(20240611u);
  check_random(rng);
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  else printf("circular_check: all checks held\n");
  return g_failed ? 1 : 0;
}
