// metagene_bins_check.cpp -- the arithmetic of one (segment, feature) pair of k_metagene (gat_amd/csrc/gat_metagene_bins.h)
// against the definition in 128-bit integers: for a plus feature the bin of base x is floor((x - (fs - F)) / w) upstream,
// Bf + floor((x - fs) * Bb / len) in the body, Bf + Bb + floor((x - fe) / w) downstream, and a minus feature is the mirror
// x -> fs + fe - 1 - x -- base by base; where a piece is too long for that, bin by bin with the first base of every bin found
// by bisection on the definition (the bin never decreases along the strand).  Also the stepping of the body's edges, the bin of
// a midpoint, the features a segment is walked over, and the LDS the launches size.
// Host only: tests/test_metagene_bins_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_metagene_bins.h"

#include <algorithm>
#include <cstdio>
#include <vector>

typedef __int128 i128;

static int g_failed = 0;
static long long g_pairs = 0, g_long = 0;

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

struct Geometry { int64_t fs, fe; bool minus; int32_t Bb, Bf; int64_t w; };
static const int64_t kTop = ((int64_t)1 << 32) - 1;

// the definition: the bin of base x, -1 outside the window
static int64_t bin_def(const Geometry& g, i128 x) {
  const i128 F = (i128)g.Bf * g.w, fs = g.fs, fe = g.fe;
  if (g.minus) x = fs + fe - 1 - x;
  if (x < fs - F || x >= fe + F) return -1;
  if (x < fs) return (int64_t)((x - (fs - F)) / g.w);
  if (x < fe) return g.Bf + (int64_t)((x - fs) * g.Bb / (fe - fs));
  return g.Bf + g.Bb + (int64_t)((x - fe) / g.w);
}

// [s, e) bin by bin from the definition: base by base where it is short, else every run of one bin found by bisection
static std::vector<int64_t> by_definition(const Geometry& g, int64_t s, int64_t e) {
  const int B = 2 * g.Bf + g.Bb;
  std::vector<int64_t> v((size_t)B, 0);
  const int64_t F = (int64_t)g.Bf * g.w, cs = std::max(s, g.fs - F), ce = std::min(e, g.fe + F);
  if (cs > s) CHECK(bin_def(g, cs - 1) < 0, "the base before the window has a bin");
  if (ce < e) CHECK(bin_def(g, ce) < 0, "the base behind the window has a bin");
  if (ce - cs <= 3000) {
    for (int64_t x = cs; x < ce; ++x) {
      const int64_t b = bin_def(g, x);
      CHECK(b >= 0 && b < B, "bin %lld of %d", (long long)b, B);
      if (b >= 0 && b < B) v[(size_t)b] += 1;
    }
    return v;
  }
  g_long += 1;
  // along the strand: t = 0 is the first base of the clipped piece in the direction of the strand
  const int64_t n = ce - cs;
  auto at = [&](int64_t t) { return bin_def(g, g.minus ? (i128)ce - 1 - t : (i128)cs + t); };
  int64_t t = 0;
  while (t < n) {
    const int64_t b = at(t);
    int64_t lo = t, hi = n;             // the first t' > t with at(t') > b
    while (hi - lo > 1) {
      const int64_t m = lo + (hi - lo) / 2;
      if (at(m) > b) hi = m; else lo = m;
    }
    CHECK(b >= 0 && b < B, "bin %lld of %d", (long long)b, B);
    if (b >= 0 && b < B) v[(size_t)b] += hi - t;
    t = hi;
  }
  return v;
}

// what metagene_piece says, spread over the bins as the kernel's vector has it
static std::vector<int64_t> by_piece(const Geometry& g, int64_t s, int64_t e, bool& any) {
  const int B = 2 * g.Bf + g.Bb;
  std::vector<int64_t> v((size_t)B, 0);
  gat::MetagenePiece p;
  any = gat::metagene_piece(s, e, g.fs, g.fe, g.minus, g.Bb, g.Bf, g.w, p);
  if (!any) return v;
  CHECK(p.up.fb >= 0 || p.down.fb >= 0 || p.body.fb >= 0, "a piece without a region");
  const gat::MetageneFlank* flanks[2] = {&p.up, &p.down};
  for (int side = 0; side < 2; ++side) {
    const gat::MetageneFlank& f = *flanks[side];
    if (f.fb < 0) continue;
    const int first_bin = side ? g.Bf + g.Bb : 0;
    CHECK(first_bin <= f.fb && f.fb <= f.lb && f.lb < first_bin + g.Bf, "flank %d bins [%d, %d]", side, f.fb, f.lb);
    if (f.fb < first_bin || f.lb >= first_bin + g.Bf || f.lb < f.fb) continue;
    CHECK(f.first >= 1 && (int64_t)f.first <= g.w && (int64_t)f.last <= g.w && (f.lb > f.fb) == (f.last > 0), "first %u last %u w %lld",
          f.first, f.last, (long long)g.w);
    v[(size_t)f.fb] += f.first;
    if (f.lb > f.fb) v[(size_t)f.lb] += f.last;
    for (int32_t b = f.fb + 1; b < f.lb; ++b) v[(size_t)b] += g.w;
  }
  if (p.body.fb >= 0) {
    const gat::MetageneBody& b = p.body;
    CHECK(0 <= b.fb && b.fb <= b.lb && b.lb < g.Bb && 0 <= b.oa && b.oa < b.ob && b.ob <= g.fe - g.fs, "body bins [%d, %d] offsets [%lld, %lld)",
          b.fb, b.lb, (long long)b.oa, (long long)b.ob);
    if (b.fb < 0 || b.lb >= g.Bb || b.lb < b.fb) return v;
    // the kernel's walk: the body offsets [lo, up) lie in body bin k
    gat::MetageneEdge E = b.edge;
    int64_t lo = b.oa;
    for (int32_t k = b.fb; k <= b.lb; ++k) {
      const int64_t edge = gat::metagene_edge_value(E), up = std::min(edge, b.ob);
      if (up > lo) v[(size_t)(g.Bf + k)] += up - lo;
      lo = up;
      gat::metagene_edge_next(E);
    }
    CHECK(lo == b.ob, "the walk over the body bins ends at %lld of %lld", (long long)lo, (long long)b.ob);
    CHECK(v[(size_t)(g.Bf + b.fb)] > 0 && v[(size_t)(g.Bf + b.lb)] > 0, "the first or the last body bin [%d, %d] got nothing", b.fb, b.lb);
  }
  return v;
}

static void check_pair(const Geometry& g, int64_t s, int64_t e) {
  if (s < 0) s = 0;
  if (e > kTop) e = kTop;
  if (e <= s) return;
  g_pairs += 1;
  bool any = false;
  const std::vector<int64_t> want = by_definition(g, s, e), got = by_piece(g, s, e, any);
  int64_t total = 0;
  for (size_t b = 0; b < want.size(); ++b) {
    total += want[b];
    CHECK(got[b] == want[b], "[%lld, %lld) feature [%lld, %lld) %c Bb %d Bf %d w %lld: bin %zu got %lld want %lld", (long long)s, (long long)e,
          (long long)g.fs, (long long)g.fe, g.minus ? '-' : '+', g.Bb, g.Bf, (long long)g.w, b, (long long)got[b], (long long)want[b]);
  }
  CHECK(any == (total > 0), "any %d total %lld", (int)any, (long long)total);
  // the midpoint form: one base, one bin
  const int64_t m = gat::profile_midpoint(s, e);
  CHECK(gat::metagene_bin(m, g.fs, g.fe, g.minus, g.Bb, g.Bf, g.w) == (int32_t)bin_def(g, m), "midpoint %lld: bin %d want %lld", (long long)m,
        gat::metagene_bin(m, g.fs, g.fe, g.minus, g.Bb, g.Bf, g.w), (long long)bin_def(g, m));
}

// the edges of the body bins: metagene_edge_at at every k, and stepped from 0, against ceil(k * len / Bb)
static void check_edges(int64_t len, int32_t Bb) {
  gat::MetageneEdge E = gat::metagene_edge_at(len, Bb, 0);
  for (int32_t k = 0; k <= Bb; ++k) {
    const int64_t want = (int64_t)(((i128)k * len + Bb - 1) / Bb);
    const gat::MetageneEdge A = gat::metagene_edge_at(len, Bb, k);
    CHECK(gat::metagene_edge_value(A) == want && gat::metagene_edge_value(E) == want && A.t == E.t && A.a == E.a,
          "len %lld Bb %d edge %d: at %lld stepped %lld want %lld", (long long)len, Bb, k, (long long)gat::metagene_edge_value(A),
          (long long)gat::metagene_edge_value(E), (long long)want);
    gat::metagene_edge_next(E);
  }
}

static void check_feature(const Geometry& g) {
  const int64_t F = (int64_t)g.Bf * g.w, lo = g.fs - F, hi = g.fe + F, len = g.fe - g.fs;
  const int64_t edges[4] = {lo, g.fs, g.fe, hi};
  for (int64_t edge : edges)
    for (int64_t d : {(int64_t)1, (int64_t)2, (int64_t)9, g.w, g.w + 1, len, (int64_t)2500}) {
      check_pair(g, edge - d, edge);           // bookended on the left of the edge
      check_pair(g, edge, edge + d);           // ... and on the right
      check_pair(g, edge - d, edge + d);       // across it
      check_pair(g, edge - d - 3, edge - 3);
      check_pair(g, edge + 1, edge + 1 + d);
    }
  check_pair(g, lo - 3, hi + 3);               // the segment swallows the window
  check_pair(g, lo, hi);
  check_pair(g, g.fs, g.fe);
  check_pair(g, g.fs + len / 3, g.fe - len / 4);
  check_pair(g, 0, kTop);
  // the body bin edges from inside: a base either side of every edge of a few bins
  for (int32_t k : {0, 1, g.Bb / 2, g.Bb - 1}) {
    const int64_t o = (int64_t)(((i128)k * len + g.Bb - 1) / g.Bb);
    check_pair(g, g.fs + o - 1, g.fs + o + 1);
    check_pair(g, g.fe - o - 1, g.fe - o + 1);
  }
}

// the walk: the features a segment meets are those in [first k with pm[k] > key (0 without a key), first k with fs[k] >= hi)
// that metagene_reaches keeps
static void check_reach() {
  uint64_t x = 88172645463325252ull;
  auto rnd = [&](uint64_t n) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (int64_t)(x % n); };
  for (int round = 0; round < 400; ++round) {
    const int K = 1 + (int)rnd(24);
    const int64_t F = round % 3 == 0 ? 0 : rnd(40), span = 600;
    std::vector<std::pair<int64_t, int64_t>> f;
    for (int k = 0; k < K; ++k) {
      const int64_t s = rnd(span), l = 1 + (k % 5 == 0 ? rnd(span) : rnd(30));     // long ones over short ones
      f.push_back({s, s + l});
    }
    std::sort(f.begin(), f.end());
    std::vector<uint32_t> pm((size_t)K);
    uint32_t m = 0;
    for (int k = 0; k < K; ++k) pm[(size_t)k] = m = std::max(m, (uint32_t)f[(size_t)k].second);
    for (int q = 0; q < 60; ++q) {
      const int64_t s = rnd(2 * span), e = s + 1 + rnd(50);
      uint32_t key = 0;
      int first = 0;
      if (gat::metagene_reach_key(s, F, key)) {
        CHECK((int64_t)key == s - F, "key %u of s %lld F %lld", key, (long long)s, (long long)F);
        first = (int)(std::upper_bound(pm.begin(), pm.end(), key) - pm.begin());
      } else {
        CHECK(s - F < 0, "no key with s %lld F %lld", (long long)s, (long long)F);
      }
      const int64_t hi = gat::metagene_reach_hi(e, F);
      for (int k = 0; k < K; ++k) {
        const bool meets = f[(size_t)k].first - F < e && f[(size_t)k].second + F > s;
        const bool walked = k >= first && f[(size_t)k].first < hi, kept = walked && gat::metagene_reaches(s, f[(size_t)k].second, F);
        CHECK(meets == kept, "segment [%lld, %lld) F %lld feature %d [%lld, %lld): meets %d walked %d kept %d", (long long)s, (long long)e,
              (long long)F, k, (long long)f[(size_t)k].first, (long long)f[(size_t)k].second, (int)meets, (int)walked, (int)kept);
        CHECK(!(k >= first && f[(size_t)k].first >= hi) || !meets, "the walk would stop before a feature that meets");
      }
    }
  }
  // the ends of the range: s - F = 2^32 - 2 is a key; fe + F passes 2^32
  uint32_t key = 0;
  CHECK(gat::metagene_reach_key(kTop - 1, 0, key) && key == (uint32_t)(kTop - 1), "key at the top");
  CHECK(!gat::metagene_reach_key(5, (int64_t)1 << 31, key), "a negative key");
  CHECK(gat::metagene_reaches(kTop - 1, kTop, (int64_t)1 << 31) && !gat::metagene_reaches(kTop - 1, kTop - 1, 0), "reaches at the top");
  CHECK(gat::metagene_reach_hi(kTop, (int64_t)1 << 31) == kTop + ((int64_t)1 << 31), "reach_hi at the top");
}

// the LDS of a launch and the table the search finds there
static void check_lds() {
  const int64_t lds = 160 * 1024;
  for (int64_t B : {1, 2, 90, 100, 256, 1023, 1024})
    for (int64_t G : {1, 3, 24, 100})
      for (int64_t knob : {0, 4, 1024, 1 << 20})
        for (int64_t longest : {1, 5, 1000, 100000}) {
          const int64_t L = gat::metagene_lds_features(knob, longest, lds, B, G);
          CHECK(0 <= L && L <= knob && L <= longest, "L %lld knob %lld longest %lld", (long long)L, (long long)knob, (long long)longest);
          for (int store = 0; store < 2; ++store) {
            const int64_t bytes = gat::metagene_lds_bytes(B, L, G, store != 0);
            CHECK(bytes == B * (store ? 0 : 36) + B * 8 * gat::kMetageneWaves + G * L * 4, "bytes %lld", (long long)bytes);
            CHECK(bytes <= lds, "B %lld G %lld L %lld: %lld bytes", (long long)B, (long long)G, (long long)L, (long long)bytes);
          }
          // the table never takes a compute unit below the workgroups it holds without one
          const int64_t without = gat::profile_workgroups_per_cu(lds, gat::metagene_lds_bytes(B, 0, G, false));
          const int64_t with = gat::profile_workgroups_per_cu(lds, gat::metagene_lds_bytes(B, L, G, false));
          CHECK(with == without, "B %lld G %lld L %lld: %lld workgroups a compute unit, %lld without the table", (long long)B, (long long)G,
                (long long)L, (long long)with, (long long)without);
        }
  CHECK(gat::metagene_lds_features(1024, 17, lds, 90, 3) == 17 && gat::metagene_lds_features(4, 17, lds, 90, 3) == 4, "the knob and the longest");
  CHECK(gat::kMetageneThreads == 256 && gat::kMetageneWaves == 4 && gat::kMetageneMaxBins == 1024, "the constants");
}

int main() {
  const int64_t lens[] = {1, 2, 3, 7, 64, 1000, kTop};
  const int32_t body[] = {1, 2, 3, 64, 66, 1024};
  struct Flank { int32_t Bf; int64_t w; };
  std::vector<Flank> flanks;
  for (int32_t Bf : {0, 1, 33})
    for (int64_t w : {1, 3, 10}) flanks.push_back({Bf, w});
  flanks.push_back({1, (int64_t)1 << 31});
  for (int64_t len : lens)
    for (int32_t Bb : body) {
      check_edges(len, Bb);
      for (const Flank& fl : flanks)
        for (int minus = 0; minus < 2; ++minus)
          for (int64_t fs : {(int64_t)0, (int64_t)1000, kTop - len, (kTop - len) / 2}) {
            if (fs < 0 || fs + len > kTop) continue;
            check_feature({fs, fs + len, minus != 0, Bb, fl.Bf, fl.w});
          }
    }
  for (int64_t len : {5, 10, 100, 4097, 1 << 20, (1 << 30) + 7}) {
    for (int32_t Bb : {4, 7, 50, 1000}) check_edges(len, Bb);
    check_feature({12345, 12345 + len, true, 50, 20, 100});
  }
  // the header's example
  check_feature({100, 110, false, 4, 1, 10});
  {
    bool any;
    const std::vector<int64_t> plus = by_piece({100, 110, false, 4, 1, 10}, 95, 112, any), minus = by_piece({100, 110, true, 4, 1, 10}, 95, 112, any);
    CHECK(plus == (std::vector<int64_t>{5, 3, 2, 3, 2, 2}) && minus == (std::vector<int64_t>{2, 3, 2, 3, 2, 5}), "the example");
    CHECK(gat::metagene_bin(103, 100, 110, false, 4, 1, 10) == 2 && gat::metagene_bin(103, 100, 110, true, 4, 1, 10) == 3, "the example's midpoint");
  }
  check_reach();
  check_lds();
  printf("metagene_bins_check: %lld pairs (%lld by bisection), %d failed\n", g_pairs, g_long, g_failed);
  return g_failed ? 1 : 0;
}
