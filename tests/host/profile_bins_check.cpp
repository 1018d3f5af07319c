// profile_bins_check.cpp -- the arithmetic of one (segment, anchor) pair of k_profile (gat_amd/csrc/gat_profile_bins.h) against
// the definition: o = sigma * (x - a), x in the window iff -R <= o < R, bin floor((o + R) / w), base by base; where a segment
// is too long for that (R = 2^31), against the interval of bases every bin covers.  Also the anchors a segment is walked
// over, and the LDS the launches size.
// Host only: tests/test_profile_bins_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_profile_bins.h"

#include <algorithm>
#include <cstdio>
#include <vector>

static int g_failed = 0;
static long long g_pairs = 0;

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

// the definition, base by base
static std::vector<int64_t> by_base(int64_t s, int64_t e, int64_t a, bool minus, int64_t w, int64_t H) {
  std::vector<int64_t> v((size_t)(2 * H), 0);
  const int64_t R = H * w;
  for (int64_t x = s; x < e; ++x) {
    const int64_t o = minus ? a - x : x - a;
    if (o < -R || o >= R) continue;
    v[(size_t)((o + R) / w)] += 1;
  }
  return v;
}
// bin b as the bases it covers, intersected with [s, e)
static std::vector<int64_t> by_bin(int64_t s, int64_t e, int64_t a, bool minus, int64_t w, int64_t H) {
  std::vector<int64_t> v((size_t)(2 * H), 0);
  const int64_t R = H * w;
  for (int64_t b = 0; b < 2 * H; ++b) {
    const int64_t lo = minus ? a + R - (b + 1) * w + 1 : a - R + b * w;
    v[(size_t)b] = std::max<int64_t>(0, std::min(e, lo + w) - std::max(s, lo));
  }
  return v;
}
// what profile_piece says, spread over the bins as the kernel's vector has it
static std::vector<int64_t> by_piece(int64_t s, int64_t e, int64_t a, bool minus, int64_t w, int64_t H, bool& any) {
  std::vector<int64_t> v((size_t)(2 * H), 0);
  gat::ProfilePiece p = {-1, -1, 0u, 0u};
  any = gat::profile_piece(s, e, a, minus, w, H * w, p);
  if (!any) return v;
  CHECK(0 <= p.fb && p.fb <= p.lb && p.lb < 2 * H, "bins [%d, %d] of %lld", p.fb, p.lb, (long long)(2 * H));
  if (p.fb < 0 || p.lb >= 2 * H || p.lb < p.fb) return v;
  CHECK(p.first >= 1 && (int64_t)p.first <= w && (int64_t)p.last <= w && (p.lb > p.fb) == (p.last > 0), "first %u last %u w %lld", p.first,
        p.last, (long long)w);
  v[(size_t)p.fb] += p.first;
  if (p.lb > p.fb) v[(size_t)p.lb] += p.last;
  for (int32_t b = p.fb + 1; b < p.lb; ++b) v[(size_t)b] += w;
  return v;
}

static void check_pair(int64_t s, int64_t e, int64_t a, bool minus, int64_t w, int64_t H) {
  ++g_pairs;
  const int64_t R = H * w;
  bool any = false;
  const std::vector<int64_t> got = by_piece(s, e, a, minus, w, H, any);
  const std::vector<int64_t> want = e - s <= 4096 ? by_base(s, e, a, minus, w, H) : by_bin(s, e, a, minus, w, H);
  int64_t total = 0;
  for (size_t b = 0; b < want.size(); ++b) {
    total += want[b];
    CHECK(got[b] == want[b], "[%lld, %lld) anchor %lld%c w %lld H %lld bin %zu: %lld, not %lld", (long long)s, (long long)e, (long long)a,
          minus ? '-' : '+', (long long)w, (long long)H, b, (long long)got[b], (long long)want[b]);
  }
  CHECK(any == (total > 0), "[%lld, %lld) anchor %lld%c w %lld H %lld: piece %d, bases %lld", (long long)s, (long long)e, (long long)a,
        minus ? '-' : '+', (long long)w, (long long)H, (int)any, (long long)total);
  // an anchor that holds a base of the segment is one the kernel's walk reaches
  if (total > 0)
    CHECK((int64_t)gat::profile_reach_lo(s, R) <= a && a < gat::profile_reach_hi(e, R), "[%lld, %lld) anchor %lld R %lld: not walked",
          (long long)s, (long long)e, (long long)a, (long long)R);
  if (e - s <= 4096 && e - s > 1) {                   // (the two references agree where both can be had)
    const std::vector<int64_t> other = by_bin(s, e, a, minus, w, H);
    CHECK(other == want, "[%lld, %lld) anchor %lld: the references differ", (long long)s, (long long)e, (long long)a);
  }
}

// every segment [s, e) with both ends from `ends`, within [0, 2^32 - 1]
static void check_ends(std::vector<int64_t> ends, int64_t a, int64_t w, int64_t H) {
  std::sort(ends.begin(), ends.end());
  ends.erase(std::unique(ends.begin(), ends.end()), ends.end());
  for (int64_t s : ends)
    for (int64_t e : ends) {
      if (s < 0 || e <= s || e > (int64_t)UINT32_MAX) continue;
      for (int minus = 0; minus < 2; ++minus) check_pair(s, e, a, minus != 0, w, H);
    }
}

int main() {
  // the worked example of include/gat_mi355.h
  {
    bool any;
    CHECK((by_piece(85, 112, 100, false, 10, 2, any) == std::vector<int64_t>{5, 10, 10, 2}), "the plus example");
    CHECK((by_piece(85, 112, 100, true, 10, 2, any) == std::vector<int64_t>{1, 10, 10, 6}), "the minus example");
    CHECK((by_piece(98, 99, 100, false, 10, 2, any) == std::vector<int64_t>{0, 1, 0, 0}), "the midpoint, plus");
    CHECK((by_piece(98, 99, 100, true, 10, 2, any) == std::vector<int64_t>{0, 0, 1, 0}), "the midpoint, minus");
    CHECK(gat::profile_midpoint(85, 112) == 98 && gat::profile_midpoint(7, 8) == 7 && gat::profile_midpoint(7, 9) == 8, "midpoint");
  }
  // s, e around the window's edges, both strands, w in {1, 3, 10}, H in {1, 2, 33}; the anchor and the bin edges beside them
  for (int64_t w : {1, 3, 10})
    for (int64_t H : {1, 2, 33})
      for (int64_t a : {1000ll, 331ll, 5ll}) {
        const int64_t R = H * w;
        std::vector<int64_t> ends;
        for (int64_t d = -1; d <= 1; ++d) {
          ends.push_back(a - R + d);
          ends.push_back(a + R + d);
          ends.push_back(a + d);
          ends.push_back(a - w + d);
          ends.push_back(a + w + d);
        }
        ends.push_back(a + R + 2);
        ends.push_back(0);
        check_ends(ends, a, w, H);
      }
  // a in {0, 1, 2^32 - 1} with R = 2^31: a - R is negative, a + R passes 2^32
  const int64_t top = (int64_t)UINT32_MAX, R = (int64_t)1 << 31;
  for (int64_t H : {1, 2, 512})
    for (int64_t a : {(int64_t)0, (int64_t)1, top}) {
      const int64_t w = R / H;
      std::vector<int64_t> ends;
      for (int64_t d = -2; d <= 2; ++d) {
        ends.push_back(a - R + d);
        ends.push_back(a + R + d);
        ends.push_back(a + d);
        ends.push_back(a - w + d);
        ends.push_back(a + w + d);
        ends.push_back(top + d);
        ends.push_back(d);
      }
      check_ends(ends, a, w, H);
    }
  CHECK(g_pairs > 5000, "only %lld pairs checked", g_pairs);

  // the LDS of a launch: what profile_lds_anchors grants fits beside the bins, is never more than asked for or needed
  for (int64_t lds : {65536ll, 163840ll})
    for (int64_t B : {2ll, 100ll, 1024ll})
      for (int64_t G : {1ll, 3ll, 24ll, 4000ll, 100000ll})
        for (int64_t knob : {0ll, 4ll, 1024ll, 1ll << 40})
          for (int64_t longest : {1ll, 5ll, 2000ll, 1ll << 31}) {
            const int64_t L = gat::profile_lds_anchors(knob, longest, lds, B, G);
            CHECK(L >= 0 && L <= knob && L <= longest, "L %lld of knob %lld, longest %lld", (long long)L, (long long)knob, (long long)longest);
            CHECK(L == 0 || gat::profile_lds_bytes(B, L, G, false) + 1024 <= lds, "L %lld B %lld G %lld: %lld bytes of %lld", (long long)L,
                  (long long)B, (long long)G, (long long)gat::profile_lds_bytes(B, L, G, false), (long long)lds);
            CHECK(gat::profile_lds_bytes(B, L, G, true) <= gat::profile_lds_bytes(B, L, G, false), "STORE takes more than FOLD");
            // the table costs the compute unit no workgroup
            CHECK(gat::profile_workgroups_per_cu(lds, gat::profile_lds_bytes(B, L, G, false)) ==
                      gat::profile_workgroups_per_cu(lds, gat::profile_lds_bytes(B, 0, G, false)),
                  "L %lld B %lld G %lld: the table takes a workgroup off the compute unit", (long long)L, (long long)B, (long long)G);
          }
  CHECK(gat::profile_lds_bytes(1024, 0, 1, false) == 1024 * 36 + 4 * 1024 * 8, "the bins of B = 1024");
  CHECK(gat::profile_workgroups_per_cu(163840, gat::profile_lds_bytes(1024, 0, 24, false)) == 2 &&
            gat::profile_workgroups_per_cu(163840, gat::profile_lds_bytes(100, 0, 24, false)) == 8, "workgroups a compute unit");
  CHECK(gat::profile_lds_anchors(1024, 2000, 163840, 1024, 24) == 117 && gat::profile_lds_anchors(1024, 83, 163840, 100, 24) == 83, "defaults");

  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("profile_bins_check: %lld pairs ok\n", g_pairs);
  return 0;
}
