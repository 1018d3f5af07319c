// reldist_bins_check.cpp -- the arithmetic of one (segment, flanking points) pair of k_reldist and the area statistic of a
// histogram (gat_amd/csrc/gat_reldist_bins.h) against the definition in unsigned __int128: bin = min(B - 1, floor(2 d B / gap)),
// area = floor(D 10^6 / (n B B)).  Also the midpoint, and the LDS the launches size.
// Host only: tests/test_reldist_bins_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_reldist_bins.h"

#include <algorithm>
#include <cstdio>
#include <vector>

typedef unsigned __int128 u128;

static int g_failed = 0;
static long long g_bins = 0, g_areas = 0;

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

static const int kBins[] = {1, 2, 3, 50, 1024};

// the definition of the bin
static int bin_by_definition(uint32_t m, uint32_t lo, uint32_t hi, int B) {
  const u128 below = (u128)m - lo, above = (u128)hi - m, d = below < above ? below : above, gap = (u128)hi - lo;
  const u128 b = 2 * d * (u128)B / gap;
  return b < (u128)(B - 1) ? (int)b : B - 1;
}
static void check_bin(uint32_t m, uint32_t lo, uint32_t hi) {
  for (int B : kBins) {
    const int got = gat::reldist_bin(m, lo, hi, B), want = bin_by_definition(m, lo, hi, B);
    CHECK(got == want && got >= 0 && got < B, "m %u in [%u, %u) B %d: bin %d, the definition has %d", m, lo, hi, B, got, want);
    g_bins += 1;
  }
}

// the definition of the area; D is checked against the terms on the way
static void check_area(const std::vector<uint64_t>& hist) {
  const int B = (int)hist.size();
  u128 n = 0, C = 0, D = 0;
  for (uint64_t v : hist) n += v;
  uint64_t D64 = 0, C64 = 0;
  for (int b = 0; b < B; ++b) {
    C += hist[(size_t)b];
    C64 += hist[(size_t)b];
    const u128 x = (u128)B * C, y = (u128)(b + 1) * n, term = x > y ? x - y : y - x;
    const uint64_t got = gat::reldist_area_term(C64, (uint64_t)n, b, B);
    CHECK((u128)got == term, "term of bin %d of %d", b, B);
    D += term;
    D64 += got;
  }
  const u128 M = n * (u128)B * (u128)B;
  const u128 want = n == 0 ? 0 : D * (u128)gat::kReldistAreaScale / M;
  const uint64_t got = gat::reldist_area(D64, (uint64_t)n, B);
  CHECK((u128)D64 == D && D <= M, "D of %d bins, n %llu", B, (unsigned long long)n);
  CHECK((u128)got == want && got <= gat::kReldistAreaScale, "area of %d bins, n %llu: %llu, the definition has %llu", B,
        (unsigned long long)n, (unsigned long long)got, (unsigned long long)want);
  g_areas += 1;
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random() {          // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

int main() {
  const uint32_t TOP = 0xFFFFFFFFu;
  // every small gap, every m in it, at the bottom and at the top of the coordinate range
  for (uint32_t gap = 1; gap <= 40; ++gap)
    for (uint32_t k = 0; k < gap; ++k) {
      check_bin(k, 0u, gap);
      check_bin(1000u + k, 1000u, 1000u + gap);
      check_bin(TOP - gap + k, TOP - gap, TOP);
    }
  // the widest gap: positions at 0 and 2^32 - 1
  for (uint32_t m : {0u, 1u, 2u, 0x3FFFFFFFu, 0x40000000u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xC0000000u, TOP - 2, TOP - 1})
    check_bin(m, 0u, TOP);
  for (int k = 0; k < 200000; ++k) {      // random flanks of any width: both divisions
    const uint32_t a = (uint32_t)next_random(), b = (uint32_t)next_random();
    if (a == b) continue;
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    check_bin(lo + (uint32_t)(next_random() % (hi - lo)), lo, hi);
    const uint32_t narrow = 1u + (uint32_t)(next_random() % (1u << 22));
    if (lo <= TOP - narrow) check_bin(lo + (uint32_t)(next_random() % narrow), lo, lo + narrow);
  }
  // the midpoint stays below the end and fits with its successor
  for (uint32_t s : {0u, 1u, 7u, TOP - 2, TOP - 1})
    for (uint32_t len : {1u, 2u, 3u, 1000u, TOP})
      if (len <= TOP - s) {
        const uint32_t m = gat::reldist_midpoint(s, s + len);
        CHECK(m == s + len / 2 && m >= s && m < s + len && m <= TOP - 1, "midpoint of [%u, %u)", s, s + len);
      }

  // the area: random histograms, all the mass in the first and in the last bin, and the largest list
  for (int B : kBins) {
    for (int k = 0; k < 200; ++k) {
      std::vector<uint64_t> hist((size_t)B);
      const uint64_t cap = 1ull << (next_random() % 21);
      for (auto& v : hist) v = next_random() % 3 ? next_random() % cap : 0;      // (at most 1024 * 2^20 < 2^31 in all)
      check_area(hist);
    }
    for (uint64_t n : {1ull, 9ull, (1ull << 31) - 1}) {
      std::vector<uint64_t> first((size_t)B, 0), last((size_t)B, 0);
      first[0] = n;
      last[(size_t)B - 1] = n;
      check_area(first);
      check_area(last);
    }
    check_area(std::vector<uint64_t>((size_t)B, 0));
  }
  {
    const uint64_t n = (1ull << 31) - 1;
    std::vector<uint64_t> even(1024, n / 1024), middle(1024, 0);
    even[1023] += n - 1024 * (n / 1024);
    middle[511] = n - 5;
    middle[512] = 5;
    check_area(even);
    check_area(middle);
    CHECK(gat::reldist_area(n * 1024 * 1024, n, 1024) == gat::kReldistAreaScale, "D == M");
  }

  // the LDS of a launch: the table never costs a workgroup, and fits
  for (int64_t lds : {65536ll, 163840ll})
    for (int B : kBins)
      for (int64_t G : {1ll, 3ll, 25ll, 400ll})
        for (int64_t knob : {0ll, 4ll, 1024ll, 1ll << 20})
          for (int64_t longest : {0ll, 1ll, 5ll, 100000ll}) {
            const int64_t L = gat::reldist_lds_points(knob, longest, lds, B, G);
            CHECK(L >= 0 && L <= knob && L <= longest, "L %lld of knob %lld, longest %lld", (long long)L, (long long)knob, (long long)longest);
            const int64_t bare = gat::reldist_lds_bytes(B, 0, G, false), with = gat::reldist_lds_bytes(B, L, G, false);
            CHECK(with == bare + G * L * 4 && with <= lds && gat::reldist_lds_bytes(B, L, G, true) < with, "bytes at B %d, L %lld, G %lld", B,
                  (long long)L, (long long)G);
            const int64_t n0 = std::min<int64_t>(8, lds / (bare + 1024)), n1 = std::min<int64_t>(8, lds / (with + 1024));
            CHECK(n1 == n0, "workgroups %lld -> %lld at B %d, L %lld, G %lld", (long long)n0, (long long)n1, B, (long long)L, (long long)G);
          }

  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("reldist_bins_check: %lld bins, %lld areas: every check held\n", g_bins, g_areas);
  return 0;
}
