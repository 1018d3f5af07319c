// metrics_tables_check.cpp -- the host side of k_metrics (gat_amd/csrc/gat_metrics_tables.h): the prefix tables against their
// definitions in plain loops, and the argument checks.  Host only: tests/test_metrics_tables_host.py compiles it with the
// address and undefined-behaviour sanitizers and runs it; exit status 0 = every check held, else the failed checks are on stderr.
#include "gat_metrics_tables.h"

#include <random>

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

// n pieces, ascending and disjoint, about a third of the neighbours adjacent
static std::vector<gat_segment> make_pieces(int n, uint32_t first, std::mt19937& rng) {
  std::vector<gat_segment> w((size_t)n);
  uint32_t pos = first;
  for (int j = 0; j < n; ++j) {
    const uint32_t len = 1u + rng() % 50u;
    w[(size_t)j] = {pos, pos + len};
    pos += len + (rng() % 3u == 0 ? 0u : 1u + rng() % 20u);
  }
  return w;
}

static void check_tables(const std::vector<std::vector<gat_segment>>& groups, int64_t lead) {
  // the CSR form, with `lead` unused pieces in front (ws_off[0] > 0)
  std::vector<gat_segment> ws((size_t)lead, gat_segment{7u, 3u});
  std::vector<int64_t> off{lead};
  for (const auto& g : groups) {
    ws.insert(ws.end(), g.begin(), g.end());
    off.push_back((int64_t)ws.size());
  }
  MetricsTables T;
  std::string err;
  const int rc = metrics_build_tables(ws.data(), off.data(), (int64_t)groups.size(), T, err);
  CHECK(rc == GAT_OK, "rc %d: %s", rc, err.c_str());
  if (rc) return;
  const size_t G = groups.size(), total = ws.size() - (size_t)lead;
  CHECK(T.off.size() == G + 1 && T.start.size() == total && T.end.size() == total && T.cum.size() == total + G && T.gaps.size() == total + G,
        "sizes %zu %zu %zu %zu %zu", T.off.size(), T.start.size(), T.end.size(), T.cum.size(), T.gaps.size());
  for (size_t g = 0; g < G; ++g) {
    const auto& w = groups[g];
    const size_t b = (size_t)T.off[g], K = w.size();
    CHECK((size_t)T.off[g + 1] - b == K, "group %zu: %d pieces", g, T.off[g + 1] - T.off[g]);
    for (size_t j = 0; j <= K; ++j) {
      unsigned long long cum = 0;
      uint32_t gaps = 0;
      for (size_t i = 0; i < j; ++i) cum += w[i].end - w[i].start;                          // the pieces below j
      for (size_t i = 1; i <= j && i < K; ++i) gaps += w[i].start > w[i - 1].end ? 1u : 0u;    // the positive gaps among 1..j
      CHECK(T.cum[b + g + j] == cum, "group %zu cum[%zu] = %llu, want %llu", g, j, T.cum[b + g + j], cum);
      if (j < K) {
        CHECK(T.gaps[b + g + j] == gaps, "group %zu gaps[%zu] = %u, want %u", g, j, T.gaps[b + g + j], gaps);
        CHECK(T.start[b + j] == w[j].start && T.end[b + j] == w[j].end, "group %zu piece %zu", g, j);
      }
    }
  }
}

static void check_refused(const std::vector<gat_segment>& ws, const std::vector<int64_t>& off, const char* what) {
  MetricsTables T;
  std::string err;
  const int rc = metrics_build_tables(ws.empty() ? nullptr : ws.data(), off.data(), (int64_t)off.size() - 1, T, err);
  CHECK(rc == GAT_ERR_ARG && !err.empty(), "%s: rc %d '%s'", what, rc, err.c_str());
}

int main() {
  std::mt19937 rng(20261018u);
  check_tables({}, 0);
  check_tables({{}}, 0);
  check_tables({{}, {}, {}}, 2);
  check_tables({{{0u, 1u}}}, 0);
  check_tables({{{0u, 10u}, {10u, 20u}, {25u, 30u}}, {}, {{2147483000u, 2147483647u}}}, 3);
  check_tables({{{0u, 4294967295u}}}, 0);                        // (a piece of 2^32 - 1 bases: the sums are 64-bit)
  for (int round = 0; round < 40; ++round) {
    std::vector<std::vector<gat_segment>> groups;
    const int G = 1 + (int)(rng() % 6u);
    for (int g = 0; g < G; ++g) {
      const int sizes[] = {0, 1, 2, 63, 64, 65, 300};
      groups.push_back(make_pieces(sizes[rng() % 7u], rng() % 1000u, rng));
    }
    check_tables(groups, (int64_t)(rng() % 3u));
  }
  check_refused({{0u, 5u}}, {-1, 0}, "ws_off[0] < 0");
  check_refused({{0u, 5u}, {7u, 9u}}, {0, 2, 1}, "ws_off decreases");
  check_refused({{0u, 5u}, {4u, 9u}}, {0, 2}, "overlapping pieces");
  check_refused({{6u, 9u}, {0u, 5u}}, {0, 2}, "unsorted pieces");
  check_refused({{0u, 5u}, {7u, 7u}}, {0, 2}, "an empty piece");
  check_refused({{5u, 0u}}, {0, 1}, "a piece that ends before it starts");
  check_refused({}, {0, 1}, "NULL workspace with pieces");
  {                                                             // the same pieces in two groups are fine: groups are independent
    const std::vector<gat_segment> w{{0u, 5u}, {5u, 9u}};
    check_tables({w, w}, 0);
  }
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  else printf("metrics_tables_check: all checks held\n");
  return g_failed ? 1 : 0;
}
