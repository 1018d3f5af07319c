// local_windows_check.cpp -- what k_local's launches decide on the host (gat_amd/csrc/gat_local_windows.h): the windows of a
// call against plain loops over every (track, contig, window), and the LDS sizes against each other.
// Host only: tests/test_local_windows_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_local_windows.h"

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

struct Seg { uint32_t start, end; };
using gat::LocalWindow;

// tracks[t][c]: normalized lists; bins[c]; the windows against a loop over every window of every (track, contig)
static void check_windows(const std::vector<std::vector<std::vector<Seg>>>& tracks, const std::vector<int64_t>& bins, int64_t bin_size,
                          int64_t W, int64_t base, const char* what) {
  const int32_t T = (int32_t)tracks.size(), C = (int32_t)bins.size();
  std::vector<Seg> annos((size_t)base, Seg{7u, 9u});          // (entries before anno_off[0] belong to somebody else)
  std::vector<int64_t> anno_off{base}, bin_off{0};
  for (int32_t t = 0; t < T; ++t)
    for (int32_t c = 0; c < C; ++c) {
      annos.insert(annos.end(), tracks[t][c].begin(), tracks[t][c].end());
      anno_off.push_back((int64_t)annos.size());
    }
  for (int32_t c = 0; c < C; ++c) bin_off.push_back(bin_off.back() + bins[c]);
  std::vector<LocalWindow> got;
  const bool ok = gat::local_build_windows(annos.data(), anno_off.data(), T, C, bin_size, bin_off.data(), W, got);
  CHECK(ok, "%s: refused", what);
  const int64_t total = bin_off[C], reach = (((int64_t)1 << 32) + bin_size - 1) / bin_size;
  size_t at = 0;
  for (int32_t t = 0; t < T; ++t)
    for (int32_t c = 0; c < C; ++c) {
      const std::vector<Seg>& a = tracks[t][c];
      const int64_t eff = std::min(bins[c], reach);
      for (int64_t b = 0; b < eff; b += W) {
        const int64_t nb = std::min(W, eff - b), lo = b * bin_size, hi = lo + nb * bin_size;
        int64_t first = -1, count = 0;
        for (size_t k = 0; k < a.size(); ++k)
          if ((int64_t)a[k].end > lo && (int64_t)a[k].start < hi) {
            if (first < 0) first = (int64_t)k;
            CHECK(first + count == (int64_t)k, "%s: the intervals of a window are not consecutive", what);
            ++count;
          }
        if (count == 0) continue;
        if (at >= got.size()) { CHECK(false, "%s: track %d contig %d bin %lld: window missing", what, t, c, (long long)b); return; }
        const LocalWindow& w = got[at++];
        CHECK(w.lo == lo && w.nb == nb && w.contig == c && w.K == count, "%s: track %d contig %d bin %lld: lo %lld nb %d contig %d K %d, want %lld %lld %d %lld",
              what, t, c, (long long)b, (long long)w.lo, w.nb, w.contig, w.K, (long long)lo, (long long)nb, c, (long long)count);
        CHECK(w.out == (int64_t)t * total + bin_off[c] + b, "%s: out %lld", what, (long long)w.out);
        CHECK(w.a0 == anno_off[(size_t)t * C + c] - base + first, "%s: a0 %lld, want %lld", what, (long long)w.a0,
              (long long)(anno_off[(size_t)t * C + c] - base + first));
        CHECK(w.lo < (int64_t)1 << 32 && w.nb >= 1 && w.nb <= W && w.out + w.nb <= (int64_t)T * total, "%s: a window out of range", what);
        CHECK(w.a0 >= 0 && w.a0 + w.K <= (int64_t)annos.size() - base, "%s: a slice out of range", what);
      }
    }
  CHECK(at == got.size(), "%s: %zu windows too many", what, got.size() - at);
}

static std::vector<Seg> random_normalized(std::mt19937& r, int n, uint32_t from, uint32_t span, uint32_t max_len) {
  std::vector<Seg> out;
  uint64_t x = from + r() % (span / (n + 1) + 1);
  for (int k = 0; k < n; ++k) {
    const uint64_t len = 1 + r() % max_len;
    if (x + len > (uint64_t)from + span || x + len > UINT32_MAX) break;
    out.push_back(Seg{(uint32_t)x, (uint32_t)(x + len)});
    x += len + (r() % 3 == 0 ? 0 : r() % (2 * span / (n + 1) + 1));
  }
  return out;
}

int main() {
  std::mt19937 r(12345);
  // hand-made: an interval ending on a window's first base, one starting on its last, adjacent intervals, an empty track, a
  // contig without bins, a track wholly beyond the last bin, a track that begins far into the contig
  {
    std::vector<std::vector<std::vector<Seg>>> tracks = {
        {{{5, 40}, {40, 41}, {79, 80}, {80, 120}, {500, 501}}, {{0, 50}}, {{60, 90}}},
        {{}, {}, {}},
        {{{1000, 1001}}, {}, {{0, 50}}},
    };
    for (int64_t W : {1, 4, 7, 64, 1024})
      for (int64_t base : {0, 3}) check_windows(tracks, {130, 0, 5}, 10, W, base, "hand");
  }
  // coordinates up to 2^32 - 1: bins of 2^31 and of 1, more bins than coordinates reach
  {
    std::vector<std::vector<std::vector<Seg>>> tracks = {{{{5, 6}, {0x7fffffffu, 0x80000001u}, {0xfffffffeu, 0xffffffffu}}, {{0xfffffff0u, 0xffffffffu}}}};
    for (int64_t W : {1, 2, 3, 1024}) check_windows(tracks, {2, 5}, (int64_t)1 << 31, W, 0, "far");
    check_windows(tracks, {((int64_t)1 << 32) + 10, 0}, 1, (int64_t)1 << 30, 0, "far bins of one base");
  }
  for (int round = 0; round < 400; ++round) {
    const int T = 1 + (int)(r() % 3), C = 1 + (int)(r() % 3);
    const int64_t bin_size = (int64_t[]){1, 3, 7, 50, 1000}[r() % 5], W = (int64_t[]){1, 2, 4, 5, 64, 1920}[r() % 6];
    std::vector<std::vector<std::vector<Seg>>> tracks((size_t)T);
    std::vector<int64_t> bins;
    for (int c = 0; c < C; ++c) bins.push_back(r() % 4 == 0 ? 0 : (int64_t)(r() % 700));
    for (auto& t : tracks)
      for (int c = 0; c < C; ++c)
        t.push_back(random_normalized(r, (int)(r() % 4 == 0 ? 0 : r() % 40), (uint32_t)(r() % 2000), (uint32_t)(1 + r() % (uint32_t)(bin_size * 800 + 10)),
                                      (uint32_t)(1 + r() % (uint32_t)(bin_size * 9 + 1))));
    check_windows(tracks, bins, bin_size, W, (int64_t)(r() % 5), "random");
  }
  // the LDS of a window: the widest window fits with its kilobyte to spare, the next one does not; the store variant needs less
  for (int64_t lds : {(int64_t)65536, (int64_t)160 * 1024})
    for (int64_t L : {1, 4, 1024, 2048, 8192}) {
      const int64_t W = gat::local_max_window(lds, L);
      if (W < 1) continue;
      CHECK((int64_t)gat::local_lds_bytes(W, L, false) + 1024 <= lds && (int64_t)gat::local_lds_bytes(W + 1, L, false) + 1024 > lds,
            "lds %lld L %lld: W %lld", (long long)lds, (long long)L, (long long)W);
      CHECK(gat::local_lds_bytes(W, L, true) < gat::local_lds_bytes(W, L, false) && gat::local_lds_bytes(W, L, true) % 8 == 0, "store");
    }
  CHECK(gat::local_lds_bytes(1024, 1024, false) == 64 * 1024 + 8 * 1024, "64 bytes a bin and 8 an interval");
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("local_windows_check: ok\n");
  return 0;
}
