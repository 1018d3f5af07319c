// pairs_tiles_check.cpp -- what k_pairs' launches decide on the host and the index arithmetic host and device share
// (gat_amd/csrc/gat_pairs_tiles.h) against plain loops: the order of the pairs, the tiles of a call, which slots of a tile are
// pairs, and the LDS a tile takes.
// Host only: tests/test_pairs_tiles_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_pairs_tiles.h"

#include <cstdio>
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

// k(i, j) counts the pairs in their order: a bijection onto [0, P)
static void check_order(int64_t T) {
  int64_t n = 0;
  for (int64_t i = 0; i < T; ++i)
    for (int64_t j = i; j < T; ++j, ++n) CHECK(gat::pairs_index(i, j, T) == n, "T %lld: k(%lld, %lld) = %lld, the loop says %lld", (long long)T, (long long)i, (long long)j, (long long)gat::pairs_index(i, j, T), (long long)n);
  CHECK(gat::pairs_count(T) == n, "T %lld: P %lld, the loop says %lld", (long long)T, (long long)gat::pairs_count(T), (long long)n);
}

// every pair belongs to exactly one slot of one tile, and every slot that is a pair is the pair its place says
static void check_tiles(int64_t T) {
  const int64_t P = gat::pairs_count(T), nb = gat::pairs_blocks(T), n_tiles = gat::pairs_tiles(T);
  CHECK(nb == (T + 63) / 64 && n_tiles == nb * (nb + 1) / 2, "T %lld: %lld blocks, %lld tiles", (long long)T, (long long)nb, (long long)n_tiles);
  std::vector<int> owners((size_t)P, 0);
  int64_t t = 0;
  for (int64_t bi = 0; bi < nb; ++bi)
    for (int64_t bj = bi; bj < nb; ++bj, ++t) {
      int I = -1, J = -1;
      gat::pairs_tile_at(t, nb, I, J);
      CHECK(I == bi && J == bj, "T %lld: tile %lld is (%d, %d), the loop says (%lld, %lld)", (long long)T, (long long)t, I, J, (long long)bi, (long long)bj);
      for (int a = 0; a < gat::kPairsBlock; ++a)
        for (int b = 0; b < gat::kPairsBlock; ++b) {
          const int64_t i = bi * 64 + a, j = bj * 64 + b, k = gat::pairs_slot((int)bi, (int)bj, a, b, T);
          const bool is_pair = i < T && j < T && i <= j;
          CHECK((k >= 0) == is_pair, "T %lld: slot (%d, %d) of tile (%lld, %lld): %lld", (long long)T, a, b, (long long)bi, (long long)bj, (long long)k);
          if (k < 0 || !is_pair) continue;
          CHECK(k < P && k == gat::pairs_index(i, j, T), "T %lld: slot (%d, %d) of tile (%lld, %lld): %lld", (long long)T, a, b, (long long)bi, (long long)bj, (long long)k);
          if (k < P) owners[(size_t)k] += 1;
        }
    }
  CHECK(t == n_tiles, "T %lld: %lld tiles walked, %lld counted", (long long)T, (long long)t, (long long)n_tiles);
  for (int64_t k = 0; k < P; ++k) CHECK(owners[(size_t)k] == 1, "T %lld: pair %lld has %d slots", (long long)T, (long long)k, owners[(size_t)k]);
}

// the first level of the searches fits beside the counts, whatever the knob and the number of groups
static void check_lds() {
  for (int64_t G : {1, 2, 3, 24, 32, 33, 1000, 100000})
    for (int64_t knob : {-5, 0, 1, 4, 32, 2048, 1 << 30}) {
      const int64_t L = gat::pairs_lds_pieces(knob, G), bytes = gat::pairs_lds_bytes(L, G);
      CHECK(L >= 0 && L <= (knob > 0 ? knob : 0), "G %lld, knob %lld: L %lld", (long long)G, (long long)knob, (long long)L);
      CHECK(bytes == 16384 + G * L * 128 * 4 && bytes <= 32 * 1024, "G %lld, knob %lld: %lld bytes", (long long)G, (long long)knob, (long long)bytes);
      // as many as fit: one more per (group, track) would not
      if (L < knob) CHECK(gat::pairs_lds_bytes(L + 1, G) > 32 * 1024, "G %lld, knob %lld: L %lld leaves room", (long long)G, (long long)knob, (long long)L);
    }
  CHECK(gat::kPairsTileSlots == gat::kPairsSlotsPerThread * gat::kPairsThreads, "a thread's slots");
  CHECK(gat::pairs_count(gat::kPairsMaxTracks) == 2098176, "P at the cap: %lld", (long long)gat::pairs_count(gat::kPairsMaxTracks));
}

int main() {
  for (int64_t T : {0, 1, 2, 63, 64, 65, 128, 130, 2048}) {
    check_order(T);
    check_tiles(T);
  }
  check_lds();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("pairs_tiles_check: ok\n");
  return 0;
}
