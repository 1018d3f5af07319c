// signal_sum_check.cpp -- the arithmetic of one segment of k_signal (gat_amd/csrc/gat_signal_sum.h: two searches over the
// pieces' ends, the prefix sums the records carry, at most two clips) against the definition, base by base: every layout of up
// to 4 pieces in [0, 12), every segment in [0, 14), with all ends in the search table and with blocks of 2, 3 and 4 pieces
// behind it; the two shortcuts on cases made for them; the extreme values, against 128-bit arithmetic.
// Host only: tests/test_signal_sum_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_signal_sum.h"

#include <algorithm>
#include <cstdio>
#include <vector>

static int g_failed = 0;
static long long g_cases = 0, g_layouts = 0, g_records_read = 0;

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

struct Piece {
  uint32_t s, e;
  int32_t q;
};

static std::vector<gat::SignalPiece> records(const std::vector<Piece>& p) {
  std::vector<gat::SignalPiece> r(p.size() + 1);      // (one more than is ever read: the sanitizer sees a read beyond K)
  gat::signal_fill(r.data(), (int64_t)p.size(), [&](int64_t k, uint32_t& s, uint32_t& e, int32_t& q) { s = p[(size_t)k].s; e = p[(size_t)k].e; q = p[(size_t)k].q; });
  r.resize(p.size());
  r.shrink_to_fit();
  return r;
}

// what the kernel does with a limit of L ends in LDS: the table, then signal_sum
struct Staged {
  const std::vector<gat::SignalPiece>& r;
  gat::BlockTable bt;
  std::vector<uint32_t> lds;
  Staged(const std::vector<gat::SignalPiece>& records_, int L) : r(records_), bt(gat::block_table((int)records_.size(), L)), lds((size_t)bt.nl) {
    const int K = (int)r.size();
    for (int t = 0; t < bt.nl; ++t) lds[(size_t)t] = r[(size_t)std::min(K - 1, (t + 1) * bt.stride - 1)].end;
  }
  gat::SignalSum sum(uint32_t s, uint32_t e) const {
    return gat::signal_sum(lds.data(), bt.nl, (int)r.size(), bt.stride, s, e, [&](int m) { return r.at((size_t)m).end; },
                           [&](int k) { ++g_records_read; return r.at((size_t)k); });
  }
};
static gat::SignalSum by_header(const std::vector<gat::SignalPiece>& r, int L, uint32_t s, uint32_t e) { return Staged(r, L).sum(s, e); }

// the definition, base by base
static gat::SignalSum by_base(const std::vector<Piece>& p, uint32_t s, uint32_t e) {
  gat::SignalSum x = {0u, 0};
  for (uint32_t b = s; b < e; ++b)
    for (const Piece& k : p)
      if (k.s <= b && b < k.e) { x.c += 1; x.w += k.q; }
  return x;
}

static const int32_t kValues[3][4] = {{3, -2, 5, -7}, {-4, 4, 0, 1}, {1, 1, 1, 1}};

static void check_layout(const std::vector<Piece>& base) {
  ++g_layouts;
  for (int v = 0; v < 3; ++v) {
    std::vector<Piece> p = base;
    for (size_t k = 0; k < p.size(); ++k) p[k].q = kValues[v][k];
    const std::vector<gat::SignalPiece> r = records(p);
    const Staged staged[3] = {Staged(r, 100), Staged(r, 2), Staged(r, 1)};     // every end in the table; blocks of 2; one block (of up to 4)
    for (uint32_t s = 0; s < 14; ++s)
      for (uint32_t e = s + 1; e <= 14; ++e) {
        const gat::SignalSum want = by_base(p, s, e);
        for (const Staged& st : staged) {
          const int L = (int)st.lds.size();
          const long long before = g_records_read;
          const gat::SignalSum got = st.sum(s, e);
          ++g_cases;
          CHECK(got.c == want.c && got.w == want.w, "K %zu values %d L %d [%u, %u): (%llu, %lld), by base (%llu, %lld)", p.size(), v, L, s, e,
                (unsigned long long)got.c, (long long)got.w, (unsigned long long)want.c, (long long)want.w);
          CHECK(g_records_read - before <= 3, "[%u, %u) read %lld records", s, e, g_records_read - before);
        }
      }
  }
}

// every list of up to 4 sorted, disjoint, non-empty intervals in [0, 12), adjacent ones included
static void layouts(std::vector<Piece>& p, uint32_t from) {
  check_layout(p);
  if (p.size() == 4) return;
  for (uint32_t s = from; s < 12; ++s)
    for (uint32_t e = s + 1; e <= 12; ++e) {
      p.push_back({s, e, 0});
      layouts(p, e);
      p.pop_back();
    }
}

static void shortcuts() {
  // (the first end beyond s is at or beyond e: one search, one record; the last piece is the first: no prefix entry)
  const std::vector<Piece> p = {{10, 20, 7}, {20, 30, -3}, {40, 50, 11}};
  const std::vector<gat::SignalPiece> r = records(p);
  struct { uint32_t s, e; uint64_t c; int64_t w; long long reads; } cases[] = {
      {12, 18, 6, 42, 1},       // inside one piece
      {12, 20, 8, 56, 1},       // ... to its end
      {5, 10, 0, 0, 1},         // bookended before the first piece: no hit
      {30, 40, 0, 0, 1},        // the gap, bookended on both sides
      {30, 41, 1, 11, 1},       // one base of the last piece
      {19, 21, 2, 4, 2},        // over the seam of two adjacent pieces
      {25, 35, 5, -15, 2},      // ends in the gap: the piece behind it is looked at and is not reached
      {0, 100, 30, 150, 2},     // across all pieces, behind the last
      {15, 35, 15, 5, 3},       // across two pieces into the gap: the piece behind it, then the last one reached
      {15, 45, 20, 60, 2},      // clipped at both ends, across the gap
      {50, 60, 0, 0, 0},        // behind the last piece: no record at all
  };
  for (const auto& k : cases)
    for (int L : {100, 2, 1}) {
      const long long before = g_records_read;
      const gat::SignalSum got = by_header(r, L, k.s, k.e);
      CHECK(got.c == k.c && got.w == k.w, "[%u, %u) L %d: (%llu, %lld)", k.s, k.e, L, (unsigned long long)got.c, (long long)got.w);
      CHECK(g_records_read - before == k.reads, "[%u, %u) L %d: %lld records read, %lld expected", k.s, k.e, L, g_records_read - before, k.reads);
    }
  const gat::SignalSum none = by_header(records({}), 8, 3, 9);       // K == 0
  CHECK(none.c == 0 && none.w == 0, "K == 0");
}

static void extremes() {
  const int32_t Q = INT32_MAX;
  const uint32_t TOP = UINT32_MAX, HALF = 1u << 31;
  // M = (2^31 - 1) * (2^32 - 1) < 2^63: the largest a (track, group) can be
  const std::vector<Piece> layouts_[] = {{{0, TOP, Q}}, {{0, TOP, -Q}}, {{0, HALF, Q}, {HALF, TOP, Q}}, {{0, HALF, Q}, {HALF, TOP, -Q}},
                                         {{0, 1, -Q}, {1, HALF, Q}, {HALF + 5, TOP - 1, -Q}, {TOP - 1, TOP, Q}}};
  const uint32_t at[] = {0, 1, 2, HALF - 1, HALF, HALF + 1, HALF + 5, HALF + 6, TOP - 2, TOP - 1, TOP};
  for (const auto& p : layouts_) {
    const std::vector<gat::SignalPiece> r = records(p);
    for (uint32_t s : at)
      for (uint32_t e : at) {
        if (e <= s) continue;
        __int128 c = 0, w = 0;
        for (const Piece& k : p) {
          const uint32_t lo = std::max(s, k.s), hi = std::min(e, k.e);
          if (hi > lo) { c += hi - lo; w += (__int128)k.q * (hi - lo); }
        }
        for (int L : {100, 2, 1}) {
          const gat::SignalSum got = by_header(r, L, s, e);
          ++g_cases;
          CHECK((__int128)got.c == c && (__int128)got.w == w, "extreme K %zu L %d [%u, %u): (%llu, %lld)", p.size(), L, s, e,
                (unsigned long long)got.c, (long long)got.w);
        }
      }
  }
  const gat::SignalSum whole = by_header(records(layouts_[0]), 4, 0, TOP);
  CHECK(whole.w == (int64_t)Q * (int64_t)TOP && whole.w > ((int64_t)1 << 62), "the largest sum");
}

int main() {
  static_assert(sizeof(gat::SignalPiece) == 32 && alignof(gat::SignalPiece) == 32, "one aligned 32-byte record a piece");
  std::vector<Piece> p;
  layouts(p, 0);
  shortcuts();
  extremes();
  CHECK(g_layouts > 1000, "only %lld layouts", g_layouts);
  printf("signal_sum_check: %lld layouts, %lld cases, %d failed\n", g_layouts, g_cases, g_failed);
  return g_failed ? 1 : 0;
}
