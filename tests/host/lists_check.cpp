// lists_check.cpp -- what the list reductions share (gat_amd/csrc/gat_lists.h): the two-level search against a linear scan, the
// block table's invariants, list_at in both layouts, and the run-per-workgroup rule against the three expressions it replaced.
// Host only: tests/test_lists_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; exit
// status 0 = every check held, else the failed checks are on stderr.
#include "gat_lists.h"

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

using gat::BlockTable;
using gat::ListSet;

// ---- block_table, block_search

static void check_block_table(int K, int L) {
  const BlockTable bt = gat::block_table(K, L);
  CHECK(bt.nl <= L, "K %d L %d: nl %d", K, L, bt.nl);
  CHECK(bt.stride >= 1 && (bt.stride == 1) == (K <= L), "K %d L %d: stride %d", K, L, bt.stride);
  if (K == 0) CHECK(bt.nl == 0, "K 0 L %d: nl %d", L, bt.nl);
  else CHECK((int64_t)bt.nl * bt.stride >= K && K > (int64_t)(bt.nl - 1) * bt.stride, "K %d L %d: stride %d nl %d", K, L, bt.stride, bt.nl);
}

template <bool UPPER>
static int linear(const std::vector<uint32_t>& v, uint32_t x) {
  for (size_t j = 0; j < v.size(); ++j)
    if (UPPER ? v[j] > x : v[j] >= x) return (int)j;
  return (int)v.size();
}

// the K ascending values `value` searched through an LDS image of at most L words, built as the kernels build it
static void check_search(const std::vector<uint32_t>& value, int L, const char* what) {
  const int K = (int)value.size();
  const BlockTable bt = gat::block_table(K, L);
  if (bt.nl > L || (K > 0 && bt.nl < 1)) return;      // (check_block_table has said so)
  std::vector<uint32_t> lds((size_t)bt.nl);           // exactly nl words: a probe beyond them is the sanitizer's
  for (int t = 0; t < bt.nl; ++t) lds[(size_t)t] = value[(size_t)std::min(K - 1, (t + 1) * bt.stride - 1)];
  int probes = 0, bad_probe = 0;
  auto glob = [&](int m) {
    ++probes;
    if (m < 0 || m >= K) { ++bad_probe; return 0u; }
    return value[(size_t)m];
  };
  std::vector<uint32_t> queries{0u, UINT32_MAX};
  for (uint32_t v : value) { queries.push_back(v - 1u); queries.push_back(v); queries.push_back(v + 1u); }
  std::sort(queries.begin(), queries.end());
  queries.erase(std::unique(queries.begin(), queries.end()), queries.end());
  for (uint32_t x : queries) {
    const int up = gat::block_search<true>(lds.data(), bt.nl, K, bt.stride, x, glob);
    const int lw = gat::block_search<false>(lds.data(), bt.nl, K, bt.stride, x, glob);
    const int want_up = linear<true>(value, x), want_lw = linear<false>(value, x);
    CHECK(up == want_up, "%s K %d L %d stride %d: first > %u is %d, want %d", what, K, L, bt.stride, x, up, want_up);
    CHECK(lw == want_lw, "%s K %d L %d stride %d: first >= %u is %d, want %d", what, K, L, bt.stride, x, lw, want_lw);
  }
  CHECK(bad_probe == 0, "%s K %d L %d: %d probes outside [0, K)", what, K, L, bad_probe);
  if (bt.stride == 1) CHECK(probes == 0, "%s K %d L %d: %d probes of the values with all of them in the image", what, K, L, probes);
}

static void check_searches(int K, int L, std::mt19937& rng) {
  check_block_table(K, L);
  // pieces, ascending and disjoint, about a third of the neighbours adjacent (an end equals the next start): their starts,
  // their ends, and -- values that repeat within one array -- starts and ends merged
  std::vector<uint32_t> starts, ends, both;
  uint32_t pos = 1u + rng() % 5u;
  for (int j = 0; j < K; ++j) {
    const uint32_t len = 1u + rng() % 4u;
    starts.push_back(pos);
    ends.push_back(pos + len);
    pos += len + (rng() % 3u == 0 ? 0u : 1u + rng() % 3u);
  }
  for (int j = 0; j < K; ++j) both.push_back(j % 2 == 0 ? starts[(size_t)(j / 2)] : ends[(size_t)(j / 2)]);
  std::sort(both.begin(), both.end());
  for (int j = 2; j + 1 < K; j += 5) both[(size_t)j] = both[(size_t)j + 1];      // (and runs of equal values for certain)
  std::sort(both.begin(), both.end());
  check_search(starts, L, "starts");
  check_search(ends, L, "ends");
  check_search(both, L, "repeats");
  if (K > 0) {                                        // the ends of the range of values
    std::vector<uint32_t> edge((size_t)K, UINT32_MAX);
    for (int j = 0; j < K / 2; ++j) edge[(size_t)j] = 0u;
    check_search(edge, L, "0 and 2^32 - 1");
  }
}

// ---- list_at

static void check_list_at() {
  // a batch of 2 samples x 3 groups on a slab of 10 slots a sample; the lengths of group g at n_index[g] of 4 a sample
  // (not the identity: an isochore problem's lengths are indexed by contig, its offsets by position)
  std::vector<uint2> slab(20);
  for (uint32_t k = 0; k < 20; ++k) slab[k] = make_uint2(100u + k, 200u + k);
  const int32_t c_off[3] = {0, 4, 7}, n_index[3] = {2, 0, 3};
  const int32_t n_arr[8] = {3, -1, 4, 2, 1, -1, 0, 3};
  ListSet S = {};
  S.seg = slab.data(); S.seg_stride = 10; S.c_off = c_off; S.n_arr = n_arr; S.n_stride = 4; S.n_index = n_index;
  const int want_n[2][3] = {{4, 3, 2}, {0, 1, 3}};
  for (int i = 0; i < 2; ++i)
    for (int g = 0; g < 3; ++g) {
      int n = -7;
      const uint2* p = gat::list_at(S, i, g, 3, n);
      CHECK(p == slab.data() + i * 10 + c_off[g] && n == want_n[i][g], "slab list (%d, %d): at %lld, %d long", i, g, (long long)(p - slab.data()), n);
      if (n > 0) CHECK(p[n - 1].x == 100u + (uint32_t)(i * 10 + c_off[g] + n - 1), "slab list (%d, %d): last segment", i, g);
    }
  // the caller's lists: 2 entities x 3 groups, some empty
  const int64_t csr[7] = {0, 2, 2, 5, 9, 9, 12};
  std::vector<uint2> seg(12);
  for (uint32_t k = 0; k < 12; ++k) seg[k] = make_uint2(k, k + 1u);
  ListSet Cs = {};
  Cs.seg = seg.data(); Cs.csr = csr;
  for (int i = 0; i < 2; ++i)
    for (int g = 0; g < 3; ++g) {
      int n = -7;
      const uint2* p = gat::list_at(Cs, i, g, 3, n);
      CHECK(p == seg.data() + csr[i * 3 + g] && n == (int)(csr[i * 3 + g + 1] - csr[i * 3 + g]), "CSR list (%d, %d): at %lld, %d long", i, g,
            (long long)(p - seg.data()), n);
    }
  // 64-bit arithmetic: sample 2^20 of a slab of 2^12 slots a sample lies beyond 2^31 elements (only the address is formed)
  {
    const int32_t one_off[1] = {5}, one_index[1] = {0};
    std::vector<int32_t> lens((size_t)1 << 20, 0);
    lens.back() = 9;
    ListSet B = {};
    B.seg = slab.data(); B.seg_stride = 4096; B.c_off = one_off; B.n_arr = lens.data(); B.n_stride = 1; B.n_index = one_index;
    int n = -7;
    const int64_t i = ((int64_t)1 << 20) - 1;
    const uintptr_t p = (uintptr_t)gat::list_at(B, i, 0, 1, n), want = (uintptr_t)slab.data() + (uintptr_t)((i * 4096 + 5) * 8);
    CHECK(p == want && n == 9, "slab list beyond 2^31 elements: %d long", n);
  }
}

// ---- run_per_block: the three expressions as the launches had them

static int64_t metrics_lpb(int64_t n_lists, int64_t n_groups) {
  int64_t lpb = n_lists;
  while (lpb > 16 && n_groups * ((n_lists + lpb - 1) / lpb) < 2048) lpb = (lpb + 1) / 2;
  return std::max<int64_t>(std::max<int64_t>(1, std::min(lpb, n_lists)), (n_lists + 65534) / 65535);
}
static int64_t distance_qpb(int64_t n_q, int64_t n_t, int64_t n_groups) {
  int64_t qpb = n_q;
  while (qpb > 16 && n_t * n_groups * ((n_q + qpb - 1) / qpb) < 2048) qpb = (qpb + 1) / 2;
  return std::max<int64_t>(std::max<int64_t>(1, std::min(qpb, n_q)), (n_q + 65534) / 65535);
}
static int64_t coverage_spb(int64_t nb, int64_t n_windows, int64_t knob, int64_t slab_stride) {
  int64_t spb = knob > 0 ? knob : nb;
  if (knob <= 0)
    while (spb > 16 && n_windows * ((nb + spb - 1) / spb) < 1024) spb = (spb + 1) / 2;
  spb = std::max<int64_t>(1, std::min<int64_t>(std::min(spb, nb), (int64_t)INT32_MAX / std::max<int64_t>(1, slab_stride)));
  return std::max(spb, (nb + 65534) / 65535);
}

static void check_run_per_block() {
  std::vector<int64_t> ns, fixed;
  for (int64_t n = 1; n <= 300; ++n) ns.push_back(n);
  for (int64_t n = 301; n <= 70000; n += 211) ns.push_back(n);
  for (int64_t n : {16, 17, 32767, 32768, 65534, 65535, 65536, 65537, 69999, 70000}) ns.push_back(n);
  for (int64_t p = 1; p <= 4096; p *= 2)
    for (int64_t f : {p - 1, p, p + 1})
      if (f >= 1) fixed.push_back(f);
  const int64_t strides[] = {1, 1000, ((int64_t)1 << 31) - 1}, knobs[] = {-1, 0, 1, 5, 16, 17, 4096, 100000};
  for (int64_t n : ns)
    for (int64_t f : fixed) {
      const int64_t got = gat::run_per_block(n, f, 2048, gat::kNoRunCap);
      CHECK(got == metrics_lpb(n, f), "metrics: %lld lists x %lld groups: %lld, was %lld", (long long)n, (long long)f, (long long)got, (long long)metrics_lpb(n, f));
      CHECK(got >= 1 && (n + got - 1) / got <= 65535, "%lld lists in runs of %lld: beyond the grid's y", (long long)n, (long long)got);
      // (the distance launch is `n_t * n_groups` wide: the same product either way it is split)
      const int64_t got_d = gat::run_per_block(n, f * 3, 2048, gat::kNoRunCap);
      CHECK(got_d == distance_qpb(n, f, 3), "distances: %lld x (%lld x 3): %lld, was %lld", (long long)n, (long long)f, (long long)got_d, (long long)distance_qpb(n, f, 3));
      for (int64_t stride : strides)
        for (int64_t knob : knobs) {
          const int64_t got_c = gat::coverage_run_per_block(n, f, knob, stride), was = coverage_spb(n, f, knob, stride);
          CHECK(got_c == was, "coverage: %lld samples x %lld windows, knob %lld, slab stride %lld: %lld, was %lld", (long long)n, (long long)f,
                (long long)knob, (long long)stride, (long long)got_c, (long long)was);
        }
    }
}

int main() {
  std::mt19937 rng(20261019u);
  const int Ls[] = {1, 2, 3, 7, 8, 64};
  for (int K = 0; K <= 70; ++K)
    for (int L : Ls) check_searches(K, L, rng);
  check_searches(2049, 2048, rng);
  check_searches(4096, 2048, rng);
  check_searches(4097, 2048, rng);
  check_list_at();
  check_run_per_block();
  if (g_failed) fprintf(stderr, "%d checks failed\n", g_failed);
  else printf("lists_check: all checks held\n");
  return g_failed ? 1 : 0;
}
