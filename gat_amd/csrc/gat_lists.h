// gat_lists.h -- what the reductions over lists of segments (gat_coverage.h, gat_metrics.h, gat_distance.h) and their
// launches share: where list (i, g) lies and how long it is, the two-level search their kernels start in LDS, and how long a
// run of lists a workgroup takes.  Plain code for host and device -- no intrinsic, no runtime call -- so that all of it runs
// (and is checked: tests/host/lists_check.cpp) without a device.
#pragma once
#include <stdint.h>
#include <hip/hip_vector_types.h>      // uint2 (types only)

namespace gat {

// n_entities x n_groups lists.  csr == nullptr: a sampler batch -- list (i, g) at seg + i * seg_stride + c_off[g],
// n_arr[i * n_stride + n_index[g]] long; else the caller's: seg[csr[i * n_groups + g] .. csr[i * n_groups + g + 1])
struct ListSet {
  const uint2* seg;
  int64_t seg_stride;
  const int32_t* c_off;
  const int32_t* n_arr;
  int32_t n_stride;
  const int32_t* n_index;
  const int64_t* csr;
};

// list (i, g) of G groups: its segments, n of them
__host__ __device__ inline const uint2* list_at(const ListSet& S, int64_t i, int g, int G, int& n) {
  if (S.csr != nullptr) {
    const int64_t b = S.csr[i * G + g];
    n = (int)(S.csr[i * G + g + 1] - b);
    return S.seg + b;
  }
  n = S.n_arr[i * S.n_stride + S.n_index[g]];
  return S.seg + i * S.seg_stride + S.c_off[g];
}

// K ascending values searched from an LDS image of L words: all of them (stride 1) when K <= L, else the last value of each
// of nl <= L blocks of `stride` consecutive values (the last block may be short): lds[t] = value[min(K - 1, (t + 1) * stride - 1)]
struct BlockTable { int stride, nl; };
__host__ __device__ inline BlockTable block_table(int K, int L) {
  const int stride = K <= L ? 1 : (K + L - 1) / L;
  return {stride, K == 0 ? 0 : (K + stride - 1) / stride};
}

// first j in [0, K) whose value is > x (UPPER) / >= x (else), K: none.  The block is found in lds; with stride > 1 the search
// ends in the K values themselves, glob(m) the value of element m: log2(stride) probes
template <bool UPPER, class Glob>
__host__ __device__ inline int block_search(const uint32_t* lds, int nl, int K, int stride, uint32_t x, Glob glob) {
  int a = 0, b = nl;
  while (a < b) {
    const int m = (a + b) >> 1;
    const uint32_t v = lds[m];
    if (UPPER ? v > x : v >= x) b = m; else a = m + 1;
  }
  if (a == nl) return K;
  if (stride == 1) return a;
  int lo = a * stride, hi = (K < lo + stride ? K : lo + stride) - 1;       // (glob(hi) is lds[a]: it qualifies)
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    const uint32_t v = glob(m);
    if (UPPER ? v > x : v >= x) hi = m; else lo = m + 1;
  }
  return lo;
}

// The run of lists a workgroup takes, of n lists in a launch whose grid is `fixed` wide: all n, halved while the run is longer
// than 16 and the launch has fewer than `target` workgroups; at most `cap`; and within the grid's y
__host__ __device__ inline int64_t run_per_block(int64_t n, int64_t fixed, int64_t target, int64_t cap) {
  int64_t run = n;
  while (run > 16 && fixed * ((n + run - 1) / run) < target) run = (run + 1) / 2;
  run = run < n ? run : n;
  run = run < cap ? run : cap;
  run = run > 1 ? run : 1;
  const int64_t floor_y = (n + 65534) / 65535;
  return run > floor_y ? run : floor_y;
}
constexpr int64_t kNoRunCap = INT64_MAX;

// k_coverage's run of samples: the knob's where it is set (no halving), else four workgroups for each of 256 compute units;
// never so long that a 32-bit word of the window could overflow (a sample holds at most slab_stride segments)
__host__ __device__ inline int64_t coverage_run_per_block(int64_t n, int64_t n_windows, int64_t knob, int64_t slab_stride) {
  const int64_t cap32 = (int64_t)INT32_MAX / (slab_stride > 1 ? slab_stride : 1);
  return knob > 0 ? run_per_block(n, n_windows, 0, knob < cap32 ? knob : cap32) : run_per_block(n, n_windows, 1024, cap32);
}

}  // namespace gat
