// gat_efdr.h -- the resampling-based false discovery rate read off the count matrix of a run, the FDR counterpart of step-down
// minP (gat_minp.h) and what the Annotator's "False Discovery summary" (annotator/src/app/FalseDiscoveryStats.java of the
// reference tree; Engine.computeFDR, gat/Engine.pyx:3366-3501, is its obsolete port) estimates: column i of the matrix is one
// draw from the joint null distribution of the family, so the number of rows of column i that would be called at a threshold
// is one draw of the number of false calls there.  With T, kobs and K[r][i] = T(r, row_r[i]) those of gat_minp.h,
//
//   D[r][i] = 1 if row_r[i] > mean_r else 0                       (the comparison T branches on: 1 = over-represented tail)
//   V_d(t)  = #{(r, i) : K[r][i] <= t and D[r][i] == d}            at every distinct kobs t
//   N_d[i]  = #{r : K[r][i] <= L and D[r][i] == d}                 per level L (at most kEfdrLevels of them)
//
// A sample is "significant at t" exactly when an observed value equal to it would be.  Everything is an integer; Rn, the
// prefix sums over the thresholds, the running minimum and the division stay on the host.
//
// k_efdr: one pass over a batch's rows of K (written by k_minp_rank).  One thread per sample, lanes on consecutive samples
// (coalesced 4-byte loads of a row of K and 8-byte loads of the matrix row: D is recomputed, no second rank kernel and K
// stays what gat_minp_counts reads); grid y: slabs of rows, so that few samples x many rows still fills the chip.  The sorted
// distinct thresholds of a chunk sit in LDS; an element finds the first j with thr[j] >= K by binary search and adds 1 to the
// workgroup's LDS bin [d][j] -- so bin[d][j] counts thr[j-1] < K <= thr[j], and V_d(thr[j]) is the host's prefix sum.  An
// element at or below `below` (the last threshold of the chunk in front) or above the chunk's last threshold is not counted
// by this chunk's pass.  At its end a workgroup adds its non-zero bins to the 64-bit global bins with vector atomics:
// integer adds, the result does not depend on their order.  The same lane compares K with the levels, keeps N_d[i] in
// registers across the slab's rows and adds them to the int32 arrays [level][d][S] that are carried from batch to batch
// (vector atomics too: the slabs of one column of blocks share a sample).
#pragma once
#include "gat_device.h"

namespace gat {

constexpr int kEfdrThreads = 256;
constexpr int kEfdrLevels = 8;
constexpr int kEfdrThresholdBytes = 12;        // LDS per threshold: the threshold and its two bins
constexpr int kEfdrUnroll = 4;

struct EfdrArgs {
  const int32_t* K;           // [batch row][S]
  const int64_t* counts;      // the matrix K was ranked from (MinpRankArgs::counts), for D
  int64_t row_stride;
  int32_t S, n_rows;          // n_rows: rows of this batch
  int32_t rows_per_slab;      // blockIdx.y takes the batch rows [y * rows_per_slab, (y + 1) * rows_per_slab)
  const int32_t* rows;        // per batch row: the row of the matrix
  const uint8_t* is_double;   // per row of the matrix
  const double* means;        // per row of the matrix
  const int32_t* thr;         // the chunk's thresholds, sorted ascending, distinct
  int32_t n_thr;              // >= 0 (0: only the levels are counted)
  int32_t below;              // the last threshold of the chunk in front (0 for the first chunk: K >= 1)
  unsigned long long* bins;   // [2][bins_stride], at the chunk's first threshold: d = 1 in row 0, d = 0 in row 1
  int64_t bins_stride;
  int32_t levels[kEfdrLevels];   // unused ones -1: nothing is at or below them
  int32_t n_levels;           // 0: this pass does not count levels (every chunk but the batch's first)
  int32_t* per_sample;        // [level][2][S]: N_1 in row 0, N_0 in row 1
};

__global__ __launch_bounds__(kEfdrThreads) void k_efdr(EfdrArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  int32_t* thr = reinterpret_cast<int32_t*>(lds);             // [n_thr]
  uint32_t* bin = lds + A.n_thr;                              // [2][n_thr]; a workgroup counts at most 256 x rows_per_slab < 2^32
  const int tid = threadIdx.x;
  const int n_thr = A.n_thr;
  for (int j = tid; j < n_thr; j += kEfdrThreads) { thr[j] = A.thr[j]; bin[j] = 0u; bin[n_thr + j] = 0u; }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kEfdrThreads + tid;
  const bool valid = i < (int64_t)A.S;
  const int64_t S = A.S;
  const int b0 = (int)blockIdx.y * A.rows_per_slab;
  const int b1 = b0 + A.rows_per_slab < A.n_rows ? b0 + A.rows_per_slab : A.n_rows;
  const int32_t below = A.below;
  const int32_t last = n_thr > 0 ? thr[n_thr - 1] : 0;
  int32_t n1[kEfdrLevels], n0[kEfdrLevels];
#pragma unroll
  for (int l = 0; l < kEfdrLevels; ++l) n1[l] = n0[l] = 0;
  auto load = [&](int b, int32_t& k, bool& d) {
    const int row = A.rows[b];
    const int64_t v = A.counts[(int64_t)row * A.row_stride + i];
    k = A.K[(int64_t)b * S + i];
    d = (A.is_double[row] != 0 ? __longlong_as_double(v) : (double)v) > A.means[row];
  };
  auto count = [&](int32_t k, bool d) {
    if (k > below && k <= last) {
      int lo = 0, hi = n_thr - 1;                             // first j with thr[j] >= k: there is one, k <= last
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (thr[mid] < k) lo = mid + 1; else hi = mid;
      }
      atomicAdd(&bin[(d ? 0 : n_thr) + lo], 1u);
    }
#pragma unroll
    for (int l = 0; l < kEfdrLevels; ++l) {
      const int32_t hit = k <= A.levels[l] ? 1 : 0;
      n1[l] += d ? hit : 0;
      n0[l] += d ? 0 : hit;
    }
  };
  if (valid) {
    int b = b0;
    for (; b + kEfdrUnroll <= b1; b += kEfdrUnroll) {         // the loads of four rows in flight together
      int32_t k[kEfdrUnroll];
      bool d[kEfdrUnroll];
#pragma unroll
      for (int u = 0; u < kEfdrUnroll; ++u) load(b + u, k[u], d[u]);
#pragma unroll
      for (int u = 0; u < kEfdrUnroll; ++u) count(k[u], d[u]);
    }
    for (; b < b1; ++b) {
      int32_t k;
      bool d;
      load(b, k, d);
      count(k, d);
    }
#pragma unroll
    for (int l = 0; l < kEfdrLevels; ++l) {
      if (l < A.n_levels) {
        if (n1[l] != 0) atomicAdd(&A.per_sample[((int64_t)l * 2) * S + i], n1[l]);
        if (n0[l] != 0) atomicAdd(&A.per_sample[((int64_t)l * 2 + 1) * S + i], n0[l]);
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < 2 * n_thr; j += kEfdrThreads) {
    const uint32_t c = bin[j];
    if (c != 0u) atomicAdd(&A.bins[j < n_thr ? (int64_t)j : A.bins_stride + (int64_t)(j - n_thr)], (unsigned long long)c);
  }
}

}  // namespace gat
