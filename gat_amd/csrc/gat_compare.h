// gat_compare.h -- gat-compare.py's null distribution of a fold-change difference (scripts/gat-compare.py:214-231 of the
// reference), formed where the sampled counts are: for a pair (data1, data2) of result rows and every sample i
//
//   fc1 = obs_a / (a[ia][i] + pseudo_count);  fc1 = fc1 + 0.0001
//   fc2 = obs_b / (b[ib][i] + pseudo_count);  fc2 = fc2 + 0.0001
//   row[p][i] = log(fc1 / fc2) + delta
//
// in this order of IEEE operations (explicit round-to-nearest intrinsics, no contraction).  k_compare_rows writes the rows
// of a batch of pairs into a scratch block; k_null_stats (gat_stats.h) then reads that block like a count matrix of doubles
// with vals[p] = delta.  Up to the logarithm the row is numpy's bit for bit; the device's log and numpy's are each good to
// about an ulp and are not the same function ("k_compare_rows").
//
// One workgroup per pair.  A lane handles two neighbouring samples per step: a 16-byte load from each source row where the
// row starts on a 16-byte boundary (rows of an odd number of samples start on one only every other row: those take two
// 8-byte loads, the wave still covers one contiguous kilobyte), and one 16-byte store -- the scratch rows have an even
// stride, so every one of them is aligned.  Each source row is read once.  IEEE throughout: a zero denominator gives inf,
// inf / inf gives nan, as numpy does; how many elements of the row are not finite is counted per pair (the host recomputes
// such a pair with numpy).
#pragma once
#include "gat_device.h"

namespace gat {

constexpr int kCompareThreads = 256;

struct CompareArgs {
  const double* a;            // [rows of a][S]
  const double* b;            // [rows of b][S]; may be a
  int32_t S, n_pairs;
  const int32_t* ia;          // per pair: row of a, row of b
  const int32_t* ib;
  const double* obs_a;        // per pair
  const double* obs_b;
  const double* delta;
  double pseudo_count;
  double* rows;               // [pair][row_stride] scratch; row_stride even, the block 16-byte aligned
  int64_t row_stride;
  uint32_t* n_nonfinite;      // per pair
};

__device__ __forceinline__ double compare_value(double a, double b, double obs_a, double obs_b, double pseudo_count, double delta) {
#pragma clang fp contract(off)
  double fc1 = __ddiv_rn(obs_a, __dadd_rn(a, pseudo_count));
  fc1 = __dadd_rn(fc1, 0.0001);
  double fc2 = __ddiv_rn(obs_b, __dadd_rn(b, pseudo_count));
  fc2 = __dadd_rn(fc2, 0.0001);
  return __dadd_rn(log(__ddiv_rn(fc1, fc2)), delta);
}

__device__ __forceinline__ double2 compare_load2(const double* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const double2*>(p);
  return make_double2(p[0], p[1]);
}

__global__ __launch_bounds__(kCompareThreads) void k_compare_rows(CompareArgs A) {
  __shared__ uint32_t bad_total;
  const int p = blockIdx.x;
  if (p >= A.n_pairs) return;
  const int tid = threadIdx.x;
  const double* __restrict__ ra = A.a + (int64_t)A.ia[p] * A.S;
  const double* __restrict__ rb = A.b + (int64_t)A.ib[p] * A.S;
  double* __restrict__ out = A.rows + (int64_t)p * A.row_stride;
  const double obs_a = A.obs_a[p], obs_b = A.obs_b[p], delta = A.delta[p], pc = A.pseudo_count;
  const bool al_a = (reinterpret_cast<uintptr_t>(ra) & 15) == 0, al_b = (reinterpret_cast<uintptr_t>(rb) & 15) == 0;
  if (tid == 0) bad_total = 0;
  __syncthreads();
  uint32_t bad = 0;
  const int n2 = A.S >> 1;
  for (int j = tid; j < n2; j += kCompareThreads) {
    const double2 x = compare_load2(ra + 2 * j, al_a), y = compare_load2(rb + 2 * j, al_b);
    double2 r;
    r.x = compare_value(x.x, y.x, obs_a, obs_b, pc, delta);
    r.y = compare_value(x.y, y.y, obs_a, obs_b, pc, delta);
    bad += (isfinite(r.x) ? 0u : 1u) + (isfinite(r.y) ? 0u : 1u);
    *reinterpret_cast<double2*>(out + 2 * j) = r;
  }
  if ((A.S & 1) && tid == (n2 & (kCompareThreads - 1))) {      // the odd last sample: the lane behind the last pair's
    const int i = A.S - 1;
    const double r = compare_value(ra[i], rb[i], obs_a, obs_b, pc, delta);
    bad += isfinite(r) ? 0u : 1u;
    out[i] = r;
  }
  bad = wave_total_u32(bad);
  if ((tid & (kWave - 1)) == 0 && bad) atomicAdd(&bad_total, bad);
  __syncthreads();
  if (tid == 0) A.n_nonfinite[p] = bad_total;
}

}  // namespace gat
