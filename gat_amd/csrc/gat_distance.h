// gat_distance.h -- how far the intervals of one list lie from the nearest interval of another, summed where the lists are
// (gat_list_distances, gat_sample_distances; the two counters the reference's to-do list names and never built,
// doc/contents.rst:78-81: "Closest distance of segment to annotation" / "of annotation to segment").
//
// T is a normalized list of K >= 1 intervals (sorted, disjoint, none empty; adjacent ones allowed), Q = [s, e) a query with
// e > s.  j = the first index with T[j].end > s (K: none).  T[j].start < e: they share a base, d = 0.  Else d = the smaller of
// T[j].start - e + 1 (j < K) and s - T[j - 1].end + 1 (j > 0): the convention of `bedtools closest -d` -- bookended
// intervals are at distance 1.  Per (Q list, T list) four 64-bit words: n (queries with e > s where K > 0), sum (of d),
// near (d <= max_distance), none (queries with e > s where K == 0).  Queries with e <= s are skipped.  Q lists are taken in
// any order and may overlap themselves.
//
// Segment-parallel.  A workgroup (256 threads, 4 waves) owns ONE T list -- (entity, group) -- and a run of the Q lists of the
// same group; a WAVE owns one (Q list, T list): its lanes stride over the queries, each does ONE binary search and at most two
// more reads, the wave reduces the words with shuffles and lane 0 adds them to the output -- [list][track][4], the sum over
// the groups -- with 64-bit integer atomic adds: a partial sum has one owner and is added once, integer adds commute, so the
// order in which the groups' partial sums arrive cannot change a bit.  (The caller zeroes the output.)
// Which side is staged is the direction, and nothing else differs: segment-to-annotation stages the track's contig, shared by
// every list the workgroup takes; annotation-to-segment stages the sample's list and streams the tracks -- the arrangement of
// k_count_swap.  Both sides come in either layout (ListSet, gat_lists.h): a sampler batch, or a caller's CSR.
// LDS holds what the search starts in: all K of the staged list when K <= lds_pieces (the search then never leaves the chip),
// else the last end of each of ceil(K / stride) blocks of `stride` consecutive intervals -- the search finds the block in LDS
// and ends in global memory, log2(stride) probes (block_search, gat_lists.h).
#pragma once
#include "gat_device.h"
#include "gat_lists.h"

namespace gat {

constexpr int kDistanceThreads = 256;
constexpr int kDistanceWaves = kDistanceThreads / kWave;
constexpr int kDistanceWords = 4;

struct DistanceArgs {
  ListSet t, q;                           // the staged side (normalized lists) and the streamed side (queries)
  int32_t n_t, n_q;                       // entities on either side
  int32_t n_groups;
  int32_t q_per_block;
  int32_t lds_pieces;                     // L: the dynamic LDS is 8 * L bytes
  int64_t out_stride_t, out_stride_q;     // the words of (t, q) are at out + (t * out_stride_t + q * out_stride_q) * kDistanceWords
  unsigned long long max_distance;
  unsigned long long* out;                // [n_lists][n_tracks][kDistanceWords], zeroed by the caller
};

__host__ __device__ inline size_t distance_lds_bytes(int64_t L) { return (size_t)L * 8; }

// d of the query [s, e), e > s, against the K >= 1 intervals T.  l_e[t], t < nl: the end of the last interval of block t
// (blocks of `stride` intervals; stride 1: the intervals themselves, their starts in l_s)
__device__ __forceinline__ long long distance_of(const uint32_t* l_s, const uint32_t* l_e, int nl, const uint2* __restrict__ T, int K,
                                                 int stride, uint32_t s, uint32_t e) {
  const int j = block_search<true>(l_e, nl, K, stride, s, [&](int m) { return T[m].y; });      // the first end beyond s
  long long d = LLONG_MAX;
  if (j < K) {
    const long long ts = (long long)(stride == 1 ? l_s[j] : T[j].x);
    if (ts < (long long)e) return 0;
    d = ts - (long long)e + 1;
  }
  if (j > 0) {
    const long long te = (long long)(stride == 1 ? l_e[j - 1] : T[j - 1].y);      // (<= s: j is the first end beyond s)
    const long long left = (long long)s - te + 1;
    d = left < d ? left : d;
  }
  return d;
}

__global__ __launch_bounds__(kDistanceThreads) void k_distance(DistanceArgs A) {
  extern __shared__ uint32_t dist_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int G = A.n_groups;
  const int64_t ti = (int64_t)(blockIdx.x / (unsigned)G);
  const int g = (int)(blockIdx.x % (unsigned)G);
  int K;
  const uint2* __restrict__ T = list_at(A.t, ti, g, G, K);
  const int L = A.lds_pieces;
  const BlockTable bt = block_table(K, L);
  const int stride = bt.stride, nl = bt.nl;
  uint32_t* l_s = dist_lds;
  uint32_t* l_e = dist_lds + L;
  for (int t = tid; t < nl; t += kDistanceThreads) {
    const uint2 v = T[min(K - 1, (t + 1) * stride - 1)];
    l_s[t] = v.x;
    l_e[t] = v.y;
  }
  __syncthreads();

  const int q0 = (int)blockIdx.y * A.q_per_block;
  const int q1 = min(q0 + A.q_per_block, A.n_q);
  for (int qi = q0 + wave; qi < q1; qi += kDistanceWaves) {
    int n;
    const uint2* __restrict__ Q = list_at(A.q, qi, g, G, n);
    long long cnt = 0, sum = 0, near = 0;
    for (int j = lane; j < n; j += kWave) {
      const uint2 sg = Q[j];
      if (sg.y <= sg.x) continue;
      cnt += 1;
      if (K > 0) {
        const long long d = distance_of(l_s, l_e, nl, T, K, stride, sg.x, sg.y);
        sum += d;
        near += (unsigned long long)d <= A.max_distance ? 1 : 0;
      }
    }
    cnt = wave_sum_i64(cnt);
    sum = wave_sum_i64(sum);
    near = wave_sum_i64(near);
    if (lane == 0 && cnt != 0) {
      unsigned long long* o = A.out + (ti * A.out_stride_t + (int64_t)qi * A.out_stride_q) * kDistanceWords;
      if (K > 0) {
        atomicAdd(o + 0, (unsigned long long)cnt);
        if (sum != 0) atomicAdd(o + 1, (unsigned long long)sum);
        if (near != 0) atomicAdd(o + 2, (unsigned long long)near);
      } else {
        atomicAdd(o + 3, (unsigned long long)cnt);
      }
    }
  }
}

}  // namespace gat
