// gat_metrics.h -- how a list of segments sits in a workspace, summed where the list is (gat_list_metrics,
// gat_sample_metrics; the numbers behind SegmentsSummary.update, gat/IO.py:353-408, which forms them with three merge-joins --
// filter, intersect, subtract -- on the host).  For a list L and the normalized pieces W of its group (sorted, disjoint, maybe
// adjacent), every segment [s, e) of L has
//
//   lo = the first piece with end > s,  hi = the last piece with start < e,  k = max(0, hi - lo + 1)
//
// and adds to 64-bit words:  n += 1;  bases += e - s;  pairs += k;  inter += |[s, e) n W|;  touched += e - s where k > 0;
// outside_pieces += 1 where k == 0, else [s < W[lo].start] + [e > W[hi].end] + the positive gaps between the pieces lo..hi.
// Two more words hold what the reference's subtract never reaches: its merge-join ends with the last piece of the
// intersection, so the segments that follow the last segment with k > 0 -- all of them with k == 0; every segment where no
// segment has k > 0 -- are missing from its result.  With M = the largest start of a segment with k > 0 (-1: none):
// tail_n += 1 and tail_bases += e - s where s > M.  For a sorted, disjoint L the eight words give the lengths and sums of the
// reference's three lists (tests/metrics_model.py proves it); for any other list they are the definition: overlapping
// segments count with their multiplicity.
//
// Segment-parallel.  A workgroup (256 threads, 4 waves) owns one group and a run of consecutive lists; a WAVE owns one
// (list, group): its lanes stride over the list, each does the two binary searches, takes `inter` and the gap count from
// the host's prefix tables (gat_metrics_tables.h), and the wave reduces the words with shuffles -- no sum crosses a wave,
// so nothing goes through LDS or an atomic.  M is a wave maximum; a second walk over the list, without searches, sums the tail.
// Lane 0 writes the eight words with plain stores: one owner per word, deterministic.
// LDS holds the pieces the searches start in: all K of the group when K <= lds_pieces (the searches then never leave the chip),
// else the last start and end of each of ceil(K / stride) blocks of `stride` consecutive pieces -- the search finds the block
// in LDS and ends in global memory, log2(stride) probes.  Lists are taken in any order: there is no sorted / unsorted route.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"

namespace gat {

constexpr int kMetricsThreads = 256;
constexpr int kMetricsWaves = kMetricsThreads / kWave;
constexpr int kMetricsWords = 8;

struct MetricsArgs {
  ListSet lists;                          // n_lists x n_groups of them, a sampler batch or the caller's
  int32_t n_lists;
  int32_t n_groups;
  int32_t lists_per_block;
  int32_t lds_pieces;                     // L: the dynamic LDS is 8 * L bytes
  // the groups' pieces and prefix tables (MetricsTables)
  const uint32_t* ws_start;
  const uint32_t* ws_end;
  const unsigned long long* ws_cum;
  const uint32_t* ws_gaps;
  const int32_t* ws_off;
  long long* out;                         // [n_lists][n_groups][kMetricsWords]
};

__host__ __device__ inline size_t metrics_lds_bytes(int64_t L) { return (size_t)L * 8; }

__global__ __launch_bounds__(kMetricsThreads) void k_metrics(MetricsArgs A) {
  extern __shared__ uint32_t met_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int g = blockIdx.x, G = A.n_groups;
  const int wb = A.ws_off[g], K = A.ws_off[g + 1] - wb;
  const uint32_t* __restrict__ gs = A.ws_start + wb;
  const uint32_t* __restrict__ ge = A.ws_end + wb;
  const unsigned long long* __restrict__ cum = A.ws_cum + wb + g;
  const uint32_t* __restrict__ gaps = A.ws_gaps + wb + g;
  const int L = A.lds_pieces;
  const BlockTable bt = block_table(K, L);
  const int stride = bt.stride, nl = bt.nl;
  uint32_t* l_s = met_lds;
  uint32_t* l_e = met_lds + L;
  for (int t = tid; t < nl; t += kMetricsThreads) {
    const int j = min(K - 1, (t + 1) * stride - 1);
    l_s[t] = gs[j];
    l_e[t] = ge[j];
  }
  __syncthreads();

  const int i0 = (int)blockIdx.y * A.lists_per_block;
  const int i1 = min(i0 + A.lists_per_block, A.n_lists);
  for (int i = i0 + wave; i < i1; i += kMetricsWaves) {
    int n;
    const uint2* __restrict__ seg = list_at(A.lists, i, g, G, n);
    long long bases = 0, pairs = 0, inter = 0, touched = 0, pieces = 0, last = -1, tail_n = 0, tail_bases = 0;
    for (int j = lane; j < n; j += kWave) {
      const uint2 sg = seg[j];
      const long long s = (long long)sg.x, e = (long long)sg.y;
      bases += e - s;
      int lo = 0, hi = -1;
      if (K > 0) {
        lo = block_search<true>(l_e, nl, K, stride, sg.x, [&](int m) { return ge[m]; });
        hi = block_search<false>(l_s, nl, K, stride, sg.y, [&](int m) { return gs[m]; }) - 1;
      }
      if (hi < lo) { pieces += 1; continue; }
      const long long w_lo = (long long)(stride == 1 ? l_s[lo] : gs[lo]), w_hi = (long long)(stride == 1 ? l_e[hi] : ge[hi]);
      last = s > last ? s : last;
      pairs += hi - lo + 1;
      touched += e - s;
      inter += (long long)(cum[hi + 1] - cum[lo]) - (s > w_lo ? s - w_lo : 0) - (w_hi > e ? w_hi - e : 0);
      pieces += (s < w_lo ? 1 : 0) + (e > w_hi ? 1 : 0) + (long long)(gaps[hi] - gaps[lo]);
    }
    last = wave_max_i64(last);
    for (int j = lane; j < n; j += kWave) {
      const uint2 sg = seg[j];
      if ((long long)sg.x > last) { tail_n += 1; tail_bases += (long long)sg.y - (long long)sg.x; }
    }
    bases = wave_sum_i64(bases);
    pairs = wave_sum_i64(pairs);
    inter = wave_sum_i64(inter);
    touched = wave_sum_i64(touched);
    pieces = wave_sum_i64(pieces);
    tail_n = wave_sum_i64(tail_n);
    tail_bases = wave_sum_i64(tail_bases);
    if (lane == 0) {
      long long* o = A.out + ((int64_t)i * G + g) * kMetricsWords;
      o[0] = (long long)n; o[1] = bases; o[2] = pairs; o[3] = inter; o[4] = touched; o[5] = pieces;
      o[6] = tail_n; o[7] = tail_bases;
    }
  }
}

}  // namespace gat
