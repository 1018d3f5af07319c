// gat_signal.h -- what a quantitative track (conservation, GC content, a ChIP signal: pieces with a value each) amounts to
// over the segments of a list, summed where the lists are (gat_list_signal, gat_sample_signal).  include/gat_mi355.h has the
// definition; gat_signal_sum.h one segment's arithmetic: two searches over the pieces' ends and at most three 32-byte records.
//
// Segment-parallel, in the arrangement of k_distance's direction 0.  A workgroup (256 threads, 4 waves) owns ONE (track,
// group) and a run of the segment lists of that group; a WAVE owns one (list, track): its lanes stride over the segments, the
// wave reduces the four words -- n, covered, hit, sum -- with shuffles and lane 0 adds them to the output, [list][track][4],
// the sum over the groups, with 64-bit integer atomic adds (zero words are skipped): a partial sum has one owner and is added
// once, integer adds commute, so neither the order in which the groups arrive nor how the lists are cut into workgroups can
// change a bit.  (The caller zeroes the output.)  The lists come in either layout (ListSet, gat_lists.h).
// LDS holds what both searches start in, the pieces' ends: all K when K <= lds_pieces (the searches then never leave the
// chip), else the last end of each of ceil(K / stride) blocks of `stride` consecutive pieces -- a search finds its block in LDS
// and ends in the records' ends in global memory, log2(stride) probes (block_search).  4 bytes a piece: the default 2 048 are
// 8 KB, eight workgroups a compute unit.
#pragma once
#include "gat_device.h"
#include "gat_lists.h"
#include "gat_signal_sum.h"

namespace gat {

constexpr int kSignalThreads = 256;
constexpr int kSignalWaves = kSignalThreads / kWave;
constexpr int kSignalWords = 4;                 // GAT_SIGNAL_WORDS: n, covered, hit, sum

struct SignalArgs {
  ListSet q;                              // the segment lists
  const SignalPiece* rec;                 // the records of every (track, group), track-major
  const int64_t* rec_off;                 // [n_tracks * n_groups + 1]
  int32_t n_tracks, n_q;
  int32_t n_groups;
  int32_t q_per_block;
  int32_t lds_pieces;                     // L: the dynamic LDS is 4 * L bytes
  unsigned long long* out;                // [n_q][n_tracks][kSignalWords], zeroed by the caller
};

__host__ __device__ inline size_t signal_lds_bytes(int64_t L) { return (size_t)L * 4; }

__global__ __launch_bounds__(kSignalThreads) void k_signal(SignalArgs A) {
  extern __shared__ uint32_t signal_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int G = A.n_groups;
  const int64_t ti = (int64_t)(blockIdx.x / (unsigned)G);
  const int g = (int)(blockIdx.x % (unsigned)G);
  const int64_t r0 = A.rec_off[blockIdx.x];
  const int K = (int)(A.rec_off[blockIdx.x + 1] - r0);
  const SignalPiece* __restrict__ R = A.rec + r0;
  const BlockTable bt = block_table(K, A.lds_pieces);
  const int stride = bt.stride, nl = bt.nl;
  for (int t = tid; t < nl; t += kSignalThreads) {
    const int64_t m = ((int64_t)t + 1) * stride - 1;
    signal_lds[t] = R[m < (int64_t)K - 1 ? m : (int64_t)K - 1].end;
  }
  __syncthreads();

  const int q0 = (int)blockIdx.y * A.q_per_block;
  const int q1 = min(q0 + A.q_per_block, A.n_q);
  for (int qi = q0 + wave; qi < q1; qi += kSignalWaves) {
    int n;
    const uint2* __restrict__ Q = list_at(A.q, qi, g, G, n);
    long long cnt = 0, covered = 0, hit = 0, sum = 0;
    for (int j = lane; j < n; j += kWave) {
      const uint2 sg = Q[j];
      if (sg.y <= sg.x) continue;
      cnt += 1;
      const SignalSum x = signal_sum(signal_lds, nl, K, stride, sg.x, sg.y, [&](int m) { return R[m].end; }, [&](int k) { return R[k]; });
      covered += (long long)x.c;
      hit += x.c != 0 ? 1 : 0;
      sum += x.w;
    }
    cnt = wave_sum_i64(cnt);
    covered = wave_sum_i64(covered);
    hit = wave_sum_i64(hit);
    sum = wave_sum_i64(sum);
    if (lane == 0 && cnt != 0) {
      unsigned long long* o = A.out + ((int64_t)qi * A.n_tracks + ti) * kSignalWords;
      atomicAdd(o + 0, (unsigned long long)cnt);
      if (covered != 0) atomicAdd(o + 1, (unsigned long long)covered);
      if (hit != 0) atomicAdd(o + 2, (unsigned long long)hit);
      if (sum != 0) atomicAdd(o + 3, (unsigned long long)sum);
    }
  }
}

}  // namespace gat
