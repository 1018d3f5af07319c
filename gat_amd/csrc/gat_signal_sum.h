// gat_signal_sum.h -- the arithmetic of one segment of k_signal (gat_signal.h): how many of its bases carry a value of a signal
// track, and the sum of the values over them.  A track's group is K >= 0 pieces (s_k, e_k, q_k): the intervals normalized
// (sorted, disjoint, none empty; adjacent ones allowed), q_k a signed 32-bit value with |q_k| <= 2^31 - 1.  For [s, e), e > s:
//     c = sum_k |[s, e) n [s_k, e_k)|          w = sum_k q_k * |[s, e) n [s_k, e_k)|
// in O(log K) through the prefix sums PC[k] = sum_{i<k} len_i (unsigned 64) and PW[k] = sum_{i<k} q_i * len_i (signed 64):
//     j0 = the first k with e_k > s (K: none), j1 = the first k with e_k >= e, last = j1 if (j1 < K and s_j1 < e) else j1 - 1
//     j0 > last: c = w = 0;  else c = PC[last + 1] - PC[j0], w = PW[last + 1] - PW[j0], less what piece j0 has before s and
//     piece `last` has from e on.
// A piece is one 32-byte record {start, end, q, pad, PC[k], PW[k]}: the one or two pieces a segment touches bring their
// prefix entries with them (PC[last + 1] = PC[last] + len_last), so a segment costs its searches and at most three aligned
// 32-byte reads, and there is no table of K + 1 entries beside the pieces.  With M = sum_k |q_k| * len_k < 2^63 (the host
// checks it before anything is built) every PW[k], every difference of two of them and every clip is at most M in size: no
// signed operation here leaves 64 bits.
// Plain code for host and device -- no intrinsic, no runtime call -- so that all of it runs (and is checked:
// tests/host/signal_sum_check.cpp) without a device.
#pragma once
#include <stdint.h>
#include "gat_lists.h"

namespace gat {

struct alignas(32) SignalPiece {
  uint32_t start, end;
  int32_t q;
  uint32_t pad;
  uint64_t pc;      // PC[k]: the bases of the pieces before this one
  int64_t pw;       // PW[k]: sum of q * length over the pieces before this one
};
static_assert(sizeof(SignalPiece) == 32, "one piece is one 32-byte record");

struct SignalSum {
  uint64_t c;
  int64_t w;
};

// the K records of one (track, group): piece(k, s, e, q) gives piece k.  (M < 2^63 is the caller's to have checked.)
template <class Piece>
inline void signal_fill(SignalPiece* out, int64_t K, Piece piece) {
  uint64_t pc = 0;
  int64_t pw = 0;
  for (int64_t k = 0; k < K; ++k) {
    uint32_t s, e;
    int32_t q;
    piece(k, s, e, q);
    out[k] = {s, e, q, 0u, pc, pw};
    pc += (uint64_t)(e - s);
    pw += (int64_t)q * (int64_t)(e - s);
  }
}

// q * the bases of [s, e) in the one piece r, which it overlaps
__host__ __device__ inline SignalSum signal_one_piece(const SignalPiece& r, uint32_t s, uint32_t e) {
  const uint32_t lo = r.start > s ? r.start : s, hi = r.end < e ? r.end : e;
  return {(uint64_t)(hi - lo), (int64_t)r.q * (int64_t)(hi - lo)};
}

// (c, w) of [s, e), e > s, against K pieces.  l_e[t], t < nl: the end of the last piece of block t (block_table: blocks of
// `stride` pieces; stride 1: the ends themselves); end_of(m): the end of piece m where the search leaves the table (stride >
// 1); rec(k): piece k's record.  Both searches run over the ends.  Two shortcuts that change no result: where e_j0 >= e the
// second search is not made (j1 == j0), and where last == j0 the value is q_j0 * the overlap, without a prefix entry.
template <class EndOf, class Rec>
__host__ __device__ inline SignalSum signal_sum(const uint32_t* l_e, int nl, int K, int stride, uint32_t s, uint32_t e, EndOf end_of, Rec rec) {
  const int j0 = block_search<true>(l_e, nl, K, stride, s, end_of);       // the first end beyond s
  if (j0 >= K) return {0u, 0};
  const SignalPiece a = rec(j0);
  if (a.end >= e) return a.start < e ? signal_one_piece(a, s, e) : SignalSum{0u, 0};
  // (a ends before e and beyond s: it is overlapped, and j1 > j0)
  const int j1 = block_search<false>(l_e, nl, K, stride, e, end_of);      // the first end at or beyond e
  int last = j1 - 1;
  SignalPiece b = a;
  bool have_b = last == j0;
  if (j1 < K) {
    const SignalPiece r = rec(j1);
    if (r.start < e) { last = j1; b = r; have_b = true; }
  }
  if (last == j0) return signal_one_piece(a, s, e);
  if (!have_b) b = rec(last);
  const uint64_t len_b = (uint64_t)(b.end - b.start);
  SignalSum x = {b.pc + len_b - a.pc, b.pw + (int64_t)b.q * (int64_t)len_b - a.pw};
  if (a.start < s) { x.c -= (uint64_t)(s - a.start); x.w -= (int64_t)a.q * (int64_t)(s - a.start); }
  if (b.end > e) { x.c -= (uint64_t)(b.end - e); x.w -= (int64_t)b.q * (int64_t)(b.end - e); }
  return x;
}

}  // namespace gat
