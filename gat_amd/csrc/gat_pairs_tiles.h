// gat_pairs_tiles.h -- what the launches of k_pairs (gat_pairs.h) decide on the host, and the index arithmetic host and device
// share: the order of the pairs, the tiles of a call, which slots of a tile are pairs, and the LDS a tile takes.  Plain code
// -- no intrinsic, no runtime call -- so that all of it runs (and is checked: tests/host/pairs_tiles_check.cpp) without a
// device.
//
// T tracks give P = T (T + 1) / 2 pairs (i, j), i <= j, in the order (0,0), (0,1), .., (0,T-1), (1,1), ..:
//   k(i, j) = i * T - i (i - 1) / 2 + (j - i)
// The tracks are cut into nb = ceil(T / 64) blocks of 64; a tile is a pair of blocks (I, J), I <= J, in the same order.  Slot
// (a, b) of tile (I, J), a, b < 64, is the pair (i, j) = (64 I + a, 64 J + b); it exists when j < T and i <= j (i <= j < T).
// Every pair belongs to exactly one slot: that of tile (i / 64, j / 64).
#pragma once
#include <stdint.h>

namespace gat {

constexpr int kPairsBlock = 64;                 // tracks of a block: a lane each
constexpr int kPairsThreads = 256;
constexpr int kPairsWaves = kPairsThreads / kPairsBlock;
constexpr int kPairsMaxTracks = 2048;           // the contract's cap: 2 098 176 pairs
constexpr int kPairsTileSlots = kPairsBlock * kPairsBlock;
constexpr int kPairsSlotsPerThread = kPairsTileSlots / kPairsThreads;
constexpr int kPairsTileTracks = 2 * kPairsBlock;        // block I's and block J's
constexpr int64_t kPairsCountBytes = (int64_t)kPairsTileSlots * 4;      // a sample's 32-bit counts of a tile
constexpr int64_t kPairsTableBudget = 16 * 1024;                        // ... beside them, the searches' first level: 32 KB a workgroup

__host__ __device__ inline int64_t pairs_count(int64_t T) { return T * (T + 1) / 2; }
__host__ __device__ inline int64_t pairs_index(int64_t i, int64_t j, int64_t T) { return i * T - i * (i - 1) / 2 + (j - i); }
__host__ __device__ inline int64_t pairs_blocks(int64_t T) { return (T + kPairsBlock - 1) / kPairsBlock; }
__host__ __device__ inline int64_t pairs_tiles(int64_t T) { return pairs_count(pairs_blocks(T)); }

// tile t of nb blocks: its blocks (I, J), I <= J
__host__ __device__ inline void pairs_tile_at(int64_t t, int64_t nb, int& I, int& J) {
  int64_t i = 0;
  while (t >= nb - i) { t -= nb - i; ++i; }
  I = (int)i;
  J = (int)(i + t);
}
// slot (a, b) of tile (I, J) of T tracks: the index of its pair, -1 where it is none
__host__ __device__ inline int64_t pairs_slot(int I, int J, int a, int b, int64_t T) {
  const int64_t i = (int64_t)I * kPairsBlock + a, j = (int64_t)J * kPairsBlock + b;
  return j < T && i <= j ? pairs_index(i, j, T) : -1;
}

// The first level of a track's search in LDS: per (group, track of the tile) L ends, as many as the budget holds beside the
// counts -- at most `knob`, 0: the searches start in global memory
__host__ __device__ inline int64_t pairs_lds_pieces(int64_t knob, int64_t n_groups) {
  const int64_t fit = kPairsTableBudget / ((n_groups > 1 ? n_groups : 1) * kPairsTileTracks * 4);
  const int64_t L = knob < fit ? knob : fit;
  return L > 0 ? L : 0;
}
__host__ __device__ inline int64_t pairs_lds_bytes(int64_t L, int64_t n_groups) {
  return kPairsCountBytes + n_groups * L * kPairsTileTracks * 4;
}

}  // namespace gat
