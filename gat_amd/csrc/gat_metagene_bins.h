// gat_metagene_bins.h -- the arithmetic of one (segment, feature) pair of k_metagene (gat_metagene.h), and what its launches
// decide on the host.  A feature is (fs, fe, sigma): 0 <= fs < fe <= 2^32 - 1, len = fe - fs, and a strand sigma in {+1, -1}.
// With Bb = body_bins >= 1, Bf = flank_bins >= 0, w = flank_bin_size in [1, 2^31], F = Bf * w <= 2^31 and B = 2 Bf + Bb bins,
// the window of the feature is the bases [fs - F, fe + F).  The ORIENTED offset of base x is u = x - (fs - F) for a plus
// feature and u = (fe + F - 1) - x for a minus one -- the mirror x -> fs + fe - 1 - x maps the window onto itself, so, unlike
// k_profile's minus window, nothing shifts by a base -- and 0 <= u < 2 F + len:
//
//   upstream    u < F               bin = floor(u / w)                                      in [0, Bf)
//   body        F <= u < F + len    bin = Bf + floor((u - F) * Bb / len)                     the product stays below 2^42
//   downstream  F + len <= u        bin = Bf + Bb + floor((u - F - len) / w)
//
// Body bin k holds the body offsets [ceil(k * len / Bb), ceil((k + 1) * len / Bb)): with len < Bb some hold none.  Everything
// is 64-bit: fs - F goes below 0 and fe + F passes 2^32.  Plain code for host and device -- no intrinsic, no runtime call -- so
// that all of it runs (and is checked: tests/host/metagene_bins_check.cpp) without a device.
#pragma once
#include <stdint.h>
#include "gat_profile_bins.h"

namespace gat {

constexpr int kMetageneThreads = kProfileThreads;      // k_metagene has k_profile's ownership and its LDS layout
constexpr int kMetageneWaves = kProfileWaves;
constexpr int kMetageneMaxBins = 1024;                 // GAT_METAGENE_MAX_BINS

// What the bases of a piece put into the bins of one flank: the bins [fb, lb] (of the B, not of the flank); `first` bases into
// fb; when lb > fb, `last` bases into lb and w into every bin between them.  fb < 0: nothing.
struct MetageneFlank {
  int32_t fb, lb;
  uint32_t first, last;
};
// The edge of a body bin while the bins are stepped: ceil(k * len / Bb) = t + (a > 0), with t = floor(k * len / Bb) and
// a = (k * len) mod Bb; q = len / Bb and r = len mod Bb carry it from k to k + 1 without a division.
struct MetageneEdge {
  int64_t t;
  uint32_t a, q, r, bb;
};
// ... and into the body: the body offsets [oa, ob), which lie in the body bins [fb, lb] (0-based within the body; add Bf).
// `edge` is the upper edge of bin fb.  fb < 0: nothing.
struct MetageneBody {
  int32_t fb, lb;
  int64_t oa, ob;
  MetageneEdge edge;
};
struct MetagenePiece {
  MetageneFlank up, down;
  MetageneBody body;
};

// the edge between body bins k - 1 and k, 0 <= k <= Bb (k * r < 2^20: the two divisions are 32-bit)
__host__ __device__ inline MetageneEdge metagene_edge_at(int64_t len, int32_t Bb, int32_t k) {
  MetageneEdge E;
  E.bb = (uint32_t)Bb;
  E.q = (uint32_t)len / E.bb;
  E.r = (uint32_t)len - E.q * E.bb;
  const uint32_t kr = (uint32_t)k * E.r, c = kr / E.bb;
  E.t = (int64_t)k * E.q + c;
  E.a = kr - c * E.bb;
  return E;
}
__host__ __device__ inline int64_t metagene_edge_value(const MetageneEdge& E) { return E.t + (E.a > 0u ? 1 : 0); }
__host__ __device__ inline void metagene_edge_next(MetageneEdge& E) {
  E.t += E.q;
  E.a += E.r;
  if (E.a >= E.bb) { E.a -= E.bb; E.t += 1; }
}

// the flank offsets [a, b), 0 <= a < b <= F, into the flank whose first bin is `base` (a and b - 1 are below 2^31 and w is at
// most 2^31: the divisions are 32-bit)
__host__ __device__ inline void metagene_flank(int64_t a, int64_t b, int64_t w, int32_t base, MetageneFlank& f) {
  const uint32_t fb = (uint32_t)a / (uint32_t)w, lb = (uint32_t)(b - 1) / (uint32_t)w;
  f.fb = base + (int32_t)fb;
  f.lb = base + (int32_t)lb;
  if (fb == lb) {
    f.first = (uint32_t)(b - a);
    f.last = 0u;
  } else {
    f.first = (uint32_t)((int64_t)(fb + 1) * w - a);
    f.last = (uint32_t)(b - (int64_t)lb * w);
  }
}

// [s, e), e > s, against the feature (fs, fe, minus): false where no base of it lies in the window.  The clip is exact; the
// oriented offsets of the piece are [us, ue), ascending in x for a plus feature and descending for a minus one, cut at F and
// F + len into the three regions.  The body costs one 64-bit division where the piece stays in one bin (the edge above it says
// so) and two where it does not.
__host__ __device__ inline bool metagene_piece(int64_t s, int64_t e, int64_t fs, int64_t fe, bool minus, int32_t Bb, int32_t Bf, int64_t w,
                                               MetagenePiece& p) {
  const int64_t F = (int64_t)Bf * w, len = fe - fs, lo = fs - F, hi = fe + F;      // the window's bases [lo, hi)
  const int64_t cs = s > lo ? s : lo, ce = e < hi ? e : hi;
  if (ce <= cs) return false;
  const int64_t us = minus ? hi - ce : cs - lo, ue = minus ? hi - cs : ce - lo;
  p.up.fb = p.down.fb = p.body.fb = -1;
  if (us < F) metagene_flank(us, ue < F ? ue : F, w, 0, p.up);
  if (ue > F + len) metagene_flank((us > F + len ? us : F + len) - (F + len), ue - (F + len), w, Bf + Bb, p.down);
  const int64_t oa = (us > F ? us : F) - F, ob = (ue < F + len ? ue : F + len) - F;
  if (ob > oa) {
    MetageneBody& b = p.body;
    b.oa = oa;
    b.ob = ob;
    b.fb = (int32_t)((uint64_t)oa * (uint64_t)Bb / (uint64_t)len);
    b.edge = metagene_edge_at(len, Bb, b.fb + 1);
    b.lb = ob <= metagene_edge_value(b.edge) ? b.fb : (int32_t)((uint64_t)(ob - 1) * (uint64_t)Bb / (uint64_t)len);
  }
  return true;
}

// the bin of the one base x (GAT_METAGENE_MIDPOINTS counts the midpoint of a segment: profile_midpoint), -1 outside the window:
// one bin, one division
__host__ __device__ inline int32_t metagene_bin(int64_t x, int64_t fs, int64_t fe, bool minus, int32_t Bb, int32_t Bf, int64_t w) {
  const int64_t F = (int64_t)Bf * w, len = fe - fs, lo = fs - F, hi = fe + F;
  if (x < lo || x >= hi) return -1;
  const int64_t u = minus ? hi - 1 - x : x - lo;
  if (u < F) return (int32_t)((uint32_t)u / (uint32_t)w);
  if (u >= F + len) return Bf + Bb + (int32_t)((uint32_t)(u - F - len) / (uint32_t)w);
  return Bf + (int32_t)((uint64_t)(u - F) * (uint64_t)Bb / (uint64_t)len);
}

// Reach.  Within a (track, group) the features ascend by (fs, fe, minus) and may overlap and nest, so their ends do not
// ascend; pm[k] = max(fe[0 .. k]) does.  The features a segment [s, e) can meet -- fs[k] - F < e and fe[k] + F > s -- lie in
// the index range [first k with pm[k] + F > s, first k with fs[k] >= e + F); inside it, those with fe[k] + F > s.
// metagene_reach_key: the search is for the first k with pm[k] > key; false: every k qualifies (s - F < 0), start at 0.
__host__ __device__ inline bool metagene_reach_key(int64_t s, int64_t F, uint32_t& key) {
  if (s < F) return false;
  key = (uint32_t)(s - F);
  return true;
}
__host__ __device__ inline int64_t metagene_reach_hi(int64_t e, int64_t F) { return e + F; }
__host__ __device__ inline bool metagene_reaches(int64_t s, int64_t fe, int64_t F) { return fe + F > s; }

// dynamic LDS of a launch, k_profile's layout with pm in the table:
// (sum[B], sumsq[B], obs[B] | n_pos[B], n_less[B], n_eq[B])  part[waves][B], diff[waves][B]  tab[G][L]
__host__ __device__ inline int64_t metagene_lds_bytes(int64_t B, int64_t L, int64_t n_groups, bool store) {
  return profile_lds_bytes(B, L, n_groups, store);
}
// The entries of pm of a (track, group) the search finds in LDS: at most `knob`, no more than the longest (track, group) holds,
// and what the LDS of a compute unit takes beside the bins without costing a workgroup (profile_lds_anchors has the rule and
// the measurement behind it) -- 0: the searches run in global memory
__host__ __device__ inline int64_t metagene_lds_features(int64_t knob, int64_t longest, int64_t lds, int64_t B, int64_t n_groups) {
  return profile_lds_anchors(knob, longest, lds, B, n_groups);
}

}  // namespace gat
