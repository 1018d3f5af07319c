// gat_samplers.h -- the samplers there are (gat_problem_desc::sampler), one entry each: what the host code asks about a
// sampler it asks here.  Plain host code: no runtime call (checked without a device: tests/host/samplers_check.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gat_mi355.h"

struct SamplerInfo {
  int32_t id;            // GAT_SAMPLER_*: its index in kSamplers
  const char* name;      // the Python class (gat_amd/engine.py), as the messages name it
  bool wave_per_unit;    // its kernel is a wave per work unit with its stream in LDS (k_shift, k_permute, k_permute_local, k_brute_force,
                         // k_circular, k_universe: no k_rng + k_place in front) -- per-unit streams only, no reference-stream mode
  bool draws_lengths;    // it draws a segment's length from the unit's histogram: only such a sampler is bound by nbuckets
};

inline constexpr SamplerInfo kSamplers[] = {
    {GAT_SAMPLER_ANNOTATOR, "SamplerAnnotator", false, true},
    {GAT_SAMPLER_SEGMENTS, "SamplerSegments", false, true},
    {GAT_SAMPLER_SHIFT, "SamplerShift", true, false},
    {GAT_SAMPLER_GLOBAL_PERMUTATION, "SamplerGlobalPermutation", true, false},
    {GAT_SAMPLER_LOCAL_PERMUTATION, "SamplerLocalPermutation", true, false},
    {GAT_SAMPLER_BRUTE_FORCE, "SamplerBruteForce", true, true},
    {GAT_SAMPLER_CIRCULAR, "SamplerCircular", true, false},
    {GAT_SAMPLER_UNIVERSE, "SamplerUniverse", true, false},
};
constexpr int32_t kNumSamplers = (int32_t)(sizeof(kSamplers) / sizeof(kSamplers[0]));

constexpr bool samplers_in_id_order() {
  for (int32_t i = 0; i < kNumSamplers; ++i)
    if (kSamplers[i].id != i) return false;
  return true;
}
static_assert(samplers_in_id_order(), "kSamplers[i] is the entry of sampler id i");

// the entry of sampler s, nullptr for an id there is no sampler of
constexpr const SamplerInfo* sampler_info(int32_t s) { return s >= 0 && s < kNumSamplers ? &kSamplers[s] : nullptr; }
