// samplers_check.cpp -- the table of samplers (gat_amd/csrc/gat_samplers.h) and the three predicates that look things up in it
// (gat_host.h: sampler_is_known, sampler_runs_wave_per_unit; gat_prep_units.h: sampler_draws_lengths) against the values the
// predicates had as chains of comparisons, written out here.  Host only: tests/test_samplers_host.py compiles it with the
// address and undefined-behaviour sanitizers and runs it; exit status 0 = every check held, else the failed checks are on stderr.
#include "gat_host.h"
#include "gat_prep_units.h"

#include <climits>

thread_local std::string g_last_error;      // (gat_host.h declares it; the library's is gat_mi355.hip's)

static int g_failed = 0;

#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++g_failed;                                \
      fprintf(stderr, "FAIL %s: ", #cond);       \
      fprintf(stderr, __VA_ARGS__);              \
      fprintf(stderr, "\n");                     \
    }                                            \
  } while (0)

int main() {
  // id: known, a wave per unit, draws lengths -- as the three chains had it
  static const struct { int32_t id; const char* name; bool known, wave, lengths; } want[] = {
      {0, "SamplerAnnotator", true, false, true},        {1, "SamplerSegments", true, false, true},
      {2, "SamplerShift", true, true, false},            {3, "SamplerGlobalPermutation", true, true, false},
      {4, "SamplerLocalPermutation", true, true, false}, {5, "SamplerBruteForce", true, true, true},
      {6, "SamplerCircular", true, true, false},         {7, "SamplerUniverse", true, true, false},
      {-1, nullptr, false, false, false},                {8, nullptr, false, false, false},
      {INT32_MAX, nullptr, false, false, false},         {INT32_MIN, nullptr, false, false, false},
      {9, nullptr, false, false, false},                 {-8, nullptr, false, false, false},
  };
  CHECK(kNumSamplers == 8, "%d entries", (int)kNumSamplers);
  for (const auto& w : want) {
    const SamplerInfo* e = sampler_info(w.id);
    CHECK((e != nullptr) == w.known, "id %d", (int)w.id);
    if (e != nullptr && w.known) {
      CHECK(e == &kSamplers[w.id] && e->id == w.id, "id %d: entry of %d", (int)w.id, (int)e->id);
      CHECK(std::string(e->name) == w.name, "id %d: %s", (int)w.id, e->name);
    }
    CHECK(sampler_is_known(w.id) == w.known, "id %d", (int)w.id);
    CHECK(sampler_runs_wave_per_unit(w.id) == w.wave, "id %d", (int)w.id);
    CHECK(sampler_draws_lengths(w.id) == w.lengths, "id %d", (int)w.id);
  }
  CHECK(GAT_SAMPLER_ANNOTATOR == 0 && GAT_SAMPLER_SEGMENTS == 1 && GAT_SAMPLER_SHIFT == 2 && GAT_SAMPLER_GLOBAL_PERMUTATION == 3 &&
            GAT_SAMPLER_LOCAL_PERMUTATION == 4 && GAT_SAMPLER_BRUTE_FORCE == 5 && GAT_SAMPLER_CIRCULAR == 6 && GAT_SAMPLER_UNIVERSE == 7,
        "the ids of include/gat_mi355.h");
  if (g_failed) {
    fprintf(stderr, "samplers_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("samplers_check: ok\n");
  return 0;
}
