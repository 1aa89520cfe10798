// Host driver of an interleaved push's eligibility (siddhi_amd/csrc/mix_plan.h): test infrastructure
// only. tests/test_mix_plan_host.py loads it from libmix_plan_host.so and asks why a call splits.
#include <cstring>

#include "../../siddhi_amd/csrc/mix_plan.h"

extern "C" {

// consumers: n_parts bitmasks of mixplan::Consumer (only the first MAX_PARTS are read, as the engine fills
// them). Returns 0 and an empty reason for a native call, else 1 and the reason
int mph_why_split(int n_parts, const uint32_t* consumers, long long total, int knob_split, int comm, int timed_gen,
                  char* why, size_t cap) {
  sdh::mixplan::Call c;
  c.n_parts = n_parts;
  for (int p = 0; p < n_parts && p < sdh::mixplan::MAX_PARTS; ++p) c.consumers[p] = consumers[p];
  c.total = total;
  c.knob_split = knob_split != 0;
  c.comm = comm != 0;
  c.timed_gen = timed_gen != 0;
  const char* r = sdh::mixplan::why_split(c);
  if (cap) {
    strncpy(why, r ? r : "", cap - 1);
    why[cap - 1] = 0;
  }
  return r ? 1 : 0;
}

int mph_max_parts() { return sdh::mixplan::MAX_PARTS; }

// the Consumer bit of a kind by name (so the test's table names kinds, not numbers); 0: unknown
unsigned mph_kind(const char* name) {
  using namespace sdh::mixplan;
  const struct {
    const char* n;
    uint32_t k;
  } kinds[] = {{"chain", C_CHAIN}, {"gen", C_GEN},   {"ratchet", C_RATCHET},   {"gate", C_GATE},  {"seq", C_SEQ},
               {"wave", C_WAVE},   {"part", C_PART}, {"slab", C_SLAB},         {"gen_part", C_GEN_PART},
               {"range", C_RANGE}};
  for (const auto& x : kinds)
    if (!strcmp(x.n, name)) return x.k;
  return 0;
}
}
