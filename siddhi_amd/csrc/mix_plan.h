// mix_plan.h -- which path an interleaved push takes (sdh_engine_push_mixed; DESIGN.md §3.2 "Interleaved
// pushes"): a pure function over plain data, without HIP, so the host tests drive it directly
// (tests/native/mix_plan_host.cpp). engine.hip fills a Call from the engine's plans and asks why_split.
#pragma once
#include <stdint.h>

namespace sdh {
namespace mixplan {

constexpr int MAX_PARTS = 8;  // (= MIX_MAXP, nfa_types.h)

// the kinds of query that read a named stream, one bit each
enum Consumer : uint32_t {
  C_CHAIN = 1u << 0,     // K_chain
  C_GEN = 1u << 1,       // the K_gen kernel, in the unpartitioned set
  C_RATCHET = 1u << 2,   // K_ratchet
  C_GATE = 1u << 3,      // K_gate
  C_SEQ = 1u << 4,       // a K_seq group of the unpartitioned set
  C_WAVE = 1u << 5,      // K_wave
  C_PART = 1u << 6,      // K_part
  C_SLAB = 1u << 7,      // K_slab
  C_GEN_PART = 1u << 8,  // the K_gen kernel, in a partition's set
  C_RANGE = 1u << 9,     // the stream's index is past what a K_gen-family query can name, and the engine holds one
};

struct Call {
  int32_t n_parts = 0;
  uint32_t consumers[MAX_PARTS] = {};  // per part: the kinds that read its stream (the first MAX_PARTS parts)
  int64_t total = 0;                   // events of the call
  bool knob_split = false;             // SDH_MIX_SPLIT
  bool comm = false;                   // the engine belongs to a communicator
  bool timed_gen = false;              // a K_gen set has absent states: time passes for it on every push
};

// nullptr: the call runs natively (one K_chain launch and / or one K_gen launch over the merged
// sequence); else why it runs as one push per same-stream run
inline const char* why_split(const Call& c) {
  if (c.knob_split) return "SDH_MIX_SPLIT";
  if (c.comm) return "the engine belongs to a communicator";
  if (c.n_parts > MAX_PARTS) return "more than 8 parts";
  if (c.total >= INT32_MAX) return "2^31 - 1 events or more";
  if (c.timed_gen) return "a K_gen set has absent states";
  for (int p = 0; p < c.n_parts; ++p) {
    const uint32_t k = c.consumers[p];
    if (k & C_RATCHET) return "a K_ratchet query reads a named stream";
    if (k & C_GATE) return "a K_gate query reads a named stream";
    if (k & C_RANGE) return "a named stream is past the K_gen family's stream range";
    if (k & C_SEQ) return "a K_seq group reads a named stream";
    if (k & C_WAVE) return "a K_wave query reads a named stream";
    if (k & C_PART) return "a K_part query reads a named stream";
    if (k & C_SLAB) return "a K_slab query reads a named stream";
    if (k & C_GEN_PART) return "a partitioned K_gen query reads a named stream";
  }
  return nullptr;
}

}  // namespace mixplan
}  // namespace sdh
