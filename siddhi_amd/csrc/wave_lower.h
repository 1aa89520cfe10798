// wave_lower.h -- host-side K_wave shape selection (no HIP: the engine and the host tests share it).
//
// K_wave (nfa_wave.hip) runs the unpartitioned count pattern
//   every e1=S[f1] -> e2=S[f2] <min:max> -> e3=S[f3] [within T]
// one wave per query, one lane per partial. The shape is K_part's PK_COUNT (part_lower.h) without its
// `partition with`: wave_shape applies the same checks, through the same helpers, with
// q.partition < 0 in place of >= 0, and says why it declines. One condition differs, because the
// planner marks every unpartitioned `every` with it: e1 may carry its own within-every link
// (kpart_three_why explains why that link is inert). Every other query stays where it plans
// otherwise (K_chain, K_seq, K_gen).
#pragma once
#include "part_lower.h"

namespace sdh {

// the K_wave shape of query qi: kind PK_COUNT with cmax / n_e1 / n_first / n_last as kpart_shape fills
// them, or kind -1 and *why (a static string) the reason
inline KPart wave_shape(const kg::LProgram& P, int qi, const kg::GQuery& g, const char** why = nullptr) {
  const kg::LQuery& q = P.q[qi];
  KPart k;
  const char* w = nullptr;
  if (q.partition >= 0) w = "a partitioned query (K_part)";
  else if (q.type != kg::Q_PATTERN) w = "a sequence";
  else if ((w = kpart_pattern_why(q, g))) {
  } else if ((w = kpart_three_why(q, true))) {  // (e1's own within-every link: inert, part_lower.h)
  } else {
    w = kpart_count_why(q, g, k);
  }
  if (w) k = KPart{};
  if (why) *why = w ? w : "";
  return k;
}

}  // namespace sdh
