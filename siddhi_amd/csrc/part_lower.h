// part_lower.h -- host-side K_part shape selection (no HIP: the engine and the host tests share it).
//
// K_part (part_body.h) runs partitioned same-stream patterns whose structure compact partial tables
// reproduce exactly:
//   PK_OR / PK_AND  every e1=S[f1] -> e2=S[f2] or|and e3=S[f3] [within T]
//   PK_COUNT        every e1=S[f1] -> e2=S[f2] <min:max> -> e3=S[f3] [within T]
//   PK_CHAIN        every e1=S[f1] -> e2=S[f2] [-> e3=S[f3] [-> e4=S[f4]]] [within T]
// kpart_shape decides which of them, if any, a query is; every other query stays where it plans
// otherwise (K_slab, K_gen).
#pragma once
#include <utility>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
// a host compiler reading nfa_types.h: the launch structs' HIP spellings
#define __host__
#define __device__
struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
#endif

#include "gen_lower.h"
#include "nfa_types.h"

namespace sdh {

// K_part shape of a query (kpart_shape; kind < 0: none). PK_COUNT: n_e1 / n_first / n_last are the
// captured words of e1, e2[0] and e2[last] that f3 reads (0 or the stream's n_cap). PK_CHAIN: the same
// three fields are the captured words of slots 0, 1 and 2 that a later state's filter reads, and cmax
// is S - 2, the slots between e1 and the trigger whose seq the entry keeps.
struct KPart {
  int kind = -1, sA = 1, sB = 2, cmax = 0, n_e1 = 0, n_first = 0, n_last = 0;
};

// every slot reference of state i's filters: (slot, chain index) pairs
inline void filter_refs(const kg::LState& st, std::vector<std::pair<int64_t, int64_t>>& refs) {
  for (const auto& f : st.filters)
    for (const auto& in : f)
      if (in.op == kg::OP_ATTR || in.op == kg::OP_STREAM_IS_NULL) refs.push_back({in.a, in.b});
}

// PK_CHAIN: a linear chain of 2 .. MAXLO + 1 stream states over one stream (the match table orders one
// event's matches by the MAXLO earlier slots' seqs, nfa_types.h). f1 reads its own event; f_s the
// current event and the earlier slots at chain index 0 / CURRENT (one event per slot)
inline KPart kpart_chain_shape(const kg::LQuery& q, const kg::GQuery& g) {
  KPart k;
  const int S = (int)q.st.size();
  if (S < 2 || S > MAXLO + 1) return k;
  const int s0 = q.st[0].stream;
  for (const auto& x : q.st)
    if (x.kind != kg::K_STREAM || x.stream != s0 || x.waiting != -1 || x.within_every != -1 || x.callback != -1) return k;
  if (q.recvs.size() != 1 || q.recvs[0].stream != s0 || (int)q.recvs[0].procs.size() != S) return k;
  for (int i = 0; i < S; ++i) {
    const kg::LState& x = q.st[i];
    if (q.recvs[0].procs[i] != i) return k;
    if (x.is_start != (i == 0) || x.next_every != (i == 0 ? 0 : -1)) return k;
    if (x.next_pre != (i + 1 < S ? i + 1 : -1) || (x.has_selector != 0) != (i == S - 1)) return k;
  }
  const int ncap = g.n_cap[s0];
  std::vector<std::pair<int64_t, int64_t>> r;
  for (int i = 0; i < S; ++i) {
    // an event reached in any other way than OP_ATTR / OP_STREAM_IS_NULL declines
    for (const auto& f : q.st[i].filters)
      for (const auto& in : f)
        if (in.op == kg::OP_EVENT_TS || kg::op_delta(in.op) == kg::OP_DELTA_BAD) return k;
    r.clear();
    filter_refs(q.st[i], r);
    for (const auto& x : r) {
      if (x.first < 0 || x.first > i || (x.second != 0 && x.second != -1)) return k;
      if (x.first == i) continue;  // the current event
      if (x.first == 0) k.n_e1 = ncap;
      else if (x.first == 1) k.n_first = ncap;
      else k.n_last = ncap;
    }
  }
  k.cmax = S - 2;
  k.kind = PK_CHAIN;
  return k;
}

// The checks of kpart_shape, in its order, as steps a sibling selector shares (wave_lower.h: the same
// count shape without its partition). Each returns nullptr, or why the query is not that shape.

// what every K_part shape needs of a pattern query whatever its states are
inline const char* kpart_pattern_why(const kg::LQuery& q, const kg::GQuery& g) {
  for (const auto& x : q.st)
    if (x.waiting != -1) return "an absent side";  // absent sides run on K_gen
  // start ids exist only with `within` (StateInputStreamParser.java:126-138): then e1 alone
  if (!(q.start_ids.empty() || (q.start_ids.size() == 1 && q.start_ids[0] == 0))) return "start states beyond e1";
  if (g.max_depth > kg::RSTACK) return "a filter deeper than the register stack";
  if (q.start_ids.empty() && q.within >= 0) return "`within` without start ids";
  if (q.st.empty()) return "no states";
  return nullptr;
}

// three states on one stream, one receiver that runs e1 first, `every` on e1 only.
// start_within_every: e1 may name itself as its within-every state. The planner sets that link on the
// states inside `every` of an unpartitioned query only (a partitioned one never carries it), and on
// the start state it is inert: the link acts when a partial expires in the state that carries it, and
// the seed e1 holds has no start-state event to expire by (kgen.h seq_lookback makes the same
// argument). K_part passes false: its answers stay what they were for any blob.
inline const char* kpart_three_why(const kg::LQuery& q, bool start_within_every = false) {
  if (q.st.size() != 3) return "not three states";
  const int s = q.st[0].stream;
  for (size_t i = 0; i < q.st.size(); ++i) {
    const auto& x = q.st[i];
    const bool we_ok = x.within_every == -1 || (start_within_every && i == 0 && x.is_start && x.within_every == 0);
    if (x.stream != s || !we_ok || x.callback != -1) return "a second stream, or a state-level within / callback";
  }
  if (q.recvs.size() != 1 || q.recvs[0].stream != s || q.recvs[0].procs.size() != 3 || q.recvs[0].procs[0] != 0)
    return "not one receiver in state order";
  const kg::LState& e1 = q.st[0];
  if (e1.kind != kg::K_STREAM || !e1.is_start || e1.next_every != 0 || e1.has_selector) return "e1 is not the `every` start state";
  return nullptr;
}

// states 1 and 2 are the count chain `e2=S[f2]<min:max> -> e3=S[f3]`: fills k (cmax, n_e1, n_first,
// n_last; kind = PK_COUNT) as far as it gets
inline const char* kpart_count_why(const kg::LQuery& q, const kg::GQuery& g, KPart& k) {
  const kg::LState &e1 = q.st[0], &c = q.st[1], &e3 = q.st[2];
  const auto& procs = q.recvs[0].procs;
  if (c.kind != kg::K_COUNT) return c.kind == kg::K_LOGICAL ? "a logical state" : "no count state in the middle";
  if (c.min < 1) return "count min below 1";
  if (c.max == INT32_MAX) return "an unbounded count";  // (`<n:>`: the planner's Integer.MAX_VALUE)
  if (c.max > PK_CMAX) return "count max beyond PK_CMAX";
  if (c.min > c.max) return "count min above max";
  if (c.next_pre != 2 || c.next_every != -1 || c.has_selector || e1.next_pre != 1) return "the count state is not the middle state";
  if (e3.kind != kg::K_STREAM || e3.next_pre != -1 || e3.next_every != -1 || !e3.has_selector) return "e3 is not the last stream state";
  if (procs[1] != 1 || procs[2] != 2) return "not one receiver in state order";
  std::vector<std::pair<int64_t, int64_t>> r;
  filter_refs(c, r);  // the count filter reads only the event it is appending (CURRENT)
  for (const auto& x : r)
    if (x.first != 1 || x.second != -1) return "f2 reads more than the current event";
  r.clear();
  filter_refs(e3, r);  // e3 reads e1, e2[0], e2[last] (= CURRENT of another state) and itself
  const int ncap = g.n_cap[q.st[0].stream];
  for (const auto& x : r) {
    if (x.first == 1) {
      if (x.second == 0) k.n_first = ncap;
      else if (x.second == -1) k.n_last = ncap;
      else return "f3 reads a chain event other than e2[0] / e2[last]";
    } else if (x.first == 0) {
      k.n_e1 = ncap;
    }
  }
  k.cmax = c.max;
  k.kind = PK_COUNT;
  return nullptr;
}

inline KPart kpart_shape(const kg::LProgram& P, int qi, const kg::GQuery& g) {
  KPart k;
  const kg::LQuery& q = P.q[qi];
  if (q.partition < 0 || q.type != kg::Q_PATTERN) return k;
  if (kpart_pattern_why(q, g)) return k;
  {
    bool all_stream = true;
    for (const auto& x : q.st) all_stream &= x.kind == kg::K_STREAM;
    if (all_stream) return kpart_chain_shape(q, g);
  }
  if (kpart_three_why(q)) return k;
  const kg::LState& e1 = q.st[0];
  std::vector<std::pair<int64_t, int64_t>> r;
  const auto& procs = q.recvs[0].procs;
  if (q.st[1].kind == kg::K_LOGICAL) {
    const kg::LState &a = q.st[1], &b = q.st[2];
    if (b.kind != kg::K_LOGICAL || a.partner != 2 || b.partner != 1 || a.ltype != b.ltype) return k;
    for (const auto* x : {&a, &b})
      if (x->is_start || x->next_pre != -1 || x->next_every != -1 || !x->has_selector) return k;
    if (e1.next_pre != 1 && e1.next_pre != 2) return k;
    if (!((procs[1] == 1 && procs[2] == 2) || (procs[1] == 2 && procs[2] == 1))) return k;
    for (int i = 1; i <= 2; ++i) {  // the sides' filters read only their own slot (event-only)
      r.clear();
      filter_refs(q.st[i], r);
      for (const auto& x : r)
        if (x.first != i) return k;
    }
    k.sA = procs[1];  // registration order: the side processed second
    k.sB = procs[2];
    k.kind = a.ltype == kg::L_AND ? PK_AND : PK_OR;
    return k;
  }
  kpart_count_why(q, g, k);  // (a declined query keeps kind -1)
  return k;
}

}  // namespace sdh
