// part_chain.h -- K_part's chain kind (PK_CHAIN, part_body.h chain_tile): what one event does to one
// chain partial, written once for the kernel and the host (KG_FN), with the entry layout both share.
//
//   every e1=S[f1] -> e2=S[f2] [-> e3=S[f3] [-> e4=S[f4]]] [within T]      (one stream, one key)
//
// Why a partial's own words are enough (paths relative to core/query/input/stream/state/):
//   * every partial is opened by e1 (StreamPostStateProcessor.java:53-72; the every-clone re-arms
//     e1) and enters e2's pending list at the next event (two-phase add / update): the processors of
//     one stream run in reverse registration order -- e_S, .., e2, e1 -- so the event that opens a
//     partial, or advances it into state s, is never seen by it in its new state;
//   * every stream state checks `within` before its filter (StreamPreStateProcessor.java:292-337,
//     isExpired :102-113): an expired partial leaves whatever list holds it;
//   * f_s reads the current event and the partial's earlier slots only, so whether a partial advances,
//     completes or expires at an event depends on the events and on its own words: the partials can
//     be walked one at a time through a tile of events (entry-major) with the event-major result;
//   * the matches of one event come from e_S's pending list, in list order. A partial joins state
//     s + 1's list when it passes f_s, after those that passed earlier, and those passing at the same
//     event keep state s's list order: by induction the list of state s is ordered by ascending
//     (seq of slot s-1, .., seq of slot 0), most significant first, and so are one event's matches
//     with s = S - 1. The match records carry the slots' seqs and the table sorts by that key.
#pragma once
#include "kgen.h"

namespace sdh {

// (the entry accessors as the kernels have always had them: device functions under hipcc)
#ifdef __HIPCC__
#define PC_FN __device__
#define PC_FORCE_FN __device__ __forceinline__
#else
#define PC_FN inline
#define PC_FORCE_FN inline
#endif
// entry word offsets of a count or chain partial: ts1, seq1, flags, then cmax seq words (the count
// chain; a chain partial's slots 1 .. S-2), then the captured words later filters read: e1's, the
// count chain's first and last event's (a chain partial's slots 0, 1 and 2)
struct PartOffs {
  int cmax, n_e1, n_first, n_last;
  PC_FN int o_e1() const { return 3 + cmax; }
  PC_FN int o_first() const { return 3 + cmax + n_e1; }
  PC_FN int o_last() const { return 3 + cmax + n_e1 + n_first; }
};

// a count partial as f3 sees it (a chain partial as f2 .. f4 see it): the three captured word groups
// and their null bits in the flags word (16 / 24 / 32 + j)
template <class Ref>
struct PartEnt {
  Ref e;
  int64_t fl;
  PartOffs of;
  PC_FN int64_t e1(int j) const { return e.get(of.o_e1() + j); }
  PC_FN int64_t first(int j) const { return e.get(of.o_first() + j); }
  PC_FN int64_t last(int j) const { return e.get(of.o_last() + j); }
  PC_FN bool e1_null(int j) const { return (fl >> (16 + j)) & 1; }
  PC_FN bool first_null(int j) const { return (fl >> (24 + j)) & 1; }
  PC_FN bool last_null(int j) const { return (fl >> (32 + j)) & 1; }
};

template <class Ref>
PC_FORCE_FN PartEnt<Ref> part_ent(const Ref& e, int64_t fl, const PartOffs& of) {
  return PartEnt<Ref>{e, fl, of};
}

// StreamPreStateProcessor.isExpired:102-113 (dev::expired)
KG_FN bool chain_expired(int64_t ts1, int64_t ts, int64_t within) {
  if (within < 0) return false;
  const int64_t d = (int64_t)((uint64_t)ts1 - (uint64_t)ts);
  const int64_t a = d < 0 ? (int64_t)(0ull - (uint64_t)d) : d;
  return a > within;
}

enum { CS_WAIT = 0, CS_ADVANCE = 1, CS_DONE = 2, CS_EXPIRED = 3 };

// One event for one chain partial of S states with `filled` slots beyond e1 (it waits in state
// s = filled + 1): expiry first, then f_s -- pass(s) -- over the event and the partial as it is.
// The states are tried from S - 1 down, each under the test s == filled + 1, so the lanes of a wave
// that hold partials in different states run one state's filter at a time.
template <class Pass>
KG_FN int chain_step(int S, int filled, int64_t ts1, int64_t ts, int64_t within, Pass&& pass) {
  if (chain_expired(ts1, ts, within)) return CS_EXPIRED;
  int r = CS_WAIT;
  for (int s = S - 1; s >= 1; --s)
    if (s == filled + 1 && pass(s)) r = s == S - 1 ? CS_DONE : CS_ADVANCE;
  return r;
}

// e1 opens a partial: ts1, seq1, slot 0's captured words; returns its flags word (no filled slots)
template <class Ref, class Ev>
KG_FN int64_t chain_open(const Ref& e, const PartOffs& of, int ncap, int64_t ts, int64_t seq, const Ev& ev) {
  e.set(0, ts);
  e.set(1, seq);
  for (int j = 0; j < of.n_e1 && j < ncap; ++j) e.set(of.o_e1() + j, ev.word(j));
  return (int64_t)(ev.nul & 0xff) << 16;
}

// CS_ADVANCE at state s (1 <= s <= S - 2): the event becomes slot s -- its seq, and its captured
// words and null bits where the set keeps that slot; returns the new flags word
template <class Ref, class Ev>
KG_FN int64_t chain_advance(const Ref& e, int64_t fl, const PartOffs& of, int ncap, int s, int64_t seq, const Ev& ev) {
  e.set(3 + s - 1, seq);
  const int64_t nb = (int64_t)(ev.nul & 0xff);
  if (s == 1) {
    for (int j = 0; j < of.n_first && j < ncap; ++j) e.set(of.o_first() + j, ev.word(j));
    fl = (fl & ~(0xffll << 24)) | (nb << 24);
  } else if (s == 2) {
    for (int j = 0; j < of.n_last && j < ncap; ++j) e.set(of.o_last() + j, ev.word(j));
    fl = (fl & ~(0xffll << 32)) | (nb << 32);
  }
  return (fl & ~0xffll) | (int64_t)s;
}

// slot k's seq of a partial with at least k filled slots (k = 0: e1)
template <class Ref>
KG_FN int64_t chain_slot_seq(const Ref& e, int k) {
  return k == 0 ? e.get(1) : e.get(3 + k - 1);
}

// an attribute's raw word as the typed bytecode's value (FilterProcessor.java:55-66)
KG_FN kg::Val chain_typed(const kg::GInsn& in, int64_t raw, bool isnull) {
  kg::Val v{in.res, 1, 0};
  if (!isnull) {
    v.null = 0;
    v.bits = in.res == kg::T_INT ? (int64_t)(int32_t)raw : in.res == kg::T_FLOAT ? (int64_t)(uint32_t)raw : raw;
  }
  return v;
}

// f_s interpreted: slot s at index 0 / CURRENT is the event, slots 0, 1 and 2 below s the partial's
// e1 / first / last words (kpart_shape admits no other reference, and every slot below s is filled)
template <class Ev, class En>
KG_FN bool chain_filter(const kg::GQuery* q, const kg::GQuery* ql, int s, const Ev& ev, const En& en) {
  const kg::GState& gs = q->st[s];
  for (int f = 0; f < gs.n_filt; ++f) {
    const kg::Val v = kg::eval_code<kg::RegStack>(
        q, ql, gs.fb[f], gs.fe[f],
        [&](const kg::GInsn& in) {
          const int j = (int)in.imm;
          if (in.a == s) return chain_typed(in, ev.word(j), ev.null(j));
          if (in.a == 0) return chain_typed(in, en.e1(j), en.e1_null(j));
          if (in.a == 1) return chain_typed(in, en.first(j), en.first_null(j));
          return chain_typed(in, en.last(j), en.last_null(j));
        },
        [&](const kg::GInsn&) { return false; });
    if (v.null || !v.bits) return false;
  }
  return true;
}

}  // namespace sdh
