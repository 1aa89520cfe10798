// wave_step.h -- K_wave (nfa_wave.hip): what one event does to one partial of the unpartitioned count
// pattern, written once for the kernel and the host (KG_FN).
//
//   every e1=S[f1] -> e2=S[f2] <min:max> -> e3=S[f3] [within T]
//
// An entry uses K_part's PK_COUNT layout (nfa_types.h, PartOffs): ts0, e1's seq, flags (len | in-e3-list
// << 8 | the null bytes of e1 / e2[0] / e2[last] << 16 / 24 / 32), cmax chain seqs, then the captured
// words of e1, e2[0] and e2[last] that f3 reads.
//
// Why a partial's own words are enough is part_body.h's argument for the count chain (the reference's
// e3 list is the creation-ordered subset of partials with len >= min; the count state appends every
// f2-passing event while len < max and makes no `within` check; e3 checks `within`, then f3 over the
// partial as it is at that event; f1 and f2 read the event only). wave_step restates the inner loop of
// part_body.h's count_tile. That copy stays inline there: sharing one function with the partitioned
// count kernel moved it from 126 to 137 VGPRs plus scratch, so the two copies exist
// side by side and tests/test_wave_host.py checks this one against the oracle.
#pragma once
#include "part_chain.h"

namespace sdh {

enum { WS_KEEP = 0, WS_DONE = 1, WS_DEAD = 2 };

// the flags word's fields
KG_FN int wave_len(int64_t fl) { return (int)(fl & 0xff); }
KG_FN bool wave_in3(int64_t fl) { return (fl >> 8) & 1; }

// an event-only filter of state `sid` (FilterProcessor.java:55-66 over the typed bytecode): the state's
// own slot at index 0 / CURRENT is the event, every other reference is null
template <class Ev>
KG_FN bool wave_ev_filter(const kg::GQuery* q, int sid, const Ev& ev) {
  const kg::GState& gs = q->st[sid];
  for (int f = 0; f < gs.n_filt; ++f) {
    const kg::Val v = kg::eval_code<kg::RegStack>(
        q, q, gs.fb[f], gs.fe[f],
        [&](const kg::GInsn& in) {
          const bool here = in.a == sid && (in.b == 0 || in.b == -1);
          return chain_typed(in, here ? ev.word((int)in.imm) : 0, !here || ev.null((int)in.imm));
        },
        [&](const kg::GInsn& in) { return !(in.a == sid && (in.b == 0 || in.b == -1)); });
    if (v.null || !v.bits) return false;
  }
  return true;
}

// f3 over the partial as it is now: slot 2 the current event, slot 0 e1, slot 1 the chain's first
// (index 0) or last (CURRENT) event -- all exist (len >= min >= 1)
template <class Ev, class En>
KG_FN bool wave_f3(const kg::GQuery* q, const Ev& ev, const En& en) {
  const kg::GState& s3 = q->st[2];
  for (int f = 0; f < s3.n_filt; ++f) {
    const kg::Val v = kg::eval_code<kg::RegStack>(
        q, q, s3.fb[f], s3.fe[f],
        [&](const kg::GInsn& in) {
          const bool here = in.b == 0 || in.b == -1;
          const int j = (int)in.imm;
          if (in.a == 2) return chain_typed(in, here ? ev.word(j) : 0, !here || ev.null(j));
          if (in.a == 0) return chain_typed(in, here ? en.e1(j) : 0, !here || en.e1_null(j));
          const bool first = in.b == 0;
          return chain_typed(in, first ? en.first(j) : en.last(j), first ? en.first_null(j) : en.last_null(j));
        },
        [&](const kg::GInsn&) { return false; });
    if (v.null || !v.bits) return false;
  }
  return true;
}

// e1 opens a partial at the event (ts, seq, ev): every word of the entry is written (the chain and
// the first / last captures as zeros), so a table holds no stale word; returns its flags word. The
// partial is in the count state's list from the next event on.
template <class Ref, class Ev>
KG_FN int64_t wave_open(const Ref& e, const PartOffs& of, int ncap, int64_t ts, int64_t seq, const Ev& ev) {
  const int ew = 3 + of.cmax + of.n_e1 + of.n_first + of.n_last;
  for (int w = 3; w < ew; ++w) e.set(w, 0);
  e.set(0, ts);
  e.set(1, seq);
  for (int j = 0; j < of.n_e1 && j < ncap; ++j) e.set(of.o_e1() + j, ev.word(j));
  const int64_t fl = (int64_t)(ev.nul & 0xff) << 16;
  e.set(2, fl);
  return fl;
}

// One event (ts, seq, ev; pass2: it passes f2) for one partial, in the reference's order:
//   1. in e3's list: expired against ts0 -> it leaves the list; else f3 over the partial as it is now
//      (f3()) -> WS_DONE;
//   2. len < max and the event passes f2 -> append (seq, first / last captures and their null bits);
//      at len == min the partial enters e3's list, visible from the next event;
//   3. in neither list -> WS_DEAD.
// fl is the partial's flags word, updated in place; the entry's word 2 is the caller's to store.
template <class Ref, class Ev, class F3>
KG_FN int wave_step(const Ref& e, int64_t& fl, const PartOffs& of, int ncap, int cmin, int cmax, int64_t within,
                    int64_t ts, int64_t seq, const Ev& ev, bool pass2, F3&& f3) {
  int len = wave_len(fl);
  bool in3 = wave_in3(fl);
  if (in3) {
    if (chain_expired(e.get(0), ts, within)) in3 = false;
    else if (f3()) return WS_DONE;
  }
  if (len < cmax && pass2) {
    e.set(3 + len, seq);
    const int64_t nb = (int64_t)(ev.nul & 0xff);
    if (len == 0) {
      for (int j = 0; j < of.n_first && j < ncap; ++j) e.set(of.o_first() + j, ev.word(j));
      fl = (fl & ~(0xffll << 24)) | (nb << 24);
    }
    for (int j = 0; j < of.n_last && j < ncap; ++j) e.set(of.o_last() + j, ev.word(j));
    fl = (fl & ~(0xffll << 32)) | (nb << 32);
    ++len;
    if (len == cmin) in3 = true;  // CountPost: next.addState at n == min (visible next event)
  }
  fl = (fl & ~0x1ffll) | (int64_t)len | ((int64_t)in3 << 8);
  return (!in3 && len >= cmax) ? WS_DEAD : WS_KEEP;
}

}  // namespace sdh
