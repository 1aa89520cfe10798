// select_body.h -- the device selector's lane body: one completed match -> one output row.
//
// Restates QuerySelector.process (core/query/selector/QuerySelector.java:76-169) for a `select` list
// without aggregation: every output attribute is an expression over the match's StateEvent, evaluated
// with the typed bytecode of the filters (kgen.h: Val, typed_compare, arith, eval_insns_imm).
// OP_ATTR(a, b, imm) reads attribute imm of the event StateEvent.getStreamEvent (StateEvent.java:138-182)
// resolves for slot a at chain index b; the event's words come from the engine's event store, a
// row-major ring in HBM indexed by global sequence number (select.hip).
//
// Written once for host and device (KG_FN), like kgen.h: select.hip runs it one lane per match,
// tests/native/select_host.cpp builds it for the host and checks it against siddhi_amd/selector.py.
#pragma once
#include "kgen.h"

namespace sdh {
namespace sel {

constexpr int MAXOUT = 64;  // outputs per query (one null-mask bit each)

// the event store: event `seq` is row seq & mask, W = 2 + (the most attributes any stream has) words
// {ts, null bits (bit a: attribute a is null), attribute words}; rows [lo, next seq) are present
struct Store {
  const int64_t* rows;
  int64_t mask;
  int64_t lo;
  int32_t W;
  int32_t pad;
};

// word w of event seq's row (w: 0 ts, 1 null bits, 2 + a attribute a)
KG_FN int64_t store_index(int64_t seq, int64_t mask, int W, int w) { return (seq & mask) * W + w; }

// one output of a shape: its code range in the instruction table and its result type; `direct`
// marks a single OP_ATTR (select e1.symbol as s): a load, no trip through the stack machine
struct Out {
  int32_t b, e;
  int32_t type;
  int32_t direct;
};
// a shape: the outputs of every query whose select lists are equal apart from CONST immediates
struct Shape {
  int32_t out0, n_out;
  int32_t depth;  // deepest evaluation stack of any output
  int32_t pad;
};
// a query: its shape and its own CONST immediates (consts[const0 + k]: the k-th CONST of the shape in
// program order; a CONST instruction of the table carries k in imm)
struct Query {
  int32_t shape, n_out;
  int64_t const0;
};
struct Tables {
  const kg::GInsn* code;
  const Out* outs;
  const Shape* shapes;
  const Query* queries;
  const int64_t* consts;
};

// A match's slots. Words: the match table's form, per slot a count c then c event seqs.
// (ts: the match's StateEvent timestamp, what OP_EVENT_TS reads)
struct WordsMatch {
  const int64_t* w;
  int64_t len;
  int64_t ts = 0;
  // the chain of `slot`: its length, and `at` = the index of its first seq in w
  KG_FN int64_t chain(int slot, int64_t& at) const {
    int64_t j = 0;
    for (int s = 0; s < slot && j < len; ++s) j += 1 + w[j];
    at = j + 1;
    return j < len ? w[j] : 0;
  }
  KG_FN int64_t seq(int64_t at, int64_t k) const { return w[at + k]; }
};
// Pair: a K_ratchet match, two one-event slots {e1}, {e2} (a placed window's compact rows).
struct PairMatch {
  int64_t e1, e2;
  int64_t ts = 0;
  KG_FN int64_t chain(int slot, int64_t& at) const {
    at = slot;
    return slot < 2 ? 1 : 0;
  }
  KG_FN int64_t seq(int64_t at, int64_t) const { return at ? e2 : e1; }
};

// StateEvent.getStreamEvent(int[]):138-182 on a slot's chain (siddhi_amd/selector.py _chain_at): false
// when it resolves to no event; b >= 0 the b-th event, -1 the last, -2 the one before it, lower values
// counted from the end alike
template <class Match>
KG_FN bool event_of(const Match& m, int slot, int64_t idx, int64_t& seq) {
  int64_t at;
  const int64_t c = m.chain(slot, at);
  const int64_t k = idx >= 0 ? idx : c + idx;
  if (c <= 0 || k < 0 || k >= c) return false;
  seq = m.seq(at, k);
  return true;
}

enum { ERR_EVICTED = 1 };  // a referenced event has left the store

template <class Match>
KG_FN kg::Val attr_of(const Store& st, const Match& m, const kg::GInsn& in, int32_t& err) {
  kg::Val v{in.res, 1, 0};
  if (in.op == kg::OP_EVENT_TS) return kg::Val{kg::T_LONG, 0, m.ts};  // EventTimestampFunctionExecutor.execute:70-72
  int64_t seq;
  // seq -1: the empty event an absent logical side borrows (StreamEventPool.borrowEvent), all null
  if (!event_of(m, in.a, in.b, seq) || seq < 0) return v;
  if (seq < st.lo) {
    err |= ERR_EVICTED;
    return v;
  }
  const int64_t* row = st.rows + store_index(seq, st.mask, st.W, 0);
  if (((uint64_t)row[1] >> in.imm) & 1ull) return v;
  v.null = 0;
  v.bits = row[2 + in.imm];
  return v;
}

// a value as an output cell: the raw 64-bit encoding of siddhi_amd/events.py (null: 0)
KG_FN int64_t cell_of(const kg::Val& v, int type) {
  if (v.null) return 0;
  switch (type) {
    case kg::T_INT: return (int64_t)(int32_t)v.bits;
    case kg::T_FLOAT: return (int64_t)(uint32_t)v.bits;
    case kg::T_BOOL: return v.bits ? 1 : 0;
    default: return v.bits;
  }
}

// Row i of n: the outputs of the lane's query (shape sh, wave-uniform on the device; constants qc its
// own) into cells[c * n + i]; returns the null bits of cells [0, sh.n_out)
template <class Stack, class Match>
KG_FN uint64_t project(const Tables& T, const Shape& sh, const int64_t* qc, const Store& st, const Match& m,
                       int64_t* cells, int64_t n, int64_t i, int32_t& err) {
  uint64_t nulls = 0;
  for (int c = 0; c < sh.n_out; ++c) {
    const Out& o = T.outs[sh.out0 + c];
    kg::Val v;
    if (o.direct) {
      v = attr_of(st, m, T.code[o.b], err);
    } else {
      v = kg::eval_insns_imm<Stack>(
          T.code, [&](int pc) { return qc[T.code[pc].imm]; }, o.b, o.e,
          [&](const kg::GInsn& in) { return attr_of(st, m, in, err); },
          [&](const kg::GInsn& in) {
            int64_t seq;
            return !event_of(m, in.a, in.b, seq);
          });
    }
    if (v.null) nulls |= 1ull << c;
    cells[(int64_t)c * n + i] = cell_of(v, o.type);
  }
  return nulls;
}

}  // namespace sel
}  // namespace sdh
