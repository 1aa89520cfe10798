// chain_lower.h -- host-side lowering of a linear chain query of the pattern IR (siddhi_amd/ir.py) to
// K_chain's tables: the ChainQuery (pre-keyed compare atoms, columns, captures) and the query's
// residual programs (chain_pred.h), and K_ratchet plan selection. No HIP here, so a host test
// (tests/native/chain_host.cpp) calls the same code the engine does (engine_lower.hip).
//
// Per state the filters' top-level ANDs are flattened into conjuncts:
//   * a compare of two leaves (attribute / constant), or a bare bool leaf, is an atom: its operands
//     are converted once into compare-domain keys, and it is evaluated for a whole tile (event-only)
//     or per partial (the state's one capture-reading atom, StateDesc in nfa_chain.hip);
//   * every other conjunct built from the residual opcodes (residual_arity), and a state's second
//     and later capture-reading atoms, go to the state's residual programs: the tile residual (reads
//     no earlier slot; evaluated once per event when the tile is staged) or the partial residual
//     (evaluated per (partial, event)). Conjuncts of one program are joined by OP_AND.
// What keeps a query off K_chain (Lowered::why says which): functions and stream-null tests in a
// filter, a reference to a later slot, more than cpred::CMAXCODE residual instructions, an
// evaluation deeper than kg::RSTACK, the column or capture table exhausted.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
// a host compiler reading nfa_types.h: the launch structs' HIP spellings
#define __host__
#define __device__
struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
#endif

#include "chain_pred.h"
#include "gen_lower.h"
#include "nfa_types.h"

namespace sdh {
namespace eng {

inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// the IR as read (format: siddhi_amd/ir.py)
struct Insn {
  int op, lt, rt, res;
  int64_t a, b, imm;
};
struct IState {
  int kind, stream, is_start, min, max, ltype, partner, next_pre, next_every, within_every, callback,
      this_last, has_selector;
  int64_t waiting;  // absent states: the 'for' time (ms), else -1
  std::vector<std::vector<Insn>> filters;
};
struct IQuery {
  int type, partition;
  int64_t within;
  std::vector<IState> st;
};
struct IProgram {
  std::vector<std::vector<int>> stream_types;
  std::vector<IQuery> q;
};

// a filter's expression tree node
struct Node {
  int kind;  // 0 leaf operand, 1 cmp, 2 and, 3 other
  Insn ins;
  int l = -1, r = -1;
  int first = 0;  // the subtree is the instructions [first, own index] of the postfix code
};

// a query lowered to a ChainQuery; rcode holds its residual programs, the ChainQuery's rt_* / rp_*
// ranges index it (the engine rebases them into its one device table)
struct Lowered {
  bool ok = false;
  std::string why;
  ChainQuery cq{};
  std::vector<int> streams;
  std::vector<kg::GInsn> rcode;
};

// K_ratchet plan of a query (ratchet_plan)
struct RatchetPlan {
  bool ok = false;
  int stream = 0, key_attr = 0, key_conv = 0, key_kind = 0, xmask = 0;
  std::vector<RatchetAtom> f0;
  std::vector<int64_t> f0c;
  // K_gate (nfa_gate.hip): e2's event-only conjuncts `cur.b OP const` (empty: plain K_ratchet)
  std::vector<RatchetAtom> g;
  std::vector<int64_t> gc;
  int64_t within = -1;
  // grouping signature: everything except the per-lane constants and `within`
  std::vector<int64_t> sig() const {
    std::vector<int64_t> v{stream, key_kind, key_attr, key_conv, xmask, within >= 0, (int64_t)f0.size(),
                           (int64_t)g.size()};
    for (const auto* atoms : {&f0, &g})
      for (const auto& a : *atoms)
        v.insert(v.end(), {a.attr, a.conv, a.cur_left, a.mask, a.f64, a.cur2, a.attr2, a.conv2});
    return v;
  }
};

namespace lower {

// ------------------------------------------------------------------------------------------
// IR reader (format: siddhi_amd/ir.py)
// ------------------------------------------------------------------------------------------
enum { OP_CONST = 1, OP_ATTR, OP_IS_NULL, OP_STREAM_IS_NULL, OP_CMP, OP_AND, OP_OR, OP_NOT, OP_ARITH };
enum { K_STREAM = 0, K_COUNT, K_LOGICAL };
enum { Q_PATTERN = 0, Q_SEQUENCE };

struct WordReader {
  const int64_t* w;
  size_t n, i = 0;
  int64_t next() {
    if (i >= n) throw kg::LowerError("IR blob truncated");
    return w[i++];
  }
};

inline std::vector<Insn> read_code(WordReader& r) {
  std::vector<Insn> c((size_t)r.next());
  for (auto& x : c) {
    int64_t w0 = r.next();
    x.op = (int)(w0 & 0xff);
    x.lt = (int)((w0 >> 8) & 0xff);
    x.rt = (int)((w0 >> 16) & 0xff);
    x.res = (int)((w0 >> 24) & 0xff);
    x.a = r.next();
    x.b = r.next();
    x.imm = r.next();
  }
  return c;
}

}  // namespace lower

// (throws kg::LowerError on a malformed blob)
inline IProgram read_chain_ir(const void* blob, size_t len) {
  using namespace lower;
  if (!blob || len < 16 || memcmp(blob, "SDHIR001", 8) != 0) throw kg::LowerError("bad IR magic");
  WordReader r{reinterpret_cast<const int64_t*>(static_cast<const char*>(blob) + 8), (len - 8) / 8};
  IProgram p;
  if (r.next() != 2) throw kg::LowerError("unsupported IR version");
  p.stream_types.resize((size_t)r.next());
  for (auto& s : p.stream_types) {
    s.resize((size_t)r.next());
    for (auto& t : s) t = (int)r.next();
  }
  int64_t ns = r.next();
  for (int64_t k = 0; k < ns; ++k) {
    int64_t nb = r.next();
    for (int64_t j = 0; j < (nb + 7) / 8; ++j) r.next();
  }
  p.q.resize((size_t)r.next());
  for (auto& q : p.q) {
    q.type = (int)r.next();
    q.within = r.next();
    q.st.resize((size_t)r.next());
    q.partition = (int)r.next();
    r.next();
    for (auto& s : q.st) {
      s.kind = (int)r.next(); s.stream = (int)r.next(); s.is_start = (int)r.next();
      s.min = (int)r.next(); s.max = (int)r.next(); s.ltype = (int)r.next();
      s.partner = (int)r.next(); s.next_pre = (int)r.next(); s.next_every = (int)r.next();
      s.within_every = (int)r.next(); s.callback = (int)r.next(); s.this_last = (int)r.next();
      s.has_selector = (int)r.next();
      s.waiting = r.next();
      s.filters.resize((size_t)r.next());
      for (auto& f : s.filters) f = read_code(r);
    }
    int64_t n = r.next();
    for (int64_t k = 0; k < n; ++k) r.next();           // start ids
    n = r.next();
    for (int64_t k = 0; k < n; ++k) {                    // receivers
      r.next(); r.next();
      int64_t np = r.next();
      for (int64_t j = 0; j < np; ++j) r.next();
    }
    n = r.next();
    for (int64_t k = 0; k < n * 4; ++k) r.next();        // runtime tree
    n = r.next();
    for (int64_t k = 0; k < n; ++k) read_code(r);        // selector outputs (kg::read_program keeps them)
  }
  return p;  // partitions follow; partitioned queries are rejected by the lowering below
}

namespace lower {

// ------------------------------------------------------------------------------------------
// lowering: IR query -> ChainQuery (predicate atoms + captures) and residual programs
// ------------------------------------------------------------------------------------------
// Compare domain of a typed compare (restates ExpressionParser.java:539-1220 + compare/**):
// ordering compares promote like Java binary numeric promotion; ==/!= of Long x Float compare in
// double (EqualCompareConditionExpressionExecutorLongFloat.java:36, ...FloatLong.java:37).
inline int domain_of(int lt, int rt, int op) {
  if (lt == T_STRING || lt == T_BOOL) return D_RAW;
  if (lt == T_DOUBLE || rt == T_DOUBLE) return D_F64;
  if (lt == T_FLOAT || rt == T_FLOAT) {
    if ((op == CMP_EQ || op == CMP_NE) && (lt == T_LONG || rt == T_LONG)) return D_F64;
    return D_F32;
  }
  if (lt == T_LONG || rt == T_LONG) return D_I64;
  return D_I32;
}

// conversion of an operand of attribute type t into the key of domain d (enum Conv)
inline int conv_of(int t, int d) {
  switch (d) {
    case D_I32:
    case D_I64: return t == T_INT ? CV_I64_INT : CV_I64_LONG;
    case D_F32: return t == T_INT ? CV_F32_INT : t == T_LONG ? CV_F32_LONG : CV_F64_FLOAT;  // float->double is exact
    case D_F64:
      return t == T_INT ? CV_F64_INT : t == T_LONG ? CV_F64_LONG : t == T_FLOAT ? CV_F64_FLOAT : CV_F64_DOUBLE;
    default: return CV_RAW;
  }
}

inline int64_t host_key(int64_t raw, int conv) {  // host twin of to_key() in nfa_chain.hip
  auto dbits = [](double d) { int64_t b; memcpy(&b, &d, 8); return b; };
  auto f_of = [](int64_t r) { uint32_t u = (uint32_t)r; float f; memcpy(&f, &u, 4); return f; };
  switch (conv) {
    case CV_I64_INT: return (int64_t)(int32_t)(uint32_t)raw;
    case CV_I64_LONG: return raw;
    case CV_F32_INT: return dbits((double)(float)(int32_t)(uint32_t)raw);
    case CV_F32_LONG: return dbits((double)(float)raw);
    case CV_F32_FLOAT:
    case CV_F64_FLOAT: return dbits((double)f_of(raw));
    case CV_F64_INT: return dbits((double)(int32_t)(uint32_t)raw);
    case CV_F64_LONG: return dbits((double)raw);
    default: return raw;
  }
}

inline int mask_of(int op) {
  switch (op) {
    case CMP_EQ: return CM_EQ;
    case CMP_NE: return CM_EQ | CM_NOT;
    case CMP_GT: return CM_GT;
    case CMP_GE: return CM_GT | CM_EQ;
    case CMP_LT: return CM_LT;
    default: return CM_LT | CM_EQ;
  }
}

// The opcodes a residual program may hold, with their operand counts; -1 keeps the query off K_chain.
// OP_STREAM_IS_NULL stays out (kgen.h answers it from the slot's chain, K_gen keeps such queries), and
// so do the built-in functions (kg::OP_SELECT ...): tests/test_gpu_functions.py pins function queries
// off K_chain. Taking one in is a `case` line here (its arity), nothing else.
inline int residual_arity(int op) {
  switch (op) {
    case OP_CONST: case OP_ATTR: return 0;
    case OP_IS_NULL: case OP_NOT: return 1;
    case OP_CMP: case OP_AND: case OP_OR: case OP_ARITH: return 2;
    default: return -1;
  }
}

}  // namespace lower

// allow_residual == false (SDH_CHAIN_PRED=0): a query that needs a residual program is declined
inline Lowered lower_query(const IProgram& P, int qi, bool allow_residual = true) {
  using namespace lower;
  Lowered L;
  const IQuery& q = P.q[qi];
  const int n = (int)q.st.size();
  auto fail = [&](const std::string& w) { L.ok = false; L.why = fmt("query %d: %s", qi, w.c_str()); return L; };
  if (q.partition >= 0) return fail("partitioned queries are not on the GPU path yet");
  if (q.type != Q_PATTERN) return fail("sequences are not on the GPU path yet");
  if (n < 1 || n > MAXS) return fail(fmt("%d states (chain kernel supports 1..%d)", n, MAXS));
  ChainQuery& c = L.cq;
  c.qid = qi;
  c.n_states = n;
  c.within = q.within;
  for (int s = 0; s < n; ++s) {
    const IState& st = q.st[s];
    if (st.kind != K_STREAM) return fail("count/logical states are not on the GPU path yet");
    if (st.is_start != (s == 0)) return fail("not a linear chain");
    if (st.next_pre != (s + 1 < n ? s + 1 : -1)) return fail("not a linear chain");
    if (s > 0 && st.next_every != -1) return fail("`every` inside the chain is not on the GPU path yet");
    if (s == 0 && st.next_every != -1 && st.next_every != 0) return fail("every scope");
    if (s > 0 && st.within_every != -1) return fail("within-every re-arm");
    if (st.callback != -1) return fail("count callback");
    if (st.has_selector != (s == n - 1)) return fail("selector placement");
    c.state_stream[s] = st.stream;
    if (std::find(L.streams.begin(), L.streams.end(), st.stream) == L.streams.end())
      L.streams.push_back(st.stream);
  }
  c.every = q.st[0].next_every == 0;
  for (int s = 0; s < n; ++s)
    if ((int)P.stream_types[q.st[s].stream].size() > MAXATTR) return fail("too many attributes");
  // a single input stream and `every` make event-chunk warm-up exact
  c.chunkable = (L.streams.size() == 1) && c.every && q.within >= 0 && n >= 2;

  // the column of (stream, attribute, conversion) and the capture of (slot, column): found or added,
  // -1 when the table is full
  // (a residual's raw word is also what a long's or a double's key column holds: to_key passes both through)
  auto same_conv = [](int have, int want) {
    return have == want || (want == CV_RAW && (have == CV_I64_LONG || have == CV_F64_DOUBLE));
  };
  auto col_for = [&](int stream, int attr, int cv) {
    for (int cc = 0; cc < c.n_col; ++cc)
      if (c.col_attr[cc] == attr && same_conv(c.col_conv[cc], cv) && c.col_stream[cc] == stream) return cc;
    if (c.n_col >= MAXCOL) return -1;
    const int col = c.n_col++;
    c.col_attr[col] = attr;
    c.col_conv[col] = cv;
    c.col_stream[col] = stream;
    return col;
  };
  auto cap_for = [&](int slot, int col) {
    for (int cc = 0; cc < c.n_cap; ++cc)
      if (c.cap_slot[cc] == slot && c.cap_col[cc] == col) return cc;
    if (c.n_cap >= MAXCAP) return -1;
    c.cap_slot[c.n_cap] = slot;
    c.cap_col[c.n_cap] = col;
    return c.n_cap++;
  };
  const char* const no_room = "operand not addressable (too many columns / captures)";

  int na = 0;
  for (int s = 0; s < n; ++s) {
    c.atom_begin[s] = na;
    std::vector<Atom> const_atoms, x_atoms;
    std::vector<int> x_cols;
    // the state's residual conjuncts, each a postfix program; [0] tile, [1] partial
    std::vector<std::vector<kg::GInsn>> conj[2];
    // single-event slots resolve only chain index CURRENT (-1) and 0 (StateEvent.getStreamEvent:138-182),
    // others read null
    auto reads_cap = [&](const Insn& in) { return in.op == OP_ATTR && (in.b == -1 || in.b == 0) && in.a < s; };
    for (const auto& code : q.st[s].filters) {
      // postfix -> tree
      std::vector<Node> nodes;
      std::vector<int> stk;
      for (const Insn& ins : code) {
        Node nd;
        nd.ins = ins;
        nd.first = (int)nodes.size();
        const int ar = residual_arity(ins.op);
        if (ar < 0) return fail("filter uses a function or a stream-null test (not on K_chain)");
        if ((int)stk.size() < ar) return fail("malformed filter bytecode");
        nd.kind = ar == 0 ? 0 : ins.op == OP_CMP ? 1 : ins.op == OP_AND ? 2 : 3;
        if (ar == 2) { nd.r = stk.back(); stk.pop_back(); }
        if (ar >= 1) {
          nd.l = stk.back(); stk.pop_back();
          nd.first = nodes[nd.l].first;
        }
        nodes.push_back(nd);
        stk.push_back((int)nodes.size() - 1);
      }
      if (stk.size() != 1) return fail("malformed filter bytecode");
      // flatten the conjunction into conjuncts
      std::vector<int> todo{stk.back()};
      std::vector<int> leaves;
      while (!todo.empty()) {
        int x = todo.back(); todo.pop_back();
        if (nodes[x].kind == 2) { todo.push_back(nodes[x].r); todo.push_back(nodes[x].l); }
        else leaves.push_back(x);
      }
      for (int x : leaves) {
        const Node& nd = nodes[x];
        const bool cmp_atom = nd.kind == 1 && nodes[nd.l].kind == 0 && nodes[nd.r].kind == 0;
        const bool bool_atom = nd.kind == 0 && nd.ins.res == T_BOOL;
        if (nd.kind == 0 && !bool_atom) return fail("unsupported filter form");
        bool as_atom = cmp_atom || bool_atom;
        // a state carries one capture-reading atom (StateDesc, nfa_chain.hip): the others are residual
        const bool reads = cmp_atom ? reads_cap(nodes[nd.l].ins) || reads_cap(nodes[nd.r].ins) : reads_cap(nd.ins);
        if (as_atom && reads && !x_atoms.empty()) as_atom = false;
        if (!as_atom) {
          if (!allow_residual) return fail("filter needs a residual program (SDH_CHAIN_PRED=0)");
          std::vector<kg::GInsn> prog;
          bool partial = false;
          for (int k = nd.first; k <= x; ++k) {
            const Insn& in = code[(size_t)k];
            kg::GInsn g{};
            g.op = (int8_t)in.op; g.lt = (int8_t)in.lt; g.rt = (int8_t)in.rt; g.res = (int8_t)in.res;
            g.imm = in.imm;
            if (in.op == OP_ATTR) {
              g.imm = 0;
              if (in.a < 0 || in.a >= n) return fail("malformed filter bytecode");
              if (in.b != -1 && in.b != 0) {
                g.a = cpred::RA_NULL;
              } else if (in.a > s) {
                return fail("filter reads a later slot");
              } else {
                const int col = col_for(q.st[in.a].stream, (int)in.imm, CV_RAW);
                if (col < 0) return fail(no_room);
                if (in.a == s) {
                  g.a = cpred::RA_CUR;
                  g.b = col;
                } else {
                  const int cap = cap_for((int)in.a, col);
                  if (cap < 0) return fail(no_room);
                  g.a = cpred::RA_CAP;
                  g.b = cap;
                  partial = true;
                }
              }
            }
            prog.push_back(g);
          }
          conj[partial ? 1 : 0].push_back(prog);
          continue;
        }
        Atom A{};
        Insn li, ri;
        int op;
        if (cmp_atom) {
          li = nodes[nd.l].ins;
          ri = nodes[nd.r].ins;
          op = (int)nd.ins.imm;
        } else {
          // bare bool operand as a filter: FilterProcessor drops null and false
          li = nd.ins;
          ri = Insn{OP_CONST, 0, 0, T_BOOL, 0, 0, 1};
          op = CMP_EQ;
        }
        const int dom = domain_of(li.res, ri.res, op);
        A.mask = mask_of(op);
        A.f64 = (dom == D_F32 || dom == D_F64) ? 1 : 0;
        // operand -> (kind, index, const key)
        auto operand = [&](const Insn& in, int& k, int& idx, int64_t& cst) -> bool {
          const int cv = conv_of(in.res, dom);
          idx = 0;
          cst = 0;
          if (in.op == OP_CONST) { k = OPK_CONST; cst = host_key(in.imm, cv); return true; }
          if (in.b != -1 && in.b != 0) { k = OPK_NULL; return true; }
          if (in.a > s) return false;
          const int col = col_for(q.st[in.a].stream, (int)in.imm, cv);
          if (col < 0) return false;
          if (in.a == s) { k = OPK_CUR; idx = col; return true; }
          const int cap = cap_for((int)in.a, col);
          if (cap < 0) return false;
          k = OPK_CAP;
          idx = cap;
          return true;
        };
        if (!operand(li, A.lk, A.li, A.lc) || !operand(ri, A.rk, A.ri, A.rc)) return fail(no_room);
        if (A.lk == OPK_CAP || A.rk == OPK_CAP) {
          x_atoms.push_back(A);
          x_cols.push_back(A.lk == OPK_CUR ? A.li : A.rk == OPK_CUR ? A.ri : -1);
        } else {
          const_atoms.push_back(A);
        }
      }
    }
    // partial-independent atoms first (tile-vectorized), the capture reader last (per partial)
    if (na + (int)(const_atoms.size() + x_atoms.size()) > MAXATOM) return fail("too many predicate atoms");
    if (c.n_xa + (int)x_atoms.size() > MAXXA) return fail("too many capture-reading predicate atoms");
    for (const Atom& A : const_atoms) c.atoms[na++] = A;
    c.xa_first[s] = c.n_xa;
    c.xa_count[s] = (int)x_atoms.size();
    for (size_t k = 0; k < x_atoms.size(); ++k) {
      c.atoms[na] = x_atoms[k];
      c.xa_atom[c.n_xa] = na;
      c.xa_col[c.n_xa] = x_cols[k];
      ++c.n_xa;
      ++na;
    }
    // the residual programs: conjuncts joined by OP_AND; the evaluation stays within the register stack
    for (int kind = 0; kind < 2; ++kind) {
      const int b = (int)L.rcode.size();
      for (size_t k = 0; k < conj[kind].size(); ++k) {
        L.rcode.insert(L.rcode.end(), conj[kind][k].begin(), conj[kind][k].end());
        if (k > 0) {
          kg::GInsn g{};
          g.op = (int8_t)OP_AND; g.lt = g.rt = g.res = (int8_t)T_BOOL;
          L.rcode.push_back(g);
        }
      }
      const int e = (int)L.rcode.size();
      (kind ? c.rp_b : c.rt_b)[s] = b;
      (kind ? c.rp_e : c.rt_e)[s] = e;
      int depth = 0, maxd = 0;
      for (int pc = b; pc < e; ++pc) {
        depth += kg::op_delta(L.rcode[(size_t)pc].op);
        maxd = std::max(maxd, depth);
      }
      if (maxd > kg::RSTACK)
        return fail(fmt("residual program needs %d stack entries (K_chain evaluates in %d)", maxd, kg::RSTACK));
    }
    if ((int)L.rcode.size() > cpred::CMAXCODE)
      return fail(fmt("residual programs longer than %d instructions", cpred::CMAXCODE));
  }
  c.atom_begin[n] = na;
  for (int s = n + 1; s <= MAXS; ++s) c.atom_begin[s] = na;
  L.ok = true;
  return L;
}

// a residual program on any state
inline bool has_residual(const ChainQuery& c) {
  for (int s = 0; s < c.n_states; ++s)
    if (c.rt_e[s] > c.rt_b[s] || c.rp_e[s] > c.rp_b[s]) return true;
  return false;
}

namespace lower {

// ------------------------------------------------------------------------------------------
// K_ratchet plan selection: 2-state `every e1=S[f0] -> e2=S[cur.a OP e1.a]`
// ------------------------------------------------------------------------------------------

// an event-only atom `cur OP const` / `const OP cur` (a start filter's or a gate's) as a RatchetAtom
// and its constant; false for any other operand shape
inline bool const_atom(const ChainQuery& c, const Atom& A, RatchetAtom& ra, int64_t& cst) {
  ra = RatchetAtom{};
  ra.mask = A.mask;
  ra.f64 = A.f64;
  if (A.lk == OPK_CUR && A.rk == OPK_CONST) {
    ra.attr = c.col_attr[A.li]; ra.conv = c.col_conv[A.li]; ra.cur_left = 1; cst = A.rc;
  } else if (A.lk == OPK_CONST && A.rk == OPK_CUR) {
    ra.attr = c.col_attr[A.ri]; ra.conv = c.col_conv[A.ri]; ra.cur_left = 0; cst = A.lc;
  } else {
    return false;
  }
  return true;
}

}  // namespace lower

inline RatchetPlan ratchet_plan(const ChainQuery& c) {
  using namespace lower;
  RatchetPlan r;
  if (c.n_states != 2 || !c.every || c.state_stream[0] != c.state_stream[1]) return r;
  if (has_residual(c)) return r;  // K_ratchet and K_gate know atoms only
  if (c.n_cap != 1 || c.cap_slot[0] != 0) return r;
  if (c.xa_count[1] != 1 || c.xa_count[0] != 0) return r;
  const int x_at = c.xa_atom[c.xa_first[1]];
  // state 1's other atoms: event-only constant compares gate it (K_gate); none for K_ratchet
  for (int a = c.atom_begin[1]; a < c.atom_begin[2]; ++a) {
    if (a == x_at) continue;
    RatchetAtom ga;
    int64_t cst = 0;
    if (!const_atom(c, c.atoms[a], ga, cst) || r.g.size() >= (size_t)RMAXF0) return RatchetPlan();
    r.g.push_back(ga);
    r.gc.push_back(cst);
  }
  const Atom& X = c.atoms[x_at];
  int mask = X.mask;
  if (mask & CM_NOT) return r;
  if (!(mask & (CM_LT | CM_GT)) || ((mask & CM_LT) && (mask & CM_GT))) return r;  // ordering only
  int cur_col;
  if (X.lk == OPK_CUR && X.rk == OPK_CAP) {
    cur_col = X.li;
  } else if (X.lk == OPK_CAP && X.rk == OPK_CUR) {
    cur_col = X.ri;
    const int lt = mask & CM_LT, gt = mask & CM_GT;
    mask = (mask & CM_EQ) | (lt ? CM_GT : 0) | (gt ? CM_LT : 0);  // key OP cur == cur OP' key
  } else {
    return r;
  }
  if (c.cap_col[0] != cur_col) return r;  // key = e1 value of the same column and conversion
  const int conv = c.col_conv[cur_col];
  // both operands are the same column with the same conversion: a float column compared in
  // binary64 orders exactly as in binary32, an int column as int32 (32-bit ring entries)
  switch (conv) {
    case CV_F32_INT: case CV_F32_LONG: case CV_F32_FLOAT: case CV_F64_FLOAT: r.key_kind = KK_F32; break;
    case CV_I64_INT: case CV_F64_INT: r.key_kind = KK_I32; break;
    case CV_I64_LONG: r.key_kind = KK_I64; break;
    case CV_F64_LONG: case CV_F64_DOUBLE: r.key_kind = KK_F64; break;
    default: return r;
  }
  if (r.key_kind < 0) return r;
  if (!r.g.empty() && r.key_kind != KK_F32 && r.key_kind != KK_I32) return RatchetPlan();  // (K_gate: 32-bit keys)
  const int na0 = c.atom_begin[1] - c.atom_begin[0];
  if (na0 > RMAXF0) return r;
  for (int a = c.atom_begin[0]; a < c.atom_begin[1]; ++a) {
    const Atom& A = c.atoms[a];
    RatchetAtom ra{};
    ra.mask = A.mask;
    ra.f64 = A.f64;
    int64_t cst = 0;
    if (A.lk == OPK_CUR && A.rk == OPK_CONST) {
      ra.attr = c.col_attr[A.li]; ra.conv = c.col_conv[A.li]; ra.cur_left = 1; cst = A.rc;
    } else if (A.lk == OPK_CONST && A.rk == OPK_CUR) {
      ra.attr = c.col_attr[A.ri]; ra.conv = c.col_conv[A.ri]; ra.cur_left = 0; cst = A.lc;
    } else if (A.lk == OPK_CUR && A.rk == OPK_CUR && r.g.empty()) {  // (K_gate: constant atoms only)
      ra.attr = c.col_attr[A.li]; ra.conv = c.col_conv[A.li]; ra.cur_left = 1;
      ra.cur2 = 1; ra.attr2 = c.col_attr[A.ri]; ra.conv2 = c.col_conv[A.ri];
    } else {
      return r;  // null operands / constant-only atoms: leave them to K_chain
    }
    r.f0.push_back(ra);
    r.f0c.push_back(cst);
  }
  r.stream = c.state_stream[0];
  r.key_attr = c.col_attr[cur_col];
  r.key_conv = conv;
  r.xmask = mask;
  r.within = c.within;
  r.ok = true;
  return r;
}

}  // namespace eng
}  // namespace sdh
