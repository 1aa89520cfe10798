// chain_host.cpp -- test-only host build of K_chain's lowering (siddhi_amd/csrc/chain_lower.h) and of
// the lane body its kernels evaluate residual programs with (chain_pred.h). tests/chain_host.py builds
// it with its own compiler command and checks the lowering's decisions and, over events, a state's
// whole filter (atoms and residuals) against siddhi_amd/selector.py. Built with -DCHAIN_HOST_MAIN it
// is a stand-alone program that runs a table of residual programs once (for sanitizer builds).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siddhi_amd/csrc/chain_lower.h"

using namespace sdh;

namespace {
struct Host {
  eng::IProgram P;
  std::vector<eng::Lowered> L;  // by query; lowered on demand
  std::vector<int> mode;        // -1: not lowered yet, else the `allow_residual` it was lowered with
};

// the raw word of an attribute as a tile load reads it (4-byte columns zero-extend, bools are bytes)
int64_t raw_word(int type, int64_t v) {
  switch (type) {
    case T_INT: case T_FLOAT: case T_STRING: return (int64_t)(uint32_t)v;
    case T_BOOL: return v & 0xff;
    default: return v;
  }
}

// host twin of cmp_keys() in nfa_chain.hip
bool cmp_keys(int mask, int f64, int64_t l, int64_t r) {
  bool lt, gt, eq;
  if (f64) {
    double a, b;
    memcpy(&a, &l, 8);
    memcpy(&b, &r, 8);
    lt = a < b; gt = b < a; eq = a == b;
  } else {
    lt = l < r; gt = r < l; eq = l == r;
  }
  const bool v = (lt && (mask & CM_LT)) || (gt && (mask & CM_GT)) || (eq && (mask & CM_EQ));
  return v != ((mask & CM_NOT) != 0);
}

// State s's whole filter of lowered query L over slot events: vals / nulls [slot][na] (slot s is the
// current event). The atoms through host_key / cmp_keys, the two residuals through the kernels' lane body
bool state_pass(const eng::IProgram& P, int qi, const eng::Lowered& L, int s, const int64_t* vals, const uint8_t* nulls,
                int na) {
  const ChainQuery& c = L.cq;
  auto col_word = [&](int slot, int col, bool& nul) {
    const int a = c.col_attr[col];
    nul = nulls[slot * na + a] != 0;
    const int t = P.stream_types[(size_t)P.q[(size_t)qi].st[(size_t)slot].stream][(size_t)a];
    return raw_word(t, vals[slot * na + a]);
  };
  auto operand = [&](int k, int idx, int64_t cst, bool& nul) -> int64_t {
    nul = false;
    if (k == OPK_CONST) return cst;
    if (k == OPK_NULL) { nul = true; return 0; }
    const int slot = k == OPK_CUR ? s : c.cap_slot[idx];
    const int col = k == OPK_CUR ? idx : c.cap_col[idx];
    return eng::lower::host_key(col_word(slot, col, nul), c.col_conv[col]);
  };
  for (int a = c.atom_begin[s]; a < c.atom_begin[s + 1]; ++a) {
    const Atom& A = c.atoms[a];
    bool ln, rn;
    const int64_t l = operand(A.lk, A.li, A.lc, ln), r = operand(A.rk, A.ri, A.rc, rn);
    if (ln || rn || !cmp_keys(A.mask, A.f64, l, r)) return false;
  }
  auto cur = [&](int col, bool& nul) { return col_word(s, col, nul); };
  auto cap = [&](int idx, bool& nul) { return col_word(c.cap_slot[idx], c.cap_col[idx], nul); };
  if (c.rt_e[s] > c.rt_b[s] && !cpred::residual_pass(L.rcode.data(), c.rt_b[s], c.rt_e[s], cur, cap)) return false;
  if (c.rp_e[s] > c.rp_b[s] && !cpred::residual_pass(L.rcode.data(), c.rp_b[s], c.rp_e[s], cur, cap)) return false;
  return true;
}

const eng::Lowered& lowered(Host* h, int qi, int allow) {
  if (h->mode[(size_t)qi] != allow) {
    h->L[(size_t)qi] = eng::lower_query(h->P, qi, allow != 0);
    h->mode[(size_t)qi] = allow;
  }
  return h->L[(size_t)qi];
}
}  // namespace

extern "C" {

void* clh_create(const void* blob, size_t len) {
  try {
    Host* h = new Host;
    h->P = eng::read_chain_ir(blob, len);
    h->L.resize(h->P.q.size());
    h->mode.assign(h->P.q.size(), -1);
    return h;
  } catch (const std::exception&) {
    return nullptr;
  }
}
void clh_destroy(void* p) { delete static_cast<Host*>(p); }

// lowers query qi; out: [0] ok, [1] n_col, [2] n_cap, [3] n_xa, [4] atoms, [5] residual instructions,
// [6] K_ratchet / K_gate takes it, then per state s < 4 at [8 + 4 s]: xa_count, tile atoms (those that
// read no capture), tile residual length, partial residual length. Returns ok
int clh_lower(void* p, int qi, int allow_residual, int32_t* out) {
  Host* h = static_cast<Host*>(p);
  const eng::Lowered& L = lowered(h, qi, allow_residual);
  const ChainQuery& c = L.cq;
  for (int k = 0; k < 24; ++k) out[k] = 0;
  out[0] = L.ok;
  if (!L.ok) return 0;
  out[1] = c.n_col; out[2] = c.n_cap; out[3] = c.n_xa; out[4] = c.atom_begin[c.n_states];
  out[5] = (int32_t)L.rcode.size();
  out[6] = eng::ratchet_plan(c).ok;
  for (int s = 0; s < c.n_states; ++s) {
    out[8 + 4 * s] = c.xa_count[s];
    out[9 + 4 * s] = c.atom_begin[s + 1] - c.atom_begin[s] - c.xa_count[s];
    out[10 + 4 * s] = c.rt_e[s] - c.rt_b[s];
    out[11 + 4 * s] = c.rp_e[s] - c.rp_b[s];
  }
  return 1;
}
const char* clh_why(void* p, int qi, int allow_residual) {
  return lowered(static_cast<Host*>(p), qi, allow_residual).why.c_str();
}
// column c of the lowered query: [0] attribute, [1] conversion, [2] stream
void clh_col(void* p, int qi, int c, int32_t* out) {
  const ChainQuery& q = lowered(static_cast<Host*>(p), qi, 1).cq;
  out[0] = q.col_attr[c]; out[1] = q.col_conv[c]; out[2] = q.col_stream[c];
}

// state s's filter over n cases; case i's slot events are vals / nulls [i][slot < n_states][na]
void clh_state_pass(void* p, int qi, int s, int64_t n, const int64_t* vals, const uint8_t* nulls, int na, uint8_t* out) {
  Host* h = static_cast<Host*>(p);
  const eng::Lowered& L = lowered(h, qi, 1);
  const int S = L.cq.n_states;
  for (int64_t i = 0; i < n; ++i)
    out[i] = state_pass(h->P, qi, L, s, vals + i * S * na, nulls + i * S * na, na) ? 1 : 0;
}

}  // extern "C"

#ifdef CHAIN_HOST_MAIN
// stand-alone: residual programs written by hand over adversarial words, each checked against its value
// computed here in plain C++ (the Java rules of kgen.h restated), every arithmetic op with /0 and %0
int main() {
  using kg::GInsn;
  auto attr = [](int kind, int idx, int type) { GInsn g{}; g.op = kg::OP_ATTR; g.res = (int8_t)type; g.a = kind; g.b = idx; return g; };
  auto cst = [](int type, int64_t imm) { GInsn g{}; g.op = kg::OP_CONST; g.res = (int8_t)type; g.imm = imm; return g; };
  auto op2 = [](int op, int lt, int rt, int res, int64_t imm) {
    GInsn g{}; g.op = (int8_t)op; g.lt = (int8_t)lt; g.rt = (int8_t)rt; g.res = (int8_t)res; g.imm = imm; return g;
  };
  auto op1 = [](int op) { GInsn g{}; g.op = (int8_t)op; g.res = kg::T_BOOL; return g; };
  const int64_t ints[] = {0, 1, -1, 7, INT32_MAX, INT32_MIN, 16777217};
  int bad = 0, ran = 0;
  for (int64_t x : ints)
    for (int64_t y : ints)
      for (int ar = kg::AR_ADD; ar <= kg::AR_MOD; ++ar) {
        // cur.0 (int) `ar` cap.0 (int) > 3  or  cap.1 is null   -- cap.1 null in every other case
        const bool c1_null = ((x + y) & 1) != 0;
        const std::vector<GInsn> code{attr(cpred::RA_CUR, 0, kg::T_INT), attr(cpred::RA_CAP, 0, kg::T_INT),
                                      op2(kg::OP_ARITH, kg::T_INT, kg::T_INT, kg::T_INT, ar), cst(kg::T_INT, 3),
                                      op2(kg::OP_CMP, kg::T_INT, kg::T_INT, kg::T_BOOL, kg::CMP_GT),
                                      attr(cpred::RA_CAP, 1, kg::T_LONG), op1(kg::OP_IS_NULL),
                                      op2(kg::OP_OR, kg::T_BOOL, kg::T_BOOL, kg::T_BOOL, 0), op1(kg::OP_NOT), op1(kg::OP_NOT)};
        const bool got = cpred::residual_pass(
            code.data(), 0, (int)code.size(), [&](int, bool& nul) { nul = false; return (int64_t)(uint32_t)x; },
            [&](int c, bool& nul) { nul = c == 1 && c1_null; return c == 0 ? (int64_t)(uint32_t)y : (int64_t)5; });
        const int32_t a = (int32_t)x, b = (int32_t)y;
        bool vnull = false;
        int32_t v = 0;
        switch (ar) {
          case kg::AR_ADD: v = (int32_t)((uint32_t)a + (uint32_t)b); break;
          case kg::AR_SUB: v = (int32_t)((uint32_t)a - (uint32_t)b); break;
          case kg::AR_MUL: v = (int32_t)((uint32_t)a * (uint32_t)b); break;
          case kg::AR_DIV: if (b == 0) vnull = true; else v = (a == INT32_MIN && b == -1) ? INT32_MIN : a / b; break;
          default: if (b == 0) vnull = true; else v = b == -1 ? 0 : a % b;
        }
        const bool want = (!vnull && v > 3) || c1_null;
        ++ran;
        if (got != want) {
          std::printf("x %lld y %lld op %d: got %d want %d\n", (long long)x, (long long)y, ar, got, want);
          ++bad;
        }
      }
  // a null operand index (RA_NULL) and an empty range
  {
    const std::vector<GInsn> code{attr(cpred::RA_NULL, 0, kg::T_DOUBLE), op1(kg::OP_IS_NULL)};
    auto none = [](int, bool& nul) { nul = true; return (int64_t)0; };
    if (!cpred::residual_pass(code.data(), 0, 2, none, none)) { std::printf("RA_NULL is null: false\n"); ++bad; }
    if (cpred::residual_pass(code.data(), 0, 0, none, none)) { std::printf("empty program: true\n"); ++bad; }
    ran += 2;
  }
  std::printf(bad ? "FAILED\n" : "ok %d\n", ran);
  return bad != 0;
}
#endif
