// chain_pred.h -- K_chain's residual programs: what a state's filter holds beyond the pre-keyed compare
// atoms (or / not / is null / arithmetic, compares of computed values, a state's second and later
// capture-reading atoms), as postfix bytecode for kgen.h's stack machine. chain_lower.h writes the
// programs; nfa_chain.hip runs them on the lane that holds the event (tile residual) or the partial
// (partial residual). Written once for host and device (KG_FN), so tests/native runs the kernel's
// own lane body.
//
// A residual OP_ATTR is rewritten by the lowering so the kernel needs no search:
//   a = RA_CUR  b = column c of the ChainQuery's column table (conversion CV_RAW: the raw word)
//   a = RA_CAP  b = capture c of the partial
//   a = RA_NULL a chain index other than CURRENT / 0 of a one-event slot: reads null
// and res is the attribute's static type. A CONST carries its own immediate: the programs are per
// query, a wave runs one query, so instruction fetches and immediates are wave-uniform.
#pragma once
#include "kgen.h"

namespace sdh {
namespace cpred {

enum { RA_CUR = 0, RA_CAP = 1, RA_NULL = 2 };
constexpr int CMAXCODE = 48;  // residual instructions per query (all states, both kinds)

// code[b, e) over the operands cur(c, null&) / cap(c, null&), each returning the raw word (a 4-byte
// column's zero-extended, as the tile loads it). FilterProcessor.process:55-66: null and false drop.
// The stack is the register one: chain_lower.h refuses programs deeper than kg::RSTACK.
template <class Cur, class Cap>
KG_FN bool residual_pass(const kg::GInsn* code, int b, int e, Cur cur, Cap cap) {
  const kg::Val v = kg::eval_insns_imm<kg::RegStack>(
      code, [&](int pc) { return code[pc].imm; }, b, e,
      [&](const kg::GInsn& in) {
        kg::Val x{in.res, 1, 0};
        bool nul = true;
        int64_t raw = 0;
        if (in.a == RA_CUR) raw = cur((int)in.b, nul);
        else if (in.a == RA_CAP) raw = cap((int)in.b, nul);
        if (!nul) {
          x.null = 0;
          x.bits = in.res == kg::T_INT ? (int64_t)(int32_t)raw : in.res == kg::T_FLOAT ? (int64_t)(uint32_t)raw : raw;
        }
        return x;
      },
      [](const kg::GInsn&) { return false; });
  return kg::sp_true(v);
}

}  // namespace cpred
}  // namespace sdh
