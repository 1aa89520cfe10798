// engine_lower.hip -- the engine's callers of the host-side lowerings: the IR reader, the lowering of a
// linear chain query to a ChainQuery and K_ratchet plan selection (all three in chain_lower.h, which a
// host test builds too), and the select lists (select_lower.h).
#include "engine_int.h"

namespace sdh {
namespace eng {

// the pattern IR as the chain lowering reads it (chain_lower.h); a malformed blob is SDH_E_INVALID
IProgram read_ir(const void* blob, size_t len) {
  try {
    return read_chain_ir(blob, len);
  } catch (const kg::LowerError& ex) {
    throw Error(SDH_E_INVALID, ex.what());
  }
}

// chain_lower.h's lowering under this engine's knobs: SDH_CHAIN_PRED=0 declines every query that
// needs a residual program (they plan as before K_chain took general predicates: K_gen)
Lowered lower_chain(const IProgram& P, int qi) {
  bool residual = true;
  if (const char* v = sdh::knob("SDH_CHAIN_PRED")) residual = atoi(v) != 0;
  return lower_query(P, qi, residual);
}

// ------------------------------------------------------------------------------------------
// lowering: the queries' `select` lists -> the device selector's tables (select_lower.h): per query
// n_out, per output its code range and result type, the instructions in one table; shapes
// deduplicated, CONST immediates per query, single-OP_ATTR outputs marked for the direct load
// ------------------------------------------------------------------------------------------
sel::Program lower_outputs(const kg::LProgram& P) { return sel::lower_select(P); }

int attr_width(int t) {
  switch (t) {
    case T_INT: case T_FLOAT: case T_STRING: return 4;
    case T_BOOL: return 1;
    default: return 8;
  }
}

}  // namespace eng
}  // namespace sdh
