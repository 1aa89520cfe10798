// select_lower.h -- host-side lowering of the queries' `select` lists (the IR's output programs,
// siddhi_amd/ir.py OutputIR) to the device selector's tables (select_body.h).
//
// Queries whose outputs are equal bytecode apart from CONST immediates share one shape -- what the
// filters do with kg::LaneConsts and the group templates: 10K patterns that differ in a threshold are
// one shape. The immediates go to a per-query table, and a CONST instruction of the shared table
// carries its index there.
#pragma once
#include <map>
#include <vector>

#include "gen_lower.h"
#include "select_body.h"

namespace sdh {
namespace sel {

struct Program {
  std::vector<kg::GInsn> code;
  std::vector<Out> outs;
  std::vector<Shape> shapes;
  std::vector<Query> queries;
  std::vector<int64_t> consts;
  std::vector<std::vector<int>> types;  // [query] the SDH_T_* type of each output
  int width = 0;                        // the most outputs any query has
  int max_depth = 0;
  int over = -1;                        // a query with more than MAXOUT outputs (-1: none)
  bool bad = false;                     // an output references a slot or attribute the program lacks
  Tables tables() const {
    return Tables{code.data(), outs.data(), shapes.data(), queries.data(), consts.data()};
  }
};

inline Program lower_select(const kg::LProgram& P) {
  Program S;
  std::map<std::vector<int64_t>, int> shape_of;
  for (size_t qi = 0; qi < P.q.size(); ++qi) {
    const auto& q = P.q[qi];
    Query Q{};
    Q.n_out = (int)q.outs.size();
    Q.const0 = (int64_t)S.consts.size();
    std::vector<int> ty;
    if (Q.n_out > MAXOUT) {
      if (S.over < 0) S.over = (int)qi;
      Q.n_out = 0;
      Q.shape = -1;
      S.queries.push_back(Q);
      S.types.push_back(ty);
      continue;
    }
    // the shape's signature: every instruction field but a CONST's immediate
    std::vector<int64_t> sig;
    for (const auto& c : q.outs) {
      sig.push_back((int64_t)c.size());
      for (const auto& in : c) {
        sig.insert(sig.end(), {in.op, in.lt, in.rt, in.res, in.a, in.b, in.op == kg::OP_CONST ? 0 : in.imm});
        if (in.op == kg::OP_CONST) S.consts.push_back(in.imm);
        if (in.op == kg::OP_ATTR || in.op == kg::OP_STREAM_IS_NULL) {
          if (in.a < 0 || in.a >= (int64_t)q.st.size()) S.bad = true;
          else if (in.op == kg::OP_ATTR &&
                   (in.imm < 0 || in.imm >= (int64_t)P.stream_types[q.st[in.a].stream].size()))
            S.bad = true;
        }
      }
      ty.push_back(c.empty() ? 0 : c.back().res);
    }
    S.width = std::max(S.width, Q.n_out);
    S.types.push_back(ty);
    auto it = shape_of.find(sig);
    if (it == shape_of.end()) {
      Shape sh{};
      sh.out0 = (int32_t)S.outs.size();
      sh.n_out = Q.n_out;
      int k = 0;
      for (const auto& c : q.outs) {
        Out o{};
        o.b = (int32_t)S.code.size();
        int depth = 0, maxd = 0;
        for (const auto& in : c) {
          kg::GInsn x{};
          x.op = (int8_t)in.op; x.lt = (int8_t)in.lt; x.rt = (int8_t)in.rt; x.res = (int8_t)in.res;
          x.a = (int32_t)in.a;
          x.b = in.b;
          x.imm = in.op == kg::OP_CONST ? k++ : in.imm;
          S.code.push_back(x);
          const int dd = kg::op_delta((int)in.op);
          if (dd == kg::OP_DELTA_BAD) S.bad = true;  // an opcode this build does not know
          else depth += dd;
          maxd = std::max(maxd, depth);
        }
        o.e = (int32_t)S.code.size();
        o.type = c.empty() ? 0 : c.back().res;
        o.direct = c.size() == 1 && c[0].op == kg::OP_ATTR;
        sh.depth = std::max(sh.depth, maxd);
        S.outs.push_back(o);
      }
      S.max_depth = std::max(S.max_depth, sh.depth);
      it = shape_of.emplace(sig, (int)S.shapes.size()).first;
      S.shapes.push_back(sh);
    }
    Q.shape = it->second;
    S.queries.push_back(Q);
  }
  return S;
}

}  // namespace sel
}  // namespace sdh
