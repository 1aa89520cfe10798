// nfa_part_chain.hip -- K_part's chain kind (PK_CHAIN: part_body.h chain_tile, part_chain.h) with the
// shape's filters interpreted; spec.hip compiles the same body with the filters as straight-line
// code. A unit of its own: in nfa_part.hip its instantiation shares the interpreter's functions with
// the count kernel and moves that kernel's register allocation (126 -> 137 VGPRs, 8 B of scratch).
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "part_body.h"

namespace sdh {

// the chain's filters interpreted: f1 reads the event (slot 0), f_s the event and the partial's
// earlier slots (chain_filter); the other kinds' filters are never called
struct PartChainInterp {
  static constexpr int kRegEntries = 0, kEW = 1;  // the whole table in the global state block
  static constexpr bool kHotRegs = false;         // (GMAXNA-wide hot rows would not stay in VGPRs)
  static constexpr int kNA = kg::GMAXNA, kOutW = 1536;
  struct K {};
  __device__ static void load(K&, const kg::GQuery*, const PartLaunch&, const int64_t*) {}
  __device__ static PartOffs offs(const PartLaunch& L) { return PartOffs{L.cmax, L.n_e1, L.n_first, L.n_last}; }
  __device__ static bool f1(const K&, const kg::GQuery* q, const kg::GQuery* ql, const PartLaunch& L, const PartEv& ev) {
    return chain_filter(q, ql, 0, ev, part_ent(GRef{nullptr}, 0, offs(L)));
  }
  __device__ static bool fa(const K&, const kg::GQuery*, const kg::GQuery*, const PartLaunch&, const PartEv&) { return false; }
  __device__ static bool fb(const K&, const kg::GQuery*, const kg::GQuery*, const PartLaunch&, const PartEv&) { return false; }
  __device__ static bool f2(const K&, const kg::GQuery*, const kg::GQuery*, const PartLaunch&, const PartEv&) { return false; }
  template <class En>
  __device__ static bool f3(const K&, const kg::GQuery*, const kg::GQuery*, const PartLaunch&, const PartEv&, const En&) {
    return false;
  }
  template <class En>
  __device__ static bool fs(const K&, const kg::GQuery* q, const kg::GQuery* ql, const PartLaunch&, int s,
                            const PartEv& ev, const En& en) {
    return chain_filter(q, ql, s, ev, en);
  }
};

__global__ __launch_bounds__(64) void nfa_part_chain_kernel(PartLaunch L) { part_body<PK_CHAIN, PartChainInterp>(L); }

}  // namespace sdh

extern "C" hipError_t sdh_launch_part_chain(const sdh::PartLaunch* L, hipStream_t s) {
  if (L->n_items <= 0) return hipSuccess;
  const dim3 grid(L->xcd ? (L->n_items + 7) & ~7 : L->n_items);
  hipLaunchKernelGGL(sdh::nfa_part_chain_kernel, grid, dim3(64), 0, s, *L);
  return hipGetLastError();
}
