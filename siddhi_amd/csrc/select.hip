// select.hip -- the event store's append and the device selector (sdh_engine_poll_rows).
//
// The reference hands every completed StateEvent to QuerySelector.process (QuerySelector.java:76-169),
// which evaluates the `select` list and emits the output event. Here a poll does that for the whole
// window at once: one lane per match, in sdh_engine_poll's order, runs select_body.h over the match's
// slots and the event store, and writes the row column-major (each output column of a wave is one
// coalesced store).
//
// Event store: a row-major ring in HBM, event `seq` at row seq & (cap - 1) as W int64 words
// {ts, null bits, attribute words widened to the raw 64-bit encoding}. The projection reads events by
// a per-match index, so one event is one 8 * W-byte segment rather than one scattered access per column.
// The append runs once per push and writes rows by seq, so an exact re-run or a split push rewrites
// the same rows.
//
// Lanes of one wave may belong to queries of different shapes (select_lower.h): the wave loops over
// the distinct shapes present (the shape of the first pending lane, read into a scalar register; the
// lanes that have it run it), so the instruction fetch stays wave-uniform; the constants come from
// the lane's own query.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "nfa_types.h"
#include "select_body.h"

namespace sdh {

namespace {

inline unsigned grid(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

// one thread per (event, word): coalesced column reads, coalesced row writes
__global__ __launch_bounds__(256) void store_append_kernel(StreamBatch B, uint32_t float_mask,
                                                           int64_t* __restrict__ rows, int64_t mask, int W) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B.n * W) return;
  const int64_t i = idx / W;
  const int w = (int)(idx - i * W);
  int64_t v = 0;
  if (w == 0) {
    v = B.ts[i];
  } else if (w == 1) {
#pragma unroll
    for (int a = 0; a < MAXATTR; ++a)
      if (a < B.n_attr && B.nul[a] && B.nul[a][i]) v |= (int64_t)1 << a;
  } else {
#pragma unroll
    for (int a = 0; a < MAXATTR; ++a) {
      if (a != w - 2 || a >= B.n_attr) continue;
      if (B.width[a] == 8) v = static_cast<const int64_t*>(B.col[a])[i];
      else if (B.width[a] == 1) v = static_cast<const uint8_t*>(B.col[a])[i];
      else if ((float_mask >> a) & 1u) v = (int64_t)static_cast<const uint32_t*>(B.col[a])[i];
      else v = (int64_t)static_cast<const int32_t*>(B.col[a])[i];
    }
  }
  rows[sel::store_index(B.seq_base + i, mask, W, w)] = v;
}

// rows of seqs [lo, lo + n) from one ring into another (sdh_engine_retain_events growing the store)
__global__ __launch_bounds__(256) void store_relay_kernel(const int64_t* __restrict__ src, int64_t src_mask,
                                                          int64_t* __restrict__ dst, int64_t dst_mask, int W,
                                                          int64_t lo, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * W) return;
  const int64_t s = lo + idx / W;
  const int w = (int)(idx % W);
  dst[sel::store_index(s, dst_mask, W, w)] = src[sel::store_index(s, src_mask, W, w)];
}

struct SelArgs {
  sel::Tables T;
  sel::Store st;
  // sorted window: the match table through the poll's permutation, po_q = the sorted query column
  MatchTable M;
  const int32_t* perm;
  const int64_t* po_q;
  // placed window: K_ratchet's compact rows {query, e2 - seq_ref, e2 - e1, 0} and the window's event times
  const int32_t* crow;
  const int64_t* ts_log;
  int64_t seq_ref;
  int32_t cw, width;
  int64_t n;
  int32_t* oq;
  int64_t* ots;   // (placed: the sorted window's ts / seq columns come from the poll's gather)
  int64_t* oseq;
  int64_t* cells;
  uint64_t* nulls;
  int32_t* err;
};

template <bool DEEP, class Match>
__device__ __forceinline__ void select_lane(const SelArgs& A, int64_t i, int q, const Match& m) {
  const sel::Query Q = A.T.queries[q];
  const int64_t* qc = A.T.consts + Q.const0;
  int32_t err = 0;
  uint64_t nulls = 0;
  const int shape = Q.shape;
  bool todo = Q.n_out > 0;
  // (a wave-uniform loop: every round retires at least the lane whose shape it took)
  for (;;) {
    const uint64_t pend = __builtin_amdgcn_ballot_w64(todo);
    if (!pend) break;
    const int s = __builtin_amdgcn_readlane(shape, __builtin_ctzll(pend));
    if (todo && s == shape) {
      const sel::Shape sh = A.T.shapes[s];
      if (!DEEP || sh.depth <= kg::RSTACK)
        nulls = sel::project<kg::RegStack>(A.T, sh, qc, A.st, m, A.cells, A.n, i, err);
      else
        nulls = sel::project<kg::ArrStack>(A.T, sh, qc, A.st, m, A.cells, A.n, i, err);
      todo = false;
    }
  }
  for (int c = Q.n_out; c < A.width; ++c) A.cells[(int64_t)c * A.n + i] = 0;
  if (Q.n_out < 64) nulls |= ~0ull << Q.n_out;
  A.oq[i] = q;
  A.nulls[i] = nulls;
  if (err) atomicOr(A.err, err);
}

template <bool DEEP>
__global__ __launch_bounds__(256) void select_sorted_kernel(SelArgs A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int32_t p = A.perm[i];
  const sel::WordsMatch m{A.M.words + A.M.woff[p], A.M.wlen[p], A.M.ts[p]};
  select_lane<DEEP>(A, i, (int)A.po_q[i], m);
}

template <bool DEEP>
__global__ __launch_bounds__(256) void select_placed_kernel(SelArgs A) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int32_t* r = A.crow + i * A.cw;
  int q, d2, d1;
  if (A.cw == 4) {
    const int4 v = *reinterpret_cast<const int4*>(r);
    q = v.x; d2 = v.y; d1 = v.z;
  } else {
    q = r[0]; d2 = r[1]; d1 = r[2];
  }
  sel::PairMatch m;
  m.e2 = A.seq_ref + (int64_t)d2;
  m.e1 = m.e2 - (int64_t)d1;
  m.ts = A.ts_log[d2];
  A.ots[i] = m.ts;
  A.oseq[i] = m.e2;
  select_lane<DEEP>(A, i, q, m);
}

}  // namespace
}  // namespace sdh

using namespace sdh;

extern "C" hipError_t sdh_store_append(const StreamBatch* B, uint32_t float_mask, int64_t* rows, int64_t mask, int W,
                                       hipStream_t s) {
  if (B->n <= 0) return hipSuccess;
  hipLaunchKernelGGL(store_append_kernel, dim3(grid(B->n * W, 256)), dim3(256), 0, s, *B, float_mask, rows, mask, W);
  return hipGetLastError();
}

extern "C" hipError_t sdh_store_relay(const int64_t* src, int64_t src_mask, int64_t* dst, int64_t dst_mask, int W,
                                      int64_t lo, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(store_relay_kernel, dim3(grid(n * W, 256)), dim3(256), 0, s, src, src_mask, dst, dst_mask, W, lo, n);
  return hipGetLastError();
}

extern "C" hipError_t sdh_select_sorted(const sel::Tables* T, const sel::Store* st, int deep, MatchTable M,
                                        const int32_t* perm, const int64_t* po_q, int64_t n, int width, int32_t* oq,
                                        int64_t* cells, uint64_t* nulls, int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  SelArgs A{};
  A.T = *T; A.st = *st; A.M = M; A.perm = perm; A.po_q = po_q; A.n = n; A.width = width;
  A.oq = oq; A.cells = cells; A.nulls = nulls; A.err = err;
  if (deep) hipLaunchKernelGGL(select_sorted_kernel<true>, dim3(grid(n, 256)), dim3(256), 0, s, A);
  else hipLaunchKernelGGL(select_sorted_kernel<false>, dim3(grid(n, 256)), dim3(256), 0, s, A);
  return hipGetLastError();
}

extern "C" hipError_t sdh_select_placed(const sel::Tables* T, const sel::Store* st, int deep, const int32_t* crow,
                                        int cw, const int64_t* ts_log, int64_t seq_ref, int64_t n, int width,
                                        int32_t* oq, int64_t* ots, int64_t* oseq, int64_t* cells, uint64_t* nulls,
                                        int32_t* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  SelArgs A{};
  A.T = *T; A.st = *st; A.crow = crow; A.cw = cw; A.ts_log = ts_log; A.seq_ref = seq_ref; A.n = n; A.width = width;
  A.oq = oq; A.ots = ots; A.oseq = oseq; A.cells = cells; A.nulls = nulls; A.err = err;
  if (deep) hipLaunchKernelGGL(select_placed_kernel<true>, dim3(grid(n, 256)), dim3(256), 0, s, A);
  else hipLaunchKernelGGL(select_placed_kernel<false>, dim3(grid(n, 256)), dim3(256), 0, s, A);
  return hipGetLastError();
}
