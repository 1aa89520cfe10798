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
#include "rec_rows.h"
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


// ---- rows from device records (sdh_engine_records_rows; rec_rows.h) ----
// Window row A.out0 + k of the call is row first + k of its part; the kernels write only their part's
// rows of the window's arrays, so up to three launches fill one output.
struct RecArgs {
  int64_t first, n;   // the part's rows [first, first + n) ...
  int64_t out0;       // ... are the window's rows [out0, out0 + n)
  int64_t seq_base;
  // part 1: K_ratchet blocks
  const int64_t* match;
  int32_t blk_recs, wide;
  const int32_t* blk_count;
  const int32_t* blk_group;
  const int32_t* blk_side;
  const RatchetGroup* groups;
  const int64_t* row_off;  // [nb + 1]
  int64_t nb;
  // part 2: flat records by their word offsets
  const int64_t* flat;
  const int64_t* rec_off;
  // part 3: K_chain segments
  const int64_t* chain;
  const int64_t* seg_off;   // [items] first record
  const int64_t* seg_row;   // [items + 1] exclusive prefix of the segments' counts
  int64_t items;
  int32_t rec_words;
  const int32_t* qinfo;
};

// the trigger's ts word from the event store (what the table append takes from the batch)
__device__ __forceinline__ int64_t trigger_ts(const SelArgs& A, int64_t seq) {
  if (seq < A.st.lo) {
    atomicOr(A.err, (int32_t)sel::ERR_EVICTED);
    return 0;
  }
  return A.st.rows[sel::store_index(seq, A.st.mask, A.st.W, 0)];
}

// The last i in [0, n) with le(i), for a predicate that holds on a prefix of [0, n) that includes 0,
// found by the whole workgroup: each round the 256 threads probe 256 evenly spaced candidates at once
// and count the hits, so a table of n entries costs ceil(log256 n) dependent loads where a binary
// search costs log2 n (a workgroup does this before it can start: at 17,000 blocks 2 rounds for 15).
// Every thread of the workgroup calls it and gets the same answer.
template <class F>
__device__ __forceinline__ int64_t wg_last(int64_t n, F le) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t step = (hi - lo - 1 + 255) / 256;
    const int64_t p = lo + ((int64_t)threadIdx.x + 1) * step;
    const int c = __syncthreads_count(p < hi && le(p));
    const int64_t nh = lo + ((int64_t)c + 1) * step;
    lo += (int64_t)c * step;
    hi = nh < hi ? nh : hi;
  }
  return lo;
}

// One workgroup projects REC_RUN consecutive rows of part 1. It cuts them at block boundaries into runs
// of entries of one block. A rec4 run reads the side entries it needs once, coalesced, from the block's
// tail: each sets a head (its index) at its first entry of the run in LDS and leaves its trigger there,
// and a max-scan over the heads (per wave by lane shifts, across waves through LDS) carries the index
// forward, so an entry costs one LDS read where ratchet_record searches the side entries
// (SEARCH: that search per entry, for the A/B). Entries are read as coalesced dwords.
constexpr int REC_RUN = 4096;
constexpr int REC_SIDE = REC_RUN + 64;  // side entries of a run kept in LDS (more: read from the block)

template <bool DEEP, bool SEARCH>
__global__ __launch_bounds__(256) void select_ratchet_records_kernel(SelArgs A, RecArgs R) {
  __shared__ int32_t s_head[REC_RUN];
  __shared__ uint32_t s_e2[REC_SIDE];
  __shared__ int32_t s_wmax[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t k0 = (int64_t)blockIdx.x * REC_RUN;  // index in [0, R.n)
  const int64_t k1 = k0 + REC_RUN < R.n ? k0 + REC_RUN : R.n;
  if (k0 >= k1) return;
  const int64_t row0 = R.first + k0;
  int64_t b = wg_last(R.nb, [&](int64_t i) { return R.row_off[i] <= row0; });  // (rr::locate)
  const int64_t blk_bytes = (int64_t)R.blk_recs * 8 << (R.wide ? 1 : 0);
  while (k0 < k1 && b < R.nb) {  // (wave- and workgroup-uniform)
    const int64_t r0 = R.row_off[b];
    const int cnt = R.blk_count[b];
    const int64_t row = R.first + k0;
    if (row >= r0 + cnt) {  // an empty block
      ++b;
      continue;
    }
    const int i0 = (int)(row - r0);
    const int len = (int)(cnt - i0 < k1 - k0 ? cnt - i0 : k1 - k0);
    const int ns = R.blk_side[b];
    const char* B = reinterpret_cast<const char*>(R.match) + (size_t)b * blk_bytes;
    const RatchetGroup* G = R.groups + R.blk_group[b];
    const bool expand = ns >= 0 && !SEARCH;
    int j0 = 0;
    if (expand) {
      // (rr::side_of(i0); the side entries ascend by first, so each thread stops at its first one past the run)
      j0 = (int)wg_last(ns, [&](int64_t j) { return (int)rr::side_entry(B, blk_bytes, (int)j)[0] <= i0; });
      for (int p = tid; p < len; p += 256) s_head[p] = -1;
      __syncthreads();
      for (int j = j0 + tid; j < ns; j += 256) {
        const uint2 se = *reinterpret_cast<const uint2*>(rr::side_entry(B, blk_bytes, j));
        if ((int)se.x >= i0 + len) break;
        const int p = rr::head_slot(se.x, i0);
        if (p < len) atomicMax(&s_head[p], j);
        if (j - j0 < REC_SIDE) s_e2[j - j0] = se.y;
      }
      __syncthreads();
    }
    int carry = j0;
    for (int c = 0; c < len; c += 256) {
      const int p = c + tid;
      const bool live = p < len;
      uint32_t e2off = 0;
      if (expand) {
        int v = live ? s_head[p] : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(v, o);
          if (lane >= o) v = v > t ? v : t;
        }
        const int par = (c >> 8) & 1;
        if (lane == 63) s_wmax[par][wv] = v;
        __syncthreads();
        int pre = carry;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int t = s_wmax[par][w];
          if (w < wv) pre = pre > t ? pre : t;
          carry = carry > t ? carry : t;
        }
        v = v > pre ? v : pre;
        if (live) e2off = v - j0 < REC_SIDE ? s_e2[v - j0] : rr::side_entry(B, blk_bytes, v)[1];
      }
      if (live) {
        const int i = i0 + p;
        rr::Pair pr;
        if (ns >= 0) {
          if (SEARCH) e2off = rr::side_entry(B, blk_bytes, rr::side_of(B, blk_bytes, ns, i))[1];
          pr = rr::pair_rec4(reinterpret_cast<const uint32_t*>(B)[i], e2off, R.seq_base);
        } else if (!R.wide) {
          const uint2 r = reinterpret_cast<const uint2*>(B)[i];
          pr = rr::pair_rec8(r.x, r.y, R.seq_base);
        } else {
          const uint4 r = reinterpret_cast<const uint4*>(B)[i];
          pr = rr::pair_rec16(r.x, r.y, r.z, R.seq_base);
        }
        sel::PairMatch m;
        m.e1 = pr.e1;
        m.e2 = pr.e2;
        m.ts = trigger_ts(A, pr.e2);
        const int64_t o = R.out0 + k0 + p;
        A.ots[o] = m.ts;
        A.oseq[o] = m.e2;
        select_lane<DEEP>(A, o, G->qid[pr.ln], m);
      }
    }
    __syncthreads();  // (the next run reuses the heads)
    k0 += len;
    ++b;
  }
}

// one lane per flat record of the window (rec_off: flat_heads_kernel)
template <bool DEEP>
__global__ __launch_bounds__(256) void select_flat_records_kernel(SelArgs A, RecArgs R) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= R.n) return;
  rr::FlatMatch m;
  int q = 0;
  int64_t seq = 0;
  bool own = false;
  if (!rr::flat_open(R.flat + R.rec_off[R.first + k], R.seq_base, m, q, seq, own)) return;  // (no head is a pad)
  if (!own) m.ts = trigger_ts(A, seq);
  const int64_t o = R.out0 + k;
  A.ots[o] = m.ts;
  A.oseq[o] = seq;
  select_lane<DEEP>(A, o, q, m);
}

// one lane per K_chain record of the window
template <bool DEEP>
__global__ __launch_bounds__(256) void select_chain_records_kernel(SelArgs A, RecArgs R) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= R.n) return;
  const int64_t row = R.first + k;
  const int64_t it = rr::locate(R.seg_row, R.items, row);
  const int64_t* v = R.chain + (R.seg_off[it] + (row - R.seg_row[it])) * R.rec_words;
  const int q = (int)v[0];
  int S = R.qinfo[2 * q];
  if (S > R.rec_words - 2) S = R.rec_words - 2;
  rr::ChainMatch m{v, S, v[1]};
  const int64_t o = R.out0 + k;
  A.ots[o] = m.ts;
  A.oseq[o] = S > 0 ? v[2 + S - 1] : 0;
  select_lane<DEEP>(A, o, q, m);
}

// The heads of the flat records: device-record mode keeps no record index (dev_common.h LaneOut), and a
// record is found only by walking the buffer from its start by each first word's span. The walk is a
// chain of dependent reads, so it is cut into tiles of HEAD_TILE words and made in three passes:
//   flat_hops_kernel  (one workgroup per tile) takes EVERY word of its tile as a possible head and finds,
//                     by pointer doubling in LDS, where a walk entering the tile at that word would leave
//                     it (its offset into the words after the tile) and how many records it would pass;
//   flat_chain_kernel (one lane) follows that table from word 0: one dependent read per tile instead of
//                     one per record, giving each tile its true entry word and its first record's index;
//   flat_heads_kernel (one workgroup per tile) walks its tile from that entry in LDS and lists the heads.
// Pads are stepped over and not listed.
constexpr int HEAD_TILE = 4096;
constexpr int HEAD_SINK = HEAD_TILE;  // the hop of a word whose record ends past the tile

__global__ __launch_bounds__(256) void flat_hops_kernel(const int64_t* __restrict__ out, int64_t words,
                                                        uint32_t* __restrict__ exit_off, uint16_t* __restrict__ passed) {
  __shared__ uint16_t nx[2][HEAD_TILE + 1];
  __shared__ uint16_t ct[2][HEAD_TILE + 1];
  __shared__ uint32_t ex[2][HEAD_TILE + 1];
  const int64_t base = (int64_t)blockIdx.x * HEAD_TILE;
  for (int i = threadIdx.x; i <= HEAD_TILE; i += 256) {
    int n = HEAD_SINK, c = 0;
    uint32_t e = 0;
    if (i < HEAD_TILE && base + i < words) {
      const int64_t w0 = out[base + i];
      const int64_t to = (int64_t)i + rr::rec_span(w0);
      c = rr::rec_kind(w0) != rr::KIND_PAD;
      if (to < HEAD_TILE) n = (int)to;
      else e = (uint32_t)(to - HEAD_TILE);
    }
    nx[0][i] = (uint16_t)n;
    ct[0][i] = (uint16_t)c;
    ex[0][i] = e;
  }
  __syncthreads();
  int cur = 0;
  // (a hop moves at least one word on, so 2^12 hops leave a tile of 2^12 words; the sink hops to itself)
  for (int r = 0; r < 12; ++r) {
    for (int i = threadIdx.x; i <= HEAD_TILE; i += 256) {
      const int n = nx[cur][i];
      nx[cur ^ 1][i] = nx[cur][n];
      ct[cur ^ 1][i] = (uint16_t)(ct[cur][i] + ct[cur][n]);
      ex[cur ^ 1][i] = ex[cur][i] + ex[cur][n];
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int i = threadIdx.x; i < HEAD_TILE; i += 256) {
    if (base + i >= words) break;
    exit_off[base + i] = ex[cur][i];
    passed[base + i] = ct[cur][i];
  }
}

__global__ void flat_chain_kernel(const uint32_t* __restrict__ exit_off, const uint16_t* __restrict__ passed,
                                  int64_t words, int64_t tiles, int64_t* __restrict__ tile_entry,
                                  int64_t* __restrict__ tile_first, unsigned long long* n_out) {
  if (blockIdx.x || threadIdx.x) return;
  int64_t entry = 0, n = 0;  // entry: the walk's position, as an offset into tile t
  for (int64_t t = 0; t < tiles; ++t) {
    tile_entry[t] = entry;
    tile_first[t] = n;
    const int64_t at = t * HEAD_TILE + entry;
    if (entry >= HEAD_TILE || at >= words) {  // a record or pad covers this tile
      entry -= HEAD_TILE;
      continue;
    }
    n += passed[at];
    entry = exit_off[at];
  }
  *n_out = (unsigned long long)n;
}

__global__ __launch_bounds__(64) void flat_heads_kernel(const int64_t* __restrict__ out, int64_t words,
                                                        const int64_t* __restrict__ tile_entry,
                                                        const int64_t* __restrict__ tile_first,
                                                        int64_t* __restrict__ rec_off, int64_t cap) {
  __shared__ int64_t tile[HEAD_TILE];
  const int64_t base = (int64_t)blockIdx.x * HEAD_TILE;
  const int64_t entry = tile_entry[blockIdx.x];
  if (entry >= HEAD_TILE) return;  // (uniform)
  for (int t = threadIdx.x; t < HEAD_TILE; t += 64) tile[t] = base + t < words ? out[base + t] : 0;
  __syncthreads();
  if (threadIdx.x) return;
  const int end = (int)(base + HEAD_TILE < words ? HEAD_TILE : words - base);
  int64_t n = tile_first[blockIdx.x];
  for (int pos = (int)entry; pos < end;) {
    const int64_t w0 = tile[pos];
    if (rr::rec_kind(w0) != rr::KIND_PAD) {
      if (n < cap) rec_off[n] = base + pos;
      ++n;
    }
    const int64_t span = rr::rec_span(w0);
    if (span >= HEAD_TILE) break;
    pos += (int)span;
  }
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

// sdh_engine_records_rows: part `part` (0 K_ratchet blocks, 1 flat records, 2 K_chain segments) of a
// window; search != 0: the per-entry side search instead of the side-run expansion (A/B only)
extern "C" hipError_t sdh_select_records(const sel::Tables* T, const sel::Store* st, int deep, int part, int search,
                                         const sdh::RecRows* R, int64_t n_out, int width, int32_t* oq, int64_t* ots,
                                         int64_t* oseq, int64_t* cells, uint64_t* nulls, int32_t* err,
                                         hipStream_t s) {
  if (R->n <= 0) return hipSuccess;
  SelArgs A{};
  A.T = *T; A.st = *st; A.n = n_out; A.width = width;
  A.oq = oq; A.ots = ots; A.oseq = oseq; A.cells = cells; A.nulls = nulls; A.err = err;
  RecArgs K{};
  K.first = R->first; K.n = R->n; K.out0 = R->out0; K.seq_base = R->seq_base;
  K.match = R->match; K.blk_recs = R->blk_recs; K.wide = R->wide; K.blk_count = R->blk_count;
  K.blk_group = R->blk_group; K.blk_side = R->blk_side; K.groups = R->groups; K.row_off = R->row_off; K.nb = R->nb;
  K.flat = R->flat; K.rec_off = R->rec_off;
  K.chain = R->chain; K.seg_off = R->seg_off; K.seg_row = R->seg_row; K.items = R->items;
  K.rec_words = R->rec_words; K.qinfo = R->qinfo;
  if (part == 0) {
    const dim3 g(grid(K.n, REC_RUN));
    if (search) hipLaunchKernelGGL((select_ratchet_records_kernel<false, true>), g, dim3(256), 0, s, A, K);
    else if (deep) hipLaunchKernelGGL((select_ratchet_records_kernel<true, false>), g, dim3(256), 0, s, A, K);
    else hipLaunchKernelGGL((select_ratchet_records_kernel<false, false>), g, dim3(256), 0, s, A, K);
  } else if (part == 1) {
    if (deep) hipLaunchKernelGGL(select_flat_records_kernel<true>, dim3(grid(K.n, 256)), dim3(256), 0, s, A, K);
    else hipLaunchKernelGGL(select_flat_records_kernel<false>, dim3(grid(K.n, 256)), dim3(256), 0, s, A, K);
  } else {
    if (deep) hipLaunchKernelGGL(select_chain_records_kernel<true>, dim3(grid(K.n, 256)), dim3(256), 0, s, A, K);
    else hipLaunchKernelGGL(select_chain_records_kernel<false>, dim3(grid(K.n, 256)), dim3(256), 0, s, A, K);
  }
  return hipGetLastError();
}

// temp: sdh_flat_heads_temp(words) bytes
extern "C" size_t sdh_flat_heads_temp(int64_t words) {
  const int64_t tiles = (words + HEAD_TILE - 1) / HEAD_TILE;
  return (size_t)words * 4 + (((size_t)words * 2 + 7) & ~(size_t)7) + (size_t)tiles * 16 + 64;
}
extern "C" hipError_t sdh_flat_heads(const int64_t* out, int64_t words, void* temp, int64_t* rec_off, int64_t cap,
                                     unsigned long long* n_out, hipStream_t s) {
  if (words <= 0) return hipMemsetAsync(n_out, 0, 8, s);
  const int64_t tiles = (words + HEAD_TILE - 1) / HEAD_TILE;
  // (8-byte parts first: the tile tables, then the per-word tables)
  int64_t* tile_entry = static_cast<int64_t*>(temp);
  int64_t* tile_first = tile_entry + tiles;
  uint32_t* exit_off = reinterpret_cast<uint32_t*>(tile_first + tiles);
  uint16_t* passed = reinterpret_cast<uint16_t*>(exit_off + words);
  hipLaunchKernelGGL(flat_hops_kernel, dim3((unsigned)tiles), dim3(256), 0, s, out, words, exit_off, passed);
  hipLaunchKernelGGL(flat_chain_kernel, dim3(1), dim3(64), 0, s, exit_off, passed, words, tiles, tile_entry, tile_first,
                     n_out);
  hipLaunchKernelGGL(flat_heads_kernel, dim3((unsigned)tiles), dim3(64), 0, s, out, words, tile_entry, tile_first, rec_off,
                     cap);
  return hipGetLastError();
}
