// nfa_chain.hip -- NFA-step kernel (K1 + K2 + K3 of SURVEY §2) for chain-family queries:
//
//     every? e0=S[f0] -> e1=S[f1(e0)] -> ... -> e{n-1}=S[f{n-1}(...)] [within T]
//
// Semantics restated from the reference (state/ = siddhi-core .../query/input/stream/state/):
//   * one pending partial per (pattern, trigger) -- StreamPreStateProcessor.processAndReturn:292-337
//   * a partial added during event j becomes pending for event j+1 (two-phase newAndEvery ->
//     pending promotion, :203-227,281-289; multi-stream receivers process states in reverse
//     registration order, PatternMultiProcessStreamReceiver.java:38-44) -- here: states are swept
//     from the last to the first, so an advanced partial is never seen twice for one event
//   * lazy `within` expiry measured against the start slot (isExpired:102-113), checked before
//     the filter, only on non-start states
//   * start state with `every` keeps its (stateless) seed forever (StreamPostStateProcessor:66-68
//     re-arms a shallow clone); without `every` the seed is consumed by its first match (R3)
//   * the last state emits (isEventReturned, :310-313) and drops the partial (stateChanged)
//   * predicates: conjunctions of typed compares, null -> false (FilterProcessor:55-66,
//     CompareConditionExpressionExecutor:39-43), evaluated in Java's promotion domain; conjuncts that
//     are more than a compare of two operands (or / not / is null / arithmetic) run as residual
//     programs through kgen.h's stack machine (chain_pred.h; the R = true kernels)
//
// Mapping to CDNA4: one 64-lane wave owns one (query instance, event chunk); each lane holds one
// partial match in registers (K register sets -> 64*K partials). Every 64 events the wave stages
// a tile in its private LDS region: one coalesced load per attribute column, converted once per
// event into compare-domain keys (f64 or i64), so the per-event predicate is a branch-free pair of
// compares read by wave-uniform (broadcast) LDS loads. New partials take the first free lane
// (ctz of the inverted live-lane ballot); matches are compacted with ballot + mbcnt into the
// wave's contiguous output segment. No MFMA: the step is compare/branch work.
//
// Exactness of event-chunk parallelism: for chunkable queries (every on the start
// state, within T, one input stream) chunk c > 0 re-derives its start state by replaying the
// events from w0 = lower_bound(ts, ts[c0-1] - T) without emitting; any partial older than w0
// has expired by event c0-1. Requires non-decreasing timestamps, which every wave verifies on
// the range it reads (err[1]); the host re-runs the batch unchunked otherwise.
//
// Paged form (nfa_chain_paged_kernel; more than 512 partials per query -- 256 in an engine with a
// residual program, engine_int.h chain_reg_limit -- or SDH_CHAIN_PAGED, or an interleaved push, whose
// MIX = true instantiations are described at the kernel): the
// reference's pending lists are unbounded (StreamPreStateProcessor.java:59-60, :203-216, walked in
// full at :298) and registers end at 64 * 8 partials, so past that the table stays in HBM, same
// field-major layout, in pages of 64 entries (one coalesced load per field). The walk is entry-major
// per 64-event tile: the tile is staged as above, then every live page is loaded into one register
// set, sees the tile's events in order, and is stored back compacted; the partials the seed opens
// in the tile form one fresh page -- lane k holds the one opened at event k, takes part in the
// events after k only -- whose survivors are appended at the tail. The register form walks
// event-major (each event through every partial). Both give the same matches and the same state:
//   * a chain partial's fate depends on the events and its own words only: no partial reads another,
//     and the seed is stateless (`every` re-arms it unchanged; without `every` the first passing
//     event consumes it, which the staged smask[0] alone decides);
//   * each partial sees the same events in the same order in both walks: a partial opened or
//     advanced at event j is next examined at j + 1 (states are swept last to first, so the advanced
//     partial is not seen again at j; the fresh page's lane k joins after event k's sweep), and a page
//     runs the tile's events k = 0 .. cnt-1 in order, tiles in order; so lazy expiry (checked when an
//     event of the state's stream arrives, before the filter) fires at the same event as well;
//   * what differs is the order in which the matches of one push leave the kernel (page by page,
//     not event by event) and the lanes the survivors end in. Neither is observable: the match table
//     orders rows by trigger seq, receiver rank and the slot seqs (nfa_types.h, MatchTable), device
//     records promise no order within a segment (include/siddhi_hip.h), and a table lane's index
//     is read by nothing.
// Stores go to a write cursor that never passes the read cursor (a page stores at most the 64 entries
// it loaded, from registers), so the table is compacted in place: the first tile of an item that
// continues the persisted state reads part[inb] (holes allowed) and writes the working table, later
// tiles read and write the working table. The working table of a query's last chunk is part[1 - inb];
// the earlier chunks' are scratch tables of the same capacity (a chunk's live partials are a subset of
// the unchunked run's at the same event, so no chunk needs more than the table does). A tail past the
// capacity sets err[0], and the item goes on counting what it could not store (err[3]), so the host
// re-runs the push once at a size that fits -- part[inb] is read, never written, until then.
#include <hip/hip_runtime.h>

#include "chain_pred.h"
#include "launchers.h"
#include "nfa_types.h"

namespace sdh {

__device__ __forceinline__ int wave_mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int64_t rfl64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Number.floatValue()/doubleValue()/longValue() into the compare domain (see enum Conv)
__device__ __forceinline__ int64_t to_key(uint64_t raw, int conv) {
  switch (conv) {
    case CV_I64_INT: return (int64_t)(int32_t)(uint32_t)raw;
    case CV_I64_LONG: return (int64_t)raw;
    case CV_F32_INT: return __double_as_longlong((double)(float)(int32_t)(uint32_t)raw);
    case CV_F32_LONG: return __double_as_longlong((double)(float)(int64_t)raw);
    case CV_F32_FLOAT:
    case CV_F64_FLOAT: return __double_as_longlong((double)__uint_as_float((uint32_t)raw));
    case CV_F64_INT: return __double_as_longlong((double)(int32_t)(uint32_t)raw);
    case CV_F64_LONG: return __double_as_longlong((double)(int64_t)raw);
    default: return (int64_t)raw;  // CV_F64_DOUBLE, CV_RAW
  }
}

// typed compare of two keys: ((lt & b0) | (gt & b1) | (eq & b2)) ^ b3 -- IEEE semantics for f64
// keys (NaN: only != holds), exactly Java's primitive compares
__device__ __forceinline__ bool cmp_keys(int mask, int f64, int64_t l, int64_t r) {
  bool lt, gt, eq;
  if (f64) {
    const double a = __longlong_as_double(l), b = __longlong_as_double(r);
    lt = a < b;
    gt = b < a;
    eq = a == b;
  } else {
    lt = l < r;
    gt = r < l;
    eq = l == r;
  }
  const bool v = (lt && (mask & CM_LT)) || (gt && (mask & CM_GT)) || (eq && (mask & CM_EQ));
  return v != ((mask & CM_NOT) != 0);
}

// Math.abs(a - b) > within with Java long wrap-around (Math.abs(Long.MIN_VALUE) < 0)
__device__ __forceinline__ bool expired(int64_t t0, int64_t t, int64_t within) {
  int64_t d = (int64_t)((uint64_t)t0 - (uint64_t)t);
  int64_t a = d < 0 ? (int64_t)(0ull - (uint64_t)d) : d;
  return a > within;
}

// one register set of partial matches: lane l of set k holds partial 64*k + l
struct PSet {
  int st;                  // state id the partial is pending at, -1 = free lane
  int64_t ts0;             // timestamp of the start-state event (within reference)
  int64_t sq[MAXS - 1];    // event sequence number per filled slot
  int64_t cp[MAXCAP];      // captured operand keys read by later filters
  uint32_t cn;             // captured-null bits
};

__device__ __forceinline__ int64_t cap_get(const PSet P, int idx) {
  int64_t v = P.cp[0];
#pragma unroll
  for (int c = 1; c < MAXCAP; ++c) v = (idx == c) ? P.cp[c] : v;
  return v;
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int k) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, k);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), k);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// one atom on per-lane operands (tile time: lane = event; step time: lane = partial)
__device__ __forceinline__ bool atom_eval(const Atom& A, int64_t l, bool ln, int64_t r, bool rn) {
  return !ln && !rn && cmp_keys(A.mask, A.f64, l, r);
}

// first index i in [0, c0) with ts[i] >= target (64-ary search, all lanes cooperate)
__device__ int64_t lower_bound_ts(const int64_t* ts, int64_t c0, int64_t target, int lane) {
  int64_t lo = 0, hi = c0;  // answer in [lo, hi]
  while (hi - lo > 1) {
    const int64_t span = hi - lo;
    const int64_t p = lo + (span * lane) / WAVE;  // probe positions, p < hi
    const uint64_t m = __ballot(ts[p] < target);
    const int nb = __popcll(m);                   // ts is sorted: the first nb probes are below
    const int64_t nlo = nb == 0 ? lo : lo + (span * (nb - 1)) / WAVE + 1;
    const int64_t nhi = nb == WAVE ? hi : lo + (span * nb) / WAVE;
    lo = rfl64(nlo);
    hi = rfl64(nhi);
    if (lo == hi) break;
  }
  if (lo < c0 && ts[lo] < target) lo = lo + 1;
  return lo;
}

// Per-state predicate/capture descriptor, resolved once per wave into SGPRs so that the event
// loop carries no data-dependent decisions about the query's shape.
struct StateDesc {
  int active;        // state fed by this launch's stream
  int has_x;         // state has a capture-reading atom (at most one: chain_lower.h sends a state's
                     // further capture readers to its partial residual)
  int l_cap, r_cap;  // operand is a captured value (index in lcap/rcap)
  int l_cur, r_cur;  // operand is the current event (key in xcur)
  int lcap, rcap;
  int64_t lc, rc;    // constant keys (used when neither CAP nor CUR)
  int l_null, r_null;
  int f64, mask;
  uint32_t capmask;  // captures taken when a partial passes this state
  int rp_b, rp_e;    // R kernels: the state's partial residual, instructions [rp_b, rp_e) of rcode
};

// The residual hooks of the R = true kernels (chain_pred.h). Tile residual, lane = event: the lane's
// own raw column words and null bits. Partial residual, lane = partial: the current event's words are
// wave-uniform (readlane of the staged column at k), the captures the lane's own. partial_residual is
// called with every lane active: lane k computes the word the others read from it.
template <class ColKey>
__device__ __forceinline__ bool tile_residual(const kg::GInsn* code, int b, int e, const ColKey& col_key, uint32_t cnul) {
  return cpred::residual_pass(
      code, b, e, [&](int c, bool& nul) { nul = (cnul >> c) & 1u; return col_key(c); },
      [](int, bool& nul) { nul = true; return (int64_t)0; });
}
// (a partial's captures as named words, by value: an array behind a reference stays in private memory)
struct Caps {
  int64_t c0, c1, c2, c3;
  uint32_t cn;
};
static_assert(MAXCAP == 4, "Caps names the captures");
__device__ __forceinline__ Caps caps_of(const PSet& P) { return Caps{P.cp[0], P.cp[1], P.cp[2], P.cp[3], P.cn}; }
template <class ColKey>
__device__ __forceinline__ bool partial_residual(const kg::GInsn* code, int b, int e, const ColKey& col_key,
                                                 const uint32_t cnul_k, const int k, const Caps C) {
  return cpred::residual_pass(
      code, b, e, [&](int c, bool& nul) { nul = (cnul_k >> c) & 1u; return readlane64(col_key(c), k); },
      [&](int c, bool& nul) {
        nul = (C.cn >> c) & 1u;
        return c == 1 ? C.c1 : c == 2 ? C.c2 : c == 3 ? C.c3 : C.c0;
      });
}

template <int S, int K, bool R>
__global__ __launch_bounds__(256) void nfa_chain_kernel(ChainLaunch L) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + wv;
  if (wid >= L.n_work) return;
  const WorkItem W = L.work[wid];
  const ChainQuery* __restrict__ Q = L.queries + W.q;
  const int stream = L.b.stream;
  const int pcap = L.pcap;
  // ---- wave-uniform program, resolved into SGPRs for the whole chunk ----
  const int64_t within = Q->within < 0 ? INT64_MAX : Q->within;
  const int every = Q->every, n_cap = Q->n_cap, qid = Q->qid, n_col = Q->n_col;
  StateDesc D[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    StateDesc d{};
    d.active = Q->state_stream[s] == stream;
    d.has_x = Q->xa_count[s] > 0;
    if (d.has_x) {
      const Atom& A = Q->atoms[Q->xa_atom[Q->xa_first[s]]];
      d.l_cap = A.lk == OPK_CAP; d.r_cap = A.rk == OPK_CAP;
      d.l_cur = A.lk == OPK_CUR; d.r_cur = A.rk == OPK_CUR;
      d.lcap = d.l_cap ? A.li : 0; d.rcap = d.r_cap ? A.ri : 0;
      d.lc = A.lc; d.rc = A.rc;
      d.l_null = A.lk == OPK_NULL; d.r_null = A.rk == OPK_NULL;
      d.f64 = A.f64; d.mask = A.mask;
    }
    uint32_t cm = 0;
    for (int c = 0; c < n_cap; ++c) cm |= (Q->cap_slot[c] == s ? 1u : 0u) << c;
    d.capmask = cm;
    if constexpr (R) {
      d.rp_b = Q->rp_b[s];
      d.rp_e = Q->rp_e[s];
    }
    D[s] = d;
  }

  // ---- start state: persisted table (chunk 0 / window reaching the batch start) or replay ----
  int64_t w0 = 0;
  if (W.chunk > 0) w0 = lower_bound_ts(L.b.ts, W.c0, L.b.ts[W.c0 - 1] - within, lane);
  PSet P[K];
  int seed_alive = 1;
  if (w0 == 0) {
    const int64_t* pin = L.part[W.inb] + (size_t)W.q * NF * pcap;
    seed_alive = L.hdr[W.inb][W.q].seed_alive;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      const int li = kk * WAVE + lane;
      P[kk].st = (int)pin[F_STATE * pcap + li];
      P[kk].ts0 = pin[F_TS0 * pcap + li];
#pragma unroll
      for (int s = 0; s < MAXS - 1; ++s) P[kk].sq[s] = pin[(F_SEQ0 + s) * pcap + li];
#pragma unroll
      for (int c = 0; c < MAXCAP; ++c) P[kk].cp[c] = pin[(F_CAP0 + c) * pcap + li];
      P[kk].cn = (uint32_t)pin[F_CAPNULL * pcap + li];
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      P[kk].st = -1;
      P[kk].ts0 = 0;
#pragma unroll
      for (int s = 0; s < MAXS - 1; ++s) P[kk].sq[s] = 0;
#pragma unroll
      for (int c = 0; c < MAXCAP; ++c) P[kk].cp[c] = 0;
      P[kk].cn = 0;
    }
  }

  int64_t nmatch = 0;
  int64_t* seg = L.match + W.seg_off * L.rec_words;
  const int RW = L.rec_words;
  bool unordered = false, overflow = false, seg_over = false;
  int64_t prev_tile_ts = (w0 == 0) ? L.b.prev_ts : L.b.ts[w0 - 1];

  for (int64_t t = w0; t < W.c1; t += WAVE) {
    // ---- stage 64 events, one per lane: coalesced column loads converted once into
    //      compare-domain keys; partial-independent atoms evaluated for the whole tile ----
    const int64_t e = t + lane;
    const bool live = e < W.c1;
    const int64_t ets = live ? L.b.ts[e] : INT64_MAX;
    int64_t ck[MAXCOL];
    uint32_t cnul = 0;
#pragma unroll
    for (int c = 0; c < MAXCOL; ++c) {
      ck[c] = 0;
      if (c < n_col && Q->col_stream[c] == stream) {
        const int a = Q->col_attr[c];
        uint64_t raw = 0;
        if (live) {
          const int wdt = L.b.width[a];
          if (wdt == 8) raw = ((const uint64_t*)L.b.col[a])[e];
          else if (wdt == 4) raw = ((const uint32_t*)L.b.col[a])[e];
          else raw = ((const uint8_t*)L.b.col[a])[e];
          if (L.b.nul[a] && ((const uint8_t*)L.b.nul[a])[e]) cnul |= 1u << c;
        }
        ck[c] = to_key(raw, Q->col_conv[c]);
      }
    }
    auto col_key = [&](int col) {
      int64_t v = ck[0];
#pragma unroll
      for (int c = 1; c < MAXCOL; ++c) v = (col == c) ? ck[c] : v;
      return v;
    };
    // per state: bit k set iff event k passes every atom of the state that reads no capture
    uint64_t smask[S];
    int64_t xcur[S];      // current-event operand of the state's capture-reading atom
    uint32_t xnul = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      bool ok = live && D[s].active;
      xcur[s] = 0;
      if (D[s].active) {
        const int a1 = Q->atom_begin[s + 1] - Q->xa_count[s];
        for (int a = Q->atom_begin[s]; a < a1; ++a) {
          const Atom& A = Q->atoms[a];
          const int64_t l = A.lk == OPK_CUR ? col_key(A.li) : A.lc;
          const int64_t r = A.rk == OPK_CUR ? col_key(A.ri) : A.rc;
          const bool ln = A.lk == OPK_NULL || (A.lk == OPK_CUR && ((cnul >> A.li) & 1u));
          const bool rn = A.rk == OPK_NULL || (A.rk == OPK_CUR && ((cnul >> A.ri) & 1u));
          ok = ok && atom_eval(A, l, ln, r, rn);
        }
        if (D[s].has_x) {
          const int col = Q->xa_col[Q->xa_first[s]];
          if (col >= 0) {
            xcur[s] = col_key(col);
            xnul |= ((cnul >> col) & 1u) << s;
          }
        }
        if constexpr (R) {
          const int rb = Q->rt_b[s], re = Q->rt_e[s];
          if (re > rb) ok = ok && tile_residual(L.rcode, rb, re, col_key, cnul);
        }
      }
      smask[s] = __ballot(ok);
    }
    int64_t capv[MAXCAP];
    uint32_t capn = 0;
#pragma unroll
    for (int c = 0; c < MAXCAP; ++c) {
      capv[c] = 0;
      if (c < n_cap) {
        capv[c] = col_key(Q->cap_col[c]);
        capn |= ((cnul >> Q->cap_col[c]) & 1u) << c;
      }
    }
    // timestamps must be non-decreasing for chunk warm-up to be exact
    int64_t pred = __shfl_up(ets, 1, WAVE);
    if (lane == 0) pred = prev_tile_ts;
    if (live && ets < pred) unordered = true;
    prev_tile_ts = __shfl(ets, WAVE - 1, WAVE);

    const int cnt = (int)((W.c1 - t) < WAVE ? (W.c1 - t) : WAVE);
#pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
      const int64_t j = t + k;
      const bool emit_ok = j >= W.c0;
      const int64_t cts = readlane64(ets, k);
      const int64_t cseq = L.b.seq_base + j;
      const uint32_t capn_k = __builtin_amdgcn_readlane(capn, k);
      const uint32_t xnul_k = __builtin_amdgcn_readlane(xnul, k);
      const uint32_t cnul_k = R ? __builtin_amdgcn_readlane(cnul, k) : 0u;

      // ---- non-start states, last to first (reverse registration order) ----
#pragma unroll
      for (int s = S - 1; s >= 1; --s) {
        const StateDesc& d = D[s];
        if (!d.active) continue;
        const bool last = (s == S - 1);
        const bool cpass = (smask[s] >> k) & 1ull;
        const int64_t cur = readlane64(xcur[s], k);
        const bool curn = (xnul_k >> s) & 1u;
        // the state's test of one partial before its residual: in the state, not expired, the event
        // passes the tile mask, the capture-reading atom holds
        auto atoms_pass = [&](const PSet& Pk, bool& exp) __attribute__((always_inline)) {
          const bool in_s = Pk.st == s;
          exp = in_s && expired(Pk.ts0, cts, within);
          bool pass = in_s && !exp && cpass;
          if (d.has_x) {
            const int64_t lcap = cap_get(Pk, d.lcap), rcap = cap_get(Pk, d.rcap);
            const int64_t l = d.l_cap ? lcap : d.l_cur ? cur : d.lc;
            const int64_t r = d.r_cap ? rcap : d.r_cur ? cur : d.rc;
            const bool ln = d.l_null || (d.l_cur && curn) || (d.l_cap && ((Pk.cn >> d.lcap) & 1u));
            const bool rn = d.r_null || (d.r_cur && curn) || (d.r_cap && ((Pk.cn >> d.rcap) & 1u));
            pass = pass && !ln && !rn && cmp_keys(d.mask, d.f64, l, r);
          }
          return pass;
        };
        // R: the partial residual, once per register set that holds a candidate. The sets are walked by
        // a run-time index over one copy of the interpreter (K inlined copies per state would not fit
        // the registers), the set's captures picked by compares; bit kk of rfail: the lane's partial of
        // set kk fails
        uint32_t rfail = 0;
        if constexpr (R) {
          if (d.rp_e > d.rp_b && cpass) {
            uint32_t cand = 0;
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
              bool exp;
              cand |= (atoms_pass(P[kk], exp) ? 1u : 0u) << kk;
            }
#pragma unroll 1
            for (int k2 = 0; k2 < K; ++k2) {
              if (__ballot((cand >> k2) & 1u) == 0) continue;
              Caps C = caps_of(P[0]);
#pragma unroll
              for (int kk = 1; kk < K; ++kk) {
                const Caps X = caps_of(P[kk]);
                const bool me = k2 == kk;
                C.c0 = me ? X.c0 : C.c0; C.c1 = me ? X.c1 : C.c1; C.c2 = me ? X.c2 : C.c2; C.c3 = me ? X.c3 : C.c3;
                C.cn = me ? X.cn : C.cn;
              }
              if (!partial_residual(L.rcode, d.rp_b, d.rp_e, col_key, cnul_k, k, C)) rfail |= 1u << k2;
            }
          }
        }
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          if (__ballot(P[kk].st == s) == 0) continue;
          bool exp;
          bool pass = atoms_pass(P[kk], exp);
          if constexpr (R) pass = pass && !((rfail >> kk) & 1u);
          if (last) {
            const uint64_t m = __ballot(pass);
            if (m && emit_ok) {
              const int64_t rank = nmatch + wave_mbcnt(m);
              if (nmatch + __popcll(m) > W.seg_cap) {
                seg_over = true;
              } else if (pass) {
                int64_t* r = seg + rank * RW;
                r[0] = qid;
                r[1] = cts;
#pragma unroll
                for (int q2 = 0; q2 < S - 1; ++q2) r[2 + q2] = P[kk].sq[q2];
                r[2 + S - 1] = cseq;
              }
              nmatch += __popcll(m);
            }
            if (pass || exp) P[kk].st = -1;
          } else {
            if (exp) P[kk].st = -1;
            if (pass) {
              P[kk].st = s + 1;
              P[kk].sq[s] = cseq;
#pragma unroll
              for (int c = 0; c < MAXCAP; ++c) {
                const bool take = (d.capmask >> c) & 1u;
                const int64_t v = readlane64(capv[c], k);
                const uint32_t nb = (capn_k >> c) & 1u;
                P[kk].cp[c] = take ? v : P[kk].cp[c];
                P[kk].cn = take ? ((P[kk].cn & ~(1u << c)) | (nb << c)) : P[kk].cn;
              }
            }
          }
        }
      }

      // ---- start state: the seed (every re-arms it, otherwise one match consumes it) ----
      if (seed_alive && ((smask[0] >> k) & 1ull)) {
        if (S == 1) {
          if (emit_ok) {
            if (nmatch + 1 > W.seg_cap) {
              seg_over = true;
            } else if (lane == 0) {
              int64_t* r = seg + nmatch * RW;
              r[0] = qid;
              r[1] = cts;
              r[2] = cseq;
            }
            nmatch += 1;
          }
        } else {
          int slot_set = -1, slot_lane = 0;
#pragma unroll
          for (int kk = 0; kk < K; ++kk) {
            const uint64_t freem = ~__ballot(P[kk].st >= 0);
            if (slot_set < 0 && freem != 0) {
              slot_set = kk;
              slot_lane = __builtin_ctzll(freem);
            }
          }
          if (slot_set < 0) overflow = true;
          const uint32_t cm0 = D[0].capmask;
#pragma unroll
          for (int kk = 0; kk < K; ++kk) {
            if (kk != slot_set) continue;
            const bool mine = lane == slot_lane;
            P[kk].st = mine ? 1 : P[kk].st;
            P[kk].ts0 = mine ? cts : P[kk].ts0;
            P[kk].sq[0] = mine ? cseq : P[kk].sq[0];
            P[kk].cn = mine ? 0u : P[kk].cn;
#pragma unroll
            for (int c = 0; c < MAXCAP; ++c) {
              const bool take = mine && ((cm0 >> c) & 1u);
              const int64_t v = readlane64(capv[c], k);
              P[kk].cp[c] = take ? v : P[kk].cp[c];
              P[kk].cn = take ? (P[kk].cn | (((capn_k >> c) & 1u) << c)) : P[kk].cn;
            }
          }
        }
        if (!every) seed_alive = 0;
      }
    }
  }

  // ---- outputs ----
  const uint64_t any_unordered = __ballot(unordered);
  if (lane == 0) {
    L.seg_count[wid] = nmatch;
    if (overflow) atomicOr(&L.err[0], 1);
    if (any_unordered && W.n_chunks > 1) atomicOr(&L.err[1], 1);
    if (seg_over) atomicOr(&L.err[2], 1);
  }
  if (W.chunk == W.n_chunks - 1) {  // the last chunk owns the instance's final state
    int64_t* pout = L.part[1 - W.inb] + (size_t)W.q * NF * pcap;
    int nlive = 0;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      const int li = kk * WAVE + lane;
      pout[F_STATE * pcap + li] = P[kk].st;
      pout[F_TS0 * pcap + li] = P[kk].ts0;
#pragma unroll
      for (int s = 0; s < MAXS - 1; ++s) pout[(F_SEQ0 + s) * pcap + li] = P[kk].sq[s];
#pragma unroll
      for (int c = 0; c < MAXCAP; ++c) pout[(F_CAP0 + c) * pcap + li] = P[kk].cp[c];
      pout[F_CAPNULL * pcap + li] = P[kk].cn;
      nlive += __popcll(__ballot(P[kk].st >= 0));
    }
    if (lane == 0) {
      InstHeader h;
      h.seed_alive = seed_alive;
      h.n_live = nlive;
      h.overflow = overflow;
      h.unordered = any_unordered != 0;
      L.hdr[1 - W.inb][W.q] = h;
    }
  }
}

// ---- the paged form (header: "Paged form") ----

// page entry li of a field-major table with `cap` lanes per field; the fields the query does not use
// (slots past S - 2, captures past n_cap) are neither read nor written
template <int S>
__device__ __forceinline__ void page_load(const int64_t* tab, int cap, int li, int n_cap, PSet& P) {
  P.ts0 = tab[F_TS0 * cap + li];
#pragma unroll
  for (int s = 0; s < MAXS - 1; ++s) P.sq[s] = s < S - 1 ? tab[(F_SEQ0 + s) * cap + li] : 0;
#pragma unroll
  for (int c = 0; c < MAXCAP; ++c) P.cp[c] = c < n_cap ? tab[(F_CAP0 + c) * cap + li] : 0;
  P.cn = n_cap > 0 ? (uint32_t)tab[F_CAPNULL * cap + li] : 0u;
}

// the page's live lanes, compacted, at entries at .. of the table; entries past `cap` are not stored.
// Returns the live count
template <int S>
__device__ __forceinline__ int page_store(int64_t* tab, int cap, int64_t at, int n_cap, const PSet& P) {
  const bool lv = P.st >= 0;
  const uint64_t m = __ballot(lv);
  const int64_t li = at + wave_mbcnt(m);
  if (lv && li < cap) {
    tab[F_STATE * cap + li] = P.st;
    tab[F_TS0 * cap + li] = P.ts0;
#pragma unroll
    for (int s = 0; s < S - 1; ++s) tab[(F_SEQ0 + s) * cap + li] = P.sq[s];
#pragma unroll
    for (int c = 0; c < MAXCAP; ++c)
      if (c < n_cap) tab[(F_CAP0 + c) * cap + li] = P.cp[c];
    if (n_cap > 0) tab[F_CAPNULL * cap + li] = P.cn;
  }
  return __popcll(m);
}

// MIX (an interleaved push, DESIGN.md §3.2 "Interleaved pushes"): the tile's events come from several
// parts, one stream each. Lane e stages event idx[e] of part order[e]: its columns are loaded from that
// part alone (the lanes of one part in a tile hold consecutive indices, so each part's loads stay
// coalesced), a state is examined at event k iff k's part carries the state's stream, and the seed opens
// at the events of the start state's stream. Which part carries a state's stream is wave-uniform (sp[],
// SGPRs); which events a state sees is one ballot per state and tile (stm[]). One-state queries run here
// too under MIX (every passing event is a match; they hold no partials).
template <int S, bool R, bool MIX>
__global__ __launch_bounds__(256) void nfa_chain_paged_kernel(ChainLaunch L) {
  static_assert(S >= 2 || MIX, "a one-state chain holds no partials");
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int wid = blockIdx.x * 4 + wv;
  if (wid >= L.n_work) return;
  const WorkItem W = L.work[wid];
  const ChainQuery* __restrict__ Q = L.queries + W.q;
  const int stream = L.b.stream;
  const int pcap = L.pcap;
  // ---- wave-uniform program, resolved into SGPRs for the whole chunk (as nfa_chain_kernel) ----
  const int64_t within = Q->within < 0 ? INT64_MAX : Q->within;
  const int every = Q->every, n_cap = Q->n_cap, qid = Q->qid, n_col = Q->n_col;
  StateDesc D[S];
  [[maybe_unused]] const MixLaunch* __restrict__ M = L.mix;
  [[maybe_unused]] int sp[S];  // MIX: the part that carries state s's stream (-1: none of this call)
#pragma unroll
  for (int s = 0; s < S; ++s) {
    StateDesc d{};
    if constexpr (MIX) {
      sp[s] = M->part_of_stream[Q->state_stream[s]];
      d.active = sp[s] >= 0;
    } else {
      d.active = Q->state_stream[s] == stream;
    }
    d.has_x = Q->xa_count[s] > 0;
    if (d.has_x) {
      const Atom& A = Q->atoms[Q->xa_atom[Q->xa_first[s]]];
      d.l_cap = A.lk == OPK_CAP; d.r_cap = A.rk == OPK_CAP;
      d.l_cur = A.lk == OPK_CUR; d.r_cur = A.rk == OPK_CUR;
      d.lcap = d.l_cap ? A.li : 0; d.rcap = d.r_cap ? A.ri : 0;
      d.lc = A.lc; d.rc = A.rc;
      d.l_null = A.lk == OPK_NULL; d.r_null = A.rk == OPK_NULL;
      d.f64 = A.f64; d.mask = A.mask;
    }
    uint32_t cm = 0;
    for (int c = 0; c < n_cap; ++c) cm |= (Q->cap_slot[c] == s ? 1u : 0u) << c;
    d.capmask = cm;
    if constexpr (R) {
      d.rp_b = Q->rp_b[s];
      d.rp_e = Q->rp_e[s];
    }
    D[s] = d;
  }

  bool any_active = false;  // a non-start state reads this launch's stream (MIX: set per tile)
#pragma unroll
  for (int s = 1; s < S; ++s) any_active = any_active || D[s].active;

  int64_t w0 = 0;
  if (W.chunk > 0) w0 = lower_bound_ts(L.b.ts, W.c0, L.b.ts[W.c0 - 1] - within, lane);
  // the working table: the query's next persisted table (last chunk), or the item's scratch one. The
  // first tile of an item continuing the persisted state (w0 == 0) reads part[inb], which may have
  // holes (the register forms leave them); every later tile reads the working table, which has none
  const bool last_chunk = W.chunk == W.n_chunks - 1;
  int64_t* tab = last_chunk ? L.part[1 - W.inb] + (size_t)W.q * NF * pcap : L.scratch + (size_t)W.scr * NF * pcap;
  const int64_t* pin = L.part[W.inb] + (size_t)W.q * NF * pcap;
  int seed_alive = w0 == 0 ? L.hdr[W.inb][W.q].seed_alive : 1;
  int64_t nt = 0;             // entries of the working table
  int64_t lost = 0, need = 0; // partials that found no room; the most entries (stored + lost) at a tile's end

  int64_t nmatch = 0;
  int64_t* seg = L.match + W.seg_off * L.rec_words;
  const int RW = L.rec_words;
  bool unordered = false, seg_over = false;
  int64_t prev_tile_ts = (w0 == 0) ? L.b.prev_ts : L.b.ts[w0 - 1];

  // (an item without events still carries the persisted table over: one pass with an empty tile)
  bool first = true;
  for (int64_t t = w0; first || t < W.c1; t += WAVE) {
    // ---- stage 64 events, one per lane (as nfa_chain_kernel) ----
    const int64_t e = t + lane;
    const bool live = e < W.c1;
    const int64_t ets = live ? L.b.ts[e] : INT64_MAX;
    [[maybe_unused]] int ep = -1;     // MIX: the event's part and its index within it
    [[maybe_unused]] int64_t ei = 0;
    if constexpr (MIX) {
      if (live) {
        ep = M->order[e];
        ei = M->idx[e];
      }
    }
    int64_t ck[MAXCOL];
    uint32_t cnul = 0;
#pragma unroll
    for (int c = 0; c < MAXCOL; ++c) {
      ck[c] = 0;
      if constexpr (MIX) {
        // the column's part is wave-uniform; only that part's events load it (the others: key 0, not null)
        const int pc = c < n_col ? M->part_of_stream[Q->col_stream[c]] : -1;
        if (pc >= 0) {
          const StreamBatch& Bp = M->parts[pc];
          const int a = Q->col_attr[c];
          uint64_t raw = 0;
          if (ep == pc) {
            const int wdt = Bp.width[a];
            if (wdt == 8) raw = ((const uint64_t*)Bp.col[a])[ei];
            else if (wdt == 4) raw = ((const uint32_t*)Bp.col[a])[ei];
            else raw = ((const uint8_t*)Bp.col[a])[ei];
            if (Bp.nul[a] && ((const uint8_t*)Bp.nul[a])[ei]) cnul |= 1u << c;
          }
          ck[c] = to_key(raw, Q->col_conv[c]);
        }
      } else if (c < n_col && Q->col_stream[c] == stream) {
        const int a = Q->col_attr[c];
        uint64_t raw = 0;
        if (live) {
          const int wdt = L.b.width[a];
          if (wdt == 8) raw = ((const uint64_t*)L.b.col[a])[e];
          else if (wdt == 4) raw = ((const uint32_t*)L.b.col[a])[e];
          else raw = ((const uint8_t*)L.b.col[a])[e];
          if (L.b.nul[a] && ((const uint8_t*)L.b.nul[a])[e]) cnul |= 1u << c;
        }
        ck[c] = to_key(raw, Q->col_conv[c]);
      }
    }
    // (the keys captured by value: by reference the compiler keeps ck in scratch memory here)
    auto col_key = [ck](int col) {
      int64_t v = ck[0];
#pragma unroll
      for (int c = 1; c < MAXCOL; ++c) v = (col == c) ? ck[c] : v;
      return v;
    };
    uint64_t smask[S];
    [[maybe_unused]] uint64_t stm[S];  // MIX: the tile's events of state s's stream
    int64_t xcur[S];
    uint32_t xnul = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      bool ok = live && D[s].active;
      if constexpr (MIX) {
        ok = ok && ep == sp[s];
        stm[s] = __ballot(ok);
      }
      xcur[s] = 0;
      if (D[s].active) {
        const int a1 = Q->atom_begin[s + 1] - Q->xa_count[s];
        for (int a = Q->atom_begin[s]; a < a1; ++a) {
          const Atom& A = Q->atoms[a];
          const int64_t l = A.lk == OPK_CUR ? col_key(A.li) : A.lc;
          const int64_t r = A.rk == OPK_CUR ? col_key(A.ri) : A.rc;
          const bool ln = A.lk == OPK_NULL || (A.lk == OPK_CUR && ((cnul >> A.li) & 1u));
          const bool rn = A.rk == OPK_NULL || (A.rk == OPK_CUR && ((cnul >> A.ri) & 1u));
          ok = ok && atom_eval(A, l, ln, r, rn);
        }
        if (D[s].has_x) {
          const int col = Q->xa_col[Q->xa_first[s]];
          if (col >= 0) {
            xcur[s] = col_key(col);
            xnul |= ((cnul >> col) & 1u) << s;
          }
        }
        if constexpr (R) {
          const int rb = Q->rt_b[s], re = Q->rt_e[s];
          if (re > rb) ok = ok && tile_residual(L.rcode, rb, re, col_key, cnul);
        }
      }
      smask[s] = __ballot(ok);
    }
    int64_t capv[MAXCAP];
    uint32_t capn = 0;
#pragma unroll
    for (int c = 0; c < MAXCAP; ++c) {
      capv[c] = 0;
      if (c < n_cap) {
        capv[c] = col_key(Q->cap_col[c]);
        capn |= ((cnul >> Q->cap_col[c]) & 1u) << c;
      }
    }
    if constexpr (MIX) {
      // (one unchunked item: the timestamp-order flag drives the chunk fallback only. A tile with no
      // event of a non-start state's stream walks no page)
      any_active = false;
#pragma unroll
      for (int s = 1; s < S; ++s) any_active = any_active || stm[s] != 0;
    } else {
      int64_t pred = __shfl_up(ets, 1, WAVE);
      if (lane == 0) pred = prev_tile_ts;
      if (live && ets < pred) unordered = true;
      prev_tile_ts = __shfl(ets, WAVE - 1, WAVE);
    }

    const int cnt = W.c1 <= t ? 0 : (int)((W.c1 - t) < WAVE ? (W.c1 - t) : WAVE);

    // the tile's events through one page, in order: the non-start body of nfa_chain_kernel at K = 1.
    // `open` (the fresh page only): lane k's partial exists from the end of event k on
    // (inlined at both calls: a page is registers, never an object in memory)
    auto run_events = [&](PSet& P, const uint64_t open) __attribute__((always_inline)) {
#pragma unroll 1
      for (int k = 0; k < cnt; ++k) {
        if (__ballot(P.st >= 0) == 0 && (open >> k) == 0) break;  // nothing left to examine or open
        const int64_t j = t + k;
        const bool emit_ok = j >= W.c0;
        const int64_t cts = readlane64(ets, k);
        const int64_t cseq = L.b.seq_base + j;
        const uint32_t capn_k = __builtin_amdgcn_readlane(capn, k);
        const uint32_t xnul_k = __builtin_amdgcn_readlane(xnul, k);
        const uint32_t cnul_k = R ? __builtin_amdgcn_readlane(cnul, k) : 0u;
#pragma unroll
        for (int s = S - 1; s >= 1; --s) {
          const StateDesc& d = D[s];
          if (!d.active) continue;
          if constexpr (MIX) {
            if (!((stm[s] >> k) & 1ull)) continue;  // event k is of another stream
          }
          const bool last = (s == S - 1);
          const bool cpass = (smask[s] >> k) & 1ull;
          const int64_t cur = readlane64(xcur[s], k);
          const bool curn = (xnul_k >> s) & 1u;
          const bool in_s = P.st == s;
          if (__ballot(in_s) == 0) continue;
          const bool exp = in_s && expired(P.ts0, cts, within);
          bool pass = in_s && !exp && cpass;
          if (d.has_x) {
            const int64_t lcap = cap_get(P, d.lcap), rcap = cap_get(P, d.rcap);
            const int64_t l = d.l_cap ? lcap : d.l_cur ? cur : d.lc;
            const int64_t r = d.r_cap ? rcap : d.r_cur ? cur : d.rc;
            const bool ln = d.l_null || (d.l_cur && curn) || (d.l_cap && ((P.cn >> d.lcap) & 1u));
            const bool rn = d.r_null || (d.r_cur && curn) || (d.r_cap && ((P.cn >> d.rcap) & 1u));
            pass = pass && !ln && !rn && cmp_keys(d.mask, d.f64, l, r);
          }
          // (a lane of the fresh page that is not open yet is not in_s: it never passes)
          if constexpr (R) {
            // (every lane evaluates: the current event's words are read from lane k, which computes
            // them only while it is active -- `pass && ...` would mask it off with its own partial)
            if (d.rp_e > d.rp_b && __ballot(pass)) {
              const bool rp = partial_residual(L.rcode, d.rp_b, d.rp_e, col_key, cnul_k, k, caps_of(P));
              pass = pass && rp;
            }
          }
          if (last) {
            const uint64_t m = __ballot(pass);
            if (m && emit_ok) {
              const int64_t rank = nmatch + wave_mbcnt(m);
              if (nmatch + __popcll(m) > W.seg_cap) {
                seg_over = true;
              } else if (pass) {
                int64_t* r = seg + rank * RW;
                r[0] = qid;
                r[1] = cts;
#pragma unroll
                for (int q2 = 0; q2 < S - 1; ++q2) r[2 + q2] = P.sq[q2];
                r[2 + S - 1] = cseq;
              }
              nmatch += __popcll(m);
            }
            if (pass || exp) P.st = -1;
          } else {
            if (exp) P.st = -1;
            if (pass) {
              P.st = s + 1;
              P.sq[s] = cseq;
#pragma unroll
              for (int c = 0; c < MAXCAP; ++c) {
                const bool take = (d.capmask >> c) & 1u;
                const int64_t v = readlane64(capv[c], k);
                const uint32_t nb = (capn_k >> c) & 1u;
                P.cp[c] = take ? v : P.cp[c];
                P.cn = take ? ((P.cn & ~(1u << c)) | (nb << c)) : P.cn;
              }
            }
          }
        }
        if (((open >> k) & 1ull) && lane == k) P.st = 1;
      }
    };

    // ---- the live pages: load, run the tile, store back compacted. The write cursor wc never
    //      passes the read cursor p0 (a page stores at most the 64 entries it loaded) ----
    //      A stream that feeds no state but the start state (the A pushes of `A -> B`) examines no
    //      partial: after the first tile has carried the table over, only the fresh pages are added
    if (first || any_active) {
      const int64_t* src = first ? pin : tab;
      const int64_t n_src = first ? (w0 == 0 ? pcap : 0) : nt;
      int64_t wc = 0;
      for (int64_t p0 = 0; p0 < n_src; p0 += WAVE) {
        const int64_t li = p0 + lane;
        PSet P;
        P.st = li < n_src ? (int)src[F_STATE * pcap + li] : -1;
        if (__ballot(P.st >= 0) == 0) continue;
        page_load<S>(src, pcap, (int)(li < n_src ? li : p0), n_cap, P);
        run_events(P, 0);
        wc += page_store<S>(tab, pcap, wc, n_cap, P);
      }
      nt = wc;
    }

    // ---- the fresh page: lane k holds the partial the seed opens at event k ----
    uint64_t open = seed_alive ? smask[0] : 0;
    if (!every && open) {  // without `every` the first match consumes the seed
      open &= 0 - open;
      seed_alive = 0;
    }
    if constexpr (S == 1) {
      // (MIX only) every event the seed passes is a match of its own
      if (open) {
        const bool mine = (open >> lane) & 1ull;
        const int64_t rank = nmatch + wave_mbcnt(open);
        if (nmatch + __popcll(open) > W.seg_cap) {
          seg_over = true;
        } else if (mine) {
          int64_t* r = seg + rank * RW;
          r[0] = qid;
          r[1] = ets;
          r[2] = L.b.seq_base + e;
        }
        nmatch += __popcll(open);
      }
    } else if (open) {
      const uint32_t cm0 = D[0].capmask;
      PSet F;
      F.st = -1;
      F.ts0 = ets;
      F.sq[0] = L.b.seq_base + e;
#pragma unroll
      for (int s = 1; s < MAXS - 1; ++s) F.sq[s] = 0;
#pragma unroll
      for (int c = 0; c < MAXCAP; ++c) F.cp[c] = ((cm0 >> c) & 1u) ? capv[c] : 0;
      F.cn = capn & cm0;
      if (any_active) run_events(F, open);
      else F.st = ((open >> lane) & 1ull) ? 1 : -1;  // (no event of the tile examines them)
      const int fresh = page_store<S>(tab, pcap, nt, n_cap, F);
      const int64_t room = pcap - nt;
      const int64_t kept = fresh < room ? fresh : room;
      lost += fresh - kept;
      nt += kept;
    }
    need = nt + lost > need ? nt + lost : need;
    // the next tile's loads read what other lanes of this wave stored
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    first = false;
  }

  // ---- outputs ----
  const uint64_t any_unordered = __ballot(unordered);
  if (lane == 0) {
    L.seg_count[wid] = nmatch;
    if (lost > 0) {
      atomicOr(&L.err[0], 1);
      atomicMax(&L.err[3], (int)(need < INT32_MAX ? need : INT32_MAX));
    }
    if (any_unordered && W.n_chunks > 1) atomicOr(&L.err[1], 1);
    if (seg_over) atomicOr(&L.err[2], 1);
  }
  if (last_chunk) {  // the working table is the instance's final state: free the lanes past its end
    for (int64_t li = nt + lane; li < pcap; li += WAVE) tab[F_STATE * pcap + li] = -1;
    if (lane == 0) {
      InstHeader h;
      h.seed_alive = seed_alive;
      h.n_live = (int)nt;
      h.overflow = lost > 0;
      h.unordered = any_unordered != 0;
      L.hdr[1 - W.inb][W.q] = h;
    }
  }
}

// table rows re-strided from old_cap to new_cap lanes (new_cap > old_cap): new lanes are free
__global__ void chain_relayout_kernel(const int64_t* src, int64_t* dst, int64_t rows, int old_cap, int new_cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * new_cap) return;
  const int64_t row = i / new_cap;
  const int l = (int)(i - row * new_cap);
  dst[i] = l < old_cap ? src[row * old_cap + l] : (row % NF == F_STATE ? -1 : 0);
}

}  // namespace sdh

template <int S, bool R>
static hipError_t launch_s(int k, const sdh::ChainLaunch* L, int n_blocks, size_t lds, hipStream_t s) {
  switch (k) {
    case 1: hipLaunchKernelGGL((sdh::nfa_chain_kernel<S, 1, R>), dim3(n_blocks), dim3(256), lds, s, *L); break;
    case 2: hipLaunchKernelGGL((sdh::nfa_chain_kernel<S, 2, R>), dim3(n_blocks), dim3(256), lds, s, *L); break;
    case 4: hipLaunchKernelGGL((sdh::nfa_chain_kernel<S, 4, R>), dim3(n_blocks), dim3(256), lds, s, *L); break;
    case 8:
      // (R = true with partials: not built, the engine pages past 256 partials -- chain_reg_limit)
      if constexpr (R && S >= 2) return hipErrorInvalidValue;
      else hipLaunchKernelGGL((sdh::nfa_chain_kernel<S, 8, R>), dim3(n_blocks), dim3(256), lds, s, *L);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <bool R>
static hipError_t launch_r(int n_states, int k, const sdh::ChainLaunch* L, int n_blocks, size_t lds, hipStream_t s) {
  switch (n_states) {
    case 1: return launch_s<1, R>(k, L, n_blocks, lds, s);
    case 2: return launch_s<2, R>(k, L, n_blocks, lds, s);
    case 3: return launch_s<3, R>(k, L, n_blocks, lds, s);
    case 4: return launch_s<4, R>(k, L, n_blocks, lds, s);
    default: return hipErrorInvalidValue;
  }
}

template <bool R, bool MIX>
static hipError_t launch_paged_r(int n_states, const sdh::ChainLaunch* L, int n_blocks, hipStream_t s) {
  switch (n_states) {
    case 1:
      if constexpr (MIX) hipLaunchKernelGGL((sdh::nfa_chain_paged_kernel<1, R, MIX>), dim3(n_blocks), dim3(256), 0, s, *L);
      else return hipErrorInvalidValue;
      break;
    case 2: hipLaunchKernelGGL((sdh::nfa_chain_paged_kernel<2, R, MIX>), dim3(n_blocks), dim3(256), 0, s, *L); break;
    case 3: hipLaunchKernelGGL((sdh::nfa_chain_paged_kernel<3, R, MIX>), dim3(n_blocks), dim3(256), 0, s, *L); break;
    case 4: hipLaunchKernelGGL((sdh::nfa_chain_paged_kernel<4, R, MIX>), dim3(n_blocks), dim3(256), 0, s, *L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// host-side launchers (C linkage inside the library). resid: a K_chain query of the engine has a
// residual program (chain_pred.h), so the launch takes the R = true instantiation; one S, one K and
// one R serve a whole launch, and an R = true kernel runs the atom-only queries beside it unchanged
extern "C" hipError_t sdh_launch_chain(int n_states, int k, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                       size_t lds, hipStream_t s) {
  if (n_blocks <= 0) return hipSuccess;
  return resid ? launch_r<true>(n_states, k, L, n_blocks, lds, s) : launch_r<false>(n_states, k, L, n_blocks, lds, s);
}

// the paged form: chains of two to four states (a one-state chain holds no partials and stays on
// sdh_launch_chain)
extern "C" hipError_t sdh_launch_chain_paged(int n_states, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                             hipStream_t s) {
  if (n_blocks <= 0) return hipSuccess;
  return resid ? launch_paged_r<true, false>(n_states, L, n_blocks, s)
               : launch_paged_r<false, false>(n_states, L, n_blocks, s);
}

// an interleaved push (ChainLaunch::mix): the MIX = true paged kernels, chains of one to four states
extern "C" hipError_t sdh_launch_chain_mixed(int n_states, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                             hipStream_t s) {
  if (n_blocks <= 0) return hipSuccess;
  if (!L->mix) return hipErrorInvalidValue;
  return resid ? launch_paged_r<true, true>(n_states, L, n_blocks, s)
               : launch_paged_r<false, true>(n_states, L, n_blocks, s);
}

// `rows` table rows ([q][field]) of old_cap lanes each -> new_cap lanes each (K_chain table growth)
extern "C" hipError_t sdh_chain_relayout(const int64_t* src, int64_t* dst, int64_t rows, int old_cap, int new_cap,
                                         hipStream_t s) {
  const int64_t n = rows * new_cap;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sdh::chain_relayout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows,
                     old_cap, new_cap);
  return hipGetLastError();
}
