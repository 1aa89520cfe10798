// nfa_ratchet_shared.hip -- K_ratchet, shared-pops form: the pops of the threshold-ratchet family
// (nfa_ratchet.hip) computed once per push instead of once per 64-pattern group.
#include <hipcub/hipcub.hpp>

#include "launchers.h"
#include "ratchet_common.h"

#ifndef SDH_RATCHET_NOSTORE
#define SDH_RATCHET_NOSTORE 0
#endif
#ifndef SDH_RATCHET_NOSCATTER
#define SDH_RATCHET_NOSCATTER 0  // (timing only: the scatter's LDS writes compiled out, the records are garbage)
#endif
#ifndef SDH_RATCHET_MASK_CXX
#define SDH_RATCHET_MASK_CXX 0
#endif
#ifndef SDH_RATCHET_NT
#define SDH_RATCHET_NT 1  // the flush's 16-B stores carry the non-temporal policy bit (0: the default policy, to measure against)
#endif

namespace sdh {

// ------------------------------------------------------------------------------------------
// Shared-pops form (SIM launches writing rec4 device records). By the deque argument
// in nfa_ratchet.hip's head, partial i of any lane is popped by N(i), the first later event j with `x_j OP x_i`: every
// event between fails the compare against key_i, and at j every newer entry of the lane (keys no
// better than key_i) pops first. N does not depend on the pattern, which decides only whether i opened
// a partial (f0) and whether it was still alive at N(i) (`within`; with ordered timestamps an entry
// expired before N(i) is expired at N(i)). So lane p's matches are {(i, N(i)) : f0_p(i), ts_N(i) -
// ts_i <= within_p}: a pre-pass lists the pairs once per push, sorted by N(i), and each group filters
// them (two float compares and an integer compare per pair) instead of replaying its deques.
// ------------------------------------------------------------------------------------------
template <int XM>
__device__ __forceinline__ bool sh_cmp(float a, float b) {  // `a OP b`; false if either is NaN
  return XM == 0 ? a > b : XM == 1 ? a >= b : XM == 2 ? a < b : a <= b;
}
__device__ __forceinline__ float sh_nan() { return __uint_as_float(0x7fc00000u); }

// best key of each 64 entries of `in` (fmaxf / fminf skip NaN: an all-NaN block gives NaN, which fails
// every compare)
template <int XM>
__global__ __launch_bounds__(256) void ratchet_shared_level(const float* __restrict__ in, int64_t n_in,
                                                            float* __restrict__ out, int64_t n_out) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_out) return;
  const int64_t e = t * 64 + lane;
  float v = e < n_in ? in[e] : sh_nan();
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float o = __shfl_xor(v, d, WAVE);
    v = XM < 2 ? fmaxf(v, o) : fminf(v, o);
  }
  if (lane == 0) out[t] = v;
}

// the first j >= start with `x_j OP key`, or -1: up the tree from start's block until a block's best
// key passes, then down to the event (at most 2 * levels + 1 loads of 64 entries). All arguments are
// wave-uniform.
template <int XM>
__device__ int64_t sh_find_wave(const SharedLaunch& S, int64_t start, float key, int lane) {
  int64_t pos = start;
  int lvl = -1;
  for (;;) {
    const int64_t nl = lvl < 0 ? S.n : pick(S.lvl_n, lvl);
    if (pos >= nl) return -1;
    const float* a = lvl < 0 ? S.x : pick(S.lvl, lvl);
    const int64_t b0 = pos & ~(int64_t)63, p = b0 + lane;
    const float v = (p >= pos && p < nl) ? a[p] : sh_nan();
    const uint64_t m = wballot(sh_cmp<XM>(v, key));
    if (m) {
      pos = b0 + __builtin_ctzll(m);
      break;
    }
    if (lvl == S.n_lvl - 1) return -1;
    pos = (b0 >> 6) + 1;
    ++lvl;
  }
  while (lvl >= 0) {
    const int64_t b0 = pos << 6;
    --lvl;
    const int64_t nl = lvl < 0 ? S.n : pick(S.lvl_n, lvl);
    const float* a = lvl < 0 ? S.x : pick(S.lvl, lvl);
    const int64_t p = b0 + lane;
    const float v = p < nl ? a[p] : sh_nan();
    const uint64_t m = wballot(sh_cmp<XM>(v, key));
    if (!m) return -1;  // (unreachable: the block's best key passed)
    pos = b0 + __builtin_ctzll(m);
  }
  return pos;
}

// the same search by one lane alone (the carried partials: lane = pattern)
template <int XM>
__device__ int64_t sh_find_lane(const SharedLaunch& S, int64_t start, float key) {
  int64_t pos = start;
  int lvl = -1;
  for (;;) {
    const int64_t nl = lvl < 0 ? S.n : pick(S.lvl_n, lvl);
    if (pos >= nl) return -1;
    const float* a = lvl < 0 ? S.x : pick(S.lvl, lvl);
    const int64_t end = (pos | 63) + 1 < nl ? (pos | 63) + 1 : nl;
    bool f = false;
    for (; pos < end; ++pos)
      if (sh_cmp<XM>(a[pos], key)) {
        f = true;
        break;
      }
    if (f) break;
    if (lvl == S.n_lvl - 1) return -1;
    pos = ((end - 1) >> 6) + 1;
    ++lvl;
  }
  while (lvl >= 0) {
    pos <<= 6;
    --lvl;
    const int64_t nl = lvl < 0 ? S.n : pick(S.lvl_n, lvl);
    const float* a = lvl < 0 ? S.x : pick(S.lvl, lvl);
    const int64_t end = pos + 64 < nl ? pos + 64 : nl;
    for (; pos < end; ++pos)
      if (sh_cmp<XM>(a[pos], key)) break;
    if (pos >= end) return -1;  // (unreachable)
  }
  return pos;
}

// N(i) of every batch event (one wave per 64-event tile), the ordered-timestamp check (err[1], with
// prev_ts) and the counts of pairs and of U
template <int XM>
__global__ __launch_bounds__(64) void ratchet_shared_next(SharedLaunch S, const int64_t* __restrict__ ts,
                                                          int64_t prev_ts, int32_t* err) {
  const int lane = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * 64, e = t0 + lane;
  const bool live = e < S.n;
  const float x = live ? S.x[e] : sh_nan();
  const int64_t et = live ? ts[e] : INT64_MAX;
  const int64_t pt = e == 0 ? prev_ts : (live ? ts[e - 1] : INT64_MAX);
  if (wballot(live && et < pt) != 0 && lane == 0) atomicOr(&err[1], 1);
  const bool valid = live && x == x;
  // inside the tile: the first later lane that passes
  int64_t N = -1;
  for (int k = 1; k < WAVE; ++k) {
    const float xk = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), k));
    if (lane < k && N < 0 && sh_cmp<XM>(xk, x)) N = t0 + k;
  }
  // beyond it: the unresolved lanes' keys are no better from older to newer, so from the newest to
  // the oldest their N's do not decrease: each search starts at the previous result, and after a miss
  // every older one misses too
  uint64_t um = wballot(valid && N < 0);
  int64_t from = t0 + WAVE;
  while (um) {
    const int k = 63 - __builtin_clzll(um);
    um &= ~(1ull << k);
    const float xk = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), k));
    const int64_t j = sh_find_wave<XM>(S, from, xk, lane);
    if (j < 0) break;
    if (lane == k) N = j;
    from = j;
  }
  if (live) {
    S.nkey[e] = N >= 0 ? (uint32_t)N : (uint32_t)(valid ? S.n : S.n + 1);
    S.nval[e] = (uint32_t)e;
  }
  const uint64_t pm = wballot(N >= 0), umk = wballot(valid && N < 0);
  if (lane == 0) {
    if (pm) atomicAdd(&S.cnt[0], (uint32_t)__popcll(pm));
    if (umk) atomicAdd(&S.cnt[1], (uint32_t)__popcll(umk));
  }
}

// the sorted (N(i), i) -> 16-B pair records
__global__ __launch_bounds__(256) void ratchet_shared_pairs(SharedLaunch S, const int64_t* __restrict__ ts) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= S.n) return;
  const uint32_t j = S.skey[p];
  if ((int64_t)j >= S.n) return;
  const uint32_t i = S.sval[p];
  SharedPair r;
  r.j = j;
  r.d = j - i;
  r.key = __float_as_uint(S.x[i]);
  const int64_t a = ts[j] - ts[i];
  r.age = a > INT32_MAX ? INT32_MAX : a < 0 ? 0 : (int32_t)a;  // (out of range only in batches that re-run)
  S.pairs[p] = r;
}

// Carried partials: the wave of each group's first item walks every lane's persisted deque from the
// newest entry to the oldest. An entry's match event is the first batch event that passes against its
// key; along a lane these do not decrease towards the older entries, so each search starts at the
// previous result. An entry matches unless expired at that event (64-bit: it may be older than the
// pairs' 32-bit ages); without a match event it survives unless expired at the batch's last event.
template <int XM>
__global__ __launch_bounds__(64) void ratchet_shared_carried(RatchetLaunch L, SharedLaunch S) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= L.n_items) return;
  const RatchetItem W = L.items[blockIdx.x];
  if (W.chunk != 0) return;
  const RatchetGroup* __restrict__ G = L.groups + W.g;
  const int64_t within = G->within[lane];
  const size_t gb = (size_t)W.g * L.rsmax * WAVE;
  const int n_in = lane < G->n_lanes ? pick(L.st, W.inb)[W.g].n[lane] : 0;
  const int64_t* __restrict__ i_ts = pick(L.ent_ts, W.inb);
  const int64_t* __restrict__ i_sq = pick(L.ent_seq, W.inb);
  const int64_t* __restrict__ i_ky = pick(L.ent_key, W.inb);
  const int ob = 1 - W.inb;
  int64_t* __restrict__ o_ts = pick(L.ent_ts, ob);
  int64_t* __restrict__ o_sq = pick(L.ent_seq, ob);
  int64_t* __restrict__ o_ky = pick(L.ent_key, ob);
  {
    // the lane constants the emission kernel reads wave-uniformly (SharedLaunch::bounds)
    const bool active = lane < G->n_lanes;
    const int32_t w32 = !active ? -1 : within >= INT32_MAX ? INT32_MAX : (int32_t)within;
    float flo, fhi;
    sim_bounds(G, lane, active, flo, fhi);
    float glo = flo, ghi = fhi;  // the group's widest bounds: a pair outside them is nobody's
    int32_t gw = w32;
    // the smallest `within` and upper bound of the active lanes: a tile inside both skips the compares
    int32_t wmin = active ? w32 : INT32_MAX;
    float himin = active ? fhi : __int_as_float(0x7f800000);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      glo = fminf(glo, __shfl_xor(glo, d, WAVE));
      ghi = fmaxf(ghi, __shfl_xor(ghi, d, WAVE));
      gw = max(gw, __shfl_xor(gw, d, WAVE));
      wmin = min(wmin, __shfl_xor(wmin, d, WAVE));
      himin = fminf(himin, __shfl_xor(himin, d, WAVE));
    }
    const uint32_t flags = (wballot(active && fhi != __int_as_float(0x7f800000)) ? SHB_HI : 0u) |
                           (wballot(active && w32 != INT32_MAX) ? SHB_AGE : 0u);
    uint32_t* __restrict__ b = S.bounds + (size_t)W.g * SH_BOUNDS;
    b[lane] = __float_as_uint(flo);
    b[WAVE + lane] = __float_as_uint(fhi);
    b[2 * WAVE + lane] = (uint32_t)w32;
    b[3 * WAVE + lane] = lane == SHW_GLO ? __float_as_uint(glo) : lane == SHW_GHI ? __float_as_uint(ghi)
                         : lane == SHW_GW ? (uint32_t)gw : lane == SHW_FLAGS ? flags
                         : lane == SHW_WMIN ? (uint32_t)wmin : lane == SHW_HIMIN ? __float_as_uint(himin) : 0u;
  }
  const int64_t t_last = L.b.ts[S.n - 1];
  int nm = 0, c = n_in - 1, aged = 0, d4 = 0;
  int64_t from = 0;
  for (; c >= 0; --c) {
    const size_t o = gb + (size_t)c * WAVE + lane;
    const int64_t j = sh_find_lane<XM>(S, from, __uint_as_float((uint32_t)i_ky[o]));
    if (j < 0) break;  // (nor do the older entries have one)
    from = j;
    if (!expired(i_ts[o], L.b.ts[j], within)) {
      const uint64_t dist = (uint64_t)(L.b.seq_base + j - i_sq[o]);
      if (dist >= 0x80000000ull) aged = 1;
      if (dist >= (1ull << 26)) d4 = 1;
      S.cm[gb + (size_t)nm * WAVE + lane] = make_uint2((uint32_t)j, (uint32_t)i_sq[o]);
      ++nm;
    }
  }
  int ns = 0;
  for (int i = 0; i <= c; ++i) {
    const size_t o = gb + (size_t)i * WAVE + lane;
    const int64_t t0 = i_ts[o];
    if (expired(t0, t_last, within)) continue;
    const int64_t sq = i_sq[o];
    if ((uint64_t)(L.b.seq_base + S.n - 1 - sq) >= 0x80000000ull) aged = 1;
    const size_t w = gb + (size_t)ns * WAVE + lane;
    o_ts[w] = t0;
    o_ky[w] = i_ky[o];
    o_sq[w] = sq;
    ++ns;
  }
  S.cm_n[W.g * WAVE + lane] = nm;
  S.cs_n[W.g * WAVE + lane] = ns;
  if (wballot(aged != 0) != 0 && lane == 0) atomicOr(&L.err[3], 1);
  if (wballot(d4 != 0) != 0 && lane == 0) atomicOr(&L.err[4], 1);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const int o = __shfl_up(v, d, WAVE);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ uint64_t below64(int k) { return k >= 64 ? ~0ull : (1ull << k) - 1; }  // bits < k

// entries of a wave's LDS staging window (4 B each; a multiple of 4)
#ifndef SDH_RATCHET_WIN
#define SDH_RATCHET_WIN 2048
#endif

// The take masks of two tiles: lane k holds one pair of each tile (key, age), bit p of T says that
// pattern p of the group takes it. The patterns' constants are lane reads of the group's bounds rows
// (vlo, vhi, vw: lane p holds pattern p's), each used for both tiles; walking p downwards,
// `m + m + take` inserts one bit per step.
// HI / AGE: some pattern has a finite upper bound / a `within` (otherwise the compare is dropped).
template <bool HI, bool AGE>
__device__ __forceinline__ void sh_take_masks(uint32_t vlo, uint32_t vhi, uint32_t vw, float k0, int32_t a0, float k1,
                                              int32_t a1, uint64_t& T0, uint64_t& T1) {
  // (written out: left to itself the compiler keeps the 128 compare results in scalar registers,
  // spills them to lanes and materialises each bit with a select and an or. SDH_RATCHET_MASK_CXX=1
  // builds the plain C++ step instead, to measure the two against each other: DESIGN.md §3.1)
  asm volatile("" : "+v"(vlo), "+v"(vhi), "+v"(vw));  // (the lane reads stay inside the caller's loop)
  uint32_t m0[2] = {0, 0}, m1[2] = {0, 0};
  uint64_t tmp;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int p = 31; p >= 0; --p) {
      const int q = h * 32 + p;
      const float lo = __uint_as_float(__builtin_amdgcn_readlane(vlo, q));
      const float hi = HI ? __uint_as_float(__builtin_amdgcn_readlane(vhi, q)) : 0.f;
      const int32_t w = AGE ? (int32_t)__builtin_amdgcn_readlane(vw, q) : 0;
#define SH_STEP(M, K, A)                                                                                       \
  if (HI && AGE)                                                                                               \
    asm("v_cmp_le_f32 vcc, %[lo], %[k]\n\tv_cmp_ge_f32 %[t], %[hi], %[k]\n\ts_and_b64 vcc, vcc, %[t]\n\t"      \
        "v_cmp_ge_i32 %[t], %[w], %[a]\n\ts_and_b64 vcc, vcc, %[t]\n\tv_addc_co_u32 %[m], vcc, %[m], %[m], vcc" \
        : [m] "+v"(M), [t] "=&s"(tmp) : [lo] "s"(lo), [hi] "s"(hi), [w] "s"(w), [k] "v"(K), [a] "v"(A) : "vcc"); \
  else if (HI)                                                                                                 \
    asm("v_cmp_le_f32 vcc, %[lo], %[k]\n\tv_cmp_ge_f32 %[t], %[hi], %[k]\n\ts_and_b64 vcc, vcc, %[t]\n\t"      \
        "v_addc_co_u32 %[m], vcc, %[m], %[m], vcc"                                                             \
        : [m] "+v"(M), [t] "=&s"(tmp) : [lo] "s"(lo), [hi] "s"(hi), [k] "v"(K) : "vcc");                        \
  else if (AGE)                                                                                                \
    asm("v_cmp_le_f32 vcc, %[lo], %[k]\n\tv_cmp_ge_i32 %[t], %[w], %[a]\n\ts_and_b64 vcc, vcc, %[t]\n\t"       \
        "v_addc_co_u32 %[m], vcc, %[m], %[m], vcc"                                                             \
        : [m] "+v"(M), [t] "=&s"(tmp) : [lo] "s"(lo), [w] "s"(w), [k] "v"(K), [a] "v"(A) : "vcc");              \
  else                                                                                                         \
    asm("v_cmp_le_f32 vcc, %[lo], %[k]\n\tv_addc_co_u32 %[m], vcc, %[m], %[m], vcc"                            \
        : [m] "+v"(M) : [lo] "s"(lo), [k] "v"(K) : "vcc")
#if SDH_RATCHET_MASK_CXX
      m0[h] = m0[h] + m0[h] + ((k0 >= lo && (!HI || k0 <= hi) && (!AGE || a0 <= w)) ? 1u : 0u);
      m1[h] = m1[h] + m1[h] + ((k1 >= lo && (!HI || k1 <= hi) && (!AGE || a1 <= w)) ? 1u : 0u);
#else
      SH_STEP(m0[h], k0, a0);
      SH_STEP(m1[h], k1, a1);
#endif
#undef SH_STEP
    }
  }
  (void)tmp;
  T0 = ((uint64_t)m0[1] << 32) | m0[0];
  T1 = ((uint64_t)m1[1] << 32) | m1[0];
}

// Emission: one wave per item (group x range of e2 events) writes rec4 blocks (the block machinery of
// nfa_ratchet_kernel's PM 4). First the group's carried matches at the item's events, lane = pattern,
// by ascending e2. Then the item's pairs, 64 per tile with lane = pair: the take mask of each pair
// over the group's patterns (sh_take_masks), the pairs' entry counts scanned into offsets, one side
// entry per event and block from two ballots, the entries scattered through an LDS window (one
// wave-wide write per pair where the pairs are dense, one walk of its mask per lane where they are
// sparse) and copied to the block in whole-wave contiguous stores. A tile that does not fit the block
// is cut at the last pair that does. The group's last item writes the next deques: the carried
// survivors are in place, U follows.
__global__ __launch_bounds__(64) void nfa_ratchet_shared_kernel(RatchetLaunch L, SharedLaunch S) {
  __shared__ __attribute__((aligned(16))) uint32_t win[SDH_RATCHET_WIN];
  constexpr int SH_PASS = SDH_RATCHET_WIN - 4;  // entries per pass through the window (4 slots of alignment slack)
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;
  if (wid >= L.n_items) return;
  const RatchetItem W = L.items[wid];
  const RatchetGroup* __restrict__ G = L.groups + W.g;
  const uint32_t* __restrict__ bt = S.bounds + (size_t)W.g * SH_BOUNDS;  // (written by ratchet_shared_carried)
  const int64_t within = G->within[lane];
  const uint32_t vlo = bt[lane], vhi = bt[WAVE + lane], vw = bt[2 * WAVE + lane];
  const float flo = __uint_as_float(vlo), fhi = __uint_as_float(vhi);
  const float glo = __uint_as_float(bt[3 * WAVE + SHW_GLO]), ghi = __uint_as_float(bt[3 * WAVE + SHW_GHI]);
  const int32_t gw = (int32_t)bt[3 * WAVE + SHW_GW];
  const uint32_t gflags = bt[3 * WAVE + SHW_FLAGS];
  const int32_t gwmin = (int32_t)bt[3 * WAVE + SHW_WMIN];
  const float ghimin = __uint_as_float(bt[3 * WAVE + SHW_HIMIN]);
  const uint64_t lanes_m = below64(G->n_lanes);  // (idle patterns take nothing)
  // the pair form's lane constants: the pattern's bits of an entry, its mask bit, and the byte offset
  // of its slot in a pair every active pattern takes (idle lanes: beyond any pass)
  const uint32_t lp = (uint32_t)lane << 26;
  const uint64_t lbit = 1ull << lane;
  const uint32_t fslot4 = lane < G->n_lanes ? (uint32_t)lane * 4u : 0x40000000u;
  const size_t gb = (size_t)W.g * L.rsmax * WAVE;
  const uint32_t sb32 = (uint32_t)L.b.seq_base;
  const uint32_t c0 = (uint32_t)W.c0, c1 = (uint32_t)W.c1;  // (rec4: batches of at most 2^26 events)

  // ---- block state (nfa_ratchet_kernel, PM 4) ----
  // (cap: the bytes of the open block, 0 before the first one; cur_j: the event of the block's last
  // side entry)
  constexpr uint32_t NO_J = 0xffffffffu;
  int blk = -1, fill = 0, sfill = 0, cap = 0, mover = 0;
  uint32_t cur_j = NO_J;
  unsigned long long n_emit = 0, n_bytes = 0;
  __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(L.match, 0, 0, 0x00020000);
  auto close_blk = [&]() {
    if (blk >= 0 && lane == 0) {
      L.blk_count[blk] = fill;
      L.blk_side[blk] = sfill;
    }
    if (blk >= 0) {
      n_emit += (unsigned long long)fill;
      n_bytes += (unsigned long long)fill * 4 + (unsigned long long)sfill * 8;
    }
  };
  auto roll = [&]() {
    close_blk();
    sfill = 0;
    cur_j = NO_J;
    cap = L.blk_recs * 8;
    int nb = 0;
    if (lane == 0) nb = atomicAdd(L.blk_next, 1);
    nb = __builtin_amdgcn_readfirstlane(nb);
    const bool over = nb >= L.n_blocks;
    mover |= over ? 1 : 0;
    blk = over ? -1 : nb;
    nb = over ? L.n_blocks : nb;  // (the spare block)
    if (!over && lane == 0) L.blk_group[nb] = W.g;
    fill = 0;
    const uint64_t base = (uint64_t)(reinterpret_cast<char*>(L.match) + (size_t)nb * L.blk_recs * 8);
    const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)base), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    wrs = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)bhi << 32) | blo), 0,
                                            __builtin_amdgcn_readfirstlane(L.blk_recs * 8), 0x00020000);
  };
  // the carried phase (lane = pattern): the lanes of ballot m write `val` as entries of event j. A
  // block is left when less than a pair's worth (64 entries and a side entry) is free
  auto emit = [&](uint32_t j, bool take, uint64_t m, uint32_t val) {
    // (counted here, through a convergent read: the compiler otherwise sinks the popcount into both
    // arms of the lane-variant `take` branch, and the value merged behind that branch, and with it
    // fill, the room test and the block's descriptor, counts as lane-variant: every store then sits
    // in a loop over its descriptor)
    const int n_m = __builtin_amdgcn_readfirstlane(__popcll(m));
    if (4 * (fill + WAVE) + 8 * (sfill + 1) > cap) roll();
    if (j != cur_j) {  // the event's side entry (again at the head of a block it spills into)
      if (lane == 0) {
        const u32x2 se = {(uint32_t)fill, j};
        __builtin_amdgcn_raw_buffer_store_b64(se, wrs, cap - (sfill + 1) * 8, 0, 0);
      }
      ++sfill;
      cur_j = j;
    }
    if (take && !SDH_RATCHET_NOSTORE)
      __builtin_amdgcn_raw_buffer_store_b32(val | ((uint32_t)lane << 26), wrs, (fill + wave_mbcnt(m)) * 4, 0, 0);
    fill += n_m;
  };

  // ---- the lane's carried matches from c0 on ----
  const int ncm = S.cm_n[W.g * WAVE + lane];
  int ci = 0;
  uint32_t cj = 0xffffffffu, cq = 0;
  auto cm_load = [&]() {
    cj = 0xffffffffu;
    if (ci < ncm) {
      const uint2 v = S.cm[gb + (size_t)ci * WAVE + lane];
      if (v.x < c1) {
        cj = v.x;
        cq = v.y;
      }
    }
  };
  cm_load();
  while (cj < c0) {
    ++ci;
    cm_load();
  }
  uint32_t cmin = wave_min_u32(cj);
  auto flush_carried = [&](uint32_t upto) {  // every carried match at an event <= upto
    while (cmin <= upto) {
      const uint32_t j = cmin;
      const bool t = cj == j;
      emit(j, t, wballot(t), ((sb32 + j) - cq) & 0x03ffffffu);
      if (t) {
        ++ci;
        cm_load();
      }
      cmin = wave_min_u32(cj);
    }
  };

  // ---- the item's pairs: j in [c0, c1) ----
  const int64_t P = S.cnt[0];
  auto lower = [&](uint32_t j) {
    int64_t lo = 0, hi = P;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (S.pairs[mid].j < j) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const int64_t p0 = rfl64(lower(c0)), p1 = rfl64(lower(c1));  // (wave-uniform, and known to be)
  flush_carried(0xfffffffeu);  // (a phase of their own: an event may own a side entry of each phase)

  // one tile: lane k holds pair k = entries {d | p << 26} of event j for the set bits p of T,
  // ascending. Pairs are sorted by j, so an event's pairs are a run of lanes
  const uint64_t below_k = (1ull << lane) - 1, le_k = below_k | (1ull << lane);
  auto tile = [&](uint32_t j, uint32_t d, uint64_t T) {
    const int c = __popcll(T);
    const uint64_t has = wballot(c > 0);
    if (!has) return;  // (candidates of the widest bounds, no taker: nothing is written)
    const uint64_t fullm = wballot(T == lanes_m);  // pairs every active pattern takes
    const int incl = wave_incl_scan(c, lane), off = incl - c;
    const uint32_t jp = (uint32_t)__shfl_up((int)j, 1, WAVE);
    const uint64_t jdiff = wballot(lane == 0 || j != jp);  // the runs' first lanes
    for (int a = 0;;) {  // the lanes from a on, as far as the block has room
      const uint64_t am = ~below64(a), hm = has & am;
      if (!hm) break;
      const int off_a = __builtin_amdgcn_readlane(off, a);
      // a pair opens a side entry if it has entries and no earlier pair of its run from lane a on
      // has; the first one continues the block's last side entry if that is its event's
      const uint64_t st = (jdiff | (1ull << a)) & le_k & am;
      const int s = 63 - __clzll(st | 1);  // the run's first lane, a at least (lanes below a open nothing)
      bool opens = lane >= a && c > 0 && (has & below_k & ~((1ull << s) - 1)) == 0;
      if (lane == __builtin_ctzll(hm) && j == cur_j) opens = false;
      const uint64_t om = wballot(opens);
      const int rank = wave_mbcnt(om);
      // the longest prefix [a, b) whose entries and side entries fit (the need grows with the lane)
      const int need = 4 * (fill + incl - off_a) + 8 * (sfill + rank + (opens ? 1 : 0));
      const uint64_t nf = wballot(need > cap) & am;
      const int b = nf ? __builtin_ctzll(nf) : 64;
      if (b == a) {  // (not even pair a: a fresh block holds it, launch_ratchet checks the block size)
        roll();
        continue;
      }
      const uint64_t chunk = below64(b) & am, omc = om & chunk;
      const bool mine = (chunk >> lane) & 1;
      const int E = (b == 64 ? __builtin_amdgcn_readlane(incl, 63) : __builtin_amdgcn_readlane(off, b)) - off_a;
      if (opens && mine) {
        const u32x2 se = {(uint32_t)(fill + off - off_a), j};
        __builtin_amdgcn_raw_buffer_store_b64(se, wrs, cap - (sfill + rank + 1) * 8, 0, 0);
      }
      // the entries through the window, a pass at a time: the scatter writes them, then the wave copies
      // the pass out. Entry 0 of the pass sits at slot fill & 3 of the window, so a 16-B-aligned quad of
      // the window is one of the block: the middle goes out as 16-B stores (1 KiB per wave instruction),
      // up to three entries at either end as 4-B stores.
      // Two forms of the scatter, chosen per block part. Pair form (lane = pattern): a scalar loop over
      // the pairs whose entries meet the pass, one wave-wide write at consecutive slots per pair; a pair
      // every active pattern takes needs no rank. Lane form (lane = pair): each lane writes its next
      // entries while they lie inside the pass, low half of T first. The lane form's trips are the
      // largest count, the pair form's the pairs with entries (nz): with nz * nz <= E the mean count
      // E / nz is at least nz, and the pair form never takes more trips
      const int nz = __popcll(has & chunk);
      const bool pairform = S.scatter == SH_SCATTER_PAIR || (S.scatter == SH_SCATTER_RULE && nz * nz <= E);
      uint32_t rlo = mine ? (uint32_t)T : 0u, rhi = mine ? (uint32_t)(T >> 32) : 0u;
      const int rel = off - off_a;
      uint32_t pos = (uint32_t)rel;
      const int sh = fill & 3;
      for (int w0 = 0; w0 < E; w0 += SH_PASS) {
        if (SDH_RATCHET_NOSCATTER) {
        } else if (pairform) {
          // (a pair that straddles a pass boundary is visited in both passes)
          const uint64_t pm = wballot(mine && c > 0 && rel + c > w0 && rel < w0 + SH_PASS);
          // (a full pair's write is not predicated: a slot outside the pass lands, clamped, on window
          // words the flush never reads -- below slot sh, or from sh + SH_PASS to the last word)
          const int wb4 = (sh - w0) * 4;
          for (uint64_t fm = pm & fullm; fm;) {
            const int k = __builtin_ctzll(fm);
            fm &= ~(1ull << k);
            const uint32_t x = (uint32_t)(__builtin_amdgcn_readlane(rel, k) * 4 + wb4) + fslot4;
            const uint32_t dk = __builtin_amdgcn_readlane(d, k);
            *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(win) + min(x, (uint32_t)(SDH_RATCHET_WIN - 1) * 4u)) = dk | lp;
          }
          for (uint64_t qm = pm & ~fullm; qm; qm &= qm - 1) {
            const int k = __builtin_ctzll(qm);
            const uint64_t Tk = (uint64_t)readlane64((int64_t)T, k);
            const uint32_t slot = (uint32_t)(__builtin_amdgcn_readlane(rel, k) - w0) + (uint32_t)wave_mbcnt(Tk);
            const uint32_t dk = __builtin_amdgcn_readlane(d, k);
            if ((Tk & lbit) != 0 && slot < (uint32_t)SH_PASS) win[sh + slot] = dk | lp;
          }
        } else {
          uint32_t idx = pos - (uint32_t)w0;  // (beyond the pass for a lane whose entries start later)
          while (rlo != 0 && idx < (uint32_t)SH_PASS) {
            win[sh + idx] = d | ((uint32_t)__builtin_ctz(rlo) << 26);
            rlo &= rlo - 1;
            ++idx;
          }
          while (rlo == 0 && rhi != 0 && idx < (uint32_t)SH_PASS) {
            win[sh + idx] = d | ((32u + (uint32_t)__builtin_ctz(rhi)) << 26);
            rhi &= rhi - 1;
            ++idx;
          }
          pos = (uint32_t)w0 + idx;
        }
        __syncthreads();
        const int n = min(SH_PASS, E - w0), g0 = fill + w0;  // (g0 - sh is a multiple of 4)
        const int nh = min(n, (4 - sh) & 3), nq = (n - nh) >> 2, nt = n - nh - 4 * nq;
        if (lane < nh + nt) {
          const int e = lane < nh ? lane : 4 * nq + lane;
          const uint32_t v = win[sh + e];
          if (!SDH_RATCHET_NOSTORE) __builtin_amdgcn_raw_buffer_store_b32(v, wrs, (g0 + e) * 4, 0, 0);
        }
        for (int q0 = 0; q0 < nq; q0 += WAVE) {
          const int q = q0 + lane;
          if (q < nq) {
            const u32x4 v = reinterpret_cast<const u32x4*>(win)[((sh + nh) >> 2) + q];  // (sh + nh is 0 or 4)
            if (!SDH_RATCHET_NOSTORE) __builtin_amdgcn_raw_buffer_store_b128(v, wrs, (g0 + nh + 4 * q) * 4, 0, SDH_RATCHET_NT ? 2 : 0);
          }
        }
        __syncthreads();
      }
      fill += E;
      sfill += __builtin_amdgcn_readfirstlane(__popcll(omc));
      if (omc) cur_j = __builtin_amdgcn_readlane(j, 63 - __clzll(omc));
      if (b == 64) break;
      roll();
      a = b;
    }
  };

  // ---- the item's pairs, two tiles per read of the group's constants ----
  for (int64_t t = p0; t < p1; t += 2 * WAVE) {
    const bool live0 = t + lane < p1, live1 = t + WAVE + lane < p1;
    uint4 pr0 = make_uint4(0, 0, 0, 0), pr1 = pr0;
    if (live0) pr0 = reinterpret_cast<const uint4*>(S.pairs)[t + lane];
    if (live1) pr1 = reinterpret_cast<const uint4*>(S.pairs)[t + WAVE + lane];
    const float k0 = __uint_as_float(pr0.z), k1 = __uint_as_float(pr1.z);
    const int32_t a0 = (int32_t)pr0.w, a1 = (int32_t)pr1.w;
    const bool cand0 = live0 && k0 >= glo && k0 <= ghi && a0 <= gw, cand1 = live1 && k1 >= glo && k1 <= ghi && a1 <= gw;
    if (wballot(cand0 || cand1) == 0) continue;  // outside the group's widest bounds: nobody's
    uint64_t T0, T1;
    // a compare every active pattern passes for every candidate of both tiles is dropped: with
    // age <= min w32 (key <= min fhi) `a <= w` (`k <= hi`) holds for each of them, equality included;
    // the other pairs' masks are zeroed below
    uint32_t fl = gflags;
    if ((fl & SHB_AGE) && wballot((cand0 && a0 > gwmin) || (cand1 && a1 > gwmin)) == 0) fl &= ~SHB_AGE;
    if ((fl & SHB_HI) && wballot((cand0 && !(k0 <= ghimin)) || (cand1 && !(k1 <= ghimin))) == 0) fl &= ~SHB_HI;
    if (fl == 0) sh_take_masks<false, false>(vlo, vhi, vw, k0, a0, k1, a1, T0, T1);
    else if (fl == SHB_AGE) sh_take_masks<false, true>(vlo, vhi, vw, k0, a0, k1, a1, T0, T1);
    else if (fl == SHB_HI) sh_take_masks<true, false>(vlo, vhi, vw, k0, a0, k1, a1, T0, T1);
    else sh_take_masks<true, true>(vlo, vhi, vw, k0, a0, k1, a1, T0, T1);
    T0 = cand0 ? T0 & lanes_m : 0;
    T1 = cand1 ? T1 & lanes_m : 0;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) tile(h ? pr1.x : pr0.x, h ? pr1.y : pr0.y, h ? T1 : T0);
  }
  close_blk();

  int overflow = 0;
  if (W.chunk == W.n_chunks - 1) {
    // ---- the next deques: the carried survivors (ratchet_shared_carried), then U filtered by the
    // lane's f0 and `within` at the batch's last event, oldest first ----
    const int ob = 1 - W.inb;
    int64_t* __restrict__ o_ts = pick(L.ent_ts, ob);
    int64_t* __restrict__ o_sq = pick(L.ent_seq, ob);
    int64_t* __restrict__ o_ky = pick(L.ent_key, ob);
    int cnt = S.cs_n[W.g * WAVE + lane];
    const int64_t nU = S.cnt[1];
    const int64_t t_last = L.b.ts[S.n - 1];
    for (int64_t u0 = 0; u0 < nU; u0 += WAVE) {
      const bool live = u0 + lane < nU;
      const uint32_t idx = live ? S.sval[P + u0 + lane] : 0u;
      const float uk = live ? S.x[idx] : sh_nan();
      const int64_t ut = live ? L.b.ts[idx] : 0;
      uint64_t cand = wballot(live && uk >= glo && uk <= ghi && (gw == INT32_MAX || !expired(ut, t_last, (int64_t)gw)));
      while (cand) {
        const int k = __builtin_ctzll(cand);
        cand &= cand - 1;
        const float key = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(uk), k));
        const int64_t tk = readlane64(ut, k);
        const uint32_t ik = __builtin_amdgcn_readlane(idx, k);
        if (key >= flo && key <= fhi && !expired(tk, t_last, within)) {
          if (cnt < L.rsmax) {
            const size_t o = gb + (size_t)cnt * WAVE + lane;
            o_ts[o] = tk;
            o_ky[o] = (int64_t)(uint64_t)__float_as_uint(key);
            o_sq[o] = L.b.seq_base + (int64_t)ik;
            ++cnt;
          } else {
            overflow = 1;
          }
        }
      }
    }
    pick(L.st, ob)[W.g].n[lane] = cnt;
  }
  const uint64_t any_over = wballot(overflow != 0);
  if (lane == 0) {
    if (n_emit) atomicAdd(L.rec_total, n_emit);
    if (n_bytes) atomicAdd(L.rec_total + 2, n_bytes);
    if (any_over) atomicOr(&L.err[0], 1);
    if (mover) atomicOr(&L.err[2], 1);
  }
}

}  // namespace sdh

// ---- shared-pops form: host entry points ----
extern "C" size_t sdh_ratchet_shared_temp(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs((void*)nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)n, 0, 32);
  return b;
}

extern "C" int sdh_ratchet_shared_occupancy() {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sdh::nfa_ratchet_shared_kernel, 64, 0) != hipSuccess) return 0;
  return nb;
}

template <int XM>
static hipError_t shared_pre(const sdh::SharedLaunch& S, const sdh::StreamBatch* B, int32_t* err, void* temp,
                             size_t temp_bytes, hipStream_t s) {
  const float* in = S.x;
  int64_t n_in = S.n;
  for (int k = 0; k < S.n_lvl; ++k) {
    hipLaunchKernelGGL(sdh::ratchet_shared_level<XM>, dim3((unsigned)((S.lvl_n[k] + 3) / 4)), dim3(256), 0, s, in, n_in,
                       S.lvl[k], S.lvl_n[k]);
    in = S.lvl[k];
    n_in = S.lvl_n[k];
  }
  hipLaunchKernelGGL(sdh::ratchet_shared_next<XM>, dim3((unsigned)((S.n + 63) / 64)), dim3(64), 0, s, S, B->ts, B->prev_ts, err);
  int bits = 1;
  while (((int64_t)1 << bits) <= S.n + 1) ++bits;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, S.nkey, S.skey, S.nval, S.sval, (int)S.n, 0, bits, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sdh::ratchet_shared_pairs, dim3((unsigned)((S.n + 255) / 256)), dim3(256), 0, s, S, B->ts);
  return hipGetLastError();
}

// the pre-pass of one (stream, key column, OP) of a push: tree, N(i), sorted pairs, counts (S.cnt zeroed
// by the caller)
extern "C" hipError_t sdh_launch_ratchet_shared_pre(const sdh::SharedLaunch* S, const sdh::StreamBatch* B, int32_t* err,
                                                    void* temp, size_t temp_bytes, hipStream_t s) {
  if (S->n <= 0) return hipSuccess;
  switch (S->xm) {
    case 0: return shared_pre<0>(*S, B, err, temp, temp_bytes, s);
    case 1: return shared_pre<1>(*S, B, err, temp, temp_bytes, s);
    case 2: return shared_pre<2>(*S, B, err, temp, temp_bytes, s);
    default: return shared_pre<3>(*S, B, err, temp, temp_bytes, s);
  }
}

// the groups of one launch: carried partials, then the emission items
extern "C" hipError_t sdh_launch_ratchet_shared(const sdh::RatchetLaunch* L, const sdh::SharedLaunch* S, hipStream_t s) {
  if (L->n_items <= 0) return hipSuccess;
  const dim3 grid(L->n_items), block(64);
  switch (S->xm) {
    case 0: hipLaunchKernelGGL(sdh::ratchet_shared_carried<0>, grid, block, 0, s, *L, *S); break;
    case 1: hipLaunchKernelGGL(sdh::ratchet_shared_carried<1>, grid, block, 0, s, *L, *S); break;
    case 2: hipLaunchKernelGGL(sdh::ratchet_shared_carried<2>, grid, block, 0, s, *L, *S); break;
    default: hipLaunchKernelGGL(sdh::ratchet_shared_carried<3>, grid, block, 0, s, *L, *S); break;
  }
  hipLaunchKernelGGL(sdh::nfa_ratchet_shared_kernel, grid, block, 0, s, *L, *S);
  return hipGetLastError();
}
