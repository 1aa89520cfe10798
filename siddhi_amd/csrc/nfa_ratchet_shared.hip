// nfa_ratchet_shared.hip -- K_ratchet, shared-pops form: the pops of the threshold-ratchet family
// (nfa_ratchet.hip) computed once per push instead of once per 64-pattern group.
#include <hipcub/hipcub.hpp>

#include "launchers.h"
#include "ratchet_common.h"

#ifndef SDH_RATCHET_NOSTORE
#define SDH_RATCHET_NOSTORE 0
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

// Emission: one wave per item (group x range of e2 events) filters the item's pairs, 64 per tile, and
// writes rec4 blocks as nfa_ratchet_kernel's PM 4 does (same block machinery). The group's carried
// matches, per lane by ascending e2, are merged in by their least pending e2 (wave-uniform). The
// group's last item writes the next deques: the carried survivors are in place, U follows.
__global__ __launch_bounds__(64) void nfa_ratchet_shared_kernel(RatchetLaunch L, SharedLaunch S) {
  const int lane = threadIdx.x;
  const int wid = blockIdx.x;
  if (wid >= L.n_items) return;
  const RatchetItem W = L.items[wid];
  const RatchetGroup* __restrict__ G = L.groups + W.g;
  const bool active = lane < G->n_lanes;
  const int64_t within = G->within[lane];
  const int32_t w32 = !active ? -1 : within >= INT32_MAX ? INT32_MAX : (int32_t)within;
  float flo, fhi;
  sim_bounds(G, lane, active, flo, fhi);
  // the group's widest bounds: a pair outside them is nobody's
  float glo = flo, ghi = fhi;
  int32_t gw = w32;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    glo = fminf(glo, __shfl_xor(glo, d, WAVE));
    ghi = fmaxf(ghi, __shfl_xor(ghi, d, WAVE));
    gw = max(gw, __shfl_xor(gw, d, WAVE));
  }
  const size_t gb = (size_t)W.g * L.rsmax * WAVE;
  const uint32_t sb32 = (uint32_t)L.b.seq_base;
  const uint32_t c0 = (uint32_t)W.c0, c1 = (uint32_t)W.c1;  // (rec4: batches of at most 2^26 events)

  // ---- block state (nfa_ratchet_kernel, PM 4) ----
  constexpr int FULL_FILL = 1 << 30;
  int blk = -1, fill = FULL_FILL, sfill = 0, mover = 0;
  bool new_blk = false;
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
    new_blk = true;
    int nb = 0;
    if (lane == 0) nb = atomicAdd(L.blk_next, 1);
    nb = __builtin_amdgcn_readfirstlane(nb);
    if (nb >= L.n_blocks) {
      mover = 1;
      blk = -1;
      nb = L.n_blocks;  // (the spare block)
    } else {
      if (lane == 0) L.blk_group[nb] = W.g;
      blk = nb;
    }
    fill = 0;
    const uint64_t base = (uint64_t)(reinterpret_cast<char*>(L.match) + (size_t)nb * L.blk_recs * 8);
    const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)base), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    wrs = __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)bhi << 32) | blo), 0,
                                            __builtin_amdgcn_readfirstlane(L.blk_recs * 8), 0x00020000);
  };
  uint32_t cur_j = 0xffffffffu;  // the event of the block's last side entry
  // the lanes of ballot m write `val` as entries of event j
  auto emit = [&](uint32_t j, bool take, uint64_t m, uint32_t val) {
    if (fill > ((L.blk_recs * 8 - 4 * WAVE * 4 - 8 - sfill * 8) >> 2)) roll();
    if (j != cur_j || new_blk) {  // the event's side entry (again at the head of a block it spills into)
      if (lane == 0) {
        const u32x2 se = {(uint32_t)fill, j};
        __builtin_amdgcn_raw_buffer_store_b64(se, wrs, L.blk_recs * 8 - (sfill + 1) * 8, 0, 0);
      }
      ++sfill;
      cur_j = j;
      new_blk = false;
    }
    if (take && !SDH_RATCHET_NOSTORE)
      __builtin_amdgcn_raw_buffer_store_b32(val | ((uint32_t)lane << 26), wrs, (fill + wave_mbcnt(m)) * 4, 0, 0);
    fill += __popcll(m);
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
  const int64_t p0 = lower(c0), p1 = lower(c1);
  for (int64_t t = p0; t < p1; t += WAVE) {
    const bool live = t + lane < p1;
    uint4 pr = make_uint4(0, 0, 0, 0);
    if (live) pr = reinterpret_cast<const uint4*>(S.pairs)[t + lane];
    const float pk = __uint_as_float(pr.z);
    uint64_t cand = wballot(live && pk >= glo && pk <= ghi && (int32_t)pr.w <= gw);
    while (cand) {
      const int k = __builtin_ctzll(cand);
      cand &= cand - 1;
      const uint32_t j = __builtin_amdgcn_readlane(pr.x, k);
      const uint32_t d = __builtin_amdgcn_readlane(pr.y, k);
      const float key = __uint_as_float(__builtin_amdgcn_readlane(pr.z, k));
      const int32_t age = (int32_t)__builtin_amdgcn_readlane(pr.w, k);
      if (cmin <= j) flush_carried(j);
      const bool take = key >= flo && key <= fhi && age <= w32;
      const uint64_t m = wballot(take);
      if (m) emit(j, take, m, d);
    }
  }
  flush_carried(0xfffffffeu);
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
