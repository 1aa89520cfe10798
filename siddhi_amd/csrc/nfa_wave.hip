// nfa_wave.hip -- K_wave: the unpartitioned count pattern
//   every e1=S[f1] -> e2=S[f2] <min:max> -> e3=S[f3(e1, e2[0], e2[last], cur)] [within T]
// one wave per query, one lane per partial, the partial table in HBM in pages of 64 entries
// (wave_lower.h decides the shape; wave_step.h is the per-partial step and names the exactness
// argument, which is part_body.h's for the count chain).
//
// Mapping to CDNA4. The work item is a query and the workgroup one 64-lane wave (the choice among
// groupings is argued in DESIGN.md §3.13 from the kernel's register and LDS figures). Per tile of 64
// events:
//   * the tile is staged once, coalesced, in LDS: ts, seq, the query's captured attribute words, null
//     bits (as K_part and K_chain do);
//   * f1 and f2 read the event only, so they are evaluated once per tile with lane = event: m1 and m2
//     are two wave-uniform 64-bit ballots (K_part evaluates them per lane's query, 64 events each);
//   * every live page is walked: loaded field-major (one coalesced 512-B load per word) into an LDS
//     page whose column `lane` is that lane's entry, each lane steps its partial through the tile's
//     events in order (wave_step, f3 at lane = partial, the event's words read by broadcast), and the
//     survivors are stored compacted -- ballot + mbcnt, creation order -- at the write cursor, which
//     never passes the read cursor: a page's survivors land below the page's own end, and only the
//     next tile (after a workgroup barrier) reads what this one wrote;
//   * an event at which no lane of the page is in e3's list and whose m2 bit is clear cannot change
//     the page (no expiry, no f3, no append): it is skipped with a scalar test;
//   * the partials the tile's events open form a fresh page, lane = opening event: lane k joins after
//     event k's own sweep (the reference's two-phase add: a partial is in the count state's list from
//     the next event on), and a partial opened by the tile's last event is stored unstepped. The
//     survivors are appended at the tail, so a table stays in creation order.
// All lanes interpret the same query's bytecode (kgen.h eval_code), so instruction fetch and the
// bytecode loads are wave-uniform.
//
// Order. Neither the order records leave the kernel nor the lane a partial sits in is observable.
// The reference delivers one event's matches of a query in e3's pending-list order, which is the
// partials' creation order, i.e. ascending e1 seq (part_body.h). Every record carries e1's seq as its
// emission index (the narrow record as the distance back from the trigger), the device match table
// stores it as the row's first tiebreak, and a poll sorts by (trigger seq, receiver rank, tiebreak):
// the engine asks for that tiebreak pass whenever it holds K_wave queries (engine.hip append_gen).
// Two matches of one (query, event) never share an e1, so the key is total and the delivered order is
// the reference's whatever page, lane or flush a record came from. Compaction keeps creation order
// only so that the table is a deterministic function of the events (snapshots compare equal).
//
// Overflow is loud and exact: survivors past the table's capacity are not stored, err[0] is set, and
// the walk goes on counting: the entries that did not fit are carried in `lost` as if every one of
// them survived the rest of the push, so err[3] ends as an upper bound of the entries a table needed
// (a capacity at which the re-run cannot overflow again, reached in one growth). The
// output table is the other one of the query's two, so the persisted table is untouched until the
// host accepts the pass; it re-runs the push at a capacity that fits.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "launchers.h"
#include "wave_step.h"

namespace sdh {

namespace {

// the current event: captured words and null bits from the LDS staging tile (word j at w[j * 64])
struct WaveEv {
  const int64_t* w;
  uint32_t nul;
  __device__ int64_t word(int j) const { return w[j * 64]; }
  __device__ bool null(int j) const { return (nul >> j) & 1u; }
};

// a lane's entry in the LDS page: word w at p[w * 64] (the lanes' columns are bank-conflict free)
struct PageRef {
  int64_t* p;
  __device__ int64_t get(int w) const { return p[w * 64]; }
  __device__ void set(int w, int64_t v) const { p[w * 64] = v; }
};

using WaveOutW = dev::WaveOutT<512, true>;

}  // namespace

__global__ __launch_bounds__(64) void nfa_wave_kernel(WaveLaunch L) {
  extern __shared__ int64_t pg[];  // [ew][64] the page being stepped
  __shared__ int64_t t_ts[64], t_seq[64], t_w[kg::GMAXNA][64];
  __shared__ uint32_t t_nul[64];
  __shared__ typename WaveOutW::Shared out_sh;
  const int lane = threadIdx.x;
  const int item = (int)dev::grid_item(L.xcd);
  if (item >= L.n_items) return;
  const kg::GQuery* __restrict__ q = L.tab.queries + L.qlist[item];
  const int stream = L.b.stream;
  const int ncap = q->n_cap[stream];
  const int cmin = q->st[1].min, cmax = q->st[1].max;
  const int64_t within = q->within, qid = q->qid;
  const PartOffs of{L.cmax, L.n_e1, L.n_first, L.n_last};
  const int ew = L.ew, cap = L.cap;
  const int64_t stride = WV_HDR + (int64_t)cap * ew;
  const int64_t* __restrict__ in = L.in + (int64_t)item * stride;
  int64_t* out = L.out + (int64_t)item * stride;  // (later tiles read it too: no restrict)
  const unsigned long long below = (1ull << lane) - 1ull;
  WaveOutW o;
  o.g = dev::lane_out(L.sink);
  o.sh = &out_sh;
  o.init();
  const PageRef e{pg + lane};
  const bool nb_ok = L.b.n < (int64_t)INT32_MAX;  // batch offsets fit a narrow record's int32
  unsigned long long nrec = 0;
  int n = (int)in[0];   // live entries (wave-uniform)
  int need = n;         // the most entries the table had to hold (an upper bound once it overflowed)
  int lost = 0;         // entries that found no room so far (counted on as if all of them survive)
  bool cap_over = false;
  // live partials as sdh_stats counts them everywhere: entries of the non-start states' pending lists
  // after the push's last event (the reference's two-phase add: a partial joins a list at one event and
  // is pending there from the next). Counted over the last tile's kept partials; header word 1
  int pend = (int)in[1];

  // the lanes holding `keep` store their entries (the LDS page's columns) at entries wpos .. of the
  // output table, in lane order; returns the new cursor (entries past the capacity are counted only)
  auto store_kept = [&](bool keep, int wpos) {
    const unsigned long long km = __ballot(keep);
    const int at = wpos + __popcll(km & below);
    if (keep && at < cap) {
      int64_t* d = out + WV_HDR + ((int64_t)(at >> 6) * ew) * 64 + (at & 63);
      for (int w = 0; w < ew; ++w) d[w * 64] = e.get(w);
    }
    return wpos + __popcll(km);
  };
  // a completed partial's record (collective): the narrow count record (nfa_types.h; key id 0 of the
  // engine's one-word key table: -1) when e1's distance fits int32, else the K_gen record
  auto emit_done = [&](int done, int len) {
    const unsigned long long dm = __ballot(done >= 0);
    nrec += __popcll(dm);  // (wave-uniform: lane 0 adds the wave's total at the end)
    if (!L.sink.write_records || !dm) return;
    const int64_t sq = done >= 0 ? t_seq[done] : 0;
    len = min(len, cmax);  // (a chain never outgrows its entry's words)
    const int64_t e1s = e.get(1);
    const bool nar = nb_ok && !L.wide && sq - e1s <= (int64_t)INT32_MAX;
    const int words = nar ? nrec_count_words(len) : 7 + 2 + 1 + len + 2;
    o.emit_n(done >= 0 ? 1 : 0, words, [&](auto r) {
      if (nar) {
        r[0] = nrec_pack(-(words + (NREC_KIND_COUNT << 16)), qid);
        r[1] = nrec_pack(sq - L.b.seq_base, 0);
        r[2] = nrec_pack(sq - e1s, len);
        for (int c = 0; c < len; c += 2)
          r[3 + c / 2] = nrec_pack(sq - e.get(3 + c), c + 1 < len ? sq - e.get(4 + c) : 0);
        return;
      }
      r[0] = words;
      r[1] = qid;
      r[2] = -1;  // an unpartitioned query's key
      r[3] = t_ts[done];
      r[4] = sq;
      r[5] = e1s;  // emission index: e1's seq (the pending-list order)
      r[6] = 3 | (stream << 16);
      r[7] = 1;
      r[8] = e1s;
      r[9] = len;
      for (int c = 0; c < len; ++c) r[10 + c] = e.get(3 + c);
      r[10 + len] = 1;
      r[11 + len] = sq;
    });
  };
  // the lanes with `alive` step their entries (LDS page) through events te_lo .. cnt-1, a lane from
  // its own te0 on; returns the event a lane's partial completed on (-1: none) and clears `alive` of
  // the partials that completed or died
  // new3: the partial entered e3's list at the tile's last event (it is in that list's pending
  // entries only from the next event on)
  auto step_page = [&](bool& alive, bool& new3, int te0, int te_lo, int cnt, unsigned long long m2) {
    const bool had = alive;
    new3 = false;
    int64_t fl = alive ? e.get(2) : 0;
    int done = -1;
    for (int te = te_lo; te < cnt; ++te) {
      if (!__ballot(alive)) break;
      const bool on = alive && te >= te0;
      // no lane in e3's list and the event does not pass f2: nothing can change (scalar test)
      if (!((m2 >> te) & 1) && !__ballot(on && wave_in3(fl))) continue;
      if (!on) continue;
      const WaveEv ev{&t_w[0][te], t_nul[te]};
      const bool was3 = wave_in3(fl);
      const int r = wave_step(e, fl, of, ncap, cmin, cmax, within, t_ts[te], t_seq[te], ev, (m2 >> te) & 1,
                              [&]() { return wave_f3(q, ev, part_ent(e, fl, of)); });
      if (r == WS_DONE) done = te;
      if (r != WS_KEEP) alive = false;
      if (te == cnt - 1) new3 = !was3 && wave_in3(fl);
    }
    if (had) e.set(2, fl);  // (a completed partial's record reads its length from it)
    return done;
  };

  for (int64_t t0 = 0; t0 < L.b.n; t0 += 64) {
    const int cnt = L.b.n - t0 < 64 ? (int)(L.b.n - t0) : 64;
    if (lane < cnt) {
      const int64_t p = t0 + lane;
      t_ts[lane] = L.b.ts[p];
      t_seq[lane] = L.b.seq_base + p;
      uint32_t nb = 0;
      for (int j = 0; j < L.na; ++j) {
        bool nl = false;
        t_w[j][lane] = j < ncap ? dev::raw_word(L.b, q->cap_attr[stream][j], p, nl) : 0;
        if (nl) nb |= 1u << j;
      }
      t_nul[lane] = nb;
    }
    __syncthreads();
    // f1 / f2 once per tile, lane = event (one call site: the interpreter is inlined once)
    unsigned long long m1 = 0, m2 = 0;
    for (int sid = 0; sid < 2; ++sid) {
      bool pass = false;
      if (lane < cnt) pass = wave_ev_filter(q, sid, WaveEv{&t_w[0][lane], t_nul[lane]});
      const unsigned long long m = __ballot(pass);
      m1 = sid == 0 ? m : m1;
      m2 = sid == 1 ? m : m2;
    }
    const int64_t* src = (t0 == 0 ? in : out) + WV_HDR;
    int wpos = 0;
    pend = 0;
    // the pages held before the tile, oldest first, then the fresh page: lane k holds the partial
    // event k opens, stepped from event k + 1
    const int np = (n + 63) >> 6;
    for (int pi = 0; pi <= np; ++pi) {
      const bool fresh = pi == np;
      if (fresh && !m1) break;
      bool alive;
      int te0 = 0, te_lo = 0;
      if (!fresh) {
        alive = pi * 64 + lane < n;
        if (alive) {
          const int64_t* s = src + ((int64_t)pi * ew) * 64 + lane;
          for (int w = 0; w < ew; ++w) e.set(w, s[w * 64]);
        }
      } else {
        alive = (m1 >> lane) & 1;
        if (alive) wave_open(e, of, ncap, t_ts[lane], t_seq[lane], WaveEv{&t_w[0][lane], t_nul[lane]});
        te0 = lane + 1;
        te_lo = __ffsll((long long)m1);
      }
      bool new3;
      const int done = step_page(alive, new3, te0, te_lo, cnt, m2);
      emit_done(done, done >= 0 ? wave_len(e.get(2)) : 0);
      wpos = store_kept(alive, wpos);
      // the pending-list entries the kept partials stand for (see `pend`): the count state's list
      // holds a partial while len < max, from the event after the one that opened it; e3's list from
      // the event after the one at which len reached min
      const int64_t fl = alive ? e.get(2) : 0;
      pend += __popcll(__ballot(alive && wave_len(fl) < cmax && !(fresh && lane == cnt - 1)));
      pend += __popcll(__ballot(alive && wave_in3(fl) && !new3));
    }
    if (wpos > cap) {
      cap_over = true;
      lost += wpos - cap;
    }
    n = min(wpos, cap);
    need = max(need, n + lost);
    __syncthreads();  // the tile is rewritten next; the next walk reads what this one stored
  }
  if (lane == 0) {
    out[0] = n;
    out[1] = pend;
  }
  o.close();
  if (lane == 0) {
    if (nrec) atomicAdd(L.sink.rec_count, nrec);
    if (cap_over) {
      atomicOr(&L.err[0], 1);
      atomicMax(&L.err[3], need);
    }
  }
  if (o.over) atomicOr(&L.err[2], 1);
}

// live partials of n tables: header word 1 (the pending-list entries, nfa_wave_kernel `pend`)
__global__ __launch_bounds__(256) void wave_live_kernel(const int64_t* __restrict__ st, int64_t n, int64_t stride,
                                                        unsigned long long* acc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long v = i < n ? (unsigned long long)st[i * stride + 1] : 0;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(acc, v);
}

}  // namespace sdh

extern "C" hipError_t sdh_launch_wave(const sdh::WaveLaunch* L, hipStream_t s) {
  if (L->n_items <= 0) return hipSuccess;
  const dim3 grid(L->xcd ? (L->n_items + 7) & ~7 : L->n_items);
  hipLaunchKernelGGL(sdh::nfa_wave_kernel, grid, dim3(64), (size_t)L->ew * 64 * 8, s, *L);
  return hipGetLastError();
}

extern "C" hipError_t sdh_live_wave(const int64_t* st, int64_t n, int64_t stride, unsigned long long* acc,
                                    hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sdh::wave_live_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st, n, stride, acc);
  return hipGetLastError();
}
