// engine_int.h -- what the engine's units (engine*.hip) share: the error type, device and host
// buffers, the lowered IR, `struct sdh_engine`, and the functions that cross a unit boundary.
// Everything here has hidden visibility: the library exports the C ABI (include/siddhi_hip.h) only.
//
//   engine.hip          the C ABI, knobs, sdh_engine_create (plan selection); the device match table and
//                       its polls; pushes; the multi-GPU exchange; the event store
//   engine_gen.hip      the K_gen family (K_gen / K_seq / K_part / K_slab / K_wave): sets and groups, arena and
//                       table growth, the journal, partition routing and the launches of a push
//   engine_lower.hip    the callers of the host-side lowerings (chain_lower.h, select_lower.h)
//   engine_ratchet.hip  K_chain and K_ratchet / K_gate / shared-pops launches
//   engine_slab.hip     K_slab arena maintenance
//   engine_snap.hip     the snapshot blob: format, prologue and the order of its sections, each a
//                       snap_save_X / snap_load_X pair in the unit that owns that state
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <tuple>
#include <array>
#include <cmath>
#include <map>
#include <unordered_map>
#include <memory>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/siddhi_hip.h"
#include "chain_lower.h"
#include "comm.h"
#include "knobs.h"
#include "gen_lower.h"
#include "nfa_types.h"
#include "select_lower.h"
#include "slab.h"
#include "snap_io.h"

#pragma GCC visibility push(hidden)

namespace sdh {
namespace eng {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) throw Error(SDH_E_DEVICE, fmt("%s: %s", #x, hipGetErrorString(e_))); \
  } while (0)

// (the IR as read, a query lowered to a ChainQuery, the K_ratchet plan, fmt: chain_lower.h)

// SDH_ALLOC_TRACE=1: one stderr line per device buffer (re)allocation (p99 push/poll latency hunts)
inline void alloc_trace(const char* what, size_t bytes) {
  const bool on = sdh::knob("SDH_ALLOC_TRACE") != nullptr;
  if (on) fprintf(stderr, "[sdh] alloc %s %zu bytes\n", what, bytes);
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  // grows by at least half its size (a buffer sized per push or per poll would otherwise be freed and
  // allocated again whenever the count edges up: hipFree synchronises the device, a p99 spike)
  // The first allocation takes an eighth more than asked: a buffer sized exactly by its first push
  // or poll reallocated at the next one a few elements larger (C2's 64K-push leg: a 1.1-s poll, eight
  // ~4-GB hipFree + hipMalloc pairs)
  void ensure(size_t want) {
    if (want <= n) return;
    const size_t cap = std::max(want + want / 8, n + n / 2);
    alloc_trace("ensure", cap * sizeof(T));
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    n = 0;
    if (hipMalloc(&p, cap * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      HIPCHK(hipMalloc(&p, want * sizeof(T)));
      n = want;
      return;
    }
    n = cap;
  }
  // grow to at least `want` elements keeping the first `keep` (stream-ordered copy)
  void grow_keep(size_t want, size_t keep, hipStream_t s) {
    if (want <= n) return;
    // (an eighth more on the first allocation, as ensure; and at least 1 MB: growing state tables of a
    // few hundred KB doubled inside small pushes -- C2's 1-event pushes, a 1.1-ms p99)
    size_t cap = std::max(std::max(want + want / 8, n * 2), ((size_t)1 << 20) / sizeof(T));
    alloc_trace("grow_keep", cap * sizeof(T));
    T* q = nullptr;
    if (hipMalloc(&q, cap * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      cap = want;
      if (hipMalloc(&q, cap * sizeof(T)) != hipSuccess)
        throw Error(SDH_E_CAPACITY, fmt("device memory exhausted growing a %zu-byte buffer", cap * sizeof(T)));
    }
    if (p && keep) HIPCHK(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (p) HIPCHK(hipFree(p));
    p = q;
    n = cap;
  }
  void swap(DevBuf& o) {  // (a grown copy takes the buffer's place; the old one is freed with `o`)
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// host output buffer of a poll: pinned when the runtime grants it (faster D2H), else pageable
template <class T>
struct HostBuf {
  T* p = nullptr;
  size_t n = 0;
  bool pinned = false;
  void ensure(size_t want) {
    if (want <= n) return;
    release();
    const size_t cap = std::max(want + want / 8, n * 2);  // (an eighth of headroom, as DevBuf)
    alloc_trace("host", cap * sizeof(T));
    if (hipHostMalloc((void**)&p, cap * sizeof(T), hipHostMallocDefault) == hipSuccess) {
      pinned = true;
    } else {
      (void)hipGetLastError();
      p = (T*)malloc(cap * sizeof(T));
      if (!p) throw Error(SDH_E_CAPACITY, "host memory exhausted for the poll output");
      pinned = false;
    }
    n = cap;
  }
  void release() {
    if (!p) return;
    if (pinned) (void)hipHostFree(p);
    else free(p);
    p = nullptr;
  }
  ~HostBuf() { release(); }
};

}  // namespace eng
}  // namespace sdh

// (a global-scope type of the ABI: its members name sdh:: and sdh::eng:: types unqualified)
using namespace sdh;
using namespace sdh::eng;

struct sdh_engine {
  sdh_config cfg{};
  int dev = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  IProgram prog;
  std::vector<Lowered> lq;           // local (this shard's) queries
  int K = 1, pcap = 64, rec_words = 3;
  // K_chain tables: partials_per_inst == 0 grows them on overflow (chain_grow), past 512 partials or
  // under SDH_CHAIN_PAGED in the paged form (nfa_chain.hip), whose earlier chunks work in d_pscratch
  bool chain_growing = false, chain_paged = false, chain_force_paged = false;
  int64_t chain_regrows = 0;         // table growths so far (sdh_stats.pool_regrows)
  DevBuf<int64_t> d_pscratch;
  DevBuf<ChainQuery> d_q;
  DevBuf<kg::GInsn> d_rcode;         // the K_chain queries' residual programs (chain_pred.h), one table
  bool chain_resid = false;          // a K_chain query has one: the R = true kernels run
  DevBuf<InstHeader> d_hdr[2];
  DevBuf<int64_t> d_part[2];
  std::vector<int> cur;              // which buffer holds each local query's state
  // interleaved pushes (sdh_engine_push_mixed; mixed.hip): `mix` is set while a native
  // call's launches run (launch_once then takes the MIX = true K_chain kernels, gen_pass the mixed walk
  // of nfa_gen_kernel over the unpartitioned groups that read a stream of mix_mask: the named streams
  // with events in the call); the pre-pass's outputs, and the host parts' columns in HBM (one buffer per
  // part: d_batch holds one batch)
  const MixLaunch* mix = nullptr;
  uint32_t mix_mask = 0;
  DevBuf<MixLaunch> d_mix;
  DevBuf<int32_t> d_mix_order, d_mix_idx, d_mix_pos, d_mix_cnt, d_mix_pstream, d_mix_err;
  DevBuf<int64_t> d_mix_ts, d_mix_total;
  DevBuf<uint8_t> d_mix_batch[MIX_MAXP];
  int64_t mixed_native = 0, mixed_split = 0;  // calls so far by path (sdh_engine_debug_mixed_pushes)
  // batch staging for host-resident input
  DevBuf<uint8_t> d_batch;           // a host batch's columns in HBM (stage_host_batch)
  HostBuf<uint8_t> stage[2];         // pinned staging slots
  hipEvent_t ev_stage[2] = {nullptr, nullptr}, ev_h0 = nullptr, ev_h1 = nullptr;
  int stage_next = 0;
  hipStream_t h2d = nullptr;         // side stream of host-to-device batch copies
  std::vector<int64_t> prev_ts;      // per stream
  int64_t seq = 0;
  // last launch
  DevBuf<WorkItem> d_work;
  DevBuf<int64_t> d_seg_count, d_seg_off, d_dst_off, d_match;
  DevBuf<int32_t> d_err;
  std::vector<WorkItem> work;
  std::vector<int64_t> seg_count;
  int64_t device_matches = 0;        // K_chain matches of the last push
  // device match table (matches.hip): every match since the last poll with its R18 sort keys
  struct Table {
    DevBuf<uint64_t> hi, lo[MAXLO];
    DevBuf<int64_t> seq, q, key, ts, woff, wlen, words;
    int64_t n = 0, nw = 0;           // rows / words used
    int n_lo = 0;                    // tiebreak passes the rows need
    bool placed = false;             // the rows are K_ratchet matches already in R18 order in po_*
    // chunk delivery keys (nfa_types.h): allocated once a chunk push joins the window; rows
    // [0, ck_n) have theirs, the rest are single-event rows filled at the poll
    DevBuf<uint64_t> chi, clo;
    bool chunked = false;
    bool chunk_pushed = false;       // a chunk push joined the window (every rank alike: same pushes)
    int64_t ck_n = 0;
    int64_t max_run = 0;             // largest run start / key position a chunk row carries
  } mt;
  // the chunk push in progress (sdh_batch.chunk): its first event's seq, its length, and per
  // partition keyed on its stream each event's same-key run start (ck_runs[slot][event])
  struct Chunk {
    bool active = false;
    int64_t first_seq = 0, n = 0;
    int stream = -1;
  } ck;
  DevBuf<int32_t> ck_runs, d_ck_major, d_ck_minor, d_ck_qslot;
  std::vector<int32_t> ck_major, ck_minor;  // [query][stream] subscriber rank (+1), rank in partition
  int64_t seq_ref = 0;               // global seq at the last poll (<= every trigger seq in mt)
  DevBuf<int32_t> d_out_rank;        // [query][stream] R18 receiver rank
  DevBuf<int32_t> d_qinfo;           // [query] (states, stream of the last state)
  // poll scratch and outputs (device), host copies of the outputs
  DevBuf<uint64_t> p_keys;
  DevBuf<int32_t> p_perm;
  DevBuf<uint8_t> p_temp;
  DevBuf<int64_t> po_q, po_key, po_ts, po_seq, po_tb, po_len, po_off, po_words;
  HostBuf<int64_t> ho_q, ho_key, ho_ts, ho_seq, ho_tb, ho_off, ho_words;
  // compact rows (sdh_matches_compact): a placed window's rows live here (the ABI columns are
  // filled from them at a full poll), with the window's event times ts_log[seq - seq_ref]; cw =
  // 2 + the most states any query has
  DevBuf<int32_t> pc_rows, pc_err;
  DevBuf<int64_t> ts_log;
  HostBuf<int32_t> hc_rows;
  int cw = 4;
  // ---- event store and device selector (select.hip; sdh_engine_retain_events / sdh_engine_poll_rows) ----
  // ev_cap == 0: no retention, and no push does any work for it. Otherwise ev_rows is a ring of ev_cap
  // (a power of two) rows of ev_w words indexed by seq; events [max(ev_first, seq - ev_cap), seq) are present
  int64_t ev_cap = 0, ev_first = 0;
  int ev_w = 2;
  DevBuf<int64_t> ev_rows;
  sel::Program selp;                 // the select lists, lowered (select_lower.h) at the first retain
  bool sel_ready = false;
  DevBuf<kg::GInsn> d_sel_code;
  DevBuf<sel::Out> d_sel_outs;
  DevBuf<sel::Shape> d_sel_shapes;
  DevBuf<sel::Query> d_sel_queries;
  DevBuf<int64_t> d_sel_consts;
  DevBuf<int32_t> pr_q, pr_err;      // sdh_rows outputs (ts / seq share po_ts / po_seq)
  DevBuf<int64_t> pr_cells;
  DevBuf<uint64_t> pr_nulls;
  HostBuf<int32_t> hr_q;
  HostBuf<int64_t> hr_cells;
  HostBuf<uint64_t> hr_nulls;
  // sdh_engine_records_rows: the window's rows (sized by max_rows, reused across calls) and what a push's
  // records need once to be located by row -- the flat records' word offsets (select.hip
  // flat_heads_kernel) and the K_chain segments' first rows; rr_ready: bit p = part p's is made
  DevBuf<int32_t> rr_q;
  DevBuf<int64_t> rr_ts, rr_seq, rr_cells;
  DevBuf<uint64_t> rr_nulls;
  HostBuf<int32_t> hrr_q;
  HostBuf<int64_t> hrr_ts, hrr_seq, hrr_cells;
  HostBuf<uint64_t> hrr_nulls;
  DevBuf<int64_t> rr_rec_off, rr_seg_off, rr_seg_row;
  DevBuf<unsigned long long> rr_heads;
  DevBuf<uint8_t> rr_tmp;            // (the walk's tables: 6 bytes per word of the flat buffer)
  int rr_ready = 0;
  // ---- K_gen (general interpreter) ----
  kg::LProgram lp;                   // full IR (receivers, runtime tree, partitions)
  std::vector<int> out_rank;         // R18 rank per (query, stream)
  std::vector<kg::GQuery> gq;
  DevBuf<kg::GQuery> d_gq;
  std::vector<int32_t> lane_q;       // [group][64]
  DevBuf<int32_t> d_lane_q;
  DevBuf<int64_t> d_lconst;          // [group][lc_slots][64] lane constants (kg::LaneConsts)
  int lc_slots = kg::LC_FIRST;
  std::vector<int32_t> group_tmpl;   // [group] shape template (a member query)
  DevBuf<int32_t> d_group_tmpl;
  std::vector<int32_t> group_seq;    // [group] window length S when the group runs on K_seq, else 0
  std::map<int, hipFunction_t> seq_spec;  // K_seq shape template -> its shape-compiled kernel (spec.h)
  std::vector<DevBuf<int32_t>> d_glists;  // [stream] unpartitioned groups: K_seq rows, then K_gen groups
  std::vector<DevBuf<int64_t>> seq_tail;  // [stream] last SEQ_TMAX events (K_seq windows)
  std::vector<int32_t> seq_tail_len;
  int gB32 = 1, gB64 = 1;
  int gHotS = 1, gHotNU = 1;  // K_gen LDS hot-word cache extents (max states / node-mask words)
  kg::Sizing gsz;                    // K_gen pool sizing (grows on overflow: gen_relayout)
  // absent states (kgen.h fire_timers): the runtime's start time and whether any query has them
  bool started = false;
  int64_t start_ts = 0;
  bool has_absent = false;
  bool has_fanout = false;           // a partition query reads a stream the partition does not key
  DevBuf<int32_t> d_fan_rank;        // [query][stream] its rank within the partition (fan-out), -1
  int64_t advance_to = INT64_MIN;    // set while a time advance runs (sdh_engine_advance_time)
  std::vector<char> gq_arena;        // [gq] the query runs on K_gen (has an instance arena)
  std::vector<uint32_t> gq_kind;     // [gq] the plan that runs the query, as a mixplan::Consumer bit (mix_plan.h)
  int64_t gen_regrows = 0;           // pool growths so far (sdh_stats)
  struct GenSet {
    int partition = -1;              // -1: the unpartitioned K_gen queries
    int group_base = 0, n_groups = 0;
    int64_t key_cap = 0;             // instance blocks = key_cap * n_groups (partitioned)
    bool timed = false;              // a group has absent states (a timer queue): time passes for the set
    DevBuf<int32_t> a32;
    DevBuf<int64_t> a64;
    DevBuf<int32_t> s32;             // scratch arenas of event chunks 1.. (unpartitioned sets)
    DevBuf<int64_t> s64;
    // exact re-runs: the blocks the current pass modifies, as they were before it (gen_journal)
    DevBuf<int32_t> j32;
    DevBuf<int64_t> j64, jidx;
    int64_t jn = 0;
    // interleaved pushes: the K_gen groups that read a stream of the call, cached by the call's mix_mask
    std::map<uint32_t, DevBuf<int32_t>> mix_glists;
  };
  std::vector<std::unique_ptr<GenSet>> gsets;
  // per partition: PartitionRuntime's key -> instance map (dense key ids), shared by the
  // partition's K_gen set and K_part sets (PartitionRuntime.java:257-306)
  struct Route {
    DevBuf<unsigned long long> tkey;
    DevBuf<int32_t> tid, n_keys;
    DevBuf<int64_t> key_of_id;
    int64_t tmask = 0, max_keys = 0;
    // fan-out partitions: keys in creation order (dense id, value), for the junction-map order
    bool track = false;
    int kkind = 0;                   // key values: 0 int / long, 1 bool, 2 string (dictionary ids),
                                     // 3 float, 4 double (raw bits; NaN canonical)
    int64_t nk_seen = 0;
    std::vector<int64_t> korder_kid, korder_key;
    DevBuf<int64_t> nk_tmp;
    struct Fan {
      int64_t n = -1;  // keys the positions cover
      DevBuf<int32_t> pos;
    };
    std::map<int, Fan> fan;  // [stream] per-kid positions in that stream's junction map
  };
  std::vector<std::unique_ptr<Route>> routes;  // [partition] (null: no device set uses it)
  // K_part (nfa_part.hip): one set per (partition, kind, stream); state blocks (key, group) double-buffered
  // per key: cur[kid] says which of st[0] / st[1] holds the key's current tables
  struct PartSet {
    int partition = -1, kind = 0, stream = 0;  // (the one stream every query of the set reads)
    int group_base = 0, n_groups = 0;
    int cap = 8, ew = 3, sA = 1, sB = 2, cmax = 0, n_e1 = 0, n_first = 0, n_last = 0;
    int64_t key_cap = 0;
    bool ran = false;                // launched in the current pass
    DevBuf<int64_t> st;              // [2][key_cap * n_groups][PK_HDR + cap * ew][64]
    DevBuf<int32_t> cur, nxt;        // [key_cap]
    int64_t bw() const { return PK_HDR + (int64_t)cap * ew; }
    std::map<int, hipFunction_t> spec;  // shape template -> shape-compiled kernel (spec.h)
  };
  std::vector<std::unique_ptr<PartSet>> psets;
  int64_t part_regrows = 0;          // K_part table growths so far (sdh_stats.pool_regrows)
  int part_chain_lo = 0;            // PK_CHAIN sets: the tiebreak passes their rows need (states - 1; 0: none)
  // K_wave (nfa_wave.hip): one set per stream; a wave per query, a lane per partial. Two tables per
  // query, st[cur] the current ones; a push writes st[1 - cur] and the host swaps once it is accepted
  struct WaveSet {
    int stream = 0;
    std::vector<int32_t> qs;         // the set's queries (indices into gq), one work item each
    DevBuf<int32_t> d_qs;
    int cap = 64;                    // entries per table: 64 x pages (grows on overflow: wave_grow_cap). One
                                     // capacity per set: a deep query grows every table of its stream's set
    int ew = 3, cmax = 0, n_e1 = 0, n_first = 0, n_last = 0, na = 0;
    int cur = 0;
    bool ran = false;                // launched in the current pass
    DevBuf<int64_t> st[2];           // [query][WV_HDR + cap * ew]
    int64_t stride() const { return WV_HDR + (int64_t)cap * ew; }
  };
  std::vector<std::unique_ptr<WaveSet>> wsets;
  DevBuf<int32_t> d_werr;            // per K_wave set: [0] table capacity, [2] output overflow, [3] entries needed
  DevBuf<unsigned long long> d_wave_live;  // one word: the accumulator of wave_live_partials
  DevBuf<int64_t> d_wave_key;        // one word, -1: the key table of the K_wave queries' narrow records
  int64_t wave_regrows = 0;          // K_wave table growths so far (sdh_stats.pool_regrows)
  int64_t wave_items = 0;            // K_wave work items of the last push
  // K_slab (nfa_slab.hip): one set per partition; its queries' partials as sparse entries, one block
  // per (key, group) in nsub sub-rings of a slab, found through the directory [key][group]
  struct SlabSet {
    int partition = -1;
    int group_base = 0, n_groups = 0;
    int64_t key_cap = 0;
    std::vector<slab::Shape> shapes;
    std::vector<int32_t> group_shape, group_ew;
    DevBuf<slab::Shape> d_shapes;
    DevBuf<int32_t> d_group_shape, d_group_ew;
    std::vector<std::vector<int32_t>> glist;  // [stream] set groups reading it
    std::vector<DevBuf<int32_t>> d_glist;
    DevBuf<uint64_t> dir;                     // [key_cap * n_groups]
    int nsub = 256;                           // sub-rings (separate buffers: they grow one at a time)
    std::vector<uint32_t*> ring;
    std::vector<int64_t> cap;                 // words per ring
    DevBuf<uint32_t*> d_ring;
    DevBuf<int64_t> d_cap;
    DevBuf<unsigned long long> head, tail, head_bak;
    std::vector<unsigned long long> h_head, h_tail, h_push0;  // h_push0: heads before the last push
    // Ring buffers are carved from an arena of large chunks that are never returned while the engine
    // lives: a ring that grows takes a new range and gives its old one back to the free list (adjacent
    // free ranges merge), so growing costs no driver allocation once the arena holds enough. (A
    // hipMalloc of GBs stalls for seconds from time to time on this driver, whether or not memory
    // was freed; tools/alloc_probe.py.) sdh_engine_reserve sizes the arena up front.
    struct Chunk {
      uint8_t* base;
      size_t bytes;
      std::map<size_t, size_t> free;  // offset -> length
    };
    std::vector<Chunk> chunks;
    size_t arena_bytes = 0;
    bool add_chunk(size_t bytes) {
      void* p = nullptr;
      alloc_trace("slab_chunk", bytes);
      if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      chunks.push_back(Chunk{(uint8_t*)p, bytes, {}});
      chunks.back().free[0] = bytes;
      arena_bytes += bytes;
      return true;
    }
    uint32_t* take(size_t bytes) {
      for (auto& c : chunks)
        for (auto it = c.free.begin(); it != c.free.end(); ++it) {
          if (it->second < bytes) continue;
          const size_t off = it->first, len = it->second;
          c.free.erase(it);
          if (len > bytes) c.free[off + bytes] = len - bytes;
          return (uint32_t*)(c.base + off);
        }
      return nullptr;
    }
    uint32_t* alloc_ring(int64_t words) {
      const size_t bytes = ((size_t)words * 4 + 4095) & ~(size_t)4095;
      if (uint32_t* p = take(bytes)) return p;
      // a new chunk: as large as the arena so far (the chunks double), or what the device still has
      size_t want = std::max(bytes, std::max(arena_bytes, (size_t)1 << 30));
      for (;;) {
        if (add_chunk(want)) return take(bytes);
        if (want == bytes) return nullptr;
        want = std::max(bytes, want / 2);
      }
    }
    void free_ring(uint32_t* p, int64_t words) {
      if (!p) return;
      const size_t bytes = ((size_t)words * 4 + 4095) & ~(size_t)4095;
      for (auto& c : chunks) {
        if ((uint8_t*)p < c.base || (uint8_t*)p >= c.base + c.bytes) continue;
        size_t off = (size_t)((uint8_t*)p - c.base), len = bytes;
        auto nx = c.free.lower_bound(off);
        if (nx != c.free.end() && nx->first == off + len) {
          len += nx->second;
          nx = c.free.erase(nx);
        }
        if (nx != c.free.begin()) {
          auto pv = std::prev(nx);
          if (pv->first + pv->second == off) {
            off = pv->first;
            len += pv->second;
            c.free.erase(pv);
          }
        }
        c.free[off] = len;
        return;
      }
    }
    ~SlabSet() {
      for (auto& c : chunks) (void)hipFree(c.base);
    }
    DevBuf<long long> live, live_bak;
    DevBuf<unsigned long long> traffic;       // block bytes read + written by the last launch
    DevBuf<uint64_t> journal, journal_idx;
    int64_t items = 0;                        // items of this pass's launch (0: not launched)
    int lds_words = 4096;                     // LDS rows (uint32 words) of the large tier
    int max_na = 1;                           // the widest captured-word count of the set's shapes
    DevBuf<int32_t> defer, defer_n;           // items deferred to the large tier (nfa_slab.hip)
    int64_t deferred = 0;
    int64_t cleanings = 0, growths = 0;
  };
  std::vector<std::unique_ptr<SlabSet>> ssets;
  DevBuf<int32_t> d_serr;            // per K_slab set: [0] LDS capacity, [1] slab space, [2] output overflow
  int64_t slab_items = 0;            // K_slab work items of the last push
  std::vector<int64_t> part_kept;    // per partition: events of the last push routed to a key here
  DevBuf<int32_t> d_perr;            // per K_part set: [0] entry capacity, [2] output overflow
  DevBuf<unsigned long long> d_pprof;  // SDH_PART_PROF measurement builds: phase clocks
  DevBuf<int64_t> r_key;
  DevBuf<int64_t> t_pm;              // indexed timer sweep: the batch's timestamp prefix max
  DevBuf<int32_t> t_kseg, t_flag;    // per known key its routed segment; ts-order flag
  DevBuf<uint8_t> t_temp;
  DevBuf<uint32_t> r_kid, r_kid_s, r_uniq;
  DevBuf<int32_t> r_idx, r_idx_s, r_cnt, r_off, r_nruns;
  DevBuf<uint8_t> r_temp;
  DevBuf<int64_t> g_out;
  int64_t g_out_cap = 0;             // K_gen match record words per push
  DevBuf<unsigned long long> g_out_next;
  DevBuf<unsigned long long> g_nrec;
  DevBuf<int64_t> g_rec_off;         // word offset of each K_gen / K_seq / K_part record of the last push
  DevBuf<int64_t> g_tw;              // their table words, scanned (append_gen)
  DevBuf<uint8_t> g_twtemp;
  DevBuf<unsigned long long> g_nwide;  // K_gen-format (not narrow) records of the last append
  // sdh_engine_poll_compact_ex outputs
  DevBuf<int64_t> px_cw, px_key, px_tb;
  DevBuf<int32_t> px_chain;
  DevBuf<uint8_t> px_temp;
  HostBuf<int64_t> hx_key, hx_tb;
  HostBuf<int32_t> hx_chain;
  DevBuf<const int64_t*> d_qkeys;    // [query] its partition's key table (narrow K_part records)
  DevBuf<uint8_t> sb_buf;            // a batch in key order (K_part reads; sdh_sort_batch)
  DevBuf<unsigned long long> g_rec_next;
  int64_t g_dev_matches = 0;         // K_gen / K_seq matches of the last push
  int64_t g_used = 0;                // words of the last push's records in g_out
  bool g_journal = false;            // the current K_gen pass journals the blocks it modifies
  // ---- K_ratchet groups ----
  std::vector<RatchetGroup> rg;
  std::vector<int> rcur;             // per group: buffer holding its deques
  DevBuf<RatchetGroup> d_rg;
  DevBuf<RatchetState> d_rst[2];
  DevBuf<int64_t> d_rts[2], d_rsq[2], d_rky[2];
  DevBuf<RatchetItem> d_ritems;
  std::vector<RatchetItem> ritems;
  DevBuf<int64_t> d_rmatch;
  DevBuf<int32_t> d_blk_count, d_blk_next, d_blk_group;
  DevBuf<int32_t> d_blk_side;            // K_ratchet rec4 blocks: side entries (-1: an 8- / 16-B block)
  // shared-pops form (nfa_ratchet_shared.hip): the pre-pass's tree, N(i) keys / values (unsorted and
  // sorted), pairs, counts, sort scratch, and the groups' carried matches
  DevBuf<float> d_shtree;
  DevBuf<uint32_t> d_shkv, d_shcnt;
  DevBuf<sdh::SharedPair> d_shpairs;
  DevBuf<uint8_t> d_shtemp;
  DevBuf<uint2> d_shcm;
  DevBuf<int32_t> d_shcmn;
  DevBuf<uint32_t> d_shbounds;           // [g][SH_BOUNDS] the groups' lane constants (ratchet_shared_carried)
  int64_t r_launches = 0;                // K_ratchet steps so far (SDH_RATCHET_SHARED_ALT)
  int64_t r_shared_pushes = 0;           // pushes whose records the shared-pops form wrote
  int64_t r_rec4_reruns = 0;             // pushes re-run with 8-B records (a rec4 distance reached 2^26)
  DevBuf<unsigned long long> d_rtotal;  // device records: [0] entries, [2] bytes written
  int r_wide = 0;
  int64_t r_blocks = 0;              // capacity in blocks
  int r_blk_recs = 8192;
  int r_blocks_used = 0;             // of the last launch
  int64_t r_blk_taken = 0;           // blocks the last launch took
  double r_rec_bytes = 0;            // device records: bytes the last launch wrote (entries + side entries)
  int r_rec4 = 0;                    // device records: the last launch wrote rec4 blocks (SIM launches)
  DevBuf<int32_t> d_rlane_q;         // [group][64] query of each K_ratchet lane (-1 idle; sdh_records)
  DevBuf<int64_t> d_rrow_off;        // sdh_engine_records_compact: per-block row offsets
  DevBuf<uint8_t> d_rrow_tmp;
  bool dev_polled = false;           // the last push's device records were handed out
  int64_t last_n = 0, last_seq_base = 0;  // the last push's events and first seq
  // direct R18 placement (nfa_ratchet.hip PM): the (event, group cell) match counts, scanned
  DevBuf<int32_t> p_cnt;
  std::vector<int> place_cells;     // [stream] K_ratchet groups reading it (0: not placeable)
  // string dictionary ids -> (String.hashCode, UTF-16 length) of their text (sdh_engine_set_strings):
  // the fan-out order of partitions keyed by a string attribute
  std::unordered_map<int32_t, std::pair<int32_t, int64_t>> str_info;
  bool r_placing = false;            // the last K_ratchet launch placed its matches (compact rows)
  int64_t r_place_row0 = 0;          //   from this row of pc_rows
  DevBuf<uint8_t> p_ptemp;
  int64_t r_seq_base = 0;            // seq of the last launch's first event
  std::vector<int32_t> r_blk_count;
  int slab_lds_small = 1024;          // K_slab small-tier LDS rows (SDH_SLAB_LDS_SMALL)
  int xcd = 0;                       // per-XCD item ranges in the K_gen / K_seq / K_part / K_slab launches
                                     // (dev::grid_item; SDH_XCD=1: measured neutral)
  int rML = 8;                       // LDS ring entries per lane (power of two)
  double r_waves = 0;                // resident-wave target per launch (0: CUs x occupancy)
  int n_cu = 256;
  std::vector<std::array<int, 4>> r_sum_specs;  // tile-summary rows: (stream, attr, conv, key kind)
  DevBuf<uint64_t> d_tsmax, d_tsmin;
  DevBuf<uint8_t> d_tshas;
  int rSC = 256;                     // global spill ring entries per lane (power of two)
  int64_t rsmax = RSMAX;             // persisted deque entries per lane (grows with rSC)
  DevBuf<uint4> d_rspillA;
  DevBuf<int64_t> d_rlts;
  DevBuf<uint32_t> d_rspillB;
  std::vector<char> r_full_expiry;   // per stream: timestamps were seen out of order
  int64_t r_matches = 0;
  double r_kernel_ms = 0, r_kernel_bytes = 0;
  sdh_stats stats{};
  std::string err;
  std::string broken;                // set when a failed push left the state undefined
  std::vector<std::pair<std::string, std::string>> knobs;  // sdh_config.debug (knobs.h)
  // ---- multi-GPU exchange (comm.h; sdh_engine_push_bcast / sdh_engine_gather) ----
  sdh_comm* comm = nullptr;          // not owned
  DevBuf<uint8_t> x_batch;           // a broadcast batch received from the root
  DevBuf<uint64_t> x_keys;           // this rank's merge keys, one run
  // rank 0: every rank's run concatenated, and the merged output
  DevBuf<int64_t> xg_q, xg_key, xg_ts, xg_seq, xg_tb, xg_off, xg_words;
  DevBuf<uint64_t> xg_keys;
  DevBuf<int64_t> go_q, go_key, go_ts, go_seq, go_tb, go_len, go_off, go_src, go_pos, go_words;
  DevBuf<uint8_t> go_temp;
};

namespace sdh {
namespace eng {

// the most partials per query the register forms of K_chain hold; past it the tables are paged. With
// a residual program in the engine that is 256: the eight-set R = true form of a chain of two or more
// states does not fit the registers without private memory, so it is not built
inline int chain_reg_limit(const sdh_engine* e) { return e->chain_resid ? 256 : 512; }

// a small device value the host decides on: copied over the engine's stream, which is then drained
inline void d2h_sync(sdh_engine* e, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
}

// a device range into / out of a snapshot blob (snap_io.h)
inline void put_dev(snap::Writer& w, const void* dptr, size_t bytes) {
  void* to = w.bytes(bytes);
  if (bytes) HIPCHK(hipMemcpy(to, dptr, bytes, hipMemcpyDeviceToHost));
}
inline void get_dev(snap::Reader& r, void* dptr, size_t bytes) {
  const void* from = r.bytes(bytes);
  if (bytes) HIPCHK(hipMemcpy(dptr, from, bytes, hipMemcpyHostToDevice));
}

// ---- functions that cross a unit boundary, by defining unit ----
// engine.hip
void snap_save_events(sdh_engine* e, snap::Writer& w), snap_load_events(sdh_engine* e, snap::Reader& r, bool stored);
// engine_lower.hip
IProgram read_ir(const void* blob, size_t len);
Lowered lower_chain(const IProgram& P, int qi);
int attr_width(int t);
sel::Program lower_outputs(const kg::LProgram& P);
// engine_gen.hip
void gen_build(sdh_engine* e, const std::vector<int>& qis);
void gen_grow(sdh_engine* e, sdh_engine::GenSet& gs, int64_t keys);
void gen_relayout(sdh_engine* e, const kg::Sizing& sz, bool remap);
void check_fan_strings(const sdh_engine* e, int stream);
double gen_journal_bound(sdh_engine* e, int64_t n);
void part_grow(sdh_engine* e, sdh_engine::PartSet& ps, int64_t keys);
void launch_gen(sdh_engine* e, int stream, const StreamBatch& B, double* ms_out, double* bytes_out);
void snap_save_gen(sdh_engine* e, snap::Writer& w), snap_load_gen(sdh_engine* e, snap::Reader& r);
void snap_save_routes(sdh_engine* e, snap::Writer& w), snap_load_routes(sdh_engine* e, snap::Reader& r);
void snap_save_part(sdh_engine* e, snap::Writer& w), snap_load_part(sdh_engine* e, snap::Reader& r);
void snap_save_seq(sdh_engine* e, snap::Writer& w), snap_load_seq(sdh_engine* e, snap::Reader& r);
void snap_save_wave(sdh_engine* e, snap::Writer& w), snap_load_wave(sdh_engine* e, snap::Reader& r);
int64_t wave_live_partials(sdh_engine* e);
// engine_ratchet.hip
void launch(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2],
            const std::vector<int>& qs, bool allow_chunks, bool* unordered);
void ratchet_build(sdh_engine* e, std::vector<std::pair<RatchetPlan, int>>& plans);
void launch_ratchet(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2]);
void snap_save_chain(sdh_engine* e, snap::Writer& w), snap_load_chain(sdh_engine* e, snap::Reader& r, int64_t spcap);
void snap_save_ratchet(sdh_engine* e, snap::Writer& w), snap_load_ratchet(sdh_engine* e, snap::Reader& r);
// engine_slab.hip
void slab_heads(sdh_engine* e, sdh_engine::SlabSet& ss);
void slab_init(sdh_engine* e, sdh_engine::SlabSet& ss, int64_t cap);
void slab_grow_keys(sdh_engine* e, sdh_engine::SlabSet& ss, int64_t keys);
void slab_prepare(sdh_engine* e, sdh_engine::SlabSet& ss, const std::vector<int64_t>* demand = nullptr);
void slab_rollback(sdh_engine* e, sdh_engine::SlabSet& ss);
int64_t slab_live_partials(sdh_engine* e, const sdh_engine::SlabSet& ss);
int64_t slab_live_words(sdh_engine* e, const sdh_engine::SlabSet& ss);
void snap_save_slab(sdh_engine* e, snap::Writer& w), snap_load_slab(sdh_engine* e, snap::Reader& r);
// engine_snap.hip
void snap_save(sdh_engine* e, snap::Writer& w);
void snap_load(sdh_engine* e, snap::Reader r);

}  // namespace eng
}  // namespace sdh

#pragma GCC visibility pop
