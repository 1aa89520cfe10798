// engine_slab.hip -- K_slab arena maintenance: directory growth, slab space, cleaning, rollback.
#include "engine_int.h"
#include "launchers.h"

namespace sdh {
namespace eng {

// ------------------------------------------------------------------------------------------
// K_slab host side (nfa_slab.hip): directory growth with the key table, slab space (reclaiming a
// sub-ring's oldest half, growing), rollback of a failed push
// ------------------------------------------------------------------------------------------
void slab_heads(sdh_engine* e, sdh_engine::SlabSet& ss) {
  ss.h_head.resize(ss.nsub);
  HIPCHK(hipMemcpyAsync(ss.h_head.data(), ss.head.p, ss.nsub * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
}

namespace {

void slab_upload_rings(sdh_engine::SlabSet& ss) {
  HIPCHK(hipMemcpy(ss.d_ring.p, ss.ring.data(), ss.nsub * sizeof(uint32_t*), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ss.d_cap.p, ss.cap.data(), ss.nsub * 8, hipMemcpyHostToDevice));
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

uint32_t* ring_malloc(sdh_engine* e, sdh_engine::SlabSet& ss, int64_t words) {
  (void)e;
  uint32_t* p = ss.alloc_ring(words);
  if (!p) throw Error(SDH_E_CAPACITY, fmt("device memory exhausted allocating a %.2f GB K_slab ring", words * 4.0 / 1e9));
  return p;
}

}  // namespace

// fresh, empty sub-rings of `cap` words each
void slab_init(sdh_engine* e, sdh_engine::SlabSet& ss, int64_t cap) {
  for (size_t r = 0; r < ss.ring.size(); ++r) ss.free_ring(ss.ring[r], r < ss.cap.size() ? ss.cap[r] : 0);
  cap = (cap + 3) & ~3ll;
  ss.ring.assign(ss.nsub, nullptr);
  ss.cap.assign(ss.nsub, cap);
  for (auto& p : ss.ring) p = ring_malloc(e, ss, cap);
  ss.d_ring.ensure(ss.nsub);
  ss.d_cap.ensure(ss.nsub);
  slab_upload_rings(ss);
  ss.head.ensure(ss.nsub);
  ss.tail.ensure(ss.nsub);
  ss.head_bak.ensure(ss.nsub);
  HIPCHK(hipMemset(ss.head.p, 0, ss.nsub * 8));
  HIPCHK(hipMemset(ss.tail.p, 0, ss.nsub * 8));
  ss.h_head.assign(ss.nsub, 0);
  ss.h_tail.assign(ss.nsub, 0);
  ss.h_push0.assign(ss.nsub, 0);
  ss.live.ensure(256);
  ss.live_bak.ensure(256);
  ss.traffic.ensure(256);
  HIPCHK(hipMemset(ss.live.p, 0, 256 * 8));
}

// directory room for `keys` keys (key-major: the old entries are a prefix; new keys' blocks empty)
void slab_grow_keys(sdh_engine* e, sdh_engine::SlabSet& ss, int64_t keys) {
  if (keys <= ss.key_cap) return;
  int64_t cap = std::max<int64_t>(64, ss.key_cap);
  while (cap < keys) cap *= 2;
  const size_t old_n = (size_t)ss.key_cap * ss.n_groups, new_n = (size_t)cap * ss.n_groups;
  DevBuf<uint64_t> nd;
  if (hipMalloc(&nd.p, new_n * 8) != hipSuccess)
    throw Error(SDH_E_CAPACITY, fmt("device memory exhausted growing the K_slab directory to %lld keys", (long long)cap));
  nd.n = new_n;
  HIPCHK(hipMemsetAsync(nd.p + old_n, 0, (new_n - old_n) * 8, e->stream));
  if (old_n) HIPCHK(hipMemcpyAsync(nd.p, ss.dir.p, old_n * 8, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  ss.dir.swap(nd);
  ss.key_cap = cap;
}

namespace {

// One directory pass moving blocks (nfa_slab.hip slab_move_kernel); false if a destination ring
// ran out of room (nothing is lost: a block keeps its old place until its directory word moves)
bool slab_move_raw(sdh_engine* e, sdh_engine::SlabSet& ss, uint64_t* dir, uint32_t* const* src_ring,
                   const int64_t* src_cap, const unsigned long long* src_tail, int src_nsub,
                   const std::vector<unsigned long long>& limit, const std::vector<uint8_t>& active,
                   uint32_t* const* dst_ring, const int64_t* dst_cap, unsigned long long* dst_head,
                   const unsigned long long* dst_tail, int dst_nsub, std::vector<uint8_t>* ring_fail = nullptr) {
  DevBuf<unsigned long long> d_lim;
  DevBuf<uint8_t> d_act;
  d_lim.ensure(limit.size());
  HIPCHK(hipMemcpyAsync(d_lim.p, limit.data(), limit.size() * 8, hipMemcpyHostToDevice, e->stream));
  if (!active.empty()) {
    d_act.ensure(active.size());
    HIPCHK(hipMemcpyAsync(d_act.p, active.data(), active.size(), hipMemcpyHostToDevice, e->stream));
  }
  e->d_err.ensure(4);
  HIPCHK(hipMemsetAsync(e->d_err.p, 0, 16, e->stream));
  DevBuf<uint8_t> d_rf;
  if (ring_fail) {
    d_rf.ensure(dst_nsub);
    HIPCHK(hipMemsetAsync(d_rf.p, 0, dst_nsub, e->stream));
  }
  HIPCHK(sdh_slab_move(dir, ss.key_cap * ss.n_groups, ss.n_groups, ss.d_group_ew.p, src_ring, src_cap, src_tail,
                       src_nsub, d_lim.p, active.empty() ? nullptr : d_act.p, dst_ring, dst_cap, dst_head, dst_tail,
                       dst_nsub, e->d_err.p, ring_fail ? d_rf.p : nullptr, e->stream));
  int32_t err = 0;
  HIPCHK(hipMemcpyAsync(&err, e->d_err.p, 4, hipMemcpyDeviceToHost, e->stream));
  if (ring_fail) {
    ring_fail->assign(dst_nsub, 0);
    HIPCHK(hipMemcpyAsync(ring_fail->data(), d_rf.p, dst_nsub, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return err == 0;
}

// rings `which` into new buffers of new_cap[r] words holding their live blocks (a batch at a time,
// so the extra memory is a batch's worth)
void slab_grow(sdh_engine* e, sdh_engine::SlabSet& ss, const std::vector<int>& which,
               const std::vector<int64_t>& new_cap) {
  // (up to 32 rings and 8 GB of new buffers at a time: old and new buffers coexist while a batch
  // moves, and C5's rings reach GBs each -- 32 at a time took tens of GB on top of the state)
  const int BATCH = 32;
  const int64_t BATCH_WORDS = (int64_t)2 << 30;
  for (size_t b0 = 0, b1 = 0; b0 < which.size(); b0 = b1) {
    const double t_start = now_ms();
    std::vector<uint32_t*> nring(ss.ring);
    std::vector<int64_t> ncap(ss.cap);
    std::vector<uint8_t> active(ss.nsub, 0);
    int64_t words = 0;
    for (b1 = b0; b1 < which.size() && b1 < b0 + BATCH && (b1 == b0 || words + new_cap[b1] <= BATCH_WORDS); ++b1) {
      const int r = which[b1];
      ncap[r] = (new_cap[b1] + 3) & ~3ll;
      nring[r] = ring_malloc(e, ss, ncap[r]);
      active[r] = 1;
      words += ncap[r];
    }
    DevBuf<uint32_t*> d_nr;
    DevBuf<int64_t> d_nc;
    DevBuf<unsigned long long> nh, nt;
    d_nr.ensure(ss.nsub);
    d_nc.ensure(ss.nsub);
    nh.ensure(ss.nsub);
    nt.ensure(ss.nsub);
    const double t_alloc = now_ms();
    HIPCHK(hipMemcpy(d_nr.p, nring.data(), ss.nsub * sizeof(uint32_t*), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nc.p, ncap.data(), ss.nsub * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(nh.p, 0, ss.nsub * 8));
    HIPCHK(hipMemset(nt.p, 0, ss.nsub * 8));
    if (!slab_move_raw(e, ss, ss.dir.p, ss.d_ring.p, ss.d_cap.p, ss.tail.p, ss.nsub,
                       std::vector<unsigned long long>(ss.nsub, ~0ull), active, d_nr.p, d_nc.p, nh.p, nt.p, ss.nsub))
      throw Error(SDH_E_CAPACITY, "K_slab: a ring overflowed while growing");
    std::vector<unsigned long long> moved(ss.nsub);
    HIPCHK(hipMemcpy(moved.data(), nh.p, ss.nsub * 8, hipMemcpyDeviceToHost));
    const double t_move = now_ms();
    for (int r = 0; r < ss.nsub; ++r) {
      if (!active[r]) continue;
      ss.free_ring(ss.ring[r], ss.cap[r]);
      ss.ring[r] = nring[r];
      ss.cap[r] = ncap[r];
      ss.h_head[r] = moved[r];
      ss.h_tail[r] = 0;
      ss.h_push0[r] = 0;
    }
    slab_upload_rings(ss);
    HIPCHK(hipMemcpy(ss.head.p, ss.h_head.data(), ss.nsub * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ss.tail.p, ss.h_tail.data(), ss.nsub * 8, hipMemcpyHostToDevice));
    ss.growths += (int64_t)(b1 - b0);
    if (sdh::knob("SDH_SLAB_TRACE"))
      fprintf(stderr, "[sdh] slab grow: %zu rings, %.2f GB: alloc %.1f ms, move %.1f ms, free %.1f ms\n", b1 - b0,
              words * 4e-9, t_alloc - t_start, t_move - t_alloc, now_ms() - t_move);
  }
}

}  // namespace

// Room for the next push in every ring. The rings are log-structured: a push appends the entries it
// changes, the old copies die in place. A ring whose free room falls below its live words plus 1.25x
// what it took in the last push is cleaned in place: every block written before that push moves to
// its head (the blocks of the last push are current) -- the oldest 4x the room the next push needs
// (SDH_SLAB_SPAN), mostly dead copies -- once its free room falls below 5x that need (SDH_SLAB_CLEAN_AT):
// a few pushes per cleaning, each a directory pass. A ring below 1.4x (live + headroom) words (SDH_SLAB_GROW_AT) moves
// its live blocks into a fresh buffer of 1.6x that (SDH_SLAB_GROW_TO): the reservation stays
// under 2x the live words, and the cleaning moves (wave-cooperative, nfa_slab.hip) are cheap enough
// to run at most pushes. A push that still overflows is undone and re-run with room for 1.25x its
// demand (re-runs cost time, never matches).
// (C5: cleaning only when a push lacked room never fit in place -- the ring was full by then -- so
// every cleaning reallocated; growing by the ring's span instead of its live words doubled the
// reservation every other step and ran out of HBM.)
// demand: words a failed push tried to take per ring (room for 1.25x that is made instead)
void slab_prepare(sdh_engine* e, sdh_engine::SlabSet& ss, const std::vector<int64_t>* demand) {
  const double t_prep = now_ms();
  std::vector<int64_t> need(ss.nsub);
  std::vector<unsigned long long> limit(ss.nsub);
  std::vector<uint8_t> clean(ss.nsub, 0);
  // live words per ring (one pass over the directory)
  std::vector<unsigned long long> live(ss.nsub, 0);
  {
    DevBuf<unsigned long long> acc;
    acc.ensure(ss.nsub);
    HIPCHK(hipMemsetAsync(acc.p, 0, ss.nsub * 8, e->stream));
    HIPCHK(sdh_slab_live_words_ring(ss.dir.p, ss.key_cap * ss.n_groups, ss.n_groups, ss.d_group_ew.p, ss.nsub, acc.p,
                                    e->stream));
    HIPCHK(hipMemcpyAsync(live.data(), acc.p, ss.nsub * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  bool any = false;
  for (int r = 0; r < ss.nsub; ++r) {
    const int64_t alloc = (int64_t)(ss.h_head[r] - ss.h_push0[r]);
    need[r] = std::max<int64_t>(alloc + alloc / 4, 4096);
    if (demand) need[r] = std::max<int64_t>(need[r], (*demand)[r] + (*demand)[r] / 4);
    const int64_t used = (int64_t)(ss.h_head[r] - ss.h_tail[r]);
    // clean once the room falls below SDH_SLAB_CLEAN_AT x the push's need (then the live blocks of
    // the span still fit at the head: the in-place move needs room for them, and a span holds at most
    // SDH_SLAB_SPAN x need live words)
    const double clean_at = sdh::knob("SDH_SLAB_CLEAN_AT") ? atof(sdh::knob("SDH_SLAB_CLEAN_AT")) : 3.0;
    if ((double)(ss.cap[r] - used) >= clean_at * (double)need[r]) continue;
    // the oldest quarter of the ring (at least twice the headroom): mostly dead copies, so the move
    // is small (SDH_SLAB_CLEAN=all: everything before the last push)
    const unsigned long long cur = ss.h_push0[r] > ss.h_tail[r] ? ss.h_push0[r] : ss.h_head[r];
    const bool all = sdh::knob("SDH_SLAB_CLEAN") && !strcmp(sdh::knob("SDH_SLAB_CLEAN"), "all");
    // (the span a push needs, not a fixed share of the ring: every live block in it moves, and the
    // oldest blocks of a ring are not all dead -- a quarter of the ring per push moved 15 % of C5's
    // device time. C5 sweep, CLEAN_AT:SPAN:GROW_TO -> slab_move share of the 24-step run, ms/step,
    // reserved/live: 5:4:1.6 10.0 %, 457, 1.80; 3:2:1.6 7.8 %, 458, 1.95; 3:2:1.5 8.8 %, 447, 1.75;
    // 4:3:1.6 9.0 %, 469, 1.96; 5:8:1.6 30 %, 632; 9:8:1.6 42 %, 822; GROW_TO 2.0 at 5:4 5.9 %, 2.13)
    const double span_x = sdh::knob("SDH_SLAB_SPAN") ? atof(sdh::knob("SDH_SLAB_SPAN")) : 2.0;
    const unsigned long long span = (unsigned long long)std::max<int64_t>((int64_t)(span_x * need[r]), 4096);
    limit[r] = all ? cur : std::min<unsigned long long>(cur, ss.h_tail[r] + span);
    clean[r] = 1;
    any = true;
  }
  std::vector<int> grow;
  std::vector<int64_t> gcap;
  if (any) {
    // (a ring's blocks move within that ring, so rings succeed or fail on their own)
    std::vector<uint8_t> fail;
    (void)slab_move_raw(e, ss, ss.dir.p, ss.d_ring.p, ss.d_cap.p, ss.tail.p, ss.nsub, limit, clean, ss.d_ring.p,
                        ss.d_cap.p, ss.head.p, ss.tail.p, ss.nsub, &fail);
    slab_heads(e, ss);
    for (int r = 0; r < ss.nsub; ++r)
      if (clean[r] && !fail[r]) ss.h_tail[r] = limit[r];
    HIPCHK(hipMemcpy(ss.tail.p, ss.h_tail.data(), ss.nsub * 8, hipMemcpyHostToDevice));
    ++ss.cleanings;
    // a ring below 2x (live + headroom) cannot clean in place for long: a fresh buffer of 2.5x that
    // takes its live blocks (slab_grow compacts as it moves; sized from the live words, not the
    // ring's span, which counts dead blocks: sizing from the span doubled the reservation every
    // other C5 step and ran out of HBM)
    const double grow_at = sdh::knob("SDH_SLAB_GROW_AT") ? atof(sdh::knob("SDH_SLAB_GROW_AT")) : 1.4;
    const double grow_to = sdh::knob("SDH_SLAB_GROW_TO") ? atof(sdh::knob("SDH_SLAB_GROW_TO")) : 1.5;
    for (int r = 0; r < ss.nsub; ++r) {
      if (!clean[r]) continue;
      const int64_t used = (int64_t)(ss.h_head[r] - ss.h_tail[r]);
      const double base = (double)((int64_t)live[r] + need[r]);
      if (!fail[r] && ss.cap[r] - used >= need[r] && (double)ss.cap[r] >= grow_at * base) continue;
      grow.push_back(r);
      gcap.push_back(std::max<int64_t>(ss.cap[r], (int64_t)(grow_to * base)));
    }
  }
  if (sdh::knob("SDH_SLAB_TRACE")) {
    fprintf(stderr, "[sdh] slab prepare: live pass + cleaning %.1f ms\n", now_ms() - t_prep);
    int64_t c = 0, u = 0, nd = 0, g = 0;
    for (int r = 0; r < ss.nsub; ++r) {
      c += ss.cap[r];
      u += (int64_t)(ss.h_head[r] - ss.h_tail[r]);
      nd += need[r];
    }
    for (int64_t x : gcap) g += x;
    fprintf(stderr, "[sdh] slab prepare: %d rings, cap %.2f GB, used %.2f GB, need %.2f GB, demand %d, grow %zu rings to %.2f GB\n",
            ss.nsub, c * 4e-9, u * 4e-9, nd * 4e-9, demand ? 1 : 0, grow.size(), g * 4e-9);
  }
  if (!grow.empty()) slab_grow(e, ss, grow, gcap);
  ss.h_push0 = ss.h_head;
}

// undo this pass's launch of the set (its directory changes; its allocations are dropped)
void slab_rollback(sdh_engine* e, sdh_engine::SlabSet& ss) {
  if (ss.items <= 0) return;
  HIPCHK(sdh_slab_rollback(ss.dir.p, ss.journal.p, ss.journal_idx.p, ss.items, ss.live_bak.p, ss.live.p, e->stream));
  HIPCHK(hipMemcpyAsync(ss.head.p, ss.head_bak.p, ss.nsub * 8, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  ss.items = 0;
  slab_heads(e, ss);
}

// the words of the set's live blocks (one pass over the directory)
int64_t slab_live_words(sdh_engine* e, const sdh_engine::SlabSet& ss) {
  DevBuf<unsigned long long> acc;
  acc.ensure(1);
  HIPCHK(hipMemsetAsync(acc.p, 0, 8, e->stream));
  HIPCHK(sdh_slab_live_words(ss.dir.p, ss.key_cap * ss.n_groups, ss.n_groups, ss.d_group_ew.p, acc.p, e->stream));
  unsigned long long w = 0;
  d2h_sync(e, &w, acc.p, 8);
  return (int64_t)w;
}

int64_t slab_live_partials(sdh_engine* e, const sdh_engine::SlabSet& ss) {
  long long v[256];
  HIPCHK(hipMemcpyAsync(v, ss.live.p, sizeof v, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  int64_t n = 0;
  for (long long x : v) n += x;
  return n;
}

// ---- snapshot section (engine_snap.hip): the live blocks packed into one ring, the directory pointing
// into it, the counters ----
namespace {
// a one-ring arena over `buf` for slab_move_raw: the device's ring pointer and capacity words
struct OneRing {
  DevBuf<uint32_t*> ring;
  DevBuf<int64_t> cap;
  OneRing(const DevBuf<uint32_t>& buf, int64_t words) {
    ring.ensure(1);
    cap.ensure(1);
    const int64_t c = std::max<int64_t>(4, words);
    HIPCHK(hipMemcpy(ring.p, &buf.p, sizeof(uint32_t*), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(cap.p, &c, 8, hipMemcpyHostToDevice));
  }
};
}  // namespace

void snap_save_slab(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->ssets.size());
  for (auto& up : e->ssets) {
    auto& ss = *up;
    const int64_t n_dir = ss.key_cap * ss.n_groups;
    DevBuf<unsigned long long> ph, pt;
    ph.ensure(1);
    pt.ensure(1);
    HIPCHK(hipMemset(ph.p, 0, 8));
    HIPCHK(hipMemset(pt.p, 0, 8));
    const int64_t words = slab_live_words(e, ss);
    DevBuf<uint64_t> dcopy;
    DevBuf<uint32_t> packed;
    dcopy.ensure(std::max<int64_t>(1, n_dir));
    packed.ensure(std::max<int64_t>(1, words));
    if (n_dir) HIPCHK(hipMemcpy(dcopy.p, ss.dir.p, n_dir * 8, hipMemcpyDeviceToDevice));
    OneRing one(packed, words);
    if (words && !slab_move_raw(e, ss, dcopy.p, ss.d_ring.p, ss.d_cap.p, ss.tail.p, ss.nsub,
                                std::vector<unsigned long long>(ss.nsub, ~0ull), {}, one.ring.p, one.cap.p, ph.p, pt.p, 1))
      throw Error(SDH_E_DEVICE, "K_slab snapshot: packing failed");
    w.put(ss.partition);
    w.put(ss.key_cap);
    w.put(ss.n_groups);
    w.put(ss.lds_words);
    w.put(words);
    put_dev(w, dcopy.p, (size_t)n_dir * 8);
    put_dev(w, packed.p, (size_t)words * 4);
    put_dev(w, ss.live.p, 256 * 8);
  }
}

void snap_load_slab(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->ssets.size(), "snapshot of a different program");
  for (auto& up : e->ssets) {
    auto& ss = *up;
    snap::need(r.get() == ss.partition, "snapshot of a different program");
    const int64_t key_cap = r.get(), ng = r.get(), lds = r.get(), words = r.get();
    snap::need(ng == ss.n_groups && key_cap >= 0 && key_cap <= ((int64_t)1 << 32) && words >= 0 && lds >= 64 && lds <= 13312,
               "bad snapshot K_slab set");
    ss.lds_words = (int)lds;
    ss.key_cap = 0;
    DevBuf<uint64_t>().swap(ss.dir);  // freed: reallocated at the snapshot's capacity
    slab_grow_keys(e, ss, key_cap);
    snap::need(ss.key_cap == key_cap, "snapshot key capacity mismatch");
    get_dev(r, ss.dir.p, (size_t)key_cap * ng * 8);
    DevBuf<uint32_t> packed;
    packed.ensure(std::max<int64_t>(1, words));
    get_dev(r, packed.p, (size_t)words * 4);
    slab_init(e, ss, std::max<int64_t>(1 << 16, 2 * (words / ss.nsub) + 65536));
    get_dev(r, ss.live.p, 256 * 8);
    DevBuf<unsigned long long> zt;
    zt.ensure(1);
    HIPCHK(hipMemset(zt.p, 0, 8));
    OneRing one(packed, words);
    if (words && !slab_move_raw(e, ss, ss.dir.p, one.ring.p, one.cap.p, zt.p, 1, std::vector<unsigned long long>(1, ~0ull), {},
                                ss.d_ring.p, ss.d_cap.p, ss.head.p, ss.tail.p, ss.nsub))
      throw Error(SDH_E_CAPACITY, "K_slab restore: a ring overflowed");
    slab_heads(e, ss);
    ss.h_push0 = ss.h_head;
  }
}

}  // namespace eng
}  // namespace sdh
