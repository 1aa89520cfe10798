// engine_snap.hip -- the snapshot blob: its prologue and the order of its sections. Each section is a
// snap_save_X / snap_load_X pair in the unit that owns the state (engine_int.h).
#include "engine_int.h"

namespace sdh {
namespace eng {

// The format (snap_io.h: int64 words; a byte payload is padded with zeros to whole words). This list
// and the pairs it names are its definition; any change to it takes a new SNAP_VERSION.
//   prologue  magic, version, n_q, pcap, gB32, gB64, R, N, LC, started, start_ts, seq, n_streams,
//             prev_ts[n_streams]
//   chain     per K_chain query: seed_alive, n_live, table[NF][pcap]
//   ratchet   n_groups; per group, per lane (64): n, then n x (ts0, seq, key)
//   gen       n_sets; per set: partition, key_cap, blocks, a32[blocks x gB32 x 64] (4 B each),
//             a64[blocks x gB64 x 64]
//   routes    n_partitions; per partition: present; if so slots, tkey[slots], tid[slots] (4 B), n_keys
//             (4 B), key_of_id[max_keys], key kind, keys seen, n_order, n_order x (key id, key)
//   part      n_sets; per set: partition, kind, cap, key_cap, both tables [2][key_cap][groups][bw][64],
//             cur[key_cap] (4 B)
//   seq       n_streams; per stream: tail length, tail[SEQ_TMAX x SEQ_TW]
//   slab      n_sets; per set: partition, key_cap, n_groups, lds_words, words, dir[key_cap x n_groups]
//             (pointing into:) the live blocks packed into one ring[words] (4 B), live[256]
//   events    versions 9 and 11 only: cap, row words, first retained seq, then the retained rows in seq order
//   wave      versions 10 and 11 only (an engine with K_wave queries): n_sets; per set: stream, queries,
//             entry words, cap, the queries' current tables [queries][WV_HDR + cap x entry words]
// An engine without K_wave queries writes versions 8 / 9, byte for byte what it wrote before the wave
// section existed; one with K_wave queries writes 10 / 11: the same layout followed by `wave`.
constexpr int64_t SNAP_MAGIC = 0x5344485350415254LL;
constexpr int64_t SNAP_VERSION = 8;
constexpr int64_t SNAP_VERSION_EVENTS = 9;  // version 8 followed by the event store (sdh_engine_retain_events)
constexpr int64_t SNAP_VERSION_WAVE = 10;   // version 8 / 9 followed by the wave section: 10 / 11

void snap_save(sdh_engine* e, snap::Writer& w) {
  w.put(SNAP_MAGIC);
  // (an engine that keeps events writes version 9; K_wave queries add the wave section: 10 / 11)
  w.put((e->ev_cap ? SNAP_VERSION_EVENTS : SNAP_VERSION) + (e->wsets.empty() ? 0 : SNAP_VERSION_WAVE - SNAP_VERSION));
  w.put((int64_t)e->lq.size());
  w.put(e->pcap);
  w.put(e->gB32);
  w.put(e->gB64);
  w.put(e->gsz.R);
  w.put(e->gsz.N);
  w.put(e->gsz.LC);
  w.put(e->started ? 1 : 0);
  w.put(e->start_ts);
  w.put(e->seq);
  w.put((int64_t)e->prev_ts.size());
  w.put(e->prev_ts.begin(), e->prev_ts.end());
  snap_save_chain(e, w);
  snap_save_ratchet(e, w);
  snap_save_gen(e, w);
  snap_save_routes(e, w);
  snap_save_part(e, w);
  snap_save_seq(e, w);
  snap_save_slab(e, w);
  if (e->ev_cap) snap_save_events(e, w);
  if (!e->wsets.empty()) snap_save_wave(e, w);
}

// Nothing changes before every check that needs no change has passed: a blob refused by then leaves the
// engine as it was. A failure after that leaves it half loaded, so it is marked broken (check_usable)
// until a restore succeeds; the sections free and regrow what they replace, so one can.
void snap_load(sdh_engine* e, snap::Reader r) {
  using snap::need;
  need(r.get() == SNAP_MAGIC, "bad snapshot magic");
  const int64_t version = r.get();
  // this engine's versions: with K_wave queries 10 / 11, without 8 / 9 (a blob of the other pair is
  // of another program's plans: refused here, before anything changes)
  const int64_t vbase = e->wsets.empty() ? SNAP_VERSION : SNAP_VERSION_WAVE;
  need(version == vbase || version == vbase + 1, "snapshot of another format version");
  const bool stored = version == vbase + 1;
  const size_t nq = (size_t)r.get();
  const int64_t spcap = r.get();  // the snapshot's K_chain table capacity
  need(nq == e->lq.size() && spcap >= 64 && spcap % 64 == 0 && spcap <= (1 << 24), "snapshot of a different program");
  if (spcap != e->pcap && !e->chain_growing)
    throw Error(SDH_E_INVALID, fmt("snapshot of K_chain tables of %lld partials per query: this engine's are fixed at "
                                   "%d (partials_per_inst)", (long long)spcap, e->pcap));
  const int64_t b32 = r.get(), b64 = r.get();
  const kg::Sizing sz{(int)r.get(), (int)r.get(), (int)r.get()};
  need(sz.R >= 1 && sz.R <= kg::GMAXPOOL && sz.N >= 1 && sz.N <= kg::GMAXPOOL && sz.LC >= 1 && sz.LC <= (1 << 16),
       "bad snapshot K_gen pool sizing");
  const int64_t started = r.get(), start_ts = r.get(), seq = r.get();
  const size_t ns = (size_t)r.get();
  need(ns == e->prev_ts.size(), "snapshot of a different program");
  const int64_t* prev_ts = r.words(ns);
  try {
    // the snapshot's pools may have grown past this engine's: take its sizing (snap_load_gen loads the arenas)
    if (sz.R != e->gsz.R || sz.N != e->gsz.N || sz.LC != e->gsz.LC) gen_relayout(e, sz, false);
    need(b32 == e->gB32 && b64 == e->gB64, "snapshot of a different K_gen arena layout (another build or pool sizing)");
    e->started = started != 0;  // the runtime's start time (absent states' schedules)
    e->start_ts = start_ts;
    e->seq = seq;
    std::copy(prev_ts, prev_ts + ns, e->prev_ts.begin());
    snap_load_chain(e, r, spcap);
    snap_load_ratchet(e, r);
    snap_load_gen(e, r);
    snap_load_routes(e, r);
    snap_load_part(e, r);
    snap_load_seq(e, r);
    snap_load_slab(e, r);
    snap_load_events(e, r, stored);
    if (!e->wsets.empty()) snap_load_wave(e, r);
  } catch (...) {
    e->broken = "a failed restore";
    throw;
  }
}

}  // namespace eng
}  // namespace sdh
