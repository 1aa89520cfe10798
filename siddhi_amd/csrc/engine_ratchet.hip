// engine_ratchet.hip -- launch paths of K_chain and of K_ratchet with its K_gate and shared-pops forms.
#include "engine_int.h"
#include "launchers.h"

namespace sdh {
namespace eng {

namespace {
int32_t launch_once(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2],
                    const std::vector<int>& qs, bool allow_chunks, bool* unordered);

// K_chain tables with room for `want` partials per query: both buffers re-laid on the device
// ([q][field][pcap]: the field rows move, the new lanes are free). Up to 512 partials the sizes are
// 64, 128, 256 and 512 (the K register sets of nfa_chain_kernel, which one-state queries keep using
// beside the paged form, cover exactly 64 * K lanes); beyond that any multiple of 64 (the paged form)
void chain_grow(sdh_engine* e, int64_t want) {
  int64_t cap = e->pcap;
  if (want <= 512) {
    while (cap < want) cap *= 2;
  } else {
    cap = std::max<int64_t>(cap, (want + 63) / 64 * 64);
  }
  if (cap <= e->pcap) return;
  if (cap > (1 << 24)) throw Error(SDH_E_CAPACITY, "more than 2^24 pending partials in one chain pattern");
  const int64_t rows = (int64_t)std::max<size_t>(e->lq.size(), 1) * NF;
  DevBuf<int64_t> nw[2];
  for (int b = 0; b < 2; ++b) {
    if (hipMalloc(&nw[b].p, (size_t)rows * cap * 8) != hipSuccess) {
      (void)hipGetLastError();
      nw[b].p = nullptr;
      throw Error(SDH_E_CAPACITY, fmt("device memory exhausted growing the K_chain tables to %lld partials per query",
                                      (long long)cap));
    }
    nw[b].n = (size_t)rows * cap;
    HIPCHK(sdh_chain_relayout(e->d_part[b].p, nw[b].p, rows, e->pcap, (int)cap, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int b = 0; b < 2; ++b) {
    e->d_part[b].swap(nw[b]);
  }
  e->pcap = (int)cap;
  e->K = cap <= 64 ? 1 : cap <= 128 ? 2 : cap <= 256 ? 4 : 8;
  e->chain_paged = e->chain_force_paged || cap > chain_reg_limit(e);
  ++e->chain_regrows;
}
}  // namespace

// One K_chain step of the queries `qs` over batch B. A table overflow of a growing engine
// (partials_per_inst == 0) is re-run here at a larger table: the kernels read part[cur] and write
// part[1 - cur], and cur flips only after this returns (do_push), so the input tables are intact when
// err[0] comes back and the re-run is exact by construction. Every attempt plans its items, segments
// and counts afresh, so a failed one leaves nothing behind.
void launch(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2],
            const std::vector<int>& qs, bool allow_chunks, bool* unordered) {
  double ms_failed = 0;
  for (;;) {
    const int32_t need = launch_once(e, stream, B, t01, qs, allow_chunks, unordered);
    e->stats.last_kernel_ms += ms_failed;
    if (need < 0) return;
    ms_failed = e->stats.last_kernel_ms;
    // the register forms can only double; the paged form counted what it could not store, so one
    // re-run fits (with an eighth of headroom, and at most 8x: a long push counts partials as lost
    // that would have expired had they been stored)
    // (an interleaved push runs the paged form at every table size)
    int64_t want = 2 * (int64_t)e->pcap;
    if (e->chain_paged || e->mix)
      want = std::min<int64_t>(8 * (int64_t)e->pcap, std::max<int64_t>(want, (int64_t)need + need / 8));
    if (sdh::knob("SDH_TRACE"))
      fprintf(stderr, "[sdh] chain tables %d -> %lld partials per query (needed %d)\n", e->pcap, (long long)want, need);
    chain_grow(e, want);
  }
}

namespace {
// one attempt; returns -1, or after a table overflow of a growing engine the partials per query the
// paged form asked for (the register forms: 0)
int32_t launch_once(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2],
                    const std::vector<int>& qs, bool allow_chunks, bool* unordered) {
  const int64_t n = B.n;
  // chunk planning: enough waves to fill 256 CUs, chunks >> the warm-up window
  double ev_per_ms = 1.0;
  if (n > 1) ev_per_ms = (double)n / (double)std::max<int64_t>(1, t01[1] - t01[0]);
  const int64_t min_chunk = e->cfg.chunk_events > 0 ? e->cfg.chunk_events : 4096;
  const double target_waves = 16384.0;
  // every wave replays (warm-up) + emits about the same number of events, so the launch has no
  // serial tail: wave length T >= 2x the largest warm-up and ~ total work / target_waves
  double max_warm = 0;
  for (int li : qs) {
    const ChainQuery& c = e->lq[li].cq;
    if (c.chunkable) max_warm = std::max(max_warm, (double)c.within * ev_per_ms + 64.0);
  }
  const double T = std::max({2.0 * max_warm, (double)n * qs.size() / target_waves, 2.0 * min_chunk});
  e->work.clear();
  int64_t seg = 0, scr = 0;
  // queries grouped by state count (one kernel instantiation per group)
  std::vector<int> order(qs);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return e->lq[a].cq.n_states < e->lq[b].cq.n_states; });
  // the paged form runs the queries that hold partials (two states or more). Each chunk but a query's
  // last works in a scratch table of pcap entries; together they take at most 1 GiB,
  // which bounds the chunks per paged query
  // (an interleaved push, e->mix: the MIX = true paged kernels for every query, one-state ones too)
  auto paged = [&](int li) { return e->mix || (e->chain_paged && e->lq[li].cq.n_states >= 2); };
  int64_t n_paged = 0;
  for (int li : order) n_paged += paged(li) ? 1 : 0;
  const int64_t tbl_bytes = (int64_t)NF * e->pcap * 8;
  const int64_t paged_chunks = 1 + ((int64_t)1 << 30) / (tbl_bytes * std::max<int64_t>(1, n_paged));
  for (int li : order) {
    const ChainQuery& c = e->lq[li].cq;
    int64_t C = 1;
    if (allow_chunks && c.chunkable) {
      const double warm = (double)c.within * ev_per_ms + 64.0;
      const double emit_len = std::max((double)min_chunk, T - warm);
      C = std::max<int64_t>(1, (int64_t)std::ceil((double)n / emit_len));
      if (paged(li)) C = std::min(C, paged_chunks);
    }
    for (int64_t ch = 0; ch < C; ++ch) {
      WorkItem w{};
      w.q = li;
      w.chunk = (int)ch;
      w.n_chunks = (int)C;
      w.inb = e->cur[li];
      w.c0 = n * ch / C;
      w.c1 = n * (ch + 1) / C;
      w.seg_off = seg;
      w.seg_cap = (w.c1 - w.c0) + e->pcap + 1;
      seg += w.seg_cap;
      w.scr = paged(li) && ch + 1 < C ? scr++ : -1;
      e->work.push_back(w);
    }
  }
  const int n_items = (int)e->work.size();
  if (scr > 0) e->d_pscratch.ensure((size_t)scr * NF * e->pcap);
  e->d_work.ensure(n_items);
  e->d_seg_count.ensure(n_items);
  e->d_match.ensure((size_t)seg * e->rec_words);
  e->d_err.ensure(4);
  HIPCHK(hipMemcpyAsync(e->d_work.p, e->work.data(), n_items * sizeof(WorkItem), hipMemcpyHostToDevice,
                        e->stream));
  HIPCHK(hipMemsetAsync(e->d_err.p, 0, 16, e->stream));
  ChainLaunch L{};
  L.queries = e->d_q.p;
  L.work = e->d_work.p;
  L.n_work = n_items;
  L.pcap = e->pcap;
  L.b = B;
  for (int b = 0; b < 2; ++b) {
    L.hdr[b] = e->d_hdr[b].p;
    L.part[b] = e->d_part[b].p;
  }
  L.match = e->d_match.p;
  L.rec_words = e->rec_words;
  L.seg_count = e->d_seg_count.p;
  L.err = e->d_err.p;
  L.scratch = e->d_pscratch.p;
  L.rcode = e->d_rcode.p;
  L.mix = e->mix;
  const size_t lds = 0;
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  for (int i0 = 0; i0 < n_items;) {
    const int S = e->lq[e->work[i0].q].cq.n_states;
    int i1 = i0;
    while (i1 < n_items && e->lq[e->work[i1].q].cq.n_states == S) ++i1;
    ChainLaunch Ls = L;
    Ls.work = e->d_work.p + i0;
    Ls.seg_count = e->d_seg_count.p + i0;
    Ls.n_work = i1 - i0;
    if (e->mix) HIPCHK(sdh_launch_chain_mixed(S, e->chain_resid, &Ls, (Ls.n_work + 3) / 4, e->stream));
    else if (paged(e->work[i0].q)) HIPCHK(sdh_launch_chain_paged(S, e->chain_resid, &Ls, (Ls.n_work + 3) / 4, e->stream));
    else HIPCHK(sdh_launch_chain(S, e->K, e->chain_resid, &Ls, (Ls.n_work + 3) / 4, lds, e->stream));
    i0 = i1;
  }
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  int32_t errs[4];
  e->seg_count.resize(n_items);
  HIPCHK(hipMemcpyAsync(errs, e->d_err.p, 16, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(e->seg_count.data(), e->d_seg_count.p, n_items * 8, hipMemcpyDeviceToHost,
                        e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  e->stats.last_kernel_ms = ms;
  if (errs[0]) {
    if (!e->chain_growing)
      throw Error(SDH_E_CAPACITY, "partial-match table overflow: raise partials_per_inst (0: tables grow)");
    return std::max(0, errs[3]);
  }
  if (errs[2]) throw Error(SDH_E_CAPACITY, "match segment overflow");
  *unordered = errs[1] != 0;
  // algorithmic bytes of this launch: every item streams its [w0, c1) events once
  // (approximated by c1-c0 plus warm-up), reads and writes its partial table, writes its matches
  int64_t ev_bytes = 8;
  for (int a = 0; a < B.n_attr; ++a) ev_bytes += B.width[a];
  double bytes = 0;
  int64_t total_matches = 0;
  for (int i = 0; i < n_items; ++i) {
    const WorkItem& w = e->work[i];
    const ChainQuery& c = e->lq[w.q].cq;
    double warm = w.chunk > 0 ? std::min<double>((double)w.c0, (double)c.within * ev_per_ms) : 0.0;
    bytes += ((double)(w.c1 - w.c0) + warm) * ev_bytes;
    total_matches += e->seg_count[i];
  }
  bytes += (double)qs.size() * 2.0 * NF * e->pcap * 8;  // partial tables in + out
  bytes += (double)total_matches * e->rec_words * 8;
  e->stats.last_kernel_bytes = bytes;
  e->device_matches = total_matches;
  return -1;
}
}  // namespace

// ------------------------------------------------------------------------------------------
// K_ratchet host side
// ------------------------------------------------------------------------------------------
namespace {
int ratchet_sim(const sdh::RatchetGroup& g);
}  // namespace

void ratchet_build(sdh_engine* e, std::vector<std::pair<RatchetPlan, int>>& plans) {
  // lanes: normal mode in receiver-rank order (a wave's lanes are then consecutive ranks, which the
  // direct placement needs: place_cells); SDH_FLAG_DEVICE_MATCHES mode by `within`, so that similar
  // warm-up windows share a wave (SDH_RATCHET_LANES=rank|within overrides)
  const char* lo = sdh::knob("SDH_RATCHET_LANES");
  const bool by_rank = lo ? strcmp(lo, "rank") == 0 : !(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES);
  const size_t ns = e->prog.stream_types.size();
  auto rank = [&](const std::pair<RatchetPlan, int>& p) { return e->out_rank[(size_t)p.second * ns + p.first.stream]; };
  std::stable_sort(plans.begin(), plans.end(), [&](const auto& a, const auto& b) {
    const auto sa = a.first.sig(), sb = b.first.sig();
    if (sa != sb) return sa < sb;
    if (by_rank) return rank(a) < rank(b);
    return a.first.within < b.first.within;
  });
  for (size_t i = 0; i < plans.size();) {
    size_t j = i;
    const auto sg = plans[i].first.sig();
    while (j < plans.size() && j - i < 64 && plans[j].first.sig() == sg) ++j;
    RatchetGroup g{};
    const RatchetPlan& P = plans[i].first;
    g.n_lanes = (int)(j - i);
    g.stream = P.stream;
    g.key_attr = P.key_attr;
    g.key_conv = P.key_conv;
    g.key_kind = P.key_kind;
    g.xmask = P.xmask;
    g.n_f0 = (int)P.f0.size();
    for (int a = 0; a < g.n_f0; ++a) g.f0[a] = P.f0[a];
    g.n_g = (int)P.g.size();
    for (int a = 0; a < g.n_g; ++a) g.g[a] = P.g[a];
    g.sim = g.n_g ? 0 : ratchet_sim(g);
    g.wmax = -1;
    for (int l = 0; l < 64; ++l) {
      const size_t k = i + std::min<size_t>(l, j - i - 1);  // idle lanes mirror the last pattern
      const RatchetPlan& Q = plans[k].first;
      g.qid[l] = plans[k].second;
      g.within[l] = Q.within < 0 ? INT64_MAX : Q.within;
      if (l < g.n_lanes) g.wmax = std::max(g.wmax, Q.within);
      for (int a = 0; a < g.n_f0; ++a) g.f0c[a][l] = Q.f0c[a];
      for (int a = 0; a < g.n_g; ++a) g.gc[a][l] = Q.gc[a];
    }
    e->rg.push_back(g);
    i = j;
  }
  // per-tile x summaries: one row per distinct (stream, key column, conversion, key kind)
  e->r_sum_specs.clear();
  for (auto& g : e->rg) {
    const std::array<int, 4> spec{g.stream, g.key_attr, g.key_conv, g.key_kind};
    int slot = -1;
    for (size_t k = 0; k < e->r_sum_specs.size(); ++k)
      if (e->r_sum_specs[k] == spec) slot = (int)k;
    if (slot < 0) {
      slot = (int)e->r_sum_specs.size();
      e->r_sum_specs.push_back(spec);
    }
    g.sum_slot = slot;
  }
  const size_t ng = e->rg.size();
  e->rcur.assign(ng, 0);
  e->r_full_expiry.assign(e->prog.stream_types.size(), 0);
  if (!ng) return;
  e->d_rg.ensure(ng);
  HIPCHK(hipMemcpy(e->d_rg.p, e->rg.data(), ng * sizeof(RatchetGroup), hipMemcpyHostToDevice));
  for (int b = 0; b < 2; ++b) {
    e->d_rst[b].ensure(ng);
    HIPCHK(hipMemset(e->d_rst[b].p, 0, ng * sizeof(RatchetState)));
    e->d_rts[b].ensure(ng * e->rsmax * WAVE);
    e->d_rsq[b].ensure(ng * e->rsmax * WAVE);
    e->d_rky[b].ensure(ng * e->rsmax * WAVE);
  }
  e->d_blk_next.ensure(4);
}

namespace {
// persisted deques with room for `want` entries per lane: [g][rsmax][64] re-strided (both buffers)
void ratchet_grow_rsmax(sdh_engine* e, int64_t want) {
  if (want <= e->rsmax) return;
  int64_t cap = e->rsmax;
  while (cap < want) cap *= 2;
  const size_t ng = e->rg.size(), ob = (size_t)e->rsmax * WAVE * 8, nb = (size_t)cap * WAVE * 8;
  for (int b = 0; b < 2; ++b)
    for (DevBuf<int64_t>* buf : {&e->d_rts[b], &e->d_rsq[b], &e->d_rky[b]}) {
      DevBuf<int64_t> nw;
      nw.ensure(ng * cap * WAVE);
      HIPCHK(hipMemcpy2DAsync(nw.p, nb, buf->p, ob, ob, ng, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      buf->swap(nw);
    }
  e->rsmax = cap;
}

int64_t ratchet_count_matches(sdh_engine* e) {
  int64_t n = 0;
  for (int i = 0; i < e->r_blocks_used; ++i) n += e->r_blk_count[i];
  return n;
}

// one NFA step of every ratchet group fed by `stream` over batch B (exact re-runs on overflow /
// out-of-order timestamps: the groups' input deques are double-buffered and untouched until the
// launch succeeds)
// f0 atoms a K_ratchet launch variant must handle: the one-atom variant assumes a constant
// interval, so a group with a two-column atom (`cur.a OP cur.b`) takes the general variant
int ratchet_nf(const sdh::RatchetGroup& g) {
  for (int a = 0; a < g.n_f0; ++a)
    if (g.f0[a].cur2) return sdh::RMAXF0;
  return g.n_f0;
}

// the SIM form (nfa_ratchet.hip): float keys from a float column, one start atom over that same
// column compared in the float / double domain against a constant, without negation
int ratchet_sim(const sdh::RatchetGroup& g) {
  if (sdh::knob("SDH_RATCHET_NO_SIM")) return 0;
  if (g.key_kind != sdh::KK_F32 || g.key_conv == sdh::CV_F32_INT || g.key_conv == sdh::CV_F32_LONG || g.n_f0 != 1)
    return 0;
  const sdh::RatchetAtom& A = g.f0[0];
  return (A.attr == g.key_attr && !A.cur2 && A.f64 && (A.conv == sdh::CV_F32_FLOAT || A.conv == sdh::CV_F64_FLOAT) &&
          !(A.mask & sdh::CM_NOT)) ? 1 : 0;
}


// A normal-mode push places its K_ratchet matches directly (nfa_ratchet.hip PM: COUNT per (event,
// group) cell, scan, WRITE as compact rows after the window's rows) when they are its only matches
// -- the chain and K_gen launches ran first and produced none, and the window holds no table rows
// --, the stream's groups are rank-ordered (place_cells), the cells stay within 2^30, the seqs of
// the window within 2^31 of seq_ref, and the launch runs without the full-expiry scan.
bool ratchet_placeable(const sdh_engine* e, int stream, int64_t seq_base, int64_t n_events, bool full) {
  const int nc = e->place_cells[(size_t)stream];
  return nc > 0 && !(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) && !full && n_events > 0 && !e->ck.active &&
         e->device_matches == 0 && e->g_dev_matches == 0 && (e->mt.n == 0 || e->mt.placed) &&
         (double)n_events * nc < (double)(1 << 30) && seq_base + n_events - e->seq_ref < INT32_MAX &&
         !sdh::knob("SDH_NO_PLACE");
}
}  // namespace

void launch_ratchet(sdh_engine* e, int stream, const StreamBatch& B, const int64_t t01[2]) {
  e->r_placing = false;
  e->r_blocks_used = 0;
  e->r_matches = 0;
  e->r_kernel_ms = 0;
  e->r_kernel_bytes = 0;
  e->r_rec_bytes = 0;
  e->r_rec4 = 0;
  ++e->r_launches;
  std::vector<int> gs;
  for (int g = 0; g < (int)e->rg.size(); ++g)
    if (e->rg[g].stream == stream) gs.push_back(g);
  if (gs.empty()) return;
  const int64_t n = B.n;
  int64_t lanes = 0;
  for (int g : gs) lanes += e->rg[g].n_lanes;
  const bool devrec = (e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) != 0;
  if (e->r_blocks == 0) {
    // a first guess (at most 8 GiB of blocks): a push that needs more re-runs once with the count of
    // blocks its waves asked for
    int64_t want = e->cfg.match_capacity > 0 ? e->cfg.match_capacity : std::max<int64_t>(1 << 20, n * lanes * 3 / 4);
    if (e->cfg.match_capacity <= 0) want = std::min<int64_t>(want, (int64_t)1 << 30);
    e->r_blocks = (want + e->r_blk_recs - 1) / e->r_blk_recs;
  }
  e->d_rtotal.ensure(3);  // [0] device-record entries, [1] the placement total, [2] device-record bytes
  // (the kernels roll to a fresh block when 64 entries and a side entry do not fit the open one)
  if (e->r_blk_recs * 8 < 4 * WAVE + 8) throw Error(SDH_E_INVALID, "K_ratchet blocks smaller than one wave of records");
  bool no_place = false, no_rec4 = false;
  for (int attempt = 0; attempt < 40; ++attempt) {
    // out-of-order timestamps seen on this stream, timestamps so extreme that `ts0 + within`
    // could wrap, or a batch spanning 2^31 - 2 ms or more (the lazy forms' 32-bit deadline domain,
    // nfa_ratchet.hip rel_deadline): exact per-entry expiry scan, no chunking
    const int64_t lim = (int64_t)1 << 61;
    const bool full = e->r_full_expiry[stream] != 0 || t01[0] < -lim || t01[0] > lim || t01[1] < -lim ||
                      t01[1] > lim || (B.prev_ts != INT64_MIN && (B.prev_ts < -lim || B.prev_ts > lim)) ||
                      t01[1] - t01[0] > (int64_t)INT32_MAX - 2;
    // ---- chunk planning: chunk c > 0 rebuilds its starting deques by a reverse scan of the
    // `within` window (a few instructions per 64 events), so chunks can be short. Each launch
    // (one key kind x orientation) gets one resident wave per slot of the chip -- CUs x the
    // kernel's occupancy -- of at least min_chunk emitted events each ----
    // (C2 expansion, 64K-event pushes, tools/sweep_minchunk.sh: 2,048 events per chunk at least
    // 3.66 ms per push / 3.56 compact, 1,024 3.42 / 3.43, 512 3.43 / 3.48, 256 3.68 / 3.68)
    const int64_t def_chunk = sdh::knob("SDH_RATCHET_MIN_CHUNK") ? atoll(sdh::knob("SDH_RATCHET_MIN_CHUNK")) : 1024;
    const int64_t min_chunk = e->cfg.chunk_events > 0 ? e->cfg.chunk_events : def_chunk;
    e->ritems.clear();
    std::vector<int> order(gs);
    // launches: one per (key kind, orientation, SIM form); SIM also needs the key column null-free
    // in this batch
    auto lsim = [&](int g) { return e->rg[g].sim && !B.nul[e->rg[g].key_attr] ? 1 : 0; };
    auto lgate = [&](int g) { return e->rg[g].n_g > 0 ? 1 : 0; };  // K_gate groups (nfa_gate.hip)
    // the shared-pops form (nfa_ratchet_shared.hip): SIM launches writing rec4 device
    // records of a push large enough to repay the pre-pass. SDH_RATCHET_SHARED_MIN, C2 at 10K patterns
    // in device-record mode, ms per push with the form on / off: 4,096 events 0.51 /
    // 0.52, 16,384 0.67 / 0.60, 65,536 1.21 / 1.21, 262,144 2.68 / 3.38, 8M 61.7 / 85.7 -- the default
    // lies between the tie and the first clear gain. SDH_RATCHET_NO_SHARED switches the form off;
    // SDH_RATCHET_SHARED_ALT=k (tests) keeps it to every other K_ratchet step, the odd ones for k = 1
    const bool rec4_ok = devrec && n <= ((int64_t)1 << 26) && !full && !no_rec4;
    bool use_shared = rec4_ok && !sdh::knob("SDH_RATCHET_NO_SHARED");
    if (use_shared) {
      const char* mn = sdh::knob("SDH_RATCHET_SHARED_MIN");
      use_shared = n >= std::max<int64_t>(1, mn ? atoll(mn) : 131072);
      if (const char* alt = sdh::knob("SDH_RATCHET_SHARED_ALT")) use_shared = use_shared && (e->r_launches & 1) == (atoi(alt) & 1);
    }
    auto lshared = [&](int g) {
      return use_shared && lsim(g) && !lgate(g) && B.width[e->rg[g].key_attr] == 4;
    };
    // (a shared-pops launch has one pre-pass, so it also holds one key column: eligibility is per group,
    // and the shared groups' launches are cut by column and conversion as well)
    auto lkey = [&](int g) {
      const bool sh = lshared(g);
      return std::make_tuple(lgate(g), e->rg[g].key_kind, e->rg[g].xmask, lsim(g), sh ? 1 : 0,
                             sh ? e->rg[g].key_attr : -1, sh ? e->rg[g].key_conv : -1);
    };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lkey(a) < lkey(b); });
    for (size_t i0 = 0; i0 < order.size();) {
      size_t i1 = i0;
      int nf = 0;
      while (i1 < order.size() && lkey(order[i1]) == lkey(order[i0])) nf = std::max(nf, ratchet_nf(e->rg[order[i1++]]));
      // items per launch: 8 rounds of the chip's resident slots (CUs x occupancy). Short chunks
      // balance the groups' uneven match density, and a chunk's reverse-scan warm-up is cheap (tile
      // summaries). C2 at 10K patterns, tools/sweep_ratchet.sh (SDH_RATCHET_WAVES): 8,192 items
      // 117.8 ms/step, 16,384 110.9, 32,768 103.3, 65,536 100.2, 131,072 100.8, 524,288 104.4
      double slots = e->r_waves;
      if (slots <= 0) {
        const int occ = lshared(order[i0]) ? sdh_ratchet_shared_occupancy()
                        : lgate(order[i0]) ? sdh_gate_occupancy(nf, nf)
                                         : sdh_ratchet_occupancy(e->rg[order[i0]].key_kind, full, nf, e->rML, lsim(order[i0]));
        // (the shared-pops form, whose items have no warm-up to repeat: 16 rounds. SDH_RATCHET_WAVES at
        // C2's 8M-event step: 16,384 items 70.3 ms, 32,768 64.3, 8 rounds 61.7, 131,072 60.3, 262,144 61.2)
        slots = (lshared(order[i0]) ? 16.0 : 8.0) * (double)e->n_cu * std::max(1, occ);
      }
      // chunks per chunkable group: as many as fit the item target (floor, not ceil: a partial
      // extra round of items runs as a nearly idle tail -- C2 at 10K once had 8,321 items for 8,192
      // slots, 128.7 ms/step, against 117.7 at 8,164), at least min_chunk events each. Groups
      // without `within` cannot chunk (no reverse-scan window) and hold one item each.
      int64_t n_chunkable = 0;
      // (the shared-pops form's items need no warm-up: every group chunks, `within` or not)
      const bool shared = lshared(order[i0]);
      for (size_t i = i0; i < i1; ++i) n_chunkable += (shared || (!full && e->rg[order[i]].wmax >= 0)) ? 1 : 0;
      const int64_t free_slots = std::max<int64_t>(1, (int64_t)slots - ((int64_t)(i1 - i0) - n_chunkable));
      const int64_t c_fit = n_chunkable > 0 ? std::max<int64_t>(1, free_slots / n_chunkable) : 1;
      const int64_t c_min = std::max<int64_t>(1, n / std::max<int64_t>(1, min_chunk));
      for (size_t i = i0; i < i1; ++i) {
        const int g = order[i];
        const RatchetGroup& G = e->rg[g];
        int64_t C = 1;
        if (shared) {
          C = std::min(c_fit, c_min);
        } else if (!full && G.wmax >= 0) {
          C = std::min(c_fit, c_min);
          // a chunk's warm-up walks its `within` window back from its first event: tiles whose best
          // key is dominated by the later ones are skipped on their summary, but flat or rising key
          // runs are walked event by event. Chunks x window events <= max(16 x the batch, 2^24)
          // bounds that worst case (a 67M-event window spanning the batch: 16 chunks) and binds
          // nowhere near C2's windows (1-60 s, up to 60K events, in 8M- or 64K-event pushes)
          const double span = (double)std::max<int64_t>(1, t01[1] - t01[0]);
          const double win_ev = std::min((double)n, (double)G.wmax * (double)n / span);
          const double budget = std::max(16.0 * (double)n, 16777216.0);
          C = std::min<int64_t>(C, std::max<int64_t>(1, (int64_t)(budget / std::max(1.0, win_ev))));
        }
        for (int64_t ch = 0; ch < C; ++ch) {
          RatchetItem it{};
          it.g = g;
          it.chunk = (int)ch;
          it.n_chunks = (int)C;
          it.inb = e->rcur[g];
          it.c0 = n * ch / C;
          it.c1 = n * (ch + 1) / C;
          e->ritems.push_back(it);
        }
      }
      i0 = i1;
    }
    const int n_items = (int)e->ritems.size();
    e->d_ritems.ensure(n_items);
    HIPCHK(hipMemcpyAsync(e->d_ritems.p, e->ritems.data(), n_items * sizeof(RatchetItem),
                          hipMemcpyHostToDevice, e->stream));
    // 8-B records address e2 by a 26-bit batch offset; larger batches use 16-B records. A placing
    // launch writes no records: COUNT, scan, WRITE (compact rows)
    const bool placing = !no_place && ratchet_placeable(e, stream, B.seq_base, n, full);
    const int wide = n > ((int64_t)1 << 26) ? 1 : 0;
    if (n > ((int64_t)1 << 32)) throw Error(SDH_E_INVALID, "batch larger than 2^32 events");
    e->d_rmatch.ensure((size_t)(e->r_blocks + 1) * e->r_blk_recs * (wide ? 2 : 1));  // (+ the spare block)
    e->d_rspillA.ensure((size_t)n_items * e->rSC * WAVE);
    e->d_rlts.ensure((size_t)n_items * e->rML * WAVE);
    bool any64 = false;
    for (int g : gs) any64 |= e->rg[g].key_kind == KK_F64 || e->rg[g].key_kind == KK_I64;
    if (any64) e->d_rspillB.ensure((size_t)n_items * e->rSC * WAVE);
    e->d_blk_count.ensure((size_t)e->r_blocks);
    e->d_blk_group.ensure((size_t)e->r_blocks);
    e->d_blk_side.ensure((size_t)e->r_blocks);
    e->d_err.ensure(5);
    HIPCHK(hipMemsetAsync(e->d_err.p, 0, 20, e->stream));
    HIPCHK(hipMemsetAsync(e->d_blk_next.p, 0, 4, e->stream));
    HIPCHK(hipMemsetAsync(e->d_rtotal.p, 0, 24, e->stream));
    // per-tile x summaries for the warm-up scans (rows of this stream's key specs)
    const int64_t n_tiles = (n + 63) / 64;
    const size_t n_rows = e->r_sum_specs.size();
    e->d_tsmax.ensure(n_rows * n_tiles);
    e->d_tsmin.ensure(n_rows * n_tiles);
    e->d_tshas.ensure(n_rows * n_tiles);
    if (!full)
      for (size_t r = 0; r < n_rows; ++r) {
        const auto& sp = e->r_sum_specs[r];
        if (sp[0] != stream) continue;
        // (the shared-pops form has its own tree: a row only its groups read is not built)
        bool read = false;
        for (int g : gs) read = read || (e->rg[g].sum_slot == (int)r && !lshared(g));
        if (!read) continue;
        HIPCHK(sdh_launch_ratchet_summary(sp[3], &B, sp[1], sp[2], n_tiles, e->d_tsmax.p + r * n_tiles,
                                          e->d_tsmin.p + r * n_tiles, e->d_tshas.p + r * n_tiles, e->stream));
      }
    RatchetLaunch L{};
    L.groups = e->d_rg.p;
    L.full_expiry = full;
    L.tsum_max = e->d_tsmax.p;
    L.tsum_min = e->d_tsmin.p;
    L.tsum_has = e->d_tshas.p;
    L.n_tiles = n_tiles;
    L.b = B;
    L.rsmax = e->rsmax;
    for (int b = 0; b < 2; ++b) {
      L.st[b] = e->d_rst[b].p;
      L.ent_ts[b] = e->d_rts[b].p;
      L.ent_seq[b] = e->d_rsq[b].p;
      L.ent_key[b] = e->d_rky[b].p;
    }
    L.spillA = e->d_rspillA.p;
    L.spillB = e->d_rspillB.p;
    L.match = e->d_rmatch.p;
    L.blk_count = e->d_blk_count.p;
    L.blk_side = e->d_blk_side.p;
    // device records take the 4-B rec4 entries where they can
    L.rec4 = (devrec && !wide && !full && !no_rec4) ? 1 : 0;
    L.blk_group = e->d_blk_group.p;
    L.wide = wide;
    L.blk_next = e->d_blk_next.p;
    L.n_blocks = (int32_t)std::min<int64_t>(e->r_blocks, INT32_MAX);
    L.blk_recs = e->r_blk_recs;
    L.dev_records = devrec ? 1 : 0;
    L.rec_total = e->d_rtotal.p;
    L.err = e->d_err.p;
    const int nc = e->place_cells[(size_t)stream];
    const int64_t cells = n * nc + 1;  // (+1: the scan's total)
    if (placing) {
      e->p_cnt.ensure((size_t)cells);
      HIPCHK(hipMemsetAsync(e->p_cnt.p + cells - 1, 0, 4, e->stream));
      L.pcnt = e->p_cnt.p;
      L.n_cells = nc;
    }
    e->r_placing = false;
    int any_rec4 = 0, any_shared = 0;
    // the shared-pops form's buffers for the launch of group g0
    auto shared_setup = [&](int g0) {
      SharedLaunch S{};
      const RatchetGroup& G = e->rg[g0];
      S.x = (const float*)B.col[G.key_attr];
      S.n = n;
      S.xm = G.xmask == sdh::CM_GT ? 0 : G.xmask == (sdh::CM_GT | sdh::CM_EQ) ? 1 : G.xmask == sdh::CM_LT ? 2 : 3;
      int64_t tot = 0;
      for (int64_t cur = n; cur > 64 && S.n_lvl < sdh::SH_LEVELS;) {
        cur = (cur + 63) / 64;
        S.lvl_n[S.n_lvl++] = cur;
        tot += cur;
      }
      e->d_shtree.ensure((size_t)tot + 1);
      tot = 0;
      for (int k = 0; k < S.n_lvl; ++k) {
        S.lvl[k] = e->d_shtree.p + tot;
        tot += S.lvl_n[k];
      }
      e->d_shkv.ensure((size_t)n * 4);
      S.nkey = e->d_shkv.p;
      S.nval = e->d_shkv.p + n;
      S.skey = e->d_shkv.p + 2 * n;
      S.sval = e->d_shkv.p + 3 * n;
      e->d_shpairs.ensure((size_t)n);
      S.pairs = e->d_shpairs.p;
      e->d_shcnt.ensure(2);
      S.cnt = e->d_shcnt.p;
      const size_t ng = e->rg.size();
      e->d_shcm.ensure(ng * (size_t)e->rsmax * WAVE);
      e->d_shcmn.ensure(2 * ng * WAVE);
      S.cm = e->d_shcm.p;
      S.cm_n = e->d_shcmn.p;
      S.cs_n = e->d_shcmn.p + ng * WAVE;
      e->d_shbounds.ensure(ng * (size_t)sdh::SH_BOUNDS);
      S.bounds = e->d_shbounds.p;
      if (const char* v = sdh::knob("SDH_RATCHET_SCATTER"))
        S.scatter = !strcmp(v, "pair") ? sdh::SH_SCATTER_PAIR : !strcmp(v, "lane") ? sdh::SH_SCATTER_LANE : sdh::SH_SCATTER_RULE;
      e->d_shtemp.ensure(sdh_ratchet_shared_temp(n) + 16);
      return S;
    };
    // one launch per (key kind, orientation, SIM form)
    auto run = [&](const RatchetLaunch& L0) {
      for (int i0 = 0; i0 < n_items;) {
        const int g0 = e->ritems[i0].g;
        const int kk = e->rg[g0].key_kind, xm = e->rg[g0].xmask, sim = lsim(g0), gate = lgate(g0);
        int i1 = i0;
        while (i1 < n_items && lkey(e->ritems[i1].g) == lkey(g0)) ++i1;
        RatchetLaunch Ls = L0;
        Ls.items = e->d_ritems.p + i0;
        Ls.n_items = i1 - i0;
        int nf = 0;
        for (int i = i0; i < i1; ++i) nf = std::max(nf, ratchet_nf(e->rg[e->ritems[i].g]));
        // spill regions are indexed by the item's position in its launch
        Ls.spillA = e->d_rspillA.p + (size_t)i0 * e->rSC * WAVE;
        Ls.lds_ts = e->d_rlts.p + (size_t)i0 * e->rML * WAVE;
        Ls.spillB = any64 ? e->d_rspillB.p + (size_t)i0 * e->rSC * WAVE : nullptr;
        Ls.rec4 = L0.rec4 && sim && !gate ? 1 : 0;  // (rec4 blocks come from the SIM form only)
        any_rec4 |= Ls.rec4;
        if (Ls.rec4 && !Ls.pcnt && !Ls.crow && lshared(g0)) {
          // one pre-pass per launch = per (stream, key column, OP) of the push
          const SharedLaunch S = shared_setup(g0);
          HIPCHK(hipMemsetAsync(S.cnt, 0, 8, e->stream));
          HIPCHK(sdh_launch_ratchet_shared_pre(&S, &B, e->d_err.p, e->d_shtemp.p, e->d_shtemp.n, e->stream));
          HIPCHK(sdh_launch_ratchet_shared(&Ls, &S, e->stream));
          any_shared = 1;
        } else if (gate) {
          int ng = 0;
          for (int i = i0; i < i1; ++i) ng = std::max(ng, e->rg[e->ritems[i].g].n_g);
          HIPCHK(sdh_launch_gate(kk, xm, full, nf, ng, e->rSC, &Ls, e->stream));
        } else {
          HIPCHK(sdh_launch_ratchet(kk, xm, full, nf, full ? 0 : sim, e->rML, e->rSC, &Ls, e->stream));
        }
        i0 = i1;
      }
    };
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    run(L);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    int32_t errs[5], used = 0;
    HIPCHK(hipMemcpyAsync(errs, e->d_err.p, 20, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&used, e->d_blk_next.p, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    if (sdh::knob("SDH_TRACE"))
      fprintf(stderr, "[sdh] ratchet stream %d n %lld attempt %d full %d rec4 %d items %d blocks %d/%lld errs %d %d %d %d %d: %.2f ms\n",
              stream, (long long)n, attempt, (int)full, L.rec4, n_items, used, (long long)e->r_blocks, errs[0], errs[1],
              errs[2], errs[3], errs[4], ms);
    if (errs[3]) throw Error(SDH_E_CAPACITY, "a pending partial is more than 2^31 events old");
    if (errs[1] && !full) {  // timestamps out of order: exact re-run with the full expiry scan
      e->r_full_expiry[stream] = 1;
      continue;
    }
    if (errs[0]) {
      // exact re-run with a larger spill ring (and persisted deques to hold it): the reference's
      // pending list is unbounded (StreamPreStateProcessor.java:298)
      if (e->rSC >= (1 << 24))
        throw Error(SDH_E_CAPACITY, fmt("more than %d pending partials in one pattern", e->rML + e->rSC));
      e->rSC *= 2;
      ratchet_grow_rsmax(e, e->rML + e->rSC);
      continue;
    }
    if (errs[2]) {
      // out of blocks: blk_next ends at the number of blocks the launch's waves asked for (a wave past
      // the last block writes into the spare one and keeps counting), so one re-run with that many fits
      const int64_t need = std::max<int64_t>(2 * e->r_blocks, (int64_t)used + used / 64 + 64);
      const int64_t blk_bytes = (int64_t)e->r_blk_recs * 8 * (wide ? 2 : 1);
      size_t fr = 0, tot = 0;
      HIPCHK(hipMemGetInfo(&fr, &tot));
      const double have = (double)fr + (double)e->d_rmatch.n * 8.0 - (double)(1 << 30);
      int64_t nb = std::max<int64_t>((int64_t)used + used / 64 + 64, e->r_blocks + 1);
      if ((double)(need + 1) * blk_bytes <= have) nb = std::max(nb, need);
      if ((double)(nb + 1) * blk_bytes > have || nb >= INT32_MAX)
        throw Error(SDH_E_CAPACITY, fmt("the push's match records need %.1f GB of HBM (%.1f GB free): push fewer events "
                                        "per call", (double)(nb + 1) * blk_bytes / 1e9, have / 1e9));
      e->r_blocks = nb;
      continue;
    }
    if (errs[4] && L.rec4) {  // a rec4 entry's e1 distance reached 2^26: exact re-run with 8-B records
      no_rec4 = true;  // (this push only: the next one tries rec4 again)
      ++e->r_rec4_reruns;
      continue;
    }
    int64_t placed_rows = 0;
    if (placing) {
      // the (event, cell) counts -> each cell's first row; then the same items again, writing
      e->p_ptemp.ensure(sdh_place_temp_bytes(cells));
      HIPCHK(sdh_place_total(e->p_cnt.p, cells, e->d_rtotal.p + 1, e->stream));
      HIPCHK(sdh_place_scan(e->p_cnt.p, cells, e->p_ptemp.p, e->p_ptemp.n, e->stream));
      unsigned long long tot = 0;
      HIPCHK(hipMemcpyAsync(&tot, e->d_rtotal.p + 1, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      placed_rows = (int64_t)tot;
      const int64_t n0 = e->mt.n;
      if (tot >= (unsigned long long)INT32_MAX || n0 + placed_rows >= INT32_MAX) {  // (2^31 rows: table records)
        no_place = true;
        continue;
      }
      e->pc_rows.grow_keep((size_t)((n0 + placed_rows) * e->cw), (size_t)(n0 * e->cw), e->stream);
      RatchetLaunch W = L;
      W.pcnt = nullptr;
      W.pbase = e->p_cnt.p;
      W.crow = e->pc_rows.p;
      W.cw = e->cw;
      W.row0 = n0;
      e->r_place_row0 = n0;
      W.seq_ref = e->seq_ref;
      float ms2 = 0;
      HIPCHK(hipEventRecord(e->ev0, e->stream));
      run(W);
      HIPCHK(hipEventRecord(e->ev1, e->stream));
      HIPCHK(hipEventSynchronize(e->ev1));
      HIPCHK(hipEventElapsedTime(&ms2, e->ev0, e->ev1));
      ms += ms2;
    }
    for (int g : gs) e->rcur[g] ^= 1;
    e->r_shared_pushes += any_shared;
    e->r_placing = placing;
    e->r_blk_taken = used;
    e->r_seq_base = B.seq_base;
    if (placing) {
      e->r_blocks_used = 0;
      e->r_matches = placed_rows;
    } else if (devrec) {  // left on the device for sdh_engine_poll_records: the blocks 0 .. used-1
      unsigned long long tot[3] = {0, 0, 0};
      HIPCHK(hipMemcpy(tot, e->d_rtotal.p, 24, hipMemcpyDeviceToHost));
      e->r_blocks_used = used;
      e->r_matches = (int64_t)tot[0];
      e->r_rec_bytes = (double)tot[2];
      e->r_rec4 = any_rec4;
    } else {
      e->r_blocks_used = std::min<int>(used, (int)e->r_blocks);
      e->r_blk_count.resize(e->r_blocks_used);
      if (e->r_blocks_used)
        HIPCHK(hipMemcpy(e->r_blk_count.data(), e->d_blk_count.p, e->r_blocks_used * 4, hipMemcpyDeviceToHost));
      e->r_matches = ratchet_count_matches(e);
    }
    e->r_kernel_ms = ms;
    e->r_wide = wide;
    // algorithmic bytes: every group streams the batch's operand columns once
    // (ts + x-atom column + f0 columns; the warm-up re-reads are overhead, not counted), writes
    // 32 B per match (SURVEY §8(d)'s unit; the device record is 8 B, expanded at poll) and reads +
    // writes its persisted deques (24 B per pending partial)
    double bytes = 0;
    for (int g : gs) {
      const RatchetGroup& G = e->rg[g];
      int64_t ev_bytes = 8 + B.width[G.key_attr];
      for (int a = 0; a < G.n_f0; ++a) {
        if (G.f0[a].attr != G.key_attr) ev_bytes += B.width[G.f0[a].attr];
        if (G.f0[a].cur2 && G.f0[a].attr2 != G.key_attr) ev_bytes += B.width[G.f0[a].attr2];
      }
      for (int a = 0; a < G.n_g; ++a)  // (K_gate's gate columns)
        if (G.g[a].attr != G.key_attr) ev_bytes += B.width[G.g[a].attr];
      bytes += (double)n * ev_bytes;
    }
    bytes += (double)e->r_matches * 32.0;
    e->r_kernel_bytes = bytes;
    return;
  }
  throw Error(SDH_E_CAPACITY, "ratchet launch did not converge");
}

// ---- snapshot sections (engine_snap.hip): K_chain, per query its header and table
void snap_save_chain(sdh_engine* e, snap::Writer& w) {
  const size_t tbl = (size_t)NF * e->pcap;
  for (size_t q = 0; q < e->lq.size(); ++q) {
    InstHeader h;
    HIPCHK(hipMemcpy(&h, e->d_hdr[e->cur[q]].p + q, sizeof h, hipMemcpyDeviceToHost));
    w.put(h.seed_alive);
    w.put(h.n_live);
    put_dev(w, e->d_part[e->cur[q]].p + q * tbl, tbl * 8);
  }
}

// (spcap: the snapshot's table capacity. A growing engine adopts larger tables; smaller ones load into
// the lanes they have)
void snap_load_chain(sdh_engine* e, snap::Reader& r, int64_t spcap) {
  if (spcap > e->pcap) chain_grow(e, spcap);
  const size_t tbl = (size_t)NF * e->pcap;
  std::vector<int64_t> rows(tbl);
  for (size_t q = 0; q < e->lq.size(); ++q) {
    InstHeader h{(int32_t)r.get(), (int32_t)r.get(), 0, 0};
    const int64_t* src = r.words((size_t)NF * spcap);
    for (int f = 0; f < NF; ++f) {
      int64_t* row = rows.data() + (size_t)f * e->pcap;
      std::copy(src + (size_t)f * spcap, src + (size_t)(f + 1) * spcap, row);
      std::fill(row + spcap, row + e->pcap, f == F_STATE ? -1 : 0);
    }
    HIPCHK(hipMemcpy(e->d_hdr[e->cur[q]].p + q, &h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_part[e->cur[q]].p + q * tbl, rows.data(), tbl * 8, hipMemcpyHostToDevice));
  }
}

// K_ratchet deques: per group, per lane: n then n x (ts0, seq, key)
void snap_save_ratchet(sdh_engine* e, snap::Writer& w) {
  const size_t ng = e->rg.size();
  w.put((int64_t)ng);
  for (size_t g = 0; g < ng; ++g) {
    const int b = e->rcur[g];
    RatchetState rs;
    HIPCHK(hipMemcpy(&rs, e->d_rst[b].p + g, sizeof rs, hipMemcpyDeviceToHost));
    std::vector<int64_t> t(e->rsmax * WAVE), sq(e->rsmax * WAVE), ky(e->rsmax * WAVE);
    const size_t o = g * e->rsmax * WAVE;
    HIPCHK(hipMemcpy(t.data(), e->d_rts[b].p + o, t.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sq.data(), e->d_rsq[b].p + o, sq.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ky.data(), e->d_rky[b].p + o, ky.size() * 8, hipMemcpyDeviceToHost));
    for (int l = 0; l < WAVE; ++l) {
      w.put(rs.n[l]);
      for (int i = 0; i < rs.n[l]; ++i) {
        w.put(t[i * WAVE + l]);
        w.put(sq[i * WAVE + l]);
        w.put(ky[i * WAVE + l]);
      }
    }
  }
}

void snap_load_ratchet(sdh_engine* e, snap::Reader& r) {
  const size_t ng = (size_t)r.get();
  snap::need(ng == e->rg.size(), "snapshot of a different program");
  // the persisted capacity grows to the longest deque first (a copy of the reader scans ahead for it)
  int64_t longest = 0;
  snap::Reader scan = r;
  for (size_t k = 0; k < ng * WAVE; ++k) {
    const int64_t nl = scan.get();
    snap::need(nl >= 0 && nl <= ((int64_t)1 << 26) && 3 * (size_t)nl <= scan.left(), "bad snapshot deque length");
    longest = std::max(longest, nl);
    scan.skip(3 * (size_t)nl);
  }
  ratchet_grow_rsmax(e, longest);
  for (size_t g = 0; g < ng; ++g) {
    const int b = e->rcur[g];
    RatchetState rs{};
    std::vector<int64_t> t(e->rsmax * WAVE, 0), sq(e->rsmax * WAVE, 0), ky(e->rsmax * WAVE, 0);
    for (int l = 0; l < WAVE; ++l) {
      rs.n[l] = (int32_t)r.get();
      for (int i = 0; i < rs.n[l]; ++i) {
        t[i * WAVE + l] = r.get();
        sq[i * WAVE + l] = r.get();
        ky[i * WAVE + l] = r.get();
      }
    }
    const size_t o = g * e->rsmax * WAVE;
    HIPCHK(hipMemcpy(e->d_rst[b].p + g, &rs, sizeof rs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_rts[b].p + o, t.data(), t.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_rsq[b].p + o, sq.data(), sq.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_rky[b].p + o, ky.data(), ky.size() * 8, hipMemcpyHostToDevice));
  }
}

}  // namespace eng
}  // namespace sdh
