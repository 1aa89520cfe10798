// engine.hip -- host side of libsiddhi_hip.so: plan selection, HBM state management, batching
// and match hand-off. Implements include/siddhi_hip.h.
// IR lowering is in engine_lower.hip, the K_gen / K_seq / K_part / K_slab passes in engine_gen.hip, the
// K_chain and K_ratchet launches in engine_ratchet.hip, the K_slab arena in engine_slab.hip, the snapshot
// blob in engine_snap.hip (engine_int.h).
//
// The reference has no device boundary; the engine is the GpuStateStreamRuntime half that replaces
// StateInputStreamParser's object graph (core/util/parser/StateInputStreamParser.java:77-398) with
// device tables, and the receiver loop (core/query/input/*ProcessStreamReceiver.java) with one
// batched launch per pushed event batch.
#include "engine_int.h"
#include "launchers.h"
#include "mix_plan.h"
#include "rec_rows.h"

namespace {

void ensure_state(sdh_engine* e) {
  const size_t nq = e->lq.size();
  for (int b = 0; b < 2; ++b) {
    e->d_hdr[b].ensure(std::max<size_t>(nq, 1));
    e->d_part[b].ensure(std::max<size_t>(nq, 1) * NF * e->pcap);
  }
  // initial state: every query seeded (QueryRuntime.init -> StreamPreStateProcessor.init:157-166)
  std::vector<InstHeader> h(nq);
  for (auto& x : h) x = InstHeader{1, 0, 0, 0};
  std::vector<int64_t> part(nq * NF * e->pcap, 0);
  for (size_t q = 0; q < nq; ++q)
    for (int l = 0; l < e->pcap; ++l) part[(q * NF + F_STATE) * e->pcap + l] = -1;
  for (int b = 0; b < 2; ++b) {
    if (nq) {
      HIPCHK(hipMemcpy(e->d_hdr[b].p, h.data(), nq * sizeof(InstHeader), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->d_part[b].p, part.data(), part.size() * 8, hipMemcpyHostToDevice));
    }
  }
  e->cur.assign(nq, 0);
}

// ---- device match table (matches.hip) ----
sdh::MatchTable table_view(sdh_engine* e) {
  sdh::MatchTable T{};
  auto& t = e->mt;
  T.hi = t.hi.p;
  for (int k = 0; k < MAXLO; ++k) T.lo[k] = t.lo[k].p;
  T.seq = t.seq.p;
  T.q = t.q.p;
  T.key = t.key.p;
  T.ts = t.ts.p;
  T.woff = t.woff.p;
  T.wlen = t.wlen.p;
  T.words = t.words.p;
  T.chi = t.chi.p;
  T.clo = t.clo.p;
  return T;
}

// room for `rows` more rows and `words` more words (contents kept)
void table_reserve(sdh_engine* e, int64_t rows, int64_t words) {
  auto& t = e->mt;
  const size_t want = (size_t)(t.n + rows), keep = (size_t)t.n;
  t.hi.grow_keep(want, keep, e->stream);
  for (int k = 0; k < MAXLO; ++k) t.lo[k].grow_keep(want, keep, e->stream);
  t.seq.grow_keep(want, keep, e->stream);
  t.q.grow_keep(want, keep, e->stream);
  t.key.grow_keep(want, keep, e->stream);
  t.ts.grow_keep(want, keep, e->stream);
  t.woff.grow_keep(want, keep, e->stream);
  t.wlen.grow_keep(want, keep, e->stream);
  t.words.grow_keep((size_t)(t.nw + words), (size_t)t.nw, e->stream);
}

// the last push's K_chain matches (per work item output segments) -> table
void append_chain(sdh_engine* e) {
  const int n_items = (int)e->work.size();
  if (e->device_matches == 0 || n_items == 0) return;
  std::vector<int64_t> seg_off(n_items), dst_off(n_items);
  int64_t acc = 0;
  for (int i = 0; i < n_items; ++i) {
    seg_off[i] = e->work[i].seg_off;
    dst_off[i] = acc;
    acc += e->seg_count[i];
  }
  table_reserve(e, acc, acc * 2 * MAXS);
  e->d_seg_off.ensure(n_items);
  e->d_dst_off.ensure(n_items);
  HIPCHK(hipMemcpyAsync(e->d_seg_off.p, seg_off.data(), n_items * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_dst_off.p, dst_off.data(), n_items * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(sdh_append_chain(e->d_match.p, e->d_seg_off.p, e->d_seg_count.p, e->d_dst_off.p, e->rec_words, n_items,
                          e->d_qinfo.p, e->seq_ref, e->d_out_rank.p, (int)e->prog.stream_types.size(),
                          table_view(e), e->mt.n, e->mt.nw, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mt.n += acc;
  e->mt.nw += acc * 2 * MAXS;
  e->mt.n_lo = std::max(e->mt.n_lo, e->rec_words - 3);
}

// the last push's K_ratchet match blocks -> table (ts_col: the batch's ts column, still valid)
void append_ratchet(sdh_engine* e, const int64_t* ts_col, int64_t seq_base) {
  const int nb = e->r_blocks_used;
  if (nb == 0 || e->r_matches == 0) return;
  std::vector<int64_t> dst_off(nb);
  int64_t acc = 0;
  for (int i = 0; i < nb; ++i) {
    dst_off[i] = acc;
    acc += e->r_blk_count[i];
  }
  table_reserve(e, acc, acc * 4);
  e->d_dst_off.ensure(nb);
  HIPCHK(hipMemcpyAsync(e->d_dst_off.p, dst_off.data(), nb * 8, hipMemcpyHostToDevice, e->stream));
  HIPCHK(sdh_append_ratchet(e->d_rmatch.p, e->r_blk_recs, e->r_wide, e->d_blk_count.p, e->d_blk_group.p,
                            e->d_dst_off.p, e->d_rg.p, ts_col, seq_base, e->seq_ref, e->d_out_rank.p,
                            (int)e->prog.stream_types.size(), nb, table_view(e), e->mt.n, e->mt.nw, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mt.n += acc;
  e->mt.nw += acc * 4;
  e->mt.n_lo = std::max(e->mt.n_lo, 1);
}

// per query its partition's key table, on the device (narrow K_part records carry the key's dense id)
void upload_qkeys(sdh_engine* e) {
  const size_t nq = std::max<size_t>(1, e->prog.q.size());
  std::vector<const int64_t*> qk(nq, nullptr);
  for (const auto& g : e->gq)
    if (g.partition >= 0 && g.partition < (int)e->routes.size() && e->routes[g.partition] && g.qid >= 0 &&
        (size_t)g.qid < nq)
      qk[(size_t)g.qid] = e->routes[g.partition]->key_of_id.p;
  // K_wave's narrow records carry key id 0 of a one-word table holding -1 (an unpartitioned query's key)
  for (const auto& ws : e->wsets)
    for (int gx : ws->qs)
      if (e->gq[gx].qid >= 0 && (size_t)e->gq[gx].qid < nq) qk[(size_t)e->gq[gx].qid] = e->d_wave_key.p;
  e->d_qkeys.ensure(nq);
  HIPCHK(hipMemcpyAsync(e->d_qkeys.p, qk.data(), nq * sizeof(void*), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
}

// the last push's K_gen / K_seq / K_part records -> table: each record's table words (narrow K_part
// records expand), scanned, then the rows. bts / seq_base / stream: the push's batch (narrow records
// take their trigger's ts from it); null for a time advance (timer records only)
void append_gen(sdh_engine* e, const int64_t* bts, int64_t seq_base, int stream) {
  const int64_t n_rec = e->g_dev_matches;
  if (n_rec == 0) return;
  e->g_tw.ensure((size_t)n_rec + 1);
  e->g_twtemp.ensure(sdh_gen_words_temp_bytes(n_rec));
  e->g_nwide.ensure(1);
  HIPCHK(sdh_gen_words(e->g_out.p, e->g_rec_off.p, n_rec, e->g_tw.p, e->g_twtemp.p, e->g_twtemp.n, e->g_nwide.p,
                       e->stream));
  int64_t words = 0;
  unsigned long long n_wide = 0;
  HIPCHK(hipMemcpyAsync(&n_wide, e->g_nwide.p, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&words, e->g_tw.p + n_rec, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  table_reserve(e, n_rec, words);
  upload_qkeys(e);
  HIPCHK(sdh_append_gen(e->g_out.p, e->g_rec_off.p, n_rec, e->seq_ref, e->d_out_rank.p,
                        e->has_fanout ? e->d_fan_rank.p : nullptr, (int)e->prog.stream_types.size(), table_view(e),
                        e->mt.n, e->mt.nw, e->g_tw.p, bts, seq_base, stream, e->d_qkeys.p, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mt.n += n_rec;
  e->mt.nw += words;
  // timer records: (key, query, time); fan-out records: (position, rank, emission). K_part's narrow
  // records need no tiebreak pass: the matches of one (trigger event, query) come from one lane,
  // which emits them in list order, so the stable sort on the primary key keeps them in it
  if (n_wide) e->mt.n_lo = std::max(e->mt.n_lo, e->has_absent || e->has_fanout ? 3 : 1);
  // K_part chains walk entry-major: one event's matches of an instance are ordered by the earlier
  // slots' seqs (nfa_types.h), so their rows take the tiebreak passes
  e->mt.n_lo = std::max(e->mt.n_lo, e->part_chain_lo);
  // K_wave: one event's matches of a query come from many lanes and pages; their rows carry e1's seq
  // as the first tiebreak (the pending-list order, nfa_wave.hip), so the poll takes that pass
  if (!e->wsets.empty()) e->mt.n_lo = std::max(e->mt.n_lo, 1);
}

void table_clear(sdh_engine* e) {
  e->mt.n = 0;
  e->mt.nw = 0;
  e->mt.n_lo = 0;
  e->mt.placed = false;
  e->mt.chunked = false;
  e->mt.chunk_pushed = false;
  e->mt.ck_n = 0;
  e->mt.max_run = 0;
  e->seq_ref = e->seq;
  e->r_placing = false;  // (the placed rows are gone)
}

// chunk keys of rows [ck_n, r1): single-event rows (chunk = false), or the rows the chunk push in
// progress appended (matches.hip chunk_keys_kernel)
void chunk_keys(sdh_engine* e, int64_t r1, bool chunk) {
  auto& t = e->mt;
  if (r1 <= t.ck_n) return;
  t.chi.grow_keep((size_t)r1, (size_t)t.ck_n, e->stream);
  t.clo.grow_keep((size_t)r1, (size_t)t.ck_n, e->stream);
  const int ns = (int)e->prog.stream_types.size();
  HIPCHK(sdh_chunk_keys(table_view(e), t.ck_n, r1, chunk ? 1 : 0, e->ck.first_seq - e->seq_ref, e->ck.first_seq,
                        e->ck.stream, ns, e->d_ck_major.p, e->d_ck_minor.p, e->d_ck_qslot.p, e->ck_runs.p, e->ck.n,
                        e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  t.ck_n = r1;
}

// the rows a sub-push of the chunk in progress appended, from row n0 on
void chunk_rows(sdh_engine* e, int64_t n0) {
  if (e->mt.n <= n0) return;
  e->mt.chunked = true;
  chunk_keys(e, n0, false);
  chunk_keys(e, e->mt.n, true);
}

// a placed push joins the window: its rows are already in pc_rows; the compact rows carry seqs
// only, so the window keeps the pushed events' times (ts_log[seq - seq_ref])
void place_commit(sdh_engine* e, const int64_t* ts_col, int64_t seq_base, int64_t n_events) {
  e->mt.placed = true;
  if (e->r_matches == 0) return;  // (rows reference their own push's events only)
  const int64_t t0 = seq_base - e->seq_ref;
  e->ts_log.grow_keep((size_t)(t0 + n_events), (size_t)t0, e->stream);
  HIPCHK(hipMemcpyAsync(e->ts_log.p + t0, ts_col, (size_t)n_events * 8, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mt.n += e->r_matches;
  ++e->stats.placed_pushes;
}

// placed rows -> general table rows (a later push of the window has other producers)
void placed_to_table(sdh_engine* e) {
  if (!e->mt.placed) return;
  const int64_t n = e->mt.n;
  e->mt.n = 0;
  e->mt.nw = 0;
  table_reserve(e, n, 4 * n);
  HIPCHK(sdh_placed_to_table(e->pc_rows.p, e->cw, n, e->ts_log.p, e->seq_ref, e->d_out_rank.p, e->d_qinfo.p,
                             (int)e->prog.stream_types.size(), table_view(e), e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mt.n = n;
  e->mt.nw = 4 * n;
  e->mt.n_lo = std::max(e->mt.n_lo, 1);
  e->mt.placed = false;
}

int bits_of(uint64_t v) {
  int b = 0;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// the ABI output arrays in HBM for n matches of tw words (po_*; off and len have n + 1 entries)
// (at least 64K rows: a window that edges past the last size would otherwise reallocate -- a
// device allocation inside the poll, the p99 of small pushes)
constexpr int64_t POLL_MIN_ROWS = 1 << 16;
void poll_reserve(sdh_engine* e, int64_t n, int64_t tw) {
  const size_t m = (size_t)std::max<int64_t>(n, POLL_MIN_ROWS);
  tw = std::max<int64_t>(tw, 4 * POLL_MIN_ROWS);
  n = std::max<int64_t>(n, POLL_MIN_ROWS);
  e->po_q.ensure(m);
  e->po_key.ensure(m);
  e->po_ts.ensure(m);
  e->po_seq.ensure(m);
  e->po_tb.ensure(m);
  e->po_len.ensure(n + 1);
  e->po_off.ensure(n + 1);
  e->po_words.ensure((size_t)std::max<int64_t>(tw, 1));
}

// R18 sort of the table's n > 0 rows and gather of the ABI arrays except the words; returns the
// sorted order (perm[i] = the table row of match i)
int32_t* table_order(sdh_engine* e, int64_t* total_words) {
  const int64_t n = e->mt.n;
  if (n >= INT32_MAX) throw Error(SDH_E_CAPACITY, "more than 2^31 matches between two polls");
  e->p_keys.ensure((size_t)n * 2);
  e->p_perm.ensure((size_t)n * 2);
  const size_t tb = sdh_poll_temp_bytes(n);
  e->p_temp.ensure(tb);
  poll_reserve(e, n, 0);
  // timer records' tiebreaks are a full timestamp, the query and the partition key
  const int lo_bits = e->has_absent ? 64 : std::max(1, bits_of((uint64_t)std::max<int64_t>(e->seq, 1 << 16)));
  const int hi_bits = bits_of((uint64_t)(e->seq - e->seq_ref)) + RANK_BITS;
  int clo_bits = 0;
  if (e->mt.chunked) {  // the window holds chunk rows: the single-event rows' chunk keys, 2 passes more
    chunk_keys(e, n, false);
    clo_bits = bits_of((uint64_t)e->mt.max_run) + RANK_BITS;
  }
  int32_t* perm = nullptr;
  HIPCHK(sdh_poll_sort(table_view(e), n, e->mt.n_lo, lo_bits, hi_bits, clo_bits, e->p_keys.p, e->p_perm.p,
                       e->p_temp.p, e->p_temp.n, e->po_q.p, e->po_key.p, e->po_ts.p, e->po_seq.p, e->po_tb.p,
                       e->po_len.p, e->po_off.p, &perm, total_words, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return perm;
}

// ------------------------------------------------------------------------------------------
// Event store and device selector (select.hip): sdh_engine_retain_events / sdh_engine_poll_rows
// ------------------------------------------------------------------------------------------
void check_usable(sdh_engine* e);

template <class T>
void upload(DevBuf<T>& d, const std::vector<T>& v) {
  d.ensure(std::max<size_t>(1, v.size()));
  if (!v.empty()) HIPCHK(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

// the select lists lowered (host only; sdh_engine_query_outputs needs no more)
void sel_lower(sdh_engine* e) {
  if (e->sel_ready) return;
  e->selp = lower_outputs(e->lp);
  e->sel_ready = true;
}

// the batch's events into the store, rows by seq (a batch longer than the ring: its last ev_cap events)
void store_append(sdh_engine* e, StreamBatch B, const std::vector<int>& types) {
  if (B.n > e->ev_cap) {
    const int64_t skip = B.n - e->ev_cap;
    B.ts += skip;
    for (int a = 0; a < B.n_attr; ++a) {
      B.col[a] = (const uint8_t*)B.col[a] + skip * B.width[a];
      if (B.nul[a]) B.nul[a] += skip;
    }
    B.seq_base += skip;
    B.n = e->ev_cap;
  }
  uint32_t fm = 0;
  for (int a = 0; a < B.n_attr; ++a)
    if (types[a] == T_FLOAT) fm |= 1u << a;
  HIPCHK(sdh_store_append(&B, fm, e->ev_rows.p, e->ev_cap - 1, e->ev_w, e->stream));
}

int do_retain(sdh_engine* e, int64_t events) {
  check_usable(e);
  HIPCHK(hipSetDevice(e->dev));
  if (events > ((int64_t)1 << 40)) throw Error(SDH_E_INVALID, "sdh_engine_retain_events: more than 2^40 events");
  int64_t cap = 1;
  while (cap < events) cap <<= 1;
  if (e->ev_cap == 0) {
    sel_lower(e);
    upload(e->d_sel_code, e->selp.code);
    upload(e->d_sel_outs, e->selp.outs);
    upload(e->d_sel_shapes, e->selp.shapes);
    upload(e->d_sel_queries, e->selp.queries);
    upload(e->d_sel_consts, e->selp.consts);
    size_t na = 0;
    for (const auto& s : e->prog.stream_types) na = std::max(na, s.size());
    e->ev_w = 2 + (int)na;
    e->ev_first = e->seq;  // events pushed before this call were not kept
  }
  if (cap <= e->ev_cap) return SDH_OK;
  // a larger ring: the present rows move to their places in it
  int64_t* q = nullptr;
  const size_t bytes = (size_t)cap * e->ev_w * 8;
  alloc_trace("event_store", bytes);
  if (hipMalloc(&q, bytes) != hipSuccess) {
    (void)hipGetLastError();
    throw Error(SDH_E_CAPACITY, fmt("device memory exhausted for an event store of %lld events", (long long)cap));
  }
  if (e->ev_cap) {
    const int64_t lo = std::max(e->ev_first, e->seq - e->ev_cap);
    hipError_t rc = sdh_store_relay(e->ev_rows.p, e->ev_cap - 1, q, cap - 1, e->ev_w, lo, e->seq - lo, e->stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e->stream);
    if (rc != hipSuccess) {
      (void)hipFree(q);
      HIPCHK(rc);
    }
    e->ev_first = lo;
    HIPCHK(hipFree(e->ev_rows.p));
  }
  e->ev_rows.p = q;
  e->ev_rows.n = (size_t)cap * e->ev_w;
  e->ev_cap = cap;
  return SDH_OK;
}

// sdh_engine_poll_rows: the window's matches projected into output rows. A sorted window goes through
// table_order's permutation, a placed one is read from its compact rows: neither is expanded into the
// other. An event that has left the store fails the call with the window left pending (the convention
// of do_poll_compact for rows it cannot express).
int do_poll_rows(sdh_engine* e, sdh_rows* out, bool device) {
  check_usable(e);
  if (!e->ev_cap) throw Error(SDH_E_INVALID, "sdh_engine_poll_rows: no events are kept (sdh_engine_retain_events)");
  const auto& S = e->selp;
  if (S.over >= 0)
    throw Error(SDH_E_UNSUPPORTED, fmt("query %d selects more than %d outputs", S.over, sel::MAXOUT));
  if (S.bad) throw Error(SDH_E_INVALID, "a select list names a slot or an attribute its query lacks, or holds an unknown opcode");
  if (S.max_depth > kg::GSTACK - 1)
    throw Error(SDH_E_UNSUPPORTED, "a select expression is too deep for the device evaluation stack");
  HIPCHK(hipSetDevice(e->dev));
  const int64_t n = e->mt.n;
  const int width = S.width;
  const size_t rows = (size_t)std::max<int64_t>(n, POLL_MIN_ROWS);
  e->pr_q.ensure(rows);
  e->pr_nulls.ensure(rows);
  e->pr_cells.ensure(rows * (size_t)std::max(1, width));
  e->pr_err.ensure(1);
  poll_reserve(e, n, 0);
  if (n) {
    const sel::Tables T{e->d_sel_code.p, e->d_sel_outs.p, e->d_sel_shapes.p, e->d_sel_queries.p, e->d_sel_consts.p};
    const sel::Store st{e->ev_rows.p, e->ev_cap - 1, std::max(e->ev_first, e->seq - e->ev_cap), e->ev_w, 0};
    const int deep = S.max_depth > kg::RSTACK;
    HIPCHK(hipMemsetAsync(e->pr_err.p, 0, 4, e->stream));
    if (e->mt.placed) {
      HIPCHK(sdh_select_placed(&T, &st, deep, e->pc_rows.p, e->cw, e->ts_log.p, e->seq_ref, n, width, e->pr_q.p,
                               e->po_ts.p, e->po_seq.p, e->pr_cells.p, e->pr_nulls.p, e->pr_err.p, e->stream));
    } else {
      int64_t tw = 0;
      const int32_t* perm = table_order(e, &tw);
      HIPCHK(sdh_select_sorted(&T, &st, deep, table_view(e), perm, e->po_q.p, n, width, e->pr_q.p, e->pr_cells.p,
                               e->pr_nulls.p, e->pr_err.p, e->stream));
    }
    int32_t bad = 0;
    d2h_sync(e, &bad, e->pr_err.p, 4);
    if (bad)
      throw Error(SDH_E_CAPACITY, fmt("a match reads an event that has left the event store of %lld events: raise "
                                      "sdh_engine_retain_events (the matches stay pending: sdh_engine_poll)",
                                      (long long)e->ev_cap));
  }
  out->n = n;
  out->width = width;
  out->flags = 0;
  if (device) {
    out->query = e->pr_q.p;
    out->ts = e->po_ts.p;
    out->seq = e->po_seq.p;
    out->cells = e->pr_cells.p;
    out->nulls = e->pr_nulls.p;
  } else {
    e->hr_q.ensure(rows);
    e->ho_ts.ensure(rows);
    e->ho_seq.ensure(rows);
    e->hr_nulls.ensure(rows);
    e->hr_cells.ensure(rows * (size_t)std::max(1, width));
    if (n) {
      HIPCHK(hipMemcpyAsync(e->hr_q.p, e->pr_q.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_ts.p, e->po_ts.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_seq.p, e->po_seq.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->hr_nulls.p, e->pr_nulls.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      if (width)
        HIPCHK(hipMemcpyAsync(e->hr_cells.p, e->pr_cells.p, (size_t)n * width * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    out->query = e->hr_q.p;
    out->ts = e->ho_ts.p;
    out->seq = e->ho_seq.p;
    out->cells = e->hr_cells.p;
    out->nulls = e->hr_nulls.p;
  }
  table_clear(e);
  return SDH_OK;
}

// Host-resident batch -> HBM (the StreamJunction -> receiver hand-off of north_star (2)): the
// columns go to one device buffer over the side stream `h2d`; pinned caller memory is copied
// directly, pageable memory through two pinned staging slots whose host copy of slice i+1 overlaps
// the DMA of slice i. The compute stream waits on the transfer's event.
void stage_host_batch(sdh_engine* e, const sdh_batch* b, StreamBatch& B) {
  const int na = B.n_attr;
  const int64_t n = b->n;
  struct Part {
    const void* src;
    size_t bytes, off;
  };
  std::vector<Part> parts;
  size_t total = 0;
  auto add = [&](const void* src, size_t bytes) {
    total = (total + 255) & ~(size_t)255;
    parts.push_back({src, bytes, total});
    total += bytes;
  };
  add(b->ts, (size_t)n * 8);
  for (int a = 0; a < na; ++a) add(b->cols[a], (size_t)n * B.width[a]);
  for (int a = 0; a < na; ++a)
    if (b->nulls && b->nulls[a]) add(b->nulls[a], (size_t)n);
  e->d_batch.ensure(total);
  float ms = 0;
  HIPCHK(hipEventRecord(e->ev_h0, e->h2d));
  const size_t SLICE = (size_t)4 << 20;
  for (const Part& p : parts) {
    hipPointerAttribute_t at{};
    const bool pinned = hipPointerGetAttributes(&at, p.src) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    uint8_t* dst = e->d_batch.p + p.off;
    if (pinned) {
      HIPCHK(hipMemcpyAsync(dst, p.src, p.bytes, hipMemcpyHostToDevice, e->h2d));
      continue;
    }
    for (size_t o = 0; o < p.bytes; o += SLICE) {
      const size_t len = std::min(SLICE, p.bytes - o);
      const int slot = e->stage_next;
      e->stage_next ^= 1;
      e->stage[slot].ensure(SLICE);
      HIPCHK(hipEventSynchronize(e->ev_stage[slot]));  // the slot's previous DMA has drained
      memcpy(e->stage[slot].p, (const uint8_t*)p.src + o, len);
      HIPCHK(hipMemcpyAsync(dst + o, e->stage[slot].p, len, hipMemcpyHostToDevice, e->h2d));
      HIPCHK(hipEventRecord(e->ev_stage[slot], e->h2d));
    }
  }
  HIPCHK(hipEventRecord(e->ev_h1, e->h2d));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_h1, 0));
  HIPCHK(hipEventSynchronize(e->ev_h1));
  HIPCHK(hipEventElapsedTime(&ms, e->ev_h0, e->ev_h1));
  e->stats.last_ingest_ms = ms;
  e->stats.ingest_bytes += (int64_t)total;
  size_t k = 0;
  B.ts = (const int64_t*)(e->d_batch.p + parts[k++].off);
  for (int a = 0; a < na; ++a) B.col[a] = e->d_batch.p + parts[k++].off;
  for (int a = 0; a < na; ++a) {
    B.nul[a] = nullptr;
    if (b->nulls && b->nulls[a]) B.nul[a] = e->d_batch.p + parts[k++].off;
  }
}

int do_push(sdh_engine* e, int32_t stream, const sdh_batch* b) {
  if (!b || stream < 0 || stream >= (int)e->prog.stream_types.size())
    throw Error(SDH_E_INVALID, "bad stream or batch");
  const auto& types = e->prog.stream_types[stream];
  const int na = (int)types.size();
  if (b->n_cols != na) throw Error(SDH_E_INVALID, fmt("stream %d has %d attributes, batch has %d", stream, na, b->n_cols));
  if (b->n < 0 || (e->cfg.max_batch > 0 && b->n > e->cfg.max_batch))
    throw Error(SDH_E_INVALID, "batch larger than max_batch");
  if (b->n == 0) return SDH_OK;
  check_fan_strings(e, stream);
  HIPCHK(hipSetDevice(e->dev));
  // an exact re-run needs the journal of the K_gen blocks the push modifies (gen_journal): a batch
  // whose bound does not fit a third of free HBM is pushed as two halves -- the same events in the
  // same order, so the same matches
  if (!e->gsets.empty() && b->n > 1) {
    size_t fr = 0, tot = 0;
    const char* jb = sdh::knob("SDH_JOURNAL_BUDGET");  // (tests: force the split)
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && gen_journal_bound(e, b->n) > (jb ? atof(jb) : (double)fr / 3)) {
      std::vector<const void*> c0(na), c1(na);
      std::vector<const uint8_t*> n0(na), n1(na);
      const int64_t h = b->n / 2;
      for (int a = 0; a < na; ++a) {
        c0[a] = b->cols[a];
        c1[a] = (const uint8_t*)b->cols[a] + h * attr_width(types[a]);
        n0[a] = b->nulls ? b->nulls[a] : nullptr;
        n1[a] = (b->nulls && b->nulls[a]) ? b->nulls[a] + h : nullptr;
      }
      sdh_batch first = *b, second = *b;
      first.n = h;
      first.cols = c0.data();
      first.nulls = b->nulls ? n0.data() : nullptr;
      second.n = b->n - h;
      second.ts = b->ts + h;
      second.cols = c1.data();
      second.nulls = b->nulls ? n1.data() : nullptr;
      do_push(e, stream, &first);
      return do_push(e, stream, &second);
    }
  }
  (void)hipGetLastError();
  StreamBatch B{};
  B.n = b->n;
  B.n_attr = na;
  B.stream = stream;
  B.seq_base = e->seq;
  B.prev_ts = e->prev_ts[stream];
  for (int a = 0; a < na; ++a) B.width[a] = attr_width(types[a]);
  if (b->on_device) {
    B.ts = b->ts;
    for (int a = 0; a < na; ++a) {
      B.col[a] = b->cols[a];
      B.nul[a] = b->nulls ? b->nulls[a] : nullptr;
    }
  } else {
    stage_host_batch(e, b, B);
  }
  if (e->ev_cap) store_append(e, B, types);
  std::vector<int> qs;
  for (int li = 0; li < (int)e->lq.size(); ++li)
    if (std::find(e->lq[li].streams.begin(), e->lq[li].streams.end(), stream) != e->lq[li].streams.end())
      qs.push_back(li);
  int64_t t01[2];
  if (b->on_device) {
    d2h_sync(e, &t01[0], B.ts, 8);
    d2h_sync(e, &t01[1], B.ts + (b->n - 1), 8);
  } else {
    t01[0] = b->ts[0];
    t01[1] = b->ts[b->n - 1];
  }
  double ms = 0, bytes = 0;
  int64_t consumers = 0;
  if (!e->started) {  // the runtime starts with its first event unless sdh_engine_start said when
    e->started = true;
    e->start_ts = t01[0];
  }
  // the previous push's device-only matches (SDH_FLAG_DEVICE_MATCHES) are dropped here
  e->work.clear();
  e->device_matches = 0;
  e->r_blocks_used = 0;
  e->r_blk_taken = 0;
  e->r_matches = 0;
  e->g_dev_matches = 0;
  e->g_used = 0;
  e->dev_polled = false;
  e->rr_ready = 0;
  e->last_n = b->n;
  e->last_seq_base = B.seq_base;
  for (auto& k : e->part_kept) k = b->n;
  try {
    if (!qs.empty()) {
      bool unordered = false;
      launch(e, stream, B, t01, qs, true, &unordered);
      bool chunked = false;
      for (auto& w : e->work) chunked |= w.n_chunks > 1;
      if (unordered && chunked) launch(e, stream, B, t01, qs, false, &unordered);  // exact fallback
      for (int li : qs) e->cur[li] ^= 1;
      ms += e->stats.last_kernel_ms;
      bytes += e->stats.last_kernel_bytes;
      consumers += (int64_t)qs.size();
    }
    // K_gen before K_ratchet: a push whose only matches are K_ratchet's places them directly
    double gms = 0, gbytes = 0;
    e->stats.last_gen_items = 0;
    e->stats.last_seq_items = 0;
    launch_gen(e, stream, B, &gms, &gbytes);
    ms += gms;
    bytes += gbytes;
    launch_ratchet(e, stream, B, t01);
    for (const auto& g : e->rg)
      if (g.stream == stream) consumers += g.n_lanes;
    ms += e->r_kernel_ms;
    bytes += e->r_kernel_bytes;
  } catch (const std::exception& ex) {
    // kernels may already have advanced part of the state: the engine no longer mirrors the
    // reference, so every later call fails (restore a snapshot or recreate)
    e->prev_ts[stream] = t01[1];
    e->seq += b->n;
    e->broken = ex.what();
    throw;
  }
  // (event, query) evaluations: a partition's queries see only the events routed to a key of this
  // engine (null keys and other ranks' keys are not evaluated)
  int64_t pe = b->n * consumers;
  for (const auto& g : e->gq)
    if (g.recv_n[stream] > 0) {
      ++consumers;
      pe += g.partition >= 0 && g.partition < (int)e->part_kept.size() ? e->part_kept[g.partition] : b->n;
    }
  if (consumers) {
    e->stats.pattern_events += pe;
    e->stats.matches += e->device_matches + e->r_matches;
    e->stats.last_kernel_ms = ms;
    e->stats.last_kernel_bytes = bytes;
  }
  e->prev_ts[stream] = t01[1];
  e->seq += b->n;
  e->stats.events += b->n;
  // the push is committed; its matches join the device table (R18-sorted at poll), or, when they
  // all come from K_ratchet, are already at their R18 rows (placed by the launch: no sort at poll)
  if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES)) {
    const bool only_ratchet = e->device_matches == 0 && e->g_dev_matches == 0;
    if (e->r_placing) {
      place_commit(e, B.ts, B.seq_base, b->n);
    } else if (!(only_ratchet && e->r_matches == 0)) {
      placed_to_table(e);
      const int64_t n0 = e->mt.n;
      append_chain(e);
      append_ratchet(e, B.ts, B.seq_base);
      append_gen(e, B.ts, B.seq_base, stream);
      if (e->ck.active) chunk_rows(e, n0);
    }
  }
  return SDH_OK;
}

// ------------------------------------------------------------------------------------------
// Interleaved pushes (sdh_engine_push_mixed; DESIGN.md §3.2 "Interleaved pushes")
// ------------------------------------------------------------------------------------------
struct MixRun {
  int part;
  int64_t off, n;  // events [off, off + n) of the part
};

// the maximal same-part runs of a host `order` (values already checked)
std::vector<MixRun> mix_runs(const int32_t* order, int64_t n, int n_parts) {
  std::vector<MixRun> runs;
  std::vector<int64_t> used((size_t)n_parts, 0);
  for (int64_t k = 0; k < n;) {
    const int p = order[k];
    int64_t k1 = k;
    while (k1 < n && order[k1] == p) ++k1;
    runs.push_back({p, used[p], k1 - k});
    used[p] += k1 - k;
    k = k1;
  }
  return runs;
}

// the split path: each run is a contiguous slice of its part, pushed as do_push's own journal split
// pushes its halves
void mix_split(sdh_engine* e, const sdh_mixed_part* parts, const std::vector<MixRun>& runs) {
  for (const MixRun& r : runs) {
    const sdh_batch& b = parts[r.part].batch;
    const int stream = parts[r.part].stream;
    const auto& types = e->prog.stream_types[stream];
    const int na = (int)types.size();
    std::vector<const void*> cols(na);
    std::vector<const uint8_t*> nl(na);
    for (int a = 0; a < na; ++a) {
      cols[a] = (const uint8_t*)b.cols[a] + r.off * attr_width(types[a]);
      nl[a] = (b.nulls && b.nulls[a]) ? b.nulls[a] + r.off : nullptr;
    }
    sdh_batch v = b;
    v.n = r.n;
    v.ts = b.ts + r.off;
    v.cols = cols.data();
    v.nulls = b.nulls ? nl.data() : nullptr;
    do_push(e, stream, &v);
  }
}

// the call as mix_plan.h sees it: per named stream the plans that read it, and the engine-wide facts.
// *gen_runs: a K_gen query reads a part that has events (the native call launches the K_gen kernel)
mixplan::Call mix_call(const sdh_engine* e, int n_parts, const sdh_mixed_part* parts, int64_t total, bool* gen_runs) {
  static_assert(mixplan::MAX_PARTS == MIX_MAXP, "part limit");
  mixplan::Call c;
  const char* k = sdh::knob("SDH_MIX_SPLIT");
  c.knob_split = k && atoi(k) != 0;
  c.comm = e->comm != nullptr;
  c.n_parts = n_parts;
  c.total = total;
  for (const auto& gs : e->gsets) c.timed_gen |= gs->timed;  // time passes for the set on every push, whatever its stream
  *gen_runs = false;
  for (int p = 0; p < n_parts && p < MIX_MAXP; ++p) {
    const int s = parts[p].stream;
    uint32_t kinds = 0;
    for (const auto& q : e->lq)
      if (std::find(q.streams.begin(), q.streams.end(), s) != q.streams.end()) kinds |= mixplan::C_CHAIN;
    for (const auto& g : e->rg)
      if (g.stream == s) kinds |= g.n_g > 0 ? mixplan::C_GATE : mixplan::C_RATCHET;
    if (s >= kg::GMAXSTREAM) {
      if (!e->gq.empty()) kinds |= mixplan::C_RANGE;
    } else {
      for (size_t i = 0; i < e->gq.size(); ++i)
        if (e->gq[i].recv_n[s] > 0) kinds |= e->gq_kind[i];
    }
    c.consumers[p] = kinds;
    if ((kinds & mixplan::C_GEN) && parts[p].batch.n > 0) *gen_runs = true;
  }
  return c;
}

// the native path: pre-pass, one K_chain launch and one K_gen launch over the merged sequence, the table
// append and the event store from the merged positions. cnt: the parts' events; order: host or device (order_dev)
void mix_native(sdh_engine* e, int n_parts, const sdh_mixed_part* parts, const int32_t* order, int64_t total,
                bool order_dev, bool counted) {
  const bool on_dev = parts[0].batch.on_device != 0;
  const int ns = (int)e->prog.stream_types.size();
  MixLaunch ML{};
  MixPre A{};
  ML.n_parts = A.n_parts = n_parts;
  std::vector<int32_t> pstream((size_t)ns, -1);
  std::vector<int64_t> last_ts((size_t)n_parts, 0);
  int64_t off = 0;
  for (int p = 0; p < n_parts; ++p) {
    const sdh_batch& b = parts[p].batch;
    const int stream = parts[p].stream;
    const auto& types = e->prog.stream_types[stream];
    StreamBatch& B = ML.parts[p];
    B.n = b.n;
    B.n_attr = (int)types.size();
    B.stream = stream;
    B.seq_base = e->seq;
    B.prev_ts = e->prev_ts[stream];
    for (int a = 0; a < B.n_attr; ++a) B.width[a] = attr_width(types[a]);
    pstream[stream] = p;
    A.part_n[p] = b.n;
    A.pos_off[p] = off;
    off += b.n;
    if (b.n == 0) continue;
    if (on_dev) {
      B.ts = b.ts;
      for (int a = 0; a < B.n_attr; ++a) {
        B.col[a] = b.cols[a];
        B.nul[a] = b.nulls ? b.nulls[a] : nullptr;
      }
    } else {
      // (stage_host_batch fills d_batch: each part keeps its own buffer)
      e->d_batch.swap(e->d_mix_batch[p]);
      try {
        stage_host_batch(e, &b, B);
      } catch (...) {
        e->d_batch.swap(e->d_mix_batch[p]);
        throw;
      }
      e->d_batch.swap(e->d_mix_batch[p]);
      last_ts[p] = b.ts[b.n - 1];
    }
    A.ts[p] = B.ts;
  }
  // ---- pre-pass ----
  const int64_t nb = sdh_mix_blocks(total);
  e->d_mix_idx.ensure((size_t)total);
  e->d_mix_pos.ensure((size_t)total);
  e->d_mix_ts.ensure((size_t)total);
  e->d_mix_cnt.ensure((size_t)nb * MIX_MAXP);
  e->d_mix_total.ensure(MIX_MAXP);
  e->d_mix_err.ensure(1);
  if (!order_dev) {
    e->d_mix_order.ensure((size_t)total);
    HIPCHK(hipMemcpyAsync(e->d_mix_order.p, order, (size_t)total * 4, hipMemcpyHostToDevice, e->stream));
    order = e->d_mix_order.p;
  }
  A.order = order;
  A.n = total;
  A.blk_cnt = e->d_mix_cnt.p;
  A.total = e->d_mix_total.p;
  A.err = e->d_mix_err.p;
  A.idx = e->d_mix_idx.p;
  A.ts_out = e->d_mix_ts.p;
  A.pos = e->d_mix_pos.p;
  if (!counted) {  // (a device order's counts, checked by the caller before this point, left the scan behind)
    HIPCHK(hipMemsetAsync(e->d_mix_err.p, 0, 4, e->stream));
    HIPCHK(sdh_mix_count(&A, e->stream));
  }
  HIPCHK(sdh_mix_write(&A, e->stream));
  int64_t t01[2];
  d2h_sync(e, &t01[0], e->d_mix_ts.p, 8);
  d2h_sync(e, &t01[1], e->d_mix_ts.p + (total - 1), 8);
  if (on_dev)
    for (int p = 0; p < n_parts; ++p)
      if (parts[p].batch.n > 0) d2h_sync(e, &last_ts[p], parts[p].batch.ts + (parts[p].batch.n - 1), 8);
  ML.order = order;
  ML.idx = e->d_mix_idx.p;
  e->d_mix_pstream.ensure((size_t)ns);
  HIPCHK(hipMemcpyAsync(e->d_mix_pstream.p, pstream.data(), (size_t)ns * 4, hipMemcpyHostToDevice, e->stream));
  ML.part_of_stream = e->d_mix_pstream.p;
  e->d_mix.ensure(1);
  HIPCHK(hipMemcpyAsync(e->d_mix.p, &ML, sizeof(ML), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));  // (ML and pstream are on this frame)
  // ---- the merged batch: timestamps, count and first seq; the columns are the parts' ----
  StreamBatch B{};
  B.n = total;
  B.stream = -1;
  B.seq_base = e->seq;
  B.prev_ts = INT64_MIN;
  B.ts = e->d_mix_ts.p;
  if (e->ev_cap) {
    const int64_t first = std::max<int64_t>(0, total - e->ev_cap);
    for (int p = 0; p < n_parts; ++p) {
      const auto& types = e->prog.stream_types[parts[p].stream];
      uint32_t fm = 0;
      for (int a = 0; a < ML.parts[p].n_attr; ++a)
        if (types[a] == T_FLOAT) fm |= 1u << a;
      HIPCHK(sdh_store_append_mixed(&ML.parts[p], fm, e->d_mix_pos.p + A.pos_off[p], first, e->ev_rows.p, e->ev_cap - 1,
                                    e->ev_w, e->stream));
    }
  }
  // the queries that read a stream with events in this call, and what run pushes would have counted
  std::vector<int> qs;
  int64_t pe = 0, consumers = 0;
  for (int li = 0; li < (int)e->lq.size(); ++li) {
    bool reads = false;
    for (int p = 0; p < n_parts; ++p) {
      const auto& st = e->lq[li].streams;
      if (parts[p].batch.n > 0 && std::find(st.begin(), st.end(), parts[p].stream) != st.end()) {
        reads = true;
        pe += parts[p].batch.n;
        ++consumers;
      }
    }
    if (reads) qs.push_back(li);
  }
  // the K_gen queries likewise (all of them in the unpartitioned set: mix_plan.h), per part they read
  uint32_t gen_mask = 0;
  for (int p = 0; p < n_parts; ++p) {
    const int s = parts[p].stream;
    if (parts[p].batch.n == 0 || s >= kg::GMAXSTREAM) continue;
    for (const auto& g : e->gq)
      if (g.recv_n[s] > 0) {
        gen_mask |= 1u << s;
        pe += parts[p].batch.n;
        ++consumers;
      }
  }
  if (!e->started) {
    e->started = true;
    e->start_ts = t01[0];
  }
  // (as do_push: the previous push's device-only matches are dropped here)
  e->work.clear();
  e->device_matches = 0;
  e->r_blocks_used = 0;
  e->r_blk_taken = 0;
  e->r_matches = 0;
  e->r_placing = false;
  e->r_kernel_ms = 0;
  e->r_kernel_bytes = 0;
  e->r_rec_bytes = 0;
  e->r_rec4 = 0;
  e->g_dev_matches = 0;
  e->g_used = 0;
  e->dev_polled = false;
  e->rr_ready = 0;
  e->last_n = total;
  e->last_seq_base = B.seq_base;
  for (auto& k : e->part_kept) k = total;
  e->stats.last_gen_items = 0;
  e->stats.last_seq_items = 0;
  auto commit_clock = [&]() {
    for (int p = 0; p < n_parts; ++p)
      if (parts[p].batch.n > 0) e->prev_ts[parts[p].stream] = last_ts[p];
    e->seq += total;
  };
  double ms = 0, bytes = 0;
  if (!qs.empty() || gen_mask) {
    e->mix = e->d_mix.p;
    e->mix_mask = gen_mask;
    try {
      if (!qs.empty()) {
        bool unordered = false;
        launch(e, -1, B, t01, qs, false, &unordered);
        for (int li : qs) e->cur[li] ^= 1;
        ms = e->stats.last_kernel_ms;
        bytes = e->stats.last_kernel_bytes;
      }
      // the K_gen pass after the K_chain launch, with launch_gen's own journal and exact re-runs: a pool or
      // output overflow repeats this pass alone (the K_chain launch above has its own loop)
      if (gen_mask) {
        double gms = 0, gbytes = 0;
        launch_gen(e, -1, B, &gms, &gbytes);  // (adds its records to stats.matches)
        ms += gms;
        bytes += gbytes;
      }
    } catch (const std::exception& ex) {
      e->mix = nullptr;
      e->mix_mask = 0;
      commit_clock();
      e->broken = ex.what();
      throw;
    }
    e->mix = nullptr;
    e->mix_mask = 0;
  }
  if (consumers) {
    e->stats.pattern_events += pe;
    e->stats.matches += e->device_matches;
    e->stats.last_kernel_ms = ms;
    e->stats.last_kernel_bytes = bytes;
  }
  commit_clock();
  e->stats.events += total;
  if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) && (e->device_matches > 0 || e->g_dev_matches > 0)) {
    placed_to_table(e);
    append_chain(e);
    // bstream (the rank column of narrow records) is unused here: no narrow record kind can occur, the
    // path writes K_gen's wide records only, which carry their trigger's stream in word 6
    append_gen(e, B.ts, B.seq_base, 0);
  }
}

int do_push_mixed(sdh_engine* e, int32_t n_parts, const sdh_mixed_part* parts, const int32_t* order, int64_t n_order,
                  int32_t order_on_device) {
  // ---- refusals, before anything changes ----
  if (n_parts < 0 || (n_parts > 0 && !parts) || n_order < 0 || (n_order > 0 && !order))
    throw Error(SDH_E_INVALID, "sdh_engine_push_mixed: bad parts or order");
  const int ns = (int)e->prog.stream_types.size();
  std::vector<char> named((size_t)ns, 0);
  int64_t total = 0;
  for (int p = 0; p < n_parts; ++p) {
    const sdh_batch& b = parts[p].batch;
    const int s = parts[p].stream;
    if (s < 0 || s >= ns) throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: part %d names stream %d", p, s));
    if (named[s]) throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: stream %d is named twice", s));
    named[s] = 1;
    if (b.chunk) throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: part %d is a chunk (chunk delivery is per stream)", p));
    const int na = (int)e->prog.stream_types[s].size();
    if (b.n_cols != na)
      throw Error(SDH_E_INVALID, fmt("stream %d has %d attributes, part %d has %d", s, na, p, b.n_cols));
    if (b.n < 0 || (b.n > 0 && (!b.ts || (na > 0 && !b.cols))))
      throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: part %d has a bad batch", p));
    if ((b.on_device != 0) != (parts[0].batch.on_device != 0))
      throw Error(SDH_E_INVALID, "sdh_engine_push_mixed: host and device parts in one call");
    total += b.n;
  }
  if (n_order != total)
    throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: order has %lld entries, the parts %lld events",
                                   (long long)n_order, (long long)total));
  if (e->cfg.max_batch > 0 && total > e->cfg.max_batch) throw Error(SDH_E_INVALID, "batch larger than max_batch");
  if (total == 0) return SDH_OK;
  HIPCHK(hipSetDevice(e->dev));
  bool gen_runs = false;
  bool native = mixplan::why_split(mix_call(e, n_parts, parts, total, &gen_runs)) == nullptr;
  // the K_gen pass journals the blocks it modifies (gen_journal): a call whose bound does not fit the
  // budget is not native -- decided here, before anything changes. (The split path's run pushes halve
  // their batches as do_push does.)
  if (native && gen_runs) {
    size_t fr = 0, tot = 0;
    const char* jb = sdh::knob("SDH_JOURNAL_BUDGET");
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && gen_journal_bound(e, total) > (jb ? atof(jb) : (double)fr / 3))
      native = false;
    (void)hipGetLastError();
  }
  // the parts' counts in `order`: on the host, or for a device order bound for the native path by the
  // pre-pass's count and scan (nothing of the engine's state is touched by them)
  std::vector<int32_t> horder;
  std::vector<int64_t> cnt((size_t)std::max(n_parts, 1), 0);
  bool counted = false;
  if (order_on_device && native) {
    MixPre A{};
    A.order = order;
    A.n = total;
    A.n_parts = n_parts;
    e->d_mix_cnt.ensure((size_t)sdh_mix_blocks(total) * MIX_MAXP);
    e->d_mix_total.ensure(MIX_MAXP);
    e->d_mix_err.ensure(1);
    A.blk_cnt = e->d_mix_cnt.p;
    A.total = e->d_mix_total.p;
    A.err = e->d_mix_err.p;
    HIPCHK(hipMemsetAsync(e->d_mix_err.p, 0, 4, e->stream));
    HIPCHK(sdh_mix_count(&A, e->stream));
    int64_t tot[MIX_MAXP];
    int32_t bad = 0;
    HIPCHK(hipMemcpyAsync(tot, e->d_mix_total.p, sizeof(tot), hipMemcpyDeviceToHost, e->stream));
    d2h_sync(e, &bad, e->d_mix_err.p, 4);
    if (bad) throw Error(SDH_E_INVALID, "sdh_engine_push_mixed: an order entry names no part");
    for (int p = 0; p < n_parts; ++p) cnt[p] = tot[p];
    counted = true;
  } else {
    const int32_t* ho = order;
    if (order_on_device) {
      horder.resize((size_t)total);
      HIPCHK(hipMemcpy(horder.data(), order, (size_t)total * 4, hipMemcpyDeviceToHost));
      ho = horder.data();
    }
    for (int64_t k = 0; k < total; ++k) {
      if (ho[k] < 0 || ho[k] >= n_parts) throw Error(SDH_E_INVALID, "sdh_engine_push_mixed: an order entry names no part");
      ++cnt[ho[k]];
    }
  }
  for (int p = 0; p < n_parts; ++p)
    if (cnt[p] != parts[p].batch.n)
      throw Error(SDH_E_INVALID, fmt("sdh_engine_push_mixed: order names part %d %lld times, its batch has %lld events",
                                     p, (long long)cnt[p], (long long)parts[p].batch.n));
  if (!native && (e->cfg.flags & SDH_FLAG_DEVICE_MATCHES))
    throw Error(SDH_E_UNSUPPORTED, "sdh_engine_push_mixed: this call runs as one push per same-stream run, and with "
                                   "SDH_FLAG_DEVICE_MATCHES each run would drop the records of the run before it");
  for (int p = 0; p < n_parts; ++p)
    if (parts[p].batch.n > 0) check_fan_strings(e, parts[p].stream);
  if (native) {
    mix_native(e, n_parts, parts, order, total, order_on_device != 0, counted);
    ++e->mixed_native;
  } else {
    mix_split(e, parts, mix_runs(order_on_device ? horder.data() : order, total, n_parts));
    ++e->mixed_split;
  }
  return SDH_OK;
}

// knobs.h: the knobs of the engine whose ABI call runs on this thread
thread_local const std::vector<std::pair<std::string, std::string>>* t_knobs = nullptr;
struct KnobScope {
  const std::vector<std::pair<std::string, std::string>>* prev;
  explicit KnobScope(const sdh_engine* e) : prev(t_knobs) { t_knobs = e ? &e->knobs : nullptr; }
  ~KnobScope() { t_knobs = prev; }
};

template <class F>
int guard(sdh_engine* e, F f) {
  KnobScope ks(e);
  try {
    return f();
  } catch (const Error& ex) {
    if (e) e->err = ex.what();
    return ex.code;
  } catch (const std::exception& ex) {
    if (e) e->err = ex.what();
    return SDH_E_INVALID;
  }
}

void check_usable(sdh_engine* e) {
  if (!e->broken.empty())
    throw Error(SDH_E_CAPACITY, "engine state is undefined after a failed push (" + e->broken +
                                    "); restore a snapshot or create a new engine");
}

// R18-sorted matches since the last poll; host == false leaves them in HBM (sdh_engine_poll_device)
// The window's matches R18-sorted into the ABI arrays in HBM (po_*; *tw words); with `kw_spec`
// (chunk words, lo words: sdh_engine_gather) also each row's merge key into x_keys.
int64_t poll_sorted(sdh_engine* e, int64_t* tw, const int* kw_spec = nullptr) {
  int64_t n = 0;
  *tw = 0;
  const int kw = kw_spec ? 2 * kw_spec[0] + 1 + 3 * kw_spec[1] : 0;
  if (kw) e->x_keys.ensure((size_t)std::max<int64_t>(1, e->mt.n) * kw);
  if (e->mt.placed) {  // compact rows already in R18 order (place_ratchet): 4 words per match
    n = e->mt.n;
    *tw = 4 * n;
    poll_reserve(e, n, *tw);
    HIPCHK(sdh_compact_fill(e->pc_rows.p, e->cw, n, e->ts_log.p, e->seq_ref, e->po_q.p, e->po_key.p, e->po_ts.p,
                            e->po_seq.p, e->po_tb.p, e->po_off.p, e->po_words.p, e->stream));
    if (kw)
      HIPCHK(sdh_merge_keys_placed(e->pc_rows.p, e->cw, n, e->seq_ref, e->d_out_rank.p, e->d_qinfo.p,
                                   (int)e->prog.stream_types.size(), kw_spec[0], kw_spec[1], e->x_keys.p, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  } else if (e->mt.n > 0) {
    n = e->mt.n;
    const int32_t* perm = table_order(e, tw);
    e->po_words.ensure((size_t)std::max<int64_t>(*tw, 1));
    HIPCHK(sdh_poll_words(table_view(e), perm, n, e->po_off.p, e->po_words.p, e->stream));
    if (kw)
      HIPCHK(sdh_merge_keys_table(table_view(e), perm, n, kw_spec[0], kw_spec[1], e->mt.chunked ? 1 : 0, e->x_keys.p,
                                  e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (n == 0) {
    e->po_off.ensure(1);
    HIPCHK(hipMemsetAsync(e->po_off.p, 0, 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return n;
}

int do_poll(sdh_engine* e, sdh_matches* out, bool host) {
  check_usable(e);
  int64_t tw = 0;
  const int64_t n = poll_sorted(e, &tw);
  if (host) {  // (pinned; sized like poll_reserve's device arrays)
    const int64_t hn = std::max<int64_t>(n, POLL_MIN_ROWS);
    e->ho_q.ensure(hn);
    e->ho_key.ensure(hn);
    e->ho_ts.ensure(hn);
    e->ho_seq.ensure(hn);
    e->ho_tb.ensure(hn);
    e->ho_off.ensure(hn + 1);
    e->ho_words.ensure(std::max<int64_t>(tw, 4 * POLL_MIN_ROWS));
    e->ho_off.p[0] = 0;
    if (n) {
      HIPCHK(hipMemcpyAsync(e->ho_q.p, e->po_q.p, n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_key.p, e->po_key.p, n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_ts.p, e->po_ts.p, n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_seq.p, e->po_seq.p, n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_tb.p, e->po_tb.p, n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->ho_off.p, e->po_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, e->stream));
      if (tw) HIPCHK(hipMemcpyAsync(e->ho_words.p, e->po_words.p, tw * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
    out->query = e->ho_q.p;
    out->key = e->ho_key.p;
    out->ts = e->ho_ts.p;
    out->seq = e->ho_seq.p;
    out->tb = e->ho_tb.p;
    out->off = e->ho_off.p;
    out->words = e->ho_words.p;
  } else {
    out->query = e->po_q.p;
    out->key = e->po_key.p;
    out->ts = e->po_ts.p;
    out->seq = e->po_seq.p;
    out->tb = e->po_tb.p;
    out->off = e->po_off.p;
    out->words = e->po_words.p;
  }
  out->n = n;
  table_clear(e);
  return SDH_OK;
}

// the window's matches as compact rows (sdh_engine_poll_compact): a placed window hands out its rows
// as they are; otherwise the table is R18-sorted and converted, and a row the form cannot express
// fails the call with the window left pending
int do_poll_compact(sdh_engine* e, sdh_matches_compact* out, bool device) {
  check_usable(e);
  const int64_t n = e->mt.n;
  const int w = e->cw;
  if (!e->mt.placed && n) {
    if (e->seq - e->seq_ref >= INT32_MAX) throw Error(SDH_E_UNSUPPORTED, "compact rows: seq span past 2^31");
    int64_t tw = 0;
    const int32_t* perm = table_order(e, &tw);
    e->pc_rows.ensure((size_t)(n * w));
    e->pc_err.ensure(1);
    HIPCHK(hipMemsetAsync(e->pc_err.p, 0, 4, e->stream));
    HIPCHK(sdh_table_compact(table_view(e), perm, n, w, e->seq_ref, e->pc_rows.p, e->pc_err.p, e->stream));
    int32_t bad = 0;
    d2h_sync(e, &bad, e->pc_err.p, 4);
    if (bad)
      throw Error(SDH_E_UNSUPPORTED, "compact rows: a match has a count-state chain, a partition key or a timer "
                                     "(poll it with sdh_engine_poll)");
  }
  e->pc_rows.ensure(1);
  out->n = n;
  out->seq_base = e->seq_ref;
  out->width = w;
  out->flags = 0;
  if (device) {
    out->rows = e->pc_rows.p;
  } else {
    e->hc_rows.ensure((size_t)std::max<int64_t>(n * w, POLL_MIN_ROWS * w));
    if (n) d2h_sync(e, e->hc_rows.p, e->pc_rows.p, (size_t)(n * w) * 4);
    out->rows = e->hc_rows.p;
  }
  table_clear(e);
  return SDH_OK;
}

// sdh_engine_poll_compact_ex: every match as a compact row, chains in a side array, keys and timer
// tiebreaks beside the rows
int do_poll_compact_ex(sdh_engine* e, sdh_matches_compact_ex* out, bool device) {
  check_usable(e);
  const int64_t n = e->mt.n;
  const int w = e->cw;
  const bool want_key = !e->lp.parts.empty(), want_tb = e->has_absent;
  int64_t nch = 0;
  const size_t rows = (size_t)std::max<int64_t>(1, n);
  if (want_key) e->px_key.ensure(rows);
  if (want_tb) e->px_tb.ensure(rows);
  e->px_chain.ensure(1);
  if (!e->mt.placed && n) {
    if (e->seq - e->seq_ref >= INT32_MAX) throw Error(SDH_E_UNSUPPORTED, "compact rows: seq span past 2^31");
    int64_t tw = 0;
    const int32_t* perm = table_order(e, &tw);
    e->px_cw.ensure((size_t)n + 1);
    e->px_temp.ensure(sdh_ex_temp_bytes(n));
    HIPCHK(sdh_ex_chain_words(table_view(e), perm, n, e->px_cw.p, e->px_temp.p, e->px_temp.n, e->stream));
    HIPCHK(hipMemcpyAsync(&nch, e->px_cw.p + n, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->pc_rows.ensure((size_t)(n * w));
    e->px_chain.ensure((size_t)std::max<int64_t>(1, nch));
    e->pc_err.ensure(1);
    HIPCHK(hipMemsetAsync(e->pc_err.p, 0, 4, e->stream));
    HIPCHK(sdh_ex_rows(table_view(e), perm, n, w, e->seq_ref, e->px_cw.p, e->pc_rows.p, e->px_chain.p,
                       want_key ? e->px_key.p : nullptr, want_tb ? e->px_tb.p : nullptr, e->pc_err.p, e->stream));
    int32_t bad = 0;
    d2h_sync(e, &bad, e->pc_err.p, 4);
    if (bad) throw Error(SDH_E_UNSUPPORTED, "compact rows: a seq distance past 2^31 (poll it with sdh_engine_poll)");
  } else if (n) {  // placed K_ratchet rows: no key, no timer
    if (want_key) HIPCHK(sdh_fill_i64(e->px_key.p, n, -1, e->stream));
    if (want_tb) HIPCHK(sdh_fill_i64(e->px_tb.p, n, INT64_MIN, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->pc_rows.ensure(1);
  out->n = n;
  out->seq_base = e->seq_ref;
  out->width = w;
  out->flags = 0;
  out->n_chain = nch;
  if (device) {
    out->rows = e->pc_rows.p;
    out->key = want_key ? e->px_key.p : nullptr;
    out->tb = want_tb ? e->px_tb.p : nullptr;
    out->chain = e->px_chain.p;
  } else {
    e->hc_rows.ensure((size_t)std::max<int64_t>(n * w, POLL_MIN_ROWS * w));
    e->hx_chain.ensure((size_t)std::max<int64_t>(nch, 1));
    if (n) HIPCHK(hipMemcpyAsync(e->hc_rows.p, e->pc_rows.p, (size_t)(n * w) * 4, hipMemcpyDeviceToHost, e->stream));
    if (nch) HIPCHK(hipMemcpyAsync(e->hx_chain.p, e->px_chain.p, (size_t)nch * 4, hipMemcpyDeviceToHost, e->stream));
    if (want_key) {
      e->hx_key.ensure(rows);
      if (n) HIPCHK(hipMemcpyAsync(e->hx_key.p, e->px_key.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    }
    if (want_tb) {
      e->hx_tb.ensure(rows);
      if (n) HIPCHK(hipMemcpyAsync(e->hx_tb.p, e->px_tb.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    out->rows = e->hc_rows.p;
    out->key = want_key ? e->hx_key.p : nullptr;
    out->tb = want_tb ? e->hx_tb.p : nullptr;
    out->chain = e->hx_chain.p;
  }
  table_clear(e);
  return SDH_OK;
}

// ---- multi-GPU exchange (comm.h) ----
template <class F>
void xcall(F f) {
  try {
    f();
  } catch (const Error&) {
    throw;
  } catch (const std::invalid_argument& ex) {
    throw Error(SDH_E_INVALID, ex.what());
  } catch (const std::runtime_error& ex) {
    throw Error(SDH_E_DEVICE, ex.what());
  }
}

int push_chunk(sdh_engine* e, int32_t stream, const sdh_batch* b);

// sdh_engine_push_bcast: the root's batch (staged into HBM first when it is host-resident) goes to
// every rank -- a header {n, stream, chunk, null-mask bits}, then ts, the attribute columns and the
// null masks the header names -- and every rank pushes it from HBM.
int do_push_bcast(sdh_engine* e, int32_t stream, const sdh_batch* b, int root) {
  if (!e->comm) throw Error(SDH_E_INVALID, "sdh_engine_push_bcast: no communicator (sdh_engine_set_comm)");
  HIPCHK(hipSetDevice(e->dev));
  const bool am_root = xch::rank(e->comm) == root;
  int64_t hdr[xch::HDR] = {};
  StreamBatch B{};
  if (am_root && (!b || stream < 0 || stream >= (int)e->prog.stream_types.size() ||
                  b->n_cols != (int)e->prog.stream_types[stream].size() || b->n < 0)) {
    // an invalid batch still takes part in the collective, as an error header: every rank then fails
    // this call with SDH_E_INVALID (no rank waits on a broadcast the root never makes)
    hdr[0] = -1;
    xcall([&] { xch::bcast_hdr(e->comm, hdr, root, e->stream); });
    throw Error(SDH_E_INVALID, "bad stream or batch");
  }
  if (am_root) {
    const int na = b->n_cols;
    B.n = b->n;
    B.n_attr = na;
    for (int a = 0; a < na; ++a) B.width[a] = attr_width(e->prog.stream_types[stream][a]);
    if (b->n > 0 && !b->on_device) {
      stage_host_batch(e, b, B);
    } else {
      B.ts = b->ts;
      for (int a = 0; a < na; ++a) {
        B.col[a] = b->cols[a];
        B.nul[a] = b->nulls ? b->nulls[a] : nullptr;
      }
    }
    int64_t mask = 0;
    for (int a = 0; a < na; ++a)
      if (B.nul[a]) mask |= (int64_t)1 << a;
    hdr[0] = b->n;
    hdr[1] = stream;
    hdr[2] = b->chunk;
    hdr[3] = mask;
  }
  xcall([&] { xch::bcast_hdr(e->comm, hdr, root, e->stream); });
  const int64_t n = hdr[0];
  if (n < 0) throw Error(SDH_E_INVALID, "sdh_engine_push_bcast: the root's batch was invalid (bad stream or batch)");
  stream = (int32_t)hdr[1];
  if (stream < 0 || stream >= (int)e->prog.stream_types.size()) throw Error(SDH_E_INVALID, "broadcast: bad stream");
  const auto& types = e->prog.stream_types[stream];
  const int na = (int)types.size();
  if (n == 0) return SDH_OK;
  // the receivers' layout (256-B aligned parts in x_batch), the root's sources
  std::vector<xch::Buf> bufs;
  size_t total = 0;
  auto add = [&](const void* src, size_t bytes) {
    total = (total + 255) & ~(size_t)255;
    bufs.push_back({src, (void*)(uintptr_t)total, bytes});
    total += bytes;
  };
  add(B.ts, (size_t)n * 8);
  for (int a = 0; a < na; ++a) add(am_root ? B.col[a] : nullptr, (size_t)n * attr_width(types[a]));
  for (int a = 0; a < na; ++a)
    if (hdr[3] >> a & 1) add(am_root ? B.nul[a] : nullptr, (size_t)n);
  if (!am_root) {
    e->x_batch.ensure(total);
    for (auto& x : bufs) x.dst = e->x_batch.p + (uintptr_t)x.dst;
  }
  xcall([&] { xch::bcast_bufs(e->comm, bufs, root, e->stream); });
  std::vector<const void*> cols((size_t)na);
  std::vector<const uint8_t*> nuls((size_t)na, nullptr);
  auto at = [&](size_t i) -> const void* { return am_root ? bufs[i].src : bufs[i].dst; };
  size_t k = 1;
  for (int a = 0; a < na; ++a) cols[(size_t)a] = at(k++);
  for (int a = 0; a < na; ++a)
    if (hdr[3] >> a & 1) nuls[(size_t)a] = (const uint8_t*)at(k++);
  sdh_batch db{};
  db.n = n;
  db.ts = (const int64_t*)at(0);
  db.cols = cols.data();
  db.nulls = hdr[3] ? nuls.data() : nullptr;
  db.n_cols = na;
  db.on_device = 1;
  db.chunk = (int32_t)hdr[2];
  if (db.chunk && n > 1) return push_chunk(e, stream, &db);
  return do_push(e, stream, &db);
}

// sdh_engine_gather: this rank's sorted run and its merge keys go to rank 0 (a header {n, words,
// seq_ref, kw, seq} first), which merges the world's runs on the device (comm.hip sdh_merge_runs).
int do_gather(sdh_engine* e, sdh_matches* out, bool host) {
  if (!e->comm) throw Error(SDH_E_INVALID, "sdh_engine_gather: no communicator (sdh_engine_set_comm)");
  const int me = xch::rank(e->comm), W = xch::world(e->comm);
  if (e->cfg.shard_world != W || e->cfg.shard_rank != me)
    throw Error(SDH_E_INVALID, fmt("sdh_engine_gather: the engine is shard %d of %d, the communicator's rank %d of %d",
                                   e->cfg.shard_rank, e->cfg.shard_world, me, W));
  HIPCHK(hipSetDevice(e->dev));
  // the key words every rank uses (the same on all: same program, same pushes)
  const int spec[2] = {e->mt.chunk_pushed ? 1 : 0, e->has_absent ? 1 : 0};
  const int kw = 2 * spec[0] + 1 + 3 * spec[1];
  int64_t tw = 0;
  const int64_t n = poll_sorted(e, &tw, spec);
  int64_t hdr[xch::HDR] = {n, tw, e->seq_ref, kw, e->seq, 0, 0, 0};
  std::vector<int64_t> all((size_t)W * xch::HDR);
  xcall([&] { xch::gather_hdr(e->comm, hdr, all.data(), e->stream); });
  const bool local = xch::is_local(e->comm);
  // the poll windows must agree (same pushes since the last gather): with RCCL every rank holds every
  // header and refuses a mismatch before any rank clears its table or sends; the local
  // communicator's rank 0 checks before it clears its own
  for (int r = 0; r < W && (!local || me == 0); ++r) {
    const int64_t* h = all.data() + (size_t)r * xch::HDR;
    if (h[2] != hdr[2] || h[3] != kw || h[4] != hdr[4])
      throw Error(SDH_E_INVALID, fmt("sdh_engine_gather: rank %d's poll window differs from rank %d's (pushes out of step)", r, me));
  }
  const std::vector<xch::Buf> mine = {
      {e->po_q.p, nullptr, (size_t)n * 8},    {e->po_key.p, nullptr, (size_t)n * 8},
      {e->po_ts.p, nullptr, (size_t)n * 8},   {e->po_seq.p, nullptr, (size_t)n * 8},
      {e->po_tb.p, nullptr, (size_t)n * 8},   {e->po_off.p, nullptr, (size_t)(n + 1) * 8},
      {e->po_words.p, nullptr, (size_t)tw * 8}, {e->x_keys.p, nullptr, (size_t)n * kw * 8}};
  if (me != 0) {
    xcall([&] { xch::gather_bufs(e->comm, mine, {}, e->stream); });
    HIPCHK(hipStreamSynchronize(e->stream));  // (the sends drained before the buffers change)
    table_clear(e);
    poll_reserve(e, 0, 0);
    HIPCHK(hipMemsetAsync(e->po_off.p, 0, 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = sdh_matches{0, e->po_q.p, e->po_key.p, e->po_ts.p, e->po_off.p, e->po_words.p, e->po_seq.p, e->po_tb.p};
    return SDH_OK;
  }
  std::vector<int64_t> run_off((size_t)W + 1, 0), wbase((size_t)W, 0);
  int64_t TW = 0;
  for (int r = 0; r < W; ++r) {
    run_off[(size_t)r + 1] = run_off[(size_t)r] + all[(size_t)r * xch::HDR];
    wbase[(size_t)r] = TW;
    TW += all[(size_t)r * xch::HDR + 1];
  }
  const int64_t N = run_off[(size_t)W];
  const size_t rows = (size_t)std::max<int64_t>(1, N);
  e->xg_q.ensure(rows);
  e->xg_key.ensure(rows);
  e->xg_ts.ensure(rows);
  e->xg_seq.ensure(rows);
  e->xg_tb.ensure(rows);
  e->xg_off.ensure((size_t)N + W);
  e->xg_words.ensure((size_t)std::max<int64_t>(1, TW));
  e->xg_keys.ensure(rows * kw);
  std::vector<std::vector<xch::Buf>> recv((size_t)W);
  for (int r = 0; r < W; ++r) {
    const int64_t o = run_off[(size_t)r], nr = all[(size_t)r * xch::HDR], wr = all[(size_t)r * xch::HDR + 1];
    recv[(size_t)r] = {{nullptr, e->xg_q.p + o, (size_t)nr * 8},          {nullptr, e->xg_key.p + o, (size_t)nr * 8},
                       {nullptr, e->xg_ts.p + o, (size_t)nr * 8},         {nullptr, e->xg_seq.p + o, (size_t)nr * 8},
                       {nullptr, e->xg_tb.p + o, (size_t)nr * 8},         {nullptr, e->xg_off.p + o + r, (size_t)(nr + 1) * 8},
                       {nullptr, e->xg_words.p + wbase[(size_t)r], (size_t)wr * 8},
                       {nullptr, e->xg_keys.p + o * kw, (size_t)nr * kw * 8}};
  }
  if (local) {  // rank 0's own run (RCCL: a self send / receive inside the gather)
    for (size_t i = 0; i < mine.size(); ++i)
      if (recv[0][i].bytes)
        HIPCHK(hipMemcpyAsync(recv[0][i].dst, mine[i].src, recv[0][i].bytes, hipMemcpyDeviceToDevice, e->stream));
    std::vector<std::vector<xch::Buf>> others(recv);
    others[0].clear();
    xcall([&] { xch::gather_bufs(e->comm, {}, others, e->stream); });
  } else {
    xcall([&] { xch::gather_bufs(e->comm, mine, recv, e->stream); });
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  table_clear(e);
  e->go_q.ensure(rows);
  e->go_key.ensure(rows);
  e->go_ts.ensure(rows);
  e->go_seq.ensure(rows);
  e->go_tb.ensure(rows);
  e->go_len.ensure((size_t)N + 1);
  e->go_off.ensure((size_t)N + 1);
  e->go_src.ensure(rows);
  e->go_pos.ensure(rows);
  e->go_temp.ensure(sdh_merge_temp_bytes(N));
  int64_t total = 0;
  HIPCHK(sdh_merge_runs(e->xg_keys.p, kw, run_off.data(), W, N, e->xg_q.p, e->xg_key.p, e->xg_ts.p, e->xg_seq.p,
                        e->xg_tb.p, e->xg_off.p, wbase.data(), e->go_pos.p, e->go_q.p, e->go_key.p, e->go_ts.p,
                        e->go_seq.p, e->go_tb.p, e->go_len.p, e->go_off.p, e->go_src.p, e->go_temp.p, e->go_temp.n,
                        &total, e->stream));
  if (total != TW) throw Error(SDH_E_DEVICE, "sdh_engine_gather: merged word count differs from the runs'");
  e->go_words.ensure((size_t)std::max<int64_t>(1, TW));
  HIPCHK(sdh_merge_words(e->go_src.p, e->go_off.p, N, e->xg_words.p, e->go_words.p, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (!host) {
    *out = sdh_matches{N, e->go_q.p, e->go_key.p, e->go_ts.p, e->go_off.p, e->go_words.p, e->go_seq.p, e->go_tb.p};
    return SDH_OK;
  }
  const size_t hn = (size_t)std::max<int64_t>(N, 1);
  e->ho_q.ensure(hn);
  e->ho_key.ensure(hn);
  e->ho_ts.ensure(hn);
  e->ho_seq.ensure(hn);
  e->ho_tb.ensure(hn);
  e->ho_off.ensure((size_t)N + 1);
  e->ho_words.ensure((size_t)std::max<int64_t>(TW, 1));
  const std::vector<std::tuple<void*, const void*, size_t>> cp = {
      {e->ho_q.p, e->go_q.p, (size_t)N * 8},     {e->ho_key.p, e->go_key.p, (size_t)N * 8},
      {e->ho_ts.p, e->go_ts.p, (size_t)N * 8},   {e->ho_seq.p, e->go_seq.p, (size_t)N * 8},
      {e->ho_tb.p, e->go_tb.p, (size_t)N * 8},   {e->ho_off.p, e->go_off.p, (size_t)(N + 1) * 8},
      {e->ho_words.p, e->go_words.p, (size_t)TW * 8}};
  for (const auto& c : cp)
    if (std::get<2>(c)) HIPCHK(hipMemcpyAsync(std::get<0>(c), std::get<1>(c), std::get<2>(c), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *out = sdh_matches{N, e->ho_q.p, e->ho_key.p, e->ho_ts.p, e->ho_off.p, e->ho_words.p, e->ho_seq.p, e->ho_tb.p};
  return SDH_OK;
}

// the absent states' timers due by t fire, with the next event's seq (sdh_engine_advance_time, and
// a chunk push before its first event)
void time_advance(sdh_engine* e, int64_t t) {
  if (!e->has_absent) return;
  HIPCHK(hipSetDevice(e->dev));
  StreamBatch B{};
  B.n = 0;
  B.stream = 0;
  B.n_attr = (int)e->prog.stream_types[0].size();
  B.seq_base = e->seq;
  B.prev_ts = e->prev_ts[0];
  e->work.clear();
  e->device_matches = 0;
  e->r_blocks_used = 0;
  e->r_matches = 0;
  e->r_placing = false;  // (the digest then reads no stale placed rows)
  e->g_dev_matches = 0;
  e->g_used = 0;
  e->dev_polled = false;
  e->rr_ready = 0;
  e->last_n = 0;
  e->last_seq_base = e->seq;
  double ms = 0, bytes = 0;
  e->advance_to = t;
  try {
    launch_gen(e, 0, B, &ms, &bytes);
  } catch (const std::exception& ex) {
    e->advance_to = INT64_MIN;
    e->broken = ex.what();
    throw;
  }
  e->advance_to = INT64_MIN;
  if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) && e->g_dev_matches) {
    placed_to_table(e);
    append_gen(e, nullptr, 0, 0);
  }
}

// A chunk push (sdh_batch.chunk; include/siddhi_hip.h): per partition keyed on the stream, each
// event's same-key run start (PartitionStreamReceiver.receive(Event[]):214-239 -- runs of
// consecutive events with equal String.valueOf keys; an event with a null key is skipped and does
// not end a run), and per query the run table it reads (-1: none, -2: fan-out, by key position).
// Computed on the host from the key columns (copied back for a device-resident batch).
void chunk_begin(sdh_engine* e, int stream, const sdh_batch* b) {
  const int64_t n = b->n;
  const size_t nq = e->prog.q.size();
  std::vector<int32_t> qslot(std::max<size_t>(1, nq), -1), runs;
  int slots = 0;
  bool fan = false;
  for (const auto& pd : e->lp.parts) {
    int attr = -1;
    for (const auto& k : pd.keys)
      if (k.stream == stream) attr = (int)k.code[0].imm;
    if (attr < 0) {
      if (pd.fan(stream)) {
        fan = true;
        for (int pq : pd.queries) qslot[(size_t)pq] = -2;
      }
      continue;
    }
    for (int pq : pd.queries) qslot[(size_t)pq] = slots;
    const int type = e->lp.stream_types[stream][attr];
    const int w = attr_width(type);
    std::vector<uint8_t> col((size_t)n * w), nul;
    const bool has_nul = b->nulls && b->nulls[attr];
    if (has_nul) nul.resize((size_t)n);
    if (b->on_device) {
      d2h_sync(e, col.data(), b->cols[attr], col.size());
      if (has_nul) d2h_sync(e, nul.data(), b->nulls[attr], nul.size());
    } else {
      memcpy(col.data(), b->cols[attr], col.size());
      if (has_nul) memcpy(nul.data(), b->nulls[attr], nul.size());
    }
    runs.resize((size_t)(slots + 1) * n, 0);
    int32_t* r = runs.data() + (size_t)slots * n;
    int64_t prev = 0, start = 0;
    bool have = false;
    for (int64_t i = 0; i < n; ++i) {
      if (has_nul && nul[(size_t)i]) continue;
      int64_t raw;
      if (w == 8) memcpy(&raw, col.data() + (size_t)i * 8, 8);
      else if (w == 4) {
        int32_t v;
        memcpy(&v, col.data() + (size_t)i * 4, 4);
        raw = v;
      } else raw = col[(size_t)i];
      const int64_t k = kg::key_of_raw(type, raw);
      if (!have || k != prev) start = i;
      have = true;
      prev = k;
      r[i] = (int32_t)start;
    }
    ++slots;
  }
  e->ck_runs.ensure(std::max<size_t>(1, runs.size()));
  if (!runs.empty()) HIPCHK(hipMemcpy(e->ck_runs.p, runs.data(), runs.size() * 4, hipMemcpyHostToDevice));
  e->d_ck_qslot.ensure(qslot.size());
  HIPCHK(hipMemcpy(e->d_ck_qslot.p, qslot.data(), qslot.size() * 4, hipMemcpyHostToDevice));
  e->mt.max_run = std::max<int64_t>(e->mt.max_run, fan ? (int64_t)INT32_MAX : n);
}

int push_chunk(sdh_engine* e, int32_t stream, const sdh_batch* b) {
  if (stream < 0 || stream >= (int)e->prog.stream_types.size() || b->n_cols != (int)e->prog.stream_types[stream].size())
    throw Error(SDH_E_INVALID, "bad stream or batch");
  if (e->cfg.max_batch > 0 && b->n > e->cfg.max_batch) throw Error(SDH_E_INVALID, "batch larger than max_batch");
  if (b->n >= INT32_MAX) throw Error(SDH_E_INVALID, "a chunk of 2^31 events or more");
  if (b->n > 0) check_fan_strings(e, stream);
  HIPCHK(hipSetDevice(e->dev));
  int64_t t01[2];
  if (b->on_device) {
    d2h_sync(e, &t01[0], b->ts, 8);
    d2h_sync(e, &t01[1], b->ts + (b->n - 1), 8);
  } else {
    t01[0] = b->ts[0];
    t01[1] = b->ts[b->n - 1];
  }
  chunk_begin(e, stream, b);
  // InputHandler.send(Event[]):77-85: time moves once, to the last timestamp, before the chunk
  if (!e->started) {
    e->started = true;
    e->start_ts = t01[0];
  }
  time_advance(e, t01[1]);
  e->ck.active = true;
  e->mt.chunk_pushed = true;
  e->ck.first_seq = e->seq;
  e->ck.n = b->n;
  e->ck.stream = stream;
  try {
    do_push(e, stream, b);
  } catch (...) {
    e->ck.active = false;
    throw;
  }
  e->ck.active = false;
  return SDH_OK;
}

thread_local std::string g_create_error;

}  // namespace

// ---- snapshot section (engine_snap.hip): the event store (do_retain, store_append) ----
// cap, row words, the first retained seq, then the retained rows in seq order
void sdh::eng::snap_save_events(sdh_engine* e, snap::Writer& w) {
  const int64_t lo = std::max(e->ev_first, e->seq - e->ev_cap), n = e->seq - lo;
  w.put(e->ev_cap);
  w.put(e->ev_w);
  w.put(lo);
  // (the ring holds them in at most two runs: up to its end, then from its start)
  const int64_t r0 = lo & (e->ev_cap - 1), n0 = std::min(n, e->ev_cap - r0);
  put_dev(w, e->ev_rows.p + r0 * e->ev_w, (size_t)n0 * e->ev_w * 8);
  put_dev(w, e->ev_rows.p, (size_t)(n - n0) * e->ev_w * 8);
}

// a retaining engine takes the snapshot's retained rows (those that fit its ring); a snapshot without
// them (`stored` false: version 8), or an engine that keeps no events, leaves the store empty
void sdh::eng::snap_load_events(sdh_engine* e, snap::Reader& r, bool stored) {
  e->ev_first = e->seq;
  if (!stored) return;
  const int64_t scap = r.get(), sw = r.get(), lo = r.get();
  const int64_t n = e->seq - lo;
  snap::need(scap >= 1 && sw >= 2 && sw <= 2 + MAXATTR && lo >= 0 && n >= 0 && n <= scap &&
                 (size_t)n * (size_t)sw <= r.left(), "bad snapshot event store");
  if (!e->ev_cap) {
    r.skip((size_t)(n * sw));
    return;
  }
  snap::need(sw == e->ev_w, "snapshot of a different program");
  const int64_t keep = std::min(n, e->ev_cap), first = e->seq - keep;
  r.skip((size_t)((n - keep) * sw));
  const int64_t r0 = first & (e->ev_cap - 1), n0 = std::min(keep, e->ev_cap - r0);
  get_dev(r, e->ev_rows.p + r0 * e->ev_w, (size_t)n0 * sw * 8);
  get_dev(r, e->ev_rows.p, (size_t)(keep - n0) * sw * 8);
  e->ev_first = first;
}

extern "C" {

const char* sdh_version(void) { return "libsiddhi_hip 0.2 (gfx950: K_ratchet, K_chain, K_gen, K_seq; device R18 poll)"; }

int sdh_engine_create(const void* ir, size_t len, const sdh_config* cfg, sdh_engine** out) {
  if (!out) return SDH_E_INVALID;
  *out = nullptr;
  sdh_engine* e = new sdh_engine;
  int rc = guard(e, [&]() {
    if (cfg) e->cfg = *cfg;
    // sdh_config.debug: "NAME=VALUE;..." knobs (knobs.h), copied: the caller's string need not outlive
    // the call
    if (e->cfg.debug) {
      const std::string d(e->cfg.debug);
      size_t i = 0;
      while (i < d.size()) {
        size_t j = d.find(';', i);
        if (j == std::string::npos) j = d.size();
        const std::string kv = d.substr(i, j - i);
        const size_t eq = kv.find('=');
        if (!kv.empty()) e->knobs.emplace_back(kv.substr(0, eq), eq == std::string::npos ? "1" : kv.substr(eq + 1));
        i = j + 1;
      }
      e->cfg.debug = nullptr;
    }
    if (e->cfg.shard_world <= 0) e->cfg.shard_world = 1;
    e->dev = e->cfg.device;
    // the program is validated before any device call (a malformed blob is SDH_E_INVALID with or
    // without a GPU)
    e->prog = read_ir(ir, len);
    try {
      e->lp = kg::read_program(ir, len);
    } catch (const kg::LowerError& ex) {
      throw Error(SDH_E_INVALID, ex.what());
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      (void)hipGetLastError();
      throw Error(SDH_E_DEVICE, "no HIP device (the engine has no CPU fallback)");
    }
    if (e->dev < 0 || e->dev >= ndev) throw Error(SDH_E_INVALID, fmt("device %d of %d", e->dev, ndev));
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, e->dev));
    // tuning overrides for kernel experiments: K_ratchet LDS ring depth and waves per launch
    if (const char* v = sdh::knob("SDH_RATCHET_ML")) e->rML = std::max(4, atoi(v));
    if (const char* v = sdh::knob("SDH_RATCHET_WAVES")) e->r_waves = atof(v);
    if (const char* v = sdh::knob("SDH_XCD")) e->xcd = atoi(v) != 0;
    if (const char* v = sdh::knob("SDH_SLAB_LDS_SMALL")) e->slab_lds_small = std::max(64, atoi(v));
    e->out_rank = kg::output_ranks(e->lp);
    // plan selection per query: K_ratchet (2-state threshold ratchet) > K_chain (stream-state
    // chains) > K_gen (everything else: count, logical, sequences, partitions, general predicates)
    std::vector<std::pair<RatchetPlan, int>> rplans;
    std::vector<int> gen_qs;
    const bool no_ratchet = (e->cfg.flags & SDH_FLAG_NO_RATCHET) != 0;
    const bool force_gen = (e->cfg.flags & SDH_FLAG_FORCE_GEN) != 0;
    for (int qi = 0; qi < (int)e->prog.q.size(); ++qi) {
      // multi-GPU: unpartitioned queries are sharded by pattern set (query q on rank
      // q % world); a partition's queries run on every rank, each rank owning the keys that
      // key_shard maps to it (nfa_gen.hip: foreign keys' events are dropped at routing)
      if (e->lp.q[qi].partition < 0 && qi % e->cfg.shard_world != e->cfg.shard_rank) continue;
      Lowered L = force_gen ? Lowered() : lower_chain(e->prog, qi);
      if (!L.ok) {
        gen_qs.push_back(qi);
        continue;
      }
      RatchetPlan rp = no_ratchet ? RatchetPlan() : ratchet_plan(L.cq);
      if (rp.ok) rplans.push_back({rp, qi});
      else e->lq.push_back(L);
    }
    // K_chain tables: a capacity the caller chose is fixed (SDH_E_CAPACITY lies past it); 0 starts at
    // 128 partials per query and grows on overflow (chain_grow), past 512 in the paged form
    int want = e->cfg.partials_per_inst > 0 ? e->cfg.partials_per_inst : 128;
    e->K = want <= 64 ? 1 : want <= 128 ? 2 : want <= 256 ? 4 : 8;
    e->pcap = 64 * e->K;
    e->chain_growing = e->cfg.partials_per_inst <= 0;
    if (const char* v = sdh::knob("SDH_CHAIN_PAGED")) e->chain_force_paged = atoi(v) != 0;
    e->chain_paged = e->chain_force_paged;
    int maxS = rplans.empty() ? 1 : 2;
    for (auto& L : e->lq) maxS = std::max(maxS, L.cq.n_states);
    e->rec_words = 2 + maxS;
    e->prev_ts.assign(e->prog.stream_types.size(), INT64_MIN);
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&e->h2d, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&e->ev0));
    HIPCHK(hipEventCreate(&e->ev1));
    HIPCHK(hipEventCreate(&e->ev_h0));
    HIPCHK(hipEventCreate(&e->ev_h1));
    for (auto& ev : e->ev_stage) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e->d_q.ensure(std::max<size_t>(1, e->lq.size()));
    // the queries' residual programs in one device table: each query's ranges rebased into it
    std::vector<ChainQuery> cqs;
    std::vector<kg::GInsn> rcode;
    for (auto& L : e->lq) {
      const int base = (int)rcode.size();
      for (int s = 0; s < MAXS; ++s) {
        L.cq.rt_b[s] += base; L.cq.rt_e[s] += base;
        L.cq.rp_b[s] += base; L.cq.rp_e[s] += base;
      }
      rcode.insert(rcode.end(), L.rcode.begin(), L.rcode.end());
      cqs.push_back(L.cq);
    }
    e->chain_resid = !rcode.empty();
    e->chain_paged = e->chain_force_paged || e->pcap > chain_reg_limit(e);
    e->d_rcode.ensure(std::max<size_t>(1, rcode.size()));
    if (!rcode.empty())
      HIPCHK(hipMemcpy(e->d_rcode.p, rcode.data(), rcode.size() * sizeof(kg::GInsn), hipMemcpyHostToDevice));
    if (!cqs.empty())
      HIPCHK(hipMemcpy(e->d_q.p, cqs.data(), cqs.size() * sizeof(ChainQuery), hipMemcpyHostToDevice));
    ensure_state(e);
    ratchet_build(e, rplans);
    gen_build(e, gen_qs);
    // R18 tables of the device match table: receiver rank per (query, stream), and per query its
    // state count and the stream of its last state (the trigger of a chain-plan match)
    const size_t nq_all = e->prog.q.size();
    if (nq_all >= ((size_t)1 << RANK_BITS)) throw Error(SDH_E_UNSUPPORTED, "more than 2^20 queries");
    // device ranks are out_rank + 1: rank 0 orders the absent states' timer matches before the
    // triggering event's own
    e->d_out_rank.ensure(std::max<size_t>(1, e->out_rank.size()));
    e->d_fan_rank.ensure(std::max<size_t>(1, e->out_rank.size()));
    if (!e->out_rank.empty()) {
      std::vector<int32_t> r1(e->out_rank.size()), fr(e->out_rank.size(), -1);
      for (size_t k = 0; k < r1.size(); ++k) r1[k] = e->out_rank[k] + 1;
      // fan-out (query, stream): the partition's first rank for that stream, and the query's rank
      // within it as a tiebreak below the key's junction-map position (the key-major order of
      // PartitionStreamReceiver.send(ComplexEvent))
      const size_t ns = e->prog.stream_types.size();
      for (const auto& pd : e->lp.parts)
        for (const auto& f : pd.fanout) {
          int base = INT32_MAX;
          for (int pq : pd.queries) base = std::min(base, e->out_rank[(size_t)pq * ns + f.stream]);
          for (int pq : pd.queries) {
            fr[(size_t)pq * ns + f.stream] = e->out_rank[(size_t)pq * ns + f.stream] - base;
            r1[(size_t)pq * ns + f.stream] = base + 1;
          }
        }
      HIPCHK(hipMemcpy(e->d_out_rank.p, r1.data(), r1.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->d_fan_rank.p, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
      // chunk delivery (matches.hip chunk_keys_kernel): a query's junction subscriber rank (+1) --
      // its partition's first rank on the stream -- and its rank inside the partition
      e->ck_major = r1;
      e->ck_minor.assign(r1.size(), 0);
      for (const auto& pd : e->lp.parts)
        for (size_t st = 0; st < ns; ++st) {
          int base = INT32_MAX;
          for (int pq : pd.queries) base = std::min(base, e->out_rank[(size_t)pq * ns + st]);
          for (int pq : pd.queries) {
            e->ck_major[(size_t)pq * ns + st] = base + 1;
            e->ck_minor[(size_t)pq * ns + st] = e->out_rank[(size_t)pq * ns + st] - base;
          }
        }
      e->d_ck_major.ensure(r1.size());
      e->d_ck_minor.ensure(r1.size());
      HIPCHK(hipMemcpy(e->d_ck_major.p, e->ck_major.data(), r1.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->d_ck_minor.p, e->ck_minor.data(), r1.size() * 4, hipMemcpyHostToDevice));
    }
    // direct placement cells: a stream qualifies when its K_ratchet groups, each in lane order, are
    // consecutive runs of its K_ratchet queries in receiver-rank order (a placed push has no other
    // producer); cell = the group's run position
    {
      const size_t ns = e->prog.stream_types.size();
      e->place_cells.assign(ns, 0);
      for (auto& g : e->rg) g.cell = -1;
      for (size_t st = 0; st < ns; ++st) {
        std::vector<int> gs;
        bool gated = false;  // (K_gate writes records, not placed rows)
        for (int g = 0; g < (int)e->rg.size(); ++g)
          if (e->rg[g].stream == (int)st && e->rg[g].n_lanes > 0) {
            gs.push_back(g);
            gated |= e->rg[g].n_g > 0;
          }
        if (gs.empty() || gated) continue;
        auto rk = [&](int g, int l) { return e->out_rank[(size_t)e->rg[g].qid[l] * ns + st]; };
        std::sort(gs.begin(), gs.end(), [&](int a, int b) { return rk(a, 0) < rk(b, 0); });
        std::vector<int> ranks;
        for (int g : gs)
          for (int l = 0; l < e->rg[g].n_lanes; ++l) ranks.push_back(rk(g, l));
        bool ok = true;
        for (size_t k = 1; k < ranks.size(); ++k) ok = ok && ranks[k - 1] < ranks[k];
        if (!ok) continue;
        for (size_t c = 0; c < gs.size(); ++c) e->rg[gs[c]].cell = (int)c;
        e->place_cells[st] = (int)gs.size();
      }
      if (!e->rg.empty())
        HIPCHK(hipMemcpy(e->d_rg.p, e->rg.data(), e->rg.size() * sizeof(RatchetGroup), hipMemcpyHostToDevice));
    }
    std::vector<int32_t> qinfo(std::max<size_t>(1, 2 * nq_all), 0);
    for (size_t q = 0; q < nq_all; ++q) {
      qinfo[2 * q] = (int32_t)e->prog.q[q].st.size();
      qinfo[2 * q + 1] = e->prog.q[q].st.empty() ? 0 : e->prog.q[q].st.back().stream;
    }
    e->d_qinfo.ensure(qinfo.size());
    HIPCHK(hipMemcpy(e->d_qinfo.p, qinfo.data(), qinfo.size() * 4, hipMemcpyHostToDevice));
    for (size_t q = 0; q < nq_all; ++q) e->cw = std::max(e->cw, 2 + qinfo[2 * q]);
    return SDH_OK;
  });
  if (rc != SDH_OK) {
    g_create_error = e->err;
    delete e;
    return rc;
  }
  *out = e;
  return SDH_OK;
}

int sdh_engine_push(sdh_engine* e, int32_t stream, const sdh_batch* b) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    if (b && b->chunk && b->n > 1) return push_chunk(e, stream, b);
    return do_push(e, stream, b);
  });
}

int sdh_engine_push_mixed(sdh_engine* e, int32_t n_parts, const sdh_mixed_part* parts, const int32_t* order,
                          int64_t n_order, int32_t order_on_device) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    return do_push_mixed(e, n_parts, parts, order, n_order, order_on_device);
  });
}

int sdh_engine_reserve(sdh_engine* e, int64_t bytes) {
  if (!e || bytes < 0) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    HIPCHK(hipSetDevice(e->dev));
    if (e->ssets.empty() || bytes == 0) return SDH_OK;
    const size_t per = (size_t)bytes / e->ssets.size();
    for (auto& ss : e->ssets)
      if (ss->arena_bytes < per && !ss->add_chunk(((per - ss->arena_bytes) + 4095) & ~(size_t)4095))
        throw Error(SDH_E_CAPACITY, fmt("device memory exhausted reserving %.1f GB for the sparse state", bytes / 1e9));
    return SDH_OK;
  });
}

int sdh_engine_reserve_keys(sdh_engine* e, int64_t keys) {
  if (!e || keys < 0) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    HIPCHK(hipSetDevice(e->dev));
    if (keys == 0) return SDH_OK;
    for (auto& r : e->routes)
      if (r && keys > r->max_keys)
        throw Error(SDH_E_INVALID, fmt("reserve_keys(%lld) beyond gen_max_keys (%lld)", (long long)keys,
                                       (long long)r->max_keys));
    // the same growth calls a push makes when its batch brings new keys (a prefix copy of held state)
    for (auto& gs : e->gsets)
      if (gs->partition >= 0 && gs->n_groups > 0) gen_grow(e, *gs, keys);
    for (auto& ps : e->psets) part_grow(e, *ps, keys);
    for (auto& ss : e->ssets) slab_grow_keys(e, *ss, keys);
    return SDH_OK;
  });
}

int sdh_engine_poll_compact_ex(sdh_engine* e, int32_t device, sdh_matches_compact_ex* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() { return do_poll_compact_ex(e, out, device != 0); });
}

int sdh_engine_set_comm(sdh_engine* e, sdh_comm* c) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    if (c && xch::device(c) != e->dev)
      throw Error(SDH_E_INVALID, fmt("communicator on device %d, engine on device %d", xch::device(c), e->dev));
    e->comm = c;
    return SDH_OK;
  });
}

int sdh_engine_push_bcast(sdh_engine* e, int32_t stream, const sdh_batch* b, int32_t root) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    return do_push_bcast(e, stream, b, root);
  });
}

int sdh_engine_gather(sdh_engine* e, int32_t device, sdh_matches* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    return do_gather(e, out, device == 0);
  });
}

int sdh_engine_flush(sdh_engine* e) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    HIPCHK(hipStreamSynchronize(e->stream));
    return SDH_OK;
  });
}

int sdh_engine_start(sdh_engine* e, int64_t t) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    if (e->started) throw Error(SDH_E_INVALID, "the engine has already started");
    e->started = true;
    e->start_ts = t;
    return SDH_OK;
  });
}

// Time passes to t with no event: every absent state's scheduler fires what falls due (the timer
// thread of a live runtime, Scheduler.java:258-287). Its matches join the device table like a
// push's, ordered by (timer time, query, fire order) before the next event's.
int sdh_engine_advance_time(sdh_engine* e, int64_t t) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    if (!e->started) {
      e->started = true;
      e->start_ts = t;
    }
    time_advance(e, t);
    return SDH_OK;
  });
}

int sdh_engine_pending_matches(sdh_engine* e, int64_t* n) {
  if (!e || !n) return SDH_E_INVALID;
  *n = e->mt.n + ((e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) && !e->dev_polled
                       ? e->device_matches + e->r_matches + e->g_dev_matches : 0);
  return SDH_OK;
}

int sdh_engine_poll(sdh_engine* e, sdh_matches* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() { return do_poll(e, out, true); });
}

int sdh_engine_poll_device(sdh_engine* e, sdh_matches* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() { return do_poll(e, out, false); });
}

int sdh_engine_poll_compact(sdh_engine* e, int32_t device, sdh_matches_compact* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() { return do_poll_compact(e, out, device != 0); });
}

int sdh_engine_retain_events(sdh_engine* e, int64_t events) {
  if (!e || events <= 0) return SDH_E_INVALID;
  return guard(e, [&]() { return do_retain(e, events); });
}

int sdh_engine_poll_rows(sdh_engine* e, int32_t device, sdh_rows* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() { return do_poll_rows(e, out, device != 0); });
}

int sdh_engine_query_outputs(sdh_engine* e, int32_t query, int32_t* n_out, int32_t* types, int32_t cap) {
  if (!e || !n_out || cap < 0) return SDH_E_INVALID;
  return guard(e, [&]() {
    sel_lower(e);
    if (query < 0 || (size_t)query >= e->selp.types.size()) throw Error(SDH_E_INVALID, "no such query");
    const size_t no = e->lp.q[(size_t)query].outs.size();
    *n_out = (int32_t)no;
    const auto& ty = e->selp.types[(size_t)query];
    for (size_t c = 0; types && c < ty.size() && c < (size_t)cap; ++c) types[c] = ty[c];
    return SDH_OK;
  });
}

// keys a partition has seen so far (its routing table's dense ids)
int64_t route_keys(sdh_engine* e, int partition) {
  if (partition < 0 || partition >= (int)e->routes.size() || !e->routes[partition]) return 0;
  int32_t nk = 0;
  d2h_sync(e, &nk, e->routes[partition]->n_keys.p, 4);
  return nk;
}

// Live partials of K_gen arenas, K_part tables and K_seq windows: entries of the pending lists of
// non-start states (oracle_live_partials counts every pending list, the start state's seed included)
int64_t device_live_partials(sdh_engine* e) {
  DevBuf<unsigned long long> acc;
  acc.ensure(1);
  HIPCHK(hipMemsetAsync(acc.p, 0, 8, e->stream));
  DevBuf<int32_t> d_gseq;
  if (!e->group_seq.empty()) {
    d_gseq.ensure(e->group_seq.size());
    HIPCHK(hipMemcpy(d_gseq.p, e->group_seq.data(), e->group_seq.size() * 4, hipMemcpyHostToDevice));
  }
  for (auto& up : e->gsets) {
    auto& gs = *up;
    if (!gs.a32.p || gs.n_groups == 0) continue;
    const int64_t blocks = gs.partition < 0 ? gs.n_groups : std::min(gs.key_cap, route_keys(e, gs.partition)) * gs.n_groups;
    HIPCHK(sdh_live_gen(gs.a32.p, e->gB32, blocks, gs.n_groups, gs.group_base, e->d_lane_q.p, d_gseq.p, e->d_gq.p, acc.p,
                        e->stream));
  }
  for (auto& up : e->psets) {
    auto& ps = *up;
    if (!ps.st.p || ps.key_cap == 0) continue;
    const int64_t nk = std::min(ps.key_cap, route_keys(e, ps.partition));
    HIPCHK(sdh_live_part(ps.st.p, ps.cur.p, nk, ps.n_groups, ps.key_cap * ps.n_groups, ps.bw(), acc.p, e->stream));
  }
  for (int s = 0; s < (int)e->seq_tail.size(); ++s) {
    std::vector<int32_t> gl;
    for (int g = 0; g < (int)e->group_seq.size(); ++g)
      if (e->group_seq[g] > 0 && e->gq[e->group_tmpl[g]].st[0].stream == s) gl.push_back(g);
    if (gl.empty() || e->seq_tail_len[s] <= 0) continue;
    DevBuf<int32_t> d_gl;
    d_gl.ensure(gl.size());
    HIPCHK(hipMemcpy(d_gl.p, gl.data(), gl.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(sdh_live_seq(e->seq_tail[s].p, e->seq_tail_len[s], s, d_gl.p, (int)gl.size(), e->d_lane_q.p,
                        e->d_group_tmpl.p, e->d_gq.p, acc.p, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // (d_gl is freed at scope end)
  }
  unsigned long long v = 0;
  d2h_sync(e, &v, acc.p, 8);
  return (int64_t)v;
}

// Test diagnostic: (records, order-independent hash) of the last push's K_ratchet records as the
// kernel wrote them, in either output mode (matches.hip digest_ratchet_kernel)
int sdh_engine_debug_digest(sdh_engine* e, uint64_t* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() {
    out[0] = out[1] = 0;
    DevBuf<unsigned long long> acc;
    acc.ensure(2);
    HIPCHK(hipMemsetAsync(acc.p, 0, 16, e->stream));
    if (e->r_placing)  // the last push placed its matches: its compact rows
      HIPCHK(sdh_digest_compact(e->pc_rows.p, e->cw, e->r_place_row0, e->r_matches, e->seq_ref, acc.p, e->stream));
    else
      HIPCHK(sdh_digest_ratchet(e->d_rmatch.p, e->r_blk_recs, e->r_wide, e->d_blk_count.p, e->d_blk_group.p,
                                e->d_blk_side.p, e->d_rg.p, e->r_seq_base, (int)e->r_blk_taken, acc.p, e->stream));
    d2h_sync(e, out, acc.p, 16);
    return SDH_OK;
  });
}

// Test diagnostic: pushes so far whose K_ratchet records the shared-pops form wrote
int sdh_engine_debug_shared_pushes(sdh_engine* e, int64_t* out) {
  if (!e || !out) return SDH_E_INVALID;
  *out = e->r_shared_pushes;
  return SDH_OK;
}

// Test diagnostic: sdh_engine_push_mixed calls so far run natively / split into run pushes
int sdh_engine_debug_mixed_pushes(sdh_engine* e, int64_t* out) {
  if (!e || !out) return SDH_E_INVALID;
  out[0] = e->mixed_native;
  out[1] = e->mixed_split;
  return SDH_OK;
}

// The last push's device records (SDH_FLAG_DEVICE_MATCHES; formats: include/siddhi_hip.h sdh_records)
int sdh_engine_poll_records(sdh_engine* e, sdh_records* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    *out = sdh_records{};
    if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES))
      throw Error(SDH_E_INVALID, "sdh_engine_poll_records needs SDH_FLAG_DEVICE_MATCHES (use sdh_engine_poll)");
    out->seq_base = e->last_seq_base;
    out->n_events = e->last_n;
    if (e->r_blocks_used > 0 && !e->r_placing) {
      if (e->d_rlane_q.n < e->rg.size() * WAVE) {
        std::vector<int32_t> lq(e->rg.size() * WAVE, -1);
        for (size_t g = 0; g < e->rg.size(); ++g)
          for (int l = 0; l < e->rg[g].n_lanes; ++l) lq[g * WAVE + l] = e->rg[g].qid[l];
        e->d_rlane_q.ensure(lq.size());
        HIPCHK(hipMemcpy(e->d_rlane_q.p, lq.data(), lq.size() * 4, hipMemcpyHostToDevice));
      }
      out->r_n = e->r_matches;
      out->r_blocks = e->r_blocks_used;
      out->r_bytes = (int64_t)e->r_rec_bytes;
      out->r_base = e->d_rmatch.p;
      out->r_count = e->d_blk_count.p;
      out->r_side = e->d_blk_side.p;
      out->r_group = e->d_blk_group.p;
      out->r_lane_query = e->d_rlane_q.p;
      out->r_format = e->r_rec4 ? SDH_REC_4 : e->r_wide ? SDH_REC_16 : SDH_REC_8;
      out->r_blk_bytes = e->r_blk_recs * 8 * (e->r_wide ? 2 : 1);
    }
    if (e->g_dev_matches > 0) {
      upload_qkeys(e);
      out->f_n = e->g_dev_matches;
      out->f_words = e->g_used;
      out->f_base = e->g_out.p;
      out->f_query_keys = e->d_qkeys.p;
    }
    if (e->device_matches > 0) {
      const int64_t ni = (int64_t)e->work.size();
      std::vector<int64_t> so(ni);
      for (int64_t i = 0; i < ni; ++i) so[i] = e->work[i].seg_off;
      e->d_seg_off.ensure(ni);
      HIPCHK(hipMemcpy(e->d_seg_off.p, so.data(), ni * 8, hipMemcpyHostToDevice));
      out->c_n = e->device_matches;
      out->c_items = ni;
      out->c_words = e->rec_words;
      out->c_base = e->d_match.p;
      out->c_off = e->d_seg_off.p;
      out->c_count = e->d_seg_count.p;
    }
    out->n = out->r_n + out->f_n + out->c_n;
    e->dev_polled = true;
    return SDH_OK;
  });
}

int sdh_engine_records_compact(sdh_engine* e, int32_t* rows, int64_t cap, int32_t width, int64_t* n) {
  if (!e || !n || width < 4) return SDH_E_INVALID;
  return guard(e, [&]() {
    check_usable(e);
    *n = 0;
    if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES))
      throw Error(SDH_E_INVALID, "sdh_engine_records_compact needs SDH_FLAG_DEVICE_MATCHES");
    const int nb = e->r_placing ? 0 : e->r_blocks_used;
    if (nb <= 0) return SDH_OK;
    *n = e->r_matches;
    if (!rows) return SDH_OK;
    if (cap < e->r_matches) throw Error(SDH_E_CAPACITY, fmt("%lld rows need room for %lld", (long long)cap, (long long)e->r_matches));
    e->d_rrow_off.ensure((size_t)nb + 1);
    e->d_rrow_tmp.ensure(sdh_ratchet_compact_temp(nb));
    HIPCHK(sdh_ratchet_compact(e->d_rmatch.p, e->r_blk_recs, e->r_wide, e->d_blk_count.p, e->d_blk_group.p,
                               e->d_blk_side.p, e->d_rg.p, e->r_seq_base, nb, e->d_rrow_off.p, e->d_rrow_tmp.p,
                               e->d_rrow_tmp.n, width, rows, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SDH_OK;
  });
}

// sdh_engine_records_rows: rows [first, first + max_rows) of the last push's device records, in record
// order (rec_rows.h), each projected through its query's select list. Nothing is consumed: the records
// stay as they are, and what locates a row in them (the blocks' row offsets, the flat records' heads, the
// segments' first rows) is made once per push and kept until the next.
static int do_records_rows(sdh_engine* e, int64_t first, int64_t max_rows, bool device, sdh_rows* out, int64_t* total) {
  check_usable(e);
  if (!(e->cfg.flags & SDH_FLAG_DEVICE_MATCHES))
    throw Error(SDH_E_INVALID, "sdh_engine_records_rows needs SDH_FLAG_DEVICE_MATCHES (use sdh_engine_poll_rows)");
  if (!e->ev_cap) throw Error(SDH_E_INVALID, "sdh_engine_records_rows: no events are kept (sdh_engine_retain_events)");
  if (first < 0 || max_rows < 0) throw Error(SDH_E_INVALID, "sdh_engine_records_rows: a negative window");
  const auto& S = e->selp;
  if (S.over >= 0)
    throw Error(SDH_E_UNSUPPORTED, fmt("query %d selects more than %d outputs", S.over, sel::MAXOUT));
  if (S.bad) throw Error(SDH_E_INVALID, "a select list names a slot or an attribute its query lacks, or holds an unknown opcode");
  if (S.max_depth > kg::GSTACK - 1)
    throw Error(SDH_E_UNSUPPORTED, "a select expression is too deep for the device evaluation stack");
  HIPCHK(hipSetDevice(e->dev));
  const int nb = e->r_placing ? 0 : e->r_blocks_used;
  const rr::Parts P{{nb > 0 ? e->r_matches : 0, e->g_dev_matches, e->device_matches}};
  const int64_t all = P.total();
  const int64_t n = std::max<int64_t>(0, std::min(all - first, max_rows));
  const int width = S.width;
  const size_t cw = (size_t)std::max(1, width);
  if (n) {
    try {
      e->rr_q.ensure((size_t)n);
      e->rr_ts.ensure((size_t)n);
      e->rr_seq.ensure((size_t)n);
      e->rr_nulls.ensure((size_t)n);
      e->rr_cells.ensure((size_t)n * cw);
      if (!device) {
        e->hrr_q.ensure((size_t)n);
        e->hrr_ts.ensure((size_t)n);
        e->hrr_seq.ensure((size_t)n);
        e->hrr_nulls.ensure((size_t)n);
        e->hrr_cells.ensure((size_t)n * cw);
      }
    } catch (const Error& ex) {
      if (ex.code != SDH_E_DEVICE) throw;
      (void)hipGetLastError();
      throw Error(SDH_E_CAPACITY, fmt("no device memory for a window of %lld rows: ask for fewer (max_rows)", (long long)n));
    }
    e->pr_err.ensure(1);
    const sel::Tables T{e->d_sel_code.p, e->d_sel_outs.p, e->d_sel_shapes.p, e->d_sel_queries.p, e->d_sel_consts.p};
    const sel::Store st{e->ev_rows.p, e->ev_cap - 1, std::max(e->ev_first, e->seq - e->ev_cap), e->ev_w, 0};
    const int deep = S.max_depth > kg::RSTACK;
    const int search = sdh::knob("SDH_RR_SEARCH") ? 1 : 0;
    HIPCHK(hipMemsetAsync(e->pr_err.p, 0, 4, e->stream));
    for (int p = 0; p < 3; ++p) {
      RecRows R{};
      R.n = rr::part_window(P, p, first, n, R.first);
      if (R.n <= 0) continue;
      R.out0 = P.first(p) + R.first - first;
      if (p == 0) {
        if (!(e->rr_ready & 1)) {  // the blocks' first rows (as sdh_engine_records_compact)
          e->d_rrow_off.ensure((size_t)nb + 1);
          e->d_rrow_tmp.ensure(sdh_ratchet_compact_temp(nb));
          HIPCHK(sdh_ratchet_compact(e->d_rmatch.p, e->r_blk_recs, e->r_wide, e->d_blk_count.p, e->d_blk_group.p,
                                     e->d_blk_side.p, e->d_rg.p, e->r_seq_base, nb, e->d_rrow_off.p, e->d_rrow_tmp.p,
                                     e->d_rrow_tmp.n, 4, nullptr, e->stream));
          e->rr_ready |= 1;
        }
        R.seq_base = e->r_seq_base;
        R.match = e->d_rmatch.p;
        R.blk_recs = e->r_blk_recs;
        R.wide = e->r_wide;
        R.blk_count = e->d_blk_count.p;
        R.blk_group = e->d_blk_group.p;
        R.blk_side = e->d_blk_side.p;
        R.groups = e->d_rg.p;
        R.row_off = e->d_rrow_off.p;
        R.nb = nb;
      } else if (p == 1) {
        if (!(e->rr_ready & 2)) {  // the records' heads: one walk of the buffer per push
          e->rr_rec_off.ensure((size_t)P.n[1]);
          e->rr_heads.ensure(1);
          e->rr_tmp.ensure(sdh_flat_heads_temp(e->g_used));
          HIPCHK(sdh_flat_heads(e->g_out.p, e->g_used, e->rr_tmp.p, e->rr_rec_off.p, P.n[1], e->rr_heads.p, e->stream));
          unsigned long long heads = 0;
          d2h_sync(e, &heads, e->rr_heads.p, 8);
          if ((int64_t)heads != P.n[1])
            throw Error(SDH_E_DEVICE, fmt("the flat records hold %llu heads, the push counted %lld", heads, (long long)P.n[1]));
          e->rr_ready |= 2;
        }
        R.seq_base = e->last_seq_base;
        R.flat = e->g_out.p;
        R.rec_off = e->rr_rec_off.p;
      } else {
        const int64_t ni = (int64_t)e->work.size();
        if (!(e->rr_ready & 4)) {  // the segments' first rows
          std::vector<int64_t> so((size_t)ni), row((size_t)ni + 1, 0);
          if (ni) d2h_sync(e, row.data() + 1, e->d_seg_count.p, (size_t)ni * 8);
          for (int64_t i = 0; i < ni; ++i) {
            so[(size_t)i] = e->work[(size_t)i].seg_off;
            row[(size_t)i + 1] += row[(size_t)i];
          }
          if (row[(size_t)ni] != P.n[2])
            throw Error(SDH_E_DEVICE, fmt("the K_chain segments hold %lld records, the push counted %lld",
                                          (long long)row[(size_t)ni], (long long)P.n[2]));
          upload(e->rr_seg_off, so);
          upload(e->rr_seg_row, row);
          e->rr_ready |= 4;
        }
        R.seq_base = e->last_seq_base;
        R.chain = e->d_match.p;
        R.seg_off = e->rr_seg_off.p;
        R.seg_row = e->rr_seg_row.p;
        R.items = ni;
        R.rec_words = e->rec_words;
        R.qinfo = e->d_qinfo.p;
      }
      HIPCHK(sdh_select_records(&T, &st, deep, p, search, &R, n, width, e->rr_q.p, e->rr_ts.p, e->rr_seq.p,
                                e->rr_cells.p, e->rr_nulls.p, e->pr_err.p, e->stream));
    }
    int32_t bad = 0;
    d2h_sync(e, &bad, e->pr_err.p, 4);
    if (bad)
      throw Error(SDH_E_CAPACITY, fmt("a record reads an event that has left the event store of %lld events: raise "
                                      "sdh_engine_retain_events before the push",
                                      (long long)e->ev_cap));
    if (!device) {
      HIPCHK(hipMemcpyAsync(e->hrr_q.p, e->rr_q.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->hrr_ts.p, e->rr_ts.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->hrr_seq.p, e->rr_seq.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(e->hrr_nulls.p, e->rr_nulls.p, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
      if (width)
        HIPCHK(hipMemcpyAsync(e->hrr_cells.p, e->rr_cells.p, (size_t)n * width * 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
    }
  }
  *total = all;
  *out = sdh_rows{};
  out->n = n;
  out->width = width;
  if (n) {
    out->query = device ? e->rr_q.p : e->hrr_q.p;
    out->ts = device ? e->rr_ts.p : e->hrr_ts.p;
    out->seq = device ? e->rr_seq.p : e->hrr_seq.p;
    out->cells = device ? e->rr_cells.p : e->hrr_cells.p;
    out->nulls = device ? e->rr_nulls.p : e->hrr_nulls.p;
  }
  return SDH_OK;
}

int sdh_engine_records_rows(sdh_engine* e, int64_t first, int64_t max_rows, int32_t device, sdh_rows* out,
                            int64_t* total) {
  if (!e || !out || !total) return SDH_E_INVALID;
  return guard(e, [&]() { return do_records_rows(e, first, max_rows, device != 0, out, total); });
}

int sdh_engine_push_stats(sdh_engine* e, double* last_kernel_ms, double* last_kernel_bytes) {
  if (!e || !last_kernel_ms || !last_kernel_bytes) return SDH_E_INVALID;
  *last_kernel_ms = e->stats.last_kernel_ms;  // (host-side values: no device work, no sync)
  *last_kernel_bytes = e->stats.last_kernel_bytes;
  return SDH_OK;
}

int sdh_engine_stats(sdh_engine* e, sdh_stats* out) {
  if (!e || !out) return SDH_E_INVALID;
  return guard(e, [&]() {
    const size_t nq = e->lq.size();
    std::vector<InstHeader> h[2];
    int64_t live = 0;
    for (int b = 0; b < 2 && nq; ++b) {
      h[b].resize(nq);
      d2h_sync(e, h[b].data(), e->d_hdr[b].p, nq * sizeof(InstHeader));
    }
    for (size_t q = 0; q < nq; ++q) live += h[e->cur[q]][q].n_live;
    const size_t ng = e->rg.size();
    for (int b = 0; b < 2 && ng; ++b) {
      std::vector<RatchetState> rs(ng);
      d2h_sync(e, rs.data(), e->d_rst[b].p, ng * sizeof(RatchetState));
      for (size_t g = 0; g < ng; ++g)
        if (e->rcur[g] == b)
          for (int l = 0; l < e->rg[g].n_lanes; ++l) live += rs[g].n[l];
    }
    for (auto& ss : e->ssets) live += slab_live_partials(e, *ss);
    live += device_live_partials(e);
    live += wave_live_partials(e);
    e->stats.live_partials = live;
    e->stats.pool_regrows = e->gen_regrows + e->chain_regrows + e->part_regrows + e->wave_regrows;
    e->stats.last_slab_items = e->slab_items;
    // queries per plan: K_ratchet, K_gate, K_chain, K_part, K_slab, K_seq, K_gen, K_wave
    for (auto& c : e->stats.plan_queries) c = 0;
    for (const auto& g : e->rg) e->stats.plan_queries[g.n_g ? 1 : 0] += g.n_lanes;
    e->stats.plan_queries[2] = (int64_t)e->lq.size();
    auto lanes = [&](int g) {
      int64_t c = 0;
      for (int l = 0; l < WAVE; ++l) c += e->lane_q[(size_t)g * WAVE + l] >= 0 ? 1 : 0;
      return c;
    };
    for (const auto& ps : e->psets)
      for (int g = ps->group_base; g < ps->group_base + ps->n_groups; ++g) e->stats.plan_queries[3] += lanes(g);
    for (const auto& ss : e->ssets)
      for (int g = ss->group_base; g < ss->group_base + ss->n_groups; ++g) e->stats.plan_queries[4] += lanes(g);
    for (const auto& gs : e->gsets)
      for (int g = gs->group_base; g < gs->group_base + gs->n_groups; ++g)
        e->stats.plan_queries[(size_t)g < e->group_seq.size() && e->group_seq[g] > 0 ? 5 : 6] += lanes(g);
    for (const auto& ws : e->wsets) e->stats.plan_queries[7] += (int64_t)ws->qs.size();
    *out = e->stats;
    return SDH_OK;
  });
}

// Device memory of the sparse K_slab state: the live blocks' bytes, the slab's reserved bytes (live
// blocks, not yet reclaimed superseded ones, and free room) and the directory's
int sdh_engine_state_bytes(sdh_engine* e, int64_t* live_bytes, int64_t* reserved_bytes, int64_t* dir_bytes) {
  if (!e) return SDH_E_INVALID;
  return guard(e, [&]() {
    int64_t lb = 0, rb = 0, db = 0;
    for (auto& up : e->ssets) {
      auto& ss = *up;
      lb += slab_live_words(e, ss) * 4;
      for (int64_t c : ss.cap) rb += c * 4;
      db += ss.key_cap * ss.n_groups * 8;
    }
    if (live_bytes) *live_bytes = lb;
    if (reserved_bytes) *reserved_bytes = rb;
    if (dir_bytes) *dir_bytes = db;
    return SDH_OK;
  });
}

int sdh_engine_set_strings(sdh_engine* e, int64_t n, const int32_t* ids, const int32_t* java_hash,
                           const int32_t* utf16_len) {
  if (!e || n < 0 || (n > 0 && (!ids || !java_hash || !utf16_len))) return SDH_E_INVALID;
  return guard(e, [&]() {
    for (int64_t i = 0; i < n; ++i) {
      if (utf16_len[i] < 0) throw Error(SDH_E_INVALID, "negative string length");
      e->str_info[ids[i]] = {java_hash[i], (int64_t)utf16_len[i]};
    }
    return SDH_OK;
  });
}

int sdh_engine_snapshot(sdh_engine* e, void** blob, size_t* len) {
  if (!e || !blob || !len) return SDH_E_INVALID;
  return guard(e, [&]() {
    HIPCHK(hipStreamSynchronize(e->stream));
    snap::Writer w;
    snap_save(e, w);
    *len = w.words().size() * 8;
    *blob = malloc(*len);
    memcpy(*blob, w.words().data(), *len);
    return SDH_OK;
  });
}

int sdh_engine_restore(sdh_engine* e, const void* blob, size_t len) {
  if (!e || !blob) return SDH_E_INVALID;
  return guard(e, [&]() {
    snap_load(e, snap::Reader(blob, len));
    e->g_dev_matches = 0;
    e->device_matches = 0;
    e->r_matches = 0;
    e->r_blocks_used = 0;
    e->rr_ready = 0;
    table_clear(e);
    e->broken.clear();
    return SDH_OK;
  });
}

void sdh_free(void* p) { free(p); }

void sdh_engine_destroy(sdh_engine* e) {
  if (!e) return;
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->h2d) (void)hipStreamSynchronize(e->h2d);
  for (hipEvent_t ev : {e->ev_h0, e->ev_h1, e->ev_stage[0], e->ev_stage[1]})
    if (ev) (void)hipEventDestroy(ev);
  if (e->h2d) (void)hipStreamDestroy(e->h2d);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

const char* sdh_last_error(sdh_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

}  // extern "C"

// knobs.h (t_knobs: the engine whose ABI call runs on this thread)
const char* sdh::knob(const char* name) {
  if (!t_knobs) return nullptr;
  for (const auto& kv : *t_knobs)
    if (kv.first == name) return kv.second.c_str();
  return nullptr;
}
