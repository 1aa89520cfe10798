// rec_rows_host.cpp -- siddhi_amd/csrc/rec_rows.h compiled for the host (test infrastructure only):
// the row location, the rec4 side-run expansion and the flat / K_chain record match sources that
// sdh_engine_records_rows runs on the device, callable from tests/rec_rows_host.py.
#include <cstdint>
#include <vector>

#include "../../siddhi_amd/csrc/rec_rows.h"
#include "../../siddhi_amd/csrc/select_body.h"

using namespace sdh;

extern "C" {

long long rrh_locate(const long long* off, long long n, long long row) {
  return rr::locate(reinterpret_cast<const int64_t*>(off), n, row);
}

int rrh_part_of(long long n0, long long n1, long long n2, long long row, long long* local) {
  const rr::Parts P{{n0, n1, n2}};
  int64_t l = 0;
  const int p = rr::part_of(P, row, l);
  *local = l;
  return p;
}

long long rrh_part_window(long long n0, long long n1, long long n2, int p, long long first, long long n,
                          long long* local) {
  const rr::Parts P{{n0, n1, n2}};
  int64_t l = 0;
  const int64_t c = rr::part_window(P, p, first, n, l);
  *local = l;
  return c;
}

// entries [i0, i1) of one block -> out[(i - i0) * 3 ..] = {e1, e2, lane}; fmt: 3 rec4 (ns side entries),
// 1 8-B, 2 16-B records (include/siddhi_hip.h SDH_REC_*). Returns the side entries a rec4 run read.
int rrh_pairs(const void* blk, long long blk_bytes, int fmt, int ns, int i0, int i1, long long sb, long long* out) {
  const int len = i1 - i0;
  int read = 0;
  std::vector<int32_t> head((size_t)(len > 0 ? len : 0));
  std::vector<uint32_t> e2((size_t)(len > 0 ? len : 0));
  if (fmt == 3) read = rr::expand_run(blk, blk_bytes, ns, i0, i1, head.data(), e2.data());
  const uint32_t* w = static_cast<const uint32_t*>(blk);
  for (int i = i0; i < i1; ++i) {
    rr::Pair p;
    if (fmt == 3) p = rr::pair_rec4(w[i], e2[(size_t)(i - i0)], sb);
    else if (fmt == 1) p = rr::pair_rec8(w[2 * i], w[2 * i + 1], sb);
    else p = rr::pair_rec16(w[4 * i], w[4 * i + 1], w[4 * i + 2], sb);
    out[(i - i0) * 3 + 0] = p.e1;
    out[(i - i0) * 3 + 1] = p.e2;
    out[(i - i0) * 3 + 2] = p.ln;
  }
  return read;
}

// the per-entry search the expansion replaces (the side entry of entry i)
int rrh_side_of(const void* blk, long long blk_bytes, int ns, int i) { return rr::side_of(blk, blk_bytes, ns, i); }

// Walk `n` words of flat records as flat_heads_kernel does, opening each record: per record its head
// offset, {query, trigger seq, own_ts, ts} in meta and its slot words appended to `words` (wlen their
// counts). Returns the records found (pads skipped), or -1 when an output is too small.
long long rrh_walk(const long long* buf, long long n, long long seq_base, long long* heads, long long* meta,
                   long long* wlen, long long cap_rec, long long* words, long long cap_words, long long* pads) {
  const int64_t* b = reinterpret_cast<const int64_t*>(buf);
  long long nr = 0, nw = 0;
  *pads = 0;
  for (int64_t pos = 0; pos < n; pos += rr::rec_span(b[pos])) {
    if (rr::rec_kind(b[pos]) == rr::KIND_PAD) {
      ++*pads;
      continue;
    }
    rr::FlatMatch m;
    int q = 0;
    int64_t seq = 0;
    bool own = false;
    if (!rr::flat_open(b + pos, seq_base, m, q, seq, own)) return -2;
    if (nr >= cap_rec) return -1;
    const int64_t len = rr::flat_words(m, reinterpret_cast<int64_t*>(words) + nw, cap_words - nw);
    if (nw + len > cap_words) return -1;
    heads[nr] = pos;
    meta[4 * nr + 0] = q;
    meta[4 * nr + 1] = seq;
    meta[4 * nr + 2] = own ? 1 : 0;
    meta[4 * nr + 3] = m.ts;
    wlen[nr] = len;
    nw += len;
    ++nr;
  }
  return nr;
}

// StateEvent.getStreamEvent on one flat record through the selector's event_of (select_body.h): the seq
// slot[idx] resolves to, or INT64_MIN for none
long long rrh_flat_event(const long long* rec, long long seq_base, int slot, long long idx) {
  rr::FlatMatch m;
  int q = 0;
  int64_t seq = 0, s = 0;
  bool own = false;
  if (!rr::flat_open(reinterpret_cast<const int64_t*>(rec), seq_base, m, q, seq, own)) return INT64_MIN;
  return sel::event_of(m, slot, idx, s) ? s : INT64_MIN;
}

// the same on a K_chain record {query, ts, seq_0 .. seq_{S-1}}
long long rrh_chain_event(const long long* rec, int S, int slot, long long idx) {
  const rr::ChainMatch m{reinterpret_cast<const int64_t*>(rec), S, rec[1]};
  int64_t s = 0;
  return sel::event_of(m, slot, idx, s) ? s : INT64_MIN;
}

}  // extern "C"
