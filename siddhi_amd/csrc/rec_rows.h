// rec_rows.h -- device records (SDH_FLAG_DEVICE_MATCHES; formats: include/siddhi_hip.h sdh_records) as
// the selector's match sources: what sdh_engine_records_rows needs to turn row r of a push's records
// into the slots select_body.h projects.
//
//   row location   r -> (part, block / record / segment) from exclusive prefixes of the per-block,
//                  per-record and per-segment counts
//   rec4 side runs entry i of a rec4 block belongs to the trigger of the last side entry whose `first`
//                  is <= i. For a run [i0, i1) of entries the side entries that matter are found once
//                  (two searches), each sets a head at max(first, i0) - i0 holding its index j, and a
//                  running max carries j forward: entry i then reads its trigger at one index.
//                  expand_run states that serially; select.hip's select_ratchet_records_kernel runs the
//                  same steps (the index side_of finds, head_slot, the max) with a search the whole
//                  workgroup makes at once, the heads in LDS and a wave scan
//   flat records   a full or narrow record as a match source (FlatMatch: the chain of a slot and its
//                  seqs read in place, the {count, seqs...} words flat_words lists), pads skipped by span
//   K_chain        {query, ts, seq_0 .. seq_{S-1}} (ChainMatch)
//
// Written once for host and device (KG_FN), like select_body.h: tests/native/rec_rows_host.cpp builds
// it for the host. matches.hip's ratchet_record and append_gen_kernel hold the table append's own copies
// of the two decodes (their registers stay as they are); the host test checks this description against
// a restatement of theirs.
#pragma once
#include "kgen.h"

namespace sdh {
namespace rr {

KG_FN int32_t lo32(int64_t w) { return (int32_t)(uint32_t)(uint64_t)w; }
KG_FN int32_t hi32(int64_t w) { return (int32_t)(uint32_t)((uint64_t)w >> 32); }

// ---- row location ----
// off[0 .. n]: an exclusive prefix of n counts. The item that holds `row` (off[0] <= row < off[n]): the
// last i with off[i] <= row, which is never an empty item.
KG_FN int64_t locate(const int64_t* off, int64_t n, int64_t row) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Rows are in record order: part 1 (K_ratchet blocks, in block and entry order), part 2 (flat records,
// in buffer order), part 3 (K_chain segments, in segment and record order).
struct Parts {
  int64_t n[3];
  KG_FN int64_t total() const { return n[0] + n[1] + n[2]; }
  KG_FN int64_t first(int p) const { return p == 0 ? 0 : p == 1 ? n[0] : n[0] + n[1]; }
};
// the part of `row` (0 <= row < total()) and its index inside it
KG_FN int part_of(const Parts& P, int64_t row, int64_t& local) {
  int p = 0;
  while (p < 2 && row >= P.n[p]) row -= P.n[p++];
  local = row;
  return p;
}
// window [first, first + n) cut to part p: the part's first row of it and how many (0: none)
KG_FN int64_t part_window(const Parts& P, int p, int64_t first, int64_t n, int64_t& local) {
  const int64_t a = P.first(p), b = a + P.n[p];
  const int64_t lo = first > a ? first : a, hi = first + n < b ? first + n : b;
  local = lo - a;
  return hi > lo ? hi - lo : 0;
}

// ---- K_ratchet blocks ----
constexpr uint32_t D26 = (1u << 26) - 1;

// side entry j of a rec4 block of blk_bytes: the uint32 pair {first, e2} at blk_bytes - 8 * (j + 1)
KG_FN const uint32_t* side_entry(const void* blk, int64_t blk_bytes, int j) {
  return reinterpret_cast<const uint32_t*>(static_cast<const char*>(blk) + blk_bytes - 8 * ((int64_t)j + 1));
}
// the side entry of entry i: the last one whose first <= i (side entry 0 has first == 0)
KG_FN int side_of(const void* blk, int64_t blk_bytes, int ns, int i) {
  int lo = 0, hi = ns - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)side_entry(blk, blk_bytes, mid)[0] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// where side entry `first` heads the run that starts at entry i0 (an event that began before the run
// heads its first entry)
KG_FN int head_slot(uint32_t first, int i0) { return (int)first > i0 ? (int)first - i0 : 0; }

// A record as the pair it names: e2 = the trigger's batch offset, ln its lane, and e1 (sb = the push's
// seq_base). rec4: entry {d | ln << 26}, d = s2 - e1, with its trigger from the side entries.
struct Pair {
  int64_t e1, e2;
  uint32_t off, ln;
};
KG_FN Pair pair_rec4(uint32_t entry, uint32_t e2off, int64_t sb) {
  Pair p;
  p.off = e2off;
  p.ln = entry >> 26;
  p.e2 = sb + (int64_t)e2off;
  p.e1 = p.e2 - (int64_t)(entry & D26);
  return p;
}
// 8-B {e2 | ln << 26, e1lo} and 16-B {e2, ln, e1lo, 0}: e1 = s2 - (uint32)((uint32)s2 - e1lo)
KG_FN Pair pair_lo(uint32_t off, uint32_t ln, uint32_t e1lo, int64_t sb) {
  Pair p;
  p.off = off;
  p.ln = ln;
  p.e2 = sb + (int64_t)off;
  p.e1 = p.e2 - (int64_t)(uint32_t)((uint32_t)p.e2 - e1lo);
  return p;
}
KG_FN Pair pair_rec8(uint32_t x, uint32_t y, int64_t sb) { return pair_lo(x & D26, x >> 26, y, sb); }
KG_FN Pair pair_rec16(uint32_t x, uint32_t y, uint32_t z, int64_t sb) { return pair_lo(x, y & 63, z, sb); }

// The run [i0, i1) of a rec4 block expanded serially: e2[i - i0] = the trigger offset of entry i.
// head: i1 - i0 ints of scratch. Returns the side entries the run read.
KG_FN int expand_run(const void* blk, int64_t blk_bytes, int ns, int i0, int i1, int32_t* head, uint32_t* e2) {
  const int len = i1 - i0;
  if (len <= 0) return 0;
  const int j0 = side_of(blk, blk_bytes, ns, i0), j1 = side_of(blk, blk_bytes, ns, i1 - 1) + 1;
  for (int p = 0; p < len; ++p) head[p] = -1;
  for (int j = j0; j < j1; ++j) {
    const int p = head_slot(side_entry(blk, blk_bytes, j)[0], i0);
    if (p < len && head[p] < j) head[p] = j;
  }
  int run = j0;  // (the max-scan; slot 0 always holds j0)
  for (int p = 0; p < len; ++p) {
    run = head[p] > run ? head[p] : run;
    e2[p] = side_entry(blk, blk_bytes, run)[1];
  }
  return j1 - j0;
}

// ---- flat records ----
constexpr int KIND_FULL = -1, KIND_ORAND = 0, KIND_COUNT = 1, KIND_SEQ = 2, KIND_CHAIN = 3, KIND_PAD = 4;

// the words the record (or pad) whose first word is w0 spans; never less than 1, so a walk moves on
KG_FN int64_t rec_span(int64_t w0) {
  const int32_t lo = lo32(w0);
  const int64_t n = lo >= 0 ? (int64_t)lo : (int64_t)((-(int64_t)lo) & 0xFFFF);
  return n > 0 ? n : 1;
}
KG_FN int rec_kind(int64_t w0) {
  const int32_t lo = lo32(w0);
  return lo >= 0 ? KIND_FULL : (int)((-(int64_t)lo) >> 16);
}

// One flat record as the selector's match source. A full record's slots are its own words
// {c, c seqs} from word 7 on; a narrow record's are read in place from its int32 distances back from
// the trigger sq: `at` is then the slot itself.
struct FlatMatch {
  const int64_t* r;
  int kind;
  int S;        // narrow: its slots
  int64_t sq;   // narrow: the trigger's seq
  int64_t ts = 0;
  // distance k of the int32 pairs that start at word w (low half first)
  KG_FN int64_t dist(int w, int64_t k) const { return (k & 1) ? hi32(r[w + k / 2]) : lo32(r[w + k / 2]); }
  KG_FN int64_t chain(int slot, int64_t& at) const {
    if (kind == KIND_FULL) {
      const int64_t len = (int64_t)lo32(r[0]) - 7;
      int64_t j = 0;
      for (int s = 0; s < slot && j < len; ++s) j += 1 + r[7 + j];
      at = 7 + j + 1;
      return j < len ? r[7 + j] : 0;
    }
    at = slot;
    if (slot >= S) return 0;
    if (kind == KIND_ORAND) return slot == 0 ? 1 : (slot == 1 ? hi32(r[2]) : lo32(r[3])) == INT32_MIN ? 0 : 1;
    if (kind == KIND_COUNT) return slot == 1 ? hi32(r[2]) : 1;
    return 1;
  }
  KG_FN int64_t seq(int64_t at, int64_t k) const {
    if (kind == KIND_FULL) return r[at + k];
    if (kind == KIND_ORAND) return sq - (at == 0 ? lo32(r[2]) : at == 1 ? hi32(r[2]) : lo32(r[3]));
    if (kind == KIND_COUNT) return at == 0 ? sq - lo32(r[2]) : at == 1 ? sq - dist(3, k) : sq;
    return at < S - 1 ? sq - dist(2, at) : sq;
  }
};

// the states of a narrow chain record (2 + S / 2 words, an unused upper half INT32_MIN)
KG_FN int chain_states(const int64_t* r) {
  const int words = (int)((-(int64_t)lo32(r[0])) & 0xFFFF);
  return words >= 4 ? 4 : hi32(r[2]) == INT32_MIN ? 2 : 3;
}

// Record r of a push whose batch offset 0 has seq seq_base -> its match source, query and trigger seq.
// own_ts: the record carries its ts (m.ts is set); otherwise the row's ts is the trigger's, from the
// event store. false: a pad.
KG_FN bool flat_open(const int64_t* r, int64_t seq_base, FlatMatch& m, int& q, int64_t& seq, bool& own_ts) {
  m.r = r;
  m.kind = rec_kind(r[0]);
  m.S = 0;
  m.sq = 0;
  m.ts = 0;
  if (m.kind == KIND_FULL) {
    q = (int)r[1];
    seq = r[4];
    m.ts = r[3];
    own_ts = true;
    return true;
  }
  if (m.kind < 0 || m.kind >= KIND_PAD) return false;
  q = hi32(r[0]);
  seq = m.sq = seq_base + (int64_t)(uint32_t)lo32(r[1]);
  m.S = m.kind == KIND_SEQ ? hi32(r[1]) : m.kind == KIND_CHAIN ? chain_states(r) : 3;
  own_ts = false;
  return true;
}

// the match table's slot words {c, c seqs} per slot of an opened record (what WordsMatch would read);
// returns their count, writing at most cap
KG_FN int64_t flat_words(const FlatMatch& m, int64_t* out, int64_t cap) {
  int64_t n = 0;
  if (m.kind == KIND_FULL) {
    const int64_t len = (int64_t)lo32(m.r[0]) - 7;
    for (; n < len; ++n)
      if (n < cap) out[n] = m.r[7 + n];
    return n;
  }
  for (int s = 0; s < m.S; ++s) {
    int64_t at;
    const int64_t c = m.chain(s, at);
    if (n < cap) out[n] = c;
    ++n;
    for (int64_t k = 0; k < c; ++k, ++n)
      if (n < cap) out[n] = m.seq(at, k);
  }
  return n;
}

// ---- K_chain records {query, ts, seq_0 .. seq_{S-1}} ----
struct ChainMatch {
  const int64_t* v;
  int S;
  int64_t ts = 0;
  KG_FN int64_t chain(int slot, int64_t& at) const {
    at = slot;
    return slot < S ? 1 : 0;
  }
  KG_FN int64_t seq(int64_t at, int64_t) const { return v[2 + at]; }
};

}  // namespace rr
}  // namespace sdh
