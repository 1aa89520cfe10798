// select_host.cpp -- test-only host build of the device selector's lane body
// (siddhi_amd/csrc/select_body.h), its lowering (select_lower.h) and the event store's row layout.
// tests/select_host.py builds it with its own compiler command and checks the rows against
// siddhi_amd/selector.py. Built with -DSELECT_HOST_MAIN it is a stand-alone program (a small
// self-check, for sanitizer builds of the lane body).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../siddhi_amd/csrc/select_lower.h"

using namespace sdh;

namespace {
struct Host {
  kg::LProgram P;
  sel::Program S;
};

template <class Match>
uint64_t run_row(const Host& h, int q, const sel::Store& st, const Match& m, int64_t* cells, int64_t n, int64_t i,
                 int32_t& err) {
  const sel::Tables T = h.S.tables();
  const sel::Query& Q = h.S.queries[(size_t)q];
  uint64_t nulls = 0;
  if (Q.n_out > 0) {
    const sel::Shape& sh = h.S.shapes[(size_t)Q.shape];
    const int64_t* qc = h.S.consts.data() + Q.const0;
    nulls = sh.depth <= kg::RSTACK ? sel::project<kg::RegStack>(T, sh, qc, st, m, cells, n, i, err)
                                   : sel::project<kg::ArrStack>(T, sh, qc, st, m, cells, n, i, err);
  }
  for (int c = Q.n_out; c < h.S.width; ++c) cells[(int64_t)c * n + i] = 0;
  if (Q.n_out < 64) nulls |= ~0ull << Q.n_out;
  return nulls;
}
}  // namespace

extern "C" {

void* slh_create(const void* blob, size_t len) {
  try {
    Host* h = new Host;
    h->P = kg::read_program(blob, len);
    h->S = sel::lower_select(h->P);
    if (h->S.bad || h->S.over >= 0 || h->S.max_depth > kg::GSTACK - 1) {
      delete h;
      return nullptr;
    }
    return h;
  } catch (const std::exception&) {
    return nullptr;
  }
}
void slh_destroy(void* p) { delete static_cast<Host*>(p); }
int slh_width(void* p) { return static_cast<Host*>(p)->S.width; }
int slh_shapes(void* p) { return (int)static_cast<Host*>(p)->S.shapes.size(); }
int slh_shape_of(void* p, int q) { return static_cast<Host*>(p)->S.queries[(size_t)q].shape; }
int slh_n_out(void* p, int q) { return static_cast<Host*>(p)->S.queries[(size_t)q].n_out; }
int slh_out_type(void* p, int q, int c) { return static_cast<Host*>(p)->S.types[(size_t)q][(size_t)c]; }
int slh_out_direct(void* p, int q, int c) {
  const Host* h = static_cast<Host*>(p);
  return h->S.outs[(size_t)(h->S.shapes[(size_t)h->S.queries[(size_t)q].shape].out0 + c)].direct;
}
int slh_row_words(void* p) {
  size_t na = 0;
  for (const auto& s : static_cast<Host*>(p)->P.stream_types) na = std::max(na, s.size());
  return 2 + (int)na;
}

// n events of na attributes (raw 64-bit words vals[n][na], nulls[n][na]) into the ring `rows` of cap
// rows of W words, by seq
void slh_store_append(int64_t* rows, int64_t cap, int W, int64_t seq_base, int64_t n, const int64_t* ts,
                      const int64_t* vals, const uint8_t* nulls, int na) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = seq_base + i;
    int64_t nb = 0;
    for (int a = 0; a < na; ++a)
      if (nulls && nulls[i * na + a]) nb |= (int64_t)1 << a;
    rows[sel::store_index(s, cap - 1, W, 0)] = ts[i];
    rows[sel::store_index(s, cap - 1, W, 1)] = nb;
    for (int w = 2; w < W; ++w) rows[sel::store_index(s, cap - 1, W, w)] = w - 2 < na ? vals[i * na + (w - 2)] : 0;
  }
}

// n matches in sdh_matches form (query, off, words) -> cells[width][n], nulls[n]; returns the error bits
int slh_project(void* p, int64_t n, const int64_t* query, const int64_t* off, const int64_t* words,
                const int64_t* rows, int64_t cap, int W, int64_t lo, int64_t* cells, uint64_t* nulls) {
  const Host* h = static_cast<Host*>(p);
  const sel::Store st{rows, cap - 1, lo, W, 0};
  int32_t err = 0;
  for (int64_t i = 0; i < n; ++i) {
    const sel::WordsMatch m{words + off[i], off[i + 1] - off[i]};
    nulls[i] = run_row(*h, (int)query[i], st, m, cells, n, i, err);
  }
  return err;
}

// n K_ratchet matches as compact rows {query, e2 - seq_ref, e2 - e1, ...} of cw int32
int slh_project_pairs(void* p, int64_t n, const int32_t* crow, int cw, int64_t seq_ref, const int64_t* rows,
                      int64_t cap, int W, int64_t lo, int64_t* cells, uint64_t* nulls) {
  const Host* h = static_cast<Host*>(p);
  const sel::Store st{rows, cap - 1, lo, W, 0};
  int32_t err = 0;
  for (int64_t i = 0; i < n; ++i) {
    sel::PairMatch m;
    m.e2 = seq_ref + crow[i * cw + 1];
    m.e1 = m.e2 - crow[i * cw + 2];
    nulls[i] = run_row(*h, crow[i * cw], st, m, cells, n, i, err);
  }
  return err;
}

}  // extern "C"

#ifdef SELECT_HOST_MAIN
// stand-alone self-check: StateEvent.getStreamEvent's index rules on a 3-event chain and an empty slot
int main() {
  const int64_t w[] = {3, 10, 11, 12, 0, 1, 20};
  const sel::WordsMatch m{w, 7};
  struct { int slot; int64_t idx; int64_t want; } cases[] = {
      {0, 0, 10}, {0, 2, 12}, {0, 3, -9}, {0, -1, 12}, {0, -2, 11}, {0, -3, 10}, {0, -4, -9},
      {1, 0, -9}, {1, -1, -9}, {2, 0, 20}, {2, -2, -9}, {3, 0, -9}};
  int bad = 0;
  for (const auto& c : cases) {
    int64_t s = -9;
    if (!sel::event_of(m, c.slot, c.idx, s)) s = -9;
    if (s != c.want) {
      std::printf("event_of(slot %d, idx %lld) = %lld, want %lld\n", c.slot, (long long)c.idx, (long long)s,
                  (long long)c.want);
      ++bad;
    }
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad != 0;
}
#endif
