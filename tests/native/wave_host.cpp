// wave_host.cpp -- TEST INFRASTRUCTURE ONLY: K_wave's shape selection (siddhi_amd/csrc/wave_lower.h)
// and its per-partial step (wave_step.h) on the host. The driver runs one query the way one wave of
// nfa_wave.hip runs it: a push in tiles of events, f1 / f2 once per tile (the masks m1 / m2), every
// page of 64 held partials stepped through the tile with the kernel's lock-step loop (the same skip of
// events that cannot change a page), the survivors compacted in creation order, then the fresh page
// whose lane k is the partial event k opens, stepped from event k + 1; matches ordered by the device
// table's key (trigger seq, receiver rank, e1's seq). Lets the restatement be checked against the
// oracle without a GPU. Never part of the product path.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../siddhi_amd/csrc/wave_lower.h"
#include "../../siddhi_amd/csrc/wave_step.h"

using namespace sdh;

namespace {

struct Rec {
  int64_t seq, rank, e1, query, ts;
  std::vector<int64_t> chain;
};

struct VRef {
  int64_t* p;
  int64_t get(int w) const { return p[w]; }
  void set(int w, int64_t v) const { p[w] = v; }
};

struct HEv {
  const int64_t* w;
  uint32_t nul;
  int64_t word(int j) const { return w[j]; }
  bool null(int j) const { return (nul >> j) & 1u; }
};

struct TileEv {
  int64_t ts, seq;
  int64_t w[kg::GMAXNA];
  uint32_t nul;
};

struct Host {
  kg::LProgram P;
  std::vector<kg::GQuery> gq;
  std::vector<KPart> kw, kp;
  std::vector<std::string> why;
  std::vector<int> rank;
  int tile = 64;
  std::vector<std::vector<int64_t>> tab;  // per query its entries (ew words each), creation order
  std::vector<int64_t> pend;              // per query: pending-list entries after its last push
  std::vector<int> seed;                  // per query: the start state's pending list holds its seed
  std::vector<Rec> out;
  std::string err;
};

int ew_of(const KPart& k) { return 3 + k.cmax + k.n_e1 + k.n_first + k.n_last; }

// one tile for one query: nfa_wave.hip's tile body. last: the tile ends the push
void wave_tile(Host* h, int qi, int stream, const std::vector<TileEv>& tv, bool last) {
  const kg::GQuery& q = h->gq[qi];
  const KPart& k = h->kw[qi];
  const PartOffs of{k.cmax, k.n_e1, k.n_first, k.n_last};
  const int ew = ew_of(k), ncap = q.n_cap[stream], cnt = (int)tv.size();
  const int cmin = q.st[1].min, cmax = q.st[1].max;
  uint64_t m1 = 0, m2 = 0;
  for (int te = 0; te < cnt; ++te) {
    const HEv ev{tv[te].w, tv[te].nul};
    if (wave_ev_filter(&q, 0, ev)) m1 |= 1ull << te;
    if (wave_ev_filter(&q, 1, ev)) m2 |= 1ull << te;
  }
  std::vector<int64_t>& ent = h->tab[qi];
  const int n = (int)(ent.size() / ew);
  std::vector<int64_t> kept;
  int64_t pend = 0;
  const int np = (n + 63) / 64;
  for (int pi = 0; pi <= np; ++pi) {
    const bool fresh = pi == np;
    if (fresh && !m1) break;
    // the page's lanes
    std::vector<int64_t> pg((size_t)64 * ew, 0);
    bool alive[64], had[64], new3[64];
    int te0[64], done[64];
    int64_t fl[64];
    int te_lo = 0;
    for (int l = 0; l < 64; ++l) {
      const VRef e{pg.data() + (size_t)l * ew};
      te0[l] = 0;
      done[l] = -1;
      new3[l] = false;
      if (!fresh) {
        alive[l] = pi * 64 + l < n;
        if (alive[l]) std::copy(ent.begin() + (size_t)(pi * 64 + l) * ew, ent.begin() + (size_t)(pi * 64 + l + 1) * ew, pg.begin() + (size_t)l * ew);
      } else {
        alive[l] = l < cnt && ((m1 >> l) & 1);
        if (alive[l]) wave_open(e, of, ncap, tv[l].ts, tv[l].seq, HEv{tv[l].w, tv[l].nul});
        te0[l] = l + 1;
      }
      had[l] = alive[l];
      fl[l] = alive[l] ? e.get(2) : 0;
    }
    if (fresh) te_lo = __builtin_ffsll((long long)m1);
    for (int te = te_lo; te < cnt; ++te) {
      bool any = false, any3 = false;
      for (int l = 0; l < 64; ++l) {
        any |= alive[l];
        any3 |= alive[l] && te >= te0[l] && wave_in3(fl[l]);
      }
      if (!any) break;
      if (!((m2 >> te) & 1) && !any3) continue;
      for (int l = 0; l < 64; ++l) {
        if (!(alive[l] && te >= te0[l])) continue;
        const VRef e{pg.data() + (size_t)l * ew};
        const HEv ev{tv[te].w, tv[te].nul};
        const bool was3 = wave_in3(fl[l]);
        const int r = wave_step(e, fl[l], of, ncap, cmin, cmax, q.within, tv[te].ts, tv[te].seq, ev, (m2 >> te) & 1,
                                [&]() { return wave_f3(&q, ev, part_ent(e, fl[l], of)); });
        if (r == WS_DONE) done[l] = te;
        if (r != WS_KEEP) alive[l] = false;
        if (te == cnt - 1) new3[l] = !was3 && wave_in3(fl[l]);
      }
    }
    for (int l = 0; l < 64; ++l) {
      const VRef e{pg.data() + (size_t)l * ew};
      if (had[l]) e.set(2, fl[l]);
      if (done[l] >= 0) {
        Rec rc{};
        rc.seq = tv[done[l]].seq;
        rc.rank = h->rank[(size_t)qi * h->P.stream_types.size() + stream];
        rc.e1 = e.get(1);
        rc.query = qi;
        rc.ts = tv[done[l]].ts;
        for (int c = 0; c < wave_len(fl[l]); ++c) rc.chain.push_back(e.get(3 + c));
        h->out.push_back(rc);
      }
      if (!alive[l]) continue;
      kept.insert(kept.end(), pg.begin() + (size_t)l * ew, pg.begin() + (size_t)(l + 1) * ew);
      pend += wave_len(fl[l]) < cmax && !(fresh && l == cnt - 1);
      pend += wave_in3(fl[l]) && !new3[l];
    }
  }
  ent.swap(kept);
  if (last) {
    h->pend[qi] = pend;
    h->seed[qi] = !((m1 >> (cnt - 1)) & 1);  // an e1 match re-arms the seed into the next event's list
  }
}

}  // namespace

extern "C" {

void* wvh_create(const void* blob, size_t len, char* why, size_t cap) {
  try {
    auto* h = new Host;
    h->P = kg::read_program(blob, len);
    kg::Sizing sz;
    for (int qi = 0; qi < (int)h->P.q.size(); ++qi) {
      h->gq.push_back(kg::lower_gen(h->P, qi, sz));
      const char* w = "";
      h->kw.push_back(wave_shape(h->P, qi, h->gq.back(), &w));
      h->why.push_back(w);
      h->kp.push_back(kg::reads_fanout(h->P, qi) ? KPart{} : kpart_shape(h->P, qi, h->gq.back()));
    }
    h->rank = kg::output_ranks(h->P);
    h->tab.resize(h->P.q.size());
    h->pend.assign(h->P.q.size(), 0);
    h->seed.assign(h->P.q.size(), 1);
    return h;
  } catch (const std::exception& ex) {
    snprintf(why, cap, "%s", ex.what());
    return nullptr;
  }
}

// out[7] = kind, sA, sB, cmax, n_e1, n_first, n_last of query qi under wave_shape (which = 0) or
// kpart_shape (which = 1); kind -1: not that shape
void wvh_shape(void* hp, int qi, int which, int32_t* out) {
  const KPart& k = which ? ((Host*)hp)->kp[qi] : ((Host*)hp)->kw[qi];
  const int v[7] = {k.kind, k.sA, k.sB, k.cmax, k.n_e1, k.n_first, k.n_last};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}
const char* wvh_why(void* hp, int qi) { return ((Host*)hp)->why[qi].c_str(); }

void wvh_set_tile(void* hp, int tile) { ((Host*)hp)->tile = tile < 1 ? 1 : tile > 64 ? 64 : tile; }

// one push; every query reading the stream must be a K_wave shape, others are an error
int wvh_send(void* hp, int stream, int64_t n, int64_t seq0, const int64_t* ts, const int64_t* vals,
             const uint8_t* nulls) {
  Host* h = (Host*)hp;
  try {
    const size_t na = h->P.stream_types[stream].size();
    for (int qi = 0; qi < (int)h->P.q.size(); ++qi) {
      const kg::GQuery& q = h->gq[qi];
      if (q.st[0].stream != stream) continue;
      if (h->kw[qi].kind != PK_COUNT) throw std::runtime_error("query " + std::to_string(qi) + " is not a K_wave shape: " + h->why[qi]);
      for (int64_t t0 = 0; t0 < n; t0 += h->tile) {
        std::vector<TileEv> tv;
        for (int64_t k = t0; k < n && k < t0 + h->tile; ++k) {
          TileEv ev{};
          ev.ts = ts[k];
          ev.seq = seq0 + k;
          for (int c = 0; c < q.n_cap[stream]; ++c) {
            const int a = q.cap_attr[stream][c];
            ev.w[c] = vals[k * na + a];
            if (nulls && nulls[k * na + a]) ev.nul |= 1u << c;
          }
          tv.push_back(ev);
        }
        wave_tile(h, qi, stream, tv, t0 + h->tile >= n);
      }
    }
    std::stable_sort(h->out.begin(), h->out.end(), [](const Rec& a, const Rec& b) {
      if (a.seq != b.seq) return a.seq < b.seq;
      if (a.rank != b.rank) return a.rank < b.rank;
      return a.e1 < b.e1;
    });
    return 0;
  } catch (const std::exception& ex) {
    h->err = ex.what();
    return -1;
  }
}

// live partials as the engine reports them (pending-list entries of the non-start states), and the
// start states' pending seeds, which the oracle's count includes
int64_t wvh_live(void* hp) {
  int64_t n = 0;
  for (int64_t x : ((Host*)hp)->pend) n += x;
  return n;
}
int64_t wvh_seeds(void* hp) {
  int64_t n = 0;
  for (int x : ((Host*)hp)->seed) n += x;
  return n;
}
int64_t wvh_entries(void* hp) {
  Host* h = (Host*)hp;
  int64_t n = 0;
  for (size_t qi = 0; qi < h->tab.size(); ++qi)
    if (h->kw[qi].kind == PK_COUNT) n += (int64_t)h->tab[qi].size() / ew_of(h->kw[qi]);
  return n;
}
int64_t wvh_num_matches(void* hp) { return (int64_t)((Host*)hp)->out.size(); }
int64_t wvh_match_words(void* hp) {
  int64_t w = 0;
  for (auto& r : ((Host*)hp)->out) w += 5 + (int64_t)r.chain.size();
  return w;
}
int wvh_get_matches(void* hp, int64_t* query, int64_t* key, int64_t* ts, int64_t* off, int64_t* words) {
  Host* h = (Host*)hp;
  int64_t w = 0;
  for (size_t i = 0; i < h->out.size(); ++i) {
    const Rec& r = h->out[i];
    query[i] = r.query;
    key[i] = -1;
    ts[i] = r.ts;
    off[i] = w;
    words[w++] = 1;
    words[w++] = r.e1;
    words[w++] = (int64_t)r.chain.size();
    for (int64_t x : r.chain) words[w++] = x;
    words[w++] = 1;
    words[w++] = r.seq;
  }
  off[h->out.size()] = w;
  return 0;
}
void wvh_clear(void* hp) { ((Host*)hp)->out.clear(); }
const char* wvh_error(void* hp) { return ((Host*)hp)->err.c_str(); }
void wvh_destroy(void* hp) { delete (Host*)hp; }

}  // extern "C"
