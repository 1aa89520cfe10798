// part_lower_host.cpp -- TEST INFRASTRUCTURE ONLY: K_part's shape selection (siddhi_amd/csrc/
// part_lower.h) and the chain kind's per-partial step (part_chain.h) on the host. The driver runs one
// (query, key) instance the way one lane of part_body.h's chain_tile runs it: the key's events of a
// push in tiles, every held partial stepped through a whole tile before the next one (entry-major),
// the partials the tile opens after them, the kept ones compacted in creation order; matches ordered
// by the device table's key (trigger seq, receiver rank, then the earlier slots' seqs, slot S-2 most
// significant). Lets the restatement be checked against the oracle without a GPU. Never part of the
// product path.
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../siddhi_amd/csrc/part_chain.h"
#include "../../siddhi_amd/csrc/part_lower.h"

using namespace sdh;

namespace {

struct Rec {
  int64_t seq, rank, lo[MAXLO], query, key, ts;
  std::vector<int64_t> slots;
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

struct Host {
  kg::LProgram P;
  std::vector<kg::GQuery> gq;
  std::vector<KPart> kp;
  std::vector<int> rank;
  int tile = 64;
  // per partition: key -> per partition query its entries (ew words each)
  std::vector<std::map<int64_t, std::vector<std::vector<int64_t>>>> inst;
  std::vector<Rec> out;
  std::string err;
};

struct TileEv {
  int64_t ts, seq;
  int64_t w[kg::GMAXNA];
  uint32_t nul;
};

// one tile of one key's events for one chain query: part_body.h chain_tile
void chain_tile(Host* h, int qi, int64_t key, int stream, std::vector<int64_t>& ent, const std::vector<TileEv>& tv) {
  const kg::GQuery& q = h->gq[qi];
  const KPart& kp = h->kp[qi];
  const PartOffs of{kp.cmax, kp.n_e1, kp.n_first, kp.n_last};
  const int ew = 3 + of.cmax + of.n_e1 + of.n_first + of.n_last;
  const int S = q.n_states, ncap = q.n_cap[stream], cnt = (int)tv.size();
  const int n = (int)(ent.size() / ew);
  std::vector<int64_t> kept;
  auto run = [&](std::vector<int64_t> e, int te0) {  // (a copy: the partial's words while it runs)
    const VRef r{e.data()};
    int64_t fl = r.get(2);
    int filled = (int)(fl & 0xff);
    bool alive = te0 < cnt;
    int done = -1;
    for (int te = te0; te < cnt && alive; ++te) {
      const HEv ev{tv[te].w, tv[te].nul};
      const int st = chain_step(S, filled, r.get(0), tv[te].ts, q.within,
                                [&](int s) { return chain_filter(&q, &q, s, ev, part_ent(r, fl, of)); });
      if (st == CS_ADVANCE) {
        ++filled;
        fl = chain_advance(r, fl, of, ncap, filled, tv[te].seq, ev);
      } else if (st != CS_WAIT) {
        if (st == CS_DONE) done = te;
        alive = false;
      }
    }
    if (done >= 0) {
      Rec rc{};
      rc.seq = tv[done].seq;
      rc.rank = h->rank[(size_t)qi * h->P.stream_types.size() + stream];
      rc.query = qi;
      rc.key = key;
      rc.ts = tv[done].ts;
      for (int k = 0; k < S - 1; ++k) {
        rc.lo[k] = chain_slot_seq(r, k);
        rc.slots.push_back(rc.lo[k]);
      }
      rc.slots.push_back(rc.seq);
      h->out.push_back(rc);
    }
    if (alive || (done < 0 && te0 >= cnt)) {
      r.set(2, (fl & ~0xffll) | (int64_t)filled);
      kept.insert(kept.end(), e.begin(), e.end());
    }
  };
  for (int kk = 0; kk < n; ++kk) run(std::vector<int64_t>(ent.begin() + (size_t)kk * ew, ent.begin() + (size_t)(kk + 1) * ew), 0);
  const PartEnt<VRef> none{VRef{nullptr}, 0, of};
  for (int tc = 0; tc < cnt; ++tc) {
    const HEv ev{tv[tc].w, tv[tc].nul};
    if (!chain_filter(&q, &q, 0, ev, none)) continue;  // f1 reads the event only
    std::vector<int64_t> e((size_t)ew, 0);
    e[2] = chain_open(VRef{e.data()}, of, ncap, tv[tc].ts, tv[tc].seq, ev);
    run(e, tc + 1);
  }
  ent.swap(kept);
}

}  // namespace

extern "C" {

void* plh_create(const void* blob, size_t len, char* why, size_t cap) {
  try {
    auto* h = new Host;
    h->P = kg::read_program(blob, len);
    kg::Sizing sz;
    for (int qi = 0; qi < (int)h->P.q.size(); ++qi) {
      h->gq.push_back(kg::lower_gen(h->P, qi, sz));
      h->kp.push_back(kg::reads_fanout(h->P, qi) ? KPart{} : kpart_shape(h->P, qi, h->gq.back()));
    }
    h->rank = kg::output_ranks(h->P);
    h->inst.resize(h->P.parts.size());
    return h;
  } catch (const std::exception& ex) {
    snprintf(why, cap, "%s", ex.what());
    return nullptr;
  }
}

// out[7] = kind, sA, sB, cmax, n_e1, n_first, n_last of query qi (kind -1: not a K_part shape)
void plh_shape(void* hp, int qi, int32_t* out) {
  const KPart& k = ((Host*)hp)->kp[qi];
  const int v[7] = {k.kind, k.sA, k.sB, k.cmax, k.n_e1, k.n_first, k.n_last};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
}

void plh_set_tile(void* hp, int tile) { ((Host*)hp)->tile = tile < 1 ? 1 : tile > 64 ? 64 : tile; }

// one push; every partitioned query must be a chain (PK_CHAIN), others are an error
int plh_send(void* hp, int stream, int64_t n, int64_t seq0, const int64_t* ts, const int64_t* vals,
             const uint8_t* nulls) {
  Host* h = (Host*)hp;
  try {
    const size_t na = h->P.stream_types[stream].size();
    for (size_t pi = 0; pi < h->P.parts.size(); ++pi) {
      const kg::LPart& pd = h->P.parts[pi];
      int attr = -1;
      for (const auto& key : pd.keys)
        if (key.stream == stream) attr = (int)key.code[0].imm;
      if (attr < 0) continue;
      std::map<int64_t, std::vector<int64_t>> by_key;  // the routing: each key's events in order
      for (int64_t k = 0; k < n; ++k) {
        if (nulls && nulls[k * na + attr]) continue;  // a null key drops the event
        by_key[kg::key_of_raw(h->P.stream_types[stream][attr], vals[k * na + attr])].push_back(k);
      }
      for (const auto& kv : by_key) {
        auto& v = h->inst[pi][kv.first];
        if (v.empty()) v.resize(pd.queries.size());
        for (size_t j = 0; j < pd.queries.size(); ++j) {
          const int qi = pd.queries[j];
          if (h->kp[qi].kind != PK_CHAIN) throw std::runtime_error("query " + std::to_string(qi) + " is not a K_part chain");
          const kg::GQuery& q = h->gq[qi];
          if (q.st[0].stream != stream) continue;
          for (size_t t0 = 0; t0 < kv.second.size(); t0 += h->tile) {
            std::vector<TileEv> tv;
            for (size_t t = t0; t < kv.second.size() && t < t0 + h->tile; ++t) {
              const int64_t k = kv.second[t];
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
            chain_tile(h, qi, kv.first, stream, v[j], tv);
          }
        }
      }
    }
    std::stable_sort(h->out.begin(), h->out.end(), [](const Rec& a, const Rec& b) {
      if (a.seq != b.seq) return a.seq < b.seq;
      if (a.rank != b.rank) return a.rank < b.rank;
      for (int k = MAXLO - 1; k >= 0; --k)
        if (a.lo[k] != b.lo[k]) return a.lo[k] < b.lo[k];
      return false;
    });
    return 0;
  } catch (const std::exception& ex) {
    h->err = ex.what();
    return -1;
  }
}

int64_t plh_live(void* hp) {
  Host* h = (Host*)hp;
  int64_t n = 0;
  for (size_t pi = 0; pi < h->inst.size(); ++pi)
    for (auto& kv : h->inst[pi])
      for (size_t j = 0; j < kv.second.size(); ++j) {
        const KPart& k = h->kp[h->P.parts[pi].queries[j]];
        n += (int64_t)kv.second[j].size() / (3 + k.cmax + k.n_e1 + k.n_first + k.n_last);
      }
  return n;
}
int64_t plh_num_matches(void* hp) { return (int64_t)((Host*)hp)->out.size(); }
int64_t plh_match_words(void* hp) {
  int64_t w = 0;
  for (auto& r : ((Host*)hp)->out) w += 2 * (int64_t)r.slots.size();
  return w;
}
int plh_get_matches(void* hp, int64_t* query, int64_t* key, int64_t* ts, int64_t* off, int64_t* words) {
  Host* h = (Host*)hp;
  int64_t w = 0;
  for (size_t i = 0; i < h->out.size(); ++i) {
    const Rec& r = h->out[i];
    query[i] = r.query;
    key[i] = r.key;
    ts[i] = r.ts;
    off[i] = w;
    for (int64_t x : r.slots) {
      words[w++] = 1;
      words[w++] = x;
    }
  }
  off[h->out.size()] = w;
  return 0;
}
void plh_clear(void* hp) { ((Host*)hp)->out.clear(); }
const char* plh_error(void* hp) { return ((Host*)hp)->err.c_str(); }
void plh_destroy(void* hp) { delete (Host*)hp; }

}  // extern "C"
