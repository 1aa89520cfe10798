// engine_gen.hip -- host side of the K_gen family (K_gen, K_seq, K_part, K_slab, K_wave): lowering into sets
// and groups, instance arenas and their growth, the journal of exact re-runs, partition routing, and
// the launches of one push (launch_gen -> gen_pass).
#include "engine_int.h"
#include "launchers.h"
#include "chm_order.h"
#include "java_fmt.h"
#include "mix_plan.h"
#include "part_lower.h"
#include "slab_lower.h"
#include "spec.h"
#include "wave_lower.h"

namespace sdh {
namespace eng {

namespace {

// Shape-compiled kernels (spec.h): SDH_SPEC=0 none, 1 every shape, "require" every shape and a
// failed compile is an error; default: shapes that fill at least two waves (a compile costs about
// a second once per process and shape, the interpreted kernel is exact too)
int spec_mode() {
  const char* v = sdh::knob("SDH_SPEC");
  if (!v || !*v) return 1;
  if (!strcmp(v, "0")) return 0;
  if (!strcmp(v, "require")) return 3;
  return 2;
}

void spec_build(sdh_engine* e) {
  const int mode = spec_mode();
  if (mode == 0) return;
  std::map<int, int> groups;  // K_seq template -> groups
  for (size_t g = 0; g < e->group_seq.size(); ++g)
    if (e->group_seq[g] > 0) ++groups[e->group_tmpl[g]];
  for (const auto& [t, ng] : groups) {
    if (mode == 1 && ng < 2) continue;
    std::string err;
    // ring-mode output reserves the ring in chunks (dev_common.h SDH_RING_CHUNK), so its flushes are
    // cheap and a smaller LDS buffer buys resident waves (C4 ring: 1024 words 25.9 ms/step, 768 22.9,
    // 512 23.7); normal-mode flushes take two atomics each and keep the larger buffer
    const int seq_w = (e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) ? 768 : 0;
    hipFunction_t f = sdh::spec::get_kernel(sdh::spec::seq_source(e->gq[t], seq_w), "sdh_seq_spec", &err);
    if (!f && mode == 3) throw Error(SDH_E_DEVICE, "shape-compiled K_seq kernel: " + err);
    if (f) e->seq_spec[t] = f;
  }
  int64_t n = (int64_t)e->seq_spec.size();
  for (auto& up : e->psets) {
    auto& ps = *up;
    std::map<int, int> pg;  // template -> groups
    for (int g = 0; g < ps.n_groups; ++g) ++pg[e->group_tmpl[ps.group_base + g]];
    for (const auto& [t, ng] : pg) {
      if (mode == 1 && ng < 2) continue;
      // register-resident entries per lane: the first few partials of a (query, key) instance
      // stay in VGPRs across the key's events (C3 instances hold a handful at a time)
      // (C3 at 1000 x 10K keys, or/and entries: 8 26.0 ms/step, 6 25.4, 5 25.1, 4 24.6, 3 24.4, 2 32.8)
      int regs = ps.kind == PK_COUNT ? 3 : 3;
      if (const char* v = sdh::knob(ps.kind == PK_COUNT ? "SDH_KPART_REGS_COUNT" : "SDH_KPART_REGS")) regs = std::max(0, atoi(v));
      sdh::spec::PartLayout lay{ps.kind, ps.sA, ps.sB, ps.cmax, ps.n_e1, ps.n_first, ps.n_last, ps.ew, regs};
      // (C3 ring: 1536 words 20.7 ms/step, 1024 17.5, 768 18.0, 2048 21.8)
      if (e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) lay.out_w = 1024;
      std::string err;
      hipFunction_t f = sdh::spec::get_kernel(sdh::spec::part_source(e->gq[t], lay), "sdh_part_spec", &err);
      if (!f && mode == 3) throw Error(SDH_E_DEVICE, "shape-compiled K_part kernel: " + err);
      if (f) ps.spec[t] = f, ++n;
    }
  }
  e->stats.spec_kernels = n;
}

}  // namespace

void gen_build(sdh_engine* e, const std::vector<int>& qis) {
  kg::Sizing sz;
  if (e->cfg.gen_pool_states > 0) sz.R = std::min(kg::GMAXPOOL, e->cfg.gen_pool_states);
  if (e->cfg.gen_pool_nodes > 0) sz.N = std::min(kg::GMAXPOOL, e->cfg.gen_pool_nodes);
  if (e->cfg.gen_list_cap > 0) sz.LC = std::min(1 << 16, e->cfg.gen_list_cap);
  e->gsz = sz;
  std::vector<int> gidx(e->lp.q.size(), -1);
  std::vector<KPart> kpart(e->lp.q.size());
  std::vector<char> is_slab(e->lp.q.size(), 0);
  const bool use_part = !(e->cfg.flags & SDH_FLAG_FORCE_GEN) && !sdh::knob("SDH_NO_KPART");
  const bool use_slab = !(e->cfg.flags & SDH_FLAG_FORCE_GEN) && !sdh::knob("SDH_NO_KSLAB");
  const bool use_wave = !(e->cfg.flags & SDH_FLAG_FORCE_GEN) && !sdh::knob("SDH_NO_KWAVE");
  std::vector<KPart> kwave(e->lp.q.size());
  for (int qi : qis) {
    try {
      kg::GQuery g = kg::lower_gen(e->lp, qi, sz);
      g.rank = 0;
      if (7 + g.lay.S + g.lay.N > GEN_RING_MARGIN) throw kg::LowerError("match record longer than the ring margin");
      gidx[qi] = (int)e->gq.size();
      e->gq.push_back(g);
      const bool fan = kg::reads_fanout(e->lp, qi);  // fan-out streams run on K_gen (the sweep)
      e->has_fanout |= fan;
      if (use_part && !fan) kpart[qi] = kpart_shape(e->lp, qi, g);
      if (use_wave && !fan) kwave[qi] = wave_shape(e->lp, qi, g);  // (unpartitioned: never a K_part shape)
      if (use_slab && !fan && kpart[qi].kind < 0 && kwave[qi].kind < 0) {
        slab::Shape sh;
        is_slab[qi] = slab::shape_of_query(e->lp, qi, g, &sh, nullptr) ? 1 : 0;
      }
      e->gq_arena.push_back(kpart[qi].kind < 0 && !is_slab[qi] && kwave[qi].kind < 0);
      e->has_absent |= g.lay.TQ > 0;
      if (kpart[qi].kind >= 0 || is_slab[qi] || kwave[qi].kind >= 0) continue;  // K_part / K_slab / K_wave: no K_gen arena
      e->gB32 = std::max(e->gB32, g.lay.n32);
      e->gB64 = std::max(e->gB64, g.lay.n64);
      e->gHotS = std::max(e->gHotS, g.lay.S);
      if (!g.lay.big) e->gHotNU = std::max(e->gHotNU, g.lay.NU);
    } catch (const kg::LowerError& ex) {
      throw Error(SDH_E_UNSUPPORTED, fmt("query %d: %s", qi, ex.what()));
    }
  }
  if (e->gq.empty()) return;
  // lane_q / group_tmpl rows of one set's members, bucketed by shape (see add_set)
  auto add_groups = [&](const std::vector<int>& members, bool seq_ok) {
    std::vector<std::pair<std::string, std::vector<int>>> shapes;
    for (int qi : members) {
      const kg::GQuery sh = kg::shape_of(e->gq[gidx[qi]]);
      std::string sig((const char*)&sh, sizeof sh);
      auto it = std::find_if(shapes.begin(), shapes.end(), [&](const auto& b) { return b.first == sig; });
      if (it == shapes.end()) shapes.emplace_back(std::move(sig), std::vector<int>{gidx[qi]});
      else it->second.push_back(gidx[qi]);
    }
    int n_groups = 0;
    for (const auto& b : shapes) {
      const int ng = (int)((b.second.size() + 63) / 64);
      const int S = (seq_ok && !(e->cfg.flags & SDH_FLAG_FORCE_GEN)) ? kg::seq_window(e->gq[b.second[0]]) : -1;
      for (int g = 0; g < ng; ++g) {
        e->group_seq.push_back(S > 0 ? S : 0);
        e->group_tmpl.push_back(b.second[0]);
        for (int l = 0; l < 64; ++l) {
          const size_t k = (size_t)g * 64 + l;
          e->lane_q.push_back(k < b.second.size() ? b.second[k] : -1);
        }
      }
      n_groups += ng;
    }
    return n_groups;
  };
  auto route_of = [&](int partition) {
    if ((int)e->routes.size() <= partition) e->routes.resize(partition + 1);
    if (e->routes[partition]) return;
    auto r = std::make_unique<sdh_engine::Route>();
    r->max_keys = e->cfg.gen_max_keys > 0 ? e->cfg.gen_max_keys : (1 << 20);
    int64_t slots = 1;
    while (slots < 2 * r->max_keys) slots <<= 1;
    r->tmask = slots - 1;
    r->tkey.ensure(slots + 1);
    r->tid.ensure(slots + 1);
    std::vector<unsigned long long> init((size_t)slots + 1, 0x8000000000000000ull);
    init[slots] = 0;
    HIPCHK(hipMemcpy(r->tkey.p, init.data(), init.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(r->tid.p, 0xff, (slots + 1) * 4));
    r->n_keys.ensure(1);
    HIPCHK(hipMemset(r->n_keys.p, 0, 4));
    r->key_of_id.ensure(r->max_keys);
    HIPCHK(hipMemset(r->key_of_id.p, 0, r->max_keys * 8));  // (a snapshot holds all of it: no stale device memory)
    r->track = !e->lp.parts[partition].fanout.empty();
    if (r->track && e->cfg.shard_world > 1)
      throw Error(SDH_E_UNSUPPORTED, "a non-partitioned stream inside a partition with key sharding");
    e->routes[partition] = std::move(r);
  };
  auto add_part_sets = [&](int partition, const std::vector<int>& members) {
    // one set per (kind, stream): every state of a K_part shape reads one stream, and a set's groups
    // share one buffer selector per key (cur / nxt), so all of them must run on the same pushes --
    // those of their stream. (PK_CHAIN last: older apps keep their set order.)
    const int n_streams = (int)e->prog.stream_types.size();
    for (int kind = PK_OR; kind <= PK_CHAIN; ++kind)
    for (int stream = 0; stream < n_streams; ++stream) {
      std::vector<int> m;
      for (int qi : members)
        if (kpart[qi].kind == kind && e->lp.q[qi].st[0].stream == stream) m.push_back(qi);
      if (m.empty()) continue;
      route_of(partition);
      auto ps = std::make_unique<sdh_engine::PartSet>();
      ps->partition = partition;
      ps->kind = kind;
      ps->stream = stream;
      ps->group_base = (int)(e->lane_q.size() / 64);
      ps->n_groups = add_groups(m, false);
      const KPart& k0 = kpart[m[0]];
      ps->sA = k0.sA;
      ps->sB = k0.sB;
      for (int qi : m) {
        ps->cmax = std::max(ps->cmax, kpart[qi].cmax);
        ps->n_e1 = std::max(ps->n_e1, kpart[qi].n_e1);
        ps->n_first = std::max(ps->n_first, kpart[qi].n_first);
        ps->n_last = std::max(ps->n_last, kpart[qi].n_last);
        if (kpart[qi].sA != ps->sA || kpart[qi].sB != ps->sB) throw Error(SDH_E_UNSUPPORTED, "K_part side order");
      }
      // (a chain partial uses the count layout: cmax = S - 2 slot seqs, then slots 0, 1, 2's words)
      const bool wide_entry = kind == PK_COUNT || kind == PK_CHAIN;
      ps->ew = wide_entry ? 3 + ps->cmax + ps->n_e1 + ps->n_first + ps->n_last : 3;
      ps->cap = kind == PK_COUNT ? 8 : 16;
      if (kind == PK_CHAIN) e->part_chain_lo = std::max(e->part_chain_lo, ps->cmax + 1);
      if (const char* v = sdh::knob("SDH_KPART_CAP")) ps->cap = std::max(1, atoi(v));
      e->psets.push_back(std::move(ps));
    }
  };
  // K_slab: a partition's distinct-stream patterns in one set (slab.h), groups bucketed by shape
  auto add_slab_set = [&](int partition, const std::vector<int>& members) {
    std::vector<int> m;
    for (int qi : members)
      if (is_slab[qi]) m.push_back(qi);
    if (m.empty()) return;
    route_of(partition);
    auto ss = std::make_unique<sdh_engine::SlabSet>();
    ss->partition = partition;
    ss->group_base = (int)(e->lane_q.size() / 64);
    ss->n_groups = add_groups(m, false);
    std::map<int, int> shape_of_tmpl;
    for (int g = 0; g < ss->n_groups; ++g) {
      const int t = e->group_tmpl[ss->group_base + g];
      auto it = shape_of_tmpl.find(t);
      if (it == shape_of_tmpl.end()) {
        slab::Shape sh;
        std::string why;
        if (!slab::shape_of_query(e->lp, e->gq[t].qid, e->gq[t], &sh, &why))
          throw Error(SDH_E_UNSUPPORTED, "K_slab shape: " + why);
        it = shape_of_tmpl.emplace(t, (int)ss->shapes.size()).first;
        ss->shapes.push_back(sh);
      }
      ss->group_shape.push_back(it->second);
      ss->group_ew.push_back(ss->shapes[it->second].EW);
      for (int st = 0; st < kg::GMAXSTREAM; ++st) ss->max_na = std::max<int>(ss->max_na, e->gq[t].n_cap[st]);
    }
    const int ns = (int)e->prog.stream_types.size();
    ss->glist.assign(ns, {});
    ss->d_glist.resize(ns);
    for (int g = 0; g < ss->n_groups; ++g)
      for (int st = 0; st < ns && st < kg::GMAXSTREAM; ++st)
        if (ss->shapes[ss->group_shape[g]].proc[st] >= 0) ss->glist[st].push_back(g);
    for (int st = 0; st < ns; ++st) {
      ss->d_glist[st].ensure(std::max<size_t>(1, ss->glist[st].size()));
      if (!ss->glist[st].empty())
        HIPCHK(hipMemcpy(ss->d_glist[st].p, ss->glist[st].data(), ss->glist[st].size() * 4, hipMemcpyHostToDevice));
    }
    ss->d_shapes.ensure(ss->shapes.size());
    HIPCHK(hipMemcpy(ss->d_shapes.p, ss->shapes.data(), ss->shapes.size() * sizeof(slab::Shape), hipMemcpyHostToDevice));
    ss->d_group_shape.ensure(ss->n_groups);
    HIPCHK(hipMemcpy(ss->d_group_shape.p, ss->group_shape.data(), ss->n_groups * 4, hipMemcpyHostToDevice));
    ss->d_group_ew.ensure(ss->n_groups);
    HIPCHK(hipMemcpy(ss->d_group_ew.p, ss->group_ew.data(), ss->n_groups * 4, hipMemcpyHostToDevice));
    if (const char* v = sdh::knob("SDH_SLAB_LDS_WORDS")) ss->lds_words = std::max(64, atoi(v));
    int64_t sub = 1 << 16;  // words per sub-ring; grows on demand (slab_prepare)
    if (const char* v = sdh::knob("SDH_SLAB_SUB_WORDS")) sub = std::max<int64_t>(64, atoll(v));
    slab_init(e, *ss, sub);
    e->ssets.push_back(std::move(ss));
  };
  // K_wave: the unpartitioned count patterns, one set per stream (a set's tables swap together, so all
  // of its queries must run on the same pushes -- those of their stream). The entry layout is the set's
  // widest; a table starts at one page (SDH_KWAVE_CAP: another start, for tests) and grows on overflow
  auto add_wave_sets = [&](const std::vector<int>& members) {
    const int n_streams = (int)e->prog.stream_types.size();
    for (int stream = 0; stream < n_streams; ++stream) {
      auto ws = std::make_unique<sdh_engine::WaveSet>();
      ws->stream = stream;
      for (int qi : members) {
        if (kwave[qi].kind < 0 || e->lp.q[qi].st[0].stream != stream) continue;
        ws->qs.push_back(gidx[qi]);
        ws->cmax = std::max(ws->cmax, kwave[qi].cmax);
        ws->n_e1 = std::max(ws->n_e1, kwave[qi].n_e1);
        ws->n_first = std::max(ws->n_first, kwave[qi].n_first);
        ws->n_last = std::max(ws->n_last, kwave[qi].n_last);
        ws->na = std::max<int>(ws->na, e->gq[gidx[qi]].n_cap[stream]);
      }
      if (ws->qs.empty()) continue;
      if (ws->na > kg::GMAXNA) throw Error(SDH_E_UNSUPPORTED, "K_wave: more captured attributes than GMAXNA");
      ws->ew = 3 + ws->cmax + ws->n_e1 + ws->n_first + ws->n_last;
      if (const char* v = sdh::knob("SDH_KWAVE_CAP")) ws->cap = std::max(64, (atoi(v) + 63) / 64 * 64);
      ws->d_qs.ensure(ws->qs.size());
      HIPCHK(hipMemcpy(ws->d_qs.p, ws->qs.data(), ws->qs.size() * 4, hipMemcpyHostToDevice));
      const size_t words = ws->qs.size() * (size_t)ws->stride();
      for (auto& b : ws->st) {
        b.ensure(words);
        HIPCHK(hipMemset(b.p, 0, words * 8));
      }
      e->wsets.push_back(std::move(ws));
    }
  };
  // sets: the unpartitioned queries, then one per partition; 64 queries per group (wave)
  auto add_set = [&](int partition, const std::vector<int>& members) {
    if (members.empty()) return;
    std::vector<int> gen_m;
    for (int qi : members)
      if (kpart[qi].kind < 0 && !is_slab[qi] && kwave[qi].kind < 0) gen_m.push_back(qi);
    if (partition < 0) add_wave_sets(members);
    if (partition >= 0) add_part_sets(partition, members);
    if (partition >= 0) add_slab_set(partition, members);
    if (gen_m.empty()) return;
    auto gs = std::make_unique<sdh_engine::GenSet>();
    gs->partition = partition;
    gs->group_base = (int)(e->lane_q.size() / 64);
    // one shape per group: members are bucketed by kg::shape_of (first-appearance order) and each
    // bucket is padded to whole groups, so a wave's control flow is its template's. Lane order is
    // free: matches are ordered by (seq, out_rank, emission index) in the device match table.
    gs->n_groups = add_groups(gen_m, partition < 0);
    for (int g = 0; g < gs->n_groups; ++g) gs->timed |= e->gq[e->group_tmpl[gs->group_base + g]].lay.TQ > 0;
    const size_t per_block32 = (size_t)e->gB32 * 64, per_block64 = (size_t)e->gB64 * 64;
    if (partition < 0) {
      gs->a32.ensure(per_block32 * gs->n_groups);
      gs->a64.ensure(per_block64 * gs->n_groups);
      HIPCHK(hipMemset(gs->a32.p, 0, per_block32 * gs->n_groups * 4));
      HIPCHK(hipMemset(gs->a64.p, 0, per_block64 * gs->n_groups * 8));
    } else {
      route_of(partition);
      gs->key_cap = 0;
    }
    e->gsets.push_back(std::move(gs));
  };
  std::vector<int> top;
  for (int qi : qis)
    if (e->lp.q[qi].partition < 0) top.push_back(qi);
  add_set(-1, top);
  for (int pi = 0; pi < (int)e->lp.parts.size(); ++pi) {
    // lanes in definition order, not the partition's receiver order (LPart::queries is the
    // metaQueryRuntimeMap order, which scatters a family's neighbouring queries): lane order is free
    // (the match table orders rows by rank), and neighbouring definitions share a wave's control
    // flow more often (C3: 20.9 ms/step in receiver order)
    std::vector<int> m;
    for (int qi : e->lp.parts[pi].queries)
      if (gidx[qi] >= 0) m.push_back(qi);
    std::sort(m.begin(), m.end());
    add_set(pi, m);
  }
  // which plan runs each query (what an interleaved push's eligibility asks, mix_plan.h)
  e->gq_kind.assign(e->gq.size(), 0);
  auto kind_groups = [&](int group_base, int n_groups, uint32_t kind, uint32_t seq_kind) {
    for (int g = group_base; g < group_base + n_groups; ++g)
      for (int l = 0; l < 64; ++l)
        if (e->lane_q[(size_t)g * 64 + l] >= 0) e->gq_kind[e->lane_q[(size_t)g * 64 + l]] = e->group_seq[g] > 0 ? seq_kind : kind;
  };
  for (const auto& gs : e->gsets)
    kind_groups(gs->group_base, gs->n_groups, gs->partition < 0 ? mixplan::C_GEN : mixplan::C_GEN_PART,
                gs->partition < 0 ? mixplan::C_SEQ : mixplan::C_GEN_PART);
  for (const auto& ps : e->psets) kind_groups(ps->group_base, ps->n_groups, mixplan::C_PART, mixplan::C_PART);
  for (const auto& ss : e->ssets) kind_groups(ss->group_base, ss->n_groups, mixplan::C_SLAB, mixplan::C_SLAB);
  for (const auto& ws : e->wsets)
    for (int gx : ws->qs) e->gq_kind[gx] = mixplan::C_WAVE;
  e->d_gq.ensure(e->gq.size());
  HIPCHK(hipMemcpy(e->d_gq.p, e->gq.data(), e->gq.size() * sizeof(kg::GQuery), hipMemcpyHostToDevice));
  // the groups' lane-constant table (kg::LaneConsts): [group][slot][64], slot 0 query id, 1 within,
  // 2 + k the k-th CONST instruction of the group's shape; idle lanes repeat the template's values
  {
    const size_t n_groups = e->group_tmpl.size();
    int slots = kg::LC_FIRST;
    std::vector<std::vector<int>> pcs(n_groups);
    for (size_t g = 0; g < n_groups; ++g) {
      const kg::GQuery& t = e->gq[e->group_tmpl[g]];
      for (int pc = 0; pc < t.n_code; ++pc)
        if (t.code[pc].op == kg::OP_CONST) pcs[g].push_back(pc);
      slots = std::max(slots, kg::LC_FIRST + (int)pcs[g].size());
    }
    std::vector<int64_t> lc(std::max<size_t>(1, n_groups * slots * 64), 0);
    for (size_t g = 0; g < n_groups; ++g)
      for (int l = 0; l < 64; ++l) {
        const int qi = e->lane_q[g * 64 + l];
        const kg::GQuery& x = e->gq[qi >= 0 ? qi : e->group_tmpl[g]];
        int64_t* row = lc.data() + g * slots * 64 + l;
        row[kg::LC_QID * 64] = x.qid;
        row[kg::LC_WITHIN * 64] = x.within;
        for (size_t k = 0; k < pcs[g].size(); ++k) row[(kg::LC_FIRST + k) * 64] = x.code[pcs[g][k]].imm;
      }
    e->lc_slots = slots;
    e->d_lconst.ensure(lc.size());
    HIPCHK(hipMemcpy(e->d_lconst.p, lc.data(), lc.size() * 8, hipMemcpyHostToDevice));
  }
  e->d_lane_q.ensure(e->lane_q.size());
  HIPCHK(hipMemcpy(e->d_lane_q.p, e->lane_q.data(), e->lane_q.size() * 4, hipMemcpyHostToDevice));
  e->seq_tail.resize(e->prog.stream_types.size());
  e->seq_tail_len.assign(e->prog.stream_types.size(), 0);
  for (auto& t : e->seq_tail) {
    t.ensure(SEQ_TMAX * SEQ_TW);
    HIPCHK(hipMemset(t.p, 0, SEQ_TMAX * SEQ_TW * 8));
  }
  e->d_glists.resize(e->prog.stream_types.size() + 1);
  spec_build(e);
  e->d_group_tmpl.ensure(e->group_tmpl.size());
  HIPCHK(hipMemcpy(e->d_group_tmpl.p, e->group_tmpl.data(), e->group_tmpl.size() * 4, hipMemcpyHostToDevice));
  e->g_out_next.ensure(1);
  e->g_nrec.ensure(1);
  e->d_perr.ensure(std::max<size_t>(1, e->psets.size()) * 4);
  e->d_serr.ensure(std::max<size_t>(1, e->ssets.size()) * 4);
  e->d_werr.ensure(std::max<size_t>(1, e->wsets.size()) * 4);
  if (!e->wsets.empty()) {
    e->d_wave_live.ensure(1);
    const int64_t none = -1;
    e->d_wave_key.ensure(1);
    HIPCHK(hipMemcpy(e->d_wave_key.p, &none, 8, hipMemcpyHostToDevice));
  }
}

// grow a partition set's instance arena to hold `keys` keys (blocks are key-major: a prefix copy)
void gen_grow(sdh_engine* e, sdh_engine::GenSet& gs, int64_t keys) {
  if (keys <= gs.key_cap) return;
  int64_t cap = std::max<int64_t>(64, gs.key_cap);
  while (cap < keys) cap *= 2;
  const size_t b32 = (size_t)e->gB32 * 64 * gs.n_groups, b64 = (size_t)e->gB64 * 64 * gs.n_groups;
  DevBuf<int32_t> n32;
  DevBuf<int64_t> n64;
  n32.ensure(b32 * cap);
  n64.ensure(b64 * cap);
  HIPCHK(hipMemsetAsync(n32.p, 0, b32 * cap * 4, e->stream));
  HIPCHK(hipMemsetAsync(n64.p, 0, b64 * cap * 8, e->stream));
  if (gs.key_cap > 0) {
    HIPCHK(hipMemcpyAsync(n32.p, gs.a32.p, b32 * gs.key_cap * 4, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(n64.p, gs.a64.p, b64 * gs.key_cap * 8, hipMemcpyDeviceToDevice, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  gs.a32.swap(n32);
  gs.a64.swap(n64);
  gs.key_cap = cap;
}

// K_gen pools and lists at a new sizing: every query's layout is recomputed (make_layout) and each
// set's arenas are re-laid on the device (gen_remap_kernel; remap = false: zeroed, the caller
// overwrites them). Pools only grow between pushes, so the indices the arenas hold stay valid.
void gen_relayout(sdh_engine* e, const kg::Sizing& sz, bool remap) {
  if (7 + kg::GMAXS + sz.N > GEN_RING_MARGIN) throw Error(SDH_E_CAPACITY, "K_gen node pool beyond the match-record limit");
  std::vector<kg::GLayout> oldL(e->gq.size()), newL(e->gq.size());
  int b32 = 1, b64 = 1, hot_nu = 1;
  for (size_t i = 0; i < e->gq.size(); ++i) {
    kg::GQuery& g = e->gq[i];
    oldL[i] = g.lay;
    kg::make_layout(g.lay, g.lay.S, sz.R, sz.N, sz.LC, g.lay.NA, g.lay.v32 != 0, g.lay.TQ > 0 ? sz.LC : 0);
    newL[i] = g.lay;
    if (!e->gq_arena[i]) continue;
    b32 = std::max(b32, g.lay.n32);
    b64 = std::max(b64, g.lay.n64);
    if (!g.lay.big) hot_nu = std::max(hot_nu, g.lay.NU);
  }
  DevBuf<kg::GLayout> dOld, dNew;
  dOld.ensure(oldL.size());
  dNew.ensure(newL.size());
  HIPCHK(hipMemcpy(dOld.p, oldL.data(), oldL.size() * sizeof(kg::GLayout), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dNew.p, newL.data(), newL.size() * sizeof(kg::GLayout), hipMemcpyHostToDevice));
  for (auto& up : e->gsets) {
    auto& gs = *up;
    const int64_t blocks = gs.partition < 0 ? gs.n_groups : gs.key_cap * gs.n_groups;
    DevBuf<int32_t> n32;
    DevBuf<int64_t> n64;
    n32.ensure(std::max<size_t>(1, (size_t)blocks * b32 * 64));
    n64.ensure(std::max<size_t>(1, (size_t)blocks * b64 * 64));
    HIPCHK(hipMemsetAsync(n32.p, 0, n32.n * 4, e->stream));
    HIPCHK(hipMemsetAsync(n64.p, 0, n64.n * 8, e->stream));
    if (remap)
      HIPCHK(sdh_gen_remap(e->d_lane_q.p, gs.group_base, gs.n_groups, blocks, dOld.p, dNew.p, gs.a32.p, gs.a64.p,
                           e->gB32, e->gB64, n32.p, n64.p, b32, b64, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    gs.a32.swap(n32);
    gs.a64.swap(n64);
  }
  e->gB32 = b32;
  e->gB64 = b64;
  e->gHotNU = hot_nu;
  e->gsz = sz;
  HIPCHK(hipMemcpy(e->d_gq.p, e->gq.data(), e->gq.size() * sizeof(kg::GQuery), hipMemcpyHostToDevice));
}

// A push on a stream that fans out to every key of a string-keyed partition needs the text hash of
// every key it will reach (fan_positions). Checked before any kernel runs, so a missing
// sdh_engine_set_strings (e.g. after sdh_engine_restore) fails the push with SDH_E_INVALID and leaves
// the engine usable. (A push on the keyed stream creates keys but reaches no fan-out position.)
void check_fan_strings(const sdh_engine* e, int stream) {
  for (size_t pi = 0; pi < e->lp.parts.size() && pi < e->routes.size(); ++pi) {
    const sdh_engine::Route* rt = e->routes[pi].get();
    if (!rt || !rt->track || rt->kkind != 2 || !e->lp.parts[pi].fan(stream)) continue;
    for (int64_t k : rt->korder_key)
      if (e->str_info.find((int32_t)k) == e->str_info.end())
        throw Error(SDH_E_INVALID, fmt("partition key string id %lld has no text hash (sdh_engine_set_strings)", (long long)k));
  }
}

// Upper bound of the journal bytes a push of n events over `stream` needs; do_push splits a batch
// whose bound does not fit a third of free HBM
double gen_journal_bound(sdh_engine* e, int64_t n) {
  double blocks = 0;
  for (auto& gs : e->gsets)  // an unpartitioned set's groups; the pushed keys' blocks, a timer sweep every known key's
    blocks += (double)gs->n_groups * (gs->partition < 0 ? 1.0 : (double)(gs->timed ? gs->key_cap + n : n));
  return blocks * ((double)e->gB32 * 64 * 4 + (double)e->gB64 * 64 * 8);
}

// K_part state: room for `keys` keys (new keys' blocks start empty: n = 0, buffer 0)
void part_grow(sdh_engine* e, sdh_engine::PartSet& ps, int64_t keys) {
  if (keys <= ps.key_cap) return;
  int64_t cap = std::max<int64_t>(64, ps.key_cap);
  while (cap < keys) cap *= 2;
  const size_t per_key = (size_t)ps.n_groups * ps.bw() * 64;  // int64 words per key and buffer
  DevBuf<int64_t> nst;
  DevBuf<int32_t> ncur, nnxt;
  nst.ensure(2 * per_key * cap);
  ncur.ensure(cap);
  nnxt.ensure(cap);
  HIPCHK(hipMemsetAsync(nst.p, 0, 2 * per_key * cap * 8, e->stream));
  HIPCHK(hipMemsetAsync(ncur.p, 0, cap * 4, e->stream));
  if (ps.key_cap > 0)
    for (int b = 0; b < 2; ++b)
      HIPCHK(hipMemcpyAsync(nst.p + b * per_key * cap, ps.st.p + b * per_key * ps.key_cap, per_key * ps.key_cap * 8,
                            hipMemcpyDeviceToDevice, e->stream));
  if (ps.key_cap > 0) HIPCHK(hipMemcpyAsync(ncur.p, ps.cur.p, ps.key_cap * 4, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  ps.st.swap(nst);
  ps.cur.swap(ncur);
  ps.nxt.swap(nnxt);
  ps.key_cap = cap;
}

namespace {

// the most partials one K_wave query holds (K_part's limit is 65,536 per instance)
constexpr int WAVE_MAX_CAP = 1 << 20;

// the sizing after a K_gen capacity failure of kinds `capk` (kg::CAP_*): each limit hit doubles
bool gen_grown_sizing(const sdh_engine* e, int capk, kg::Sizing* out) {
  kg::Sizing sz = e->gsz;
  if (capk & kg::CAP_FIXED) return false;
  if (capk & kg::CAP_STATES) sz.R = std::min(kg::GMAXPOOL, 2 * sz.R);
  if (capk & kg::CAP_NODES) sz.N = std::min(kg::GMAXPOOL, 2 * sz.N);
  if (capk & kg::CAP_LIST) sz.LC = std::min(1 << 16, 2 * sz.LC);
  if (sz.R == e->gsz.R && sz.N == e->gsz.N && sz.LC == e->gsz.LC) return false;
  *out = sz;
  return true;
}

// Exact re-runs (the reference never drops a match): just before a K_gen launch modifies a set's
// arena blocks, they are journaled (gen_journal_kernel); a pass whose match output, pools, K_part
// tables or K_slab space overflowed is undone by copying them back, and re-run at the grown size.
// The journal holds the blocks of this pass only -- the set's groups (unpartitioned), the pushed
// keys' blocks (partitions), every known key's (a timer sweep) -- so its cost scales with the push,
// not with the total state. mode / glist / seg_kid: as gen_journal_kernel.
void gen_journal(sdh_engine* e, sdh_engine::GenSet& gs, int mode, const int32_t* glist, const uint32_t* seg_kid,
                 int64_t slots) {
  gs.jn = 0;
  if (!e->g_journal || slots <= 0) return;
  const size_t b32 = (size_t)e->gB32 * 64, b64 = (size_t)e->gB64 * 64;
  gs.j32.ensure(b32 * slots);
  gs.j64.ensure(b64 * slots);
  gs.jidx.ensure((size_t)slots);
  HIPCHK(sdh_gen_journal(gs.a32.p, gs.a64.p, e->gB32, e->gB64, mode, glist, seg_kid, gs.n_groups, slots, gs.j32.p,
                         gs.j64.p, gs.jidx.p, 0, e->stream));
  gs.jn = slots;
}

void gen_restore_journal(sdh_engine* e) {
  for (auto& up : e->gsets) {
    auto& gs = *up;
    if (gs.jn > 0)
      HIPCHK(sdh_gen_journal(gs.a32.p, gs.a64.p, e->gB32, e->gB64, 0, nullptr, nullptr, gs.n_groups, gs.jn, gs.j32.p,
                             gs.j64.p, gs.jidx.p, 1, e->stream));
    gs.jn = 0;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
}

// K_part entry capacity x2: every block keeps its header and entries at the same word offsets
void part_grow_cap(sdh_engine* e, sdh_engine::PartSet& ps) {
  const int64_t blocks = 2 * ps.key_cap * ps.n_groups, obw = ps.bw();
  ps.cap *= 2;
  if (ps.key_cap == 0) return;
  const int64_t nbw = ps.bw();
  DevBuf<int64_t> nst;
  nst.ensure((size_t)(blocks * nbw * 64));
  HIPCHK(hipMemsetAsync(nst.p, 0, (size_t)blocks * nbw * 64 * 8, e->stream));
  HIPCHK(hipMemcpy2DAsync(nst.p, (size_t)nbw * 64 * 8, ps.st.p, (size_t)obw * 64 * 8, (size_t)obw * 64 * 8, (size_t)blocks,
                          hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  ps.st.swap(nst);
}

// K_wave tables at `cap` entries: every table keeps its header and pages at the same word offsets
// (pages are page-major: a prefix copy per table). HBM exhaustion is SDH_E_CAPACITY, as elsewhere
void wave_grow_cap(sdh_engine* e, sdh_engine::WaveSet& ws, int cap) {
  const int64_t ostride = ws.stride();
  const size_t nq = ws.qs.size();
  ws.cap = cap;
  const int64_t nstride = ws.stride();
  for (auto& b : ws.st) {
    int64_t* q = nullptr;
    if (hipMalloc(&q, nq * (size_t)nstride * 8) != hipSuccess) {
      (void)hipGetLastError();
      throw Error(SDH_E_CAPACITY, fmt("device memory exhausted growing the K_wave tables to %d partials per query", cap));
    }
    DevBuf<int64_t> nb;
    nb.p = q;
    nb.n = nq * (size_t)nstride;
    HIPCHK(hipMemsetAsync(nb.p, 0, nb.n * 8, e->stream));
    HIPCHK(hipMemcpy2DAsync(nb.p, (size_t)nstride * 8, b.p, (size_t)ostride * 8, (size_t)ostride * 8, nq,
                            hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    b.swap(nb);
  }
}

// keys this push created (ids [nk_seen, new_n)), in the order of their first events: the order
// PartitionRuntime.clonePartition adds them to every receiver's junction map
void track_new_keys(sdh_engine* e, sdh_engine::Route& rt, int64_t new_n, int64_t nruns, int kkind) {
  const int64_t m = new_n - rt.nk_seen;
  rt.nk_tmp.ensure((size_t)(2 * m));
  HIPCHK(sdh_new_keys(e->r_uniq.p, e->r_nruns.p, nruns, e->r_off.p, e->r_idx_s.p, rt.key_of_id.p, rt.nk_seen, new_n,
                      rt.nk_tmp.p, e->stream));
  std::vector<int64_t> v((size_t)(2 * m));
  HIPCHK(hipMemcpyAsync(v.data(), rt.nk_tmp.p, v.size() * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<int64_t> ord((size_t)m);
  for (int64_t k = 0; k < m; ++k) ord[(size_t)k] = k;
  std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return v[(size_t)(2 * a)] < v[(size_t)(2 * b)]; });
  for (int64_t k : ord) {
    rt.korder_kid.push_back(rt.nk_seen + k);
    rt.korder_key.push_back(v[(size_t)(2 * k + 1)]);
  }
  rt.kkind = kkind;
  rt.nk_seen = new_n;
}

// per known key its position in the fan-out stream's junction map of "streamId + key" strings
// (chm_order.h), on the device; rebuilt when keys were added
const int32_t* fan_positions(sdh_engine* e, sdh_engine::Route& rt, const kg::LFanOut& fo, int64_t nk) {
  auto& f = rt.fan[fo.stream];
  if (f.n != nk) {
    const size_t m = std::min<size_t>((size_t)nk, rt.korder_key.size());
    std::vector<int32_t> hs(m), byk((size_t)std::max<int64_t>(1, nk), 0);
    for (size_t j = 0; j < m; ++j) {
      const int64_t k = rt.korder_key[j];
      if (rt.kkind == 2) {  // String.valueOf of a string is its text: its registered hash and length
        auto it = e->str_info.find((int32_t)k);
        if (it == e->str_info.end())
          throw Error(SDH_E_INVALID, fmt("partition key string id %lld has no text hash (sdh_engine_set_strings)", (long long)k));
        hs[j] = sdh::java_hash_cat_hashed(fo.id_hash, it->second.first, it->second.second);
      } else if (rt.kkind == 3 || rt.kkind == 4) {  // Float / Double.toString (java_fmt.h)
        hs[j] = sdh::java_hash_cat(fo.id_hash, rt.kkind == 3 ? sdh::jfmt::float_to_string((uint32_t)k)
                                                             : sdh::jfmt::double_to_string((uint64_t)k));
      } else {
        hs[j] = sdh::java_hash_cat(fo.id_hash, sdh::java_value_of(rt.kkind == 1, k));
      }
    }
    const std::vector<int32_t> pos = sdh::ChmOrder().positions(hs);
    for (size_t j = 0; j < m; ++j) byk[(size_t)rt.korder_kid[j]] = pos[j];
    f.pos.ensure(byk.size());
    HIPCHK(hipMemcpy(f.pos.p, byk.data(), byk.size() * 4, hipMemcpyHostToDevice));
    f.n = nk;
  }
  return f.pos.p;
}

// ---- the launch-argument groups (nfa_types.h), one filler each; a record has at least NREC_MIN_WORDS words ----
int64_t rec_cap_of(const sdh_engine* e) { return e->g_out_cap / NREC_MIN_WORDS + 1; }

sdh::RecordSink sink_of(const sdh_engine* e, bool write) {
  return {e->g_out.p,     e->g_out_cap,  e->g_out_next.p, e->g_nrec.p,
          e->g_rec_off.p, rec_cap_of(e), e->g_rec_next.p, write ? 1 : 2};
}

sdh::GroupTables tables_of(const sdh_engine* e) {
  return {e->d_gq.p, e->d_lane_q.p, e->d_group_tmpl.p, e->d_lconst.p, e->lc_slots};
}

// the segments sdh_route_partition left for the batch, with the partition's key table
sdh::KeySegments segments_of(const sdh_engine* e, const sdh_engine::Route& rt) {
  return {e->r_off.p, e->r_cnt.p, e->r_uniq.p, rt.key_of_id.p, e->r_idx_s.p};
}

// what the steps of one pass share
struct Pass {
  sdh_engine* e;
  int stream;
  const StreamBatch& B;
  bool write;
  int64_t ev_bytes;           // bytes of one event: its timestamp and attribute words
  double bytes = 0;           // running: the HBM traffic the launches are modelled to move
  bool any = false;           // running: something ran
  int32_t tail_new_len = -1;  // the stream's K_seq tail length once the pass is accepted (-1: no K_seq launch)
};

// a shape-compiled kernel (spec.h) over `items` one-wave work groups; per-XCD item ranges pad the grid
// to a multiple of 8 (dev::grid_item)
template <class Launch>
void launch_spec(sdh_engine* e, hipFunction_t f, Launch& L, int64_t items) {
  void* args[] = {&L};
  HIPCHK(hipModuleLaunchKernel(f, (unsigned)(L.xcd ? (items + 7) & ~7ll : items), 1, 1, 64, 1, 1, 0, e->stream, args,
                               nullptr));
}

// what every K_gen launch of a set shares (the set's arenas as they are now: grow them first)
sdh::GenLaunch gen_launch_of(const Pass& p, const sdh_engine::GenSet& gs) {
  const sdh_engine* e = p.e;
  sdh::GenLaunch L{};
  L.tab = tables_of(e);
  L.b = p.B;
  L.groups = gs.n_groups;
  L.group_base = gs.group_base;
  L.a32 = gs.a32.p;
  L.a64 = gs.a64.p;
  L.B32 = e->gB32;
  L.B64 = e->gB64;
  L.hot_s = e->gHotS;
  L.hot_nu = e->gHotNU;
  L.sink = sink_of(e, p.write);
  L.err = e->d_err.p;
  L.start_ts = e->start_ts;
  L.advance_to = e->advance_to;
  L.timer_seq = e->seq + p.B.n;
  L.playback = (e->cfg.flags & SDH_FLAG_PLAYBACK) ? 1 : 0;
  L.no_timers = e->ck.active ? 1 : 0;
  L.xcd = e->xcd;
  return L;
}

// K_seq: one launch per shape (rows of one shape are contiguous), its compiled kernel if any
void seq_launches(Pass& p, const int32_t* glist, const std::vector<int32_t>& seq_rows) {
  sdh_engine* e = p.e;
  const int64_t n = p.B.n;
  for (size_t r0 = 0, r1 = 0; r0 < seq_rows.size(); r0 = r1) {
    const int tmpl = e->group_tmpl[seq_rows[r0]];
    for (r1 = r0 + 1; r1 < seq_rows.size() && e->group_tmpl[seq_rows[r1]] == tmpl;) ++r1;
    const int nrows = (int)(r1 - r0);
    sdh::SeqLaunch Q{};
    Q.xcd = e->xcd;
    Q.tab = tables_of(e);
    Q.glist = glist + r0;
    Q.n_glist = nrows;
    Q.b = p.B;
    Q.tail = e->seq_tail[p.stream].p;
    Q.tail_len = e->seq_tail_len[p.stream];
    Q.sink = sink_of(e, p.write);
    Q.err = e->d_err.p;
    const int64_t starts = n + Q.tail_len;
    // items per launch: many short chunks balance the chunks' uneven match density (C4 sweep,
    // tools/sweep_seq.sh: 4,096 items 25.2 ms/step, 8,192 19.8, 16,384 17.2, 32,768 16.2, 65,536
    // 15.8, 131,072 15.5)
    const int64_t seq_waves = sdh::knob("SDH_SEQ_WAVES") ? atoll(sdh::knob("SDH_SEQ_WAVES")) : 131072;
    const int64_t target = std::max<int64_t>(1, seq_waves / (int64_t)nrows);
    int64_t clen = std::max<int64_t>(256, (starts + target - 1) / target);
    clen = (clen + 63) / 64 * 64;  // whole LDS tiles
    Q.chunk_len = clen;
    Q.n_chunks = (int32_t)((starts + clen - 1) / clen);
    const int64_t items = (int64_t)Q.n_glist * Q.n_chunks;
    auto sp = e->seq_spec.find(tmpl);
    if (sp != e->seq_spec.end()) launch_spec(e, sp->second, Q, items);
    else HIPCHK(sdh_launch_seq(&Q, e->stream));
    p.tail_new_len = (int32_t)std::min<int64_t>(SEQ_TMAX, Q.tail_len + n);
    e->stats.last_seq_items += items;
    p.any = true;
    p.bytes += (double)n * p.ev_bytes * nrows;  // every group stages the batch once
  }
}

// K_gen over the set-relative groups `gen_groups` of an unpartitioned set (glist: the same on the
// device), in event chunks when every group's shape has a bounded look-back (kg::seq_lookback): chunk
// c > 0 rebuilds its instances from a few replayed events, so one set fills the chip
void gen_chunked(Pass& p, sdh_engine::GenSet& gs, const int32_t* glist, const std::vector<int32_t>& gen_groups) {
  sdh_engine* e = p.e;
  const int64_t n = p.B.n;
  sdh::GenLaunch L = gen_launch_of(p, gs);
  L.glist = glist;
  L.n_glist = (int32_t)gen_groups.size();
  int look = 0;
  for (int g : gen_groups) {
    const int lb = kg::seq_lookback(e->gq[e->group_tmpl[gs.group_base + g]]);
    look = lb < 0 ? -1 : std::max(look, lb);
    if (look < 0) break;
  }
  int64_t C = 1, clen = n;
  if (look >= 0 && n > 0) {
    int64_t minlen = std::max<int64_t>(256, 8 * look);
    if (const char* v = sdh::knob("SDH_GEN_CHUNK_LEN")) minlen = std::max<int64_t>(std::max(1, look), atoll(v));
    const int64_t target = std::max<int64_t>(1, 8192 / (int64_t)gen_groups.size());
    C = std::max<int64_t>(1, std::min<int64_t>((n + minlen - 1) / minlen, target));
    clen = (n + C - 1) / C;
    C = (n + clen - 1) / clen;
  }
  L.n_items = (int32_t)(C * gen_groups.size());
  L.ev_chunks = (int32_t)C;
  L.chunk_len = clen;
  const size_t blk32 = (size_t)e->gB32 * 64, blk64 = (size_t)e->gB64 * 64;
  if (C > 1) {
    gs.s32.ensure(blk32 * gs.n_groups * (C - 1));  // (indexed by set-relative group)
    gs.s64.ensure(blk64 * gs.n_groups * (C - 1));
    L.s32 = gs.s32.p;
    L.s64 = gs.s64.p;
  }
  gen_journal(e, gs, 0, L.glist, nullptr, (int64_t)gen_groups.size());
  HIPCHK(sdh_launch_gen(&L, e->stream));
  e->stats.last_gen_items += L.n_items;
  if (C > 1) {  // the last chunk's instances are the set's state after this batch
    for (int g : gen_groups) {
      const size_t sb = (size_t)(C - 2) * gs.n_groups + g;
      HIPCHK(hipMemcpyAsync(gs.a32.p + g * blk32, gs.s32.p + sb * blk32, blk32 * 4, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(gs.a64.p + g * blk64, gs.s64.p + sb * blk64, blk64 * 8, hipMemcpyDeviceToDevice, e->stream));
    }
  }
  p.any = true;
  p.bytes += (double)n * p.ev_bytes * gen_groups.size();  // every group streams the batch once
}

// an interleaved push (e->mix): one K_gen launch over the merged batch, one item per
// group whose shape reads a stream of the call (e->mix_mask). No event chunks: kg::seq_lookback needs
// one input stream. The list depends on the call's streams only: cached by their mask
void unpartitioned_mixed(Pass& p, sdh_engine::GenSet& gs) {
  sdh_engine* e = p.e;
  std::vector<int32_t> gen_groups;
  int na = 1;
  for (int g = 0; g < gs.n_groups; ++g) {
    const kg::GQuery& tq = e->gq[e->group_tmpl[gs.group_base + g]];
    bool reads = false;
    for (int s = 0; s < kg::GMAXSTREAM; ++s)
      if ((e->mix_mask >> s & 1) && tq.recv_n[s] > 0) {
        reads = true;
        na = std::max<int>(na, tq.n_cap[s]);
      }
    // (a K_seq group that reads a named stream keeps the call off this path: mix_plan.h)
    if (reads && e->group_seq[gs.group_base + g] == 0) gen_groups.push_back(g);
  }
  if (gen_groups.empty()) return;
  auto& gl = gs.mix_glists[e->mix_mask];
  if (!gl.p) {
    gl.ensure(gen_groups.size());
    HIPCHK(hipMemcpy(gl.p, gen_groups.data(), gen_groups.size() * 4, hipMemcpyHostToDevice));
  }
  sdh::GenLaunch L = gen_launch_of(p, gs);
  L.glist = gl.p;
  L.n_glist = (int32_t)gen_groups.size();
  L.n_items = L.n_glist;
  L.ev_chunks = 1;
  L.chunk_len = p.B.n;
  L.no_timers = 1;  // (no set of a native call has absent states)
  L.mix = e->mix;
  L.mix_na = na;
  L.mix_tile = 64;
  // (measurements: a tile of one event is the unstaged walk, two dependent loads ahead of every event)
  if (const char* v = sdh::knob("SDH_MIX_GEN_TILE")) {
    int t = 1;
    while (2 * t <= std::min(64, std::max(1, atoi(v)))) t *= 2;
    L.mix_tile = t;
  }
  gen_journal(e, gs, 0, L.glist, nullptr, (int64_t)gen_groups.size());
  HIPCHK(sdh_launch_gen(&L, e->stream));
  e->stats.last_gen_items += L.n_items;
  p.any = true;
  // every group reads order / idx / ts and a captured word or two per event
  p.bytes += (double)p.B.n * (16 + 8.0 * na) * gen_groups.size();
}

// an unpartitioned set: of its groups reading this stream, windowed sequences go to K_seq, the rest
// to K_gen
void unpartitioned_pass(Pass& p, sdh_engine::GenSet& gs) {
  sdh_engine* e = p.e;
  if (e->mix) return unpartitioned_mixed(p, gs);
  const int64_t n = p.B.n;
  std::vector<int32_t> seq_rows, gen_groups;
  for (int g = 0; g < gs.n_groups; ++g) {
    const kg::GQuery& tq = e->gq[e->group_tmpl[gs.group_base + g]];
    const bool timed = tq.lay.TQ > 0;  // absent states: time passes on every push and advance
    if (n == 0 ? !timed : (tq.recv_n[p.stream] == 0 && !timed)) continue;
    if (e->group_seq[gs.group_base + g] > 0) seq_rows.push_back(gs.group_base + g);
    else gen_groups.push_back(g);
  }
  if (seq_rows.empty() && gen_groups.empty()) return;
  // the lists depend on the stream only: uploaded once, before any kernel reads them
  // (one cached list per stream, and one more for time advances: B.n == 0)
  auto& gl = e->d_glists[n == 0 ? e->prog.stream_types.size() : (size_t)p.stream];
  if (!gl.p) {
    gl.ensure(std::max<size_t>(1, seq_rows.size() + gen_groups.size()));
    std::vector<int32_t> both(seq_rows);
    both.insert(both.end(), gen_groups.begin(), gen_groups.end());
    if (!both.empty()) HIPCHK(hipMemcpy(gl.p, both.data(), both.size() * 4, hipMemcpyHostToDevice));
  }
  seq_launches(p, gl.p, seq_rows);
  if (!gen_groups.empty()) gen_chunked(p, gs, gl.p + seq_rows.size(), gen_groups);
}

// whether the batch's timestamps are ordered (and leaves their prefix max in t_pm): an ordered batch
// takes the indexed sweep (each key walks its own events; its timers fire at the first event whose
// time reaches them, found by binary search), else every key walks the batch
bool batch_ordered(const Pass& p) {
  sdh_engine* e = p.e;
  const int64_t n = p.B.n;
  if (n <= 0 || sdh::knob("SDH_NO_TIMER_INDEX")) return false;
  e->t_pm.ensure((size_t)n);
  e->t_flag.ensure(1);
  e->t_temp.ensure(sdh_prefix_max_temp_bytes(n));
  HIPCHK(sdh_prefix_max(p.B.ts, n, e->t_pm.p, e->t_flag.p, e->t_temp.p, e->t_temp.n, e->stream));
  int32_t un = 1;
  d2h_sync(e, &un, e->t_flag.p, 4);
  return un == 0;
}

// the timer sweep of a partition's K_gen set over its n_keys known keys (GenLaunch::sweep). ev_kid: each
// routed event's key id (nullptr: no event is any key's own, or with fan_pos every key's); indexed: the
// batch is ordered (batch_ordered ran)
void gen_sweep(Pass& p, sdh_engine::GenSet& gs, const sdh_engine::Route& rt, const uint32_t* ev_kid, int64_t n_keys,
               bool indexed, const int32_t* fan_pos = nullptr) {
  sdh_engine* e = p.e;
  const int64_t n = p.B.n;
  sdh::GenLaunch L = gen_launch_of(p, gs);
  L.keys.key_of_id = rt.key_of_id.p;
  L.sweep = 1;
  L.ev_kid = ev_kid;
  L.n_keys = n_keys;
  L.fan_pos = fan_pos;
  if (indexed) {
    L.pm = e->t_pm.p;
    if (ev_kid) {  // the keys' own events: the routed segments
      e->t_kseg.ensure((size_t)std::max<int64_t>(1, n_keys));
      HIPCHK(sdh_key_segments(e->r_uniq.p, e->r_nruns.p, n, n_keys, e->t_kseg.p, e->stream));
      L.kseg = e->t_kseg.p;
      L.keys = segments_of(e, rt);
    }
  }
  L.n_items = (int32_t)(n_keys * gs.n_groups);
  gen_journal(e, gs, 2, nullptr, nullptr, (int64_t)L.n_items);
  if (L.n_items > 0) HIPCHK(sdh_launch_gen(&L, e->stream));
  e->stats.last_gen_items += L.n_items;
  p.any = true;
  // indexed: each key reads its own events and binary-searches pm per timer stop
  p.bytes += (double)n * p.ev_bytes * gs.n_groups * (indexed ? 1.0 : (double)n_keys);
}

struct Routed {  // what routing a batch tells the host
  int32_t n_keys, n_runs;  // keys the partition knows now; key segments of the batch (dropped events: the last)
};

// dense key ids for the batch's events and the events grouped by key (the r_* buffers), once for
// every set of the partition; keeps part_kept and the keys' creation order (fan-out partitions)
Routed route_batch(Pass& p, int pi, sdh_engine::Route& rt, int attr) {
  sdh_engine* e = p.e;
  const int64_t n = p.B.n;
  const int type = e->lp.stream_types[p.stream][attr];
  e->r_key.ensure(n);
  e->r_kid.ensure(n);
  e->r_kid_s.ensure(n);
  e->r_uniq.ensure(n);
  e->r_idx.ensure(n);
  e->r_idx_s.ensure(n);
  e->r_cnt.ensure(n);
  e->r_off.ensure(n);
  e->r_nruns.ensure(1);
  e->r_temp.ensure(sdh_route_temp_bytes(n));
  HIPCHK(sdh_route_partition(&p.B, attr, type, rt.tkey.p, rt.tid.p, rt.tmask, rt.n_keys.p, rt.key_of_id.p,
                             rt.max_keys, e->r_key.p, e->r_kid.p, e->r_kid_s.p, e->r_idx.p, e->r_idx_s.p,
                             e->r_uniq.p, e->r_cnt.p, e->r_off.p, e->r_nruns.p, e->r_temp.p, e->r_temp.n,
                             e->d_err.p + 3, e->cfg.shard_rank, e->cfg.shard_world, e->stream));
  Routed r{0, 0};
  HIPCHK(hipMemcpyAsync(&r.n_keys, rt.n_keys.p, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&r.n_runs, e->r_nruns.p, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (r.n_keys > rt.max_keys) throw Error(SDH_E_CAPACITY, "more partition keys than gen_max_keys");
  // events this engine keeps (null keys and, with key sharding, other ranks' keys sort last)
  if (r.n_runs > 0) {
    uint32_t last_kid = 0;
    int32_t last_cnt = 0;
    HIPCHK(hipMemcpyAsync(&last_kid, e->r_uniq.p + r.n_runs - 1, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&last_cnt, e->r_cnt.p + r.n_runs - 1, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if ((int)e->part_kept.size() <= pi) e->part_kept.resize(pi + 1, 0);
    e->part_kept[pi] = n - (last_kid == 0xFFFFFFFFu ? last_cnt : 0);
  }
  if (rt.track && r.n_keys > rt.nk_seen)
    track_new_keys(e, rt, r.n_keys, r.n_runs,
                   type == kg::T_BOOL ? 1 : type == kg::T_STRING ? 2 : type == kg::T_FLOAT ? 3 : type == kg::T_DOUBLE ? 4 : 0);
  // routing (key column read, key/kid/idx written and sorted)
  p.bytes += (double)n * (8 + 8 + 4 + 4 + 2 * (4 + 4) + 3 * 4);
  return r;
}

// K_gen over the routed segments: item = (key segment, group)
void gen_keyed(Pass& p, sdh_engine::GenSet& gs, const sdh_engine::Route& rt, Routed r) {
  sdh_engine* e = p.e;
  sdh::GenLaunch L = gen_launch_of(p, gs);
  L.keys = segments_of(e, rt);
  L.n_items = r.n_runs * gs.n_groups;
  gen_journal(e, gs, 1, nullptr, e->r_uniq.p, (int64_t)L.n_items);
  HIPCHK(sdh_launch_gen(&L, e->stream));
  e->stats.last_gen_items += L.n_items;
  p.any = true;
  p.bytes += (double)p.B.n * p.ev_bytes * gs.n_groups;  // every group streams its keys' events
}

// the partition's K_part sets. K_part reads each key's events as one contiguous run of a key-ordered
// copy of the batch (the routing sort's order) instead of gathering them from the batch
void part_sets(Pass& p, int pi, const sdh_engine::Route& rt, Routed r) {
  sdh_engine* e = p.e;
  sdh::StreamBatch SB{};
  bool sorted = false;
  for (size_t si = 0; si < e->psets.size(); ++si) {
    auto& ps = *e->psets[si];
    if (ps.partition != pi || ps.stream != p.stream) continue;
    part_grow(e, ps, r.n_keys);
    if (!sorted && !sdh::knob("SDH_KPART_GATHER")) {
      e->sb_buf.ensure(sdh_sorted_batch_bytes(&p.B));
      HIPCHK(sdh_sort_batch(&p.B, e->r_idx_s.p, e->sb_buf.p, &SB, e->stream));
      sorted = true;
    }
    sdh::PartLaunch P{};
    P.sorted = sorted ? 1 : 0;
    P.xcd = e->xcd;
    P.tab = tables_of(e);
    P.b = sorted ? SB : p.B;
    P.keys = segments_of(e, rt);
    P.groups = ps.n_groups;
    P.group_base = ps.group_base;
    P.kind = ps.kind;
    P.cap = ps.cap;
    P.ew = ps.ew;
    P.sA = ps.sA;
    P.sB = ps.sB;
    P.cmax = ps.cmax;
    P.n_e1 = ps.n_e1;
    P.n_first = ps.n_first;
    P.n_last = ps.n_last;
    P.wide = sdh::knob("SDH_KPART_WIDE") ? 1 : 0;
    P.st = ps.st.p;
    P.blocks = ps.key_cap * ps.n_groups;
    P.cur = ps.cur.p;
    P.nxt = ps.nxt.p;
    P.sink = sink_of(e, p.write);
    if (!p.write && sdh::knob("SDH_DEBUG_COUNT_ONLY")) P.sink.write_records = 0;  // (measurement experiments)
    P.err = e->d_perr.p + 4 * si;
    const bool prof = sdh::knob("SDH_PART_PROF") != nullptr;
    if (prof) {
      e->d_pprof.ensure(8);
      HIPCHK(hipMemsetAsync(e->d_pprof.p, 0, 8 * 8, e->stream));
      P.prof = e->d_pprof.p;
    }
    // the per-key buffer selector of untouched keys carries over
    HIPCHK(hipMemcpyAsync(ps.nxt.p, ps.cur.p, (size_t)ps.key_cap * 4, hipMemcpyDeviceToDevice, e->stream));
    // one launch per shape (its groups are contiguous), the shape-compiled kernel if there is one
    for (int g0 = 0, g1 = 0; g0 < ps.n_groups; g0 = g1) {
      const int tmpl = e->group_tmpl[ps.group_base + g0];
      for (g1 = g0 + 1; g1 < ps.n_groups && e->group_tmpl[ps.group_base + g1] == tmpl;) ++g1;
      P.g0 = g0;
      P.gn = g1 - g0;
      P.n_items = r.n_runs * P.gn;
      auto sp = ps.spec.find(tmpl);
      if (sp == ps.spec.end()) HIPCHK(sdh_launch_part(&P, e->stream));
      else if (P.n_items > 0) launch_spec(e, sp->second, P, P.n_items);
      e->stats.last_part_items += P.n_items;
    }
    if (prof) {  // per-phase clocks of this set's launches (measurement builds, part_body.h)
      unsigned long long h[8];
      d2h_sync(e, h, e->d_pprof.p, 8 * 8);
      const double w = h[5] ? (double)h[5] : 1.0;
      fprintf(stderr, "[part prof] kind %d waves %llu events/wave %.1f cycles/wave: setup %.0f stage %.0f loop %.0f end %.0f\n",
              ps.kind, h[5], h[4] / w, h[0] / w, h[1] / w, h[2] / w, h[3] / w);
    }
    ps.ran = true;
    p.any = true;
    p.bytes += (double)p.B.n * p.ev_bytes * ps.n_groups;
  }
}

// K_wave: the stream's set, one wave per query (nfa_wave.hip). It reads st[cur] and writes st[1 - cur]
void wave_sets(Pass& p) {
  sdh_engine* e = p.e;
  if (p.B.n <= 0) return;
  for (size_t si = 0; si < e->wsets.size(); ++si) {
    auto& ws = *e->wsets[si];
    if (ws.stream != p.stream) continue;
    sdh::WaveLaunch W{};
    W.tab = tables_of(e);
    W.qlist = ws.d_qs.p;
    W.b = p.B;
    W.n_items = (int32_t)ws.qs.size();
    W.cap = ws.cap;
    W.ew = ws.ew;
    W.cmax = ws.cmax;
    W.n_e1 = ws.n_e1;
    W.n_first = ws.n_first;
    W.n_last = ws.n_last;
    W.na = ws.na;
    W.in = ws.st[ws.cur].p;
    W.out = ws.st[1 - ws.cur].p;
    W.sink = sink_of(e, p.write);
    W.wide = sdh::knob("SDH_KWAVE_WIDE") ? 1 : 0;
    W.xcd = e->xcd;
    W.err = e->d_werr.p + 4 * si;
    HIPCHK(sdh_launch_wave(&W, e->stream));
    e->wave_items += W.n_items;
    ws.ran = true;
    p.any = true;
    // every query stages the batch once; a tile's walk reads and writes the live pages (not modelled:
    // they depend on the data)
    p.bytes += (double)p.B.n * p.ev_bytes * W.n_items;
  }
}

// the partition's K_slab sets: item = (key segment, group whose shape reads this stream)
void slab_sets(Pass& p, int pi, const sdh_engine::Route& rt, Routed r) {
  sdh_engine* e = p.e;
  for (size_t si = 0; si < e->ssets.size(); ++si) {
    auto& ss = *e->ssets[si];
    if (ss.partition != pi) continue;
    const auto& gl = ss.glist[p.stream];
    if (gl.empty() || r.n_runs == 0) continue;
    slab_grow_keys(e, ss, r.n_keys);
    const int64_t items = (int64_t)r.n_runs * (int64_t)gl.size();
    if (items > INT32_MAX) throw Error(SDH_E_UNSUPPORTED, "K_slab launch beyond 2^31 work items (split the batch)");
    ss.journal.ensure((size_t)items);
    ss.journal_idx.ensure((size_t)items);
    HIPCHK(hipMemsetAsync(ss.journal_idx.p, 0xff, (size_t)items * 8, e->stream));
    HIPCHK(hipMemcpyAsync(ss.head_bak.p, ss.head.p, ss.nsub * 8, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(ss.live_bak.p, ss.live.p, 256 * 8, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemsetAsync(ss.traffic.p, 0, 256 * 8, e->stream));
    sdh::SlabLaunch S{};
    S.xcd = e->xcd;
    S.tab = tables_of(e);
    S.shapes = ss.d_shapes.p;
    S.group_shape = ss.d_group_shape.p;
    S.b = p.B;
    S.keys = segments_of(e, rt);
    S.glist = ss.d_glist[p.stream].p;
    S.n_glist = (int32_t)gl.size();
    S.n_items = (int32_t)items;
    S.groups = ss.n_groups;
    S.group_base = ss.group_base;
    S.dir = ss.dir.p;
    S.journal = ss.journal.p;
    S.journal_idx = ss.journal_idx.p;
    S.ring = ss.d_ring.p;
    S.ring_cap = ss.d_cap.p;
    S.head = ss.head.p;
    S.tail = ss.tail.p;
    S.nsub = ss.nsub;
    S.lds_words = ss.lds_words;
    S.max_na = ss.max_na;
    S.live = ss.live.p;
    S.traffic = ss.traffic.p;
    S.sink = sink_of(e, p.write);
    S.err = e->d_serr.p + 4 * si;
    // two LDS tiers: every item first with small rows (more resident waves); the few whose block
    // outgrows them are deferred to a second launch with the set's full rows
    const int small = std::min(ss.lds_words, e->slab_lds_small);
    if (small < ss.lds_words) {
      ss.defer.ensure((size_t)items);
      ss.defer_n.ensure(1);
      HIPCHK(hipMemsetAsync(ss.defer_n.p, 0, 4, e->stream));
      S.lds_words = small;
      S.defer_cap = (int32_t)items;
      S.defer = ss.defer.p;
      S.defer_n = ss.defer_n.p;
    }
    HIPCHK(sdh_launch_slab(&S, e->stream));
    if (small < ss.lds_words) {
      int32_t nd = 0;
      d2h_sync(e, &nd, ss.defer_n.p, 4);
      if (nd > 0) {
        sdh::SlabLaunch D = S;
        D.lds_words = ss.lds_words;
        D.defer_cap = 0;
        D.item_list = ss.defer.p;
        D.n_items = std::min<int32_t>(nd, (int32_t)items);
        HIPCHK(sdh_launch_slab(&D, e->stream));
      }
      ss.deferred += nd;
    }
    ss.items = items;
    e->slab_items += items;
    p.any = true;
    // every item reads its directory word and its key's events; the block bytes it moves are
    // counted by the kernel (added once the pass has run)
    p.bytes += (double)p.B.n * p.ev_bytes * gl.size() + (double)items * 8;
  }
}

// A partition: route the batch once (dense key ids, events grouped by key), then run the partition's
// K_gen set, its K_part sets and its K_slab sets over the same segments. A K_gen set with absent states
// runs as a timer sweep instead: every known key's clone walks the whole batch (time passes for it
// at every event of any key or stream) and processes its own key's events; a time advance, or a
// batch of a stream the partition does not key, sweeps with no own events
void partition_pass(Pass& p, int pi) {
  sdh_engine* e = p.e;
  auto& rt = *e->routes[pi];
  const kg::LPart& pd = e->lp.parts[pi];
  const int64_t n = p.B.n;
  int attr = -1;
  for (const auto& k : pd.keys)
    if (k.stream == p.stream) attr = (int)k.code[0].imm;
  sdh_engine::GenSet* gsp = nullptr;
  for (auto& up : e->gsets)
    if (up->partition == pi) gsp = up.get();
  const bool gen = gsp && gsp->n_groups > 0, timed = gen && gsp->timed;
  if (n == 0 || attr < 0) {
    // a stream the partition does not key reaches every known key's clones (PartitionStreamReceiver
    // .send(ComplexEvent):277-281), ordered by the junction map (fan_positions)
    const kg::LFanOut* fo = n > 0 && gen ? pd.fan(p.stream) : nullptr;
    if (!timed && !fo) return;
    int32_t nk = 0;
    d2h_sync(e, &nk, rt.n_keys.p, 4);
    const int64_t nks = std::min<int64_t>(nk, gsp->key_cap);
    if (fo) gen_sweep(p, *gsp, rt, nullptr, nks, false, fan_positions(e, rt, *fo, nks));
    else gen_sweep(p, *gsp, rt, nullptr, nks, batch_ordered(p));
    return;
  }
  bool reads = gen || rt.track;  // (fan-out: every key's creation counts)
  for (auto& ps : e->psets)
    if (ps->partition == pi && ps->stream == p.stream) reads = true;
  for (auto& ss : e->ssets)
    if (ss->partition == pi && !ss->glist[p.stream].empty()) reads = true;
  if (!reads) return;
  const Routed r = route_batch(p, pi, rt, attr);
  if (gen) {
    gen_grow(e, *gsp, r.n_keys);
    if (timed) gen_sweep(p, *gsp, rt, e->r_kid.p, r.n_keys, batch_ordered(p));
    else gen_keyed(p, *gsp, rt, r);
  }
  part_sets(p, pi, rt, r);
  slab_sets(p, pi, rt, r);
}

// One pass of every K_gen / K_seq / K_wave / K_part / K_slab launch of a push over `stream` (partition routing,
// arena growth, kernels, the event-chunk copy-backs). Returns whether anything ran; *tail_new_len is set
// to the stream's K_seq tail length once the pass is accepted, if a K_seq launch ran.
bool gen_pass(sdh_engine* e, int stream, const StreamBatch& B, bool write, double* bytes_out, int32_t* tail_new_len) {
  int64_t ev_bytes = 8;
  for (int a = 0; a < B.n_attr; ++a) ev_bytes += B.width[a];
  Pass p{e, stream, B, write, ev_bytes};
  e->stats.last_gen_items = 0;
  e->stats.last_seq_items = 0;
  e->stats.last_part_items = 0;
  for (auto& gs : e->gsets)
    if (gs->partition < 0) unpartitioned_pass(p, *gs);
  e->wave_items = 0;
  // (an interleaved push: no K_wave set and no partition reads a stream of the call, mix_plan.h)
  if (!e->mix) wave_sets(p);
  e->stats.last_gen_items += e->wave_items;  // (K_wave's items, a wave each, count with K_gen's)
  for (int pi = 0; pi < (int)e->routes.size() && !e->mix; ++pi)
    if (e->routes[pi]) partition_pass(p, pi);
  if (p.tail_new_len >= 0) *tail_new_len = p.tail_new_len;
  *bytes_out = p.bytes;
  return p.any;
}

}  // namespace

// one K_gen step for every set fed by `stream`
void launch_gen(sdh_engine* e, int stream, const StreamBatch& B, double* ms_out, double* bytes_out) {
  *ms_out = 0;
  *bytes_out = 0;
  e->stats.last_gen_items = 0;
  e->stats.last_seq_items = 0;
  if (e->gsets.empty() && e->psets.empty() && e->ssets.empty() && e->wsets.empty()) return;
  const int64_t n = B.n;
  e->g_out_cap = std::max<int64_t>(e->g_out_cap, std::max<int64_t>(1 << 22, n * 64));
  static_assert((1 << 22) > 2 * GEN_RING_MARGIN, "ring capacity");
  e->d_err.ensure(4);
  e->g_rec_next.ensure(1);
  const bool write = (e->cfg.flags & SDH_FLAG_DEVICE_MATCHES) == 0;
  // the blocks a pass modifies are journaled so that an overflow (match output, K_part tables, K_gen
  // pools, K_slab space) can be undone and the push re-run exactly at the grown capacity, in both
  // output modes (device records grow like the match table's records: no push drops a match)
  e->g_journal = true;
  for (auto& up : e->gsets) up->jn = 0;
  for (auto& ss : e->ssets) slab_prepare(e, *ss);
  const size_t nss = e->ssets.size();
  std::vector<int32_t> serr(4 * std::max<size_t>(1, nss), 0);
  double bytes = 0;
  int32_t tail_len = -1;
  bool any = false;
  int32_t errs[4] = {0, 0, 0, 0};
  unsigned long long nrec = 0, used = 0;
  float ms = 0;
  const size_t nps = e->psets.size();
  std::vector<int32_t> perr(4 * std::max<size_t>(1, nps), 0);
  const size_t nws = e->wsets.size();
  std::vector<int32_t> werr(4 * std::max<size_t>(1, nws), 0);
  for (int attempt = 0;; ++attempt) {
    e->g_out.ensure((size_t)e->g_out_cap);
    if (write) e->g_rec_off.ensure((size_t)rec_cap_of(e));
    HIPCHK(hipMemsetAsync(e->d_err.p, 0, 16, e->stream));
    HIPCHK(hipMemsetAsync(e->d_perr.p, 0, perr.size() * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->d_serr.p, 0, serr.size() * 4, e->stream));
    if (nws) HIPCHK(hipMemsetAsync(e->d_werr.p, 0, werr.size() * 4, e->stream));
    e->slab_items = 0;
    HIPCHK(hipMemsetAsync(e->g_out_next.p, 0, 8, e->stream));
    HIPCHK(hipMemsetAsync(e->g_nrec.p, 0, 8, e->stream));
    HIPCHK(hipMemsetAsync(e->g_rec_next.p, 0, 8, e->stream));
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    any = gen_pass(e, stream, B, write, &bytes, &tail_len);
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipMemcpyAsync(errs, e->d_err.p, 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(perr.data(), e->d_perr.p, perr.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(serr.data(), e->d_serr.p, serr.size() * 4, hipMemcpyDeviceToHost, e->stream));
    if (nws) HIPCHK(hipMemcpyAsync(werr.data(), e->d_werr.p, werr.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&nrec, e->g_nrec.p, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&used, e->g_out_next.p, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    bool out_over = errs[2] != 0, part_over = false, slab_over = false;
    for (size_t i = 0; i < nps; ++i) {
      out_over |= perr[4 * i + 2] != 0;
      part_over |= perr[4 * i] != 0;
    }
    for (size_t i = 0; i < nss; ++i) {
      out_over |= serr[4 * i + 2] != 0;
      slab_over |= serr[4 * i] != 0 || serr[4 * i + 1] != 0;
    }
    bool wave_over = false;
    for (size_t i = 0; i < nws; ++i) {
      out_over |= werr[4 * i + 2] != 0;
      wave_over |= werr[4 * i] != 0;
    }
    kg::Sizing grown;
    const bool pools_over = errs[0] != 0 && gen_grown_sizing(e, errs[0], &grown);
    if (sdh::knob("SDH_TRACE"))
      fprintf(stderr, "[sdh] gen pass stream %d n %lld attempt %d: out %d part %d pools %d slab %d, %llu of %lld words, %.2f ms\n",
              stream, (long long)n, attempt, (int)out_over, (int)part_over, (int)pools_over, (int)slab_over, used,
              (long long)e->g_out_cap, ms);
    if ((out_over || part_over || pools_over || slab_over || wave_over) && e->g_journal && attempt < 24 &&
        (!errs[0] || pools_over) && !errs[1] && !errs[3]) {
      // undo the pass (K_gen blocks from the journal; K_part tables are double-buffered and their
      // per-key selectors are swapped only after success) and re-run it with room for every match
      // record (out_next counts the words every record asked for), every K_part partial and the
      // K_gen pools / lists that overflowed
      gen_restore_journal(e);
      for (size_t i = 0; i < nss; ++i) {
        auto& ss = *e->ssets[i];
        std::vector<int64_t> demand(ss.nsub, 0);
        if (serr[4 * i + 1] && ss.items > 0) {  // what the push tried to take from each ring
          std::vector<unsigned long long> h(ss.nsub);
          HIPCHK(hipMemcpy(h.data(), ss.head.p, ss.nsub * 8, hipMemcpyDeviceToHost));
          for (int r = 0; r < ss.nsub; ++r) demand[r] = (int64_t)(h[r] - ss.h_push0[r]);
        }
        slab_rollback(e, ss);
        if (serr[4 * i]) {  // a block outgrew the LDS staging area
          if (ss.lds_words >= 13312) throw Error(SDH_E_CAPACITY, "K_slab: more partials in one (key, group) block "
                                                                 "than the LDS staging area holds");
          ss.lds_words = std::min(13312, 2 * ss.lds_words);
        }
        if (serr[4 * i + 1]) slab_prepare(e, ss, &demand);  // a ring ran out of room: reclaim / grow
      }
      if (pools_over) {
        gen_relayout(e, grown, true);  // (the next pass journals its blocks in the new layout)
        ++e->gen_regrows;
      }
      if (out_over)
        while (e->g_out_cap < (int64_t)used + (int64_t)used / 4 + GEN_RING_MARGIN) e->g_out_cap *= 2;
      for (size_t i = 0; i < nps; ++i)
        if (perr[4 * i]) {
          if (e->psets[i]->cap >= (1 << 16))
            throw Error(SDH_E_CAPACITY, "more than 65536 pending partials in one K_part instance");
          part_grow_cap(e, *e->psets[i]);
          ++e->part_regrows;
        }
      // K_wave: the pass wrote the other table of each pair, so there is nothing to undo; the tables
      // grow to the walk's upper bound of what they need (at least double) and the pass runs again
      for (size_t i = 0; i < nws; ++i)
        if (werr[4 * i]) {
          auto& ws = *e->wsets[i];
          if (ws.cap >= WAVE_MAX_CAP)
            throw Error(SDH_E_CAPACITY, fmt("more than %d pending partials in one K_wave query", WAVE_MAX_CAP));
          const int64_t want = std::max<int64_t>(2 * (int64_t)ws.cap, ((int64_t)werr[4 * i + 3] + 63) / 64 * 64);
          wave_grow_cap(e, ws, (int)std::min<int64_t>(want, WAVE_MAX_CAP));
          ++e->wave_regrows;
        }
      continue;
    }
    if (part_over)
      throw Error(SDH_E_CAPACITY, "K_part partial table overflow (no room for an exact re-run)");
    if (out_over)
      throw Error(SDH_E_CAPACITY, "K_gen match output overflow (no room for an exact re-run)");
    if (slab_over) throw Error(SDH_E_CAPACITY, "K_slab capacity (no room for an exact re-run)");
    if (wave_over) throw Error(SDH_E_CAPACITY, "K_wave partial table overflow (no room for an exact re-run)");
    break;
  }
  // the push succeeded: its K_slab allocations are committed (the heads tell the next push's room)
  for (auto& up : e->ssets) {
    auto& ss = *up;
    if (ss.items <= 0) continue;
    slab_heads(e, ss);
    unsigned long long tr[256];
    HIPCHK(hipMemcpy(tr, ss.traffic.p, sizeof tr, hipMemcpyDeviceToHost));
    for (unsigned long long x : tr) bytes += (double)x;
    ss.items = 0;
  }
  // the push succeeded: the K_part tables it wrote become current
  for (auto& pp : e->psets)
    if (pp->ran) {
      pp->cur.swap(pp->nxt);
      pp->ran = false;
    }
  for (auto& wp : e->wsets)  // and so do the K_wave tables
    if (wp->ran) {
      wp->cur ^= 1;
      wp->ran = false;
    }
  if (tail_len >= 0 && !errs[0] && !errs[1] && !errs[3]) {
    HIPCHK(sdh_seq_tail(&B, e->seq_tail[stream].p, e->seq_tail_len[stream], tail_len, e->stream));
    e->seq_tail_len[stream] = tail_len;
  }
  *ms_out = ms;
  *bytes_out = bytes;
  if (errs[3]) throw Error(SDH_E_CAPACITY, "partition key table full");
  if (errs[1]) throw Error(SDH_E_REFERENCE, "the reference engine would throw on this stream "
                                            "(ConcurrentModification / IllegalState / NullPointer)");
  if (errs[0]) throw Error(SDH_E_CAPACITY, (errs[0] & kg::CAP_FIXED)
                                               ? "K_gen compiled-in limit exceeded (GC pin depth)"
                                               : "K_gen instance pools could not grow further (4096 StateEvents / nodes per "
                                                 "instance, or device memory)");
  if (!any) nrec = used = 0;
  *bytes_out += (double)nrec * 32.0;  // one (query, ts, seqs) record per match, as for K_ratchet
  e->stats.matches += (int64_t)nrec;
  e->g_dev_matches = (int64_t)nrec;
  e->g_used = (int64_t)used;
}

// ---- snapshot sections (engine_snap.hip): K_gen sets: instance arenas (Snapshotable state of every pre-processor of every instance)
void snap_save_gen(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->gsets.size());
  for (auto& up : e->gsets) {
    auto& gs = *up;
    const int64_t blocks = gs.partition < 0 ? gs.n_groups : gs.key_cap * gs.n_groups;
    w.put(gs.partition);
    w.put(gs.key_cap);
    w.put(blocks);
    put_dev(w, gs.a32.p, (size_t)blocks * e->gB32 * 64 * 4);
    put_dev(w, gs.a64.p, (size_t)blocks * e->gB64 * 64 * 8);
  }
}

void snap_load_gen(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->gsets.size(), "snapshot of a different program");
  for (auto& up : e->gsets) {
    auto& gs = *up;
    snap::need(r.get() == gs.partition, "snapshot of a different program");
    const int64_t key_cap = r.get(), blocks = r.get();
    if (gs.partition >= 0) {
      gen_grow(e, gs, key_cap);
      snap::need(gs.key_cap == key_cap, "snapshot key capacity mismatch");
    }
    snap::need(blocks == (gs.partition < 0 ? gs.n_groups : gs.key_cap * gs.n_groups), "snapshot arena size mismatch");
    get_dev(r, gs.a32.p, (size_t)blocks * e->gB32 * 64 * 4);
    get_dev(r, gs.a64.p, (size_t)blocks * e->gB64 * 64 * 8);
  }
}

// partition key tables (PartitionRuntime's key -> instance map) and, for fan-out partitions, the keys'
// creation order (the junction maps' insertion order)
void snap_save_routes(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->routes.size());
  for (auto& rp : e->routes) {
    w.put(rp ? 1 : 0);
    if (!rp) continue;
    const size_t slots = (size_t)rp->tmask + 2;
    w.put((int64_t)slots);
    put_dev(w, rp->tkey.p, slots * 8);
    put_dev(w, rp->tid.p, slots * 4);
    put_dev(w, rp->n_keys.p, 4);
    put_dev(w, rp->key_of_id.p, (size_t)rp->max_keys * 8);
    w.put(rp->kkind);
    w.put(rp->nk_seen);
    w.put((int64_t)rp->korder_kid.size());
    for (size_t j = 0; j < rp->korder_kid.size(); ++j) {
      w.put(rp->korder_kid[j]);
      w.put(rp->korder_key[j]);
    }
  }
}

void snap_load_routes(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->routes.size(), "snapshot of a different program");
  for (auto& rp : e->routes) {
    snap::need(r.get() == (rp ? 1 : 0), "snapshot of a different program");
    if (!rp) continue;
    const size_t slots = (size_t)r.get();
    snap::need(slots == (size_t)rp->tmask + 2, "snapshot key table mismatch");
    get_dev(r, rp->tkey.p, slots * 8);
    get_dev(r, rp->tid.p, slots * 4);
    get_dev(r, rp->n_keys.p, 4);
    get_dev(r, rp->key_of_id.p, (size_t)rp->max_keys * 8);
    rp->kkind = (int)r.get();
    rp->nk_seen = r.get();
    const int64_t nko = r.get();
    snap::need(nko >= 0 && nko <= rp->max_keys, "bad snapshot key order");
    rp->korder_kid.resize((size_t)nko);
    rp->korder_key.resize((size_t)nko);
    for (size_t j = 0; j < (size_t)nko; ++j) {
      rp->korder_kid[j] = r.get();
      rp->korder_key[j] = r.get();
    }
    rp->fan.clear();
  }
}

// K_part tables: both buffers and the per-key selector
void snap_save_part(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->psets.size());
  for (auto& pp : e->psets) {
    auto& ps = *pp;
    w.put(ps.partition);
    w.put(ps.kind);
    w.put(ps.cap);
    w.put(ps.key_cap);
    put_dev(w, ps.st.p, (size_t)2 * ps.key_cap * ps.n_groups * ps.bw() * 64 * 8);
    put_dev(w, ps.cur.p, (size_t)ps.key_cap * 4);
  }
}

void snap_load_part(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->psets.size(), "snapshot of a different program");
  for (auto& pp : e->psets) {
    auto& ps = *pp;
    snap::need(r.get() == ps.partition && r.get() == ps.kind, "snapshot of a different program");
    const int64_t cap = r.get(), key_cap = r.get();
    snap::need(cap >= 1 && cap <= (1 << 20) && key_cap >= 0 && key_cap <= (int64_t)1 << 40, "bad snapshot K_part table size");
    ps.cap = (int)cap;
    ps.key_cap = 0;
    DevBuf<int64_t>().swap(ps.st);  // freed: reallocated at the snapshot's capacity
    part_grow(e, ps, key_cap);
    snap::need(ps.key_cap == key_cap, "snapshot key capacity mismatch");
    get_dev(r, ps.st.p, (size_t)2 * ps.key_cap * ps.n_groups * ps.bw() * 64 * 8);
    get_dev(r, ps.cur.p, (size_t)ps.key_cap * 4);
  }
}

// K_wave tables: per set its stream, queries, layout and capacity, then each query's current table
// (the other one of a pair is scratch until the next push writes it)
void snap_save_wave(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->wsets.size());
  for (auto& wp : e->wsets) {
    auto& ws = *wp;
    w.put(ws.stream);
    w.put((int64_t)ws.qs.size());
    w.put(ws.ew);
    w.put(ws.cap);
    put_dev(w, ws.st[ws.cur].p, ws.qs.size() * (size_t)ws.stride() * 8);
  }
}

void snap_load_wave(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->wsets.size(), "snapshot of a different program");
  // every set's section is checked before any table is uploaded: the kernel trusts a table's live
  // count and each live entry's chain length
  struct Sec { int64_t cap; const int64_t* blob; };
  std::vector<Sec> secs;
  for (auto& wp : e->wsets) {
    auto& ws = *wp;
    snap::need(r.get() == ws.stream && (size_t)r.get() == ws.qs.size() && r.get() == ws.ew,
               "snapshot of a different program");
    const int64_t cap = r.get();
    snap::need(cap >= 64 && cap % 64 == 0 && cap <= WAVE_MAX_CAP, "bad snapshot K_wave table size");
    const size_t stride = (size_t)(WV_HDR + cap * ws.ew);
    const int64_t* blob = (const int64_t*)r.bytes(ws.qs.size() * stride * 8);
    for (size_t qx = 0; qx < ws.qs.size(); ++qx) {
      const int64_t* t = blob + qx * stride;
      const int64_t n = t[0], cmax = e->gq[ws.qs[qx]].st[1].max;
      snap::need(n >= 0 && n <= cap, "bad snapshot K_wave live count");
      for (int64_t i = 0; i < n; ++i) {  // entry i's flags word: word 2 of lane i % 64 of page i / 64
        const int64_t fl = t[WV_HDR + ((i >> 6) * ws.ew + 2) * 64 + (i & 63)];
        snap::need((fl & 0xff) <= cmax, "bad snapshot K_wave chain length");
      }
    }
    secs.push_back({cap, blob});
  }
  for (size_t si = 0; si < e->wsets.size(); ++si) {
    auto& ws = *e->wsets[si];
    const size_t words = ws.qs.size() * (size_t)(WV_HDR + secs[si].cap * ws.ew);
    if (secs[si].cap != ws.cap) {
      ws.cap = (int)secs[si].cap;
      for (auto& b : ws.st) {
        DevBuf<int64_t>().swap(b);  // freed: reallocated at the snapshot's capacity
        b.ensure(words);
      }
    }
    ws.cur = 0;
    ws.ran = false;
    HIPCHK(hipMemcpy(ws.st[0].p, secs[si].blob, words * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ws.st[1].p, 0, words * 8));
  }
}

// live partials of the K_wave tables (sdh_engine_stats)
int64_t wave_live_partials(sdh_engine* e) {
  if (e->wsets.empty()) return 0;
  unsigned long long* acc = e->d_wave_live.p;  // (allocated once, at creation)
  HIPCHK(hipMemsetAsync(acc, 0, 8, e->stream));
  for (auto& wp : e->wsets)
    HIPCHK(sdh_live_wave(wp->st[wp->cur].p, (int64_t)wp->qs.size(), wp->stride(), acc, e->stream));
  unsigned long long v = 0;
  d2h_sync(e, &v, acc, 8);
  return (int64_t)v;
}

// K_seq: each stream's tail (the only state its windowed sequences carry between pushes)
void snap_save_seq(sdh_engine* e, snap::Writer& w) {
  w.put((int64_t)e->seq_tail.size());
  for (size_t st = 0; st < e->seq_tail.size(); ++st) {
    w.put(e->seq_tail_len[st]);
    put_dev(w, e->seq_tail[st].p, SEQ_TMAX * SEQ_TW * 8);
  }
}

void snap_load_seq(sdh_engine* e, snap::Reader& r) {
  snap::need((size_t)r.get() == e->seq_tail.size(), "snapshot of a different program");
  for (size_t st = 0; st < e->seq_tail.size(); ++st) {
    const int64_t tl = r.get();
    snap::need(tl >= 0 && tl <= SEQ_TMAX, "bad snapshot tail length");
    e->seq_tail_len[st] = (int32_t)tl;
    get_dev(r, e->seq_tail[st].p, SEQ_TMAX * SEQ_TW * 8);
  }
}

}  // namespace eng
}  // namespace sdh
