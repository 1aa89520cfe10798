// launchers.h -- the host-side launchers the engine units call, declared once. They are defined in
// matches.hip and nfa_*.hip; each defining file includes this header too, so a parameter list that
// drifts from its declaration fails to compile (`extern "C"` names carry no types: it would link).
// Host-only: the hiprtc-compiled kernels do not see it. The structs are only named here; their
// definitions are in nfa_types.h and kgen.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace sdh {
struct StreamBatch;
struct ChainLaunch;
struct MixPre;
struct RatchetGroup;
struct RatchetLaunch;
struct SharedLaunch;
struct GenLaunch;
struct PartLaunch;
struct WaveLaunch;
struct SlabLaunch;
struct SeqLaunch;
struct MatchTable;
namespace kg {
struct GLayout;
struct GQuery;
}  // namespace kg
namespace sel {
struct Tables;
struct Store;
}  // namespace sel
}  // namespace sdh

// the event store and the device selector (select.hip)
extern "C" hipError_t sdh_store_append(const sdh::StreamBatch* B, uint32_t float_mask, int64_t* rows, int64_t mask,
                                       int W, hipStream_t s);
extern "C" hipError_t sdh_store_relay(const int64_t* src, int64_t src_mask, int64_t* dst, int64_t dst_mask, int W,
                                      int64_t lo, int64_t n, hipStream_t s);
extern "C" hipError_t sdh_select_sorted(const sdh::sel::Tables* T, const sdh::sel::Store* st, int deep,
                                        sdh::MatchTable M, const int32_t* perm, const int64_t* po_q, int64_t n,
                                        int width, int32_t* oq, int64_t* cells, uint64_t* nulls, int32_t* err,
                                        hipStream_t s);
extern "C" hipError_t sdh_select_placed(const sdh::sel::Tables* T, const sdh::sel::Store* st, int deep,
                                        const int32_t* crow, int cw, const int64_t* ts_log, int64_t seq_ref, int64_t n,
                                        int width, int32_t* oq, int64_t* ots, int64_t* oseq, int64_t* cells,
                                        uint64_t* nulls, int32_t* err, hipStream_t s);

// rows from device records (sdh_engine_records_rows): one part's rows [first, first + n) of the last
// push's records into rows [out0, out0 + n) of the window's arrays
namespace sdh {
struct RecRows {
  int64_t first, n, out0, seq_base;
  const int64_t* match;  // K_ratchet blocks
  int32_t blk_recs, wide;
  const int32_t* blk_count;
  const int32_t* blk_group;
  const int32_t* blk_side;
  const RatchetGroup* groups;
  const int64_t* row_off;
  int64_t nb;
  const int64_t* flat;   // flat records
  const int64_t* rec_off;
  const int64_t* chain;  // K_chain segments
  const int64_t* seg_off;
  const int64_t* seg_row;
  int64_t items;
  int32_t rec_words, pad;
  const int32_t* qinfo;
};
}  // namespace sdh
extern "C" hipError_t sdh_select_records(const sdh::sel::Tables* T, const sdh::sel::Store* st, int deep, int part,
                                         int search, const sdh::RecRows* R, int64_t n_out, int width, int32_t* oq,
                                         int64_t* ots, int64_t* oseq, int64_t* cells, uint64_t* nulls, int32_t* err,
                                         hipStream_t s);
extern "C" size_t sdh_flat_heads_temp(int64_t words);
extern "C" hipError_t sdh_flat_heads(const int64_t* out, int64_t words, void* temp, int64_t* rec_off, int64_t cap,
                                     unsigned long long* n_out, hipStream_t s);

extern "C" hipError_t sdh_launch_gen(const sdh::GenLaunch* L, hipStream_t s);
extern "C" hipError_t sdh_launch_part(const sdh::PartLaunch* L, hipStream_t s);
// the interpreted kernel of K_part's chain kind (nfa_part_chain.hip; sdh_launch_part hands PK_CHAIN on)
extern "C" hipError_t sdh_launch_part_chain(const sdh::PartLaunch* L, hipStream_t s);
// K_wave (nfa_wave.hip): one wave per unpartitioned count query, and the live entries of n tables
// (their header words, summed into acc)
extern "C" hipError_t sdh_launch_wave(const sdh::WaveLaunch* L, hipStream_t s);
extern "C" hipError_t sdh_live_wave(const int64_t* st, int64_t n, int64_t stride, unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_launch_seq(const sdh::SeqLaunch* L, hipStream_t s);
extern "C" hipError_t sdh_launch_slab(const sdh::SlabLaunch* L, hipStream_t s);
extern "C" hipError_t sdh_slab_rollback(uint64_t* dir, const uint64_t* journal, const uint64_t* journal_idx, int64_t n,
                                        const long long* live_bak, long long* live, hipStream_t s);
extern "C" hipError_t sdh_slab_move(uint64_t* dir, int64_t n_dir, int groups, const int32_t* group_ew,
                                    uint32_t* const* src_ring, const int64_t* src_cap,
                                    const unsigned long long* src_tail, int src_nsub, const unsigned long long* limit,
                                    const uint8_t* active, uint32_t* const* dst_ring, const int64_t* dst_cap,
                                    unsigned long long* dst_head, const unsigned long long* dst_tail, int dst_nsub,
                                    int32_t* err, uint8_t* ring_err, hipStream_t s);
extern "C" hipError_t sdh_slab_live_words_ring(const uint64_t* dir, int64_t n_dir, int groups, const int32_t* group_ew,
                                               int nsub, unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_slab_live_words(const uint64_t* dir, int64_t n_dir, int groups, const int32_t* group_ew,
                                          unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_seq_tail(const sdh::StreamBatch* b, int64_t* tail, int32_t tail_len, int32_t new_tail_len,
                                   hipStream_t s);
extern "C" hipError_t sdh_route_partition(const sdh::StreamBatch* B, int attr, int type, unsigned long long* tkey,
                                          int32_t* tid, int64_t table_mask, int32_t* n_keys, int64_t* key_of_id,
                                          int64_t key_cap, int64_t* key, uint32_t* kid, uint32_t* kid_sorted,
                                          int32_t* idx, int32_t* idx_sorted, uint32_t* uniq, int32_t* cnt,
                                          int32_t* off, int32_t* n_runs_dev, void* temp, size_t temp_bytes,
                                          int32_t* err, int shard_rank, int shard_world, hipStream_t s);
extern "C" size_t sdh_route_temp_bytes(int64_t n);
extern "C" hipError_t sdh_gen_remap(const int32_t* lane_q, int group_base, int n_groups, int64_t blocks,
                                    const sdh::kg::GLayout* oldL, const sdh::kg::GLayout* newL, const int32_t* o32,
                                    const int64_t* o64, int64_t oB32, int64_t oB64, int32_t* n32, int64_t* n64,
                                    int64_t nB32, int64_t nB64, hipStream_t s);

// (resid: a query of the engine has a residual program -- the R = true instantiations)
extern "C" hipError_t sdh_launch_chain(int n_states, int k, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                       size_t lds, hipStream_t s);
extern "C" hipError_t sdh_launch_chain_paged(int n_states, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                             hipStream_t s);
// an interleaved push (ChainLaunch::mix): the MIX = true paged kernels; the pre-pass over `order` and
// the event store's append at merged positions (mixed.hip)
extern "C" hipError_t sdh_launch_chain_mixed(int n_states, int resid, const sdh::ChainLaunch* L, int n_blocks,
                                             hipStream_t s);
extern "C" int64_t sdh_mix_blocks(int64_t n);
extern "C" hipError_t sdh_mix_count(const sdh::MixPre* A, hipStream_t s);
extern "C" hipError_t sdh_mix_write(const sdh::MixPre* A, hipStream_t s);
extern "C" hipError_t sdh_store_append_mixed(const sdh::StreamBatch* B, uint32_t float_mask, const int32_t* pos,
                                             int64_t first, int64_t* rows, int64_t mask, int W, hipStream_t s);
extern "C" hipError_t sdh_chain_relayout(const int64_t* src, int64_t* dst, int64_t rows, int old_cap, int new_cap,
                                         hipStream_t s);
extern "C" hipError_t sdh_launch_ratchet(int key_kind, int xmask, int full, int nf, int sim, int ML, int SC,
                                         const sdh::RatchetLaunch* L, hipStream_t s);
extern "C" int sdh_ratchet_occupancy(int key_kind, int full, int nf, int ML, int sim);
// the shared-pops form (nfa_ratchet_shared.hip)
extern "C" size_t sdh_ratchet_shared_temp(int64_t n);
extern "C" int sdh_ratchet_shared_occupancy();
extern "C" hipError_t sdh_launch_ratchet_shared_pre(const sdh::SharedLaunch* S, const sdh::StreamBatch* B, int32_t* err,
                                                    void* temp, size_t temp_bytes, hipStream_t s);
extern "C" hipError_t sdh_launch_ratchet_shared(const sdh::RatchetLaunch* L, const sdh::SharedLaunch* S, hipStream_t s);
extern "C" hipError_t sdh_launch_ratchet_summary(int key_kind, const sdh::StreamBatch* B, int attr, int conv,
                                                 int64_t n_tiles, uint64_t* tmax, uint64_t* tmin, uint8_t* thas,
                                                 hipStream_t s);
extern "C" hipError_t sdh_append_ratchet(const int64_t* match, int blk_recs, int wide, const int32_t* blk_count,
                                         const int32_t* blk_group, const int64_t* dst_off,
                                         const sdh::RatchetGroup* groups, const int64_t* ts, int64_t seq_base,
                                         int64_t seq_ref, const int32_t* out_rank, int n_streams, int n_blocks,
                                         sdh::MatchTable T, int64_t row0, int64_t word0, hipStream_t s);
extern "C" hipError_t sdh_append_chain(const int64_t* src, const int64_t* seg_off, const int64_t* seg_count,
                                       const int64_t* dst_off, int rec_words, int n_items, const int32_t* qinfo,
                                       int64_t seq_ref, const int32_t* out_rank, int n_streams, sdh::MatchTable T,
                                       int64_t row0, int64_t word0, hipStream_t s);
extern "C" size_t sdh_gen_words_temp_bytes(int64_t n_rec);
extern "C" size_t sdh_sorted_batch_bytes(const sdh::StreamBatch* b);
extern "C" hipError_t sdh_sort_batch(const sdh::StreamBatch* b, const int32_t* idx, uint8_t* buf, sdh::StreamBatch* o,
                                     hipStream_t s);
extern "C" hipError_t sdh_gen_words(const int64_t* out, const int64_t* rec_off, int64_t n_rec, int64_t* tw, void* temp,
                                    size_t temp_bytes, unsigned long long* n_wide, hipStream_t s);
extern "C" size_t sdh_ex_temp_bytes(int64_t n);
extern "C" hipError_t sdh_ex_chain_words(sdh::MatchTable T, const int32_t* perm, int64_t n, int64_t* cw, void* temp,
                                         size_t temp_bytes, hipStream_t s);
extern "C" hipError_t sdh_ex_rows(sdh::MatchTable T, const int32_t* perm, int64_t n, int width, int64_t seq_ref,
                                  const int64_t* coff, int32_t* rows, int32_t* chain, int64_t* okey, int64_t* otb,
                                  int32_t* err, hipStream_t s);
extern "C" hipError_t sdh_fill_i64(int64_t* p, int64_t n, int64_t v, hipStream_t s);
extern "C" hipError_t sdh_append_gen(const int64_t* out, const int64_t* rec_off, int64_t n_rec, int64_t seq_ref,
                                     const int32_t* out_rank, const int32_t* fan_rank, int n_streams, sdh::MatchTable T,
                                     int64_t row0, int64_t word0, const int64_t* woff, const int64_t* bts,
                                     int64_t seq_base, int bstream, const int64_t* const* qkeys, hipStream_t s);
extern "C" hipError_t sdh_new_keys(const uint32_t* uniq, const int32_t* nruns, int64_t max_runs, const int32_t* off,
                                   const int32_t* idx_s, const int64_t* key_of_id, int64_t old_n, int64_t new_n,
                                   int64_t* out, hipStream_t s);
extern "C" size_t sdh_poll_temp_bytes(int64_t n);
extern "C" hipError_t sdh_gen_journal(int32_t* a32, int64_t* a64, int64_t B32, int64_t B64, int mode,
                                       const int32_t* glist, const uint32_t* seg_kid, int groups, int64_t slots,
                                       int32_t* j32, int64_t* j64, int64_t* jidx, int restore, hipStream_t s);
extern "C" size_t sdh_place_temp_bytes(int64_t cells);
extern "C" size_t sdh_prefix_max_temp_bytes(int64_t n);
extern "C" hipError_t sdh_prefix_max(const int64_t* ts, int64_t n, int64_t* pm, int32_t* unordered, void* temp,
                                     size_t temp_bytes, hipStream_t s);
extern "C" hipError_t sdh_key_segments(const uint32_t* uniq, const int32_t* nruns, int64_t max_runs, int64_t n_keys,
                                       int32_t* kseg, hipStream_t s);
extern "C" hipError_t sdh_digest_compact(const int32_t* crow, int width, int64_t row0, int64_t n, int64_t seq_ref,
                                         unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_place_scan(int32_t* cnt, int64_t cells, void* temp, size_t temp_bytes, hipStream_t s);
extern "C" hipError_t sdh_merge_keys_table(sdh::MatchTable T, const int32_t* perm, int64_t n, int chunk_words,
                                           int lo_words, int chunked, uint64_t* keys, hipStream_t s);
extern "C" hipError_t sdh_merge_keys_placed(const int32_t* crow, int width, int64_t n, int64_t seq_ref,
                                            const int32_t* out_rank, const int32_t* qinfo, int n_streams,
                                            int chunk_words, int lo_words, uint64_t* keys, hipStream_t s);
extern "C" hipError_t sdh_place_total(const int32_t* cnt, int64_t cells, unsigned long long* tot, hipStream_t s);
extern "C" hipError_t sdh_compact_fill(const int32_t* crow, int width, int64_t rows, const int64_t* ts_log,
                                       int64_t seq_ref, int64_t* oq, int64_t* okey, int64_t* ots, int64_t* oseq,
                                       int64_t* otb, int64_t* ooff, int64_t* owords, hipStream_t s);
extern "C" hipError_t sdh_placed_to_table(const int32_t* crow, int width, int64_t n, const int64_t* ts_log,
                                          int64_t seq_ref, const int32_t* out_rank, const int32_t* qinfo,
                                          int n_streams, sdh::MatchTable T, hipStream_t s);
extern "C" hipError_t sdh_table_compact(sdh::MatchTable T, const int32_t* perm, int64_t n, int width, int64_t seq_ref,
                                        int32_t* crow, int32_t* err, hipStream_t s);
extern "C" hipError_t sdh_live_gen(const int32_t* a32, int64_t B32, int64_t blocks, int n_groups, int group_base,
                                    const int32_t* lane_q, const int32_t* group_seq, const sdh::kg::GQuery* queries,
                                    unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_live_seq(const int64_t* tail, int tail_len, int stream, const int32_t* groups, int n_groups,
                                   const int32_t* lane_q, const int32_t* group_tmpl, const sdh::kg::GQuery* queries,
                                   unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_live_part(const int64_t* st, const int32_t* cur, int64_t n_keys, int groups, int64_t blocks,
                                    int64_t bw, unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_digest_ratchet(const int64_t* match, int blk_recs, int wide, const int32_t* blk_count,
                                         const int32_t* blk_group, const int32_t* blk_side,
                                         const sdh::RatchetGroup* groups, int64_t seq_base,
                                         int n_blocks, unsigned long long* acc, hipStream_t s);
extern "C" hipError_t sdh_launch_gate(int key_kind, int xmask, int full, int nf, int ng, int SC,
                                      const sdh::RatchetLaunch* L, hipStream_t s);
extern "C" int sdh_gate_occupancy(int nf, int ng);
extern "C" size_t sdh_ratchet_compact_temp(int64_t n_blocks);
extern "C" hipError_t sdh_ratchet_compact(const int64_t* match, int blk_recs, int wide, const int32_t* blk_count,
                                          const int32_t* blk_group, const int32_t* blk_side,
                                          const sdh::RatchetGroup* groups, int64_t seq_base, int n_blocks,
                                          int64_t* row_off, void* temp, size_t temp_bytes, int width, int32_t* rows,
                                          hipStream_t s);
extern "C" hipError_t sdh_poll_sort(sdh::MatchTable T, int64_t n, int n_lo, int lo_bits, int hi_bits, int clo_bits,
                                    uint64_t* kbuf, int32_t* pbuf, void* temp, size_t temp_bytes, int64_t* oq,
                                    int64_t* okey, int64_t* ots, int64_t* oseq, int64_t* otb, int64_t* olen,
                                    int64_t* ooff, int32_t** perm_out, int64_t* total_words, hipStream_t s);
extern "C" hipError_t sdh_chunk_keys(sdh::MatchTable T, int64_t r0, int64_t r1, int chunk, int64_t cseq,
                                     int64_t first_seq, int stream, int n_streams, const int32_t* major,
                                     const int32_t* minor, const int32_t* qslot, const int32_t* runs,
                                     int64_t n_events, hipStream_t s);
extern "C" hipError_t sdh_poll_words(sdh::MatchTable T, const int32_t* perm, int64_t n, const int64_t* ooff,
                                     int64_t* owords, hipStream_t s);
