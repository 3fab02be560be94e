// What the host files of the ends-free engine share: ends_free_host.cpp
// (saln_ends_free_*, the batch itself), ends_free_long_host.cpp
// (saln_ends_free_long_*, the chunked fill's sizes, path and launches) and
// ends_free_replay_host.cpp (saln_ends_free_replay_*, the tiled replay's
// footprint and rounds).
#pragma once
#include "ends_free.hpp"
#include "host_common.hpp"

#include <vector>

namespace saln {

// A batch's or a plan's scoring as the caller gave it: the scalar scheme
// (sub == nullptr; scalar == nullptr selects the default {5, -4, -8, -6}) or a
// substitution matrix (is_sub; sub == nullptr is the caller's error).
struct EfScoreSrc {
    const saln_nw_scoring *scalar = nullptr;
    const saln_sub_matrix *sub = nullptr;
    bool is_sub = false;
    static EfScoreSrc of(const saln_nw_scoring *s) { return EfScoreSrc{s, nullptr, false}; }
    static EfScoreSrc of(const saln_sub_matrix *m) { return EfScoreSrc{nullptr, m, true}; }
};

// The batch behind saln_ends_free_align_batch (long_ok = false: the classes'
// limits and refusals) and saln_ends_free_long_align_batch (long_ok = true:
// pairs above those limits run the chunked fill) and, with tile_rows != 0,
// saln_ends_free_replay_align_batch (a chunk holds replay footprints, and the
// alignments of its chunked-path pairs come from ef_replay_run).  xdrop:
// kEfNoXdrop, or the X of saln_ends_free_xdrop_align_batch (mode
// SALN_MODE_EXTEND, long_ok false: the class fills' X-drop instances) and of
// saln_ends_free_xdrop_long_align_batch (long_ok true, tile_rows 0: pairs
// above the limits run the chunked X-drop fill, ef_xdrop_long_fill) and of
// saln_ends_free_xdrop_replay_align_batch (long_ok true, tile_rows != 0: a
// chunk holds X-drop replay footprints, ef_xdrop_replay_layout, and
// ef_replay_run takes the X).
// ends_free_host.cpp.
int ef_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                   const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                   const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                   const EfScoreSrc &scoring, uint64_t trace_budget_bytes, int want_cigar,
                   saln_ends_free_aln **out, bool long_ok, uint32_t tile_rows = 0,
                   int32_t xdrop = kEfNoXdrop);

// The plan behind saln_ends_free_plan_create and saln_ends_free_sub_plan_create
// and, with an xdrop other than kEfNoXdrop, their _xdrop_ forms.
// ends_free_host.cpp.
int ef_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off,
                   uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                   int32_t mode, const EfScoreSrc &scoring, saln_ends_free_plan **out,
                   int32_t xdrop = kEfNoXdrop);

// What ends_free_score_host.cpp (saln_ends_free_score_*) takes from
// ends_free_host.cpp: the mode and scoring checks with their messages, the
// per-pair limits and range guard, the pair descriptors in pair order, and the
// class fills' launches (pairs sorted by class and falling db length, cut where
// the length's power-of-two bucket changes).
struct EfLaunch {
    int cls;
    uint32_t first, count, ld_max;
};
int ef_check_mode(int32_t mode);
int ef_make_scoring(const EfScoreSrc &src, EfScoring *out, uint64_t *max_abs, std::vector<uint8_t> *block);
int ef_check_pair(uint64_t lq, uint64_t ld, uint64_t max_abs);
int ef_build_pairs(const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off, uint64_t n_db,
                   const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, uint64_t max_abs,
                   std::vector<EfPair> *out);
void ef_plan_launches(std::vector<EfPair> *pairs, std::vector<EfLaunch> *out);

// Device workspace of a batch's chunked fills, all on one stream: the boundary
// slots (grown to the largest launch's need) and the pair counter.
struct EfLongWorkspace {
    DevBuf bnd, counter;
    size_t bnd_bytes = 0;
    EfLongWorkspace(saln_context *ctx, hipStream_t s) : bnd(ctx, s), counter(ctx, s) {}
};

// One chunked-fill launch of pairs[first .. first + count) with dbs of at most
// ld_max rows: ef_long_slots waves.  d_sub here and below: the matrix's device
// block, or nullptr under the scalar scoring.  ends_free_long_host.cpp.
int ef_long_fill(EfLongWorkspace *ws, int32_t mode, const EfPair *d_pairs, uint32_t first,
                 uint32_t count, uint32_t ld_max, const uint8_t *d_q, const uint8_t *d_db,
                 const EfScoring &sc, const uint8_t *d_sub, uint8_t *d_codes, uint8_t *d_end_state,
                 saln_ends_free_result *d_results, hipStream_t s);

// The same launch of the chunked X-drop fill (SALN_MODE_EXTEND, xdrop >= 0):
// ef_xdrop_long_slots waves, whose boundary entries hold 16 bytes per row.
// ends_free_long_host.cpp.
int ef_xdrop_long_fill(EfLongWorkspace *ws, const EfPair *d_pairs, uint32_t first, uint32_t count,
                       uint32_t ld_max, const uint8_t *d_q, const uint8_t *d_db, const EfScoring &sc,
                       const uint8_t *d_sub, int32_t xdrop, uint8_t *d_codes, uint8_t *d_end_state,
                       saln_ends_free_result *d_results, hipStream_t s);

// Device workspace of a batch's replays, all on one stream: the walks' states
// and the forward pass's pair counter; under X-drop also the walk's own pair
// descriptors (ef_replay_run), on the host and on the device.
struct EfReplayWorkspace {
    DevBuf state, counter, walk_pairs;
    size_t state_bytes = 0, walk_pairs_bytes = 0;
    std::vector<EfPair> walk_pairs_host;
    EfReplayWorkspace(saln_context *ctx, hipStream_t s) : state(ctx, s), counter(ctx, s), walk_pairs(ctx, s) {}
};

// What ef_replay_run leaves in lens for a pair whose walk did not end within
// the rounds its lengths allow.
constexpr uint32_t kEfWalkUnfinished = 0xFFFFFFFFu;

// The tiled replay of `count` pairs of the chunked path (h_pairs on the host,
// d_pairs the same on the device; code_off: each pair's replay area in
// d_area): the forward pass, then the rounds of tile fill and tile walk, all
// queued on s, none waited for.  Records, words and lens as the class walk
// leaves them.  xdrop: kEfNoXdrop, or X with SALN_MODE_EXTEND: the X-drop
// forward pass and tile fill over ef_xdrop_replay_layout's areas (code_off a
// multiple of 16), the forward pass's steps in `reserved`.
// ends_free_replay_host.cpp.
int ef_replay_run(EfReplayWorkspace *ws, int32_t mode, const EfPair *h_pairs, const EfPair *d_pairs,
                  uint32_t count, const uint8_t *d_q, const uint8_t *d_db, const EfScoring &sc,
                  const uint8_t *d_sub, uint8_t *d_area, uint32_t tile_rows, uint8_t *d_end_state,
                  saln_ends_free_result *d_results, uint32_t *d_words, uint32_t *d_lens, hipStream_t s,
                  int32_t xdrop = kEfNoXdrop);

}  // namespace saln
