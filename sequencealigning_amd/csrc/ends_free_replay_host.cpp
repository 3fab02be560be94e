// C ABI of the ends-free engine's tiled replay traceback (include/saln.h,
// saln_ends_free_replay_*).  The batch is
// ends_free_host.cpp's (ef_align_batch with tile_rows): pairs within the
// classes' limits run as under every other entry point; a pair of the chunked
// path keeps boundary columns and checkpoint rows in place of its codes and
// gets its words from ef_replay_run below.  This file holds what the replay
// adds: the footprint of a pair, the option's check, and the host loop, and the
// X-drop forms of all three (saln_ends_free_xdrop_replay_*; DESIGN.md section
// 3k): the same batch with an X, whose chunked-path pairs run the X-drop forward
// pass and tile fill (ends_free_xdrop_replay_kernels.hip) and the same walk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>

#include "ends_free_host.hpp"

using namespace saln;

namespace {

// The option's value, or the caller's: one of the five tile heights.
int check_tile_rows(int64_t R) {
    if (ef_tile_rows_ok(R)) return SALN_OK;
    set_error("ends_free: tile_rows " + std::to_string(R) + " (option ends_free.tile_rows) is not one of "
              "64, 128, 256, 512, 1024");
    return SALN_E_INVALID;
}

}  // namespace

// The walk of a pair visits tiles (c, b) of falling c + b: it only moves up
// and left, and every round ends in another tile than it began in, or ends the
// pair.  From the end cell's tile at most chunks + row blocks - 1 tiles lie on
// such a path, so that many rounds finish every pair, and the loop runs that
// many for the largest pair whatever the device did: a pair left unfinished
// (kEfWalkUnfinished in lens) is the caller's internal error, not waited for.
// xdrop (kEfNoXdrop: none; else mode is SALN_MODE_EXTEND): the forward pass and
// the tile fill are the X-drop kernels, d_area holds ef_xdrop_replay_layout's
// areas, and the round count stays the same.
int saln::ef_replay_run(EfReplayWorkspace *ws, int32_t mode, const EfPair *h_pairs,
                        const EfPair *d_pairs, uint32_t count, const uint8_t *d_q, const uint8_t *d_db,
                        const EfScoring &sc, const uint8_t *d_sub, uint8_t *d_area, uint32_t tile_rows,
                        uint8_t *d_end_state,
                        saln_ends_free_result *d_results, uint32_t *d_words, uint32_t *d_lens,
                        hipStream_t s, int32_t xdrop) {
    if (count == 0) return SALN_OK;
    if (!ef_tile_rows_ok(tile_rows)) return SALN_E_INVALID;
    if (xdrop != kEfNoXdrop && (xdrop < 0 || mode != SALN_MODE_EXTEND)) return SALN_E_INVALID;
    uint64_t rounds = 0;
    for (uint32_t k = 0; k < count; ++k) {
        const uint64_t lq = h_pairs[k].lq, ld = h_pairs[k].ld;
        if (lq == 0 || ld == 0) continue;  // no cell, no code: the start ends it
        rounds = std::max(rounds, (lq + kEfChunkCols - 1) / kEfChunkCols + (ld + tile_rows - 1) / tile_rows - 1);
    }
    const size_t state_bytes = (size_t)count * sizeof(EfWalkState);
    if (state_bytes > ws->state_bytes) {  // alloc waits for the stream's earlier rounds
        HIP_TRY(ws->state.alloc(state_bytes));
        ws->state_bytes = state_bytes;
    }
    if (!ws->counter.p) HIP_TRY(ws->counter.alloc(16));
    auto *state = ws->state.as<EfWalkState>();
    HIP_TRY(hipMemsetAsync(ws->counter.p, 0, sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(d_lens, 0xFF, (size_t)count * sizeof(uint32_t), s));
    if (xdrop == kEfNoXdrop)
        HIP_TRY(launch_ef_fill_keep(mode, d_pairs, 0, count, d_q, d_db, sc, d_sub, d_area, tile_rows, d_end_state,
                                    d_results, std::min(count, kEfLongWaves), ws->counter.as<uint32_t>(), s));
    else
        HIP_TRY(launch_ef_xdrop_fill_keep(d_pairs, 0, count, d_q, d_db, sc, d_sub, xdrop, d_area, tile_rows,
                                          d_end_state, d_results, std::min(count, kEfLongWaves),
                                          ws->counter.as<uint32_t>(), s));
    HIP_TRY(launch_ef_replay_start(mode, d_pairs, count, d_q, d_db, d_end_state, d_results, d_words, d_lens,
                                   state, s));
    // The walk's code is the plain replay's and finds the tile at
    // ef_replay_layout's offset.  Under X-drop it gets descriptors of its own:
    // the same pairs with code_off moved so that this offset lands on
    // ef_xdrop_replay_layout's tile.  The host copy lives in the workspace: the
    // caller syncs the stream before it runs the next replay.
    const EfPair *d_walk_pairs = d_pairs;
    if (xdrop != kEfNoXdrop) {
        ws->walk_pairs_host.assign(h_pairs, h_pairs + count);
        for (EfPair &p : ws->walk_pairs_host)
            p.code_off += ef_xdrop_replay_layout(p.lq, p.ld, tile_rows).tile - ef_replay_layout(p.lq, p.ld, tile_rows).tile;
        const size_t bytes = (size_t)count * sizeof(EfPair);
        if (bytes > ws->walk_pairs_bytes) {
            HIP_TRY(ws->walk_pairs.alloc(bytes));
            ws->walk_pairs_bytes = bytes;
        }
        HIP_TRY(hipMemcpyAsync(ws->walk_pairs.p, ws->walk_pairs_host.data(), bytes, hipMemcpyHostToDevice, s));
        d_walk_pairs = ws->walk_pairs.as<EfPair>();
    }
    for (uint64_t r = 0; r < rounds; ++r) {
        if (xdrop == kEfNoXdrop)
            HIP_TRY(launch_ef_tile_fill(mode, d_pairs, count, d_q, d_db, sc, d_sub, d_area, tile_rows, state, s));
        else
            HIP_TRY(launch_ef_xdrop_tile_fill(d_pairs, count, d_q, d_db, sc, d_sub, xdrop, d_area, tile_rows, state,
                                              s));
        HIP_TRY(launch_ef_tile_walk(mode, d_walk_pairs, count, d_q, d_db, d_area, tile_rows, d_results, d_words,
                                    d_lens, state, s));
    }
    return SALN_OK;
}

extern "C" {

int saln_ends_free_replay_bytes(uint64_t len_q, uint64_t len_db, uint32_t tile_rows, uint64_t *bytes) {
    if (!bytes) return SALN_E_INVALID;
    int32_t lf = 0;
    uint32_t chunks = 0;
    int rc = saln_ends_free_long_pair_path(len_q, len_db, &lf, &chunks);
    if (rc != SALN_OK) return rc;
    const int64_t R = tile_rows ? (int64_t)tile_rows : opt(Opt::EndsFreeTileRows);
    rc = check_tile_rows(R);
    if (rc != SALN_OK) return rc;
    if (!lf) return saln_ends_free_trace_bytes(len_q, len_db, bytes);
    *bytes = ef_replay_layout(len_q, len_db, (uint64_t)R).bytes;
    return SALN_OK;
}

int saln_ends_free_xdrop_replay_bytes(uint64_t len_q, uint64_t len_db, uint32_t tile_rows, uint64_t *bytes) {
    if (!bytes) return SALN_E_INVALID;
    int32_t lf = 0;
    uint32_t chunks = 0;
    int rc = saln_ends_free_long_pair_path(len_q, len_db, &lf, &chunks);
    if (rc != SALN_OK) return rc;
    const int64_t R = tile_rows ? (int64_t)tile_rows : opt(Opt::EndsFreeTileRows);
    rc = check_tile_rows(R);
    if (rc != SALN_OK) return rc;
    if (!lf) return saln_ends_free_trace_bytes(len_q, len_db, bytes);
    *bytes = ef_xdrop_replay_layout(len_q, len_db, (uint64_t)R).bytes;
    return SALN_OK;
}

namespace {

// The replay entry points: the batch with the context's tile rows, and with
// the X of their X-drop forms.
int replay_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                 const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                 const uint32_t *pair_db, uint64_t n_pairs, int32_t mode, const EfScoreSrc &scoring,
                 uint64_t trace_budget_bytes, int want_cigar, saln_ends_free_aln **out,
                 int32_t xdrop = kEfNoXdrop) {
    if (!ctx) return SALN_E_INVALID;
    const int64_t R = ctx->opts.effective()[Opt::EndsFreeTileRows];
    const int rc = check_tile_rows(R);
    if (rc != SALN_OK) return rc;
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          scoring, trace_budget_bytes, want_cigar, out, true, (uint32_t)R, xdrop);
}

}  // namespace

int saln_ends_free_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                      uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                      uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                      uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                                      uint64_t trace_budget_bytes, int want_cigar,
                                      saln_ends_free_aln **out) {
    return replay_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                        EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out);
}

int saln_ends_free_sub_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                          uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                          uint64_t trace_budget_bytes, int want_cigar,
                                          saln_ends_free_aln **out) {
    return replay_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                        EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out);
}

int saln_ends_free_xdrop_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                            uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                            uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                            uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                            uint64_t trace_budget_bytes, int want_cigar,
                                            saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;  // negative: refused with a message
    return replay_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                        SALN_MODE_EXTEND, EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out, xdrop);
}

int saln_ends_free_sub_xdrop_replay_align_batch(saln_context *ctx, const uint8_t *q_seq,
                                                const uint64_t *q_off, uint64_t n_q, const uint8_t *db_seq,
                                                const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                                const uint32_t *pair_db, uint64_t n_pairs,
                                                const saln_sub_matrix *matrix, int32_t xdrop,
                                                uint64_t trace_budget_bytes, int want_cigar,
                                                saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;
    return replay_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                        SALN_MODE_EXTEND, EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out, xdrop);
}

}  // extern "C"
