// C ABI of the ends-free engine for pairs of any length (include/saln.h,
// saln_ends_free_long_*).  The batch is ends_free_host.cpp's: pairs within
// the classes' limits run the class fills, every other pair the chunked fill
// (ends_free_long_kernels.hip); the walk, the gather, the trace-budget chunks
// and the result handle are shared.  This file holds what the long layout
// adds: its code size, the path decision as the C ABI reports it, and the
// launches with their bounded boundary workspace (ef_long_slots), and the
// X-drop forms of both (saln_ends_free_xdrop_long_*, ef_xdrop_long_slots).
#include <hip/hip_runtime.h>

#include <climits>

#include "ends_free_host.hpp"

using namespace saln;

int saln::ef_long_fill(EfLongWorkspace *ws, int32_t mode, const EfPair *d_pairs, uint32_t first,
                       uint32_t count, uint32_t ld_max, const uint8_t *d_q, const uint8_t *d_db,
                       const EfScoring &sc, const uint8_t *d_sub, uint8_t *d_codes, uint8_t *d_end_state,
                       saln_ends_free_result *d_results, hipStream_t s) {
    if (count == 0) return SALN_OK;
    const uint64_t slot_rows = ld_max ? ld_max : 1;
    const uint32_t slots = ef_long_slots(count, ld_max);
    const size_t bytes = (size_t)slots * slot_rows * 8;
    if (bytes > ws->bnd_bytes) {  // alloc waits for the stream's earlier fills
        HIP_TRY(ws->bnd.alloc(bytes));
        ws->bnd_bytes = bytes;
    }
    if (!ws->counter.p) HIP_TRY(ws->counter.alloc(16));
    HIP_TRY(hipMemsetAsync(ws->counter.p, 0, sizeof(uint32_t), s));
    HIP_TRY(launch_ef_fill_long(mode, d_pairs, first, count, d_q, d_db, sc, d_sub, d_codes, d_end_state,
                                d_results, ws->bnd.p, slot_rows, slots, ws->counter.as<uint32_t>(), s));
    return SALN_OK;
}

int saln::ef_xdrop_long_fill(EfLongWorkspace *ws, const EfPair *d_pairs, uint32_t first, uint32_t count,
                             uint32_t ld_max, const uint8_t *d_q, const uint8_t *d_db, const EfScoring &sc,
                             const uint8_t *d_sub, int32_t xdrop, uint8_t *d_codes, uint8_t *d_end_state,
                             saln_ends_free_result *d_results, hipStream_t s) {
    if (count == 0) return SALN_OK;
    const uint64_t slot_rows = ld_max ? ld_max : 1;
    const uint32_t slots = ef_xdrop_long_slots(count, ld_max);
    const size_t bytes = (size_t)slots * slot_rows * kEfXdropBndBytes;
    if (bytes > ws->bnd_bytes) {  // alloc waits for the stream's earlier fills
        HIP_TRY(ws->bnd.alloc(bytes));
        ws->bnd_bytes = bytes;
    }
    if (!ws->counter.p) HIP_TRY(ws->counter.alloc(16));
    HIP_TRY(hipMemsetAsync(ws->counter.p, 0, sizeof(uint32_t), s));
    HIP_TRY(launch_ef_xdrop_fill_long(d_pairs, first, count, d_q, d_db, sc, d_sub, xdrop, d_codes, d_end_state,
                                      d_results, ws->bnd.p, slot_rows, slots, ws->counter.as<uint32_t>(), s));
    return SALN_OK;
}

extern "C" {

int saln_ends_free_long_pair_path(uint64_t len_q, uint64_t len_db, int32_t *long_fill,
                                  uint32_t *chunks) {
    if (!long_fill || !chunks) return SALN_E_INVALID;
    if (len_q >= (1ull << 30) || len_db >= (1ull << 30) || len_q + len_db + 2 >= (1ull << 30)) {
        set_error("ends_free: len_q + len_db + 2 reaches 2^30: no scoring keeps the scores inside "
                  "the engine's int32 range");
        return SALN_E_INVALID;
    }
    const bool lf = ef_path_of(len_q, len_db, true) == kEfLongClass;
    *long_fill = lf ? 1 : 0;
    *chunks = lf && len_q ? (uint32_t)((len_q + kEfChunkCols - 1) / kEfChunkCols) : 1;
    return SALN_OK;
}

int saln_ends_free_long_trace_bytes(uint64_t len_q, uint64_t len_db, uint64_t *bytes) {
    if (!bytes) return SALN_E_INVALID;
    int32_t lf = 0;
    uint32_t chunks = 0;
    const int rc = saln_ends_free_long_pair_path(len_q, len_db, &lf, &chunks);
    if (rc != SALN_OK) return rc;
    if (!lf) return saln_ends_free_trace_bytes(len_q, len_db, bytes);
    *bytes = len_q && len_db ? (len_db * ef_long_row_bytes(len_q) + 7) & ~7ull : 0;
    return SALN_OK;
}

int saln_ends_free_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                    uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                    uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                    uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                                    uint64_t trace_budget_bytes, int want_cigar,
                                    saln_ends_free_aln **out) {
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out, true);
}

int saln_ends_free_sub_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                        uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                        uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                        uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                        uint64_t trace_budget_bytes, int want_cigar,
                                        saln_ends_free_aln **out) {
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out, true);
}

int saln_ends_free_xdrop_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                          uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                          uint64_t trace_budget_bytes, int want_cigar,
                                          saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;  // negative: refused with a message
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                          SALN_MODE_EXTEND, EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out,
                          true, 0, xdrop);
}

int saln_ends_free_sub_xdrop_long_align_batch(saln_context *ctx, const uint8_t *q_seq,
                                              const uint64_t *q_off, uint64_t n_q, const uint8_t *db_seq,
                                              const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                              const uint32_t *pair_db, uint64_t n_pairs,
                                              const saln_sub_matrix *matrix, int32_t xdrop,
                                              uint64_t trace_budget_bytes, int want_cigar,
                                              saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                          SALN_MODE_EXTEND, EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out,
                          true, 0, xdrop);
}

}  // extern "C"
