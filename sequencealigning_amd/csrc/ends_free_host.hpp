// What the two host files of the ends-free engine share: ends_free_host.cpp
// (saln_ends_free_*, the batch itself) and ends_free_long_host.cpp
// (saln_ends_free_long_*, the chunked fill's sizes, path and launches).
#pragma once
#include "ends_free.hpp"
#include "host_common.hpp"

namespace saln {

// The batch behind saln_ends_free_align_batch (long_ok = false: the classes'
// limits and refusals) and saln_ends_free_long_align_batch (long_ok = true:
// pairs above those limits run the chunked fill).  ends_free_host.cpp.
int ef_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                   const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                   const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                   const saln_nw_scoring *scoring, uint64_t trace_budget_bytes, int want_cigar,
                   saln_ends_free_aln **out, bool long_ok);

// Device workspace of a batch's chunked fills, all on one stream: the boundary
// slots (grown to the largest launch's need) and the pair counter.
struct EfLongWorkspace {
    DevBuf bnd, counter;
    size_t bnd_bytes = 0;
    EfLongWorkspace(saln_context *ctx, hipStream_t s) : bnd(ctx, s), counter(ctx, s) {}
};

// One chunked-fill launch of pairs[first .. first + count) with dbs of at most
// ld_max rows: ef_long_slots waves.  ends_free_long_host.cpp.
int ef_long_fill(EfLongWorkspace *ws, int32_t mode, const EfPair *d_pairs, uint32_t first,
                 uint32_t count, uint32_t ld_max, const uint8_t *d_q, const uint8_t *d_db,
                 const EfScoring &sc, uint8_t *d_codes, uint8_t *d_end_state,
                 saln_ends_free_result *d_results, hipStream_t s);

}  // namespace saln
