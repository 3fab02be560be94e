// C ABI of the ends-free engine (include/saln.h, saln_ends_free_*): local,
// semi-global, overlap and extension affine-gap alignment.  Not a
// reference-parity path - the reference only declares the first two modes
// (needleman_wunsch_affine.rs:238-239, :331-332, :433-434) and has no overlap
// and no extension; the checker of the four modes is the plain model
// tests/ends_free_model.py.
//
// A batch's pairs are grouped by query class (ef_class_of) and, within a
// class, ordered by falling db length and cut where the length's power-of-two
// bucket changes: one fill launch per cut, each staging rows of its own
// longest db.  Alignment mode packs the pairs in pair order into chunks of at
// most trace_budget_bytes of codes; per chunk the fill with codes, the walk,
// the words packed on the device in pair order, then the words back.  Pairs
// whose codes alone exceed the budget run in a score-only fill of their own.
//
// The batch (ef_align_batch) also serves saln_ends_free_long_align_batch
// (ends_free_long_host.cpp): with long_ok the pairs above this file's length
// limits are not refused but run the chunked fill, one more class to
// plan_launches; everything else is shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "ends_free_host.hpp"

using namespace saln;

namespace {

using Launch = EfLaunch;

int bit_bucket(uint32_t v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// Orders pairs for the fill (class, then falling db length) and cuts them
// into launches.  long_ok: the chunked fill is one more class (ef_path_of).
void plan_launches(std::vector<EfPair> *pairs, std::vector<Launch> *out, bool long_ok = false) {
    std::stable_sort(pairs->begin(), pairs->end(), [long_ok](const EfPair &a, const EfPair &b) {
        const int ca = ef_path_of(a.lq, a.ld, long_ok), cb = ef_path_of(b.lq, b.ld, long_ok);
        return ca != cb ? ca < cb : a.ld > b.ld;
    });
    out->clear();
    for (uint32_t k = 0; k < pairs->size(); ++k) {
        const EfPair &p = (*pairs)[k];
        const int cls = ef_path_of(p.lq, p.ld, long_ok);
        if (out->empty() || out->back().cls != cls ||
            bit_bucket(out->back().ld_max) != bit_bucket(p.ld))
            out->push_back(Launch{cls, k, 0, p.ld});
        ++out->back().count;
    }
}

int check_mode(int32_t mode) {
    if (mode == SALN_MODE_LOCAL || mode == SALN_MODE_SEMI_GLOBAL || mode == SALN_MODE_OVERLAP ||
        mode == SALN_MODE_EXTEND)
        return SALN_OK;
    if (mode == SALN_MODE_GLOBAL)
        set_error("ends_free: SALN_MODE_GLOBAL is not an ends-free mode; global alignment is "
                  "saln_nw_align / saln_nw_align_batch / saln_nw_plan_create");
    else
        set_error("ends_free: unknown mode " + std::to_string(mode));
    return SALN_E_INVALID;
}

// The device block of a matrix that saln_sub_matrix_check has passed
// (ends_free.hpp: the layout and the pad column's invariant).
std::vector<uint8_t> sub_block(const saln_sub_matrix &m) {
    std::vector<uint8_t> b(kEfSubBytes, (uint8_t)kEfSubPadScore);
    std::copy(m.code, m.code + 256, b.begin());
    for (uint32_t r = 0; r < m.n_sym; ++r)
        for (uint32_t c = 0; c < m.n_sym; ++c)
            b[kEfSubCodeBytes + r * kEfSubStride + c] = (uint8_t)m.score[r][c];
    return b;
}

// The scoring a batch or a plan runs under: sc (a matrix leaves match and
// mismatch 0: its fills never read them), the range guard's factor, and the
// matrix's device block (empty under the scalar scoring).
int make_scoring(const EfScoreSrc &src, EfScoring *out, uint64_t *max_abs, std::vector<uint8_t> *block) {
    block->clear();
    if (src.is_sub) {
        int32_t mx = 0;
        const int rc = saln_sub_matrix_check(src.sub, &mx);
        if (rc != SALN_OK) return rc;
        *out = EfScoring{0, 0, src.sub->gap_open, src.sub->gap_extend};
        *max_abs = (uint64_t)mx;
        *block = sub_block(*src.sub);
        return SALN_OK;
    }
    const saln_nw_scoring *s = src.scalar;
    const EfScoring sc = s ? EfScoring{s->match, s->mismatch, s->gap_open, s->gap_extend}
                           : EfScoring{5, -4, -8, -6};
    if (sc.match <= 0 || sc.mismatch >= 0 || sc.open > 0 || sc.extend >= 0) {
        set_error("ends_free: scoring {" + std::to_string(sc.match) + ", " + std::to_string(sc.mismatch) +
                  ", " + std::to_string(sc.open) + ", " + std::to_string(sc.extend) +
                  "} is outside this engine's domain (match > 0, mismatch < 0, gap_open <= 0, "
                  "gap_extend < 0)");
        return SALN_E_INVALID;
    }
    const auto mag = [](int32_t v) { return (uint64_t)(v < 0 ? -(int64_t)v : (int64_t)v); };
    *max_abs = std::max({mag(sc.match), mag(sc.mismatch), mag(sc.open), mag(sc.extend)});
    *out = sc;
    return SALN_OK;
}

// An X-drop call's X (kEfNoXdrop: none): >= 0, and extension only (the class
// fills, the chunked fill and the tiled replay have X-drop forms).
int check_xdrop(int32_t xdrop, int32_t mode) {
    if (xdrop == kEfNoXdrop) return SALN_OK;
    if (xdrop < 0) {
        set_error("ends_free: xdrop " + std::to_string(xdrop) + " is negative (X >= 0)");
        return SALN_E_INVALID;
    }
    if (mode != SALN_MODE_EXTEND) {
        set_error("ends_free: X-drop is part of SALN_MODE_EXTEND");
        return SALN_E_INVALID;
    }
    return SALN_OK;
}

// The engine's limits for one pair (lengths, int32 range of the values).
// long_ok: the chunked fill takes the lengths the classes refuse.  xdrop (an
// X-drop call's X, else 0) is part of the range guard: everything derived from
// -infinity must stay below -X.
int check_pair(uint64_t lq, uint64_t ld, uint64_t max_abs, bool long_ok = false, uint64_t xdrop = 0) {
    if (lq > kEfMaxQ && !long_ok) {
        set_error("ends_free: a query of " + std::to_string(lq) + " columns is above the limit of " +
                  std::to_string(kEfMaxQ) + " (one chunk of the lane fill); "
                  "saln_ends_free_long_align_batch takes longer pairs");
        return SALN_E_INVALID;
    }
    if (ld > kEfMaxDb && !long_ok) {
        set_error("ends_free: a db of " + std::to_string(ld) + " rows is above the limit of " +
                  std::to_string(kEfMaxDb) + " (the db row is staged in LDS); "
                  "saln_ends_free_long_align_batch takes longer pairs");
        return SALN_E_INVALID;
    }
    if ((lq + ld + 2) * max_abs + xdrop >= (1ull << 30)) {
        set_error(std::string("ends_free: (len_q + len_db + 2) * max|scoring parameter|") +
                  (xdrop ? " + xdrop" : "") + " reaches 2^30: the scores could leave the engine's int32 range");
        return SALN_E_INVALID;
    }
    return SALN_OK;
}

uint64_t code_bytes(uint64_t lq, uint64_t ld) {
    if (lq == 0 || ld == 0) return 0;
    return (ld * ef_row_bytes(lq) + 7) & ~7ull;
}

// The same under the long entry points, which own the long layout's size, and
// (tile_rows != 0) under the replay entry points, which own the footprints
// (xdrop: the X-drop form's).
uint64_t code_bytes(uint64_t lq, uint64_t ld, bool long_ok, uint32_t tile_rows, bool xdrop) {
    uint64_t bytes = 0;
    if (!long_ok) return code_bytes(lq, ld);
    if (tile_rows && xdrop)
        return saln_ends_free_xdrop_replay_bytes(lq, ld, tile_rows, &bytes) == SALN_OK ? bytes : 0;
    if (tile_rows) return saln_ends_free_replay_bytes(lq, ld, tile_rows, &bytes) == SALN_OK ? bytes : 0;
    return saln_ends_free_long_trace_bytes(lq, ld, &bytes) == SALN_OK ? bytes : 0;
}

int build_pairs(const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off, uint64_t n_db,
                const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, uint64_t max_abs,
                std::vector<EfPair> *out, bool long_ok = false, int32_t xdrop = kEfNoXdrop) {
    out->resize(n_pairs);
    const PairIndex pairs{pair_q, pair_db, n_q, n_db};
    for (uint64_t k = 0; k < n_pairs; ++k) {
        uint64_t qi, di;
        if (!pairs.at(k, &qi, &di)) return SALN_E_INVALID;
        const uint64_t lq = q_off[qi + 1] - q_off[qi], ld = db_off[di + 1] - db_off[di];
        const int rc = check_pair(lq, ld, max_abs, long_ok, xdrop == kEfNoXdrop ? 0 : (uint64_t)xdrop);
        if (rc != SALN_OK) return rc;
        EfPair p{};
        p.q_off = q_off[qi];
        p.d_off = db_off[di];
        p.lq = (uint32_t)lq;
        p.ld = (uint32_t)ld;
        p.out = (uint32_t)k;
        p.row_bytes = (uint32_t)ef_path_row_bytes(ef_path_of(lq, ld, long_ok), lq);
        (*out)[k] = p;
    }
    return SALN_OK;
}

// The fills of `pairs` (device copy d_pairs, in plan_launches' order).  ws:
// the chunked fill's workspace (launches of kEfLongClass need one).  xdrop:
// kEfNoXdrop or X: every launch then runs its fill's X-drop form.
int run_fills(const std::vector<Launch> &launches, int32_t mode, const EfPair *d_pairs,
              const uint8_t *d_q, const uint8_t *d_db, const EfScoring &sc, const uint8_t *d_sub,
              uint8_t *d_codes, uint8_t *d_end_state, saln_ends_free_result *d_results, hipStream_t s,
              EfLongWorkspace *ws = nullptr, int32_t xdrop = kEfNoXdrop) {
    for (const Launch &l : launches) {
        if (l.cls == kEfLongClass) {
            if (!ws) return SALN_E_INVALID;
            const int rc = xdrop == kEfNoXdrop
                               ? ef_long_fill(ws, mode, d_pairs, l.first, l.count, l.ld_max, d_q, d_db, sc, d_sub,
                                              d_codes, d_end_state, d_results, s)
                               : ef_xdrop_long_fill(ws, d_pairs, l.first, l.count, l.ld_max, d_q, d_db, sc, d_sub,
                                                    xdrop, d_codes, d_end_state, d_results, s);
            if (rc != SALN_OK) return rc;
            continue;
        }
        HIP_TRY(launch_ef_fill(l.cls, mode, d_pairs, l.first, l.count, l.ld_max, d_q, d_db, sc, d_sub,
                               d_codes, d_end_state, d_results, s, xdrop));
    }
    return SALN_OK;
}

}  // namespace

// What the score entry points (ends_free_score_host.cpp) take from this file.
int saln::ef_check_mode(int32_t mode) { return check_mode(mode); }
int saln::ef_make_scoring(const EfScoreSrc &src, EfScoring *out, uint64_t *max_abs, std::vector<uint8_t> *block) {
    return make_scoring(src, out, max_abs, block);
}
int saln::ef_check_pair(uint64_t lq, uint64_t ld, uint64_t max_abs) { return check_pair(lq, ld, max_abs); }
int saln::ef_build_pairs(const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off, uint64_t n_db,
                         const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, uint64_t max_abs,
                         std::vector<EfPair> *out) {
    return build_pairs(q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, max_abs, out);
}
void saln::ef_plan_launches(std::vector<EfPair> *pairs, std::vector<EfLaunch> *out) { plan_launches(pairs, out); }

struct saln_ends_free_plan {
    saln_context *ctx = nullptr;
    EfScoring sc{};
    int32_t mode = SALN_MODE_LOCAL;
    int32_t xdrop = kEfNoXdrop;
    uint64_t n = 0;
    std::vector<Launch> launches;
    DevBuf d_pairs, d_sub;  // d_sub: the matrix's block (empty: scalar scoring)
};

// The result handle of saln_ends_free_align_batch: pair k's words are
// words[off[k] .. off[k] + res[k].cigar_len).
struct saln_ends_free_aln {
    std::vector<saln_ends_free_result> res;
    std::vector<uint64_t> off;
    std::vector<uint32_t> words;
};

extern "C" {

int saln_ends_free_pair_geometry(uint64_t len_q, uint32_t *lanes, uint32_t *cols_per_lane) {
    if (!lanes || !cols_per_lane) return SALN_E_INVALID;
    const int c = ef_class_of(len_q);
    if (c < 0) return check_pair(len_q, 0, 0);
    *lanes = (uint32_t)kEfClass[c].lanes;
    *cols_per_lane = (uint32_t)kEfClass[c].cols;
    return SALN_OK;
}

int saln_ends_free_fill_geometry(uint64_t len_q, uint64_t ld_max, int has_matrix, uint32_t *groups,
                                 uint32_t *lds_bytes) {
    if (!groups || !lds_bytes) return SALN_E_INVALID;
    const int rc = check_pair(len_q, ld_max, 0);
    if (rc != SALN_OK) return rc;
    const EfFillGeometry g = ef_fill_geometry(ef_class_of(len_q), (uint32_t)ld_max, has_matrix != 0);
    *groups = g.groups;
    *lds_bytes = (uint32_t)g.lds_bytes;
    return SALN_OK;
}

int saln_ends_free_trace_bytes(uint64_t len_q, uint64_t len_db, uint64_t *bytes) {
    if (!bytes) return SALN_E_INVALID;
    const int rc = check_pair(len_q, len_db, 0);
    if (rc != SALN_OK) return rc;
    *bytes = code_bytes(len_q, len_db);
    return SALN_OK;
}

int saln_sub_matrix_check(const saln_sub_matrix *m, int32_t *max_abs) {
    if (!m) {
        set_error("ends_free: the substitution matrix is NULL");
        return SALN_E_INVALID;
    }
    if (m->n_sym < 1 || m->n_sym > kEfSubSyms) {
        set_error("ends_free: substitution matrix n_sym " + std::to_string(m->n_sym) +
                  " is outside 1 .. " + std::to_string(kEfSubSyms));
        return SALN_E_INVALID;
    }
    if (m->reserved[0] || m->reserved[1] || m->reserved[2]) {
        set_error("ends_free: substitution matrix reserved bytes must be 0");
        return SALN_E_INVALID;
    }
    for (int b = 0; b < 256; ++b)
        if (m->code[b] >= m->n_sym) {
            set_error("ends_free: substitution matrix code[" + std::to_string(b) + "] = " +
                      std::to_string(m->code[b]) + " is not below n_sym " + std::to_string(m->n_sym));
            return SALN_E_INVALID;
        }
    if (m->gap_open > 0 || m->gap_extend >= 0) {
        set_error("ends_free: substitution matrix gaps {" + std::to_string(m->gap_open) + ", " +
                  std::to_string(m->gap_extend) + "} are outside this engine's domain (gap_open <= 0, "
                  "gap_extend < 0)");
        return SALN_E_INVALID;
    }
    const auto mag = [](int64_t v) { return v < 0 ? -v : v; };
    int64_t mx = std::max(mag(m->gap_open), mag(m->gap_extend));
    bool positive = false;
    for (uint32_t r = 0; r < m->n_sym; ++r)
        for (uint32_t c = 0; c < m->n_sym; ++c) {
            positive = positive || m->score[r][c] > 0;
            mx = std::max(mx, mag(m->score[r][c]));
        }
    if (!positive) {
        set_error("ends_free: substitution matrix has no entry > 0 inside n_sym x n_sym: no pair "
                  "could score above 0");
        return SALN_E_INVALID;
    }
    if (max_abs) *max_abs = (int32_t)std::min<int64_t>(mx, INT32_MAX);
    return SALN_OK;
}

int saln_ends_free_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                               const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                               const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                               const saln_nw_scoring *scoring, saln_ends_free_plan **out) {
    return ef_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(scoring), out);
}

int saln_ends_free_sub_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                   const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                   const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                   const saln_sub_matrix *matrix, saln_ends_free_plan **out) {
    return ef_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(matrix), out);
}

int saln_ends_free_xdrop_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                     const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                     const uint32_t *pair_db, uint64_t n_pairs,
                                     const saln_nw_scoring *scoring, int32_t xdrop,
                                     saln_ends_free_plan **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;  // negative: refused with a message
    return ef_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, SALN_MODE_EXTEND,
                          EfScoreSrc::of(scoring), out, xdrop);
}

int saln_ends_free_sub_xdrop_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                         const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                         const uint32_t *pair_db, uint64_t n_pairs,
                                         const saln_sub_matrix *matrix, int32_t xdrop,
                                         saln_ends_free_plan **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;
    return ef_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, SALN_MODE_EXTEND,
                          EfScoreSrc::of(matrix), out, xdrop);
}

}  // extern "C"

int saln::ef_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off,
                         uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                         uint64_t n_pairs, int32_t mode, const EfScoreSrc &scoring,
                         saln_ends_free_plan **out, int32_t xdrop) {
    if (!ctx || !q_off || !db_off || !out || n_pairs > 0xFFFFFFFFull) return SALN_E_INVALID;
    if (!PairIndex{pair_q, pair_db, n_q, n_db}.complete(n_pairs)) return SALN_E_INVALID;
    auto p = std::make_unique<saln_ends_free_plan>();
    p->ctx = ctx;
    p->d_pairs = DevBuf(ctx);
    p->d_sub = DevBuf(ctx);
    uint64_t max_abs = 0;
    std::vector<uint8_t> block;
    int rc = check_mode(mode);
    if (rc == SALN_OK) rc = check_xdrop(xdrop, mode);
    if (rc == SALN_OK) rc = make_scoring(scoring, &p->sc, &max_abs, &block);
    std::vector<EfPair> pairs;
    if (rc == SALN_OK)
        rc = build_pairs(q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, max_abs, &pairs, false, xdrop);
    if (rc != SALN_OK) return rc;
    p->mode = mode;
    p->xdrop = xdrop;
    p->n = n_pairs;
    plan_launches(&pairs, &p->launches);
    HIP_TRY(hipSetDevice(ctx->device));
    if (n_pairs) {
        HIP_TRY(p->d_pairs.alloc(n_pairs * sizeof(EfPair)));
        HIP_TRY(hipMemcpy(p->d_pairs.p, pairs.data(), n_pairs * sizeof(EfPair), hipMemcpyHostToDevice));
    }
    if (!block.empty()) {
        HIP_TRY(p->d_sub.alloc(block.size()));
        HIP_TRY(hipMemcpy(p->d_sub.p, block.data(), block.size(), hipMemcpyHostToDevice));
    }
    *out = p.release();
    return SALN_OK;
}

extern "C" {

int saln_ends_free_execute(saln_ends_free_plan *p, const uint8_t *d_q_seq, const uint8_t *d_db_seq,
                           saln_ends_free_result *d_results, void *stream) {
    if (!p || !d_results || !d_q_seq || !d_db_seq) return SALN_E_INVALID;
    if (!p->n) return SALN_OK;
    hipStream_t s = resolve_stream(stream, p->ctx);
    HIP_TRY(hipSetDevice(p->ctx->device));
    return run_fills(p->launches, p->mode, p->d_pairs.as<EfPair>(), d_q_seq, d_db_seq, p->sc,
                     p->d_sub.as<uint8_t>(), nullptr, nullptr, d_results, s, nullptr, p->xdrop);
}

int saln_ends_free_plan_destroy(saln_ends_free_plan *p) {
    delete p;
    return SALN_OK;
}

}  // extern "C"

// saln_ends_free_align_batch (long_ok = false) and
// saln_ends_free_long_align_batch (true): the same batch, with or without the
// chunked fill for the pairs the classes refuse.  saln_ends_free_replay_align_batch
// (long_ok and tile_rows != 0): a chunk's bytes are the pairs' replay
// footprints, and its pairs of the chunked path run ef_replay_run in place of
// the fill with codes and ef_walk_kernel.  With an X on top
// (saln_ends_free_xdrop_replay_align_batch) the footprints are the X-drop
// form's, 16-byte aligned, and ef_replay_run takes the X.
int saln::ef_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                         const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                         const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                         int32_t mode, const EfScoreSrc &scoring, uint64_t trace_budget_bytes,
                         int want_cigar, saln_ends_free_aln **out, bool long_ok, uint32_t tile_rows,
                         int32_t xdrop) {
    if (!ctx || !q_off || !db_off || !out || n_pairs > 0xFFFFFFFFull) return SALN_E_INVALID;
    if (!PairIndex{pair_q, pair_db, n_q, n_db}.complete(n_pairs)) return SALN_E_INVALID;
    EfScoring sc{};
    uint64_t max_abs = 0;
    std::vector<uint8_t> block;
    int rc = check_mode(mode);
    if (rc == SALN_OK) rc = check_xdrop(xdrop, mode);
    if (rc == SALN_OK) rc = make_scoring(scoring, &sc, &max_abs, &block);
    std::vector<EfPair> all;
    if (rc == SALN_OK)
        rc = build_pairs(q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, max_abs, &all, long_ok, xdrop);
    if (rc != SALN_OK) return rc;
    auto aln = std::make_unique<saln_ends_free_aln>();
    aln->off.assign(n_pairs + 1, 0);
    if (n_pairs == 0) {
        *out = aln.release();
        return SALN_OK;
    }
    aln->res.assign(n_pairs, saln_ends_free_result{});

    // chunks: pairs in pair order, at most `budget` bytes of codes each; the
    // pairs without codes (score only, or above the budget) in one more
    const uint64_t budget = trace_budget_bytes ? trace_budget_bytes : (1ull << 30);
    struct Chunk {
        std::vector<EfPair> pairs;
        uint64_t bytes = 0, words = 0;
    };
    std::vector<Chunk> chunks;
    Chunk plain;
    std::vector<uint8_t> capped(n_pairs, 0), unfinished(tile_rows ? n_pairs : 0, 0);
    for (uint64_t k = 0; k < n_pairs; ++k) {
        EfPair p = all[k];
        const uint64_t bytes = code_bytes(p.lq, p.ld, long_ok, tile_rows, xdrop != kEfNoXdrop);
        if (!want_cigar || bytes > budget) {
            capped[k] = want_cigar ? 1 : 0;
            plain.pairs.push_back(p);
            continue;
        }
        // an X-drop replay area holds int4 entries: it starts 16-byte aligned
        // (class codes before it in the chunk are multiples of 8 only)
        const uint64_t align = tile_rows && xdrop != kEfNoXdrop && ef_path_of(p.lq, p.ld, true) == kEfLongClass
                                   ? 15u : 0u;
        if (chunks.empty() || ((chunks.back().bytes + align) & ~align) + bytes > budget ||
            chunks.back().pairs.size() >= (1u << 30))
            chunks.emplace_back();
        Chunk &c = chunks.back();
        c.bytes = (c.bytes + align) & ~align;
        p.code_off = c.bytes;
        p.cig_off = c.words;
        c.bytes += bytes;
        c.words += (uint64_t)p.lq + p.ld;
        c.pairs.push_back(p);
    }
    std::vector<EfPair>().swap(all);
    uint64_t max_bytes = 0, max_words = 0, max_n = plain.pairs.size();
    for (const Chunk &c : chunks) {
        max_bytes = std::max(max_bytes, c.bytes);
        max_words = std::max(max_words, c.words);
        max_n = std::max<uint64_t>(max_n, c.pairs.size());
    }

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;  // every launch below runs on it: the blocks sync it alone
    DevBuf dq(ctx, s), dd(ctx, s), d_pairs(ctx, s), d_res(ctx, s), d_codes(ctx, s), d_words(ctx, s),
        d_state(ctx, s), d_lens(ctx, s), d_dst(ctx, s), d_packed(ctx, s), d_sub(ctx, s);
    const auto min16 = [](size_t n) { return std::max<size_t>(n, 16); };
    HIP_TRY(upload_seqs(dq, dd, q_seq, q_off, n_q, db_seq, db_off, n_db, 16));
    HIP_TRY(d_pairs.alloc(min16(max_n * sizeof(EfPair))));
    HIP_TRY(d_res.alloc(min16(n_pairs * sizeof(saln_ends_free_result))));
    if (!block.empty()) {  // the matrix, once per call; `block` outlives every sync below
        HIP_TRY(d_sub.alloc(block.size()));
        HIP_TRY(hipMemcpyAsync(d_sub.p, block.data(), block.size(), hipMemcpyHostToDevice, s));
    }
    const uint8_t *sub = d_sub.as<uint8_t>();
    if (!chunks.empty()) {
        HIP_TRY(d_codes.alloc(min16(max_bytes)));
        HIP_TRY(d_words.alloc(min16(max_words * sizeof(uint32_t))));
        HIP_TRY(d_packed.alloc(min16(max_words * sizeof(uint32_t))));
        HIP_TRY(d_state.alloc(min16(n_pairs)));
        HIP_TRY(d_lens.alloc(min16(max_n * sizeof(uint32_t))));
        HIP_TRY(d_dst.alloc(min16(max_n * sizeof(uint64_t))));
    }
    const uint8_t *sq = dq.as<uint8_t>(), *sd = dd.as<uint8_t>();
    auto *results = d_res.as<saln_ends_free_result>();
    std::vector<Launch> launches;
    EfLongWorkspace ws(ctx, s);
    EfReplayWorkspace rws(ctx, s);

    if (!plain.pairs.empty()) {
        plan_launches(&plain.pairs, &launches, long_ok);
        HIP_TRY(hipMemcpyAsync(d_pairs.p, plain.pairs.data(), plain.pairs.size() * sizeof(EfPair),
                               hipMemcpyHostToDevice, s));
        rc = run_fills(launches, mode, d_pairs.as<EfPair>(), sq, sd, sc, sub, nullptr, nullptr, results,
                       s, &ws, xdrop);
        if (rc != SALN_OK) return rc;
        HIP_TRY(hipStreamSynchronize(s));  // d_pairs and the host vector are reused
    }
    // Per chunk: the fills with codes and the walk (each pair's words at the
    // end of its own area), the word counts back, then the words packed on
    // the device in pair order and copied to the end of the handle's words:
    // chunks hold rising pair indices, so the handle's words stay in pair order.
    constexpr uint64_t kNoWords = ~0ull;
    std::fill(aln->off.begin(), aln->off.end(), kNoWords);
    std::vector<uint32_t> lens, order;
    std::vector<uint64_t> dst;
    for (Chunk &c : chunks) {
        const uint32_t n = (uint32_t)c.pairs.size();
        // the fills and the walk read the same descriptors, in the fills' order
        plan_launches(&c.pairs, &launches, long_ok);
        HIP_TRY(hipMemcpyAsync(d_pairs.p, c.pairs.data(), n * sizeof(EfPair), hipMemcpyHostToDevice, s));
        // replay: the pairs of the chunked path, the plan's last, walk tile by tile
        uint32_t n_walk = n;
        if (tile_rows)
            while (!launches.empty() && launches.back().cls == kEfLongClass) {
                n_walk = launches.back().first;
                launches.pop_back();
            }
        rc = run_fills(launches, mode, d_pairs.as<EfPair>(), sq, sd, sc, sub, d_codes.as<uint8_t>(),
                       d_state.as<uint8_t>(), results, s, &ws, xdrop);
        if (rc != SALN_OK) return rc;
        HIP_TRY(launch_ef_walk(mode, d_pairs.as<EfPair>(), n_walk, sq, sd, d_codes.as<uint8_t>(),
                               d_state.as<uint8_t>(), results, d_words.as<uint32_t>(),
                               d_lens.as<uint32_t>(), s));
        if (n_walk < n) {
            rc = ef_replay_run(&rws, mode, c.pairs.data() + n_walk, d_pairs.as<EfPair>() + n_walk, n - n_walk,
                               sq, sd, sc, sub, d_codes.as<uint8_t>(), tile_rows, d_state.as<uint8_t>(), results,
                               d_words.as<uint32_t>(), d_lens.as<uint32_t>() + n_walk, s, xdrop);
            if (rc != SALN_OK) return rc;
        }
        lens.resize(n);
        HIP_TRY(hipMemcpyAsync(lens.data(), d_lens.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        order.resize(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        std::sort(order.begin(), order.end(),
                  [&](uint32_t x, uint32_t y) { return c.pairs[x].out < c.pairs[y].out; });
        dst.resize(n);
        const uint64_t base = aln->words.size();
        uint64_t total = 0;
        for (const uint32_t i : order) {
            const EfPair &p = c.pairs[i];
            if (i >= n_walk && lens[i] == kEfWalkUnfinished) {  // never expected: no words
                unfinished[p.out] = 1;
                lens[i] = 0;
            }
            lens[i] = std::min(lens[i], p.lq + p.ld);
            dst[i] = total;
            aln->off[p.out] = base + total;
            total += lens[i];
        }
        if (total) {
            HIP_TRY(hipMemcpyAsync(d_dst.p, dst.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            HIP_TRY(launch_ef_gather(d_pairs.as<EfPair>(), n, d_words.as<uint32_t>(),
                                     d_lens.as<uint32_t>(), d_dst.as<uint64_t>(),
                                     d_packed.as<uint32_t>(), s));
            aln->words.resize(base + total);
            HIP_TRY(hipMemcpyAsync(aln->words.data() + base, d_packed.p, total * sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        std::vector<EfPair>().swap(c.pairs);
    }
    HIP_TRY(hipMemcpy(aln->res.data(), d_res.p, n_pairs * sizeof(saln_ends_free_result),
                      hipMemcpyDeviceToHost));
    // pairs without words sit where the next pair's words begin
    uint64_t cur = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        saln_ends_free_result &r = aln->res[k];
        if (capped[k]) r.status = SALN_TRACE_CAP;
        if (tile_rows && unfinished[k]) r.status = SALN_INTERNAL;
        if (aln->off[k] == kNoWords) {
            aln->off[k] = cur;
            r.cigar_len = 0;
        } else {
            r.cigar_len = (uint32_t)std::min<uint64_t>(r.cigar_len, aln->words.size() - aln->off[k]);
            cur = aln->off[k] + r.cigar_len;
        }
    }
    aln->off[n_pairs] = aln->words.size();
    *out = aln.release();
    return SALN_OK;
}

extern "C" {

int saln_ends_free_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                               uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                               uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                               uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                               uint64_t trace_budget_bytes, int want_cigar,
                               saln_ends_free_aln **out) {
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out, false);
}

int saln_ends_free_sub_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                   uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                   uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                   uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                   uint64_t trace_budget_bytes, int want_cigar,
                                   saln_ends_free_aln **out) {
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                          EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out, false);
}

int saln_ends_free_xdrop_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                     uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                     uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                     uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                     uint64_t trace_budget_bytes, int want_cigar,
                                     saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;  // negative: refused with a message
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                          SALN_MODE_EXTEND, EfScoreSrc::of(scoring), trace_budget_bytes, want_cigar, out,
                          false, 0, xdrop);
}

int saln_ends_free_sub_xdrop_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                         uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                         uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                         uint64_t n_pairs, const saln_sub_matrix *matrix, int32_t xdrop,
                                         uint64_t trace_budget_bytes, int want_cigar,
                                         saln_ends_free_aln **out) {
    if (xdrop == kEfNoXdrop) xdrop = INT32_MIN;
    return ef_align_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                          SALN_MODE_EXTEND, EfScoreSrc::of(matrix), trace_budget_bytes, want_cigar, out,
                          false, 0, xdrop);
}

uint64_t saln_ends_free_aln_count(const saln_ends_free_aln *a) { return a ? a->res.size() : 0; }

int saln_ends_free_aln_get(const saln_ends_free_aln *a, uint64_t pair, saln_ends_free_result *res,
                           const uint32_t **cigar) {
    if (!a || pair >= a->res.size()) return SALN_E_INVALID;
    if (res) *res = a->res[pair];
    if (cigar) *cigar = a->words.data() + a->off[pair];
    return SALN_OK;
}

void saln_ends_free_aln_free(saln_ends_free_aln *a) { delete a; }

}  // extern "C"
