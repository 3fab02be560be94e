// C ABI of the score-only search of the ends-free engine (include/saln.h,
// saln_ends_free_score_*): what does each of these pairs
// score?  One int32 per pair, exactly the `score` of saln_ends_free_align_batch.
//
// A pair runs the packed-i16 fill (ends_free_score_kernels.hip, two pairs per
// lane group) where ef_score_packed allows it, else the class fill's i32
// score-only instances (ends_free_kernels.hip, unchanged), whose records a
// small gather turns into scores.  Packed pairs are ordered by class and
// falling db length, cut into launches where the length's power-of-two bucket
// changes (dbs of fewer than 64 rows share one), and matched two by two inside
// a launch: neighbours in db length share a group, whose longer db sets the
// step count.  A launch with an odd count ends in a group of one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "ends_free_host.hpp"
#include "ends_free_score.hpp"

using namespace saln;

namespace {

// S+ of ef_score_packed: match, or the matrix's largest entry, at least 0.
uint64_t max_positive(const EfScoreSrc &src, const EfScoring &sc) {
    if (!src.is_sub) return (uint64_t)std::max<int32_t>(sc.match, 0);
    int32_t mx = 0;
    for (uint32_t r = 0; r < src.sub->n_sym; ++r)
        for (uint32_t c = 0; c < src.sub->n_sym; ++c) mx = std::max<int32_t>(mx, src.sub->score[r][c]);
    return (uint64_t)mx;
}

// Option "ends_free.score_i16": 1 the packed fill where it fits, 0 the i32 fill
// for every pair.
int check_score_i16(int64_t v) {
    if (v == 0 || v == 1) return SALN_OK;
    set_error("ends_free: option ends_free.score_i16 = " + std::to_string(v) + " is neither 0 nor 1");
    return SALN_E_INVALID;
}

// The bucket of a db length that cuts the packed launches: the power of two
// above it, and one bucket for every db of fewer than 64 rows.  A group runs
// max(m_a, m_b) + lanes - 1 steps, so among such dbs the skew is most of a
// pair's steps whatever its partner's length, and short and empty dbs find a
// partner.
int packed_bucket(uint32_t ld) {
    int b = 0;
    for (uint32_t v = std::max(ld, 32u); v; v >>= 1) ++b;
    return b;
}

}  // namespace

struct saln_ends_free_score_plan {
    saln_context *ctx = nullptr;
    EfScoring sc{};
    int32_t mode = SALN_MODE_LOCAL;
    uint64_t n = 0, n_packed = 0, n_i32 = 0;
    std::vector<EfLaunch> pk;   // over d_groups: first and count in groups
    std::vector<EfLaunch> i32;  // over d_pairs
    // d_res: the i32 fills' records, d_out: their pairs' indices in the
    // caller's order.  The plan owns them: its executes must not overlap.
    DevBuf d_groups, d_pairs, d_out, d_res, d_sub;
};

namespace {

int score_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off,
                      uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                      int32_t mode, const EfScoreSrc &scoring, saln_ends_free_score_plan **out) {
    if (!ctx || !q_off || !db_off || !out || n_pairs > 0xFFFFFFFFull) return SALN_E_INVALID;
    if (!PairIndex{pair_q, pair_db, n_q, n_db}.complete(n_pairs)) return SALN_E_INVALID;
    auto p = std::make_unique<saln_ends_free_score_plan>();
    p->ctx = ctx;
    for (DevBuf *b : {&p->d_groups, &p->d_pairs, &p->d_out, &p->d_res, &p->d_sub}) *b = DevBuf(ctx);
    uint64_t max_abs = 0;
    std::vector<uint8_t> block;
    int rc = ef_check_mode(mode);
    if (rc == SALN_OK) rc = ef_make_scoring(scoring, &p->sc, &max_abs, &block);
    const int64_t i16 = ctx->opts.effective()[Opt::EndsFreeScoreI16];
    if (rc == SALN_OK) rc = check_score_i16(i16);
    std::vector<EfPair> all;
    if (rc == SALN_OK) rc = ef_build_pairs(q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, max_abs, &all);
    if (rc != SALN_OK) return rc;
    p->mode = mode;
    p->n = n_pairs;

    const uint64_t max_pos = max_positive(scoring, p->sc);
    std::vector<EfPair> packed, plain;
    for (const EfPair &q : all)
        (i16 && ef_score_packed(q.lq, q.ld, mode, max_pos, max_abs) ? packed : plain).push_back(q);
    p->n_packed = packed.size();
    p->n_i32 = plain.size();

    // the i32 pairs: records 0 .. n_i32 - 1, and where each one's score goes
    ef_plan_launches(&plain, &p->i32);
    std::vector<uint32_t> out_idx(plain.size());
    for (uint32_t k = 0; k < plain.size(); ++k) {
        out_idx[k] = plain[k].out;
        plain[k].out = k;
    }
    // the packed pairs: by class and falling db length, cut where the length's
    // bucket changes, then two by two; of a group's two pairs the earlier in
    // the caller's order is A
    std::stable_sort(packed.begin(), packed.end(), [](const EfPair &a, const EfPair &b) {
        const int ca = ef_class_of(a.lq), cb = ef_class_of(b.lq);
        return ca != cb ? ca < cb : a.ld > b.ld;
    });
    std::vector<EfPkGroup> groups;
    for (size_t k = 0; k < packed.size();) {
        const int cls = ef_class_of(packed[k].lq);
        size_t end = k + 1;
        while (end < packed.size() && ef_class_of(packed[end].lq) == cls &&
               packed_bucket(packed[end].ld) == packed_bucket(packed[k].ld))
            ++end;
        EfLaunch g{cls, (uint32_t)groups.size(), 0, packed[k].ld};
        for (; k < end; k += 2) {
            const bool two = k + 1 < end;
            const bool swap = two && packed[k + 1].out < packed[k].out;
            const EfPair &a = packed[swap ? k + 1 : k];
            EfPkGroup pg{};
            pg.qa_off = a.q_off, pg.da_off = a.d_off, pg.n_a = a.lq, pg.m_a = a.ld, pg.out_a = a.out;
            pg.out_b = kEfPkNone;
            if (two) {
                const EfPair &b = packed[swap ? k : k + 1];
                pg.qb_off = b.q_off, pg.db_off = b.d_off, pg.n_b = b.lq, pg.m_b = b.ld, pg.out_b = b.out;
            }
            groups.push_back(pg);
            ++g.count;
        }
        k = end;
        p->pk.push_back(g);
    }

    HIP_TRY(hipSetDevice(ctx->device));
    const auto upload = [](DevBuf &b, const void *src, size_t bytes) {
        if (!bytes) return hipSuccess;
        const hipError_t e = b.alloc(bytes);
        return e != hipSuccess ? e : hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    };
    HIP_TRY(upload(p->d_groups, groups.data(), groups.size() * sizeof(EfPkGroup)));
    HIP_TRY(upload(p->d_pairs, plain.data(), plain.size() * sizeof(EfPair)));
    HIP_TRY(upload(p->d_out, out_idx.data(), out_idx.size() * sizeof(uint32_t)));
    HIP_TRY(upload(p->d_sub, block.data(), block.size()));
    if (!plain.empty()) HIP_TRY(p->d_res.alloc(plain.size() * sizeof(saln_ends_free_result)));
    *out = p.release();
    return SALN_OK;
}

int score_execute(saln_ends_free_score_plan *p, const uint8_t *d_q, const uint8_t *d_db, int32_t *d_scores,
                  hipStream_t s) {
    const uint8_t *sub = p->d_sub.as<uint8_t>();
    for (const EfLaunch &l : p->pk)
        HIP_TRY(launch_ef_score_pk(l.cls, p->mode, p->d_groups.as<EfPkGroup>(), l.first, l.count, l.ld_max, d_q,
                                   d_db, p->sc, sub, d_scores, s));
    for (const EfLaunch &l : p->i32)
        HIP_TRY(launch_ef_fill(l.cls, p->mode, p->d_pairs.as<EfPair>(), l.first, l.count, l.ld_max, d_q, d_db,
                               p->sc, sub, nullptr, nullptr, p->d_res.as<saln_ends_free_result>(), s));
    HIP_TRY(launch_ef_score_gather(p->d_res.as<saln_ends_free_result>(), p->d_out.as<uint32_t>(),
                                   (uint32_t)p->n_i32, d_scores, s));
    return SALN_OK;
}

int score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                const uint32_t *pair_db, uint64_t n_pairs, int32_t mode, const EfScoreSrc &scoring,
                int32_t *scores) {
    if (!ctx || !q_off || !db_off) return SALN_E_INVALID;
    if (!scores) {
        set_error("ends_free: scores is NULL");
        return SALN_E_INVALID;
    }
    saln_ends_free_score_plan *raw = nullptr;
    const int rc = score_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode, scoring, &raw);
    if (rc != SALN_OK) return rc;
    std::unique_ptr<saln_ends_free_score_plan> p(raw);
    if (!n_pairs) return SALN_OK;
    hipStream_t s = ctx->stream;
    DevBuf dq(ctx, s), dd(ctx, s), d_scores(ctx, s);
    HIP_TRY(upload_seqs(dq, dd, q_seq, q_off, n_q, db_seq, db_off, n_db, 16));
    HIP_TRY(d_scores.alloc(n_pairs * sizeof(int32_t)));
    const int rx = score_execute(p.get(), dq.as<uint8_t>(), dd.as<uint8_t>(), d_scores.as<int32_t>(), s);
    if (rx != SALN_OK) return rx;
    HIP_TRY(hipMemcpyAsync(scores, d_scores.p, n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SALN_OK;
}

}  // namespace

extern "C" {

int saln_ends_free_score_path(uint64_t len_q, uint64_t len_db, int32_t mode, int32_t max_pos, int32_t max_abs,
                              int32_t *packed) {
    if (!packed || max_pos < 0 || max_abs < 0) return SALN_E_INVALID;
    int rc = ef_check_mode(mode);
    if (rc == SALN_OK) rc = ef_check_pair(len_q, len_db, 0);
    if (rc != SALN_OK) return rc;
    *packed = ef_score_packed(len_q, len_db, mode, (uint64_t)max_pos, (uint64_t)max_abs) ? 1 : 0;
    return SALN_OK;
}

int saln_ends_free_score_geometry(uint64_t len_q, uint64_t ld_max, int has_matrix, uint32_t *groups,
                                  uint32_t *lds_bytes) {
    if (!groups || !lds_bytes) return SALN_E_INVALID;
    const int rc = ef_check_pair(len_q, ld_max, 0);
    if (rc != SALN_OK) return rc;
    const EfFillGeometry g = ef_score_geometry(ef_class_of(len_q), (uint32_t)ld_max, has_matrix != 0);
    *groups = g.groups;
    *lds_bytes = (uint32_t)g.lds_bytes;
    return SALN_OK;
}

int saln_ends_free_score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                               const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                               const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                               const saln_nw_scoring *scoring, int32_t *scores) {
    return score_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                       EfScoreSrc::of(scoring), scores);
}

int saln_ends_free_sub_score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                                   const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                                   const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                                   int32_t mode, const saln_sub_matrix *matrix, int32_t *scores) {
    return score_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                       EfScoreSrc::of(matrix), scores);
}

int saln_ends_free_score_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                     const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                     const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                     const saln_nw_scoring *scoring, saln_ends_free_score_plan **out) {
    return score_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                             EfScoreSrc::of(scoring), out);
}

int saln_ends_free_sub_score_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                         const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                         const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                         const saln_sub_matrix *matrix, saln_ends_free_score_plan **out) {
    return score_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                             EfScoreSrc::of(matrix), out);
}

int saln_ends_free_score_execute(saln_ends_free_score_plan *p, const uint8_t *d_q_seq, const uint8_t *d_db_seq,
                                 int32_t *d_scores, void *stream) {
    if (!p || !d_scores || !d_q_seq || !d_db_seq) return SALN_E_INVALID;
    if (!p->n) return SALN_OK;
    hipStream_t s = resolve_stream(stream, p->ctx);
    HIP_TRY(hipSetDevice(p->ctx->device));
    return score_execute(p, d_q_seq, d_db_seq, d_scores, s);
}

int saln_ends_free_score_plan_info(const saln_ends_free_score_plan *p, uint64_t *packed_pairs,
                                   uint64_t *i32_pairs) {
    if (!p) return SALN_E_INVALID;
    if (packed_pairs) *packed_pairs = p->n_packed;
    if (i32_pairs) *i32_pairs = p->n_i32;
    return SALN_OK;
}

int saln_ends_free_score_plan_destroy(saln_ends_free_score_plan *p) {
    delete p;
    return SALN_OK;
}

}  // extern "C"
