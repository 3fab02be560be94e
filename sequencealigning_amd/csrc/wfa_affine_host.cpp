// C ABI of the corrected gap-affine WFA engine (include/saln.h,
// saln_wfa_affine_*): SURVEY.md §8(f) row 4.  Not a reference-parity path —
// the reference's wfa_align (src/wfa.rs:23-42, engine wfa_host.cpp) has no
// defined output for realistic inputs; this engine returns the minimum
// gap-affine penalty with the reference's penalties (wfa.rs:14-21) by
// default, checked against the Gotoh DP (oracle/refaffine.c).
//
// Two passes: every pair first runs with a W-diagonal wavefront ring; pairs
// whose wavefront outgrows it (score -2) are compacted on the device and run
// again with the second pass's ring (2x wider by default; plan_passes decides
// both widths and keeps each pass within the 64 KB of LDS of a workgroup).
// Score -1: the penalty exceeds max_score.
//
// Alignment mode (saln_wfa_affine_align_batch): the score passes, the scores
// read back, then per chunk of at most trace_budget_bytes of trace workspace
// the trace fill (both ring widths) and the walk of
// wfa_affine_trace_kernels.hip; the handle owns the packed CIGAR words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "wfa_affine.hpp"

using namespace saln;

struct saln_wfa_affine_plan {
    saln_context *ctx = nullptr;
    WfaAffParams prm{};
    bool wide = false;  // i32 offsets (a sequence longer than 32,000 bases)
    uint64_t n = 0;
    std::vector<WfaAffPair> pairs;  // host copy of d_pairs (alignment mode reads the lengths)
    DevBuf d_pairs, d_rerun;
    DevBuf d_count;  // [rerun pairs, pass-1 next pair, pass-2 next pair]
    WfaAffParams p1{}, p2{};  // the two passes (ring width, LDS sequence staging)
    uint32_t grid1 = 0, grid2 = 0;
};

namespace {

// ring widths (diagonals) of the two passes, i16 / i32 offsets: with the
// default penalties the second pass's ring is the 64 KB LDS limit of a
// workgroup; a wavefront wider than it leaves score -2.  plan_passes narrows
// a pass whose penalties need more ring slots than fit at these widths.
constexpr int32_t kW1 = 1024, kW2 = 2048, kW1Wide = 512, kW2Wide = 1024;
constexpr uint64_t kLdsLimit = 64u << 10;  // dynamic LDS of one workgroup
constexpr uint64_t kI16MaxLen = 32000;     // longest sequence of a plan with i16 offsets
constexpr uint64_t kMaxLen = 0x3FFFFFFFull;  // longest sequence the engine takes

int make_params(const saln_wfa_penalties *pen, int32_t max_score, WfaAffParams *out) {
    const int32_t x = pen ? pen->mismatch : 4, o = pen ? pen->gap_open : 2,
                  e = pen ? pen->gap_extend : 6;
    if (x <= 0 || e <= 0 || o < 0 || x > 4096 || o > 4096 || e > 4096) return SALN_E_INVALID;
    const int32_t g = std::gcd(std::gcd(x, o + e), e);
    WfaAffParams p{};
    p.x = x, p.o = o, p.e = e, p.g = g;
    p.RM = std::max(x, o + e) / g + 1;
    p.RI = e / g + 1;
    if (p.RM > 16 || p.RI > 16) {
        set_error("wfa_affine: penalties need more than 16 wavefront ring slots");
        return SALN_E_INVALID;
    }
    p.max_score = max_score > 0 ? max_score : INT32_MAX / 2;
    *out = p;
    return SALN_OK;
}

// Workgroups (waves) of a persistent launch per CU: as many as 160 KB of LDS
// hold, at most 16.  grid_for and the geometry query both use it.
uint32_t workgroups_per_cu(const WfaAffParams &prm, bool wide) {
    const size_t lds = wfa_affine_lds_bytes(prm, wide);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(16, (160u << 10) / lds));
}

uint32_t grid_for(const WfaAffParams &prm, bool wide, uint64_t n, int device) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    const uint64_t per_cu = workgroups_per_cu(prm, wide);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, per_cu * (uint64_t)cus));
}

// What a plan's passes depend on besides the penalties, folded over the
// batch's pairs (build_pairs and saln_wfa_affine_plan_geometry): the longest
// sequence (i32 offsets above kI16MaxLen bases) and the worst-case staging needs.
struct BatchShape {
    uint64_t maxlen = 0, seq_need = 0, code_need = 0;
    bool wide() const { return maxlen > kI16MaxLen; }
    // false: a sequence longer than the engine takes
    bool add(uint64_t lq, uint64_t ld) {
        if (lq > kMaxLen || ld > kMaxLen) return false;
        maxlen = std::max({maxlen, lq, ld});
        // LDS bytes to stage both sequences (wfa_affine_kernel's layout)
        seq_need = std::max<uint64_t>(seq_need, ((lq + 47) & ~15ull) + ld + 48);
        // ... or as 2-bit codes (16 per word, the 16-byte-aligned base's
        // words plus two pad words per sequence)
        // (at any alignment of the caller's buffers)
        code_need = std::max<uint64_t>(code_need, 4 * ((15 + lq + 15) / 16 + 2 + (15 + ld + 15) / 16 + 2));
        return true;
    }
};

// The two passes of a plan (ring width, LDS sequence staging): pure host
// logic, shared by saln_wfa_affine_plan_create and
// saln_wfa_affine_plan_geometry.  Each pass stages the pair's sequences in
// LDS when they fit next to its rings within wfa2.seq_lds / the 64 KB
// workgroup limit (else reads HBM).  The kernels index a ring with
// k & (W - 1) and run 512, 1024 or 2048 diagonals, so any other requested
// width is refused; a pass whose rings do not fit the workgroup limit at the
// requested width takes the widest of those that does.
int plan_passes(const WfaAffParams &prm, bool wide, uint64_t seq_need, uint64_t code_need,
                const Options &opts, WfaAffParams *p1, WfaAffParams *p2) {
    // tuning options (saln_option_set): staged-sequence LDS, ring widths (0 auto)
    const uint64_t seq_lds = (uint64_t)opts[Opt::Wfa2SeqLds];
    const int64_t w[2] = {opts[Opt::Wfa2W1], opts[Opt::Wfa2W2]};
    WfaAffParams *out[2] = {p1, p2};
    for (int i = 0; i < 2; ++i) {
        if (w[i] != 0 && w[i] != 512 && w[i] != 1024 && w[i] != 2048) {
            set_error(std::string("wfa_affine: option wfa2.w") + (i ? "2" : "1") + " = " +
                      std::to_string(w[i]) + " is not a ring width the kernels run (0, 512, 1024, 2048)");
            return SALN_E_INVALID;
        }
        WfaAffParams q = prm;
        q.seqcap = 0;
        q.W = w[i] ? (int32_t)w[i] : wide ? (i ? kW2Wide : kW1Wide) : (i ? kW2 : kW1);
        while (q.W > 512 && wfa_affine_lds_bytes(q, wide) > kLdsLimit) q.W >>= 1;
        const uint64_t rings = wfa_affine_lds_bytes(q, wide);
        if (rings > kLdsLimit) {
            set_error("wfa_affine: the wavefront rings of penalties (" + std::to_string(prm.x) + ", " +
                      std::to_string(prm.o) + ", " + std::to_string(prm.e) + ") with " +
                      (wide ? "i32" : "i16") + " offsets need " + std::to_string(rings) +
                      " bytes of LDS at 512 diagonals, above the 65,536 of a workgroup");
            return SALN_E_INVALID;
        }
        const uint64_t cap = std::min<uint64_t>(seq_lds, kLdsLimit - rings);
        // 2-bit codes when they fit (a pair holding other bytes then reads
        // HBM), bytes too when they take little more: the kernel tries codes
        // first, then bytes, within seqcap
        uint64_t want = code_need <= cap ? code_need : 0;
        if (seq_need <= cap && seq_need <= std::max<uint64_t>(want, 8u << 10)) want = std::max(want, seq_need);
        // (rings is a multiple of 16, so the rounding stays within the limit)
        q.seqcap = (int32_t)std::min<uint64_t>((want + 15) & ~15ull, kLdsLimit - rings);
        *out[i] = q;
    }
    return SALN_OK;
}

int build_pairs(const uint64_t *q_off, uint64_t n_q, const uint64_t *db_off, uint64_t n_db,
                const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                std::vector<WfaAffPair> *out, BatchShape *shape) {
    out->resize(n_pairs);
    const PairIndex pairs{pair_q, pair_db, n_q, n_db};
    for (uint64_t k = 0; k < n_pairs; ++k) {
        uint64_t qi, di, lq, ld;
        if (!pairs.at(k, &qi, &di) || !pair_lengths(q_off, db_off, qi, di, kMaxLen, &lq, &ld) ||
            !shape->add(lq, ld))
            return SALN_E_INVALID;
        WfaAffPair p{};
        p.q_off = q_off[qi];
        p.d_off = db_off[di];
        p.lq = (uint32_t)lq;
        p.ld = (uint32_t)ld;
        p.out = (uint32_t)k;
        (*out)[k] = p;
    }
    return SALN_OK;
}

// The trace workspace of one pair (include/saln.h,
// saln_wfa_affine_trace_bytes; the kernels' layout is in the header comment
// of wfa_affine_trace_kernels.hip): T steps, wavefronts of at most `width`
// diagonals, code rows of wt diagonals.
struct TraceLayout {
    uint64_t T = 0, width = 0, wt = 64, bytes = 0;
};

TraceLayout trace_layout(const WfaAffParams &prm, uint64_t lq, uint64_t ld, int32_t score) {
    TraceLayout l;
    if (lq == 0 || ld == 0) return l;  // one gap run: no codes
    l.T = (uint64_t)(score / prm.g);
    // a gap of n columns costs o + n e, so |k| <= (score - o) / e
    const uint64_t reach = score > prm.o ? (uint64_t)((score - prm.o) / prm.e) : 0;
    l.width = std::min<uint64_t>(2 * reach + 1, lq + ld + 1);
    while (l.wt < l.width + 2) l.wt <<= 1;
    l.bytes = l.T * (l.wt / 2) + ((l.T + 15) & ~15ull);
    return l;
}

}  // namespace

// The result handle of saln_wfa_affine_align_batch: pair k's words are
// words[off[k] .. off[k] + res[k].cigar_len).
struct saln_wfa_affine_aln {
    std::vector<saln_wfa_affine_result> res;
    std::vector<uint64_t> off;
    std::vector<uint32_t> words;
};

extern "C" {

int saln_wfa_affine_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                const uint32_t *pair_db, uint64_t n_pairs,
                                const saln_wfa_penalties *pen, int32_t max_score,
                                saln_wfa_affine_plan **out) {
    if (!ctx || !q_off || !db_off || !out || n_pairs > 0xFFFFFFFFull) return SALN_E_INVALID;
    if (!PairIndex{pair_q, pair_db, n_q, n_db}.complete(n_pairs)) return SALN_E_INVALID;
    auto p = std::make_unique<saln_wfa_affine_plan>();
    p->ctx = ctx;
    int rc = make_params(pen, max_score, &p->prm);
    BatchShape shape;
    if (rc == SALN_OK)
        rc = build_pairs(q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, &p->pairs, &shape);
    p->wide = shape.wide();
    // the passes before anything touches the device: a refused ring width or
    // penalty set never reaches an allocation or a launch
    if (rc == SALN_OK)
        rc = plan_passes(p->prm, p->wide, shape.seq_need, shape.code_need,
                         ctx->opts.effective(), &p->p1, &p->p2);
    if (rc != SALN_OK) return rc;
    p->n = n_pairs;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n_pairs) {
        HIP_TRY(p->d_pairs.alloc(n_pairs * sizeof(WfaAffPair)));
        HIP_TRY(p->d_rerun.alloc(n_pairs * sizeof(WfaAffPair)));
        HIP_TRY(p->d_count.alloc(3 * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(p->d_pairs.p, p->pairs.data(), n_pairs * sizeof(WfaAffPair),
                          hipMemcpyHostToDevice));
    }
    p->grid1 = grid_for(p->p1, p->wide, n_pairs, ctx->device);
    p->grid2 = grid_for(p->p2, p->wide, n_pairs, ctx->device);
    *out = p.release();
    return SALN_OK;
}

int saln_wfa_affine_execute(saln_wfa_affine_plan *p, const uint8_t *d_q_seq,
                            const uint8_t *d_db_seq, int32_t *d_scores, void *stream) {
    if (!p || !d_scores || !d_q_seq || !d_db_seq) return SALN_E_INVALID;
    if (!p->n) return SALN_OK;
    hipStream_t s = resolve_stream(stream, p->ctx);
    HIP_TRY(hipSetDevice(p->ctx->device));
    WfaAffPair *pairs = p->d_pairs.as<WfaAffPair>(), *rerun = p->d_rerun.as<WfaAffPair>();
    uint32_t *count = p->d_count.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(count, 0, 3 * sizeof(uint32_t), s));
    HIP_TRY(launch_wfa_affine(pairs, (uint32_t)p->n, d_q_seq, d_db_seq, p->p1, p->wide, p->grid1,
                              nullptr, count + 1, d_scores, s));
    HIP_TRY(launch_wfa_affine_compact(pairs, (uint32_t)p->n, d_scores, rerun, count, s));
    // pass 2 reads its pair count from the device (no host round trip)
    HIP_TRY(launch_wfa_affine(rerun, (uint32_t)p->n, d_q_seq, d_db_seq, p->p2, p->wide, p->grid2,
                              count, count + 2, d_scores, s));
    return SALN_OK;
}

int saln_wfa_affine_plan_destroy(saln_wfa_affine_plan *p) {
    delete p;
    return SALN_OK;
}

// The score passes of a host batch: the plan, both sequence sets on the
// device with 16 bytes of padding (in dq / dd, whose allocator the scores'
// block shares) and every pair's score on the host.  A sequence longer than
// len_limit is refused before anything runs.
static int score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                       uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                       const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                       const saln_wfa_penalties *pen, int32_t max_score, uint32_t len_limit,
                       DevBuf &dq, DevBuf &dd, std::unique_ptr<saln_wfa_affine_plan> *plan,
                       int32_t *scores) {
    saln_wfa_affine_plan *p = nullptr;
    int rc = saln_wfa_affine_plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs,
                                         pen, max_score, &p);
    if (rc != SALN_OK) return rc;
    plan->reset(p);
    for (const WfaAffPair &k : p->pairs)
        if (k.lq > len_limit || k.ld > len_limit) return SALN_E_INVALID;
    DevBuf dsc = dq.sibling();
    HIP_TRY(upload_seqs(dq, dd, q_seq, q_off, n_q, db_seq, db_off, n_db, 16));
    HIP_TRY(dsc.alloc(std::max<size_t>(n_pairs * sizeof(int32_t), 16)));
    rc = saln_wfa_affine_execute(p, dq.as<uint8_t>(), dd.as<uint8_t>(), dsc.as<int32_t>(), nullptr);
    if (rc != SALN_OK) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(scores, dsc.p, n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SALN_OK;
}

int saln_wfa_affine_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                          uint64_t n_pairs, const saln_wfa_penalties *pen, int32_t max_score,
                          int32_t *scores) {
    if (!ctx || !q_off || !db_off || !scores) return SALN_E_INVALID;
    if (n_pairs == 0) return SALN_OK;
    std::unique_ptr<saln_wfa_affine_plan> plan;
    DevBuf dq, dd;
    return score_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs, pen,
                       max_score, (uint32_t)kMaxLen, dq, dd, &plan, scores);
}

int saln_wfa_affine_trace_bytes(const saln_wfa_penalties *pen, uint64_t len_q, uint64_t len_db,
                                int32_t score, uint64_t *bytes) {
    if (!bytes || score < 0) return SALN_E_INVALID;
    WfaAffParams prm{};
    const int rc = make_params(pen, 0, &prm);
    if (rc != SALN_OK) return rc;
    *bytes = trace_layout(prm, len_q, len_db, score).bytes;
    return SALN_OK;
}

int saln_wfa_affine_plan_geometry(const saln_wfa_penalties *pen, const uint64_t *len_q,
                                  const uint64_t *len_db, uint64_t n_pairs,
                                  saln_wfa_affine_pass_geometry *out) {
    if (!out || (n_pairs && (!len_q || !len_db))) return SALN_E_INVALID;
    WfaAffParams prm{}, pass[2];
    int rc = make_params(pen, 0, &prm);
    if (rc != SALN_OK) return rc;
    BatchShape shape;
    for (uint64_t k = 0; k < n_pairs; ++k)
        if (!shape.add(len_q[k], len_db[k])) return SALN_E_INVALID;
    const bool wide = shape.wide();
    rc = plan_passes(prm, wide, shape.seq_need, shape.code_need, opt_registry(), &pass[0], &pass[1]);
    if (rc != SALN_OK) return rc;
    for (int i = 0; i < 2; ++i) {
        out[i].ring_width = pass[i].W;
        out[i].seqcap = pass[i].seqcap;
        out[i].lds_bytes = (uint32_t)wfa_affine_lds_bytes(pass[i], wide);
        out[i].i32_offsets = wide ? 1 : 0;
        out[i].workgroups_per_cu = workgroups_per_cu(pass[i], wide);
    }
    return SALN_OK;
}

int saln_wfa_affine_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                uint64_t n_pairs, const saln_wfa_penalties *pen,
                                int32_t max_score, uint64_t trace_budget_bytes,
                                saln_wfa_affine_aln **out) {
    if (!ctx || !q_off || !db_off || !out) return SALN_E_INVALID;
    auto aln = std::make_unique<saln_wfa_affine_aln>();
    if (n_pairs == 0) {
        aln->off.assign(1, 0);
        *out = aln.release();
        return SALN_OK;
    }
    // the score passes (saln_wfa_affine_batch's), sequences kept on the device
    // in blocks of the context's cache; a CIGAR run holds 2^28-1 columns
    std::unique_ptr<saln_wfa_affine_plan> plan;
    hipStream_t s = ctx->stream;  // every launch below runs on it: the blocks sync it alone
    DevBuf dq(ctx, s), dd(ctx, s);
    std::vector<int32_t> scores(n_pairs);
    int rc = score_batch(ctx, q_seq, q_off, n_q, db_seq, db_off, n_db, pair_q, pair_db, n_pairs,
                         pen, max_score, 0x0FFFFFFFu, dq, dd, &plan, scores.data());
    if (rc != SALN_OK) return rc;
    aln->res.assign(n_pairs, saln_wfa_affine_result{});
    aln->off.assign(n_pairs + 1, 0);
    const std::vector<WfaAffPair> &hp = plan->pairs;

    // chunks: pairs in pair order, at most `budget` bytes of trace workspace each
    const uint64_t budget = trace_budget_bytes ? trace_budget_bytes : (1ull << 30);
    const WfaAffParams &prm = plan->prm;
    struct Chunk {
        std::vector<WfaAffTracePair> tp;  // p.out: the pair's index in the batch
        uint64_t bytes = 0, words = 0;
    };
    std::vector<Chunk> chunks;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        saln_wfa_affine_result &r = aln->res[k];
        r.score = scores[k];
        r.status = SALN_OK;
        if (r.score < 0) continue;
        const bool empty = hp[k].lq == 0 || hp[k].ld == 0;
        const TraceLayout lay = trace_layout(prm, hp[k].lq, hp[k].ld, r.score);
        if (lay.bytes > budget) {
            r.status = SALN_TRACE_CAP;
            continue;
        }
        if (chunks.empty() || chunks.back().bytes + lay.bytes > budget ||
            chunks.back().tp.size() >= (1u << 30))
            chunks.emplace_back();
        Chunk &c = chunks.back();
        WfaAffTracePair tp{};
        tp.p = hp[k];
        tp.p.reserved = empty ? 0u : (uint32_t)lay.T;
        tp.code_off = c.bytes;
        tp.cig_off = c.words;
        tp.wt = (uint32_t)lay.wt;
        tp.cig_cap = 2 * tp.p.reserved + 1;
        c.bytes += lay.bytes;
        c.words += tp.cig_cap;
        c.tp.push_back(tp);
    }
    uint64_t max_bytes = 0, max_words = 0, max_n = 0;
    for (const Chunk &c : chunks) {
        max_bytes = std::max(max_bytes, c.bytes);
        max_words = std::max(max_words, c.words);
        max_n = std::max<uint64_t>(max_n, c.tp.size());
    }
    DevBuf d_tp(ctx, s), d_codes(ctx, s), d_words(ctx, s), d_status(ctx, s), d_len(ctx, s),
        d_next(ctx, s);
    if (!chunks.empty()) {
        const auto min16 = [](size_t n) { return std::max<size_t>(n, 16); };
        HIP_TRY(d_tp.alloc(min16(max_n * sizeof(WfaAffTracePair))));
        HIP_TRY(d_codes.alloc(min16(max_bytes)));
        HIP_TRY(d_words.alloc(min16(max_words * sizeof(uint32_t))));
        HIP_TRY(d_status.alloc(min16(max_n * sizeof(int32_t))));
        HIP_TRY(d_len.alloc(min16(max_n * sizeof(uint32_t))));
        HIP_TRY(d_next.alloc(min16(2 * sizeof(uint32_t))));
    }
    // Per chunk: the fill with the first ring over every pair, the fill with
    // the second ring over the pairs the first left (kTraceRerun in their
    // status), the walk, then status / lengths / CIGAR areas back.  Chunks
    // and their pairs are in pair order, so the handle's words are appended.
    std::vector<uint64_t> ids;
    std::vector<int32_t> h_status;
    std::vector<uint32_t> h_len, h_words;
    uint64_t next_pair = 0;  // pairs before it have their offset
    for (Chunk &c : chunks) {
        const uint32_t n = (uint32_t)c.tp.size();
        ids.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            ids[i] = c.tp[i].p.out;
            c.tp[i].p.out = i;
        }
        HIP_TRY(hipMemcpy(d_tp.p, c.tp.data(), n * sizeof(WfaAffTracePair), hipMemcpyHostToDevice));
        HIP_TRY(hipMemsetAsync(d_next.p, 0, 2 * sizeof(uint32_t), s));
        const auto *dp = d_tp.as<const WfaAffTracePair>();
        const uint8_t *sq = dq.as<uint8_t>(), *sd = dd.as<uint8_t>();
        uint8_t *codes = d_codes.as<uint8_t>();
        int32_t *status = d_status.as<int32_t>();
        HIP_TRY(launch_wfa_affine_trace(dp, n, sq, sd, plan->p1, plan->wide, /*rerun=*/false,
                                        grid_for(plan->p1, plan->wide, n, ctx->device),
                                        d_next.as<uint32_t>(), codes, status, s));
        HIP_TRY(launch_wfa_affine_trace(dp, n, sq, sd, plan->p2, plan->wide, /*rerun=*/true,
                                        grid_for(plan->p2, plan->wide, n, ctx->device),
                                        d_next.as<uint32_t>() + 1, codes, status, s));
        HIP_TRY(launch_wfa_affine_walk(dp, n, sq, sd, prm, codes, status, d_words.as<uint32_t>(),
                                       d_len.as<uint32_t>(), s));
        HIP_TRY(hipStreamSynchronize(s));
        h_status.resize(n);
        h_len.resize(n);
        h_words.resize(c.words);
        HIP_TRY(hipMemcpy(h_status.data(), status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_len.data(), d_len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_words.data(), d_words.p, c.words * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) {
            saln_wfa_affine_result &r = aln->res[ids[i]];
            r.status = h_status[i] == SALN_OK ? SALN_OK : SALN_INTERNAL;
            r.cigar_len = r.status == SALN_OK ? std::min(h_len[i], c.tp[i].cig_cap) : 0;
            for (; next_pair <= ids[i]; ++next_pair) aln->off[next_pair] = aln->words.size();
            aln->words.insert(aln->words.end(), h_words.begin() + c.tp[i].cig_off,
                              h_words.begin() + c.tp[i].cig_off + r.cigar_len);
        }
        std::vector<WfaAffTracePair>().swap(c.tp);
    }
    for (; next_pair <= n_pairs; ++next_pair) aln->off[next_pair] = aln->words.size();
    *out = aln.release();
    return SALN_OK;
}

uint64_t saln_wfa_affine_aln_count(const saln_wfa_affine_aln *a) { return a ? a->res.size() : 0; }

int saln_wfa_affine_aln_get(const saln_wfa_affine_aln *a, uint64_t pair,
                            saln_wfa_affine_result *res, const uint32_t **cigar) {
    if (!a || pair >= a->res.size()) return SALN_E_INVALID;
    if (res) *res = a->res[pair];
    if (cigar) *cigar = a->words.data() + a->off[pair];
    return SALN_OK;
}

void saln_wfa_affine_aln_free(saln_wfa_affine_aln *a) { delete a; }

}  // extern "C"
