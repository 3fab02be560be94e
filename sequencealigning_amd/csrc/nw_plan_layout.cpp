// NW plan layout (nw_plan_layout.hpp).
#include "nw_plan_layout.hpp"

#include <algorithm>
#include <numeric>

namespace saln {

Scoring scoring_or_default(const saln_nw_scoring *s) {
    if (!s) return Scoring{5, -4, -8, -6};  // SCHEME, needleman_wunsch_affine.rs:15-20
    return Scoring{s->match, s->mismatch, s->gap_open, s->gap_extend};
}

// The i32 fills carry V'' = 4V + 2a + p plus the position offsets alpha*r +
// beta*c (nw_common.hpp).  |V| is at most the sentinel plus one step's
// largest change per row and column of the path; a pair passes while that
// bound, scaled and offset, stays inside int32 (the reference's own i32
// arithmetic is exact far beyond it: the pairs rejected here are ~10^8 long
// or carry penalties of ~10^4).
bool scores_fit_i32(const Scoring &s, uint64_t lq, uint64_t ld) {
    auto a = [](int64_t v) { return v < 0 ? -v : v; };
    const int64_t step = std::max({a(s.match), a(s.mismatch), a(s.gap_open) + a(s.gap_extend)});
    const long double v = 32768.0L + (long double)(lq + ld) * (long double)step;
    const long double off = 4.0L * (a(s.match) + 2 * a(s.gap_extend)) * (long double)ld +
                            4.0L * a(s.gap_extend) * (long double)lq;
    return 4.0L * v + 3.0L + off < 2147483647.0L;
}

namespace {

// Every pair's descriptor in results order: lengths, variant, CIGAR offset.
int describe_pairs(const uint64_t *q_off, const uint64_t *db_off, const PairIndex &pairs,
                   uint64_t n_pairs, const Scoring &sc, bool narrow, NwPlanLayout *L,
                   std::vector<NwPairDesc> *descs) {
    L->cigar_off.resize(n_pairs + 1);
    descs->assign(n_pairs, NwPairDesc{});  // every field 0 until set
    uint64_t cig = 0;
    // the range check and the variant depend on the shape only: batches of
    // alike pairs (the usual case) decide once per shape, not per pair
    uint64_t memo_lq = ~0ull, memo_ld = ~0ull;
    bool memo_fit = false;
    int memo_var = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        uint64_t qi, di, lq, ld;
        if (!pairs.at(k, &qi, &di) ||
            !pair_lengths(q_off, db_off, qi, di, 0x7FFFFFFFull, &lq, &ld))
            return SALN_E_INVALID;
        NwPairDesc &d = (*descs)[k];
        d.q_off = q_off[qi];
        d.db_off = db_off[di];
        if (lq != memo_lq || ld != memo_ld) {
            memo_lq = lq;
            memo_ld = ld;
            memo_fit = scores_fit_i32(sc, lq, ld);
            memo_var = memo_fit ? choose_variant((uint32_t)lq, (uint32_t)ld, sc, narrow) : 0;
        }
        if (!memo_fit) {
            set_error("pair too long for these penalties: its scores could leave the engine's "
                      "int32 range");
            return SALN_E_INVALID;
        }
        d.len_q = (uint32_t)lq;
        d.len_db = (uint32_t)ld;
        d.pair_id = (uint32_t)k;
        d.variant = (uint32_t)memo_var;
        d.cigar_off = cig;
        L->cigar_off[k] = cig;
        cig += lq + ld;
        L->cells += lq * ld;
    }
    L->cigar_off[n_pairs] = cig;
    return SALN_OK;
}

// Plan order: fill pairs grouped by variant, then by query chunk count,
// longest db first (balances the groups of a block and keeps the pairs of
// a mask pack alike); pairs with an empty side last (traceback only).
// (variant, ~chunks, ~len_db) packed in one word, ties by results index;
// a batch of alike pairs is usually in order already.  The same pass counts
// each variant's pairs; as plan order groups the variants in ascending order,
// their first pairs follow from the counts.
void order_pairs(std::vector<NwPairDesc> &&descs, NwPlanLayout *L) {
    const uint64_t n_pairs = descs.size();
    std::vector<uint64_t> skey(n_pairs);
    for (uint64_t k = 0; k < n_pairs; ++k) {
        const NwPairDesc &d = descs[k];
        const bool empty = d.len_q == 0 || d.len_db == 0;
        const uint64_t nch = empty ? 0 : variant_geom((int)d.variant).n_chunks(d.len_q);
        skey[k] = (uint64_t)(empty ? (uint32_t)kNumVariants : d.variant) << 56 |
                  ((~nch) & 0xFFFFFFull) << 32 | (uint32_t)~d.len_db;
        if (empty) continue;
        L->var_count[d.variant]++;
        L->var_maxld[d.variant] = std::max(L->var_maxld[d.variant], d.len_db);
    }
    for (int v = 0; v < kNumVariants; ++v) {
        if (L->var_count[v]) L->var_first[v] = L->n_fill;
        L->n_fill += L->var_count[v];
    }
    if (std::is_sorted(skey.begin(), skey.end())) {
        L->h_pairs = std::move(descs);  // plan order = results order: no copy
    } else {
        std::vector<uint32_t> order(n_pairs);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return skey[a] != skey[b] ? skey[a] < skey[b] : a < b;
        });
        L->h_pairs.resize(n_pairs);
        for (uint64_t r = 0; r < n_pairs; ++r) L->h_pairs[r] = descs[order[r]];
    }
}

// The column stripes' fill, decided once per plan (it sets their layout).
void choose_stripe_layout(const Scoring &sc, const Options &opts, NwPlanLayout *L) {
    uint64_t waves = 0, cols = 0, waves_k1 = 0;  // 256-column chunks, columns, 64-column stripes
    bool free_all = true;  // the packed stripes carry no alive flag (nw_common.hpp)
    const uint32_t nv = L->var_count[kStripeVariant];
    for (uint32_t r = 0; r < nv; ++r) {
        const NwPairDesc &d = L->h_pairs[L->var_first[kStripeVariant] + r];
        waves += variant_geom(kStripeVariant).n_chunks(d.len_q);
        waves_k1 += (d.len_q + 63) / 64;
        cols += d.len_q;
        free_all = free_all && sentinel_free(sc, d.len_q, d.len_db);
    }
    // packed stripes (int16x2, throughput) for batches of wide pairs; the
    // row fill (i32, latency) otherwise: 400 x 2 kbp^2 828 vs 678 GCUPS,
    // 400 x 5 kbp^2 953 vs 1,204 (one box, round 2)
    const bool wide = nv && cols / nv >= 3000;
    L->stripe_pk = waves > 0 && free_all && stripe_packed(sc, waves, wide, opts);
    L->stripe_rows = L->stripe_pk ? 0 : stripe_rows_k(waves_k1, opts);
    // boundary columns per 256-column chunk: the row fill's 4 / K stripes
    // (at most 4), else one
    L->stripe_sub = L->stripe_rows ? 4u / (uint32_t)L->stripe_rows : 1u;
}

// One pass in plan order: plan_index, the op-stream and boundary-column
// offsets of the filled pairs, the stripe work list and the progress indices.
void lay_out_scratch_and_work(NwPlanLayout *L) {
    const uint64_t n_pairs = L->h_pairs.size();
    uint64_t soff = 0, ooff = 0;
    L->plan_index.resize(n_pairs);
    L->work_first.assign(n_pairs + 1, 0);
    for (uint64_t r = 0; r < n_pairs; ++r) {
        NwPairDesc &d = L->h_pairs[r];
        L->plan_index[d.pair_id] = (uint32_t)r;
        // stripe work list: pair-major, chunk-ascending (a stripe's predecessor
        // always has a lower workgroup id)
        L->work_first[r] = (uint32_t)L->work.size();
        if (d.len_q == 0 || d.len_db == 0) continue;
        const bool stripe = d.variant == (uint32_t)kStripeVariant;
        const uint32_t nch = variant_geom((int)d.variant).n_chunks(d.len_q);
        d.ops_off = ooff;
        ooff += (d.len_q + d.len_db + 9) / 10 + 1;  // 3-bit ops, ten per word
        if (nch > 1 || stripe) {
            soff = (soff + 3) & ~3ull;  // 32-byte aligned columns (nw_fill_rows_kernel)
            d.scratch_off = soff;
            // stripes run concurrently: stripe_sub boundary columns per chunk boundary
            soff += (uint64_t)(stripe ? L->stripe_sub * nch : 1) * scratch_col(d.len_db);
        }
        if (!stripe) continue;
        d.reserved = (uint32_t)L->n_prog;
        L->n_prog += nch;
        for (uint32_t ch = 0; ch < nch; ++ch) L->work.push_back(Word2{(uint32_t)r, ch});
    }
    L->work_first[n_pairs] = (uint32_t)L->work.size();
    L->scratch_elems = soff;
    L->ops_words = ooff;
}

// Mask packs: up to 64 consecutive pairs of a variant (one traceback
// wave) with interleaved segments (nw_common.hpp Geom), unless padding
// them to the pack's longest db / widest query would cost over 25 % more
// than storing them apart.
void lay_out_masks(NwPlanLayout *L) {
    uint64_t moff = 0;
    for (int v = 0; v < kNumVariants; ++v) {
        const Geom g = variant_geom(v);
        const uint64_t lb = L->nib[v] ? g.LBn() : g.LB();
        for (uint32_t a = L->var_first[v], e = a + L->var_count[v]; a < e; a += 64) {
            const uint32_t np = std::min<uint32_t>(64, e - a);
            uint64_t rows = 0, nbm = 0, own = 0;
            for (uint32_t s = 0; s < np; ++s) {
                const NwPairDesc &d = L->h_pairs[a + s];
                rows = std::max<uint64_t>(rows, d.len_db);
                nbm = std::max<uint64_t>(nbm, g.n_blocks(d.len_q));
                own += (uint64_t)d.len_db * g.n_blocks(d.len_q) * lb;
            }
            const uint64_t packed = rows * nbm * np * lb;
            if (v == kStripeVariant) {
                // one region per 256-column chunk: the row fill's unskewed
                // 256-column tiles (bs = 4), or the packed stripes' skewed
                // lines (bs = 0: every fill step writes one whole line)
                const bool pk = L->stripe_pk;
                for (uint32_t s = 0; s < np; ++s) {
                    NwPairDesc &d = L->h_pairs[a + s];
                    d.mask_off = moff;
                    d.mask_rs = g.W();
                    d.mask_bs = pk ? 0u : (uint32_t)lb;
                    d.mask_cs = ((uint64_t)d.len_db + (pk ? 2 * g.G : g.G) - 1) * g.W();
                    moff += g.n_chunks(d.len_q) * d.mask_cs;
                }
            } else if (4 * packed <= 5 * own + 4096) {
                for (uint32_t s = 0; s < np; ++s) {
                    NwPairDesc &d = L->h_pairs[a + s];
                    d.mask_off = moff + s * lb;
                    d.mask_bs = (uint32_t)(np * lb);
                    d.mask_rs = nbm * np * lb;
                    d.mask_cs = (uint64_t)g.G * d.mask_bs;
                }
                moff += (packed + 255) & ~255ull;
            } else {
                for (uint32_t s = 0; s < np; ++s) {
                    NwPairDesc &d = L->h_pairs[a + s];
                    d.mask_off = moff;
                    d.mask_bs = (uint32_t)lb;
                    d.mask_rs = g.n_blocks(d.len_q) * lb;
                    d.mask_cs = (uint64_t)g.G * lb;
                    moff += ((uint64_t)d.len_db * d.mask_rs + 255) & ~255ull;
                }
            }
        }
    }
    L->mask_bytes = moff;
}

// Speculative stripe walks: a few long column-stripe pairs walk all
// their 256-column stripes at once (nw_traceback_coop_kernel kSpec)
// instead of one stripe after another (C4: walk 3.8 ms).  Off with
// option nw.spec = 0; nw.spec_passes walk passes (default 3).
void lay_out_spec(const Options &opts, NwPlanLayout *L) {
    const int passes = (int)opts[Opt::SpecPasses];
    const uint32_t first = L->var_first[kStripeVariant], nv = L->var_count[kStripeVariant];
    if (opts[Opt::Spec] == 0 || passes <= 0 || !nv || nv > kSpecMaxPairs) return;
    for (uint32_t r = first; r < first + nv; ++r) {
        const uint32_t S = (L->h_pairs[r].len_q + 255) / 256;
        if (S < kSpecMinStripes || S > kSpecMaxStripes) continue;
        L->spec_pair_tab.push_back(SpecPair{r, S, (uint32_t)L->spec_block_tab.size(), 0});
        for (uint32_t s = 0; s < S; ++s)
            L->spec_block_tab.push_back(Word2{(uint32_t)L->spec_pair_tab.size() - 1, s});
    }
    if (L->spec_pair_tab.empty()) return;
    L->spec_passes = passes;
    L->spec_strict = opts[Opt::SpecStrict] != 0;
}

}  // namespace

int nw_plan_layout(const uint64_t *q_off, const uint64_t *db_off, const PairIndex &pairs,
                   uint64_t n_pairs, int32_t mode, const Scoring &sc, const Options &opts,
                   bool full_codes, NwPlanLayout *out) {
    if (mode != SALN_MODE_GLOBAL) {
        set_error("not implemented");  // needleman_wunsch_affine.rs:433-434
        return SALN_NOT_IMPLEMENTED;
    }
    if (!pairs.complete(n_pairs) || n_pairs > 0xFFFFFFFFull) return SALN_E_INVALID;
    NwPlanLayout L;
    // 4-bit walk codes for the short-query packed variants: 8 x 19 groups for
    // queries of <= 152 columns, 16 x 10 up to 160; full-code plans keep byte
    // codes and the 16 x 10 groups
    const bool nib_on = !full_codes;
    for (int v = 0; v < kNumVariants; ++v) L.nib[v] = nib_on && variant_nib(v);
    std::vector<NwPairDesc> descs;
    const int rc = describe_pairs(q_off, db_off, pairs, n_pairs, sc, nib_on, &L, &descs);
    if (rc != SALN_OK) return rc;
    demote_wide_pairs(descs.data(), descs.size(), opts);
    order_pairs(std::move(descs), &L);
    choose_stripe_layout(sc, opts, &L);
    lay_out_scratch_and_work(&L);
    lay_out_masks(&L);
    // table fills (4-bit codes; full codes in 16-lane groups): a bail word per variant
    L.bail = (L.var_count[kNarrowVariant] && L.nib[kNarrowVariant]) ||
             (L.var_count[kPacked16x10] && L.nib[kPacked16x10]) ||
             (full_codes && (L.var_count[kPacked16x16] || L.var_count[kPacked16x10]));
    lay_out_spec(opts, &L);
    *out = std::move(L);
    return SALN_OK;
}

}  // namespace saln
