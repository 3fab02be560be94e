// NW variant policy (nw_policy.hpp).
#include "nw_policy.hpp"

#include <cstdlib>

namespace saln {

// Packed i16 is exact while every value and every same-cell difference stays
// inside int16 with the position offsets of nw_fill_pk_kernel (see there):
// `rows` rows of growth a and lq columns of growth b from the frame's origin.
bool packed_range_ok(uint32_t lq, uint32_t rows, const Scoring &sc) {
    const int64_t pen = 2ll * (sc.match - sc.mismatch);
    // pen >= 2: the q==d bit comes from the penalty (0 or pen in each half)
    if (pen < 2 || pen > 32 || sc.gap_extend > 0 || sc.gap_open > 0) return false;
    const int64_t span = std::max<int64_t>(
        {std::abs(sc.match), std::abs(sc.mismatch), std::abs(sc.gap_open) + std::abs(sc.gap_extend)});
    const int64_t a = 2 * (std::abs(sc.match) + std::abs(sc.gap_extend)) + 2 * span;
    return (int64_t)rows * a + (int64_t)lq * (2 * std::abs(sc.gap_extend) + 2 * span) + 256 < 30000;
}
// One int16 frame holds a launch of G-lane groups of W columns whose longest
// db has `ld` rows: the values of all W columns (a launch decides its frame
// from the group's width, not from a pair's own query) and the 32-bit staged
// db rows (kPackedLdsMax; under small penalties the value range alone admits
// more rows than the LDS holds).  choose_variant and the launches share it, so
// a pair is never handed to a frame that no guard accepted for it.
bool packed_single_ok(uint32_t G, uint32_t W, uint32_t ld, const Scoring &sc) {
    return packed_range_ok(W, ld, sc) && staged_lds_bytes(G, ld, 4) <= kPackedLdsMax;
}
// The rebasing fill (kRebase).  At step t a lane's value is
// X~(r,c) - drift * r0 with r in [r0 - G, r0 + kRebaseSteps) and
//   X~(r,c) - drift*r0 = [X~(r,c) - X~(r,0)] + [X~(r,0) - drift*r] + drift*(r - r0):
// the first term lies in [2*go, c*(2|m| + 4|ge|)] (a row's H exceeds its
// column-0 value by at most c*(m - ge), the c columns' diagonal gain over the
// gap it replaces, and falls below it by at most a gap; beta*c on top), the
// second is the constant 2*(go + ge) + 1 while hs_col0 is linear (ld <= 4096
// and |go| + 4097*|ge| < 2^15: the sentinel floor is not reached), the third
// is at most |drift| * (period + G).  M / I / D sit within an open + extend +
// penalty of H.  The db length is also bounded by the staged rows
// (kPackedLdsMax).
static bool packed_ok_rebase(uint32_t lq, uint32_t ld, const Scoring &sc, uint32_t G, uint32_t W) {
    const int64_t pen = 2ll * (sc.match - sc.mismatch);
    if (pen < 2 || pen > 32 || sc.gap_extend > 0 || sc.gap_open > 0 || lq > W) return false;
    if (staged_lds_bytes(G, ld, 2) > kPackedLdsMax || ld > 4096) return false;  // 16-bit rows
    const int64_t m = std::abs(sc.match), ge = std::abs(sc.gap_extend), go = std::abs(sc.gap_open);
    if (go + 4097 * ge >= 32768) return false;
    const int64_t drift = std::abs(2 * sc.gap_extend - 2 * sc.match + 2 * sc.gap_extend);
    // column term [-(2go + 1), W*(2m + 4ge) + 2(go + ge)] centred by rebase_center
    const int64_t col = (int64_t)W * (2 * m + 4 * ge);
    const int64_t half = std::max<int64_t>(col - rebase_center(sc, (int32_t)W), rebase_center(sc, (int32_t)W));
    const int64_t bound = half + (kRebaseSteps + (int64_t)G) * drift + 4 * (go + ge) + 2 * pen + 512;
    return bound < 30000;
}

int choose_variant(uint32_t len_q, uint32_t len_db, const Scoring &sc, bool narrow) {
    // the packed fills carry V' = 2V + p (no alive flag): sentinel-free pairs only
    if (!sentinel_free(sc, len_q, len_db))
        return len_q <= 160 ? kLanes16x10 : len_q <= 256 ? kLanes16x16 : len_q <= 512 ? kLanes64x8 : kStripeVariant;
    // 8 x 19 groups (4-bit walk codes): queries of <= 152 columns, one
    // int16 frame or the rebasing one (launch_fill decides from the widest)
    if (narrow && len_q <= 152) {
        const Geom g = kVariantTable[kNarrowVariant].g;
        if (packed_single_ok(g.G, g.W(), len_db, sc) ||
            packed_ok_rebase(len_q, len_db, sc, g.G, g.W()))
            return kNarrowVariant;
    }
    // one int16 frame, judged as the launch judges it: over the whole width of
    // the variant's lane groups (a query narrower than its group once passed
    // here on its own width, and the launch then took the rebasing frame for
    // it without packed_ok_rebase having been asked)
    if (len_q <= 512) {
        const int v = len_q <= 160 ? kPacked16x10 : len_q <= 256 ? kPacked16x16 : kPacked32x16;
        const Geom g = kVariantTable[v].g;
        if (packed_single_ok(g.G, g.W(), len_db, sc)) return v;
    }
    // longer db: the same packed variants with a rebasing int16 frame; 513 to
    // 1,024 query columns in 64-lane groups (narrower queries would leave
    // most of those lanes idle: the i32 lanes are faster for them)
    for (const int v : {kPacked16x10, kPacked16x16, kPacked32x16}) {
        const Geom g = kVariantTable[v].g;
        if (len_q <= g.W() && packed_ok_rebase(len_q, len_db, sc, g.G, g.W())) return v;
    }
    const Geom wide = kVariantTable[kWidePackedVariant].g;
    if (len_q > 512 && packed_ok_rebase(len_q, len_db, sc, wide.G, wide.W())) return kWidePackedVariant;
    if (len_q <= 160) return kLanes16x10;
    if (len_q <= 256) return kLanes16x16;
    if (len_q <= 512) return kLanes64x8;
    return kStripeVariant;  // column stripes, one wave each (launch_fill_stripes)
}

int avsa_variant(uint32_t lq, uint32_t ld_max, const Scoring &sc, const Options &o) {
    const int v = choose_variant(lq, ld_max, sc);
    // score-only queries of <= 152 columns: 8-lane groups of 19 columns (no
    // mask, so no walker segment limit): the per-step overhead over 19
    // columns and 7 steps of skew instead of 10 and 15 (C5 slice 6,738 ->
    // 7,858 GCUPS); option nw.avsa_narrow = 0 keeps the 16 x 10 geometry
    // (32 groups per block stage their db rows in LDS: 4 B per row while
    // the db stays inside one int16 frame, <= 80 KB per block)
    if (v == kPacked16x10 && lq <= 152 && o[Opt::AvsaNarrow] != 0 && ld_max <= 600)
        return kNarrowVariant;
    return v;
}

// Queries of 513-1,024 columns: the 64-lane packed variant is the
// throughput choice (two pairs per wave), the column stripes the
// latency choice (four waves per pair, pipelined): a plan with fewer than
// nw.wide_min_pairs such pairs keeps them on stripes.
void demote_wide_pairs(NwPairDesc *descs, uint64_t n, const Options &o) {
    const auto wide = [](const NwPairDesc &d) {
        return d.variant == (uint32_t)kWidePackedVariant && d.len_q > 512;
    };
    const uint64_t n_wide = (uint64_t)std::count_if(descs, descs + n, wide);
    if (n_wide && n_wide < (uint64_t)o[Opt::WideMinPairs])
        for (NwPairDesc *d = descs; d != descs + n; ++d)
            if (wide(*d)) d->variant = (uint32_t)kStripeVariant;
}

// The table-penalty fill's bonuses fit a byte (fill_pk_body, kTab) and its
// frame's floor, a few opens below zero, stays far inside int16.
static bool pk_tab_ok(const Scoring &sc) {
    const int64_t cm = 2ll * sc.match - 4ll * sc.gap_extend, cmm = 2ll * sc.mismatch - 4ll * sc.gap_extend;
    return cmm >= 0 && cm <= 255 && cmm < cm && -(int64_t)sc.gap_open <= 2000;
}
// ... and its values, biased by kFreeBias, stay positive normal halves for
// W-column lanes groups over `rows` rows: X~ = X' + 2|ge|(r + c) is at least
// the all-gap path's 4go + 4ge less an open and a mismatch for M / I / D, at
// most rows (2|m| + 2|ge|) + 2|ge| W plus the boundary flag.
// scale: 2 (V = 2x + p) or 4 (the scale-4 table body, kTabMode 4): every
// bound scales with it, and its bonuses must still fit a byte.
static bool pk_free_ok(const Scoring &sc, uint32_t W, uint32_t rows, int scale = 2) {
    if (!pk_tab_ok(sc)) return false;
    const int64_t m = std::abs(sc.match), mm = std::abs(sc.mismatch), ge = std::abs(sc.gap_extend),
                  go = std::abs(sc.gap_open);
    const int64_t f = scale / 2;
    if (f * (2ll * sc.match - 4ll * sc.gap_extend) > 255) return false;
    const int64_t lo = f * (6 * go + 6 * ge + 2 * mm + 64);
    const int64_t hi = f * ((int64_t)rows * (2 * m + 2 * ge) + 2 * ge * (int64_t)W + 2 * go + 64);
    return lo <= kFreeBias - 0x400 && hi <= 0x7BFF - kFreeBias;
}

// The table body's frame holds a launch of G x K lane groups with dbs of up
// to ld_max rows: nw.pk_tab is on, the extension-free frame holds the rows and
// the staged rows fit the LDS (the table body stages 32-bit row words, a
// rebasing fallback 16-bit ones: four workgroups per CU where it had them).
bool pk_table_ok(uint32_t G, uint32_t K, uint32_t ld_max, bool rebase, const Scoring &sc,
                 const Options &o) {
    const size_t lds = staged_lds_bytes(G, ld_max, rebase ? 2 : 4);
    return o[Opt::PkTab] && pk_free_ok(sc, G * K, ld_max) &&
           staged_lds_bytes(G, ld_max, 4) <= std::max(lds, kLdsPerCu / 4);
}

// The body a packed plan launch of G x K lane groups runs (FillPath::table):
// the table body where the launch stores 4-bit walk codes, or full parent
// sets in 16-lane groups, the workspace has a bail word and the table body's
// frame holds the launch (pk_table_ok); else the generic body.  nw.pk_tab 1:
// scale 2; 2: the scale-4 body where its window holds the launch, else scale
// 2; 3: row profiles (scale 2).  Full parent sets: row profiles.
static int pk_table_body(uint32_t G, uint32_t K, int codes, uint32_t ld_max, bool rebase,
                         const Scoring &sc, const Options &o, bool have_bail) {
    if (codes != kCodesNib && !(codes == kCodesFull && G == 16)) return 0;
    if (!have_bail || !pk_table_ok(G, K, ld_max, rebase, sc, o)) return 0;
    if (codes == kCodesFull) return 3;
    return o[Opt::PkTab] == 2 && pk_free_ok(sc, G * K, ld_max, 4) ? 4 : o[Opt::PkTab] == 3 ? 3 : 2;
}

FillPath fill_path(int variant, int codes, uint32_t ld_max, const Scoring &sc, const Options &o,
                   bool have_bail) {
    FillPath fp;
    const VariantRow &row = kVariantTable[variant];
    fp.packed = row.packed;
    if (!fp.packed) return fp;
    // packed pairs beyond one int16 frame (packed_ok_rebase) take the rebasing fill
    fp.rebase = !packed_single_ok(row.g.G, row.g.W(), ld_max, sc);
    fp.table = pk_table_body(row.g.G, row.g.K, codes, ld_max, fp.rebase, sc, o, have_bail);
    return fp;
}

uint64_t packed_blocks(uint32_t G, uint64_t count, uint32_t per_group) {
    const uint64_t gpb = 256 / G, sup = 8 * blocks_per_pack(per_group * (uint32_t)gpb);
    const uint64_t groups = (count + per_group - 1) / per_group;
    return ((groups + gpb - 1) / gpb + sup - 1) / sup * sup;
}

// Lanes per pair of a packed class's all-vs-all launch (0: not a packed variant)
static uint32_t avsa_lanes(int variant) {
    return variant_in_range(variant) && kVariantTable[variant].packed ? kVariantTable[variant].g.G : 0;
}

// The most pairs one launch of a packed class may take: the dispatch packet's
// grid size is a 32-bit count of work-items (blocks * 256 <= 2^32 - 1), so
// the largest whole number of super-blocks below that, two pairs per group.
uint64_t avsa_chunk_pairs(int variant) {
    const uint32_t G = avsa_lanes(variant);
    if (!G) return 0;
    const uint64_t gpb = 256 / G, sup = 8 * blocks_per_pack(2 * (uint32_t)gpb);
    const uint64_t blocks = (0xFFFFFFFFull / 256) / sup * sup;
    return std::min<uint64_t>(blocks * gpb * 2, 0x80000000ull);  // count is a uint32
}

uint64_t avsa_launch_blocks(int variant, uint64_t count) {
    const uint32_t G = avsa_lanes(variant);
    return G ? packed_blocks(G, count) : 0;
}

// Row-fill columns per lane: K = 1 (64-column stripes) while every stripe
// wave of the plan has a SIMD to itself (a shorter row step: C1 0.197 ->
// 0.188 ms, 5 kbp 0.75 -> 0.70 ms), else K = 2 (C4: 1,564 K = 1 waves share
// SIMDs, 19.5 vs 14.5 ms).  Option nw.rows_k = 1, 2 or 4 forces it (read per
// plan).
int stripe_rows_k(uint64_t waves_k1, const Options &o) {
    if (const int64_t v = o[Opt::RowsK]) return v == 1 ? 1 : 2;
    return waves_k1 <= 1024 ? 1 : 2;
}

// The packed stripe fill holds a row relative to the stripe's left input:
// within 256 columns of it values span 256 * (2|m| + 4|ge|) plus the gap
// and penalty offsets of M / I / D (see nw_fill_stripe_pk_kernel).
// The packed stripe fill: its 128-virtual-lane chain doubles a stripe's skew,
// so one long pair (C4, 391 waves alone on their SIMDs) fills slower (45.4 vs
// 40.1 ms) although the step is cheaper; once the stripe waves fill the chip
// it wins (400 x 5 kbp pairs: 8.0 vs 9.2 ms end to end).  Chosen per plan
// from the stripe-wave count; option nw.stripe_pk = 0 / 1 forces it.
bool stripe_packed(const Scoring &sc, uint64_t n_waves, bool wide, const Options &o) {
    const int64_t force = o[Opt::StripePk];  // -1 auto
    if (force == 0) return false;
    if (force != 1 && (n_waves < kStripePkMinWaves || !wide)) return false;
    const int64_t pen = 2ll * (sc.match - sc.mismatch);
    if (pen < 2 || pen > 32 || sc.gap_extend > 0 || sc.gap_open > 0) return false;
    const int64_t m = std::abs(sc.match), ge = std::abs(sc.gap_extend), go = std::abs(sc.gap_open);
    return 256 * (2 * m + 4 * ge) + 4 * (go + ge) + 2 * pen + 512 < 30000;
}

}  // namespace saln
