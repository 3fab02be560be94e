// CPU test (tests/test_nw_plan_layout.py): what the NW plan layout
// (nw_plan_layout.cpp) decides for a fixed set of small batches, compared byte
// for byte with tests/golden/nw_plan_layout.txt.  Sequences are never read:
// a batch is its offset tables and pair lists.
//
// Per batch a header "## name full=F scoring options", then "rc=R msg=M" and,
// when R is 0:
//   plan   the plan-level fields
//   var    per variant with pairs: first, count, longest db, 4-bit codes
//   index  plan_index (results index -> plan order)
//   cigar  cigar_off (results order, n + 1)
//   P      one line per pair in plan order, every NwPairDesc field:
//          q_off db_off mask_off mask_rs mask_bs mask_cs cigar_off scratch_off
//          ops_off len_q len_db pair_id variant reserved
//   first  work_first (plan order, n + 1)
//   work / blocks  the stripe work list / speculative block map as runs
//          x:y0-y1 (items (x, y0) .. (x, y1) in order)
//   S      one line per speculative pair: plan_idx n_stripes stripe_base reserved
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "nw_plan_layout.hpp"

using namespace saln;
using Shapes = std::vector<std::pair<uint64_t, uint64_t>>;  // (query columns, db rows) per pair

static const Scoring kDefault{5, -4, -8, -6};

static Options with(Options o, Opt k, int64_t v) {
    o.v[(int)k] = v;
    return o;
}

template <typename T>
static void list(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

static void runs(const char *tag, const std::vector<Word2> &v) {
    std::printf("%s", tag);
    for (size_t i = 0; i < v.size();) {
        size_t j = i + 1;
        while (j < v.size() && v[j].x == v[i].x && v[j].y == v[j - 1].y + 1) ++j;
        std::printf(" %u:%u-%u", v[i].x, v[i].y, v[j - 1].y);
        i = j;
    }
    std::printf("\n");
}

static void dump(const char *name, const uint64_t *q_off, const uint64_t *db_off,
                 const PairIndex &pairs, uint64_t n_pairs, int32_t mode, const Scoring &sc,
                 const Options &o, bool full) {
    std::printf("## %s full=%d %d,%d,%d,%d wide_min=%lld rows_k=%lld stripe_pk=%lld spec=%lld "
                "passes=%lld strict=%lld\n",
                name, (int)full, sc.match, sc.mismatch, sc.gap_open, sc.gap_extend,
                (long long)o[Opt::WideMinPairs], (long long)o[Opt::RowsK],
                (long long)o[Opt::StripePk], (long long)o[Opt::Spec],
                (long long)o[Opt::SpecPasses], (long long)o[Opt::SpecStrict]);
    set_error("");
    NwPlanLayout L;
    const int rc = nw_plan_layout(q_off, db_off, pairs, n_pairs, mode, sc, o, full, &L);
    std::printf("rc=%d msg=%s\n", rc, saln_last_error());
    if (rc != SALN_OK) return;
    std::printf("plan n=%zu cells=%llu n_fill=%u stripe_pk=%d stripe_rows=%d stripe_sub=%u "
                "mask_bytes=%llu scratch_elems=%llu ops_words=%llu n_prog=%llu bail=%d "
                "spec_passes=%d spec_strict=%d\n",
                L.h_pairs.size(), (unsigned long long)L.cells, L.n_fill, (int)L.stripe_pk,
                L.stripe_rows, L.stripe_sub, (unsigned long long)L.mask_bytes,
                (unsigned long long)L.scratch_elems, (unsigned long long)L.ops_words,
                (unsigned long long)L.n_prog, (int)L.bail, L.spec_passes, (int)L.spec_strict);
    for (int v = 0; v < kNumVariants; ++v)
        if (L.var_count[v] || L.var_first[v] || L.var_maxld[v])
            std::printf("var %d first=%u count=%u maxld=%u\n", v, L.var_first[v], L.var_count[v],
                        L.var_maxld[v]);
    std::printf("nib");
    for (int v = 0; v < kNumVariants; ++v) std::printf(" %d", (int)L.nib[v]);
    std::printf("\n");
    list("index", L.plan_index);
    list("cigar", L.cigar_off);
    for (const NwPairDesc &d : L.h_pairs)
        std::printf("P %llu %llu %llu %llu %u %llu %llu %llu %llu %u %u %u %u %u\n",
                    (unsigned long long)d.q_off, (unsigned long long)d.db_off,
                    (unsigned long long)d.mask_off, (unsigned long long)d.mask_rs, d.mask_bs,
                    (unsigned long long)d.mask_cs, (unsigned long long)d.cigar_off,
                    (unsigned long long)d.scratch_off, (unsigned long long)d.ops_off, d.len_q,
                    d.len_db, d.pair_id, d.variant, d.reserved);
    list("first", L.work_first);
    runs("work", L.work);
    for (const SpecPair &s : L.spec_pair_tab)
        std::printf("S %u %u %u %u\n", s.plan_idx, s.n_stripes, s.stripe_base, s.reserved);
    runs("blocks", L.spec_block_tab);
}

// pair k = (query k, db k) of the given shapes, through explicit pair lists
static void batch(const char *name, const Shapes &shapes, const Scoring &sc, const Options &o,
                  bool full = false) {
    std::vector<uint64_t> q_off{0}, db_off{0};
    std::vector<uint32_t> idx;
    for (const auto &s : shapes) {
        idx.push_back((uint32_t)idx.size());
        q_off.push_back(q_off.back() + s.first);
        db_off.push_back(db_off.back() + s.second);
    }
    dump(name, q_off.data(), db_off.data(),
         PairIndex{idx.data(), idx.data(), shapes.size(), shapes.size()}, shapes.size(),
         SALN_MODE_GLOBAL, sc, o, full);
}

static Shapes alike(size_t n, uint64_t lq, uint64_t ld) { return Shapes(n, {lq, ld}); }

int main() {
    std::printf("# NW plan layout over the batches of tests/host/nw_plan_layout_dump.cpp.\n"
                "# Written by that program from plan_create as it was before nw_plan_layout.cpp\n"
                "# existed (its body with the device calls cut, behind nw_plan_layout()'s\n"
                "# interface), not from the module: the module has to reproduce it.\n");
    const Options base = opt_registry();
    batch("empty batch", {}, kDefault, base);
    batch("empty sides among filled pairs",
          {{0, 0}, {150, 150}, {0, 40}, {200, 100}, {33, 0}, {150, 151}, {0, 0}}, kDefault, base);

    // variant edges: the all-vs-all grid (no pair lists), query-inner
    {
        std::vector<uint64_t> q_off{0}, db_off{0};
        for (const uint64_t w : {152, 153, 160, 161, 256, 257, 512, 513, 1024, 1025})
            q_off.push_back(q_off.back() + w);
        for (const uint64_t l : {1, 64, 300}) db_off.push_back(db_off.back() + l);
        for (int full = 0; full < 2; ++full)
            dump("variant edges (grid)", q_off.data(), db_off.data(),
                 PairIndex{nullptr, nullptr, 10, 3}, 30, SALN_MODE_GLOBAL, kDefault, base, full != 0);
    }

    // order: a batch in plan order (no copy), and the same pairs shuffled
    batch("in plan order", {{1300, 300}, {100, 300}, {150, 200}, {150, 200}, {120, 90}, {200, 400},
                            {256, 50}, {0, 10}}, kDefault, base);
    batch("shuffled", {{256, 50}, {0, 10}, {150, 200}, {1300, 300}, {120, 90}, {100, 300},
                       {200, 400}, {150, 200}}, kDefault, base);

    // mask packs: 64 and 65 alike pairs (4-bit codes)
    batch("64 alike", alike(64, 150, 150), kDefault, base);
    batch("65 alike", alike(65, 150, 150), kDefault, base);
    // the 25 % rule, byte codes (16 x 16 groups: 256 bytes per row): four
    // pairs, 4 * packed <= 5 * own + 4096 up to a longest db of 137 rows
    batch("pack: just below", {{200, 100}, {200, 137}, {200, 100}, {200, 100}}, kDefault, base);
    batch("pack: just above", {{200, 100}, {200, 138}, {200, 100}, {200, 100}}, kDefault, base);
    // ... and 4-bit codes (8 x 19 groups: 12 bytes per block, 96 per row):
    // 16 M <= 1500 + 5 M + 4096 / 96
    batch("pack nib: just below", {{150, 100}, {150, 140}, {150, 100}, {150, 100}}, kDefault, base);
    batch("pack nib: just above", {{150, 100}, {150, 141}, {150, 100}, {150, 100}}, kDefault, base);
    batch("pack: mixed widths and full codes", {{150, 100}, {100, 100}, {40, 100}, {160, 30}},
          kDefault, base, true);

    // wide pairs (513 to 1,024 columns): few stay on stripes, many go packed
    const Shapes wide = {{600, 200}, {1024, 300}, {513, 100}, {700, 200}, {150, 150}};
    batch("wide: few", wide, kDefault, base);
    batch("wide: many", wide, kDefault, with(base, Opt::WideMinPairs, 4));
    batch("wide: one short of many", wide, kDefault, with(base, Opt::WideMinPairs, 5));

    // column stripes: the row fill at one column per lane (stripe_sub 4), two
    // (65,537 columns: 1,025 stripes of 64; stripe_sub 2), forced
    const Shapes two = {{1300, 300}, {2000, 250}};
    batch("stripes: rows 1", two, kDefault, base);
    batch("stripes: rows 2", {{65537, 3}, {1300, 301}}, kDefault, base);
    batch("stripes: rows 2 forced", two, kDefault, with(base, Opt::RowsK, 2));
    batch("stripes: rows 1 forced", {{65537, 3}}, kDefault, with(base, Opt::RowsK, 1));
    // packed stripes (stripe_sub 1): forced, refused where a pair is not
    // sentinel-free, switched off
    batch("stripes: packed forced", two, kDefault, with(base, Opt::StripePk, 1));
    batch("stripes: packed forced, sentinel", two, Scoring{5, -4, -8, -30},
          with(base, Opt::StripePk, 1));
    // 86 pairs of 12 chunks: 1,032 >= kStripePkMinWaves; mean columns on both
    // sides of 3,000; nv above kSpecMaxPairs
    batch("stripes: 1032 waves, mean 2999", alike(86, 2999, 5), Scoring{1, 0, 0, 0}, base);
    batch("stripes: 1032 waves, mean 3000", alike(86, 3000, 5), Scoring{1, 0, 0, 0}, base);
    batch("stripes: 1032 waves, packed off", alike(86, 3000, 5), Scoring{1, 0, 0, 0},
          with(base, Opt::StripePk, 0));
    batch("stripes: 1020 waves, mean 3000", alike(85, 3000, 5), Scoring{1, 0, 0, 0}, base);
    batch("stripes: one pair of 1024 chunks", {{262144, 10}}, Scoring{1, 0, 0, 0}, base);

    // speculative walks: 7 stripes (below kSpecMinStripes), 8, 4,096 and 4,097
    // (above kSpecMaxStripes), beside table-fill pairs
    const Shapes spec = {{1792, 300}, {1793, 300}, {150, 300}, {2000, 290}, {150, 300}};
    batch("spec: 7 and 8 stripes", spec, kDefault, base);
    batch("spec: strict", spec, kDefault, with(base, Opt::SpecStrict, 1));
    batch("spec: off", spec, kDefault, with(base, Opt::Spec, 0));
    batch("spec: no passes", spec, kDefault, with(base, Opt::SpecPasses, 0));
    batch("spec: one pass", spec, kDefault, with(base, Opt::SpecPasses, 1));
    batch("spec: 4096 and 4097 stripes", {{1048576, 1}, {1048577, 1}}, kDefault, base);
    batch("spec: 16 pairs", alike(16, 2100, 20), kDefault, base);
    batch("spec: 17 pairs", alike(17, 2100, 20), kDefault, base);

    // refusals, in the order plan creation checks them
    {
        const uint64_t off2[] = {0, 100, 200}, huge[] = {0, 0x80000000ull};
        const uint64_t far[] = {0, 100000}, fits[] = {0, 0x7FFFFFFFull};
        const uint32_t i0[] = {0, 1}, bad[] = {0, 2};
        dump("refused: mode", off2, off2, PairIndex{i0, i0, 2, 2}, 2, SALN_MODE_GLOBAL + 1,
             kDefault, base, false);
        dump("refused: mode before the count", off2, off2, PairIndex{nullptr, nullptr, 2, 2}, 3,
             SALN_MODE_GLOBAL + 1, kDefault, base, false);
        dump("refused: one pair list", off2, off2, PairIndex{i0, nullptr, 2, 2}, 2,
             SALN_MODE_GLOBAL, kDefault, base, false);
        dump("refused: all-vs-all count", off2, off2, PairIndex{nullptr, nullptr, 2, 2}, 3,
             SALN_MODE_GLOBAL, kDefault, base, false);
        dump("refused: 2^32 pairs", off2, off2, PairIndex{i0, i0, 2, 2}, 1ull << 32,
             SALN_MODE_GLOBAL, kDefault, base, false);
        dump("refused: query index", off2, off2, PairIndex{bad, i0, 2, 2}, 2, SALN_MODE_GLOBAL,
             kDefault, base, false);
        dump("refused: db index", off2, off2, PairIndex{i0, bad, 2, 2}, 2, SALN_MODE_GLOBAL,
             kDefault, base, false);
        dump("refused: query too long", huge, off2, PairIndex{i0, i0, 1, 2}, 1, SALN_MODE_GLOBAL,
             kDefault, base, false);
        dump("refused: db too long", off2, huge, PairIndex{i0, i0, 2, 1}, 1, SALN_MODE_GLOBAL,
             kDefault, base, false);
        dump("refused: 2^31 - 1 columns, by range", fits, off2, PairIndex{i0, i0, 1, 2}, 1, SALN_MODE_GLOBAL,
             Scoring{1, 0, 0, 0}, base, false);
        dump("refused: penalties", far, far, PairIndex{i0, i0, 1, 1}, 1, SALN_MODE_GLOBAL,
             Scoring{10000, -10000, -10000, -10000}, base, false);
        // the index is checked before the lengths, the lengths before the range
        dump("refused: index before length", huge, huge, PairIndex{bad + 1, i0, 1, 1}, 1,
             SALN_MODE_GLOBAL, kDefault, base, false);
        dump("refused: second pair", far, far, PairIndex{i0, i0, 1, 1}, 2, SALN_MODE_GLOBAL,
             kDefault, base, false);
    }
    return 0;
}
