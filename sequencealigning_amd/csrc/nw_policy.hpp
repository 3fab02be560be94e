// NW variant policy: which fill variant a pair takes, which frame and body a
// packed launch runs, how many blocks it gets.  Integer arithmetic only, no
// HIP: tested on the CPU (tests/test_nw_policy.py).  The launch layer
// (nw_kernels.hip) and the hosts ask here and never restate a condition.
#pragma once
#include <algorithm>
#include <cstdint>

#include "nw_common.hpp"
#include "saln_options.hpp"

namespace saln {

// The fill variants (NwPairDesc::variant): i32 lane groups of G x K columns,
// column stripes, packed int16 (two pairs per lane group).
enum Variant : int {
    kLanes16x10 = 0,         // i32 lanes, queries of <= 160 columns
    kLanes16x16 = 1,         // <= 256
    kLanes64x8 = 2,          // <= 512
    kStripeVariant = 3,      // column stripes (launch_fill_stripes)
    kNarrowVariant = 4,      // packed 8 x 19 groups, queries of <= 152 columns
    kPacked16x16 = 5,        // <= 256
    kPacked32x16 = 6,        // <= 512
    kPacked16x10 = 7,        // <= 160
    kWidePackedVariant = 8,  // packed, 64-lane groups, up to 1,024 columns
};

// One row per variant: the geometry of its fill kernel and its mask layout,
// packed int16 halves or i32 lanes, and whether its walk codes may be 4-bit
// (kCodesNib): the short-query packed fills, 16 x 10 and 8 x 19 (4-bit only).
// (8-lane groups of 20 columns writing the 16 x 10 layout measured equal in
// round 1: 202 VGPRs halve the occupancy.)
struct VariantRow {
    Geom g;
    bool packed, nib;
};
constexpr VariantRow kVariantTable[kNumVariants] = {
    {{16, 10}, false, false}, {{16, 16}, false, false}, {{64, 8}, false, false},
    {{64, 4}, false, false},  {{8, 19}, true, true},    {{16, 16}, true, false},
    {{32, 16}, true, false},  {{16, 10}, true, true},   {{64, 16}, true, false}};

inline bool variant_in_range(int v) { return v >= 0 && v < kNumVariants; }
inline Geom variant_geom(int v) { return kVariantTable[v].g; }
inline bool variant_packed(int v) { return kVariantTable[v].packed; }
inline bool variant_nib(int v) { return kVariantTable[v].nib; }

int choose_variant(uint32_t len_q, uint32_t len_db, const Scoring &sc, bool narrow = false);
// the score-only all-vs-all's variant of a query against dbs of up to ld_max rows
int avsa_variant(uint32_t lq, uint32_t ld_max, const Scoring &sc, const Options &o);
// A plan's pairs of 513-1,024 query columns: the 64-lane packed variant that
// choose_variant gave them, or column stripes when the plan has few of them
void demote_wide_pairs(NwPairDesc *descs, uint64_t n, const Options &o);

bool packed_range_ok(uint32_t lq, uint32_t rows, const Scoring &sc);
bool packed_single_ok(uint32_t G, uint32_t W, uint32_t ld, const Scoring &sc);
bool pk_table_ok(uint32_t G, uint32_t K, uint32_t ld_max, bool rebase, const Scoring &sc,
                 const Options &o);

// What launch_fill does with a variant's pairs (saln_nw_plan_pair_path reports
// it): packed int16 halves or i32 lanes; for packed launches the rebasing
// frame (the longest db leaves the single int16 frame) and the body: 0
// generic, 2 / 4 the table body at that scale, 3 row profiles.
struct FillPath {
    bool packed = false, rebase = false;
    int table = 0;
};
FillPath fill_path(int variant, int codes, uint32_t ld_max, const Scoring &sc, const Options &o,
                   bool have_bail);

// Blocks of a launch of `count` pairs in G-lane groups of per_group pairs
// (packed fills: two), 256 / G groups per block, rounded up to whole XCD
// super-blocks of 8 * blocks_per_pack blocks (pack_block).
uint64_t packed_blocks(uint32_t G, uint64_t count, uint32_t per_group = 2);

// row fill (nw_fill_rows_kernel) columns per lane, 0 = the skewed stripe fill;
// waves_k1: the plan's stripe waves at one column per lane
int stripe_rows_k(uint64_t waves_k1, const Options &o);
// column stripes run the packed (int16 halves) fill for this scoring and
// this many stripe waves in the plan (decided once per plan: it sets the layout)
bool stripe_packed(const Scoring &sc, uint64_t n_waves, bool wide, const Options &o);

// score-only all-vs-all (nw_avsa.cpp); avsa_chunk_pairs: the most pairs one
// launch of a packed class may take (0: not a packed variant)
uint64_t avsa_chunk_pairs(int variant);
uint64_t avsa_launch_blocks(int variant, uint64_t count);  // workgroups of one launch

}  // namespace saln
