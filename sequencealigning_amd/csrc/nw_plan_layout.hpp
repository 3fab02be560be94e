// NW plan layout: everything a plan decides about its pairs before a device
// call is made: the variant and plan order of every pair, the offsets of its
// parent codes, boundary columns and op stream, the column stripes' layout
// and work list, the speculative-walk tables.  Integer arithmetic only, no
// HIP: tested on the CPU (tests/test_nw_plan_layout.py).  plan_create
// (nw_host.cpp) runs it, then allocates and uploads what it says; the fills
// and walkers trust every offset written here.
#pragma once
#include <cstdint>
#include <vector>

#include "nw_common.hpp"
#include "nw_policy.hpp"
#include "pair_index.hpp"
#include "saln.h"

namespace saln {

Scoring scoring_or_default(const saln_nw_scoring *s);
// a pair of these lengths stays inside the i32 fills' range under s
bool scores_fit_i32(const Scoring &s, uint64_t lq, uint64_t ld);

// Two words as the device reads them (uint2): a stripe work item (plan index,
// chunk) or a speculative block (spec pair, stripe).
struct Word2 {
    uint32_t x, y;
};

struct NwPlanLayout {
    std::vector<NwPairDesc> h_pairs;   // plan order, every field final
    std::vector<uint32_t> plan_index;  // results index -> plan order
    std::vector<uint64_t> cigar_off;   // results order, n_pairs + 1
    uint64_t cells = 0;
    uint32_t n_fill = 0;  // plan order: [0, n_fill) filled pairs, then empty-side pairs
    uint32_t var_first[kNumVariants] = {}, var_count[kNumVariants] = {};
    uint32_t var_maxld[kNumVariants] = {};  // longest db of each variant's pairs
    bool nib[kNumVariants] = {};  // variant stores 4-bit walk codes (Geom::LBn segments)
    bool stripe_pk = false;   // column stripes use the packed fill and layout
    int stripe_rows = 0;      // else: row fill with this many columns per lane (0 = skewed fill)
    uint32_t stripe_sub = 1;  // boundary columns per 256-column chunk
    uint64_t mask_bytes = 0, scratch_elems = 0, ops_words = 0;
    // column-stripe pairs (kStripeVariant): work items (plan index, chunk),
    // per-pair first work item (plan order, n_pairs + 1), progress counters
    // (NwPairDesc::reserved: a pair's first)
    std::vector<Word2> work;
    std::vector<uint32_t> work_first;
    uint64_t n_prog = 0;
    bool bail = false;  // a table fill among the launches: the workspaces need bail words
    // speculative stripe walks (a few long column-stripe pairs): pairs and
    // block map; spec_passes and spec_strict are set when there are any
    std::vector<SpecPair> spec_pair_tab;
    std::vector<Word2> spec_block_tab;
    int spec_passes = 0;
    bool spec_strict = false;  // nw.spec_strict: a pair left to the cooperative walker is an error
};

// The layout of a plan over pairs [0, n_pairs) of `pairs`.  full_codes: the
// fills store every parent set (host DFS, dense mask) instead of walk codes;
// it fixes the mask layout (4-bit walk codes for the short-query packed
// variants, bytes otherwise).  SALN_OK, or the refusal with its set_error text.
int nw_plan_layout(const uint64_t *q_off, const uint64_t *db_off, const PairIndex &pairs,
                   uint64_t n_pairs, int32_t mode, const Scoring &sc, const Options &opts,
                   bool full_codes, NwPlanLayout *out);

}  // namespace saln
