// CPU test (tests/test_nw_policy.py): what the NW variant policy (nw_policy.cpp)
// answers over a fixed grid, compared byte for byte with
// tests/golden/nw_policy_grid.txt.
//
// Per scheme and `narrow` a header line "# m,mm,go,ge narrow=N", then one line
// per (query width, db length), widths outer, in the order of kWidths / kLens:
//   <variant><flags><8 groups>
// flags: '-' i32 lanes, 'p' packed, 'r' packed with the rebasing frame.
// groups: fill_path(variant, codes, ld_max = the db length).table for bail word
// present then absent, within each the code formats 0..3, each group the four
// digits for nw.pk_tab = 0..3, or '.' where all four are 0.
// Per scheme a line "S" of stripe_packed for nw.stripe_pk = -1, 0, 1 x wide =
// 0, 1 x kWaves; at the end stripe_rows_k for nw.rows_k = 0, 1, 2 x kWaves and
// avsa_chunk_pairs / avsa_launch_blocks for variants -1 .. kNumVariants.
#include <cstdio>
#include <vector>

#include "nw_host.hpp"

using namespace saln;

static const uint32_t kWidths[] = {1, 150, 152, 153, 160, 161, 256, 257, 512, 513, 1024, 1025, 1300};
static const uint32_t kLens[] = {1, 8, 12, 100, 600, 624, 625, 700, 1227, 1228, 2000, 4096, 4097, 20000};
static const uint64_t kWaves[] = {1, 1023, 1024, 1025};
static const int kT[] = {1, 64, 256};

static Options with(Options o, Opt k, int64_t v) {
    o.v[(int)k] = v;
    return o;
}

int main() {
    std::vector<Scoring> schemes = {{5, -4, -8, -6}, {1, 0, 0, 0}, {2, -3, -5, -2}, {5, -4, -8, -600}};
    // the families of tests/test_nw_scheme_edges_gpu.py
    for (const int t : kT) {
        schemes.push_back({5, -4, -8, -t});
        schemes.push_back({t, t - 9, -8, -6});
        schemes.push_back({t, t - 5, -5, -2});
        schemes.push_back({t, t - 16, -8, -7});
        schemes.push_back({t, t - 16, 0, -40});
        schemes.push_back({t, t - 16, 0, -45});
    }
    const Options base = opt_registry();
    for (const Scoring &sc : schemes) {
        for (int narrow = 0; narrow < 2; ++narrow) {
            std::printf("# %d,%d,%d,%d narrow=%d\n", sc.match, sc.mismatch, sc.gap_open,
                        sc.gap_extend, narrow);
            for (const uint32_t lq : kWidths)
                for (const uint32_t ld : kLens) {
                    const int v = choose_variant(lq, ld, sc, narrow != 0);
                    const FillPath f0 = fill_path(v, 0, ld, sc, base, true);
                    std::printf("%d%c", v, !f0.packed ? '-' : f0.rebase ? 'r' : 'p');
                    for (int bail = 1; bail >= 0; --bail)
                        for (int codes = 0; codes < 4; ++codes) {
                            char g[5] = {};
                            bool any = false;
                            for (int tab = 0; tab < 4; ++tab) {
                                const FillPath fp =
                                    fill_path(v, codes, ld, sc, with(base, Opt::PkTab, tab), bail != 0);
                                if (fp.packed != f0.packed || fp.rebase != f0.rebase) {
                                    std::printf("\nfill_path: frame differs by codes / option\n");
                                    return 1;
                                }
                                g[tab] = (char)('0' + fp.table);
                                any |= fp.table != 0;
                            }
                            std::printf("%s", any ? g : ".");
                        }
                    std::printf("\n");
                }
        }
        std::printf("S");
        for (int force = -1; force <= 1; ++force)
            for (int wide = 0; wide < 2; ++wide)
                for (const uint64_t w : kWaves)
                    std::printf("%d", (int)stripe_packed(sc, w, wide != 0, with(base, Opt::StripePk, force)));
        std::printf("\n");
    }
    std::printf("rows_k");
    for (int k = 0; k <= 2; ++k)
        for (const uint64_t w : kWaves) std::printf(" %d", stripe_rows_k(w, with(base, Opt::RowsK, k)));
    std::printf("\n");
    for (int v = -1; v <= kNumVariants; ++v) {
        const uint64_t c = avsa_chunk_pairs(v);
        std::printf("avsa %d %llu %llu %llu\n", v, (unsigned long long)c,
                    (unsigned long long)avsa_launch_blocks(v, c),
                    (unsigned long long)avsa_launch_blocks(v, 1000001));
    }
    return 0;
}
