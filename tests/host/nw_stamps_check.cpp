// CPU test (tests/test_nw_stamps.py): the HIP-free half of the timed NW
// executes' device-side stamps (nw_stamps.hpp) - which plans are stamped, the
// pool's slot bookkeeping, the decoding of a slot's words and the totals.
// Header-only: needs neither the library nor a HIP include path.  Prints
// "ok" and exits 0, or the failed check and exits 1.
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "nw_stamps.hpp"

using namespace saln;

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                   \
        }                                                               \
    } while (0)

// what the kernels do to a slot: max of the complemented start, max of the end
static void wave(uint64_t *w, uint64_t start, uint64_t end) {
    if (~start > w[0]) w[0] = ~start;
    if (end > w[1]) w[1] = end;
}

static bool near(double a, double b) { return a - b < 1e-9 && b - a < 1e-9; }

int main() {
    // ---- the rule
    {
        uint32_t vc[kNumVariants] = {};
        vc[kNarrowVariant] = 130;
        CHECK(stamps_supported(vc, true, false, 0));
        CHECK(!stamps_supported(vc, false, false, 0));  // sequential
        CHECK(!stamps_supported(vc, true, true, 0));    // score-only
        CHECK(!stamps_supported(vc, true, false, 1));   // nw.timing_mode = 1
        vc[kPacked16x10] = 3;
        vc[kPacked16x16] = vc[kPacked32x16] = vc[kWidePackedVariant] = 1;
        CHECK(stamps_supported(vc, true, false, 0));
        for (const int v : {(int)kLanes16x10, (int)kLanes16x16, (int)kLanes64x8, (int)kStripeVariant}) {
            vc[v] = 1;
            CHECK(!stamps_supported(vc, true, false, 0));
            vc[v] = 0;
        }
        const uint32_t none[kNumVariants] = {};  // empty-side pairs only: the generic walk
        CHECK(stamps_supported(none, true, false, 0));
    }
    // ---- slots: in order, none lost or handed out twice, across three blocks
    {
        StampBook bk;
        CHECK(bk.full());  // no block yet
        std::set<std::pair<uint32_t, uint32_t>> seen;
        const uint32_t n = 2 * kStampChunk + 6;
        uint32_t grows = 0;
        for (uint32_t k = 0; k < n; ++k) {
            if (bk.full()) {
                CHECK(k % kStampChunk == 0);  // at most once per chunk of executes
                bk.grew();
                ++grows;
            }
            const StampBook::Slot s = bk.take();
            CHECK(s.block == k / kStampChunk && s.word == (k % kStampChunk) * kStampWords);
            CHECK(s.block < bk.blocks && s.word + kStampWords <= kStampChunk * kStampWords);
            CHECK(seen.insert({s.block, s.word}).second);
        }
        CHECK(grows == 3 && bk.blocks == 3 && bk.used == n);
        CHECK(bk.used_in(0) == kStampChunk && bk.used_in(1) == kStampChunk && bk.used_in(2) == 6);
        CHECK(bk.used_in(3) == 0);
        bk.reset();
        CHECK(bk.used == 0 && bk.blocks == 3 && !bk.full() && bk.used_in(0) == 0);
        CHECK(bk.take().block == 0);
        CHECK(bk.used_in(0) == 1 && bk.used_in(1) == 0);
        StampBook one;
        one.grew();
        for (uint32_t k = 0; k < kStampChunk; ++k) {
            CHECK(!one.full());
            one.take();
        }
        CHECK(one.full() && one.used_in(0) == kStampChunk);
    }
    // ---- a span's words
    {
        uint64_t w[2] = {0, 0};
        CHECK(!stamp_span(w).ran);
        wave(w, 1000, 1500);
        wave(w, 900, 1400);   // the earliest start wins ...
        wave(w, 1200, 1900);  // ... and the latest end
        const StampSpan s = stamp_span(w);
        CHECK(s.ran && s.begin == 900 && s.end == 1900);
        // a clock near the top of its range still beats the zero
        uint64_t hi[2] = {0, 0};
        wave(hi, ~0ull - 5, ~0ull - 1);
        CHECK(stamp_span(hi).ran && stamp_span(hi).begin == ~0ull - 5);
    }
    // ---- ticks to ms: 100 MHz = 1e5 ticks per ms; signed
    CHECK(near(stamp_ms(250000, 50000, 1e5), 2.0));
    CHECK(near(stamp_ms(50000, 250000, 1e5), -2.0));
    CHECK(near(stamp_ms((1ull << 40) + 7, 1ull << 40, 1e5), 7e-5));
    // ---- totals over three pipelined executes (walk n beside fill n+1)
    {
        std::vector<uint64_t> w(3 * kStampWords, 0);
        const uint64_t T = 1ull << 33;
        for (uint32_t k = 0; k < 3; ++k) {
            uint64_t *s = w.data() + k * kStampWords;
            const uint64_t f0 = T + k * 100000;      // fills: 0.8 ms, 0.2 ms apart
            wave(s, f0 + 10, f0 + 70000);
            wave(s, f0, f0 + 80000);
            wave(s + 2, f0 + 81000, f0 + 150000);    // hand-off 10 us, walk 0.7 ms
            wave(s + 2, f0 + 82000, f0 + 151000);
        }
        StampTotals t;
        stamp_accumulate(w.data(), 3, 1e5, &t);
        CHECK(t.fill.n == 3 && near(t.fill.ms, 3 * 0.8));
        CHECK(t.walk.n == 3 && near(t.walk.ms, 3 * 0.7));
        CHECK(t.execute.n == 3 && near(t.execute.ms, 3 * 1.51));
        CHECK(t.handoff.n == 3 && near(t.handoff.ms, 3 * 0.01));
        CHECK(t.fill_gap.n == 2 && near(t.fill_gap.ms, 2 * 0.2));
        // a second resolve adds; the gap across the two is not counted
        stamp_accumulate(w.data(), 1, 1e5, &t);
        CHECK(t.fill.n == 4 && t.fill_gap.n == 2 && near(t.execute.ms, 4 * 1.51));
    }
    // ---- an execute without fill kernels: a zero fill at the walk's begin
    {
        uint64_t w[kStampWords] = {0, 0, 0, 0};
        wave(w + 2, 5000, 9000);
        StampTotals t;
        stamp_accumulate(w, 1, 1e5, &t);
        CHECK(t.fill.n == 1 && t.fill.ms == 0.0);
        CHECK(near(t.walk.ms, 0.04) && near(t.execute.ms, 0.04));
        CHECK(t.handoff.n == 0 && t.fill_gap.n == 0);
    }
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
