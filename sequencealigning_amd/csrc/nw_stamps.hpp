// Device-side time stamps of timed NW executes: which plans take them, the
// slot bookkeeping of the stamp pool, and what a slot's words mean.  No HIP:
// tested on the CPU (tests/test_nw_stamps.py, tests/host/nw_stamps_check.cpp).
//
// A stamped execute owns one slot of kStampWords device words.  The fill
// kernels fold their span into words 0 and 1, the walk kernels theirs into
// words 2 and 3 (nw_common.hpp stamp_begin / stamp_end): the first wave of
// every workgroup does max(word, ~clock of its start) and max(word, clock) at
// its end, so a span's first word is the complement of its earliest start and
// its second word the latest end.  A zeroed slot is an unused one, and a span whose
// kernels did not run stays {0, 0}.  The clock is the device's constant-rate
// wall clock (hipDeviceAttributeWallClockRate, kHz).
#pragma once
#include <cstdint>

#include "nw_policy.hpp"

namespace saln {

constexpr uint32_t kStampWords = 4;   // fill begin, fill end, walk begin, walk end
constexpr uint32_t kStampChunk = 64;  // slots per block of the pool (a block per chunk of executes)

// The one rule: a timed execute is stamped iff every fill and walk kernel it
// launches takes the stamp pointer - the packed fills (nw_fill_pk_kernel,
// nw_fill_pk_tab_kernel) with the LDS or the generic walk, in a pipelined plan
// that walks.  Everything else (i32-lanes and column-stripe variants with
// their cooperative and speculative walks, score-only and sequential plans,
// nw.timing_mode = 1, the default) keeps the hipEvent path.  var_count: pairs per variant.
inline bool stamps_supported(const uint32_t *var_count, bool async_tb, bool score_only,
                             int64_t timing_mode) {
    if (timing_mode != 0 || !async_tb || score_only) return false;
    for (int v = 0; v < kNumVariants; ++v)
        if (var_count[v] && !variant_packed(v)) return false;
    return true;
}

// Slots of the pool: blocks of kStampChunk slots, handed out in order since
// the last resolve.  The owner allocates (and zeroes) a block when full().
struct StampBook {
    uint32_t blocks = 0;  // device blocks the owner holds
    uint32_t used = 0;    // slots taken since the last reset
    struct Slot {
        uint32_t block, word;  // word offset within the block
    };
    bool full() const { return used == blocks * kStampChunk; }
    void grew() { ++blocks; }
    Slot take() {  // !full()
        const Slot s{used / kStampChunk, (used % kStampChunk) * kStampWords};
        ++used;
        return s;
    }
    // slots of block b taken since the last reset (what a resolve copies back
    // and zeroes again)
    uint32_t used_in(uint32_t b) const {
        const uint32_t lo = b * kStampChunk;
        return used <= lo ? 0 : (used - lo < kStampChunk ? used - lo : kStampChunk);
    }
    void reset() { used = 0; }
};

// One span of a slot: its two words decoded.
struct StampSpan {
    uint64_t begin = 0, end = 0;  // ticks
    bool ran = false;             // a kernel stamped it
};
inline StampSpan stamp_span(const uint64_t *w) {
    StampSpan s;
    s.ran = w[0] != 0 && w[1] != 0;
    if (s.ran) {
        s.begin = ~w[0];
        s.end = w[1];
    }
    return s;
}
// signed tick difference a - b in ms at rate_khz ticks per ms
inline double stamp_ms(uint64_t a, uint64_t b, double rate_khz) {
    return (double)(int64_t)(a - b) / rate_khz;
}

// Totals over resolved executes, by the names saln_nw_plan_kernel_time serves.
struct StampTotals {
    struct Sum {
        double ms = 0;
        uint64_t n = 0;
        void add(double v) {
            ms += v;
            ++n;
        }
    };
    Sum fill, walk, execute;  // "nw_fill", "nw_traceback", "nw_execute" (fill begin to walk end)
    Sum fill_gap;             // "nw_fill_gap": fill begin of execute n+1 - fill end of execute n
    Sum handoff;              // "nw_handoff": walk begin - fill end
};
// Adds the n slots at w (the executes of one resolve, in order).  An execute
// without fill kernels (every pair has an empty side) counts a zero fill at
// its walk's begin; gaps are taken between neighbours that both filled.
inline void stamp_accumulate(const uint64_t *w, uint32_t n, double rate_khz, StampTotals *t) {
    StampSpan prev_fill;
    for (uint32_t k = 0; k < n; ++k, w += kStampWords) {
        StampSpan f = stamp_span(w);
        const StampSpan x = stamp_span(w + 2);
        if (!f.ran) f.begin = f.end = x.begin;
        t->fill.add(stamp_ms(f.end, f.begin, rate_khz));
        t->walk.add(stamp_ms(x.end, x.begin, rate_khz));
        t->execute.add(stamp_ms(x.end, f.begin, rate_khz));
        if (f.ran) t->handoff.add(stamp_ms(x.begin, f.end, rate_khz));
        if (f.ran && prev_fill.ran) t->fill_gap.add(stamp_ms(f.begin, prev_fill.end, rate_khz));
        prev_fill = f;
    }
}

}  // namespace saln
