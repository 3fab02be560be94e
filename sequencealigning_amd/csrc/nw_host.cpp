// C ABI implementation for the NW-affine engine (include/saln.h).
//
// Replaces n_w_align (src/needleman_wunsch_affine.rs:424-437) and the
// db x query pair loop that calls it (src/main.rs:61-67).  All arithmetic
// runs in the HIP kernels of nw_kernels.hip; the host only plans batches,
// moves buffers and, for the reference's text output, walks the parent codes
// the GPU produced (the reference's exhaustive DFS, :281-329).
//
// What a plan decides (variants, plan order, every offset, the stripe work
// list, the speculative tables) is decided in nw_plan_layout.cpp, without
// HIP; this file holds the plan's device state: plan_create allocates and
// uploads what the layout says, PlanOwned owns every block and event, and
// saln_nw_execute launches over them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <array>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "nw_host.hpp"
#include "nw_stamps.hpp"

using namespace saln;

// a plan's table-fill bail words per mask workspace: one per fill variant
constexpr size_t kBailBytes = kNumVariants * sizeof(uint32_t);

// Every device block and event of a plan: what alloc() and event() hand out
// is recorded here and released here, all of it, however far creation got.
// The plan's typed pointers are views.  Blocks go back to the context cache,
// so nothing may still use them: saln_nw_plan_destroy syncs the device first.
struct PlanOwned {
    saln_context *ctx = nullptr;
    std::vector<void *> blocks;
    std::vector<hipEvent_t> events;
    PlanOwned() = default;
    PlanOwned(const PlanOwned &) = delete;
    PlanOwned &operator=(const PlanOwned &) = delete;
    template <typename T>
    hipError_t alloc(T **p, size_t bytes) {
        void *b = nullptr;
        const hipError_t e = dev_alloc(ctx, &b, bytes);
        if (e != hipSuccess) return e;
        blocks.push_back(b);
        *p = static_cast<T *>(b);
        return hipSuccess;
    }
    hipError_t event(hipEvent_t *ev, unsigned flags = hipEventDefault) {
        const hipError_t e = hipEventCreateWithFlags(ev, flags);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    ~PlanOwned() {
        for (void *b : blocks) dev_free(ctx, b);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
};

// The layout (nw_plan_layout.hpp: pairs in plan order, offsets, stripe layout,
// work list, speculative tables) and the device state built from it.
struct saln_nw_plan : NwPlanLayout {
    saln_context *ctx = nullptr;
    PlanOwned own;
    Options opts{};  // the context's effective options at creation
    Scoring sc{};
    uint64_t n_pairs = 0;
    NwPairDesc *d_pairs = nullptr;
    uint8_t *d_mask = nullptr;
    uint8_t *d_mask2 = nullptr;  // second workspace for the async (2-deep) pipeline
    int32_t *d_endh2 = nullptr;
    bool async_tb = false;
    int stripe_layout() const { return stripe_pk ? 1 : stripe_rows ? 2 : 0; }
    // launch_fill's code format for variant v and whether its launch has a bail word
    int fill_codes(int v) const {
        return score_only ? kCodesNone : full_codes ? kCodesFull : nib[v] ? kCodesNib : kCodesWalk;
    }
    bool has_bail() const { return d_bail[async_tb ? buf : 0] != nullptr; }
    bool full_codes = false;  // walk codes (default) or every parent set (decided at creation)
    bool score_only = false;  // no parent codes / traceback (saln_nw_plan_set_score_only)
    int buf = 0;                           // workspace of the next execute (async mode)
    hipStream_t tb_stream = nullptr;       // traceback stream of async executes (NULL: ctx's)
    bool tb_pending[2] = {false, false};
    int last_buf = 0;
    int2 *d_scratch = nullptr;
    uint2 *d_work = nullptr;  // the layout's stripe work list
    // d_err[0]: device error flags since the last saln_nw_plan_status (bit 0
    // a dependency wait timed out, bit 1 an unlinked speculative walk under
    // SALN_SPEC_STRICT); d_err[1]: the wait limit the fills read
    uint32_t *d_prog = nullptr, *d_err = nullptr;  // d_err: kErrWords (the row fill's XCD slots after the two)
    uint32_t fill_epoch = 0;  // stripe fills launched (the XCD slots' epochs)
    uint32_t wait_limit = kWaitLimitDefault;
    bool unchecked[2] = {false, false};  // executes on workspace b since the last status
    uint32_t *d_ops = nullptr;  // traceback op-stream scratch of workspace 0
    uint32_t *d_ops2 = nullptr;  // ... of workspace 1 (async: its walks may overlap workspace 0's)
    // per workspace: the table fills' bail word (zeroed once; a table launch
    // whose waves left pairs to its fallback launch stores its epoch there)
    uint32_t *d_bail[2] = {nullptr, nullptr};
    uint32_t epoch = 0;  // table launches of this plan (the bail word's values)
    // speculative stripe walks: the layout's block map and pairs on the
    // device, stripe records, run words, per-pair done flags (plan order)
    uint32_t spec_pairs = 0, spec_blocks = 0;
    uint2 *d_spec_blocks = nullptr;
    SpecPair *d_spec_pairs = nullptr;
    SpecStripe *d_spec_stripes = nullptr;
    uint32_t *d_spec_ops = nullptr, *d_spec_done = nullptr;
    int32_t *d_endh = nullptr;
    bool timing = false;
    // hipEvents around the fill and traceback launches of each execute;
    // resolved lazily (no host sync inside execute).
    std::vector<std::array<hipEvent_t, 4>> ev_pool;
    size_t ev_used = 0;
    // stamped plans (nw_stamps.hpp stamps_supported) take no events: their
    // kernels fold the device's wall clock into a slot of the stamp pool
    // (blocks of kStampChunk slots, zeroed; resolve_events reads the used
    // slots back and zeroes them again)
    bool stamped() const {
        return stamps_supported(var_count, async_tb, score_only, opts[Opt::TimingMode]);
    }
    std::vector<unsigned long long *> stamp_blocks;
    StampBook stamps;
    double clock_khz = 0;  // ticks per ms of the stamps' clock
    hipError_t stamp_grow(hipStream_t s);  // one more zeroed block (s null: synchronously)
    std::map<std::string, std::pair<double, uint64_t>> ktime;
    int resolve_events();
    // the two events after the sub-batch events mark "traceback of workspace b done"
    hipEvent_t tb_done(int b) const { return sync_ev[1 + b]; }
    // fill -> traceback stream hand-off (async) and "traceback of workspace b
    // done" (two events)
    std::vector<hipEvent_t> sync_ev;
};
// the layout's two-word items are copied to the device as uint2
static_assert(sizeof(Word2) == sizeof(uint2), "Word2 is read as uint2");

extern "C" {

int saln_abi_version(void) { return SALN_ABI_VERSION; }

int saln_context_create(int device, saln_context **out) {
    if (!out) return SALN_E_INVALID;
    *out = nullptr;
    // host.prefault_mb: the host buffer of render batches' parent codes,
    // allocated and faulted in on a helper thread while the HIP runtime
    // starts (~0.2 s; the CLI's first full chunk otherwise faults ~0.4 GB in
    // during its mask download: 56 ms, round 6)
    saln_context::HostBuf pre;
    std::thread pre_th;
    if (const int64_t mb = opt(Opt::HostPrefaultMb); mb > 0) {
        pre_th = std::thread([&pre, mb] {
            size_t want = 0;
            void *hp = huge_alloc((size_t)mb << 20, &want);
            if (!hp) return;
            std::memset(hp, 0, want);
            pre.p = (uint8_t *)hp;
            pre.n = want;
        });
    }
    struct Join {
        std::thread &t;
        ~Join() { if (t.joinable()) t.join(); }
    } join_pre{pre_th};
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) {
        set_error("no HIP device " + std::to_string(device) + " (saln has no CPU path)");
        return SALN_E_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("device is ") + prop.gcnArchName + ", saln is built for gfx950");
        return SALN_E_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    auto *c = new saln_context;
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->tb_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        set_error("hipStreamCreate failed");
        return SALN_E_HIP;
    }
    if (pre_th.joinable()) {
        pre_th.join();
        std::swap(c->host_mask.p, pre.p);
        std::swap(c->host_mask.n, pre.n);
    }
    *out = c;
    return SALN_OK;
}

int saln_context_destroy(saln_context *ctx) {
    if (!ctx) return SALN_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    dev_cache_clear(ctx);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->tb_stream) (void)hipStreamDestroy(ctx->tb_stream);
    delete ctx;
    return SALN_OK;
}

int saln_nw_plan_destroy(saln_nw_plan *p) {
    if (!p) return SALN_OK;
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();  // the blocks go back to the context cache
    delete p;                      // PlanOwned releases every block and event
    return SALN_OK;
}

int saln_nw_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                        const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                        const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                        const saln_nw_scoring *scoring, saln_nw_plan **out) {
    return saln::plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                             scoring, false, out);
}

int saln_nw_plan_create_full(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                             const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                             const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                             const saln_nw_scoring *scoring, saln_nw_plan **out) {
    return saln::plan_create(ctx, q_off, n_q, db_off, n_db, pair_q, pair_db, n_pairs, mode,
                             scoring, true, out);
}

int saln_nw_plan_dense_mask(saln_nw_plan *p, uint64_t pair, uint8_t *out) {
    if (!p || !out || pair >= p->n_pairs) return SALN_E_INVALID;
    if (p->async_tb) {  // the mask of the last execute may sit in either workspace
        set_error("saln_nw_plan_dense_mask: synchronous plans only");
        return SALN_E_INVALID;
    }
    if (p->score_only) {  // the fills of a score-only execute store no codes
        set_error("saln_nw_plan_dense_mask: the plan is score-only (set_score_only(0) and execute first)");
        return SALN_E_INVALID;
    }
    HIP_TRY(hipSetDevice(p->ctx->device));
    for (int b = 0; b < 2; ++b)
        if (p->tb_pending[b]) HIP_TRY(hipEventSynchronize(p->tb_done(b)));
    saln::PairMask pm;
    const int rc = saln::plan_pair_mask(p, pair, &pm);
    if (rc != SALN_OK) return rc;
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair]];
    const saln::HostMask hm(pm, d.len_q, d.len_db, p->sc);
    hm.to_dense(out);
    return SALN_OK;
}

int saln_nw_plan_walk_codes(saln_nw_plan *p, uint64_t pair, uint8_t *out) {
    if (!p || !out || pair >= p->n_pairs) return SALN_E_INVALID;
    if (p->async_tb) {
        set_error("saln_nw_plan_walk_codes: synchronous plans only");
        return SALN_E_INVALID;
    }
    if (p->score_only) {  // the fills of a score-only execute store no codes
        set_error("saln_nw_plan_walk_codes: the plan is score-only (set_score_only(0) and execute first)");
        return SALN_E_INVALID;
    }
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair]];
    if (d.variant >= (uint32_t)kNumVariants || !p->nib[d.variant] || !d.len_q || !d.len_db) {
        set_error("saln_nw_plan_walk_codes: the pair's fill stores no 4-bit walk codes");
        return SALN_E_INVALID;
    }
    HIP_TRY(hipSetDevice(p->ctx->device));
    for (int b = 0; b < 2; ++b)
        if (p->tb_pending[b]) HIP_TRY(hipEventSynchronize(p->tb_done(b)));
    // segments of block b at row i: mask_off + (i-1) rs + b bs (Geom::LBn
    // bytes; column c's nibble at bit nib_bit(c) of dword c / 8)
    const Geom g = variant_geom((int)d.variant);
    // every block of each row (rs / bs of them: the pack's width) as one
    // bs-pitched 2-D region of LBn-byte rows
    const uint64_t per_row = d.mask_rs / d.mask_bs;
    std::vector<uint8_t> all((uint64_t)d.len_db * per_row * g.LBn());
    HIP_TRY(hipMemcpy2D(all.data(), g.LBn(), p->d_mask + d.mask_off, d.mask_bs, g.LBn(),
                        (uint64_t)d.len_db * per_row, hipMemcpyDeviceToHost));
    for (uint32_t i = 1; i <= d.len_db; ++i)
        for (uint32_t j = 1; j <= d.len_q; ++j) {
            const uint32_t b = (j - 1) / g.K, c = (j - 1) % g.K;
            const uint8_t *sp = all.data() + ((uint64_t)(i - 1) * per_row + b) * g.LBn();
            uint32_t w;
            std::memcpy(&w, sp + 4 * (c >> 3), 4);
            const uint32_t bit = ((c & 4u) << 2) | ((c & 1u) << 3) | ((c & 2u) << 1);
            out[(uint64_t)(i - 1) * d.len_q + (j - 1)] = (uint8_t)((w >> bit) & 15u);
        }
    return SALN_OK;
}

}  // extern "C"

// Plan creation: the layout (nw_plan_layout.cpp decides everything), then
// the device blocks it asks for, then the uploads.  A failure on the way
// destroys the plan, which releases whatever it owns by then.
int saln::plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                      const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                      const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                      const saln_nw_scoring *scoring, bool full_codes, saln_nw_plan **out) {
    if (!ctx || !q_off || !db_off || !out) return SALN_E_INVALID;
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    const Options opts = ctx->opts.effective();
    StageClock clk(opts);
    const Scoring sc = scoring_or_default(scoring);
    NwPlanLayout lay;
    const int rc = nw_plan_layout(q_off, db_off, PairIndex{pair_q, pair_db, n_q, n_db}, n_pairs,
                                  mode, sc, opts, full_codes, &lay);
    if (rc != SALN_OK) return rc;
    struct Destroy {
        void operator()(saln_nw_plan *p) const { saln_nw_plan_destroy(p); }
    };
    std::unique_ptr<saln_nw_plan, Destroy> p(new saln_nw_plan);
    static_cast<NwPlanLayout &>(*p) = std::move(lay);
    p->ctx = p->own.ctx = ctx;
    p->opts = opts;
    p->sc = sc;
    p->full_codes = full_codes;
    p->n_pairs = n_pairs;
    p->sync_ev.resize(3);
    for (auto &e : p->sync_ev) HIP_TRY(p->own.event(&e, hipEventDisableTiming));
    clk.mark("plan: layout");
    if (n_pairs) {
        const size_t nb = n_pairs * sizeof(NwPairDesc);
        HIP_TRY(p->own.alloc(&p->d_pairs, nb));
        clk.mark("plan: pairs alloc");
        // through the context's pinned staging: a pageable copy of a freshly
        // built array pins its pages first (measured 12-17 ms for the 2.7-5.2
        // MB of a render chunk's descriptors, against ~1 ms of memcpy here)
        {
            std::lock_guard<std::mutex> lk(ctx->staging_mu);
            void *st = nullptr;
            HIP_TRY(pinned_staging(ctx, nb, &st));
            std::memcpy(st, p->h_pairs.data(), nb);
            HIP_TRY(hipMemcpy(p->d_pairs, st, nb, hipMemcpyHostToDevice));
        }
        HIP_TRY(p->own.alloc(&p->d_endh, n_pairs * sizeof(int32_t)));
    }
    clk.mark("plan: pairs h2d");
    // +64 B: the traceback walker reads whole 5-dword segments
    if (p->mask_bytes) HIP_TRY(p->own.alloc(&p->d_mask, p->mask_bytes + 64));
    if (!p->work.empty()) {  // column stripes: work list, progress counters, error words
        const size_t nb = p->work.size() * sizeof(Word2);
        HIP_TRY(p->own.alloc(&p->d_work, nb));
        HIP_TRY(hipMemcpy(p->d_work, p->work.data(), nb, hipMemcpyHostToDevice));
        HIP_TRY(p->own.alloc(&p->d_prog, p->n_prog * sizeof(uint32_t)));
        HIP_TRY(p->own.alloc(&p->d_err, kErrWords * sizeof(uint32_t)));
        // every XCD slot cleared: a recycled block must not hold a live epoch
        HIP_TRY(hipMemset(p->d_err, 0, kErrWords * sizeof(uint32_t)));
        const uint32_t err01[2] = {0u, kWaitLimitDefault};
        HIP_TRY(hipMemcpy(p->d_err, err01, sizeof err01, hipMemcpyHostToDevice));
    }
    clk.mark("plan: mask+work");
    if (p->scratch_elems) HIP_TRY(p->own.alloc(&p->d_scratch, p->scratch_elems * sizeof(int2)));
    if (p->ops_words) HIP_TRY(p->own.alloc(&p->d_ops, p->ops_words * sizeof(uint32_t)));
    if (p->bail) {
        HIP_TRY(p->own.alloc(&p->d_bail[0], kBailBytes));
        HIP_TRY(hipMemset(p->d_bail[0], 0, kBailBytes));
    }
    if (!p->spec_pair_tab.empty()) {
        p->spec_pairs = (uint32_t)p->spec_pair_tab.size();
        p->spec_blocks = (uint32_t)p->spec_block_tab.size();
        const size_t nb = p->spec_blocks * sizeof(Word2), np = p->spec_pairs * sizeof(SpecPair);
        HIP_TRY(p->own.alloc(&p->d_spec_blocks, nb));
        HIP_TRY(hipMemcpy(p->d_spec_blocks, p->spec_block_tab.data(), nb, hipMemcpyHostToDevice));
        HIP_TRY(p->own.alloc(&p->d_spec_pairs, np));
        HIP_TRY(hipMemcpy(p->d_spec_pairs, p->spec_pair_tab.data(), np, hipMemcpyHostToDevice));
        HIP_TRY(p->own.alloc(&p->d_spec_stripes, p->spec_blocks * sizeof(SpecStripe)));
        HIP_TRY(p->own.alloc(&p->d_spec_ops,
                             (size_t)p->spec_blocks * kSpecOpsCap * sizeof(uint32_t)));
        HIP_TRY(p->own.alloc(&p->d_spec_done, n_pairs * sizeof(uint32_t)));
        HIP_TRY(hipMemset(p->d_spec_done, 0, n_pairs * sizeof(uint32_t)));
    }
    *out = p.release();
    return SALN_OK;
}

extern "C" {

int saln_nw_plan_info(const saln_nw_plan *p, uint64_t *mask_bytes, uint64_t *cigar_words,
                      uint64_t *cells) {
    if (!p) return SALN_E_INVALID;
    if (mask_bytes) *mask_bytes = p->mask_bytes;
    if (cigar_words) *cigar_words = p->cigar_off.back();
    if (cells) *cells = p->cells;
    return SALN_OK;
}

int saln_nw_cigar_offsets(const saln_nw_plan *p, uint64_t *off) {
    if (!p || !off) return SALN_E_INVALID;
    std::memcpy(off, p->cigar_off.data(), p->cigar_off.size() * sizeof(uint64_t));
    return SALN_OK;
}

int saln_nw_plan_set_timing(saln_nw_plan *p, int enable) {
    if (!p) return SALN_E_INVALID;
    HIP_TRY(hipSetDevice(p->ctx->device));
    if (p->ev_used || p->stamps.used) {
        const int rc = p->resolve_events();
        if (rc != SALN_OK) return rc;
    }
    p->timing = enable != 0;
    p->ktime.clear();
    // a plan whose kernels all take stamps (whatever its modes are now): the
    // pool's first block, zeroed here, outside any timed region
    if (p->timing && !p->stamps.blocks &&
        stamps_supported(p->var_count, true, false, p->opts[Opt::TimingMode])) {
        int khz = 0;
        HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, p->ctx->device));
        if (khz <= 0) {
            set_error("saln_nw_plan_set_timing: the device reports no wall clock rate");
            return SALN_E_HIP;
        }
        p->clock_khz = khz;
        HIP_TRY(p->stamp_grow(nullptr));
    }
    // the event sets of the next executes, created now rather than inside
    // them (a timed C2 step that created its four events ran 0.5 % slower,
    // round 6, profiles/r06_timing_events_ab.jsonl); more are made on demand
    constexpr size_t kEventSets = 64;
    while (p->timing && p->ev_pool.size() < kEventSets) {
        std::array<hipEvent_t, 4> e4{};
        for (auto &e : e4) HIP_TRY(p->own.event(&e));
        p->ev_pool.push_back(e4);
    }
    return SALN_OK;
}

int saln_nw_plan_kernel_time(const saln_nw_plan *p, const char *kernel, double *total_ms,
                             uint64_t *launches) {
    if (!p || !kernel) return SALN_E_INVALID;
    const int rc = const_cast<saln_nw_plan *>(p)->resolve_events();
    if (rc != SALN_OK) return rc;
    auto it = p->ktime.find(kernel);
    if (total_ms) *total_ms = it == p->ktime.end() ? 0.0 : it->second.first;
    if (launches) *launches = it == p->ktime.end() ? 0 : it->second.second;
    return SALN_OK;
}

// Waves of an LDS walk launch (nw.walk_waves; -1 auto).  Beside the next
// step's fill (async plans) every lane walks two pairs in turn: half the
// walker waves take SIMD slots from the fill, and the walk still ends inside
// it (round 5, profiles/r05_walk_waves_ab.jsonl: C2 step 0.853-0.861 ->
// 0.836-0.846 ms at 768 waves; 512 made the walk outlast the fill, 0.97 ms).
// Alone, a lane per pair (the shortest walk).
static uint32_t walk_waves(int64_t opt, uint32_t n, bool beside_fill) {
    if (opt >= 0) return (uint32_t)opt;
    return beside_fill ? (n + 127) / 128 : 0;
}

int saln_nw_execute(saln_nw_plan *p, const uint8_t *d_q, const uint8_t *d_db,
                    saln_nw_result *d_results, uint32_t *d_cigar, void *stream) {
    if (!p || !d_results || (!d_q && p->n_pairs) || (!d_db && p->n_pairs)) return SALN_E_INVALID;
    if (p->n_pairs == 0) return SALN_OK;
    HIP_TRY(hipSetDevice(p->ctx->device));
    hipStream_t s = resolve_stream(stream, p->ctx);
    // the traceback stream: the second one only in async plans (the walk of
    // execute n beside the fill of n+1); otherwise the same stream, so no
    // cross-stream hand-off sits between the fill and the walk
    hipStream_t t = p->async_tb ? (p->tb_stream ? p->tb_stream : p->ctx->tb_stream) : s;
    const int cur = p->async_tb ? p->buf : 0;
    uint8_t *mask = cur ? p->d_mask2 : p->d_mask;
    int32_t *endh = cur ? p->d_endh2 : p->d_endh;
    uint32_t *ops = cur ? p->d_ops2 : p->d_ops;
    // this workspace may still be read by the traceback of execute n-2
    if (p->tb_pending[cur]) HIP_TRY(hipStreamWaitEvent(s, p->tb_done(cur), 0));
    // boundary columns preset to kColEmpty: a row is published once its value
    // replaces the preset (nw_fill_rows_kernel).  Issued ahead of the timing
    // events, so "nw_fill" times the fill kernels alone.
    {
        const uint32_t a = p->var_first[kStripeVariant];
        const uint32_t b = a + p->var_count[kStripeVariant];
        if (a < b && p->work_first[b] > p->work_first[a]) {
            const NwPairDesc &la = p->h_pairs[b - 1];
            const uint64_t c0 = p->h_pairs[a].scratch_off;
            const uint64_t c1 = la.scratch_off + (uint64_t)p->stripe_sub *
                                                     variant_geom(kStripeVariant).n_chunks(la.len_q) *
                                                     scratch_col(la.len_db);
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p->d_scratch + c0), (int)0x80000000u,
                                      2 * (c1 - c0), s));
        }
    }
    // timed: a stamp slot where every kernel of this execute takes one (no
    // event, no packet of its own on either stream), else four timing events
    hipEvent_t *ev = nullptr;
    unsigned long long *stamp = nullptr;
    if (p->timing && p->stamped()) {
        // the pool's next block, zeroed on `s` ahead of the fills that stamp
        // it: once per kStampChunk executes
        if (p->stamps.full()) HIP_TRY(p->stamp_grow(s));
        const StampBook::Slot sl = p->stamps.take();
        stamp = p->stamp_blocks[sl.block] + sl.word;
    } else if (p->timing) {
        if (p->ev_used == p->ev_pool.size()) {
            std::array<hipEvent_t, 4> e4{};
            for (auto &e : e4) HIP_TRY(p->own.event(&e));
            p->ev_pool.push_back(e4);
        }
        ev = p->ev_pool[p->ev_used++].data();
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    // fills on `s`, then the walks on `t` (async: beside the next fill)
    FillExtras fx;
    fx.o = &p->opts;
    fx.stamp = stamp;
    // async: the table fills' fallback launches go to the walk stream, behind
    // the hand-off, so nothing but the hand-off's packets sits between this
    // fill and the next one on `s` (each packet there left ~5 us idle, rocprof
    // kernel trace, round 5)
    std::vector<std::function<hipError_t(hipStream_t)>> fallbacks;
    if (t != s) fx.deferred = &fallbacks;
    for (int v = 0; v < kNumVariants; ++v) {
        const uint32_t a = p->var_first[v], b = a + p->var_count[v];
        if (a >= b) continue;
        if (v == kStripeVariant) {
            const uint32_t w0 = p->work_first[a], w1 = p->work_first[b];
            if (w1 > w0)
                HIP_TRY(launch_fill_stripes(p->d_pairs, p->d_work + w0, w1 - w0, d_q, d_db, mask,
                                            p->d_scratch, p->d_prog, p->d_err, endh, p->sc,
                                            p->fill_codes(v),
                                            p->stripe_layout(), p->stripe_rows, s, p->opts,
                                            ++p->fill_epoch));
            continue;
        }
        fx.epoch = ++p->epoch;
        // one bail word per variant: two table fills queued before either
        // deferred fallback runs must not overwrite each other's epoch
        fx.bail = p->d_bail[cur] ? p->d_bail[cur] + v : nullptr;
        HIP_TRY(launch_fill(v, p->d_pairs, a, b - a, d_q, d_db, mask, p->d_scratch, endh, p->sc,
                            p->fill_codes(v), p->var_maxld[v], s, fx));
    }
    // the fill's end (timed with events: ev[1] doubles as the hand-off;
    // stamped or untimed: the one record without timing)
    hipEvent_t filled = ev ? ev[1] : p->sync_ev[0];
    HIP_TRY(hipEventRecord(filled, s));
    if (t != s) HIP_TRY(hipStreamWaitEvent(t, filled, 0));
    for (auto &fb : fallbacks) HIP_TRY(fb(t));
    // (async plans: the deferred fallback launches sit between ev[1] and
    // ev[2], so neither "nw_fill" nor "nw_traceback" counts them; they run
    // only for waves whose pairs hold a byte other than A, C, G, T.  Stamped
    // executes agree: the fallback kernel takes no stamp)
    if (ev) HIP_TRY(hipEventRecord(ev[2], t));
    unsigned long long *const walk_stamp = stamp ? stamp + 2 : nullptr;
    for (int v = 0; v < kNumVariants; ++v) {
        const uint32_t a = p->var_first[v], b = a + p->var_count[v];
        if (a >= b) continue;
        const bool spec = v == kStripeVariant && p->spec_pairs && !p->score_only;
        if (spec)
            HIP_TRY(launch_traceback_spec(
                p->d_pairs,
                SpecArgs{p->d_spec_blocks, p->d_spec_pairs, p->d_spec_stripes, p->d_spec_ops,
                         p->d_spec_done, 0},
                p->spec_blocks, p->spec_pairs, p->d_spec_done, p->spec_passes, d_q, d_db, mask,
                endh, d_results, d_cigar, p->sc, p->stripe_layout(),
                p->spec_strict ? p->d_err : nullptr, t));
        if (p->score_only)
            HIP_TRY(launch_score_results(p->d_pairs, a, b - a, endh, d_results, p->sc, t));
        else
            HIP_TRY(launch_traceback(v, p->d_pairs, a, b - a, d_q, d_db, mask, endh, ops,
                                     d_results, d_cigar, p->sc, p->stripe_layout(), t,
                                     spec ? p->d_spec_done : nullptr, p->nib[v],
                                     walk_waves(p->opts[Opt::WalkWaves], b - a, t != s), walk_stamp));
    }
    // pairs with an empty side (boundary-only walk) ride on the traceback stream
    if (p->n_pairs > p->n_fill && p->score_only)
        HIP_TRY(launch_score_results(p->d_pairs, p->n_fill, (uint32_t)(p->n_pairs - p->n_fill),
                                     endh, d_results, p->sc, t));
    else if (p->n_pairs > p->n_fill)
        HIP_TRY(launch_traceback(-1, p->d_pairs, p->n_fill, (uint32_t)(p->n_pairs - p->n_fill),
                                 d_q, d_db, mask, endh, ops, d_results, d_cigar, p->sc,
                                 p->stripe_layout(), t, nullptr, false, 0, walk_stamp));
    if (ev) HIP_TRY(hipEventRecord(ev[3], t));
    HIP_TRY(hipEventRecord(p->tb_done(cur), t));
    p->tb_pending[cur] = true;
    p->unchecked[cur] = true;
    p->last_buf = cur;
    if (p->async_tb) {
        p->buf ^= 1;  // results complete once saln_nw_plan_sync'ed
    } else {
        if (t != s) HIP_TRY(hipStreamWaitEvent(s, p->tb_done(cur), 0));
        p->tb_pending[cur] = false;
    }
    return SALN_OK;
}

int saln_nw_plan_pair_path(const saln_nw_plan *p, uint64_t pair, saln_nw_pair_path *out) {
    if (!p || !out || pair >= p->n_pairs) return SALN_E_INVALID;
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair]];
    *out = saln_nw_pair_path{-1, 0, 0, 0, 0, 0};
    if (!d.len_q || !d.len_db) return SALN_OK;
    const int v = (int)d.variant;
    out->variant = v;
    if (v == kStripeVariant) {
        out->stripe_pk = p->stripe_pk;
        out->packed = p->stripe_pk;
        out->rows_k = p->stripe_rows;
        return SALN_OK;
    }
    const FillPath fp = fill_path(v, p->fill_codes(v), p->var_maxld[v], p->sc, p->opts, p->has_bail());
    out->packed = fp.packed;
    out->rebase = fp.rebase;
    out->table = fp.table;
    return SALN_OK;
}

int saln_nw_plan_set_score_only(saln_nw_plan *p, int enable) {
    if (!p) return SALN_E_INVALID;
    p->score_only = enable != 0;
    return SALN_OK;
}

int saln_nw_plan_set_async(saln_nw_plan *p, int enable) {
    if (!p) return SALN_E_INVALID;
    HIP_TRY(hipSetDevice(p->ctx->device));
    if (enable && !p->d_mask2 && p->mask_bytes) {
        HIP_TRY(p->own.alloc(&p->d_mask2, p->mask_bytes + 64));
        HIP_TRY(p->own.alloc(&p->d_endh2, p->n_pairs * sizeof(int32_t)));
        if (p->ops_words) HIP_TRY(p->own.alloc(&p->d_ops2, p->ops_words * sizeof(uint32_t)));
        if (p->d_bail[0]) {
            HIP_TRY(p->own.alloc(&p->d_bail[1], kBailBytes));
            HIP_TRY(hipMemset(p->d_bail[1], 0, kBailBytes));
        }
    }
    p->async_tb = enable != 0;
    p->buf = 0;
    return SALN_OK;
}

int saln_nw_plan_set_tb_stream(saln_nw_plan *p, void *stream) {
    if (!p) return SALN_E_INVALID;
    p->tb_stream = (hipStream_t)stream;
    return SALN_OK;
}

int saln_nw_plan_status(saln_nw_plan *p, uint32_t *flags) {
    if (flags) *flags = 0;
    if (!p) return SALN_E_INVALID;
    HIP_TRY(hipSetDevice(p->ctx->device));
    for (int b = 0; b < 2; ++b)
        if (p->unchecked[b]) HIP_TRY(hipEventSynchronize(p->tb_done(b)));
    p->unchecked[0] = p->unchecked[1] = false;
    uint32_t v = 0;
    if (p->d_err) {
        HIP_TRY(hipMemcpy(&v, p->d_err, sizeof v, hipMemcpyDeviceToHost));
        if (v) HIP_TRY(hipMemset(p->d_err, 0, sizeof v));  // read and clear
    }
    if (flags) *flags = v;
    if (v & SALN_FLAG_WAIT_TIMEOUT) {
        set_error("column-stripe dependency wait timed out (results of the executes since the "
                  "last status are invalid)");
        return SALN_E_DEVICE_WAIT;
    }
    if (v & SALN_FLAG_SPEC_UNLINKED) {
        set_error("speculative stripe walk did not link (SALN_SPEC_STRICT=1)");
        return SALN_E_DEVICE_WAIT;
    }
    return SALN_OK;
}

int saln_nw_plan_set_wait_limit(saln_nw_plan *p, uint32_t polls) {
    if (!p) return SALN_E_INVALID;
    HIP_TRY(hipSetDevice(p->ctx->device));
    p->wait_limit = polls;
    if (p->d_err) HIP_TRY(hipMemcpy(p->d_err + 1, &polls, sizeof polls, hipMemcpyHostToDevice));
    return SALN_OK;
}

int saln_nw_plan_sync(saln_nw_plan *p, void *stream, int keep_latest) {
    if (!p) return SALN_E_INVALID;
    HIP_TRY(hipSetDevice(p->ctx->device));
    hipStream_t s = resolve_stream(stream, p->ctx);
    for (int b = 0; b < 2; ++b) {
        if (!p->tb_pending[b] || (keep_latest && b == p->last_buf)) continue;
        HIP_TRY(hipStreamWaitEvent(s, p->tb_done(b), 0));
        p->tb_pending[b] = false;
    }
    return SALN_OK;
}

}  // extern "C"

int saln_nw_plan::resolve_events() {
    HIP_TRY(hipSetDevice(ctx->device));
    for (size_t k = 0; k < ev_used; ++k) {
        hipEvent_t *ev = ev_pool[k].data();
        HIP_TRY(hipEventSynchronize(ev[3]));
        float a = 0, b = 0, c = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));  // fill span on the caller's stream
        HIP_TRY(hipEventElapsedTime(&b, ev[2], ev[3]));  // traceback span on its stream
        HIP_TRY(hipEventElapsedTime(&c, ev[0], ev[3]));  // whole execute
        auto &f = ktime["nw_fill"];
        f.first += a;
        f.second += 1;
        auto &t = ktime["nw_traceback"];
        t.first += b;
        t.second += 1;
        auto &x = ktime["nw_execute"];
        x.first += c;
        x.second += 1;
    }
    ev_used = 0;
    if (!stamps.used) return SALN_OK;
    // stamped executes: after the last one's walk, the used slots of each
    // block (one block unless more than kStampChunk executes are pending) are
    // read back and zeroed for their next use
    HIP_TRY(hipEventSynchronize(tb_done(last_buf)));
    std::vector<uint64_t> w((size_t)stamps.used * kStampWords);
    size_t at = 0;
    for (uint32_t b = 0; b < stamps.blocks; ++b) {
        const size_t nb = (size_t)stamps.used_in(b) * kStampWords * sizeof(uint64_t);
        if (!nb) break;
        HIP_TRY(hipMemcpy(w.data() + at, stamp_blocks[b], nb, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(stamp_blocks[b], 0, nb));
        at += nb / sizeof(uint64_t);
    }
    // (the memsets ran on the null stream, which the plan's streams do not
    // wait for: done before the next execute can stamp)
    HIP_TRY(hipStreamSynchronize(nullptr));
    StampTotals tot;
    stamp_accumulate(w.data(), stamps.used, clock_khz, &tot);
    stamps.reset();
    const std::pair<const char *, const StampTotals::Sum *> names[] = {
        {"nw_fill", &tot.fill},         {"nw_traceback", &tot.walk}, {"nw_execute", &tot.execute},
        {"nw_fill_gap", &tot.fill_gap}, {"nw_handoff", &tot.handoff}};
    for (const auto &nm : names) {
        if (!nm.second->n) continue;
        auto &k = ktime[nm.first];
        k.first += nm.second->ms;
        k.second += nm.second->n;
    }
    return SALN_OK;
}

hipError_t saln_nw_plan::stamp_grow(hipStream_t s) {
    constexpr size_t nb = (size_t)kStampChunk * kStampWords * sizeof(unsigned long long);
    unsigned long long *b = nullptr;
    hipError_t e = own.alloc(&b, nb);
    if (e != hipSuccess) return e;
    if (s) {
        e = hipMemsetAsync(b, 0, nb, s);
    } else {  // the null stream's memset, finished before any stream of the plan may stamp
        e = hipMemset(b, 0, nb);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) return e;
    stamp_blocks.push_back(b);
    stamps.grew();
    return hipSuccess;
}

// ----------------------------------------------------------- host traceback
namespace saln {

int plan_pair_mask(const saln_nw_plan *p, uint64_t pair_id, PairMask *pm) {
    if (!p || pair_id >= p->n_pairs) return SALN_E_INVALID;
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair_id]];
    if (!p->full_codes) {  // every fill stores walk codes unless the plan asks for all parents
        set_error("plan_pair_mask: plan stores walk codes only");
        return SALN_E_INVALID;
    }
    pm->g = variant_geom((int)d.variant);
    pm->m.clear();
    pm->rs = 0;
    pm->bs = pm->g.LB();
    if (d.len_q == 0 || d.len_db == 0) return SALN_OK;
    if (d.variant == (uint32_t)kStripeVariant) {  // skewed stripe regions: copied whole
        pm->rs = d.mask_rs;
        pm->bs = d.mask_bs;
        pm->cs = d.mask_cs;
        pm->m.resize(pm->g.n_chunks(d.len_q) * d.mask_cs);
        HIP_TRY(hipSetDevice(p->ctx->device));
        HIP_TRY(hipMemcpy(pm->m.data(), p->d_mask + d.mask_off, pm->m.size(), hipMemcpyDeviceToHost));
        return SALN_OK;
    }
    const uint64_t lb = pm->g.LB();
    // every row holds rs / bs blocks (the pack's width); copy them all as
    // LB-byte rows of one bs-pitched 2-D region
    const uint64_t nb = d.mask_rs / d.mask_bs;
    pm->rs = nb * lb;
    pm->cs = (uint64_t)pm->g.G * lb;
    pm->m.resize((uint64_t)d.len_db * nb * lb);
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(hipMemcpy2D(pm->m.data(), lb, p->d_mask + d.mask_off, d.mask_bs, lb,
                        (uint64_t)d.len_db * nb, hipMemcpyDeviceToHost));
    return SALN_OK;
}

int plan_next_event(saln_nw_plan *p, const saln_nw_result *d_results, uint8_t *d_next,
                    hipStream_t stream) {
    if (!p || !d_results || !d_next) return SALN_E_INVALID;
    if (!p->full_codes) {
        set_error("plan_next_event: plan stores walk codes only");
        return SALN_E_INVALID;
    }
    if (!p->n_pairs) return SALN_OK;
    HIP_TRY(hipSetDevice(p->ctx->device));
    HIP_TRY(launch_next_event(p->d_pairs, (uint32_t)p->n_pairs, p->d_mask, d_results, p->sc,
                              d_next, stream));
    return SALN_OK;
}

int plan_mask_source(const saln_nw_plan *p, const uint8_t **d_mask) {
    if (!p || !d_mask) return SALN_E_INVALID;
    if (!p->full_codes) {
        set_error("plan_mask_source: plan stores walk codes only");
        return SALN_E_INVALID;
    }
    *d_mask = p->d_mask;
    return SALN_OK;
}

// one past the largest offset of the pair's cells in every layout
// (nw_common.hpp Geom::cell): its end cell
uint64_t plan_mask_end(const saln_nw_plan *p, uint64_t pair_id) {
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair_id]];
    if (d.len_q == 0 || d.len_db == 0) return 0;
    const Geom g = variant_geom((int)d.variant);
    return d.mask_off + g.cell(d.len_db, d.len_q, d.mask_rs, d.mask_bs, d.mask_cs) + 1;
}

HostMask plan_host_mask(const saln_nw_plan *p, const uint8_t *host, uint64_t pair_id) {
    const NwPairDesc &d = p->h_pairs[p->plan_index[pair_id]];
    HostMask hm;
    hm.m = host + d.mask_off;
    hm.g = variant_geom((int)d.variant);
    hm.rs = d.mask_rs;
    hm.bs = d.mask_bs;
    hm.cs = d.mask_cs;
    hm.lq = d.len_q;
    hm.ld = d.len_db;
    hm.sc = p->sc;
    return hm;
}

void HostMask::to_dense(uint8_t *out) const {
    const uint64_t W = (uint64_t)lq + 1;
    for (uint32_t i = 0; i <= ld; ++i) {
        for (uint32_t j = 0; j <= lq; ++j) {
            uint8_t b = argmax(i, j);
            if (i >= 1 && j >= 1) b |= (uint8_t)(ibits(i, j) << 3 | dbits(i, j) << 5);
            if (i == 0 && j >= 1) b |= kDExt;  // D[0][j] <- D[0][j-1], :196
            if (j == 0 && i >= 1) b |= kIExt;  // I[i][0] <- I[i-1][0], :208
            out[(uint64_t)i * W + j] = b;
        }
    }
}

namespace {
enum { ST_M = 0, ST_I = 1, ST_D = 2 };

// Parents of a node in the reference's push order (DFS visits them reversed).
int parents(const HostMask &hm, int st, uint32_t i, uint32_t j, int *ps, uint32_t *pi,
            uint32_t *pj) {
    int n = 0;
    if (i == 0 || j == 0) {  // boundary nodes, :172-216
        if (st == ST_D && i == 0 && j >= 1) { ps[0] = ST_D; pi[0] = 0; pj[0] = j - 1; return 1; }
        if (st == ST_I && j == 0 && i >= 1) { ps[0] = ST_I; pi[0] = i - 1; pj[0] = 0; return 1; }
        return 0;
    }
    if (st == ST_M) {
        const uint8_t a = hm.argmax(i - 1, j - 1);
        if (a & kArgM) { ps[n] = ST_M; pi[n] = i - 1; pj[n] = j - 1; ++n; }
        if (a & kArgI) { ps[n] = ST_I; pi[n] = i - 1; pj[n] = j - 1; ++n; }
        if (a & kArgD) { ps[n] = ST_D; pi[n] = i - 1; pj[n] = j - 1; ++n; }
    } else if (st == ST_I) {
        const uint8_t b = hm.ibits(i, j);
        if (b & 1) { ps[n] = ST_I; pi[n] = i; pj[n] = j - 1; ++n; }
        if (b & 2) { ps[n] = ST_M; pi[n] = i; pj[n] = j - 1; ++n; }
    } else {
        const uint8_t b = hm.dbits(i, j);
        if (b & 1) { ps[n] = ST_D; pi[n] = i - 1; pj[n] = j; ++n; }
        if (b & 2) { ps[n] = ST_M; pi[n] = i - 1; pj[n] = j; ++n; }
    }
    return n;
}

// Panics when a node with parents is expanded at x == 0 (M, D) or y == 0 (M, I).
bool panics(int st, uint32_t i, uint32_t j, int np) {
    if (np == 0) return false;
    if (st == ST_M) return i == 0 || j == 0;
    if (st == ST_D) return i == 0;
    return j == 0;
}

struct Node {
    int st;
    uint32_t i, j;
};

// end states in DFS pop order: D, M, I (pushed I, M, D at :251-280)
int end_nodes(const HostMask &hm, Node *out) {
    const uint8_t a = hm.argmax(hm.ld, hm.lq);
    int n = 0;
    if (a & kArgD) out[n++] = {ST_D, hm.ld, hm.lq};
    if (a & kArgM) out[n++] = {ST_M, hm.ld, hm.lq};
    if (a & kArgI) out[n++] = {ST_I, hm.ld, hm.lq};
    return n;
}

char col_q(int st, const uint8_t *q, uint32_t j) { return st == ST_D ? '-' : (char)q[j - 1]; }
char col_d(int st, const uint8_t *d, uint32_t i) { return st == ST_I ? '-' : (char)d[i - 1]; }
}  // namespace

DfsOutcome render_blocks(const HostMask &hm, const uint8_t *q, const uint8_t *d,
                         uint64_t max_blocks, std::string *out) {
    DfsOutcome res;
    const uint32_t lq = hm.lq, ld = hm.ld;
    // Every mask layout is row-separable: cell(i, j) = (i-1) RS + co[j] (the
    // packed stripes' skew included, RS = 256), so a node's code byte is a
    // row pointer and a column offset from two tables instead of
    // Geom::cell's divisions.
    std::vector<uint64_t> co(lq + 1, 0);
    for (uint32_t j = 1; j <= lq && ld; ++j) co[j] = hm.g.cell(1, j, hm.rs, hm.bs, hm.cs);
    const uint64_t RS = hm.bs == 0 ? 256 : hm.rs;
    std::vector<const uint8_t *> rowp(ld + 1, nullptr);
    for (uint32_t i = 1; i <= ld && lq; ++i) rowp[i] = hm.m + (uint64_t)(i - 1) * RS;
    auto byte = [&](uint32_t i, uint32_t j) -> uint32_t { return rowp[i][co[j]] ^ 0x7Fu; };
    struct Item {
        uint32_t i, j, st, depth;
    };
    std::vector<Item> stack;
    stack.reserve(4 * ((size_t)lq + ld) + 8);
    // the path's columns stored back to front (depth k at cap - 1 - k), so a
    // block's three lines are three contiguous copies
    const uint32_t cap = lq + ld + 1;
    std::vector<char> p1(cap), p2(cap), pb(cap);
    {   // end states pushed I, M, D (:251-280): popped D, M, I
        const uint8_t a = hm.argmax(ld, lq);
        if (a & kArgI) stack.push_back({ld, lq, ST_I, 0});
        if (a & kArgM) stack.push_back({ld, lq, ST_M, 0});
        if (a & kArgD) stack.push_back({ld, lq, ST_D, 0});
    }
    while (!stack.empty()) {
        Item it = stack.back();
        stack.pop_back();
        // a node's last pushed parent is the next popped: it is followed at
        // once, without the stack, down the chain until a leaf
        for (;;) {
            const uint32_t i = it.i, j = it.j, st = it.st, dep = it.depth;
            if (i == 0 && j == 0) {  // :283-286
                if (max_blocks && res.blocks >= max_blocks) {
                    res.status = SALN_ENUM_CAP;
                    return res;
                }
                if (out) {
                    const uint32_t a = cap - dep;
                    out->append("alignment found\n\nseq1: ");
                    out->append(p1.data() + a, dep);
                    out->append("\n      ");
                    out->append(pb.data() + a, dep);
                    out->append("\nseq2: ");
                    out->append(p2.data() + a, dep);
                    out->push_back('\n');
                }
                ++res.blocks;
                break;
            }
            // parents in the reference's push order (parents() above)
            uint32_t ps[3], pi[3], pj[3];
            int np = 0;
            if (i == 0 || j == 0) {  // boundary nodes, :172-216
                if (st == ST_D && i == 0) { ps[0] = ST_D; pi[0] = 0; pj[0] = j - 1; np = 1; }
                else if (st == ST_I && j == 0) { ps[0] = ST_I; pi[0] = i - 1; pj[0] = 0; np = 1; }
            } else if (st == ST_M) {
                const uint32_t a = (i == 1 || j == 1) ? hm.argmax(i - 1, j - 1) : (byte(i - 1, j - 1) & 7u);
                if (a & kArgM) { ps[np] = ST_M; pi[np] = i - 1; pj[np] = j - 1; ++np; }
                if (a & kArgI) { ps[np] = ST_I; pi[np] = i - 1; pj[np] = j - 1; ++np; }
                if (a & kArgD) { ps[np] = ST_D; pi[np] = i - 1; pj[np] = j - 1; ++np; }
            } else if (st == ST_I) {
                const uint32_t b = j == 1 ? ibits_col1(hm.sc, i) : (byte(i, j - 1) >> 3) & 3u;
                if (b & 1) { ps[np] = ST_I; pi[np] = i; pj[np] = j - 1; ++np; }
                if (b & 2) { ps[np] = ST_M; pi[np] = i; pj[np] = j - 1; ++np; }
            } else {
                const uint32_t b = i == 1 ? dbits_row1(hm.sc, j) : (byte(i - 1, j) >> 5) & 3u;
                if (b & 1) { ps[np] = ST_D; pi[np] = i - 1; pj[np] = j; ++np; }
                if (b & 2) { ps[np] = ST_M; pi[np] = i - 1; pj[np] = j; ++np; }
            }
            if (np == 0) break;  // a sentinel-rooted dead end: dropped silently
            if (panics((int)st, i, j, np)) {
                res.status = SALN_REF_PANIC_BOUNDARY;
                return res;
            }
            const uint32_t x = cap - 1 - dep;
            const char c1 = col_q((int)st, q, j), c2 = col_d((int)st, d, i);
            p1[x] = c1;
            p2[x] = c2;
            pb[x] = c1 == c2 ? '|' : ' ';
            for (int k = 0; k < np - 1; ++k) stack.push_back({pi[k], pj[k], ps[k], dep + 1});
            it = {pi[np - 1], pj[np - 1], ps[np - 1], dep + 1};
        }
    }
    return res;
}

bool first_alignment(const HostMask &hm, const uint8_t *q, const uint8_t *d,
                     std::vector<uint32_t> *cigar) {
    // DFS in the reference order with "no event below" memoisation: the
    // first event is the origin (printed) or a panic node (nothing printed).
    auto key = [&](const Node &n) {
        return ((uint64_t)n.i * ((uint64_t)hm.lq + 1) + n.j) * 3 + (uint64_t)n.st;
    };
    std::unordered_set<uint64_t> dead;
    struct Frame {
        Node n;
        int np, next;  // next child index (counting down)
        int ps[3];
        uint32_t pi[3], pj[3];
    };
    std::vector<Frame> path;
    Node ends[3];
    const int ne = end_nodes(hm, ends);
    for (int e = 0; e < ne; ++e) {
        path.clear();
        auto enter = [&](const Node &n) -> int {  // 1 origin, 2 panic, 0 continue
            if (n.i == 0 && n.j == 0) return 1;
            Frame f;
            f.n = n;
            f.np = parents(hm, n.st, n.i, n.j, f.ps, f.pi, f.pj);
            if (panics(n.st, n.i, n.j, f.np)) return 2;
            f.next = f.np - 1;
            path.push_back(f);
            return 0;
        };
        int ev = enter(ends[e]);
        while (ev == 0 && !path.empty()) {
            Frame &f = path.back();
            bool descended = false;
            while (f.next >= 0) {
                const Node c{f.ps[f.next], f.pi[f.next], f.pj[f.next]};
                --f.next;
                if (dead.count(key(c))) continue;
                ev = enter(c);
                descended = true;
                break;
            }
            if (ev) break;
            if (!descended) {
                dead.insert(key(path.back().n));
                path.pop_back();
            }
        }
        if (ev == 2) return false;
        if (ev == 1) {
            if (cigar) {
                cigar->clear();
                // path holds the expanded nodes from the end to the origin's child
                for (size_t k = path.size(); k-- > 0;) {
                    const Node &n = path[k].n;
                    uint32_t op = n.st == ST_I ? SALN_CIGAR_I
                                  : n.st == ST_D ? SALN_CIGAR_D
                                  : (q[n.j - 1] == d[n.i - 1] ? SALN_CIGAR_EQ : SALN_CIGAR_X);
                    if (!cigar->empty() && (cigar->back() & 15u) == op)
                        cigar->back() += 16u;
                    else
                        cigar->push_back(16u | op);
                }
            }
            return true;
        }
    }
    return false;
}

}  // namespace saln

namespace saln {
int plan_check_error(saln_nw_plan *p) { return saln_nw_plan_status(p, nullptr); }
}  // namespace saln
