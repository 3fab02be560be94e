// What every host file of the engine needs and nothing engine-specific: the
// context, error reporting, scoped device memory, pair resolution
// (pair_index.hpp), the host thread fan-out and the upload / host-buffer helpers (host_common.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>

#include "pair_index.hpp"
#include "saln_options.hpp"
#include "saln.h"

struct saln_context {
    int device = 0;
    saln::OptOverrides opts;  // saln_context_option_set (on top of the process registry)
    hipStream_t stream = nullptr;
    hipStream_t tb_stream = nullptr;  // traceback stream (pipelined NW plans)
    // Device blocks released by plans / host-path calls, kept for reuse
    // (hipMalloc + hipFree of a 3 GB mask workspace cost more than the C2
    // kernels): size -> block; `live` maps handed-out blocks to their size.
    std::mutex mu;
    std::multimap<size_t, void *> cache;
    std::unordered_map<void *, size_t> live;
    size_t cached = 0;
    // pinned host staging for the host-path downloads (grow-only); staging_mu
    // is held by a user of the buffer from its first copy to its last host
    // read (pinned_staging may free and reallocate it when it grows)
    std::mutex staging_mu;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    // pageable host copy of render batches' mask workspaces (grow-only,
    // uninitialised, 2 MB-aligned with transparent huge pages requested: the
    // first copy into 1.1 GB of 4 KB pages spent ~0.17 s in page faults; under
    // staging_mu): pinning a GB-sized buffer costs more than the copy it
    // speeds up (measured: 333 ms to pin, 234 ms to unpin 1.1 GB)
    struct HostBuf {
        uint8_t *p = nullptr;
        size_t n = 0;
        ~HostBuf() { std::free(p); }
    } host_mask;
};

// A C-ABI stream argument: NULL = the context's own (non-blocking) stream;
// hipStreamLegacy = the legacy null stream (torch's default stream), used as
// the handle 0 that every HIP call accepts; anything else as given.
inline hipStream_t resolve_stream(void *stream, const saln_context *ctx) {
    if (!stream) return ctx->stream;
    if ((hipStream_t)stream == hipStreamLegacy) return (hipStream_t)0;
    return (hipStream_t)stream;
}

namespace saln {

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            ::saln::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
            return SALN_E_HIP;                                                             \
        }                                                                                  \
    } while (0)

// option host.timing = 1: stage times of the host-side paths on stderr
struct StageClock {
    bool on;
    explicit StageClock(const Options &o) : on(o[Opt::HostTiming] != 0) {}
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char *what) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[saln host] %-16s %8.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// Context-cached device memory: a released block is reused by a later request
// of at most twice its size; at most kDevCacheMax bytes stay cached.  A block
// must not be released while kernels may still use it (plan destroy syncs).
constexpr size_t kDevCacheMax = size_t(32) << 30;
hipError_t dev_alloc(saln_context *ctx, void **p, size_t n);
void dev_free(saln_context *ctx, void *p);
void dev_cache_clear(saln_context *ctx);
hipError_t pinned_staging(saln_context *ctx, size_t n, void **p);  // caller holds ctx->staging_mu

// A scoped device block, move-only.  Built with a context it comes from the
// context's cache (dev_alloc) and goes back to it after a sync, so work that
// may still use it has finished by then: of the device, or, built with the
// one stream its users run on, of that stream alone.  Built without a context
// it is a plain hipMalloc / hipFree block.  alloc(0) gives the allocator's
// minimum.
struct DevBuf {
    saln_context *ctx = nullptr;
    void *p = nullptr;
    bool on_stream = false;
    hipStream_t stream = nullptr;
    DevBuf() = default;
    explicit DevBuf(saln_context *c) : ctx(c) {}
    DevBuf(saln_context *c, hipStream_t s) : ctx(c), on_stream(true), stream(s) {}
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {
        reset();
        ctx = o.ctx, on_stream = o.on_stream, stream = o.stream;
        p = std::exchange(o.p, nullptr);
        return *this;
    }
    ~DevBuf() { reset(); }
    // an empty block with this one's allocator and sync
    DevBuf sibling() const { return ctx && on_stream ? DevBuf(ctx, stream) : DevBuf(ctx); }
    hipError_t alloc(size_t n) {
        reset();
        return ctx ? dev_alloc(ctx, &p, n) : hipMalloc(&p, n ? n : 1);
    }
    void reset() {
        if (!p) return;
        if (ctx) {
            (void)(on_stream ? hipStreamSynchronize(stream) : hipDeviceSynchronize());
            dev_free(ctx, p);
        } else {
            (void)hipFree(p);
        }
        p = nullptr;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

// Work items [0, n) on up to `threads` host threads (the caller included, at
// most 16 and the machine's), handed out in blocks of `grain`.
void host_parallel(uint64_t n, uint64_t grain, uint64_t threads,
                   const std::function<void(uint64_t)> &f);

// Both sequence sets of a batch on the device: q_off[n_q] / db_off[n_db]
// bytes plus `pad` each, copied when non-empty.
hipError_t upload_seqs(DevBuf &dq, DevBuf &dd, const uint8_t *q_seq, const uint64_t *q_off,
                       uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                       size_t pad);

// n bytes of uninitialised host memory rounded up to whole 2 MB pages (*got),
// 2 MB-aligned, transparent huge pages requested (advisory: fewer first-touch
// faults; 4 KB pages if THP is off).  nullptr: no memory.  std::free releases it.
void *huge_alloc(size_t n, size_t *got);

}  // namespace saln
