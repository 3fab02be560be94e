// The shared host support layer (host_common.hpp).
#include "host_common.hpp"

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace saln {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

hipError_t dev_alloc(saln_context *ctx, void **p, size_t n) {
    n = n ? (n + 255) & ~size_t(255) : 256;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->cache.lower_bound(n);
        if (it != ctx->cache.end() && it->first <= 2 * n) {
            *p = it->second;
            ctx->live[it->second] = it->first;
            ctx->cached -= it->first;
            ctx->cache.erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, n);
    if (e == hipErrorOutOfMemory) {  // give the cached blocks back and retry once
        (void)hipGetLastError();
        dev_cache_clear(ctx);
        e = hipMalloc(p, n);
    }
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->live[*p] = n;
    return hipSuccess;
}

void dev_free(saln_context *ctx, void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->live.find(p);
    if (it == ctx->live.end()) {
        (void)hipFree(p);
        return;
    }
    const size_t n = it->second;
    ctx->live.erase(it);
    if (ctx->cached + n > kDevCacheMax) {
        (void)hipFree(p);
        return;
    }
    ctx->cache.emplace(n, p);
    ctx->cached += n;
}

void dev_cache_clear(saln_context *ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto &kv : ctx->cache) (void)hipFree(kv.second);
    ctx->cache.clear();
    ctx->cached = 0;
}

hipError_t pinned_staging(saln_context *ctx, size_t n, void **p) {
    if (n > ctx->pinned_bytes) {
        const size_t want = std::max(n, ctx->pinned_bytes * 2);
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
        hipError_t e = hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        ctx->pinned_bytes = want;
    }
    *p = ctx->pinned;
    return hipSuccess;
}

void host_parallel(uint64_t n, uint64_t grain, uint64_t threads,
                   const std::function<void(uint64_t)> &f) {
    const uint64_t nt = std::min<uint64_t>(
        std::max(1u, std::min(16u, std::thread::hardware_concurrency())), threads);
    std::atomic<uint64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const uint64_t b = next.fetch_add(grain);
            if (b >= n) return;
            for (uint64_t k = b; k < std::min(n, b + grain); ++k) f(k);
        }
    };
    std::vector<std::thread> th;
    for (uint64_t i = 1; i < nt; ++i) th.emplace_back(work);
    work();
    for (auto &x : th) x.join();
}

hipError_t upload_seqs(DevBuf &dq, DevBuf &dd, const uint8_t *q_seq, const uint64_t *q_off,
                       uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                       size_t pad) {
    const uint64_t qb = q_off[n_q], db = db_off[n_db];
    hipError_t e;
    if ((e = dq.alloc(qb + pad)) != hipSuccess || (e = dd.alloc(db + pad)) != hipSuccess) return e;
    if (qb && (e = hipMemcpy(dq.p, q_seq, qb, hipMemcpyHostToDevice)) != hipSuccess) return e;
    return db ? hipMemcpy(dd.p, db_seq, db, hipMemcpyHostToDevice) : hipSuccess;
}

void *huge_alloc(size_t n, size_t *got) {
    constexpr size_t kHuge = size_t(2) << 20;
    *got = (n + kHuge - 1) / kHuge * kHuge;
    void *hp = nullptr;
    if (posix_memalign(&hp, kHuge, *got) != 0 || !hp) return nullptr;
    (void)madvise(hp, *got, MADV_HUGEPAGE);
    return hp;
}

}  // namespace saln

extern "C" const char *saln_last_error(void) { return saln::g_err.c_str(); }
