// The chunked fill of the X-drop extension (include/saln.h,
// saln_ends_free_xdrop_long_*): ef_fill_long_kernel's
// frame for SALN_MODE_EXTEND (one pair per wave, 64 x 16 columns per chunk, the
// 128-byte db ring, wave_shr:1 hand-over, a best per chunk merged on (value,
// row), pairs from a counter) with the X-drop rule of ef_row (kXdrop) and, per
// chunk, a window of rows: chunk c runs the rows lo_c .. z_c only, a chunk
// without a live cell does not run, and the pair ends at the first such chunk.
// The kernel is a template of its own: a flag on ef_fill_long_kernel would
// change the code of its existing instances (sections 3c and 3h).
//
// The rules (section 3i has the argument; tests/xdrop_long_model.py is the
// plain model of exactly these):
//  - boundary column c0 of chunk c > 0: lane 63 of chunk c - 1 published
//    (P(r, c0), I(r, c0 + 1), B(r, c0)) for every row r it ran, 16 bytes per
//    row.  The wave carries, uniform: lo_p .. z_p, the rows chunk c - 1 ran;
//    pf, the first of them whose boundary cell is unpruned (0: none); Bst =
//    B(lo_p - 1, j) of chunk c - 1's columns, c0 among them;
//  - row 0 of chunk c is live iff its left corner is: o + c0 e >= -X.  Then
//    lo_c = 1 and Bp = 0.  Else, with a live boundary cell, lo_c = pf and Bp =
//    B(pf - 1, c0) in every column (every cell of the chunk above row pf is
//    pruned, so B runs along the rows unchanged): the published entry of row
//    pf - 1, or Bst when pf = lo_p.  Else the pair ends: chunk c and every
//    later chunk are pruned throughout;
//  - the time base of the step loop, of the ring and of the boundary prefetch
//    starts at lo_c - 1: lane l runs row r = t - l + 1 at step t, from r = lo_c;
//  - rows above z_p have no entry: what the slot holds there is another
//    chunk's or another pair's, so lane 0 takes P = I = -inf for them (every
//    cell left of c0 below row z_p is pruned) and B = 0: B stands still there,
//    B(r, c0) = B(z_p, c0), and the chunk ran row r - 1 >= z_p, so B(r - 1,
//    c0 + 1) >= B(r - 1, c0) already holds it and Bin is the same;
//  - the vote, after every step: a lane is alive before its first row (if it
//    holds a real column), dead past ld, else alive iff a cell of its row or
//    the cell left of them is unpruned; lane 0 of a chunk c > 0 is also alive
//    while r <= z_p (later boundary rows may be live, and B(r, c0) still
//    grows there).  live is the largest row a lane was alive on.  The last
//    chunk leaves the loop once no lane is alive; a chunk that publishes also
//    runs on until lane 63 has run row live, so that z_c = min(ld, max(live,
//    lo_c)) is a row below which every column up to the chunk's last is
//    pruned and lane 63 has published every row up to it.
// Steps per chunk: at most (z_c - lo_c + 1) + 63 + 1; a chunk's start is not
// aligned to the refill period.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"

namespace saln {

namespace {
constexpr int kLanes = 64, kCols = 16;  // the 64 x 16 class
constexpr uint32_t kRing = 128;         // db bytes of two refills
static_assert(kLanes * kCols == (int)kEfChunkCols, "a chunk is one 64 x 16 fill");
static_assert(sizeof(int4) == kEfXdropBndBytes, "a boundary entry is one int4");
}  // namespace

// One wave per workgroup; workgroup w owns boundary slot w (slot_rows entries
// of bnd) and takes pairs from *counter until none is left.  bnd is read and
// written in this kernel (neither const nor __restrict__: ordinary vector
// loads behind the fence, ordinary vector stores).  An entry is updated in
// place as in ef_fill_long_kernel: row r's is loaded before step r - 1 and
// stored at step r + 62, by this wave in program order.
template <bool kCodes, bool kSub>
__global__ __launch_bounds__(64) void ef_xdrop_fill_long_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ codes,
    uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results, EfScoring sc,
    int4 *bnd, uint64_t slot_rows, uint32_t *counter, const uint8_t *__restrict__ sub, int32_t xdrop) {
    constexpr int K = kCols;
    constexpr int kMode = SALN_MODE_EXTEND;
    __shared__ uint8_t ring[kRing];
    const uint8_t *ef_sub = ef_sub_stage<kSub>(sub);
    const int lane = (int)threadIdx.x;
    int4 *col = bnd + (size_t)blockIdx.x * slot_rows;
    const int32_t o = sc.open, e = sc.extend;
    for (;;) {
        uint32_t gi = 0;
        if (lane == 0) gi = atomicAdd(counter, 1u);
        gi = (uint32_t)__builtin_amdgcn_readfirstlane((int)gi);
        if (gi >= count) return;
        const EfPair p = pairs[first + gi];
        const uint32_t lq = p.lq, ld = p.ld;
        const uint8_t *__restrict__ q = qs + p.q_off;
        const uint8_t *__restrict__ d = ds + p.d_off;
        if (lq == 0) {  // no column: score 0 at the origin
            if (lane == 0) ef_store_end<kCodes>(results, end_state, p.out, 0, 0u, 0u, 0u);
            continue;
        }
        const uint32_t nchunks = (lq + kEfChunkCols - 1) / (uint32_t)kEfChunkCols;
        int32_t best = 0;
        uint32_t best_i = 0, best_j = 0;
        const int T = ld ? (int)ld + kLanes - 1 : 0;  // no row: the row-0 values stand
        uint32_t steps = 0;
        // what chunk c - 1 leaves for chunk c (the header); all wave-uniform
        int lo_p = 1, z_p = 0, pf = 0;
        int32_t Bst = 0;
        for (uint32_t c = 0; c < nchunks && T; ++c) {
            const uint32_t c0 = c * (uint32_t)kEfChunkCols;
            int lo = 1;
            int32_t Bs = 0;  // B(lo - 1, j) of the chunk's columns
            if (c > 0) {
                // lane 63's stores of chunk c - 1 before the loads below
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                const bool row0 = o + (int32_t)c0 * e >= -xdrop;  // (0, c0) unpruned
                if (!row0) {
                    if (pf == 0) break;  // nothing enters the chunk: the pair ends
                    lo = pf;
                    Bs = Bst;
                    if (pf > lo_p) Bs = __builtin_amdgcn_readfirstlane(col[pf - 2].z);
                }
            }
            const int tb = lo - 1;
            const uint32_t col0 = c0 + (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
            const bool publish = c + 1 < nchunks;
            const bool real = col0 < lq;  // I hold a real column
            const int nreal = (int)min((lq - c0 + K - 1) / K, (uint32_t)kLanes);
            uint32_t qc[K];
            int32_t Hp[K], Dn[K];  // P(r-1, j) and D(r, j) of my columns
            // row 0 with its pruning; below a pruned row 0 (lo > 1) the same
            // values, all -inf, are those of row lo - 1
            int32_t hd = ef_row0<K, kMode, kSub, true>(q, lq, col0, o, e, qc, Hp, Dn, ef_sub, xdrop);
            int32_t pubF = kEfNeg, pubH = kEfNeg;
            EfDrop<K> xd;
#pragma unroll
            for (int k = 0; k < K; ++k) xd.Bp[k] = col0 + (uint32_t)k + 1 <= lq ? Bs : kEfPadB;
            xd.pubB = Bs;
            xd.X = xdrop;
            // this chunk's best of my columns: rows rise inside a chunk
            EfBest cb{0, 0u, 0u};
            uint8_t *crow = nullptr;
            if constexpr (kCodes) crow = codes + p.code_off + (size_t)c * (kEfChunkCols / 2) + (size_t)lane * (K / 2);
            // rows t + 64 .. t + 127 of the db and of the boundary column,
            // loaded at the refill of step t and used from step t + 64 on.
            // Rows past the db are never used: their loads repeat the last row
            uint32_t dnext = d[min((uint32_t)tb + (uint32_t)lane, ld - 1)];
            int4 bnext = make_int4(0, 0, 0, 0), bcur = make_int4(0, 0, 0, 0);
            if (c > 0) bnext = col[min((uint32_t)tb + (uint32_t)lane, ld - 1)];
            // the query bytes have arrived: inside the loop only the refill waits for loads
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            int live = 0, npf = 0;
            int tlast = tb;
            bool done = false;
            for (int t0 = tb; t0 < T && !done; t0 += kLanes) {
                // the refill.  One wave: its LDS accesses execute in program order
                if constexpr (kSub)
                    ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)ef_sub_code(ef_sub, dnext);
                else
                    ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)dnext;
                bcur = bnext;
                const uint32_t inext = min((uint32_t)t0 + kLanes + (uint32_t)lane, ld - 1);
                dnext = d[inext];
                if (c > 0) bnext = col[inext];
                __builtin_amdgcn_wave_barrier();
                const int tend = min(t0 + kLanes, T);
                for (int t = t0; t < tend; ++t) {
                    const int s = t - t0;
                    const int r = t - lane + 1;
                    const uint32_t dch = ring[(uint32_t)(t - lane) & (kRing - 1)];  // d[r-1]
                    // column c0 entering lane 0, row t + 1.  Chunk 0: the
                    // deletion run o + r e, pruned once below -X; I(r, 1) = -inf;
                    // B = 0.  Later chunks: lane 63's entry, and past z_p
                    // constants (the slot holds no entry of this pair there)
                    int32_t bH, bF = kEfNeg, bB = 0;
                    if (c == 0) {
                        const int32_t v = o + (t + 1) * e;
                        bH = v < -xdrop ? kEfNeg : v;
                    } else if (t + 1 <= z_p) {
                        bH = __builtin_amdgcn_readlane(bcur.x, s);
                        bF = __builtin_amdgcn_readlane(bcur.y, s);
                        bB = __builtin_amdgcn_readlane(bcur.z, s);
                    } else {
                        bH = kEfNeg;
                    }
                    const int32_t inF = ef_shr1<kLanes>(bF, pubF);  // I(r, col0+1)
                    xd.inB = ef_shr1<kLanes>(bB, xd.pubB);          // B(r, col0)
                    const int32_t inH = ef_shr1<kLanes>(bH, pubH);  // P(r, col0)
                    bool alive = false;
                    if (r >= lo && r <= (int)ld) {
                        EfCodes<K> row;
                        ef_row<K, kMode, kCodes, kSub, true>(qc, dch, inF, inH, sc, 0u, (uint32_t)r, Hp, Dn, hd,
                                                             pubF, pubH, cb, row, ef_sub, &xd);
                        if (publish && lane == kLanes - 1) col[r - 1] = make_int4(pubH, pubF, xd.pubB, 0);
                        if constexpr (kCodes) {
                            // lanes wholly past the query store nothing
                            if (real) ef_store_codes<K>(crow + (size_t)(r - 1) * p.row_bytes, row);
                        }
                        alive = xd.alive || hd != kEfNeg;  // hd: P(r, col0)
                        alive = alive || (lane == 0 && r <= z_p);
                        alive = alive && real;
                    }
                    const uint64_t bs = __ballot(alive);
                    if (bs) live = max(live, t - (int)__builtin_ctzll(bs) + 1);
                    if (publish) {
                        // lane 63's row of this step: is its boundary cell live?
                        const int r63 = t - (kLanes - 1) + 1;
                        if (r63 >= lo && r63 <= (int)ld && __builtin_amdgcn_readlane(pubH, kLanes - 1) != kEfNeg) {
                            npf = npf ? npf : r63;
                        }
                    }
                    tlast = t;
                    // lanes that have not reached row lo and hold a real column
                    const bool waiting = t - tb + 1 < nreal;
                    if (!bs && !waiting && (!publish || t - (kLanes - 1) + 1 >= live)) {
                        done = true;
                        break;
                    }
                }
            }
            const uint32_t ran = (uint32_t)(tlast - tb + 1);
            steps = steps + ran < steps ? 0xFFFFFFFFu : steps + ran;
            // a later chunk holds larger columns but starts over at row lo:
            // it wins with a larger value, or the same value in a smaller row
            const bool take = cb.v > best || (cb.v == best && cb.v > 0 && cb.i < best_i);
            best = take ? cb.v : best;
            best_i = take ? cb.i : best_i;
            best_j = take ? col0 + cb.k + 1 : best_j;
            if (publish) {
                Bst = Bs;
                lo_p = lo;
                z_p = min((int)ld, max(live, lo));
                pf = npf;
            }
        }
        ef_reduce_best<kLanes, kMode, kCodes>(lane, false, best, best_i, best_j, 0u, lq, results, end_state, p.out,
                                              steps);
        // the next pair reuses the boundary column and the ring
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

hipError_t launch_ef_xdrop_fill_long(const EfPair *pairs, uint32_t first, uint32_t count, const uint8_t *qs,
                                     const uint8_t *ds, EfScoring sc, const uint8_t *sub, int32_t xdrop,
                                     uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results,
                                     void *bnd, uint64_t slot_rows, uint32_t slots, uint32_t *counter,
                                     hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (slots == 0 || !bnd || !counter || xdrop < 0) return hipErrorInvalidValue;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(slots), dim3(kLanes), 0, s, pairs, first, count, qs, ds, codes,
                           end_state, results, sc, static_cast<int4 *>(bnd), slot_rows, counter, sub, xdrop);
        return hipGetLastError();
    };
    return ef_with_flag(sub != nullptr, [&](auto sb) {
        constexpr bool kSub = decltype(sb)::value;
        return codes ? go(ef_xdrop_fill_long_kernel<true, kSub>) : go(ef_xdrop_fill_long_kernel<false, kSub>);
    });
}

}  // namespace saln
