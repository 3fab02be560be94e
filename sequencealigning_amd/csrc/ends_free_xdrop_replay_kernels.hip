// The tiled replay of the X-drop extension (include/saln.h,
// saln_ends_free_xdrop_replay_*): the alignment of a pair
// of the chunked path under X-drop without its n x m codes.
//  - ef_xdrop_fill_keep_kernel is the forward pass: ef_xdrop_fill_long_kernel's
//    frame and rules (ends_free_xdrop_long_kernels.hip has them, and
//    tests/xdrop_long_model.py is their plain model), score only, keeping in the
//    pair's own area (ef_xdrop_replay_layout) a header per chunk, the boundary
//    columns and a checkpoint row every R rows.  It is a template of its own:
//    a flag on the existing kernel would change the code of its instances.
//  - ef_xdrop_tile_fill_kernel computes again the codes of the rows of one tile
//    (a 1,024-column chunk x a block of R rows) that lie in the chunk's window,
//    from exactly the state the forward pass had above the first of them.
//  - the walk is ef_tile_walk_kernel<SALN_MODE_EXTEND, ...>
//    (ends_free_replay_kernels.hip), unchanged: it never reads a pruned cell.
// B obeys the dependencies of the recurrence, so P, D and B on the row above a
// tile and P, I and B on the column left of it give the tile's cells as the
// same integers.
//
// The invariant (section 3k): a chunk of the forward pass runs on until lane
// 63 has run row max(live, lo_c), the last chunk included.  With that every
// lane has run every row of lo_c .. z_c, so every checkpoint row inside the
// window is whole and every boundary entry of lo_c .. z_c is written.  The tile
// fill reads a checkpoint row only inside [lo_c, z_c] and a boundary entry only
// inside [lo_{c-1}, z_{c-1}], both from the headers: it never reads an entry
// that the forward pass of this pair did not write.  What lies outside is
// stale memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"

namespace saln {

namespace {
constexpr int kLanes = 64, kCols = 16;  // the 64 x 16 class
constexpr uint32_t kRing = 128;         // db bytes of two refills
static_assert(kLanes * kCols == (int)kEfChunkCols, "a chunk is one 64 x 16 fill");
static_assert(sizeof(int4) == kEfXdropBndBytes, "a boundary entry is one int4");
static_assert(kEfTileRowBytes == kLanes * kCols / 2, "a tile row holds a chunk's codes");
}  // namespace

// One wave per workgroup, pairs from *counter.  area: the base of the pairs'
// replay areas (a pair's at code_off, 16-byte aligned); R: the tile rows.
// Column c of a pair is written by lane 63 of chunk c and read by lane 0 of
// chunk c + 1, by this wave in program order behind a workgroup fence; no
// entry is overwritten.
template <bool kSub>
__global__ __launch_bounds__(64) void ef_xdrop_fill_keep_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ end_state,
    saln_ends_free_result *__restrict__ results, EfScoring sc, int4 *area, uint32_t R,
    uint32_t *counter, const uint8_t *__restrict__ sub, int32_t xdrop) {
    constexpr int K = kCols;
    constexpr int kMode = SALN_MODE_EXTEND;
    __shared__ uint8_t ring[kRing];
    const uint8_t *ef_sub = ef_sub_stage<kSub>(sub);
    const int lane = (int)threadIdx.x;
    const int32_t o = sc.open, e = sc.extend;
    const uint32_t keep_mask = R - 1;
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
            if (lane == 0) ef_store_end<true>(results, end_state, p.out, 0, 0u, 0u, 0u);
            continue;
        }
        const uint32_t nchunks = (lq + kEfChunkCols - 1) / (uint32_t)kEfChunkCols;
        int32_t best = 0;
        uint32_t best_i = 0, best_j = 0;
        const int T = ld ? (int)ld + kLanes - 1 : 0;  // no row: the row-0 values stand, and the pair has no area
        uint32_t steps = 0;
        const EfXdropReplayLayout lay = ef_xdrop_replay_layout(lq, ld, R);
        int4 *hdr = area + (p.code_off + lay.hdr) / 16;
        int4 *colw = area + (p.code_off + lay.cols) / 16;  // column c, written
        int4 *col = colw;                                  // column c - 1, read
        int4 *cps = area + (p.code_off + lay.cps) / 16;
        // what chunk c - 1 leaves for chunk c; all wave-uniform
        int lo_p = 1, z_p = 0, pf = 0;
        int32_t Bst = 0;
        uint32_t c = 0;
        for (; c < nchunks && T; ++c) {
            const uint32_t c0 = c * (uint32_t)kEfChunkCols;
            col = colw;
            if (c > 0) colw += ld;
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
            int32_t hd = ef_row0<K, kMode, kSub, true>(q, lq, col0, o, e, qc, Hp, Dn, ef_sub, xdrop);
            int32_t pubF = kEfNeg, pubH = kEfNeg;
            EfDrop<K> xd;
#pragma unroll
            for (int k = 0; k < K; ++k) xd.Bp[k] = col0 + (uint32_t)k + 1 <= lq ? Bs : kEfPadB;
            xd.pubB = Bs;
            xd.X = xdrop;
            EfBest cb{0, 0u, 0u};
            // checkpoint rows of this chunk's columns: row R (n + 1) at cp + n * cp_stride
            int4 *cp = cps + (size_t)c * kEfChunkCols + (size_t)lane * K;
            const size_t cp_stride = (size_t)nchunks * kEfChunkCols;
            uint32_t dnext = d[min((uint32_t)tb + (uint32_t)lane, ld - 1)];
            int4 bnext = make_int4(0, 0, 0, 0), bcur = make_int4(0, 0, 0, 0);
            if (c > 0) bnext = col[min((uint32_t)tb + (uint32_t)lane, ld - 1)];
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
                    // column c0 entering lane 0, row t + 1: the fill's three cases
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
                        ef_row<K, kMode, false, kSub, true>(qc, dch, inF, inH, sc, 0u, (uint32_t)r, Hp, Dn, hd,
                                                            pubF, pubH, cb, row, ef_sub, &xd);
                        if (publish && lane == kLanes - 1) colw[r - 1] = make_int4(pubH, pubF, xd.pubB, 0);
                        if (((uint32_t)r & keep_mask) == 0 && (uint32_t)r < ld) {
                            int4 *to = cp + (size_t)((uint32_t)r / R - 1) * cp_stride;
#pragma unroll
                            for (int k = 0; k < K; ++k) to[k] = make_int4(Hp[k], Dn[k], xd.Bp[k], 0);
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
                    // the drain, in every chunk: lane 63 has run row max(live,
                    // lo), so every lane has run every row of the window
                    const bool waiting = t - tb + 1 < nreal;
                    if (!bs && !waiting && t - (kLanes - 1) + 1 >= max(live, lo)) {
                        done = true;
                        break;
                    }
                }
            }
            const uint32_t ran = (uint32_t)(tlast - tb + 1);
            steps = steps + ran < steps ? 0xFFFFFFFFu : steps + ran;
            const bool take = cb.v > best || (cb.v == best && cb.v > 0 && cb.i < best_i);
            best = take ? cb.v : best;
            best_i = take ? cb.i : best_i;
            best_j = take ? col0 + cb.k + 1 : best_j;
            const int z = min((int)ld, max(live, lo));
            if (lane == 0) hdr[c] = make_int4(lo, z, Bs, 1);
            if (publish) {
                Bst = Bs;
                lo_p = lo;
                z_p = z;
                pf = npf;
            }
        }
        // the chunks that did not run
        if (T)
            for (uint32_t cc = c + (uint32_t)lane; cc < nchunks; cc += kLanes) hdr[cc] = make_int4(0, 0, 0, 0);
        ef_reduce_best<kLanes, kMode, true>(lane, false, best, best_i, best_j, 0u, lq, results, end_state, p.out,
                                            steps);
    }
}

// One wave per pair.  The pair's walk waits for the code of the unpruned cell
// (i, j) of chunk c = (j - 1) / 1024, whose header gives lo_c <= i <= z_c.  With
// r0 = (i - 1) / R * R this fills the codes of rows max(r0, lo_c - 1) + 1 .. i
// into the tile, from the state the forward pass had above the first of them:
//   r0 < lo_c    the window starts inside this tile or on its top edge: the
//                fill's own start, ef_row0 with its pruning (all -inf when
//                lo_c > 1), Bp = Bs from the header, time base lo_c - 1
//   r0 >= lo_c   checkpoint row r0: Hp, Dn and Bp from it, hd = P(r0, col0) from
//                the left lane's entry; lane 0: the kept column c - 1 at row r0
//                inside [lo_{c-1}, z_{c-1}], else -inf; chunk 0: o + r0 e, pruned
//                below -X
// The column left of the chunk follows the fill's three cases: chunk 0's closed
// form; the kept entry for a row of [lo_{c-1}, z_{c-1}]; the constants P = I =
// -inf, B = 0 past z_{c-1}.  Rows of the tile above lo_c are not written: the
// walk cannot ask for them.  A state the header does not cover (never
// expected) fills nothing.
template <bool kSub>
__global__ __launch_bounds__(64) void ef_xdrop_tile_fill_kernel(
    const EfPair *__restrict__ pairs, uint32_t count, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, EfScoring sc, uint8_t *__restrict__ area, uint32_t R,
    const EfWalkState *__restrict__ state, const uint8_t *__restrict__ sub, int32_t xdrop) {
    constexpr int K = kCols;
    constexpr int kMode = SALN_MODE_EXTEND;
    __shared__ uint8_t ring[kRing];
    const uint8_t *ef_sub = ef_sub_stage<kSub>(sub);
    const uint32_t gi = blockIdx.x;
    if (gi >= count) return;
    const EfWalkState ws = state[gi];
    if (ws.done || ws.pend == kEfPendNone) return;
    const EfPair p = pairs[gi];
    const uint32_t lq = p.lq, ld = p.ld;
    const uint32_t i = min(ws.i, ld), j = min(ws.j, lq);
    if (i == 0 || j == 0) return;  // no such cell: the walk ends the pair
    const int lane = (int)threadIdx.x;
    const uint8_t *__restrict__ q = qs + p.q_off;
    const uint8_t *__restrict__ d = ds + p.d_off;
    const int32_t o = sc.open, e = sc.extend;
    const uint32_t nchunks = (lq + (uint32_t)kEfChunkCols - 1) / (uint32_t)kEfChunkCols;
    const uint32_t c = (j - 1) / (uint32_t)kEfChunkCols, b = (i - 1) / R;
    const uint32_t r0 = b * R;
    const EfXdropReplayLayout lay = ef_xdrop_replay_layout(lq, ld, R);
    const int4 *__restrict__ hdr = reinterpret_cast<const int4 *>(area + p.code_off + lay.hdr);
    const int4 h = hdr[c];
    const int lo = h.x, z = h.y;
    const int32_t Bs = h.z;
    if (h.w != 1 || lo < 1 || (int)i < lo || (int)i > z) return;
    // the rows chunk c - 1 kept in its column
    int lo_p = 1, z_p = 0;
    if (c > 0) {
        const int4 hp = hdr[c - 1];
        if (hp.w == 1) lo_p = max(hp.x, 1), z_p = min(hp.y, (int)ld);
    }
    const int4 *__restrict__ col =
        reinterpret_cast<const int4 *>(area + p.code_off + lay.cols) + (size_t)(c ? c - 1 : 0) * ld;
    const int4 *__restrict__ cp = reinterpret_cast<const int4 *>(area + p.code_off + lay.cps) +
                                  ((size_t)(b ? b - 1 : 0) * nchunks + c) * kEfChunkCols;
    uint8_t *__restrict__ crow = area + p.code_off + lay.tile + (size_t)lane * (K / 2);

    const bool top = (int)r0 < lo;                    // no checkpoint row: the window's own start
    const uint32_t rs = top ? (uint32_t)lo - 1 : r0;  // the row above the first row filled; the time base
    const uint32_t nrows = i - rs;                    // 1 .. R rows
    const uint32_t col0 = c * (uint32_t)kEfChunkCols + (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
    uint32_t qc[K];
    int32_t Hp[K], Dn[K];
    int32_t hd = ef_row0<K, kMode, kSub, true>(q, lq, col0, o, e, qc, Hp, Dn, ef_sub, xdrop);
    EfDrop<K> xd;
#pragma unroll
    for (int k = 0; k < K; ++k) xd.Bp[k] = col0 + (uint32_t)k + 1 <= lq ? Bs : kEfPadB;
    if (!top) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int4 v = cp[lane * K + k];
            Hp[k] = v.x;
            Dn[k] = v.y;
            xd.Bp[k] = v.z;
        }
        if (lane > 0) {
            hd = cp[lane * K - 1].x;
        } else if (c > 0) {
            hd = (int)r0 >= lo_p && (int)r0 <= z_p ? col[r0 - 1].x : kEfNeg;
        } else {
            const int32_t v = o + (int32_t)r0 * e;
            hd = v < -xdrop ? kEfNeg : v;
        }
    }
    xd.pubB = Bs;
    xd.X = xdrop;
    int32_t pubF = kEfNeg, pubH = kEfNeg;
    EfBest unused{0, 0u, 0u};  // the tile needs no end cell
    const int T = (int)nrows + kLanes - 1;
    // rows rs + t + 64 .. rs + t + 127 of the db and of the column, loaded at
    // the refill of step t.  Rows past the db are never used
    uint32_t dnext = d[min(rs + (uint32_t)lane, ld - 1)];
    int4 bnext = make_int4(0, 0, 0, 0), bcur = make_int4(0, 0, 0, 0);
    if (c > 0) bnext = col[min(rs + (uint32_t)lane, ld - 1)];
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    for (int t0 = 0; t0 < T; t0 += kLanes) {
        // one wave: its LDS accesses execute in program order
        if constexpr (kSub)
            ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)ef_sub_code(ef_sub, dnext);
        else
            ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)dnext;
        bcur = bnext;
        const uint32_t inext = min(rs + (uint32_t)t0 + kLanes + (uint32_t)lane, ld - 1);
        dnext = d[inext];
        if (c > 0) bnext = col[inext];
        __builtin_amdgcn_wave_barrier();
        const int tend = min(t0 + kLanes, T);
        for (int t = t0; t < tend; ++t) {
            const int s = t - t0;
            const int rr = t - lane + 1;  // the row counted from rs, 1 .. nrows
            const uint32_t dch = ring[(uint32_t)(t - lane) & (kRing - 1)];  // d[rs + rr - 1]
            // column c0 entering lane 0, row rs + t + 1
            const int r_in = (int)rs + t + 1;
            int32_t bH = kEfNeg, bF = kEfNeg, bB = 0;
            if (c == 0) {
                const int32_t v = o + r_in * e;
                bH = v < -xdrop ? kEfNeg : v;
            } else if (r_in >= lo_p && r_in <= z_p) {
                bH = __builtin_amdgcn_readlane(bcur.x, s);
                bF = __builtin_amdgcn_readlane(bcur.y, s);
                bB = __builtin_amdgcn_readlane(bcur.z, s);
            }
            const int32_t inF = ef_shr1<kLanes>(bF, pubF);  // I(r, col0+1)
            xd.inB = ef_shr1<kLanes>(bB, xd.pubB);          // B(r, col0)
            const int32_t inH = ef_shr1<kLanes>(bH, pubH);  // P(r, col0)
            if (rr >= 1 && rr <= (int)nrows) {
                const uint32_t r = rs + (uint32_t)rr;
                EfCodes<K> row;
                ef_row<K, kMode, true, kSub, true>(qc, dch, inF, inH, sc, 0u, r, Hp, Dn, hd, pubF, pubH, unused,
                                                   row, ef_sub, &xd);
                // lanes wholly past the query store nothing
                if (col0 < lq) ef_store_codes<K>(crow + (size_t)(r - 1 - r0) * kEfTileRowBytes, row);
            }
        }
    }
}

hipError_t launch_ef_xdrop_fill_keep(const EfPair *pairs, uint32_t first, uint32_t count, const uint8_t *qs,
                                     const uint8_t *ds, EfScoring sc, const uint8_t *sub, int32_t xdrop,
                                     uint8_t *area, uint32_t tile_rows, uint8_t *end_state,
                                     saln_ends_free_result *results, uint32_t slots, uint32_t *counter,
                                     hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (slots == 0 || !area || !counter || !end_state || xdrop < 0 || !ef_tile_rows_ok(tile_rows) ||
        (reinterpret_cast<uintptr_t>(area) & 15u))
        return hipErrorInvalidValue;
    return ef_with_flag(sub != nullptr, [&](auto sb) {
        hipLaunchKernelGGL((ef_xdrop_fill_keep_kernel<decltype(sb)::value>), dim3(slots), dim3(kLanes), 0, s, pairs,
                           first, count, qs, ds, end_state, results, sc, reinterpret_cast<int4 *>(area), tile_rows,
                           counter, sub, xdrop);
        return hipGetLastError();
    });
}

hipError_t launch_ef_xdrop_tile_fill(const EfPair *pairs, uint32_t count, const uint8_t *qs, const uint8_t *ds,
                                     EfScoring sc, const uint8_t *sub, int32_t xdrop, uint8_t *area,
                                     uint32_t tile_rows, const EfWalkState *state, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!area || !state || xdrop < 0 || !ef_tile_rows_ok(tile_rows)) return hipErrorInvalidValue;
    return ef_with_flag(sub != nullptr, [&](auto sb) {
        hipLaunchKernelGGL((ef_xdrop_tile_fill_kernel<decltype(sb)::value>), dim3(count), dim3(kLanes), 0, s, pairs,
                           count, qs, ds, sc, area, tile_rows, state, sub, xdrop);
        return hipGetLastError();
    });
}

}  // namespace saln
