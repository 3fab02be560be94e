// The tiled replay traceback of the ends-free engine (include/saln.h,
// saln_ends_free_replay_*): the alignment of a pair of
// the chunked path without its n x m codes.  The forward pass
// (ef_fill_long_kernel with kKeep, ends_free_long_kernels.hip) has kept the
// pair's boundary columns and a checkpoint row every R rows.  From those,
// ef_tile_fill_kernel computes again the codes of one tile (a 1,024-column
// chunk x a block of R rows) and ef_tile_walk_kernel walks inside it; the host
// alternates the two until every pair's walk has ended (ends_free_replay_host.cpp).
//
// The tile fill is the 64 x 16 decomposition built from ends_free_fill.hpp's
// row 0 and row (it has no end-cell tracker to keep, and its step loop is not
// the chunked fill's): the same recurrences on the same integers, so its codes
// are the chunked fill's codes.  The walk's step logic is a second copy of
// ef_walk_kernel's (ends_free_kernels.hip), split where a code is read; keep
// the two equal.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"

namespace saln {

namespace {
constexpr int kLanes = 64, kCols = 16;  // the 64 x 16 class
constexpr uint32_t kRing = 128;         // db bytes of two refills
static_assert(kLanes * kCols == (int)kEfChunkCols, "a chunk is one 64 x 16 fill");
static_assert(kEfTileRowBytes == kLanes * kCols / 2, "a tile row holds a chunk's codes");
}  // namespace

// One wave per pair.  The pair's walk waits for the code of cell (i, j): this
// fills rows r0 + 1 .. i of that cell's tile, r0 = (i - 1) / R * R, all 1,024
// columns of chunk c = (j - 1) / 1024.
//   row r0         the checkpoint row (P(r0, j), D(r0 + 1, j)); row 0's formulas for r0 = 0
//   column c0      the kept column c - 1 (P(r, c0), I(r, c0 + 1)), rows r0 + 1 .. i;
//                  the chunk-0 constants for c = 0 (extend: o + (r0 + rr) e)
//   P(r0, col0)    a lane's first diagonal: the checkpoint's cell left of its
//                  columns; lane 0 takes the kept column's row r0, or column 0's
//                  P(r0, 0): 0, but extend's o + r0 e
// The db and the column come through the chunked fill's refill: 64 rows ahead
// in a register, the db's live rows in a 128-byte LDS ring.
// kSub: as the chunked fill's (the block `sub` in LDS, symbols in qc and the ring).
template <int kMode, bool kSub = false>
__global__ __launch_bounds__(64) void ef_tile_fill_kernel(
    const EfPair *__restrict__ pairs, uint32_t count, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, EfScoring sc, uint8_t *__restrict__ area, uint32_t R,
    const EfWalkState *__restrict__ state, const uint8_t *__restrict__ sub) {
    constexpr int K = kCols;
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kExtend = kMode == SALN_MODE_EXTEND;
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
    const uint32_t r0 = b * R, nrows = i - r0;  // 1 .. R rows
    const EfReplayLayout lay = ef_replay_layout(lq, ld, R);
    // column c - 1 and checkpoint row b - 1 (only read where they exist)
    const int2 *__restrict__ col =
        reinterpret_cast<const int2 *>(area + p.code_off + lay.cols) + (size_t)(c ? c - 1 : 0) * ld;
    const int2 *__restrict__ cp = reinterpret_cast<const int2 *>(area + p.code_off + lay.cps) +
                                  ((size_t)(b ? b - 1 : 0) * nchunks + c) * kEfChunkCols;
    uint8_t *__restrict__ crow = area + p.code_off + lay.tile + (size_t)lane * (K / 2);

    const uint32_t col0 = c * (uint32_t)kEfChunkCols + (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
    uint32_t qc[K];
    int32_t Hp[K], Dn[K];
    int32_t hd = ef_row0<K, kMode, kSub>(q, lq, col0, o, e, qc, Hp, Dn, ef_sub);
    if (b > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int2 v = cp[lane * K + k];
            Hp[k] = v.x;
            Dn[k] = v.y;
        }
        hd = lane > 0 ? cp[lane * K - 1].x : c > 0 ? col[r0 - 1].x : kExtend ? o + (int32_t)r0 * e : 0;
    }
    int32_t pubF = kEfNeg, pubH = kEfNeg;
    EfBest unused = ef_best_row0<kMode>(lq, o, e);  // the tile needs no end cell
    const int T = (int)nrows + kLanes - 1;
    // rows r0 + t + 64 .. r0 + t + 127 of the db and of the column, loaded at
    // the refill of step t.  Rows past the db are never used
    uint32_t dnext = d[min(r0 + (uint32_t)lane, ld - 1)];
    int2 bnext = make_int2(0, 0), bcur = make_int2(0, 0);
    if (c > 0) bnext = col[min(r0 + (uint32_t)lane, ld - 1)];
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    for (int t0 = 0; t0 < T; t0 += kLanes) {
        // one wave: its LDS accesses execute in program order
        if constexpr (kSub)
            ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)ef_sub_code(ef_sub, dnext);
        else
            ring[((uint32_t)t0 + (uint32_t)lane) & (kRing - 1)] = (uint8_t)dnext;
        bcur = bnext;
        const uint32_t inext = min(r0 + (uint32_t)t0 + kLanes + (uint32_t)lane, ld - 1);
        dnext = d[inext];
        if (c > 0) bnext = col[inext];
        __builtin_amdgcn_wave_barrier();
        const int tend = min(t0 + kLanes, T);
        for (int t = t0; t < tend; ++t) {
            const int s = t - t0;
            const int rr = t - lane + 1;  // the row inside the tile, 1 .. nrows
            const uint32_t dch = ring[(uint32_t)(t - lane) & (kRing - 1)];  // d[r0 + rr - 1]
            // column 0, as the fills have it; extend's row of lane 0 is r0 + rr = r0 + t + 1
            int32_t bH = kExtend ? o + ((int32_t)r0 + t + 1) * e : 0, bF = kLocal || kExtend ? kEfNeg : o + e;
            if (c > 0) {
                bH = __builtin_amdgcn_readlane(bcur.x, s);
                bF = __builtin_amdgcn_readlane(bcur.y, s);
            }
            const int32_t inF = ef_shr1<kLanes>(bF, pubF);  // I(r, col0+1)
            const int32_t inH = ef_shr1<kLanes>(bH, pubH);  // P(r, col0)
            if (rr >= 1 && rr <= (int)nrows) {
                EfCodes<K> row;
                ef_row<K, kMode, true, kSub>(qc, dch, inF, inH, sc, 0u, r0 + (uint32_t)rr, Hp, Dn, hd, pubF, pubH,
                                             unused, row, ef_sub);
                // lanes wholly past the query store nothing
                if (col0 < lq) ef_store_codes<K>(crow + (size_t)(rr - 1) * kEfTileRowBytes, row);
            }
        }
    }
}

// One pair per lane: ef_walk_kernel's walk, stopped wherever the code it needs
// lies outside the tile in work and taken up again by the next launch.  The
// walk reads a code after it has moved; before each read it checks the cell
// against the tile and otherwise saves what the read would decide (pend).
// kStart: the launch before the first tile.  It takes the end cell from the
// record, decides what needs no code, and stops at the first read.
// Whatever the saved state holds, i and j are clamped into the matrix and only
// fall, every word store is guarded by the area's size, and a code is read
// only inside the rows and columns the tile fill has written for this state.
template <int kMode, bool kStart>
__global__ __launch_bounds__(64) void ef_tile_walk_kernel(
    const EfPair *__restrict__ pairs, uint32_t count, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, const uint8_t *__restrict__ area, uint32_t R,
    const uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results,
    uint32_t *__restrict__ words, uint32_t *__restrict__ lens, EfWalkState *__restrict__ state) {
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    constexpr bool kExtend = kMode == SALN_MODE_EXTEND;
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= count) return;
    const EfPair p = pairs[gi];
    const uint8_t *__restrict__ q = qs + p.q_off;
    const uint8_t *__restrict__ d = ds + p.d_off;
    const uint32_t cap = p.lq + p.ld;
    uint32_t *w = words + p.cig_off;
    uint32_t i, j, st, pend, n, run, op;
    // the tile in work: rows r0 + 1 .. i_top of chunk c_tile
    uint32_t r0 = 0, i_top = 0, c_tile = 0;
    const uint8_t *tile = nullptr;
    if constexpr (kStart) {
        const saln_ends_free_result res = results[p.out];
        // the fill's end cell, kept inside the matrix whatever the record holds
        i = min((uint32_t)max(res.db_end, 0), p.ld), j = min((uint32_t)max(res.q_end, 0), p.lq);
        st = end_state[p.out] & 1u;  // 0 M, 1 I, 2 D
        n = run = op = 0;
        pend = kEfPendNone;
        if ((kLocal || kOverlap || kExtend) && res.score <= 0) i = j = 0;
        // overlap: the end state is the end cell's own code
        if (kOverlap && i > 0 && j > 0) pend = kEfPendArg;
    } else {
        const EfWalkState ws = state[gi];
        if (ws.done) return;
        i = min(ws.i, p.ld), j = min(ws.j, p.lq);
        st = min(ws.st, 2u), pend = min(ws.pend, kEfPendDExt);
        n = min(ws.n, cap), run = ws.run, op = ws.op & 15u;
        if (pend != kEfPendNone && i > 0 && j > 0) {
            // what ef_tile_fill_kernel has just filled for this state
            r0 = (i - 1) / R * R;
            i_top = i;
            c_tile = (j - 1) / (uint32_t)kEfChunkCols;
            tile = area + p.code_off + ef_replay_layout(p.lq, p.ld, R).tile;
        } else {
            pend = kEfPendNone;
        }
    }
    auto emit = [&](uint32_t o, uint32_t len) {
        if (len == 0) return;
        if (run && o == op) {
            run += len;
            return;
        }
        if (run && n < cap) w[cap - ++n] = (run << 4) | op;
        op = o;
        run = len;
    };
    bool done = false;
    for (;;) {
        if (pend != kEfPendNone) {
            // the code of (i, j), 1 <= i, 1 <= j: inside the tile, or the next launch's
            if (tile == nullptr || i <= r0 || i > i_top || (j - 1) / (uint32_t)kEfChunkCols != c_tile) break;
            const uint32_t jc = (j - 1) % (uint32_t)kEfChunkCols;
            const uint32_t code =
                (tile[(size_t)(i - 1 - r0) * kEfTileRowBytes + (jc >> 1)] >> ((jc & 1u) * 4u)) & 15u;
            if (pend == kEfPendArg) {
                const uint32_t a = code & kEfArgMask;
                if (kLocal && a == kEfStop) {
                    done = true;
                    break;
                }
                st = a;
            } else if (pend == kEfPendIExt) {
                st = code & kEfIExt ? 1u : 0u;
            } else {
                st = code & kEfDExt ? 2u : 0u;
            }
            pend = kEfPendNone;
        }
        if (j == 0) {
            if constexpr (kExtend) {
                // column 0 above the origin is one deletion run; no code is read
                emit(SALN_CIGAR_D, i);
                i = 0;
            }
            done = true;
            break;
        }
        if (i == 0) {
            // row 0.  Overlap: a free start.  Semi-global and extend: the rest
            // of the query is one insertion.  (Local never stands here.)
            if constexpr (!kOverlap) {
                if (!kLocal) emit(SALN_CIGAR_I, j);
                j = 0;
            }
            done = true;
            break;
        }
        if (st == 0) {
            emit(q[j - 1] == d[i - 1] ? SALN_CIGAR_EQ : SALN_CIGAR_X, 1);
            --i, --j;
            if (i == 0 || j == 0) {
                // local and overlap: the alignment begins on the border
                if (kLocal || kOverlap) {
                    done = true;
                    break;
                }
                st = 1;  // semi-global and extend: row 0 is I; column 0 ends the loop
                continue;
            }
            pend = kEfPendArg;
        } else if (st == 1) {
            emit(SALN_CIGAR_I, 1);
            --j;
            // column 0: I(i, 1) opens from M(i, 0)
            st = 0;
            if (j > 0) pend = kEfPendIExt;
        } else {
            emit(SALN_CIGAR_D, 1);
            --i;
            // row 0: overlap's D(1, j) opens from M(0, j)
            st = 0;
            if (i > 0) pend = kEfPendDExt;
        }
    }
    if (done) {
        if (run && n < cap) w[cap - ++n] = (run << 4) | op;
        saln_ends_free_result res = results[p.out];
        res.q_begin = (int32_t)j;
        res.db_begin = (int32_t)i;
        res.cigar_len = n;
        results[p.out] = res;
        lens[gi] = n;
        run = 0;
    }
    state[gi] = EfWalkState{i, j, st, pend, run, op, n, done ? 1u : 0u};
}

hipError_t launch_ef_replay_start(int32_t mode, const EfPair *pairs, uint32_t count,
                                  const uint8_t *qs, const uint8_t *ds, const uint8_t *end_state,
                                  saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                                  EfWalkState *state, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 grid((count + 63) / 64), block(64);
    return ef_with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL((ef_tile_walk_kernel<decltype(m)::value, true>), grid, block, 0, s, pairs, count,
                           qs, ds, (const uint8_t *)nullptr, 1u, end_state, results, words, lens, state);
        return hipGetLastError();
    });
}

hipError_t launch_ef_tile_fill(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                               const uint8_t *ds, EfScoring sc, const uint8_t *sub, uint8_t *area,
                               uint32_t tile_rows, const EfWalkState *state, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!area || !state || !ef_tile_rows_ok(tile_rows)) return hipErrorInvalidValue;
    return ef_with_mode(mode, [&](auto m) {
        return ef_with_flag(sub != nullptr, [&](auto sb) {
            hipLaunchKernelGGL((ef_tile_fill_kernel<decltype(m)::value, decltype(sb)::value>), dim3(count),
                               dim3(kLanes), 0, s, pairs, count, qs, ds, sc, area, tile_rows, state, sub);
            return hipGetLastError();
        });
    });
}

hipError_t launch_ef_tile_walk(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                               const uint8_t *ds, const uint8_t *area, uint32_t tile_rows,
                               saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                               EfWalkState *state, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!area || !state || !ef_tile_rows_ok(tile_rows)) return hipErrorInvalidValue;
    const dim3 grid((count + 63) / 64), block(64);
    return ef_with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL((ef_tile_walk_kernel<decltype(m)::value, false>), grid, block, 0, s, pairs, count,
                           qs, ds, area, tile_rows, (const uint8_t *)nullptr, results, words, lens, state);
        return hipGetLastError();
    });
}

}  // namespace saln
