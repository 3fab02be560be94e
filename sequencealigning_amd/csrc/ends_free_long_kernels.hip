// The chunked fill of the ends-free engine (include/saln.h,
// saln_ends_free_long_*): pairs whose query is longer than one chunk of the
// 64 x 16 lane fill, or whose db is too long to stage in LDS.  DESIGN.md
// section 3d.  The walk and the gather are those of ends_free_kernels.hip:
// the codes keep the layout of ends_free_dev.hpp.
//
// ef_fill_long_kernel is the 64 x 16 decomposition of ef_fill_kernel (one
// pair per wave, 16 columns per lane in registers, rows skewed over the
// lanes, wave_shr:1 hand-over, plain int32).  What differs:
//  - the wave walks the query in chunks of 1,024 columns, left to right, and
//    runs every db row in each.  Lane 63 publishes (P(r, c0), I(r, c0 + 1))
//    of the next chunk's first column c0 into the wave's boundary column in
//    HBM; lane 0 of the next chunk takes them where chunk 0 takes constants.
//    The same wave writes and reads the column, a chunk apart: nothing waits
//    on another wave;
//  - the db is not staged whole: a 128-byte LDS ring holds the rows that are
//    live in the skew (t - 63 .. t at step t), refilled every 64 steps from a
//    register loaded 64 steps ahead;
//  - local's and extend's best cell: a best per chunk on strict > (rows rise
//    inside a chunk), merged into the running best on (value, row) at the
//    chunk's end, before the reduction over the lanes;
//  - overlap's end cell: the owner of column n (in the last chunk) keeps the
//    best P(r, n) as semi-global's does; every lane takes the last row's
//    candidates from Hp after each chunk's last row, merged on strict > so
//    that an earlier chunk keeps the smaller column; then local's reduction.
// The owner's merge, the reduction and the record are ends_free_fill.hpp's.
// Row 0, the row and the trackers are written out here and equal ef_row0 and
// ef_row: built from those, this kernel's step loop compiled to other code and
// measured 0.5-1.5 % slower.  Keep them equal.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"

namespace saln {

namespace {
constexpr int kLanes = 64, kCols = 16;  // the 64 x 16 class
constexpr uint32_t kRing = 128;         // db bytes of two refills
static_assert(kLanes * kCols == (int)kEfChunkCols, "a chunk is one 64 x 16 fill");
}  // namespace

// One wave per workgroup; workgroup w owns boundary slot w (slot_rows entries
// of bnd) and takes pairs from *counter until none is left.
//
// bnd is read and written in this kernel, so it is neither const nor
// __restrict__: its loads must stay ordinary vector loads behind the fence,
// not scalar or invariant ones.  One column per slot, updated in place: entry
// r - 1 (row r) is read by lane 0 before step r - 1 (the refill that loads it
// runs at most 128 steps earlier) and written by lane 63 at step r + 62, both
// by this wave in program order, so a row's old value is always consumed
// before its new one is stored.
//
// kKeep (the forward pass of the tiled replay; score
// only): bnd is the base of the pairs' replay areas and slot_rows the tile
// rows R.  Lane 63 publishes into the pair's own column c (chunk c + 1 reads
// it: no entry is overwritten), every lane stores Hp / Dn of its columns after
// each row that is a multiple of R and below ld, and the end state is stored.
// The instances without kKeep compile as before the flag (section 3e's table).
//
// kSub: s(i, j) from the substitution-matrix block `sub` (ends_free.hpp), copied
// into LDS once per workgroup.  qc holds the columns' symbols and the ring the
// db rows' symbols, translated as the refill stores them.  The instances
// without kSub compile as before the flag (section 3f's table).
template <int kMode, bool kCodes, bool kKeep = false, bool kSub = false>
__global__ __launch_bounds__(64) void ef_fill_long_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ codes,
    uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results, EfScoring sc,
    int2 *bnd, uint64_t slot_rows, uint32_t *counter, const uint8_t *__restrict__ sub) {
    constexpr int K = kCols;
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    constexpr bool kExtend = kMode == SALN_MODE_EXTEND;
    constexpr bool kEveryM = kLocal || kExtend;  // the tracker over every M (ef_row)
    __shared__ uint8_t ring[kRing];
    const uint8_t *ef_sub = ef_sub_stage<kSub>(sub);
    const int lane = (int)threadIdx.x;
    int2 *col = kKeep ? bnd : bnd + (size_t)blockIdx.x * slot_rows;
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
        if (lq == 0) {  // no column: score 0 at the origin in every mode
            if (lane == 0) ef_store_end<kCodes || kKeep>(results, end_state, p.out, 0, 0u, 0u, 0u);
            continue;
        }
        const uint32_t nchunks = (lq + kEfChunkCols - 1) / (uint32_t)kEfChunkCols;
        const uint32_t jend = lq - 1;
        // the lane and register of column lq in the last chunk
        const uint32_t l_end = jend % (uint32_t)kEfChunkCols / K, k_end = jend % K;
        // running best.  local and extend: best_j is the absolute column.
        // semi-global: the single owner restarts from row 0 in every chunk, the last counts.
        // overlap: the owner of column lq as semi-global's (strictly positive
        // cells only), and rbest / rbest_j, the best of the last row so far
        int32_t best = kEveryM || kOverlap ? 0 : o + (int32_t)lq * e;
        uint32_t best_i = 0, best_j = 0, best_st = kEveryM ? 0u : 1u;  // row 0 ends in I
        int32_t rbest = 0;
        uint32_t rbest_j = 0;
        const int T = ld ? (int)ld + kLanes - 1 : 0;  // no row: the row-0 values stand
        // kKeep: the pair's columns (colw written, col read) and checkpoint rows
        int2 *colw = nullptr, *cps = nullptr;
        uint32_t keep_mask = 0;
        if constexpr (kKeep) {
            const EfReplayLayout lay = ef_replay_layout(lq, ld, slot_rows);
            colw = bnd + (p.code_off + lay.cols) / 8;
            cps = bnd + (p.code_off + lay.cps) / 8;
            keep_mask = (uint32_t)slot_rows - 1;
        }
        for (uint32_t c = 0; c < nchunks; ++c) {
            if constexpr (kKeep) {
                col = colw;  // column c - 1, what the chunk before wrote
                if (c > 0) colw += ld;
            }
            const uint32_t col0 = c * (uint32_t)kEfChunkCols + (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
            const bool publish = lane == kLanes - 1 && c + 1 < nchunks;
            uint32_t qc[K];
            int32_t Hp[K], Dn[K];  // P(r-1, j) and D(r, j) of my columns
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint32_t j = col0 + k + 1;
                if constexpr (kSub)
                    qc[k] = j <= lq ? ef_sub_code(ef_sub, q[j - 1]) : kEfSubPad;
                else
                    qc[k] = j <= lq ? (uint32_t)q[j - 1] : 0x100u;  // pad columns match nothing
                // extend's row 0 is semi-global's
                Hp[k] = kLocal || kOverlap ? 0 : j <= lq ? o + (int32_t)j * e : kEfNeg;
                Dn[k] = kOverlap ? o + e : kEfNeg;  // overlap: D(1, j) opens from M(0, j) = 0
            }
            // P(0, col0), by the absolute column: also lane 0 of a chunk c > 0
            int32_t hd = kLocal || kOverlap || col0 == 0 ? 0 : col0 <= lq ? o + (int32_t)col0 * e : kEfNeg;
            int32_t pubF = kEfNeg, pubH = kEfNeg;
            // this chunk's best of my columns, as ef_fill_kernel keeps it: rows
            // rise inside a chunk, so strict > keeps the smallest row, then
            // the smallest column.  (Local pad columns need no mask: a pad
            // cell's M lies strictly below some real M of the pair, so it can
            // only displace a lane's value that is not the pair's best.  kSub:
            // the table's pad column is negative in every row for this.
            // Extend's, without the floor, neither: the argument at ef_row.)
            int32_t cbest = kEveryM || kOverlap ? 0 : o + (int32_t)lq * e;
            uint32_t cbest_i = 0, cbest_k = kEveryM ? 0u : 1u;  // semi-global: cbest_k is the end state
            uint8_t *crow = nullptr;
            if constexpr (kCodes) crow = codes + p.code_off + (size_t)c * (kEfChunkCols / 2) + (size_t)lane * (K / 2);
            // rows t + 64 .. t + 127 of the db and of the boundary column,
            // loaded at the refill of step t and used from step t + 64 on.
            // Rows past the db are never used: their loads repeat the last row
            uint32_t dnext = 0;
            int2 bnext = make_int2(0, 0), bcur = make_int2(0, 0);
            if (T) dnext = d[min((uint32_t)lane, ld - 1)];
            if (T && c > 0) {
                // lane 63's stores of chunk c - 1 before lane 0's loads
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                bnext = col[min((uint32_t)lane, ld - 1)];
            }
            // the query bytes have arrived: inside the loop only the refill waits for loads
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
            for (int t0 = 0; t0 < T; t0 += kLanes) {
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
                    // column c0 entering lane 0.  Chunk 0: P(i, 0) = 0 but in
                    // extend, I(i, 1) opens from M(i, 0) = 0 in semi-global and overlap
                    // and is -inf in local.  Extend: the deletion run P(r, 0) = o + r e
                    // of lane 0's row r = t + 1, and I(r, 1) = -inf.  Later chunks: what
                    // lane 63 published for row t + 1
                    int32_t bH = kExtend ? o + (t + 1) * e : 0, bF = kEveryM ? kEfNeg : o + e;
                    if (c > 0) {
                        bH = __builtin_amdgcn_readlane(bcur.x, s);
                        bF = __builtin_amdgcn_readlane(bcur.y, s);
                    }
                    const int32_t inF = ef_shr1<kLanes>(bF, pubF);  // I(r, col0+1)
                    const int32_t inH = ef_shr1<kLanes>(bH, pubH);  // P(r, col0)
                    if (r >= 1 && r <= (int)ld) {
                        int32_t F = inF;
                        int32_t Msel = kEfNeg, Isel = kEfNeg;
                        uint32_t nlo = 0, nhi = 0;
                        const int8_t *trow = nullptr;
                        if constexpr (kSub) trow = ef_sub_row(ef_sub, dch);
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            int32_t sij;
                            if constexpr (kSub)
                                sij = trow[qc[k]];
                            else
                                sij = qc[k] == dch ? sc.match : sc.mismatch;
                            const int32_t M = ef_add(hd, sij);
                            const int32_t I = F, D = Dn[k];
                            const int32_t P3 = max(M, max(I, D));
                            const int32_t P = kLocal ? max(P3, 0) : P3;
                            const int32_t tO = ef_add(M, o);
                            if constexpr (kCodes) {
                                uint32_t cd = M == P3 ? 0u : I == P3 ? 1u : 2u;
                                if constexpr (kLocal) cd = P3 <= 0 ? kEfStop : cd;
                                cd |= I >= tO ? kEfIExt : 0u;
                                cd |= D >= tO ? kEfDExt : 0u;
                                if (k < 8)
                                    nlo |= cd << (4 * k);
                                else
                                    nhi |= cd << (4 * (k - 8));
                            }
                            if constexpr (kEveryM) {
                                const bool b = M > cbest;
                                cbest = b ? M : cbest;
                                cbest_i = b ? (uint32_t)r : cbest_i;
                                cbest_k = b ? (uint32_t)k : cbest_k;
                            } else if constexpr (kOverlap) {
                                Msel = (uint32_t)k == k_end ? P3 : Msel;  // P(r, my k_end-th column)
                            } else {
                                Msel = (uint32_t)k == k_end ? M : Msel;
                                Isel = (uint32_t)k == k_end ? I : Isel;
                            }
                            F = ef_add(max(tO, I), e);      // I(r, j+1)
                            Dn[k] = ef_add(max(tO, D), e);  // D(r+1, j)
                            hd = Hp[k];
                            Hp[k] = P;
                        }
                        hd = inH;
                        pubF = F;
                        pubH = Hp[K - 1];
                        if constexpr (kKeep) {
                            if (publish) colw[r - 1] = make_int2(pubH, pubF);
                            if (((uint32_t)r & keep_mask) == 0 && (uint32_t)r < ld) {
                                int2 *cp = cps + ((size_t)((uint32_t)r / (uint32_t)slot_rows - 1) * nchunks + c) *
                                                     kEfChunkCols + (size_t)lane * K;
#pragma unroll
                                for (int k = 0; k < K; ++k) cp[k] = make_int2(Hp[k], Dn[k]);
                            }
                        } else {
                            if (publish) col[r - 1] = make_int2(pubH, pubF);
                        }
                        if constexpr (kOverlap) {
                            const bool b = Msel > cbest;  // the smallest row wins a tie
                            cbest = b ? Msel : cbest;
                            cbest_i = b ? (uint32_t)r : cbest_i;
                        } else if constexpr (!kEveryM) {
                            const int32_t v = max(Msel, Isel);
                            const bool b = v > cbest;  // the smallest row wins a tie
                            cbest = b ? v : cbest;
                            cbest_i = b ? (uint32_t)r : cbest_i;
                            cbest_k = b ? (Msel >= Isel ? 0u : 1u) : cbest_k;  // M before I
                        }
                        if constexpr (kCodes) {
                            if (col0 < lq)  // lanes wholly past the query store nothing
                                *reinterpret_cast<uint2 *>(crow + (size_t)(r - 1) * p.row_bytes) = make_uint2(nlo, nhi);
                        }
                    }
                }
            }
            if constexpr (kEveryM) {
                // a later chunk holds larger columns but starts over at row 1:
                // it wins with a larger value, or the same value in a smaller row
                const bool take = cbest > best || (cbest == best && cbest > 0 && cbest_i < best_i);
                best = take ? cbest : best;
                best_i = take ? cbest_i : best_i;
                best_j = take ? col0 + cbest_k + 1 : best_j;
            } else if constexpr (kOverlap) {
                best = cbest;  // the last chunk's counts, in the lane of column lq
                best_i = cbest_i;
                // the last row of this chunk: Hp holds P(ld, j) of my columns
                // (row 0's zeros when ld == 0), pad columns masked out.  Strict >
                // over rising columns and chunks keeps the smallest column
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint32_t j = col0 + (uint32_t)k + 1;
                    const bool b = j <= lq && Hp[k] > rbest;
                    rbest = b ? Hp[k] : rbest;
                    rbest_j = b ? j : rbest_j;
                }
            } else {
                best = cbest;
                best_i = cbest_i;
                best_st = cbest_k;
            }
        }
        const bool owner = (uint32_t)lane == l_end;  // of column lq, in the last chunk
        if constexpr (kOverlap) ef_overlap_end(owner, lq, ld, rbest, rbest_j, best, best_i, best_j);
        ef_reduce_best<kLanes, kMode, kCodes || kKeep>(lane, owner, best, best_i, best_j, best_st, lq, results, end_state,
                                              p.out);
        // the next pair reuses the boundary column and the ring
        if constexpr (!kKeep) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
}

hipError_t launch_ef_fill_long(int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                               const uint8_t *qs, const uint8_t *ds, EfScoring sc, const uint8_t *sub,
                               uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results, void *bnd,
                               uint64_t slot_rows, uint32_t slots, uint32_t *counter, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (slots == 0 || !bnd || !counter) return hipErrorInvalidValue;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(slots), dim3(kLanes), 0, s, pairs, first, count, qs, ds, codes,
                           end_state, results, sc, static_cast<int2 *>(bnd), slot_rows, counter, sub);
        return hipGetLastError();
    };
    return ef_with_mode(mode, [&](auto m) {
        return ef_with_flag(sub != nullptr, [&](auto sb) {
            constexpr int kMode = decltype(m)::value;
            constexpr bool kSub = decltype(sb)::value;
            return codes ? go(ef_fill_long_kernel<kMode, true, false, kSub>)
                         : go(ef_fill_long_kernel<kMode, false, false, kSub>);
        });
    });
}

hipError_t launch_ef_fill_keep(int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                               const uint8_t *qs, const uint8_t *ds, EfScoring sc, const uint8_t *sub,
                               uint8_t *area, uint32_t tile_rows, uint8_t *end_state,
                               saln_ends_free_result *results, uint32_t slots, uint32_t *counter,
                               hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (slots == 0 || !area || !end_state || !counter || !ef_tile_rows_ok(tile_rows))
        return hipErrorInvalidValue;
    return ef_with_mode(mode, [&](auto m) {
        return ef_with_flag(sub != nullptr, [&](auto sb) {
            hipLaunchKernelGGL((ef_fill_long_kernel<decltype(m)::value, false, true, decltype(sb)::value>),
                               dim3(slots), dim3(kLanes), 0, s, pairs, first, count, qs, ds, (uint8_t *)nullptr,
                               end_state, results, sc, reinterpret_cast<int2 *>(area), (uint64_t)tile_rows,
                               counter, sub);
            return hipGetLastError();
        });
    });
}

}  // namespace saln
