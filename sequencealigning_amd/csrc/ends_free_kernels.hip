// Kernels of the ends-free engine (include/saln.h, saln_ends_free_*): Gotoh
// affine-gap alignment with free ends, local (Smith-Waterman), semi-global
// (the whole query against a free db substring), overlap (dovetail: all
// four ends free, no floor) and extend (pinned at the origin, free at its
// end: the gapped extension of seed-and-extend).  NOT a reference-parity
// path: the reference only declares the first two modes.  DESIGN.md section 3 holds the recurrences,
// the tie rules and the code layout.
//
// Fill: the decomposition of the NW i32 lane fill.  One pair per group of G
// lanes, K query columns per lane in registers, the rows skewed over the
// lanes (lane l works on row t - l + 1 at step t), the left neighbour's
// boundary (P and the I candidate leaving its last column) handed over by
// DPP.  Values are plain int32.  Each lane keeps the best end cell of its own
// columns; the group reduces them at the end on (value, row, column), never
// on the step.  Row 0, a lane's row, the code store and the end cell are those
// of ends_free_fill.hpp (the chunked fill shares the end cell and keeps a row
// of its own); this kernel adds the group's db row staged in LDS, lane 0's
// boundary (column 0: constants, but extend's deletion run o + r e) and the one
// pass over the rows.  ef_xdrop_fill_kernel is extension's fill with the X-drop
// rule and a vote of the group's lanes that ends the pass early.
//
// Walk: one pair per lane, from the reported end cell along the 4-bit codes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"

namespace saln {

// kMode: SALN_MODE_LOCAL, SALN_MODE_SEMI_GLOBAL, SALN_MODE_OVERLAP or
// SALN_MODE_EXTEND.
// kSub: s(i, j) from the substitution-matrix block `sub` (ends_free.hpp), copied
// into LDS once per workgroup; the staged db row and qc then hold symbols.  The
// instances without kSub compile as before the flag.
template <int G, int K, int kMode, bool kCodes, bool kSub = false>
__global__ __launch_bounds__(256) void ef_fill_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ codes,
    uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results, EfScoring sc,
    uint32_t ld_max, const uint8_t *__restrict__ sub) {
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    constexpr bool kExtend = kMode == SALN_MODE_EXTEND;
    uint8_t *ef_sub = ef_sub_stage<kSub>(sub);  // before any thread leaves
    const int gpb = (int)blockDim.x / G;
    const int lane = (int)threadIdx.x % G, grp = (int)threadIdx.x / G;
    const uint32_t gi = blockIdx.x * (uint32_t)gpb + (uint32_t)grp;
    if (gi >= count) return;  // whole group (DPP never crosses groups)
    const EfPair p = pairs[first + gi];
    const uint32_t lq = p.lq, ld = p.ld;
    const uint8_t *__restrict__ d = ds + p.d_off;
    if (lq == 0) {  // no column: score 0 at the origin in every mode
        if (lane == 0) ef_store_end<kCodes>(results, end_state, p.out, 0, 0u, 0u, 0u);
        return;
    }
    extern __shared__ uint8_t ef_drow[];  // [groups][G + ld_max + G] db bytes
    uint8_t *myrow = ef_drow + (size_t)grp * (ld_max + 2 * G) + G;
    for (uint32_t i = (uint32_t)lane; i < ld; i += G) {
        if constexpr (kSub)
            myrow[i] = (uint8_t)ef_sub_code(ef_sub, d[i]);
        else
            myrow[i] = d[i];
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();

    const int32_t o = sc.open, e = sc.extend;
    const uint32_t col0 = (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
    const uint32_t jend = lq - 1;
    const uint32_t l_end = jend / K, k_end = jend % K;  // the lane and register of column lq
    uint32_t qc[K];
    int32_t Hp[K], Dn[K];
    int32_t hd = ef_row0<K, kMode, kSub>(qs + p.q_off, lq, col0, o, e, qc, Hp, Dn, ef_sub);
    // column 0, entering lane 0: P(i, 0) = 0 (the free start of semi-global
    // and overlap, local's floor); I(i, 1) opens from M(i, 0) = 0 in
    // semi-global and overlap and is -inf in local.  Extend: column 0 is a
    // deletion run, P(r, 0) = D(r, 0) = o + r e with r = t + 1 the row of lane 0
    // at step t (bHx below), and I(r, 1) is -inf: M(r, 0) is
    const int32_t bH = 0, bF = kLocal || kExtend ? kEfNeg : o + e;
    int32_t pubF = kEfNeg, pubH = kEfNeg;
    EfBest best = ef_best_row0<kMode>(lq, o, e);
    uint8_t *crow = nullptr;
    if constexpr (kCodes) crow = codes + p.code_off + (size_t)lane * (K / 2);
    const int T = (int)ld + G - 1;
    for (int t = 0; t < T; ++t) {
        const int r = t - lane + 1;
        const uint32_t dch = myrow[t - lane];  // d[r-1]; the pads cover rows outside the db
        const int32_t inF = ef_shr1<G>(bF, pubF);  // I(r, col0+1)
        const int32_t bHx = kExtend ? o + (t + 1) * e : bH;
        const int32_t inH = ef_shr1<G>(bHx, pubH);  // P(r, col0)
        if (r >= 1 && r <= (int)ld) {
            EfCodes<K> row;
            ef_row<K, kMode, kCodes, kSub>(qc, dch, inF, inH, sc, k_end, (uint32_t)r, Hp, Dn, hd, pubF, pubH, best,
                                           row, ef_sub);
            if constexpr (kCodes) {
                // lanes wholly past the query store nothing
                if (col0 < lq) ef_store_codes<K>(crow + (size_t)(r - 1) * p.row_bytes, row);
            }
        }
    }
    uint32_t best_j = col0 + best.k + 1;  // local's column
    if constexpr (kOverlap) {
        int32_t rbest = 0;
        uint32_t rbest_j = 0;
        ef_last_row_best<K>(Hp, col0, lq, rbest, rbest_j);
        ef_overlap_end((uint32_t)lane == l_end, lq, ld, rbest, rbest_j, best.v, best.i, best_j);
    }
    ef_reduce_best<G, kMode, kCodes>(lane, (uint32_t)lane == l_end, best.v, best.i, best_j, best.k, lq,
                                     results, end_state, p.out);
}

// The group's vote of the X-drop fill: does any of my group's G lanes hold
// `p`?  G = 16: four groups with four different pairs share the wave, so the
// wave's ballot is cut down to the group's own 16 bits; lanes of groups that
// have left the loop are inactive and ballot 0.
template <int G>
__device__ __forceinline__ bool ef_group_any(bool p) {
    const uint64_t b = __ballot(p);
    if constexpr (G == 64)
        return b != 0;
    else
        return ((b >> (threadIdx.x & 48u)) & 0xFFFFu) != 0;
}

// The X-drop extension fill (saln_ends_free_xdrop_*):
// ef_fill_kernel<G, K, SALN_MODE_EXTEND, kCodes, kSub> with the X-drop rule of
// ef_row (X = xdrop), column 0 pruned by its closed form (o + r e < -X), and a
// vote after every step: the group leaves the row loop once all its lanes are
// dead.  A lane is dead when it holds no real column, when its row is past ld,
// or when every cell of its row (pad cells always are, EfDrop) and the cell
// left of them, (r, col0), are pruned; a lane with real columns that has not
// reached row 1 is alive.
// (r, col0) belongs to the cut because the diagonal step into (r+1, col0+1)
// comes from it, and its owner, the left neighbour, is one row ahead and no
// longer votes for it.  Every path from the origin to a cell not yet computed
// crosses such a cut, so everything still to come is pruned.  The record's
// `reserved` is the number of steps run.
// The kernel keeps its own copy of ef_fill_kernel's frame: built from one
// body shared by both, every existing instance compiled to other code (other
// registers, other block order), and those instances are not to change.  A
// change to the frame above is made here too.
template <int G, int K, bool kCodes, bool kSub>
__global__ __launch_bounds__(256) void ef_xdrop_fill_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ codes,
    uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results, EfScoring sc,
    uint32_t ld_max, const uint8_t *__restrict__ sub, int32_t xdrop) {
    constexpr int kMode = SALN_MODE_EXTEND;
    uint8_t *ef_sub = ef_sub_stage<kSub>(sub);  // before any thread leaves
    const int gpb = (int)blockDim.x / G;
    const int lane = (int)threadIdx.x % G, grp = (int)threadIdx.x / G;
    const uint32_t gi = blockIdx.x * (uint32_t)gpb + (uint32_t)grp;
    if (gi >= count) return;  // whole group (DPP never crosses groups)
    const EfPair p = pairs[first + gi];
    const uint32_t lq = p.lq, ld = p.ld;
    const uint8_t *__restrict__ d = ds + p.d_off;
    if (lq == 0) {  // no column: score 0 at the origin in every mode
        if (lane == 0) ef_store_end<kCodes>(results, end_state, p.out, 0, 0u, 0u, 0u);
        return;
    }
    extern __shared__ uint8_t ef_drow[];  // [groups][G + ld_max + G] db bytes
    uint8_t *myrow = ef_drow + (size_t)grp * (ld_max + 2 * G) + G;
    for (uint32_t i = (uint32_t)lane; i < ld; i += G) {
        if constexpr (kSub)
            myrow[i] = (uint8_t)ef_sub_code(ef_sub, d[i]);
        else
            myrow[i] = d[i];
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();

    const int32_t o = sc.open, e = sc.extend;
    const uint32_t col0 = (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
    const uint32_t jend = lq - 1;
    const uint32_t l_end = jend / K, k_end = jend % K;  // the lane and register of column lq
    uint32_t qc[K];
    int32_t Hp[K], Dn[K];
    int32_t hd = ef_row0<K, kMode, kSub, true>(qs + p.q_off, lq, col0, o, e, qc, Hp, Dn, ef_sub, xdrop);
    // column 0, entering lane 0: the deletion run P(r, 0) = o + r e, r = t + 1
    // the row of lane 0 at step t, pruned once it lies below -X (bHx below);
    // I(r, 1) is -inf
    const int32_t bF = kEfNeg;
    int32_t pubF = kEfNeg, pubH = kEfNeg;
    EfBest best = ef_best_row0<kMode>(lq, o, e);
    uint8_t *crow = nullptr;
    if constexpr (kCodes) crow = codes + p.code_off + (size_t)lane * (K / 2);
    EfDrop<K> xd;
#pragma unroll
    for (int k = 0; k < K; ++k) xd.Bp[k] = col0 + (uint32_t)k + 1 <= lq ? 0 : kEfPadB;
    xd.pubB = 0;
    xd.X = xdrop;
    const bool real = col0 < lq;  // I hold a real column
    const int T = (int)ld + G - 1;
    uint32_t steps = (uint32_t)T;
    for (int t = 0; t < T; ++t) {
        const int r = t - lane + 1;
        const uint32_t dch = myrow[t - lane];  // d[r-1]; the pads cover rows outside the db
        const int32_t inF = ef_shr1<G>(bF, pubF);  // I(r, col0+1)
        const int32_t c0 = o + (t + 1) * e;
        const int32_t bHx = c0 < -xdrop ? kEfNeg : c0;
        xd.inB = ef_shr1<G>(0, xd.pubB);            // B(r, col0)
        const int32_t inH = ef_shr1<G>(bHx, pubH);  // P(r, col0)
        bool alive = r < 1;
        if (r >= 1 && r <= (int)ld) {
            EfCodes<K> row;
            ef_row<K, kMode, kCodes, kSub, true>(qc, dch, inF, inH, sc, k_end, (uint32_t)r, Hp, Dn, hd, pubF, pubH,
                                                 best, row, ef_sub, &xd);
            if constexpr (kCodes) {
                // lanes wholly past the query store nothing
                if (col0 < lq) ef_store_codes<K>(crow + (size_t)(r - 1) * p.row_bytes, row);
            }
            alive = xd.alive || hd != kEfNeg;  // hd: P(r, col0)
        }
        if (!ef_group_any<G>(alive && real)) {
            steps = (uint32_t)t + 1;
            break;
        }
    }
    ef_reduce_best<G, kMode, kCodes>(lane, (uint32_t)lane == l_end, best.v, best.i, col0 + best.k + 1, best.k, lq,
                                     results, end_state, p.out, steps);
}

// One pair per lane.  Words are written back to front so that they end at
// the end of the pair's area in forward order.
template <int kMode>
__global__ __launch_bounds__(64) void ef_walk_kernel(
    const EfPair *__restrict__ pairs, uint32_t count, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, const uint8_t *__restrict__ codes,
    const uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results,
    uint32_t *__restrict__ words, uint32_t *__restrict__ lens) {
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= count) return;
    const EfPair p = pairs[gi];
    const uint8_t *__restrict__ q = qs + p.q_off;
    const uint8_t *__restrict__ d = ds + p.d_off;
    saln_ends_free_result res = results[p.out];
    const uint32_t cap = p.lq + p.ld;
    uint32_t *w = words + p.cig_off;
    // the fill's end cell, kept inside the matrix whatever the record holds
    uint32_t i = min((uint32_t)max(res.db_end, 0), p.ld), j = min((uint32_t)max(res.q_end, 0), p.lq);
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    constexpr bool kExtend = kMode == SALN_MODE_EXTEND;
    uint32_t st = end_state[p.out] & 1u;  // 0 M, 1 I, 2 D
    uint32_t n = 0, run = 0, op = 0;
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
    if ((kLocal || kOverlap || kExtend) && res.score <= 0) i = j = 0;
    if constexpr (kOverlap) {
        // the end state is the end cell's own code: the first of M, I, D equal to P
        if (i > 0 && j > 0) st = ef_code(codes, p, i, j) & kEfArgMask;
    }
    while (j > 0) {
        if (i == 0) {
            // row 0.  Overlap: a free start, in M or after a D run that opened
            // there.  Semi-global and extend: the rest of the query is one
            // insertion.  (Local never stands here: its D(1, j) is -inf.)
            if constexpr (!kOverlap) {
                if (!kLocal) emit(SALN_CIGAR_I, j);
                j = 0;
            }
            break;
        }
        if (st == 0) {
            emit(q[j - 1] == d[i - 1] ? SALN_CIGAR_EQ : SALN_CIGAR_X, 1);
            --i, --j;
            if (i == 0 || j == 0) {
                // local: P = 0 on the border, the alignment begins here;
                // overlap: every cell of row 0 and column 0 is a free start
                if (kLocal || kOverlap) break;
                st = 1;  // semi-global and extend: row 0 is I; column 0 ends the loop
                continue;
            }
            const uint32_t a = ef_code(codes, p, i, j) & kEfArgMask;
            if (kLocal && a == kEfStop) break;
            st = a;
        } else if (st == 1) {
            emit(SALN_CIGAR_I, 1);
            --j;
            // column 0: I(i, 1) opens from M(i, 0)
            st = j > 0 && (ef_code(codes, p, i, j) & kEfIExt) ? 1u : 0u;
        } else {
            emit(SALN_CIGAR_D, 1);
            --i;
            // row 0: overlap's D(1, j) opens from M(0, j); elsewhere it is
            // -inf and a D run never reaches row 0
            st = i > 0 && (ef_code(codes, p, i, j) & kEfDExt) ? 2u : 0u;
        }
    }
    if constexpr (kExtend) {
        // column 0 above the origin is one deletion run, D(i, 0) = o + i e.  Only
        // a diagonal step arrives here: I(i, 1) is -inf below row 0
        emit(SALN_CIGAR_D, i);
        i = 0;
    }
    if (run && n < cap) w[cap - ++n] = (run << 4) | op;
    res.q_begin = (int32_t)j;
    res.db_begin = (int32_t)i;
    res.cigar_len = n;
    results[p.out] = res;
    lens[gi] = n;
}

// Packs the pairs' words (each at the end of its area) into pair order: pair
// gi's lens[gi] words go to out[dst[gi] ..).
__global__ __launch_bounds__(256) void ef_gather_kernel(
    const EfPair *__restrict__ pairs, uint32_t count, const uint32_t *__restrict__ words,
    const uint32_t *__restrict__ lens, const uint64_t *__restrict__ dst, uint32_t *__restrict__ out) {
    const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= count) return;
    const EfPair p = pairs[gi];
    const uint32_t cap = p.lq + p.ld, n = min(lens[gi], cap);
    const uint32_t *__restrict__ src = words + p.cig_off + (cap - n);
    uint32_t *__restrict__ to = out + dst[gi];
    for (uint32_t k = 0; k < n; ++k) to[k] = src[k];
}

namespace {

// What every class's launch takes.
struct FillLaunch {
    int32_t mode;
    dim3 grid, block;
    size_t lds;
    hipStream_t s;
    const EfPair *pairs;
    uint32_t first, count;
    const uint8_t *qs, *ds;
    uint8_t *codes, *end_state;
    saln_ends_free_result *results;
    EfScoring sc;
    uint32_t ld_max;
    const uint8_t *sub;
    int32_t xdrop;  // kEfNoXdrop: the plain fills
};

template <int G, int K>
hipError_t fill_class(const FillLaunch &a) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, a.grid, a.block, a.lds, a.s, a.pairs, a.first, a.count, a.qs, a.ds,
                           a.codes, a.end_state, a.results, a.sc, a.ld_max, a.sub);
        return hipGetLastError();
    };
    if (a.xdrop != kEfNoXdrop) {  // extension only: the host has checked mode and X
        auto gox = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, a.grid, a.block, a.lds, a.s, a.pairs, a.first, a.count, a.qs, a.ds,
                               a.codes, a.end_state, a.results, a.sc, a.ld_max, a.sub, a.xdrop);
            return hipGetLastError();
        };
        if (a.mode != SALN_MODE_EXTEND || a.xdrop < 0) return hipErrorInvalidValue;
        return ef_with_flag(a.sub != nullptr, [&](auto sb) {
            constexpr bool kSub = decltype(sb)::value;
            return a.codes ? gox(ef_xdrop_fill_kernel<G, K, true, kSub>)
                           : gox(ef_xdrop_fill_kernel<G, K, false, kSub>);
        });
    }
    return ef_with_mode(a.mode, [&](auto m) {
        return ef_with_flag(a.sub != nullptr, [&](auto sb) {
            constexpr int kMode = decltype(m)::value;
            constexpr bool kSub = decltype(sb)::value;
            return a.codes ? go(ef_fill_kernel<G, K, kMode, true, kSub>)
                           : go(ef_fill_kernel<G, K, kMode, false, kSub>);
        });
    });
}

}  // namespace

hipError_t launch_ef_fill(int cls, int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                          uint32_t ld_max, const uint8_t *qs, const uint8_t *ds, EfScoring sc,
                          const uint8_t *sub, uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results,
                          hipStream_t s, int32_t xdrop) {
    if (count == 0) return hipSuccess;
    if (cls < 0 || cls >= kEfClasses || ld_max > kEfMaxDb) return hipErrorInvalidValue;
    const uint32_t G = (uint32_t)kEfClass[cls].lanes;
    const EfFillGeometry geo = ef_fill_geometry(cls, ld_max, sub != nullptr);
    const uint32_t groups = geo.groups;
    const size_t lds = (size_t)geo.lds_bytes;
    const FillLaunch a{mode, dim3((count + groups - 1) / groups), dim3(groups * G), lds, s, pairs, first, count,
                       qs, ds, codes, end_state, results, sc, ld_max, sub, xdrop};
    switch (cls) {
        case 0: return fill_class<16, 10>(a);
        case 1: return fill_class<16, 16>(a);
        case 2: return fill_class<64, 8>(a);
        default: return fill_class<64, 16>(a);
    }
}

hipError_t launch_ef_walk(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                          const uint8_t *ds, const uint8_t *codes, const uint8_t *end_state,
                          saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                          hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 grid((count + 63) / 64), block(64);
    return ef_with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(ef_walk_kernel<decltype(m)::value>, grid, block, 0, s, pairs, count, qs, ds,
                           codes, end_state, results, words, lens);
        return hipGetLastError();
    });
}

hipError_t launch_ef_gather(const EfPair *pairs, uint32_t count, const uint32_t *words,
                            const uint32_t *lens, const uint64_t *dst, uint32_t *out,
                            hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(ef_gather_kernel, dim3((count + 255) / 256), dim3(256), 0, s, pairs, count,
                       words, lens, dst, out);
    return hipGetLastError();
}

}  // namespace saln
