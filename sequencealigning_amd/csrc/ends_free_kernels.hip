// Kernels of the ends-free engine (include/saln.h, saln_ends_free_*): Gotoh
// affine-gap alignment with free ends, local (Smith-Waterman), semi-global
// (the whole query against a free db substring) and overlap (dovetail: all
// four ends free, no floor).  NOT a reference-parity path: the reference only
// declares the first two modes.  DESIGN.md section 3 holds the recurrences,
// the tie rules and the code layout.
//
// Fill: the decomposition of the NW i32 lane fill.  One pair per group of G
// lanes, K query columns per lane in registers, the rows skewed over the
// lanes (lane l works on row t - l + 1 at step t), the left neighbour's
// boundary (P and the I candidate leaving its last column) handed over by
// DPP, the group's db row staged in LDS.  Values are plain int32.  Each lane
// keeps the best end cell of its own columns; the group reduces them at the
// end on (value, row, column), never on the step.
//
// Walk: one pair per lane, from the reported end cell along the 4-bit codes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_dev.hpp"

namespace saln {

// A lane's K / 2 code bytes of one row.  A pair's codes start 8-byte aligned
// and a row is a whole number of these, so 4- and 8-byte rows are aligned.
template <int K>
struct __attribute__((packed, aligned((K / 2) % 8 == 0 ? 8 : (K / 2) % 4 == 0 ? 4 : 1))) EfCodeRow {
    uint8_t b[K / 2];
};

// kMode: SALN_MODE_LOCAL, SALN_MODE_SEMI_GLOBAL or SALN_MODE_OVERLAP.
template <int G, int K, int kMode, bool kCodes>
__global__ __launch_bounds__(256) void ef_fill_kernel(
    const EfPair *__restrict__ pairs, uint32_t first, uint32_t count,
    const uint8_t *__restrict__ qs, const uint8_t *__restrict__ ds, uint8_t *__restrict__ codes,
    uint8_t *__restrict__ end_state, saln_ends_free_result *__restrict__ results, EfScoring sc,
    uint32_t ld_max) {
    static_assert(K % 2 == 0, "two cells per code byte");
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    const int gpb = (int)blockDim.x / G;
    const int lane = (int)threadIdx.x % G, grp = (int)threadIdx.x / G;
    const uint32_t gi = blockIdx.x * (uint32_t)gpb + (uint32_t)grp;
    if (gi >= count) return;  // whole group (DPP never crosses groups)
    const EfPair p = pairs[first + gi];
    const uint32_t lq = p.lq, ld = p.ld;
    const uint8_t *__restrict__ q = qs + p.q_off;
    const uint8_t *__restrict__ d = ds + p.d_off;
    saln_ends_free_result res;
    res.status = SALN_OK;
    res.q_begin = res.db_begin = -1;
    res.cigar_len = res.reserved = 0;
    if (lq == 0) {  // no column: score 0 at the origin in every mode
        if (lane == 0) {
            res.score = res.q_end = res.db_end = 0;
            results[p.out] = res;
            if constexpr (kCodes) end_state[p.out] = 0;
        }
        return;
    }
    extern __shared__ uint8_t ef_drow[];  // [groups][G + ld_max + G] db bytes
    uint8_t *myrow = ef_drow + (size_t)grp * (ld_max + 2 * G) + G;
    for (uint32_t i = (uint32_t)lane; i < ld; i += G) myrow[i] = d[i];
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();

    const int32_t o = sc.open, e = sc.extend;
    const uint32_t col0 = (uint32_t)lane * K;  // my columns: col0+1 .. col0+K
    const uint32_t jend = lq - 1;
    const uint32_t l_end = jend / K, k_end = jend % K;  // the lane and register of column lq
    uint32_t qc[K];
    int32_t Hp[K], Dn[K];  // P(r-1, j) and D(r, j) of my columns
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t j = col0 + k + 1;
        qc[k] = j <= lq ? (uint32_t)q[j - 1] : 0x100u;  // pad columns match nothing
        // row 0: semi-global P(0, j) = I(0, j) = o + j e; local and overlap P = 0
        Hp[k] = kLocal || kOverlap ? 0 : j <= lq ? o + (int32_t)j * e : kEfNeg;
        // D(1, j): M(0, j) and D(0, j) are -inf; overlap opens it from M(0, j) = 0
        Dn[k] = kOverlap ? o + e : kEfNeg;
    }
    int32_t hd = kLocal || kOverlap || col0 == 0 ? 0 : col0 <= lq ? o + (int32_t)col0 * e : kEfNeg;  // P(0, col0)
    // column 0, entering lane 0: P(i, 0) = 0 in every mode (the free start of
    // semi-global and overlap, local's floor); I(i, 1) opens from M(i, 0) = 0
    // in semi-global and overlap and is -inf in local
    const int32_t bH = 0, bF = kLocal ? kEfNeg : o + e;
    int32_t pubF = kEfNeg, pubH = kEfNeg;
    // best end cell of my columns: local every M(i, j), strictly positive;
    // semi-global max(M, I)(i, lq) in the lane holding column lq, row 0 first;
    // overlap P(i, lq) in that lane, strictly positive (the last row's
    // candidates are taken from Hp after the loop)
    int32_t best = kLocal || kOverlap ? 0 : o + (int32_t)lq * e;
    uint32_t best_i = 0, best_k = 0;  // semi-global: best_k is the end state
    if (!kLocal && !kOverlap) best_k = 1;  // row 0 ends in I
    uint8_t *crow = nullptr;
    if constexpr (kCodes) crow = codes + p.code_off + (size_t)lane * (K / 2);
    const int T = (int)ld + G - 1;
    for (int t = 0; t < T; ++t) {
        const int r = t - lane + 1;
        const uint32_t dch = myrow[t - lane];  // d[r-1]; the pads cover rows outside the db
        const int32_t inF = ef_shr1<G>(bF, pubF);  // I(r, col0+1)
        const int32_t inH = ef_shr1<G>(bH, pubH);  // P(r, col0)
        if (r >= 1 && r <= (int)ld) {
            int32_t F = inF;
            int32_t Msel = kEfNeg, Isel = kEfNeg;
            uint32_t nib[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int32_t M = ef_add(hd, qc[k] == dch ? sc.match : sc.mismatch);
                const int32_t I = F, D = Dn[k];
                const int32_t P3 = max(M, max(I, D));
                const int32_t P = kLocal ? max(P3, 0) : P3;
                const int32_t tO = ef_add(M, o);
                if constexpr (kCodes) {
                    uint32_t c = M == P3 ? 0u : I == P3 ? 1u : 2u;
                    if constexpr (kLocal) c = P3 <= 0 ? kEfStop : c;
                    c |= I >= tO ? kEfIExt : 0u;
                    c |= D >= tO ? kEfDExt : 0u;
                    nib[k] = c;
                }
                if constexpr (kLocal) {
                    // rows and columns come in increasing order: > keeps the
                    // smallest row, then the smallest column, of my columns
                    const bool b = M > best;
                    best = b ? M : best;
                    best_i = b ? (uint32_t)r : best_i;
                    best_k = b ? (uint32_t)k : best_k;
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
            if constexpr (kOverlap) {
                const bool b = Msel > best;  // the smallest row wins a tie
                best = b ? Msel : best;
                best_i = b ? (uint32_t)r : best_i;
            } else if constexpr (!kLocal) {
                const int32_t v = max(Msel, Isel);
                const bool b = v > best;  // the smallest row wins a tie
                best = b ? v : best;
                best_i = b ? (uint32_t)r : best_i;
                best_k = b ? (Msel >= Isel ? 0u : 1u) : best_k;  // M before I
            }
            if constexpr (kCodes) {
                if (col0 < lq) {  // lanes wholly past the query store nothing
                    EfCodeRow<K> w;
#pragma unroll
                    for (int k = 0; k < K; k += 2) w.b[k / 2] = (uint8_t)(nib[k] | (nib[k + 1] << 4));
                    *reinterpret_cast<EfCodeRow<K> *>(crow + (size_t)(r - 1) * p.row_bytes) = w;
                }
            }
        }
    }
    if constexpr (kOverlap) {
        // Only the lane of column lq tracked a last-column cell.  The last
        // row: Hp holds P(ld, j) of my columns (row 0's zeros when ld == 0).
        // Strict > from 0 over rising columns keeps the smallest column; pad
        // columns hold real-looking values and are masked out.
        if ((uint32_t)lane != l_end) best = 0;
        best_k = k_end;
        int32_t rbest = 0;
        uint32_t rbest_k = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool b = col0 + (uint32_t)k + 1 <= lq && Hp[k] > rbest;
            rbest = b ? Hp[k] : rbest;
            rbest_k = b ? (uint32_t)k : rbest_k;
        }
        // a last-column cell above row ld wins a tie with a last-row cell; in
        // row ld it is the corner, and the last row's smallest column wins
        const bool row = rbest > best || (rbest == best && best_i == ld);
        best = row ? rbest : best;
        best_i = row ? ld : best_i;
        best_k = row ? rbest_k : best_k;
    }
    if constexpr (kLocal || kOverlap) {
        // the group's best: the largest value, then the smallest row, then
        // the smallest column (lanes met a row at different steps: the row
        // index decides, not the step).  Lanes without a positive cell hold
        // (0, row 0, column col0+1) and lose to every real cell.
        uint32_t ij = best > 0 ? (best_i << 11) | (col0 + best_k + 1) : 0xFFFFFFFFu;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const int32_t ov = __shfl_xor(best, off, G);
            const uint32_t oij = __shfl_xor(ij, off, G);
            const bool take = ov > best || (ov == best && oij < ij);
            best = take ? ov : best;
            ij = take ? oij : ij;
        }
        if (lane == 0) {
            res.score = best;
            res.db_end = best > 0 ? (int32_t)(ij >> 11) : 0;
            res.q_end = best > 0 ? (int32_t)(ij & 2047u) : 0;
            results[p.out] = res;
            if constexpr (kCodes) end_state[p.out] = 0;
        }
    } else if ((uint32_t)lane == l_end) {
        res.score = best;
        res.db_end = (int32_t)best_i;
        res.q_end = (int32_t)lq;
        results[p.out] = res;
        if constexpr (kCodes) end_state[p.out] = (uint8_t)best_k;
    }
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
    if ((kLocal || kOverlap) && res.score <= 0) i = j = 0;
    if constexpr (kOverlap) {
        // the end state is the end cell's own code: the first of M, I, D equal to P
        if (i > 0 && j > 0) st = ef_code(codes, p, i, j) & kEfArgMask;
    }
    while (j > 0) {
        if constexpr (kOverlap) {
            // every cell of row 0 and column 0 is a free start: the walk ends
            // as soon as it stands on one, in M or after a gap that opened there
            if (i == 0) break;
            if (st == 0) {
                emit(q[j - 1] == d[i - 1] ? SALN_CIGAR_EQ : SALN_CIGAR_X, 1);
                --i, --j;
                if (i == 0 || j == 0) break;
                st = ef_code(codes, p, i, j) & kEfArgMask;
            } else if (st == 1) {
                emit(SALN_CIGAR_I, 1);
                --j;  // column 0: I(i, 1) opened from M(i, 0)
                st = j > 0 && (ef_code(codes, p, i, j) & kEfIExt) ? 1u : 0u;
            } else {
                emit(SALN_CIGAR_D, 1);
                --i;  // row 0: D(1, j) opened from M(0, j)
                st = i > 0 && (ef_code(codes, p, i, j) & kEfDExt) ? 2u : 0u;
            }
            continue;
        }
        if (i == 0) {  // semi-global row 0: the rest of the query is one insertion
            if (!kLocal) emit(SALN_CIGAR_I, j);
            j = 0;
            break;
        }
        if (st == 0) {
            emit(q[j - 1] == d[i - 1] ? SALN_CIGAR_EQ : SALN_CIGAR_X, 1);
            --i, --j;
            if (i == 0 || j == 0) {
                if (kLocal) break;  // P = 0 on the border: the alignment begins here
                st = 1;             // semi-global row 0 is I; column 0 ends the loop
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
            // (D(1, j) is -inf: a D run never reaches row 0)
            st = i > 0 && (ef_code(codes, p, i, j) & kEfDExt) ? 2u : 0u;
        }
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

template <int G, int K>
hipError_t fill_class(int32_t mode, bool with_codes, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                      const EfPair *pairs, uint32_t first, uint32_t count, const uint8_t *qs,
                      const uint8_t *ds, uint8_t *codes, uint8_t *end_state,
                      saln_ends_free_result *results, EfScoring sc, uint32_t ld_max) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, pairs, first, count, qs, ds, codes, end_state,
                           results, sc, ld_max);
        return hipGetLastError();
    };
    constexpr int kL = SALN_MODE_LOCAL, kS = SALN_MODE_SEMI_GLOBAL, kO = SALN_MODE_OVERLAP;
    if (mode == kL) return with_codes ? go(ef_fill_kernel<G, K, kL, true>) : go(ef_fill_kernel<G, K, kL, false>);
    if (mode == kO) return with_codes ? go(ef_fill_kernel<G, K, kO, true>) : go(ef_fill_kernel<G, K, kO, false>);
    if (mode != kS) return hipErrorInvalidValue;
    return with_codes ? go(ef_fill_kernel<G, K, kS, true>) : go(ef_fill_kernel<G, K, kS, false>);
}

}  // namespace

hipError_t launch_ef_fill(int cls, int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                          uint32_t ld_max, const uint8_t *qs, const uint8_t *ds, EfScoring sc,
                          uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results,
                          hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (cls < 0 || cls >= kEfClasses || ld_max > kEfMaxDb) return hipErrorInvalidValue;
    const uint32_t G = (uint32_t)kEfClass[cls].lanes;
    // as many groups per workgroup (of at most 256 lanes) as 64 KB of LDS stage rows for
    uint32_t groups = 256u / G;
    while (groups > 1 && ef_lds_bytes(cls, groups, ld_max) > (64u << 10)) --groups;
    const size_t lds = (size_t)ef_lds_bytes(cls, groups, ld_max);
    const dim3 grid((count + groups - 1) / groups), block(groups * G);
    const bool wc = codes != nullptr;
    switch (cls) {
        case 0: return fill_class<16, 10>(mode, wc, grid, block, lds, s, pairs, first, count, qs, ds, codes, end_state, results, sc, ld_max);
        case 1: return fill_class<16, 16>(mode, wc, grid, block, lds, s, pairs, first, count, qs, ds, codes, end_state, results, sc, ld_max);
        case 2: return fill_class<64, 8>(mode, wc, grid, block, lds, s, pairs, first, count, qs, ds, codes, end_state, results, sc, ld_max);
        default: return fill_class<64, 16>(mode, wc, grid, block, lds, s, pairs, first, count, qs, ds, codes, end_state, results, sc, ld_max);
    }
}

hipError_t launch_ef_walk(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                          const uint8_t *ds, const uint8_t *codes, const uint8_t *end_state,
                          saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                          hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 grid((count + 63) / 64), block(64);
    if (mode == SALN_MODE_LOCAL)
        hipLaunchKernelGGL(ef_walk_kernel<SALN_MODE_LOCAL>, grid, block, 0, s, pairs, count, qs, ds,
                           codes, end_state, results, words, lens);
    else if (mode == SALN_MODE_OVERLAP)
        hipLaunchKernelGGL(ef_walk_kernel<SALN_MODE_OVERLAP>, grid, block, 0, s, pairs, count, qs, ds,
                           codes, end_state, results, words, lens);
    else if (mode == SALN_MODE_SEMI_GLOBAL)
        hipLaunchKernelGGL(ef_walk_kernel<SALN_MODE_SEMI_GLOBAL>, grid, block, 0, s, pairs, count, qs,
                           ds, codes, end_state, results, words, lens);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
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
