// The steps of the ends-free fill: row 0, a lane's row of K cells (the Gotoh
// recurrence, the trace code, the three modes' end-cell trackers), the code
// store, overlap's last row, and the group's end cell with its record.
// ef_fill_kernel and ef_xdrop_fill_kernel (ends_free_kernels.hip) are built
// from all of them.
// ef_fill_long_kernel (ends_free_long_kernels.hip) uses those outside its
// loops (ef_overlap_end, ef_reduce_best, ef_store_end) and keeps its own row 0,
// row and chunk code: built from ef_row0 / ef_row its step loop compiled to
// other code and measured 0.5-1.5 % slower, so a change
// to the recurrence, the codes or the trackers here is made there too.
//
// A lane holds K consecutive query columns col0+1 .. col0+K (col0 absolute) in
// registers: qc their bases, Hp = P(r-1, j), Dn = D(r, j).  kMode is
// SALN_MODE_LOCAL, SALN_MODE_SEMI_GLOBAL, SALN_MODE_OVERLAP or SALN_MODE_EXTEND.
// kXdrop (extend only; include/saln.h, "X-drop extension"): every cell also
// carries B, the largest P of an unpruned cell of its dominance region, and a
// cell whose P lies more than X below max(B above, B left) is pruned: it hands
// exactly kEfNeg to its successors.  EfDrop holds what a lane keeps for it.
#pragma once
#include "ends_free_dev.hpp"

namespace saln {

// The best end cell of a lane's columns over the rows it has run, rows rising:
//   local        every M(i, j), strictly positive; k is the register of the
//                column (col0 + k + 1), the smallest row, then column, kept
//   semi-global  max(M, I)(i, lq) in the lane that holds column lq, row 0
//                first; k is the end state (0 M, 1 I)
//   overlap      P(i, lq) in that lane, strictly positive (the last row's
//                candidates: ef_last_row_best)
//   extend       local's: every M(i, j), strictly positive, no floor below it
struct EfBest {
    int32_t v;
    uint32_t i, k;
};

template <int kMode>
__device__ __forceinline__ EfBest ef_best_row0(uint32_t lq, int32_t o, int32_t e) {
    if constexpr (kMode == SALN_MODE_SEMI_GLOBAL)
        return {o + (int32_t)lq * e, 0u, 1u};  // row 0 ends in I
    else
        return {0, 0u, 0u};
}

// What kXdrop adds to a lane.  B is 0 on row 0 and in column 0 (the origin is
// the only cell there with P >= 0), so Bp starts at 0 and lane 0 takes 0.  A
// pad column starts at kEfPadB instead: every value lies below kEfPadB - X
// (the range guard), so a pad cell is always pruned, hands kEfPadB on to the
// pad cells right of it and below it, and never counts as alive: the vote
// needs no mask for the pads, as the tracker needs none.
constexpr int32_t kEfPadB = 1 << 30;
template <int K>
struct EfDrop {
    int32_t Bp[K];  // B(r-1, j) of my columns
    int32_t inB;    // B(r, col0), from the left neighbour
    int32_t pubB;   // B(r, col0+K), for the right neighbour
    int32_t X;
    bool alive;     // left by ef_row: a cell of its row was not pruned
};

// kSub (scoring under a substitution matrix, ends_free.hpp): the workgroup's
// copy in LDS of the batch's block `sub`, code[] then the score rows; nullptr
// and no LDS without kSub.  Every thread of the workgroup calls it, before any
// of them leaves the kernel.
template <bool kSub>
__device__ __forceinline__ uint8_t *ef_sub_stage(const uint8_t *__restrict__ sub) {
    if constexpr (kSub) {
        __shared__ __attribute__((aligned(16))) uint8_t lds[kEfSubBytes];
        for (uint32_t n = threadIdx.x; n < kEfSubBytes / 4; n += blockDim.x)
            reinterpret_cast<uint32_t *>(lds)[n] = reinterpret_cast<const uint32_t *>(sub)[n];
        __syncthreads();
        return lds;
    } else {
        return nullptr;
    }
}

// The staged form of a db byte under kSub: its symbol.
__device__ __forceinline__ uint32_t ef_sub_code(const uint8_t *lds, uint32_t byte) {
    return lds[byte & 0xFFu];
}

// s(i, j) under kSub: score[dch][qc], dch a staged db symbol and qc a column's
// symbol or kEfSubPad.  `trow` is ef_sub_row(dch), once per row.  The mask
// keeps the row inside the table also where the staged byte is a pad of the
// staging that no row uses.
__device__ __forceinline__ const int8_t *ef_sub_row(const uint8_t *lds, uint32_t dch) {
    return reinterpret_cast<const int8_t *>(lds) + kEfSubCodeBytes + (dch & (kEfSubSyms - 1)) * kEfSubStride;
}

// Row 0 of the columns behind col0.  Returns hd = P(0, col0).  kSub: qc holds
// the columns' symbols (sub: the block in LDS) and kEfSubPad in pad columns.
// kXdrop: (0, j) is pruned iff o + j e < -X (B is 0 all along row 0).
template <int K, int kMode, bool kSub = false, bool kXdrop = false>
__device__ __forceinline__ int32_t ef_row0(const uint8_t *__restrict__ q, uint32_t lq, uint32_t col0,
                                           int32_t o, int32_t e, uint32_t (&qc)[K], int32_t (&Hp)[K],
                                           int32_t (&Dn)[K], const uint8_t *sub = nullptr, int32_t X = 0) {
    static_assert(!kXdrop || kMode == SALN_MODE_EXTEND, "X-drop is extension's");
    // extension's row 0 is semi-global's: P(0, j) = I(0, j), D(1, j) = -inf
    constexpr bool kSemi = kMode == SALN_MODE_SEMI_GLOBAL || kMode == SALN_MODE_EXTEND;
    constexpr bool kOverlap = kMode == SALN_MODE_OVERLAP;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t j = col0 + k + 1;
        if constexpr (kSub)
            qc[k] = j <= lq ? ef_sub_code(sub, q[j - 1]) : kEfSubPad;
        else
            qc[k] = j <= lq ? (uint32_t)q[j - 1] : 0x100u;  // pad columns match nothing
        // semi-global and extend P(0, j) = I(0, j) = o + j e; local and overlap P = 0
        Hp[k] = !kSemi ? 0 : j <= lq ? o + (int32_t)j * e : kEfNeg;
        if constexpr (kXdrop) Hp[k] = Hp[k] < -X ? kEfNeg : Hp[k];
        // D(1, j): M(0, j) and D(0, j) are -inf; overlap opens it from M(0, j) = 0
        Dn[k] = kOverlap ? o + e : kEfNeg;
    }
    const int32_t h0 = !kSemi || col0 == 0 ? 0 : col0 <= lq ? o + (int32_t)col0 * e : kEfNeg;
    if constexpr (kXdrop) return h0 < -X ? kEfNeg : h0;
    return h0;
}

// A lane's K codes of one row (4 bits per cell), column col0 + 1 in the low
// nibble of w[0].
template <int K>
struct EfCodes {
    static_assert(K % 2 == 0, "two cells per code byte");
    uint32_t w[(K + 7) / 8];
};

// Stores those K / 2 bytes at `to`.  A pair's codes start 8-byte aligned and a
// row is a whole number of lanes' parts, so a part of 8 (K = 16) or 4 (K = 8)
// bytes is aligned and goes out as one store; other parts go out by bytes.
template <int K>
__device__ __forceinline__ void ef_store_codes(uint8_t *to, const EfCodes<K> &c) {
    if constexpr (K % 16 == 0) {
#pragma unroll
        for (int n = 0; n < K / 16; ++n) reinterpret_cast<uint2 *>(to)[n] = make_uint2(c.w[2 * n], c.w[2 * n + 1]);
    } else if constexpr (K % 8 == 0) {
#pragma unroll
        for (int n = 0; n < K / 8; ++n) reinterpret_cast<uint32_t *>(to)[n] = c.w[n];
    } else {
#pragma unroll
        for (int n = 0; n < K / 2; ++n) to[n] = (uint8_t)(c.w[n / 4] >> (8 * (n % 4)));
    }
}

// Row r (1 <= r <= ld) of the lane's columns.  dch = d[r-1]; inF = I(r, col0+1)
// and inH = P(r, col0) come from the left neighbour or the boundary.  Leaves
// hd = P(r, col0) for row r + 1 and pubF = I(r, col0+K+1), pubH = P(r, col0+K)
// for the right neighbour, updates the lane's best end cell, and with kCodes
// leaves the cells' codes in `codes`.  k_end: the register of column lq in its
// lane.  kSub: dch is the row's db symbol, qc the columns' symbols, and s comes
// from the block in LDS (sub) in place of sc.match / sc.mismatch.
//
// Extend keeps local's tracker (every M, strict > from 0) without local's
// floor, and its pad columns still need no mask.  Claim: a pad cell's M lies
// strictly below a real M(i, j), i, j >= 1, of the pair, or below 0, so it
// never is the pair's best and never ties with it; it can only displace a
// lane's value that is not the pair's best.  Every real P(i, j) is a real M,
// or an I or D value, which is some M of its row or column plus o + L e < 0,
// hence strictly below it, or it comes from a border, and the borders are
// P(0, 0) = 0 and o + j e < 0, o + i e < 0.  So a real P is at most a real M
// or at most 0, also where P(i-1, lq) is an I or D value.  The first pad
// column's M = P(i-1, lq) + s with s < 0 (mismatch < 0; under kSub the table's
// pad column) lies strictly below that; the pad cells' I and D lie strictly
// below an M of a real or a pad cell, and further pad columns follow by
// induction.  Nothing of this wraps: every pad value is at least
// kEfNeg - (m + 3) max|parameter| (D(i, j) >= D(1, j) + (i - 1) e bounds P
// from below in every column), which the range guard keeps above -2^31.
//
// kXdrop (xd): per cell Bin = max(B(r-1, j), B(r, j-1)); the cell is pruned iff
// P < Bin - X, and then its P, the I it hands right and the D it hands down
// are exactly kEfNeg; B(r, j) = max(Bin, outgoing P).  The tracker still needs
// no mask: a pruned cell's M is below Bin - X, and Bin is the P of an unpruned
// cell, which is at most a live M or 0 by the argument above.  Its code is
// stored but never read (a live cell's chosen predecessor holds a real value).
// Everything derived from kEfNeg is at most kEfNeg + (n + m + 2) max|parameter|,
// which the range guard (with X in it) keeps below -X <= Bin - X: pruned, and
// reset to kEfNeg, so nothing accumulates.
template <int K, int kMode, bool kCodes, bool kSub = false, bool kXdrop = false>
__device__ __forceinline__ void ef_row(const uint32_t (&qc)[K], uint32_t dch, int32_t inF, int32_t inH,
                                       const EfScoring &sc, uint32_t k_end, uint32_t r,
                                       int32_t (&Hp)[K], int32_t (&Dn)[K], int32_t &hd, int32_t &pubF,
                                       int32_t &pubH, EfBest &best, EfCodes<K> &codes,
                                       const uint8_t *sub = nullptr, EfDrop<K> *xd = nullptr) {
    static_assert(!kXdrop || kMode == SALN_MODE_EXTEND, "X-drop is extension's");
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL, kOverlap = kMode == SALN_MODE_OVERLAP;
    constexpr bool kEveryM = kLocal || kMode == SALN_MODE_EXTEND;  // the tracker over every M
    const int32_t o = sc.open, e = sc.extend;
    const int8_t *trow = nullptr;
    if constexpr (kSub) trow = ef_sub_row(sub, dch);
    int32_t F = inF;
    int32_t Msel = kEfNeg, Isel = kEfNeg;
    int32_t Bl = 0;  // kXdrop: B(r, j-1)
    bool alive = false;
    if constexpr (kXdrop) Bl = xd->inB;
    if constexpr (kCodes) {
#pragma unroll
        for (int n = 0; n < (K + 7) / 8; ++n) codes.w[n] = 0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int32_t s;
        if constexpr (kSub)
            s = trow[qc[k]];
        else
            s = qc[k] == dch ? sc.match : sc.mismatch;
        const int32_t M = ef_add(hd, s);
        const int32_t I = F, D = Dn[k];
        const int32_t P3 = max(M, max(I, D));
        int32_t P = kLocal ? max(P3, 0) : P3;
        bool cut = false;
        if constexpr (kXdrop) {
            const int32_t Bin = max(xd->Bp[k], Bl);
            cut = P3 < Bin - xd->X;
            P = cut ? kEfNeg : P3;
            Bl = max(Bin, P);
            xd->Bp[k] = Bl;
            alive = alive || !cut;
        }
        const int32_t tO = ef_add(M, o);
        if constexpr (kCodes) {
            uint32_t c = M == P3 ? 0u : I == P3 ? 1u : 2u;
            if constexpr (kLocal) c = P3 <= 0 ? kEfStop : c;
            c |= I >= tO ? kEfIExt : 0u;
            c |= D >= tO ? kEfDExt : 0u;
            codes.w[k / 8] |= c << (4 * (k % 8));
        }
        if constexpr (kEveryM) {
            // rows and columns come in increasing order: > keeps the
            // smallest row, then the smallest column, of my columns
            const bool b = M > best.v;
            best.v = b ? M : best.v;
            best.i = b ? r : best.i;
            best.k = b ? (uint32_t)k : best.k;
        } else if constexpr (kOverlap) {
            Msel = (uint32_t)k == k_end ? P3 : Msel;  // P(r, my k_end-th column)
        } else {
            Msel = (uint32_t)k == k_end ? M : Msel;
            Isel = (uint32_t)k == k_end ? I : Isel;
        }
        F = ef_add(max(tO, I), e);      // I(r, j+1)
        Dn[k] = ef_add(max(tO, D), e);  // D(r+1, j)
        if constexpr (kXdrop) {
            F = cut ? kEfNeg : F;
            Dn[k] = cut ? kEfNeg : Dn[k];
        }
        hd = Hp[k];
        Hp[k] = P;
    }
    hd = inH;
    pubF = F;
    pubH = Hp[K - 1];
    if constexpr (kXdrop) {
        xd->pubB = Bl;
        xd->alive = alive;
    }
    if constexpr (kOverlap) {
        const bool b = Msel > best.v;  // the smallest row wins a tie
        best.v = b ? Msel : best.v;
        best.i = b ? r : best.i;
    } else if constexpr (!kEveryM) {
        const int32_t v = max(Msel, Isel);
        const bool b = v > best.v;  // the smallest row wins a tie
        best.v = b ? v : best.v;
        best.i = b ? r : best.i;
        best.k = b ? (Msel >= Isel ? 0u : 1u) : best.k;  // M before I
    }
}

// Overlap's last row: Hp holds P(ld, j) of the lane's columns (row 0's zeros
// when ld == 0).  Pad columns hold real-looking values and are masked out.
// Strict > over rising columns keeps the smallest column in
// (rbest, rbest_j), rbest_j absolute; they start from (0, 0).
template <int K>
__device__ __forceinline__ void ef_last_row_best(const int32_t (&Hp)[K], uint32_t col0, uint32_t lq,
                                                 int32_t &rbest, uint32_t &rbest_j) {
    // Keep the register index of the new best (plus 1; 0: none) and add col0
    // once at the end: selecting the columns themselves makes the compiler
    // hold all K of them live over the row loop, which costs the K = 16
    // class fill with codes a wave per SIMD.
    uint32_t k1 = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool b = col0 + (uint32_t)k + 1 <= lq && Hp[k] > rbest;
        rbest = b ? Hp[k] : rbest;
        k1 = b ? (uint32_t)k + 1 : k1;
    }
    rbest_j = k1 ? col0 + k1 : rbest_j;
}

// Overlap's end cell of a lane: its last-column cell (v, i), which only the
// owner of column lq tracked, against its last-row cell.  A last-column cell
// above row ld wins a tie; in row ld it is the corner, and the last row's
// smallest column wins.
__device__ __forceinline__ void ef_overlap_end(bool owner, uint32_t lq, uint32_t ld, int32_t rbest,
                                               uint32_t rbest_j, int32_t &v, uint32_t &i, uint32_t &j) {
    if (!owner) v = 0;
    const bool row = rbest > v || (rbest == v && i == ld);
    v = row ? rbest : v;
    i = row ? ld : i;
    j = row ? rbest_j : lq;
}

// The pair's record: score and end cell; the walk fills in the rest.  steps:
// what `reserved` reports (the X-drop fill's row-loop steps; 0 elsewhere).
template <bool kCodes>
__device__ __forceinline__ void ef_store_end(saln_ends_free_result *__restrict__ results,
                                             uint8_t *__restrict__ end_state, uint32_t out, int32_t score,
                                             uint32_t db_end, uint32_t q_end, uint32_t state,
                                             uint32_t steps = 0) {
    saln_ends_free_result res;
    res.score = score;
    res.status = SALN_OK;
    res.q_begin = res.db_begin = -1;
    res.q_end = (int32_t)q_end;
    res.db_end = (int32_t)db_end;
    res.cigar_len = 0;
    res.reserved = steps;
    results[out] = res;
    if constexpr (kCodes) end_state[out] = (uint8_t)state;
}

// The group's end cell from its lanes' (v, row i, absolute column j), and the
// record.  Local, overlap and extend: the largest value, then the smallest row, then
// the smallest column (lanes met a row at different steps: the row index
// decides, not the step); lanes without a positive cell lose to every real
// cell, and a pair without one ends at the origin with score 0.  Semi-global:
// the owner of column lq holds it, with its end state.
template <int G, int kMode, bool kCodes>
__device__ __forceinline__ void ef_reduce_best(int lane, bool owner, int32_t v, uint32_t i, uint32_t j,
                                               uint32_t state, uint32_t lq,
                                               saln_ends_free_result *__restrict__ results,
                                               uint8_t *__restrict__ end_state, uint32_t out,
                                               uint32_t steps = 0) {
    if constexpr (kMode == SALN_MODE_SEMI_GLOBAL) {
        if (owner) ef_store_end<kCodes>(results, end_state, out, v, i, lq, state);
    } else {
        if (v <= 0) i = 0xFFFFFFFFu;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const int32_t ov = __shfl_xor(v, off, G);
            const uint32_t oi = __shfl_xor(i, off, G);
            const uint32_t oj = __shfl_xor(j, off, G);
            const bool take = ov > v || (ov == v && (oi < i || (oi == i && oj < j)));
            v = take ? ov : v;
            i = take ? oi : i;
            j = take ? oj : j;
        }
        if (lane == 0)
            ef_store_end<kCodes>(results, end_state, out, v, v > 0 ? i : 0u, v > 0 ? j : 0u, 0u, steps);
    }
}

}  // namespace saln
