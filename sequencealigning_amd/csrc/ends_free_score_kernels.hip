// Score-only search of the ends-free engine (include/saln.h,
// saln_ends_free_score_*): the packed-i16 fill, two pairs
// per lane group, and the gather that brings the i32 fills' scores into the
// caller's order.
//
// Decomposition: the class fill's (ends_free_kernels.hip): K query columns per
// lane in registers, the rows skewed over the G lanes of a group (lane l works
// on row t - l + 1 at step t), the left neighbour's P and I handed over by
// DPP, the group's db rows staged in LDS.  Every register holds two pairs of
// one class: pair A in its low 16 bits, pair B in its high 16 bits, so a
// v_pk_add_i16 (clamp) or v_pk_max_i16 advances two cells.  Only the score is
// kept: no row, no column, no tie rule.
//
// Range.  -infinity is -32768 and every add saturates.  The host sends a pair
// here only when every real value of its tables and every value this kernel
// forms from them (M, I, D, P, M + o, the outgoing I and D) lies inside
// [-32768, 32767] (ef_score_packed, ends_free_score.hpp): nothing real ever
// saturates.  -infinity enters a max() beside a real value, or takes e < 0 or a
// pad column's s < 0 on top and stays at -32768; it never takes a positive s:
// the only P that is -infinity is a pad column's.
//
// Unequal halves.  The two pairs differ in n and m; the group runs
// max(m_a, m_b) rows over all of its columns.
//  - Rows past a half's own m (ghost rows) see whatever db byte the other
//    half's staging left there.  Rows only feed rows below them, so no real
//    row reads a ghost row; the trackers drop a ghost row's candidates by the
//    row mask (a half is 0xFFFF iff 1 <= r <= its m).  A ghost row may saturate
//    at either end of the range; nothing reads it.
//  - Columns past a half's own n (pad columns) carry a symbol that no db byte
//    equals (0x100; under a matrix the table's pad column, strictly negative).
//    Columns only feed columns right of them, so no real column reads a pad
//    column.  Local's tracker takes every M without a column mask: a pad
//    cell's M = P(i-1, j-1) + s, s < 0, lies strictly below a P of the pair,
//    and a P is a real M, or lies below one, or is 0 (ef_row,
//    ends_free_fill.hpp, has the argument; local's floor keeps pad values
//    above -4 A like real ones).  Semi-global's tracker reads column n alone,
//    by a per-register mask, so its pad columns, which start from -infinity
//    and stay there or saturate, are never looked at.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free_fill.hpp"
#include "ends_free_score.hpp"

namespace saln {

namespace {

typedef short pk16 __attribute__((ext_vector_type(2)));
typedef unsigned short pku16 __attribute__((ext_vector_type(2)));

constexpr int32_t kPkNeg = -32768;  // -infinity of a half

__device__ __forceinline__ pk16 pk_s(uint32_t x) { return __builtin_bit_cast(pk16, x); }
__device__ __forceinline__ uint32_t pk_u(pk16 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ pk16 pk_spl(int32_t v) { return pk16{(short)v, (short)v}; }
__device__ __forceinline__ pk16 pk_two(int32_t lo, int32_t hi) { return pk16{(short)lo, (short)hi}; }
__device__ __forceinline__ pk16 pk_add(pk16 a, pk16 b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ pk16 pk_max(pk16 a, pk16 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ int32_t pk_lo(pk16 x) { return (int32_t)x.x; }
__device__ __forceinline__ int32_t pk_hi(pk16 x) { return (int32_t)x.y; }

// lane i <- lane i-1 within the group; the group's lane 0 keeps `old`.
template <int G>
__device__ __forceinline__ pk16 pk_shr1(pk16 old, pk16 v) {
    return pk_s((uint32_t)ef_shr1<G>((int32_t)pk_u(old), (int32_t)pk_u(v)));
}

// A border value of one half: o + j e for a column 1 <= j <= n, else -infinity.
__device__ __forceinline__ int32_t pk_row0(uint32_t j, uint32_t n, int32_t o, int32_t e) {
    return j <= n ? o + (int32_t)j * e : kPkNeg;
}

}  // namespace

// kMode: SALN_MODE_LOCAL or SALN_MODE_SEMI_GLOBAL.  kSub: s(i, j) from the
// matrix block in LDS (ends_free.hpp), read once per half and cell and joined
// by one v_perm; the staged rows and the columns then hold symbols, and the two
// halves' column symbols sit in registers of their own (qc[k], qc[K + k]).
// Scalar scoring: a half's column holds its query byte, or 0x100 in a pad
// column; x = q ^ d is 0 in a half iff its bytes are equal, y = min_u16(x, 1)
// is [q != d], and s = match + y (mismatch - match) is one packed multiply-add.
// y_max is that 1 in both halves, 0x00010001, and comes as an argument: told
// that y is 0 or 1, the compiler replaces the multiply-add by two compares and
// two selects per register, seven instructions for s in place of three.
template <int G, int K, int kMode, bool kSub>
__global__ __launch_bounds__(256) void ef_score_pk_kernel(
    const EfPkGroup *__restrict__ groups, uint32_t first, uint32_t count, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, int32_t *__restrict__ scores, EfScoring sc, uint32_t ld_max,
    const uint8_t *__restrict__ sub, uint32_t y_max) {
    static_assert(kMode == SALN_MODE_LOCAL || kMode == SALN_MODE_SEMI_GLOBAL, "the packed modes");
    constexpr bool kLocal = kMode == SALN_MODE_LOCAL;
    uint8_t *ef_sub = ef_sub_stage<kSub>(sub);  // before any thread leaves
    const int gpb = (int)blockDim.x / G;
    const int lane = (int)threadIdx.x % G, grp = (int)threadIdx.x / G;
    const uint32_t gi = blockIdx.x * (uint32_t)gpb + (uint32_t)grp;
    if (gi >= count) return;  // whole group (DPP never crosses groups)
    const EfPkGroup g = groups[first + gi];
    const uint32_t na = g.n_a, nb = g.n_b, ma = g.m_a, mb = g.m_b;
    const uint32_t mmax = max(ma, mb);  // <= ld_max: the launch's longest db
    extern __shared__ uint8_t ef_drow2[];  // [groups][G + ld_max + G] entries of 16 bits
    uint16_t *myrow = reinterpret_cast<uint16_t *>(ef_drow2) + (size_t)grp * (ld_max + 2 * G) + G;
    {
        const uint8_t *__restrict__ da = ds + g.da_off;
        const uint8_t *__restrict__ db = ds + g.db_off;
        for (uint32_t i = (uint32_t)lane; i < mmax; i += G) {
            uint32_t a = i < ma ? (uint32_t)da[i] : 0u, b = i < mb ? (uint32_t)db[i] : 0u;
            if constexpr (kSub) {
                a = ef_sub_code(ef_sub, a);
                b = ef_sub_code(ef_sub, b);
            }
            myrow[i] = (uint16_t)(a | (b << 8));
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();

    const int32_t o = sc.open, e = sc.extend;
    const pk16 o2 = pk_spl(o), e2 = pk_spl(e), neg2 = pk_spl(kPkNeg), zero2 = pk_spl(0);
    const pk16 match2 = pk_spl(sc.match), dmis2 = pk_spl(sc.mismatch - sc.match);
    const uint32_t col0 = (uint32_t)lane * K;  // my columns: col0+1 .. col0+K, of both halves
    uint32_t qc[kSub ? 2 * K : K];
    uint32_t sel[kLocal ? 1 : K];  // semi-global: a half is 0xFFFF iff the register is its column n
    pk16 Hp[K], Dn[K];
    uint32_t own = 0;  // the halves whose column n I hold
    {
        const uint8_t *__restrict__ qa = qs + g.qa_off;
        const uint8_t *__restrict__ qb = qs + g.qb_off;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t j = col0 + (uint32_t)k + 1;
            if constexpr (kSub) {
                qc[k] = j <= na ? ef_sub_code(ef_sub, qa[j - 1]) : kEfSubPad;
                qc[K + k] = j <= nb ? ef_sub_code(ef_sub, qb[j - 1]) : kEfSubPad;
            } else {
                // pad columns match nothing: no byte is 0x100
                qc[k] = (j <= na ? (uint32_t)qa[j - 1] : 0x100u) | ((j <= nb ? (uint32_t)qb[j - 1] : 0x100u) << 16);
            }
            // semi-global P(0, j) = I(0, j) = o + j e; local P = 0.  D(1, j) = -inf
            Hp[k] = kLocal ? zero2 : pk_two(pk_row0(j, na, o, e), pk_row0(j, nb, o, e));
            Dn[k] = neg2;
            if constexpr (!kLocal) {
                sel[k] = (j == na ? 0xFFFFu : 0u) | (j == nb ? 0xFFFF0000u : 0u);
                own |= sel[k];
            }
        }
    }
    // P(0, col0): 0 at the origin and in local
    pk16 hd = kLocal || col0 == 0 ? zero2 : pk_two(pk_row0(col0, na, o, e), pk_row0(col0, nb, o, e));
    // column 0, entering lane 0: P(i, 0) = 0 (semi-global's free start, local's
    // floor); I(i, 1) opens from M(i, 0) = 0 in semi-global and is -inf in local
    const pk16 bH = zero2, bF = kLocal ? neg2 : pk_spl(o + e);
    pk16 pubF = neg2, pubH = neg2;
    // local: max(0, every M); semi-global: row 0's P(0, n) = o + n e (n = 0: the
    // origin; the score of such a half is forced to 0 below anyway)
    pk16 best = kLocal ? zero2 : pk_two(na ? o + (int32_t)na * e : 0, nb ? o + (int32_t)nb * e : 0);
    const int T = (int)mmax + G - 1;
    for (int t = 0; t < T; ++t) {
        const int r = t - lane + 1;
        const uint32_t w = myrow[t - lane];  // d[r-1] of both halves; the pads cover rows outside
        const pk16 inF = pk_shr1<G>(bF, pubF);  // I(r, col0+1)
        const pk16 inH = pk_shr1<G>(bH, pubH);  // P(r, col0)
        if (r >= 1 && r <= (int)mmax) {
            // the halves for which row r is real
            const uint32_t rowmask = ((uint32_t)r <= ma ? 0xFFFFu : 0u) | ((uint32_t)r <= mb ? 0xFFFF0000u : 0u);
            uint32_t d2 = 0;
            const int8_t *trow_a = nullptr, *trow_b = nullptr;
            if constexpr (kSub) {
                trow_a = ef_sub_row(ef_sub, w & 0xFFu);
                trow_b = ef_sub_row(ef_sub, w >> 8);
            } else {
                d2 = __builtin_amdgcn_perm(0u, w, 0x0c010c00u);  // A's byte low, B's byte in bits 16-23
            }
            pk16 F = inF;
            pk16 rb = neg2;    // local: the row's largest M
            uint32_t acc = 0;  // semi-global: P(r, n) in the halves I own
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pk16 s;
                if constexpr (kSub) {
                    const uint32_t sa = (uint32_t)(int32_t)trow_a[qc[k]], sb = (uint32_t)(int32_t)trow_b[qc[K + k]];
                    s = pk_s(__builtin_amdgcn_perm(sb, sa, 0x05040100u));  // (sa, sb), 16 bits each
                } else {
                    const pku16 x = __builtin_bit_cast(pku16, qc[k] ^ d2);
                    const pku16 y = __builtin_elementwise_min(x, __builtin_bit_cast(pku16, y_max));
                    s = __builtin_bit_cast(pk16, y) * dmis2 + match2;
                }
                const pk16 M = pk_add(hd, s);
                const pk16 I = F, D = Dn[k];
                const pk16 P3 = pk_max(M, pk_max(I, D));
                const pk16 P = kLocal ? pk_max(P3, zero2) : P3;
                const pk16 tO = pk_add(M, o2);
                if constexpr (kLocal)
                    rb = pk_max(rb, M);
                else
                    acc = (pk_u(P) & sel[k]) | acc;
                F = pk_add(pk_max(tO, I), e2);      // I(r, j+1)
                Dn[k] = pk_add(pk_max(tO, D), e2);  // D(r+1, j)
                hd = Hp[k];
                Hp[k] = P;
            }
            hd = inH;
            pubF = F;
            pubH = Hp[K - 1];
            if constexpr (kLocal) {
                // a ghost row's half becomes 0, which never beats best >= 0
                best = pk_max(best, pk_s(pk_u(rb) & rowmask));
            } else {
                // max over the real rows of P(r, n) = max(M, I)(r, n): D(r, n)
                // lies strictly below an M of column n.  Everything else -inf
                const uint32_t valid = rowmask & own;
                best = pk_max(best, pk_s((acc & valid) | (pk_u(neg2) & ~valid)));
            }
        }
    }
    if constexpr (kLocal) {
        uint32_t b = pk_u(best);
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) b = pk_u(pk_max(pk_s(b), pk_s((uint32_t)__shfl_xor((int)b, off, G))));
        if (lane == 0) {
            scores[g.out_a] = pk_lo(pk_s(b));
            if (g.out_b != kEfPkNone) scores[g.out_b] = pk_hi(pk_s(b));
        }
    } else {
        // the lane that holds a half's column n has its score; without a column
        // (n = 0) the score is 0 and lane 0 writes it
        const bool wa = na ? (own & 0xFFFFu) != 0 : lane == 0;
        const bool wb = nb ? (own & 0xFFFF0000u) != 0 : lane == 0;
        if (wa) scores[g.out_a] = na ? pk_lo(best) : 0;
        if (wb && g.out_b != kEfPkNone) scores[g.out_b] = nb ? pk_hi(best) : 0;
    }
}

__global__ __launch_bounds__(256) void ef_score_gather_kernel(
    const saln_ends_free_result *__restrict__ results, const uint32_t *__restrict__ out, uint32_t count,
    int32_t *__restrict__ scores) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) scores[out[k]] = results[k].score;
}

namespace {

struct ScoreLaunch {
    int32_t mode;
    dim3 grid, block;
    size_t lds;
    hipStream_t s;
    const EfPkGroup *groups;
    uint32_t first, count;
    const uint8_t *qs, *ds;
    int32_t *scores;
    EfScoring sc;
    uint32_t ld_max;
    const uint8_t *sub;
};

template <int G, int K>
hipError_t score_class(const ScoreLaunch &a) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, a.grid, a.block, a.lds, a.s, a.groups, a.first, a.count, a.qs, a.ds, a.scores,
                           a.sc, a.ld_max, a.sub, 0x00010001u);
        return hipGetLastError();
    };
    return ef_with_flag(a.sub != nullptr, [&](auto sb) {
        constexpr bool kSub = decltype(sb)::value;
        return a.mode == SALN_MODE_LOCAL ? go(ef_score_pk_kernel<G, K, SALN_MODE_LOCAL, kSub>)
                                         : go(ef_score_pk_kernel<G, K, SALN_MODE_SEMI_GLOBAL, kSub>);
    });
}

}  // namespace

hipError_t launch_ef_score_pk(int cls, int32_t mode, const EfPkGroup *groups, uint32_t first, uint32_t count,
                              uint32_t ld_max, const uint8_t *qs, const uint8_t *ds, EfScoring sc,
                              const uint8_t *sub, int32_t *scores, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (cls < 0 || cls >= kEfClasses || ld_max > kEfMaxDb) return hipErrorInvalidValue;
    if (mode != SALN_MODE_LOCAL && mode != SALN_MODE_SEMI_GLOBAL) return hipErrorInvalidValue;
    const uint32_t G = (uint32_t)kEfClass[cls].lanes;
    const EfFillGeometry geo = ef_score_geometry(cls, ld_max, sub != nullptr);
    const ScoreLaunch a{mode, dim3((count + geo.groups - 1) / geo.groups), dim3(geo.groups * G),
                        (size_t)geo.lds_bytes, s, groups, first, count, qs, ds, scores, sc, ld_max, sub};
    switch (cls) {
        case 0: return score_class<16, 10>(a);
        case 1: return score_class<16, 16>(a);
        case 2: return score_class<64, 8>(a);
        default: return score_class<64, 16>(a);
    }
}

hipError_t launch_ef_score_gather(const saln_ends_free_result *results, const uint32_t *out, uint32_t count,
                                  int32_t *scores, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(ef_score_gather_kernel, dim3((count + 255) / 256), dim3(256), 0, s, results, out, count,
                       scores);
    return hipGetLastError();
}

}  // namespace saln
