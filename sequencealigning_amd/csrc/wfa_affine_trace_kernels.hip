// Corrected gap-affine WFA with the alignment (saln_wfa_affine_align_batch):
// the trace fill and the walk + replay that turn a pair's known penalty into
// one optimal alignment as CIGAR words.  The score-only engine, its
// recurrences and its geometry are wfa_affine_kernels.hip's; the device
// helpers both files use are in wfa_affine_dev.hpp.
//
// Trace fill (wfa_affine_trace_kernel): the same recurrences, one wave per
// pair, lanes over the diagonals of a step, the LDS ring, staged sequences.
// The pair's step count T = penalty / g is known from the score pass
// (WfaAffPair.reserved), so the fill runs exactly T steps and must converge
// at step T and at no earlier one; anything else is reported in the pair's
// status (SALN_INTERNAL) and never looped on.  For every (step t, diagonal k)
// it writes a 4-bit origin code to HBM:
//   bits 0-1  the source of the pre-extension M: 0 none (not a cell), 1 X
//             (M[t - x/g][k] + 1), 2 I[t][k], 3 D[t][k];
//   bit 2     I[t][k] came from I[t - e/g][k-1] (extend), not from
//             M[t - (o+e)/g][k-1] (open);
//   bit 3     D[t][k] came from D[t - e/g][k+1] (extend), not from
//             M[t - (o+e)/g][k+1] (open).
// Tie-break (fixed, so a pair's CIGAR does not depend on its batch, its chunk
// or the run): M prefers X, then I, then D; a gap prefers extend over open.
// Layout: step t's row is at (t - 1) * (wt / 2) bytes of the pair's code
// area, diagonal k's code is nibble k & (wt - 1) of it (low nibble first);
// wt is a power of two >= the widest possible wavefront + 2, so the walker
// needs no per-step range table and no two diagonals of a step share a nibble.
//
// Walk + replay (wfa_affine_walk_kernel, one lane per pair): backwards from
// (T, ld - lq, M) over the codes to (0, 0, M), collecting the edit ops (X,
// gap in the query, gap in the db) and for each op one bit: the path is in M
// right after it (X, and the op that closes a gap).  Then forwards from
// (0, 0): extend along matches (an '=' run), apply an op, extend again only
// where the bit is set.  Every M entry of a wavefront is fully extended, so
// this reproduces the WFA path without stored offsets.  The replay must end
// at (lq, ld) with the penalty T * g, else the pair's status is SALN_INTERNAL.
// Every loop is bounded (the walk by 2 T + 2 state changes, the replay by T
// ops and lq + ld columns), and no kernel waits on another workgroup.
//
// Orientation: the kernel's I component advances the db offset h - a column
// of '-' against a db base, SALN_CIGAR_D; its D component advances the query
// - a query base against '-', SALN_CIGAR_I.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "saln.h"
#include "wfa_affine.hpp"
#include "wfa_affine_dev.hpp"

namespace saln {

namespace {

enum : uint32_t { kOpX = 1, kOpI = 2, kOpD = 3, kOpInM = 4 };  // op bytes of the walk

// The trace fill of one pair: 0; 1 for an internal inconsistency (no
// convergence at exactly step T, or a wavefront wider than the code row); 2
// when a wavefront is wider than the ring (the caller's wider ring is next).
template <typename OffT, typename S>
__device__ __forceinline__ int32_t wfa_trace_pair(const S &q, int32_t lq, const S &d, int32_t ld,
                                                  const WfaAffParams &prm, int32_t T, int32_t *rng,
                                                  OffT *Mr, OffT *Ir, OffT *Dr,
                                                  uint8_t *__restrict__ codes, int32_t wt) {
    constexpr int32_t kNeg = OffTraits<OffT>::kNeg;
    const int32_t lane = (int32_t)threadIdx.x;
    const int32_t W = prm.W, wm = prm.W - 1;
    const int32_t tx = prm.x / prm.g, toe = (prm.o + prm.e) / prm.g, te = prm.e / prm.g;
    const int32_t kend = ld - lq;
    const size_t pitch = (size_t)(wt >> 1);
    __builtin_amdgcn_wave_barrier();
    if (lane < 3 * kRingMax) {  // every slot empty
        rng[2 * lane] = kEmptyLo;
        rng[2 * lane + 1] = -kEmptyLo;
    }
    if (lane == 0) {  // s = 0: M[0][0] = 0, extended
        Mr[0] = (OffT)extend(q, lq, d, ld, 0, 0);
        rng[0] = 0;
        rng[1] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    const bool conv0 = kend == 0 && (int32_t)Mr[0] >= ld;
    if (T == 0) return conv0 ? 0 : 1;
    if (conv0) return 1;
    auto wrap = [](int32_t v, int32_t r) { return v < 0 ? v + r : v; };
    int32_t sM = 0, sI = 0;  // slot of step t (t % RM, t % RI)
    for (int32_t t = 1; t <= T; ++t) {
        sM = sM + 1 == prm.RM ? 0 : sM + 1;
        sI = sI + 1 == prm.RI ? 0 : sI + 1;
        auto src = [&](int comp, int32_t ts, int32_t slot_now, int32_t back, int32_t ring,
                       int32_t &slot, int32_t &lo, int32_t &hi) __attribute__((always_inline)) {
            if (ts < 0) {
                slot = 0;
                lo = kEmptyLo;
                hi = -kEmptyLo;
                return;
            }
            slot = wrap(slot_now - back, ring);  // back < ring
            lo = rng[2 * (comp * kRingMax + slot)];
            hi = rng[2 * (comp * kRingMax + slot) + 1];
        };
        int32_t soe, loMo, hiMo, sx, loMx, hiMx, sie, loI, hiI, sde, loD, hiD;
        src(0, t - toe, sM, toe, prm.RM, soe, loMo, hiMo);
        src(0, t - tx, sM, tx, prm.RM, sx, loMx, hiMx);
        src(1, t - te, sI, te, prm.RI, sie, loI, hiI);
        src(2, t - te, sI, te, prm.RI, sde, loD, hiD);
        int32_t iLo = max(min(loMo, loI) + 1, -lq), iHi = min(max(hiMo, hiI) + 1, ld);
        int32_t dLo = max(min(loMo, loD) - 1, -lq), dHi = min(max(hiMo, hiD) - 1, ld);
        if (iLo > iHi) iLo = kEmptyLo, iHi = -kEmptyLo;
        if (dLo > dHi) dLo = kEmptyLo, dHi = -kEmptyLo;
        const int32_t xLo = max(loMx, -lq), xHi = min(hiMx, ld);
        const int32_t mLo = min(min(iLo, dLo), xLo <= xHi ? xLo : kEmptyLo);
        const int32_t mHi = max(max(iHi, dHi), xLo <= xHi ? xHi : -kEmptyLo);
        if (mLo > mHi) {  // nothing at this score: no cell, no code the walk can reach
            if (t == T) return 1;
            if (lane == 0) {
                rng[2 * sM] = kEmptyLo, rng[2 * sM + 1] = -kEmptyLo;
                rng[2 * (kRingMax + sI)] = kEmptyLo, rng[2 * (kRingMax + sI) + 1] = -kEmptyLo;
                rng[2 * (2 * kRingMax + sI)] = kEmptyLo, rng[2 * (2 * kRingMax + sI) + 1] = -kEmptyLo;
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        const int32_t span = mHi - mLo;
        // the ring holds W diagonals; a code row holds wt, and the chunks
        // below start at an even diagonal (mLo or mLo - 1)
        if (span + 3 > wt) return 1;
        if (span + 1 > W) return 2;
        auto span_of = [](int32_t lo, int32_t hi) { return (uint32_t)max(hi - lo, 0); };
        const uint32_t spMo = span_of(loMo, hiMo), spMx = span_of(loMx, hiMx);
        const uint32_t spI = span_of(loI, hiI), spD = span_of(loD, hiD);
        // LDS reads are always in bounds (k & wm); an empty source has
        // lo = 2^29 and span 0, so k - lo never passes
        auto rd = [&](const OffT *ring, int32_t slot, int32_t k, int32_t lo,
                      uint32_t sp) __attribute__((always_inline)) {
            const int32_t v = (int32_t)ring[slot * W + (k & wm)];
            return (uint32_t)(k - lo) <= sp ? v : kNeg;
        };
        // an offset h on diagonal k is a cell iff 0 <= h <= ld and h - k <= lq
        auto cell = [&](int32_t h, int32_t k) __attribute__((always_inline)) {
            return max(max(-h, h - ld), h - k - lq) <= 0;
        };
        uint8_t *__restrict__ row = codes + (size_t)(t - 1) * pitch;
        // Chunks of 64 diagonals from an even one, so lanes 2j and 2j + 1
        // hold the two nibbles of one code byte.  Target slots differ from
        // every source slot (RM > max(toe, tx), RI > te), so chunks read and
        // write freely; only diagonals of [mLo, mHi] are written.
        const int32_t kbase = mLo & ~1;
        for (int32_t kc = kbase; kc <= mHi; kc += 64) {  // uniform
            const int32_t k = kc + lane;
            const bool inr = (uint32_t)(k - mLo) <= (uint32_t)span;
            const int32_t Mo_l = rd(Mr, soe, k - 1, loMo, spMo), Ie = rd(Ir, sie, k - 1, loI, spI);
            const int32_t Mo_r = rd(Mr, soe, k + 1, loMo, spMo), De = rd(Dr, sde, k + 1, loD, spD);
            int32_t I = max(Mo_l, Ie) + 1;
            I = cell(I, k) ? I : kNeg;
            int32_t D = max(Mo_r, De);
            D = cell(D, k) ? D : kNeg;
            int32_t X = rd(Mr, sx, k, loMx, spMx) + 1;
            X = cell(X, k) ? X : kNeg;
            int32_t M = max(X, max(I, D));
            uint32_t code = M < 0 ? 0u : X >= max(I, D) ? 1u : I >= D ? 2u : 3u;
            code |= (Ie >= Mo_l ? 4u : 0u) | (De >= Mo_r ? 8u : 0u);
            if (!inr) code = 0, M = kNeg;
            if (M >= 0) M = extend(q, lq, d, ld, M - k, M);
            if (inr) {
                Mr[sM * W + (k & wm)] = (OffT)M;
                Ir[sI * W + (k & wm)] = (OffT)I;
                Dr[sI * W + (k & wm)] = (OffT)D;
            }
            const uint32_t hi_nib = (uint32_t)__shfl_xor((int)code, 1);
            // k is even here and >= mLo - 1; k + 1 <= mHi + 1 < mLo - 1 + wt
            if (!(lane & 1) && k <= mHi) row[(k & (wt - 1)) >> 1] = (uint8_t)(code | (hi_nib << 4));
        }
        if (lane == 0) {
            rng[2 * sM] = mLo, rng[2 * sM + 1] = mHi;
            rng[2 * (kRingMax + sI)] = iLo, rng[2 * (kRingMax + sI) + 1] = iHi;
            rng[2 * (2 * kRingMax + sI)] = dLo, rng[2 * (2 * kRingMax + sI) + 1] = dHi;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        const bool conv = kend >= mLo && kend <= mHi && (int32_t)Mr[sM * W + (kend & wm)] >= ld;
        if (t == T) return conv ? 0 : 1;
        if (conv) return 1;
    }
    return 1;
}

template <typename OffT>
__global__ __launch_bounds__(64) void wfa_affine_trace_kernel(
    const WfaAffTracePair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, WfaAffParams prm, int rerun, uint32_t *__restrict__ next,
    uint8_t *__restrict__ codes, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    // the score kernel's LDS layout (wfa_affine_lds_bytes): ranges, rings, sequences
    int32_t *rng = (int32_t *)lds_raw;
    OffT *Mr = (OffT *)(lds_raw + 2 * 3 * kRingMax * 2 * sizeof(int32_t));
    OffT *Ir = Mr + prm.RM * prm.W;
    OffT *Dr = Ir + prm.RI * prm.W;
    lds_cu8_raw *sbuf = (lds_cu8_raw *)(((uintptr_t)(Dr + prm.RI * prm.W) + 15) & ~(uintptr_t)15);
    const int32_t lane = (int32_t)threadIdx.x;

    for (;;) {
        uint32_t got = 0;
        if (lane == 0) got = __hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t pi = __builtin_amdgcn_readlane(got, 0);
        if (pi >= n_pairs) break;
        const WfaAffTracePair tp = pairs[pi];
        // the second launch takes only what the first ring was too narrow for
        if (rerun && __builtin_amdgcn_readfirstlane(status[tp.p.out]) != kTraceRerun) continue;
        const int32_t lq = (int32_t)tp.p.lq, ld = (int32_t)tp.p.ld, T = (int32_t)tp.p.reserved;
        const uint8_t *__restrict__ q = qs + tp.p.q_off;
        const uint8_t *__restrict__ d = ds + tp.p.d_off;
        uint8_t *__restrict__ pc = codes + tp.code_off;
        const int32_t wt = (int32_t)tp.wt;
        int32_t bad = 0;
        // The ranges grow with the score whatever the sequences hold, so the
        // pair's widest wavefront is known from T (the host's trace_layout):
        // a pair the first ring cannot hold goes to the second launch at once.
        const int32_t score = T * prm.g;
        const int32_t reach = min(score > prm.o ? (score - prm.o) / prm.e : 0, lq + ld);
        if (!rerun && lq != 0 && ld != 0 && min(2 * reach + 1, lq + ld + 1) > prm.W) {
            bad = 2;
        } else if (lq != 0 && ld != 0) {  // a pair with an empty side has no codes
            auto run = [&](const auto &Q, const auto &D) __attribute__((always_inline)) {
                return wfa_trace_pair<OffT>(Q, lq, D, ld, prm, T, rng, Mr, Ir, Dr, pc, wt);
            };
            // staged 2-bit codes, else staged bytes, else HBM
            const int32_t qa = (int32_t)((uintptr_t)q & 15), da = (int32_t)((uintptr_t)d & 15);
            const int32_t qwords = (qa + lq + 15) / 16 + 2, dwords = (da + ld + 15) / 16 + 2;
            const int32_t qspan = (lq + 47) & ~15;  // staged q bytes: +15 lead, +16 tail pad
            bool done = false;
            if (4 * (qwords + dwords) <= prm.seqcap) {
                __builtin_amdgcn_wave_barrier();
                const bool okq = stage_codes(q, lq, sbuf);
                const bool okd = stage_codes(d, ld, sbuf + 4 * qwords);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                if (okq && okd) {
                    const SeqCodes Q{(lds_cu32 *)sbuf, qa};
                    const SeqCodes D{(lds_cu32 *)(sbuf + 4 * qwords), da};
                    bad = run(Q, D);
                    done = true;
                }
            }
            if (!done && qspan + ld + 48 <= prm.seqcap) {
                __builtin_amdgcn_wave_barrier();
                lds_cu8 *lq8 = stage(q, lq, sbuf);
                lds_cu8 *ld8 = stage(d, ld, sbuf + qspan);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                bad = run(SeqBytes<lds_cu8 *>{lq8}, SeqBytes<lds_cu8 *>{ld8});
            } else if (!done) {
                bad = run(SeqBytes<const uint8_t *>{q}, SeqBytes<const uint8_t *>{d});
            }
        }
        if (lane == 0)
            status[tp.p.out] = !bad                 ? (int32_t)SALN_OK
                               : bad == 2 && !rerun ? kTraceRerun
                                                    : (int32_t)SALN_INTERNAL;
        __builtin_amdgcn_wave_barrier();
    }
}

// Appends a run to a pair's CIGAR words, merging it with an equal last op.
struct CigarOut {
    uint32_t *w;
    uint32_t n, cap;
    bool ok;
    __device__ __forceinline__ void add(uint32_t op, uint32_t run) {
        if (!run) return;
        if (n && (w[n - 1] & 15u) == op) {
            w[n - 1] += run << 4;
        } else if (n < cap) {
            w[n++] = (run << 4) | op;
        } else {
            ok = false;
        }
    }
};

// One lane per pair: the walk over the codes and the replay (header comment).
__global__ __launch_bounds__(64) void wfa_affine_walk_kernel(
    const WfaAffTracePair *__restrict__ pairs, uint32_t n_pairs, const uint8_t *__restrict__ qs,
    const uint8_t *__restrict__ ds, WfaAffParams prm, uint8_t *__restrict__ codes,
    int32_t *__restrict__ status, uint32_t *__restrict__ cigar, uint32_t *__restrict__ cigar_len) {
    const uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= n_pairs) return;
    const WfaAffTracePair tp = pairs[pi];
    const int32_t lq = (int32_t)tp.p.lq, ld = (int32_t)tp.p.ld, T = (int32_t)tp.p.reserved;
    CigarOut out{cigar + tp.cig_off, 0u, tp.cig_cap, true};
    if (lq == 0 || ld == 0) {  // one gap run (or nothing)
        out.add(SALN_CIGAR_I, (uint32_t)lq);
        out.add(SALN_CIGAR_D, (uint32_t)ld);
        cigar_len[tp.p.out] = out.n;
        if (!out.ok) status[tp.p.out] = SALN_INTERNAL;
        return;
    }
    cigar_len[tp.p.out] = 0;
    if (status[tp.p.out] != SALN_OK) return;
    const int32_t tx = prm.x / prm.g, toe = (prm.o + prm.e) / prm.g, te = prm.e / prm.g;
    const int32_t wt = (int32_t)tp.wt;
    const size_t pitch = (size_t)(wt >> 1);
    const uint8_t *__restrict__ pc = codes + tp.code_off;
    uint8_t *__restrict__ ops = codes + tp.code_off + (size_t)T * pitch;  // T op bytes
    // walk: (t, k, comp) from (T, ld - lq, M) to (0, 0, M); ops fill from the back
    int32_t t = T, k = ld - lq, comp = 0, n_ops = 0;
    bool closing = false, ok = true;
    for (int64_t it = 0; it < 2 * (int64_t)T + 2 && t > 0 && ok; ++it) {
        const uint32_t byte = pc[(size_t)(t - 1) * pitch + (size_t)((k & (wt - 1)) >> 1)];
        const uint32_t code = (k & 1) ? byte >> 4 : byte & 15u;
        if (comp == 0) {
            const uint32_t s = code & 3u;
            if (s == 0) {
                ok = false;
            } else if (s == 1) {
                if (n_ops == T) ok = false;
                else ops[T - ++n_ops] = (uint8_t)(kOpX | kOpInM);
                t -= tx;
            } else {
                comp = (int32_t)s - 1;  // 1 I, 2 D: same (t, k), its last gap column
                closing = true;
            }
        } else {
            const bool ext = comp == 1 ? (code & 4u) != 0 : (code & 8u) != 0;
            if (n_ops == T) ok = false;
            else ops[T - ++n_ops] = (uint8_t)((comp == 1 ? kOpI : kOpD) | (closing ? kOpInM : 0u));
            closing = false;
            k += comp == 1 ? -1 : 1;
            t -= ext ? te : toe;
            if (!ext) comp = 0;
        }
    }
    if (t != 0 || k != 0 || comp != 0) ok = false;
    // replay
    const uint8_t *__restrict__ q = qs + tp.p.q_off;
    const uint8_t *__restrict__ d = ds + tp.p.d_off;
    const SeqBytes<const uint8_t *> Q{q}, D{d};
    int32_t v = 0, h = 0;
    int64_t pen = 0;
    if (ok) {
        h = extend(Q, lq, D, ld, 0, 0);
        v = h;
        out.add(SALN_CIGAR_EQ, (uint32_t)h);
    }
    bool in_m = true;  // the path is in M before the next op (a gap op then opens)
    uint32_t gap = 0;  // the open gap's op
    for (int32_t j = T - n_ops; j < T && ok; ++j) {
        const uint32_t o = ops[j], op = o & 3u;
        if (op == kOpX) {
            if (v >= lq || h >= ld) { ok = false; break; }
            ++v, ++h;
            pen += prm.x;
            out.add(SALN_CIGAR_X, 1u);
        } else {
            if (!in_m && gap != op) { ok = false; break; }
            if (op == kOpI ? h >= ld : v >= lq) { ok = false; break; }
            pen += prm.e + (in_m ? prm.o : 0);
            if (op == kOpI) ++h, out.add(SALN_CIGAR_D, 1u);
            else ++v, out.add(SALN_CIGAR_I, 1u);
            gap = op;
        }
        in_m = (o & kOpInM) != 0;
        if (in_m) {
            const int32_t h2 = extend(Q, lq, D, ld, v, h);
            out.add(SALN_CIGAR_EQ, (uint32_t)(h2 - h));
            v += h2 - h;
            h = h2;
        }
    }
    if (!in_m || v != lq || h != ld || pen != (int64_t)T * prm.g || !out.ok) ok = false;
    if (ok) {
        cigar_len[tp.p.out] = out.n;
    } else {
        status[tp.p.out] = SALN_INTERNAL;
    }
}

}  // namespace

hipError_t launch_wfa_affine_trace(const WfaAffTracePair *pairs, uint32_t n, const uint8_t *qs,
                                   const uint8_t *ds, const WfaAffParams &prm, bool wide,
                                   bool rerun, uint32_t grid, uint32_t *next, uint8_t *codes,
                                   int32_t *status, hipStream_t stream) {
    if (!n) return hipSuccess;
    const size_t lds = wfa_affine_lds_bytes(prm, wide);
    if (wide)
        wfa_affine_trace_kernel<int32_t><<<dim3(grid), dim3(64), lds, stream>>>(
            pairs, n, qs, ds, prm, (int)rerun, next, codes, status);
    else
        wfa_affine_trace_kernel<int16_t><<<dim3(grid), dim3(64), lds, stream>>>(
            pairs, n, qs, ds, prm, (int)rerun, next, codes, status);
    return hipGetLastError();
}

hipError_t launch_wfa_affine_walk(const WfaAffTracePair *pairs, uint32_t n, const uint8_t *qs,
                                  const uint8_t *ds, const WfaAffParams &prm, uint8_t *codes,
                                  int32_t *status, uint32_t *cigar, uint32_t *cigar_len,
                                  hipStream_t stream) {
    if (!n) return hipSuccess;
    wfa_affine_walk_kernel<<<dim3((n + 63) / 64), dim3(64), 0, stream>>>(
        pairs, n, qs, ds, prm, codes, status, cigar, cigar_len);
    return hipGetLastError();
}

}  // namespace saln
