// Device helpers shared by the corrected gap-affine WFA kernels
// (wfa_affine_kernels.hip: score only; wfa_affine_trace_kernels.hip: score
// and alignment): the LDS ring's constants, the sequence views the extension
// reads (bytes in HBM or LDS, 2-bit codes in LDS), extend, and the staging of
// a pair's sequences into LDS.  Device code only; include from a .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

namespace saln {

namespace {

constexpr int kRingMax = 16;
// An empty range is (kEmptyLo, -kEmptyLo): min / max of ranges and the +-1
// of the recurrences keep it empty without tests.
constexpr int32_t kEmptyLo = 1 << 29;
typedef __attribute__((address_space(3))) uint8_t lds_cu8_raw;
typedef const lds_cu8_raw lds_cu8;
typedef const __attribute__((address_space(3))) uint32_t lds_cu32;

template <typename OffT>
struct OffTraits;
template <>
struct OffTraits<int16_t> {
    static constexpr int32_t kNeg = -32768;
};
template <>
struct OffTraits<int32_t> {
    static constexpr int32_t kNeg = INT32_MIN / 4;
};

// 4 bytes at p (4-aligned or not) from the two aligned dwords covering them.
// Global sequences: both dwords hold a byte of the sequence (callers check 5
// readable bytes at p), so nothing past the sequence's last dword is read.
// LDS sequences: the staged copy is padded.
template <typename P>
__device__ __forceinline__ uint32_t load4(P p) {
    const uintptr_t a = (uintptr_t)p;
    typedef typename std::remove_pointer<P>::type cu8;
    typedef typename std::conditional<std::is_same<cu8, const lds_cu8>::value, const lds_cu32,
                                      const uint32_t>::type cu32;
    cu32 *w = (cu32 *)(a & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(a & 3));
}

// A sequence as the extension reads it: chunk(i) holds bases i, i+1, ... in
// kStep fields of kBits bits (equal bases <=> equal fields), at(i) one base.
// Bytes (global memory or staged in LDS): 4 bases per chunk; a chunk at i
// needs bytes i .. i+4 readable (kNeed).
template <typename P>
struct SeqBytes {
    P p;
    static constexpr int32_t kStep = 4, kShift = 3, kNeed = 5;
    __device__ __forceinline__ uint32_t chunk(int32_t i) const { return load4(p + i); }
    __device__ __forceinline__ uint32_t at(int32_t i) const { return p[i]; }
};
// 2-bit codes staged in LDS ((c >> 1) & 3: A 0, C 1, T 2, G 3): word w holds
// the codes of the 16 bytes at the sequence's 16-byte-aligned base + 16 w,
// off = the sequence's start within the first word.  A chunk is 16 bases
// (a funnel shift of two words; the staged words are padded by two).
struct SeqCodes {
    lds_cu32 *w;
    int32_t off;
    static constexpr int32_t kStep = 16, kShift = 1, kNeed = 16;
    __device__ __forceinline__ uint32_t chunk(int32_t i) const {
        const uint32_t j = (uint32_t)(i + off);
        const uint64_t pair = ((uint64_t)w[(j >> 4) + 1] << 32) | w[j >> 4];
        return (uint32_t)(pair >> (2u * (j & 15u)));
    }
    __device__ __forceinline__ uint32_t at(int32_t i) const {
        const uint32_t j = (uint32_t)(i + off);
        return (w[j >> 4] >> (2u * (j & 15u))) & 3u;
    }
};

// Extend (v, h) along matching bases: returns the new text offset.
template <typename S>
__device__ __forceinline__ int32_t extend(const S &q, int32_t lq, const S &d, int32_t ld, int32_t v,
                                          int32_t h) {
    for (;;) {
        if (v + S::kNeed <= lq && h + S::kNeed <= ld) {
            const uint32_t x = q.chunk(v) ^ d.chunk(h);
            if (x) return h + (int32_t)(__builtin_ctz(x) >> S::kShift);
            v += S::kStep;
            h += S::kStep;
        } else {
            while (v < lq && h < ld && q.at(v) == d.at(h)) {
                ++v;
                ++h;
            }
            return h;
        }
    }
}

// Copy len bytes at src into LDS at dst (16-byte granules from src & ~15,
// so the copy starts at dst + (src & 15)); returns the staged pointer.
__device__ __forceinline__ lds_cu8 *stage(const uint8_t *src, int32_t len, lds_cu8_raw *dst) {
    const uintptr_t a = (uintptr_t)src, base = a & ~(uintptr_t)15;
    const int32_t nblk = (int32_t)((((a + (uintptr_t)len + 15) & ~(uintptr_t)15) - base) / 16);
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    for (int32_t i = (int32_t)threadIdx.x; i < nblk; i += 64) {
        const uint4 v = ((const uint4 *)base)[i];
        lds_u32 *w = (lds_u32 *)dst + 4 * i;
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    return dst + (a & 15);
}

// The 2-bit codes of len bytes at src into LDS words at dst (word i: the 16
// bytes at (src & ~15) + 16 i), two zero words after them; returns whether
// every byte of the sequence is A, C, G or T (wave-uniform).
__device__ __forceinline__ bool stage_codes(const uint8_t *src, int32_t len, lds_cu8_raw *dst) {
    const uintptr_t a = (uintptr_t)src, base = a & ~(uintptr_t)15;
    const int32_t off = (int32_t)(a & 15);
    const int32_t nblk = (off + len + 15) / 16;
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    lds_u32 *w = (lds_u32 *)dst;
    bool bad = false;
    for (int32_t i = (int32_t)threadIdx.x; i < nblk + 2; i += 64) {
        uint32_t code = 0;
        if (i < nblk) {
            const uint4 v = ((const uint4 *)base)[i];
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t y = (x[k] >> 1) & 0x03030303u;
                code |= ((y * 0x00041041u) >> 18 & 0xFFu) << (8u * k);
#pragma unroll
                for (int b = 0; b < 4; ++b) {  // the sequence's bytes must be A, C, G, T
                    const int32_t pos = 16 * i + 4 * k + b - off;
                    const uint32_t c = (x[k] >> (8 * b)) & 0xFFu;
                    const bool acgt = c == 'A' || c == 'C' || c == 'G' || c == 'T';
                    bad |= pos >= 0 && pos < len && !acgt;
                }
            }
        }
        w[i] = code;
    }
    return !__builtin_amdgcn_ballot_w64(bad);
}

}  // namespace

}  // namespace saln
