// Device helpers shared by the fills and the walk of the ends-free engine:
// the 4-bit trace code of a cell and where it lives, -infinity and its
// arithmetic, the lane hand-over.  The fill's own steps (row 0, a row, the end
// cell) are in ends_free_fill.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ends_free.hpp"

namespace saln {

// Code of cell (i, j), 1 <= i <= len_db, 1 <= j <= len_q:
//   bits 0-1  the first of M, I, D (0, 1, 2) equal to max(M, I, D) at the cell:
//             the state a walk arriving by a diagonal step continues in;
//             3 (local only): max(M, I, D) <= 0, the walk stops here
//   bit 2     I(i, j+1) extends I(i, j) (clear: it opens from M(i, j))
//   bit 3     D(i+1, j) extends D(i, j) (clear: it opens from M(i, j))
// Extend wins a tie with open.  Row i-1 of a pair starts at byte
// code_off + (i-1) * row_bytes; column j is nibble (j-1) of the row, low
// nibble first.
constexpr uint32_t kEfArgMask = 3u, kEfStop = 3u, kEfIExt = 4u, kEfDExt = 8u;

// -infinity of the recurrences.  Every real value lies above it: a batch
// whose values could reach 2^30 in magnitude is refused by the host.
constexpr int32_t kEfNeg = -(1 << 30);

__device__ __forceinline__ uint32_t ef_code(const uint8_t *codes, const EfPair &p, uint32_t i,
                                            uint32_t j) {
    const uint8_t b = codes[p.code_off + (uint64_t)(i - 1) * p.row_bytes + ((j - 1) >> 1)];
    return (b >> (((j - 1) & 1u) * 4u)) & 15u;
}

// a + b with wrap-around: the pad columns past the query carry values that
// are never read and may leave the int32 range.
__device__ __forceinline__ int32_t ef_add(int32_t a, int32_t b) {
    return (int32_t)((uint32_t)a + (uint32_t)b);
}

// lane i <- lane i-1 within the group of G lanes; the group's lane 0 keeps `old`.
template <int G>
__device__ __forceinline__ int32_t ef_shr1(int32_t old, int32_t v) {
    static_assert(G == 16 || G == 64, "group must be a DPP row or the wave");
    if constexpr (G == 16)
        return __builtin_amdgcn_update_dpp(old, v, 0x111 /*row_shr:1*/, 0xf, 0xf, false);
    else
        return __builtin_amdgcn_update_dpp(old, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}

}  // namespace saln
