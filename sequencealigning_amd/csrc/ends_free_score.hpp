// Score-only search of the ends-free engine (include/saln.h,
// saln_ends_free_score_*): what the host file
// (ends_free_score_host.cpp) and the packed-i16 fill
// (ends_free_score_kernels.hip) share.  HIP-free but for the launch
// declarations.
#pragma once
#include "ends_free.hpp"

namespace saln {

// One lane group of a packed launch: pair A in the low 16 bits of every
// register, pair B in the high 16 bits, both of the launch's class.  A group
// with one pair has n_b = m_b = 0, offsets 0 and out_b = kEfPkNone: nothing of
// B is read and nothing is written for it.
struct EfPkGroup {
    uint64_t qa_off, da_off, qb_off, db_off;
    uint32_t n_a, m_a, n_b, m_b, out_a, out_b;  // out: the pair's index in the caller's order
    uint32_t pad[2];
};
static_assert(sizeof(EfPkGroup) == 64, "EfPkGroup layout");
constexpr uint32_t kEfPkNone = 0xFFFFFFFFu;

// Does a pair of n columns and m rows run the packed fill?  max_pos (S+): the
// largest positive s(i, j); max_abs (A): the largest |parameter|, gaps
// included.  Local and semi-global only, and only while every value the kernel
// forms stays inside int16 (DESIGN.md section 3l has the proof):
//   min(n, m) S+ + 4 A < 2^15          both modes
//   (n + 4) A < 2^15                   semi-global
// The one place the decision is made: saln_ends_free_score_path and the plan
// both ask it.
inline bool ef_score_packed(uint64_t n, uint64_t m, int32_t mode, uint64_t max_pos, uint64_t max_abs) {
    if (mode != SALN_MODE_LOCAL && mode != SALN_MODE_SEMI_GLOBAL) return false;
    if (n > kEfMaxQ || m > kEfMaxDb || max_pos > (1u << 15) || max_abs > (1u << 15)) return false;
    if (std::min(n, m) * max_pos + 4 * max_abs >= (1u << 15)) return false;
    if (mode == SALN_MODE_SEMI_GLOBAL && (n + 4) * max_abs >= (1u << 15)) return false;
    return true;
}

// Dynamic LDS of a packed workgroup of `groups` lane groups: each group's two
// db rows, interleaved (one 16-bit entry per row: A's byte low, B's high),
// padded by `lanes` entries on both sides as the class fill's row is.
inline uint64_t ef_score_lds_bytes(int cls, uint32_t groups, uint32_t ld_max) {
    return (uint64_t)groups * 2u * ((uint64_t)ld_max + 2u * (uint32_t)kEfClass[cls].lanes);
}

// The workgroup of a packed launch: ef_fill_geometry's rule over rows of twice
// the bytes.  A single group of the longest dbs takes 130,256 bytes (and the
// matrix block), below a CU's 160 KB.  The one place the decision is made:
// saln_ends_free_score_geometry and the launch both ask it.
inline EfFillGeometry ef_score_geometry(int cls, uint32_t ld_max, bool has_matrix) {
    const uint64_t budget = (64u << 10) - (has_matrix ? kEfSubBytes : 0u);
    uint32_t groups = 256u / (uint32_t)kEfClass[cls].lanes;
    while (groups > 1 && ef_score_lds_bytes(cls, groups, ld_max) > budget) --groups;
    return EfFillGeometry{groups, ef_score_lds_bytes(cls, groups, ld_max)};
}

// Packed fill of groups[first .. first + count), all of class cls with dbs of
// at most ld_max rows; mode SALN_MODE_LOCAL or SALN_MODE_SEMI_GLOBAL.  sub:
// nullptr or the matrix's device block (ends_free.hpp).  Writes one int32 per
// pair at scores[out].
hipError_t launch_ef_score_pk(int cls, int32_t mode, const EfPkGroup *groups, uint32_t first, uint32_t count,
                              uint32_t ld_max, const uint8_t *qs, const uint8_t *ds, EfScoring sc,
                              const uint8_t *sub, int32_t *scores, hipStream_t s);
// scores[out[k]] = results[k].score for k < count: the i32 fills' records into
// the caller's order.
hipError_t launch_ef_score_gather(const saln_ends_free_result *results, const uint32_t *out, uint32_t count,
                                  int32_t *scores, hipStream_t s);

}  // namespace saln
