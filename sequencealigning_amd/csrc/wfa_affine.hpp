// Shared host/device definitions of the corrected gap-affine WFA engine
// (wfa_affine_kernels.hip, wfa_affine_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace saln {

struct WfaAffPair {  // 32 bytes
    uint64_t q_off, d_off;
    uint32_t lq, ld;
    uint32_t out;  // index into scores
    uint32_t reserved;
};

struct WfaAffParams {
    int32_t x, o, e;     // mismatch, gap open, gap extend (gap of length L: o + L*e)
    int32_t g;           // gcd(x, o+e, e): scores step in units of g
    int32_t RM, RI;      // ring slots: M (max(x, o+e)/g + 1), I/D (e/g + 1)
    int32_t W;           // diagonals per wavefront slot (power of two)
    int32_t max_score;   // give up above this penalty (score -1)
    int32_t seqcap;      // LDS bytes for a pair's staged sequences (0: read them from HBM)
};

size_t wfa_affine_lds_bytes(const WfaAffParams &prm, bool wide);
// n_dev (optional): the pair count is read from device memory (n bounds it)
// next: a zeroed device counter the launch's waves take pair indices from
hipError_t launch_wfa_affine(const WfaAffPair *pairs, uint32_t n, const uint8_t *qs,
                             const uint8_t *ds, const WfaAffParams &prm, bool wide,
                             uint32_t grid, const uint32_t *n_dev, uint32_t *next, int32_t *scores,
                             hipStream_t stream);
hipError_t launch_wfa_affine_compact(const WfaAffPair *pairs, uint32_t n, const int32_t *scores,
                                     WfaAffPair *out, uint32_t *count, hipStream_t stream);

// Alignment mode (wfa_affine_trace_kernels.hip).  One pair of a trace chunk:
// p.out indexes the chunk's status / cigar_len arrays, p.reserved is the
// pair's step count T = penalty / g.
struct WfaAffTracePair {  // 64 bytes
    WfaAffPair p;
    uint64_t code_off;  // the pair's code area in the chunk's workspace (bytes)
    uint64_t cig_off;   // its CIGAR words in the chunk's word buffer
    uint32_t wt;        // diagonals per code row (a power of two; the row pitch is wt / 2 bytes)
    uint32_t cig_cap;   // words at cig_off (2 T + 1)
    uint32_t pad[2];
};
// Trace fill of the chunk's pairs with prm's ring (W, seqcap); next: a zeroed
// device counter.  First launch (rerun false): every pair; status[p.out] =
// SALN_OK, SALN_INTERNAL, or kTraceRerun where the ring was too narrow.
// Second launch (rerun true, the wider ring): the kTraceRerun pairs only.
constexpr int32_t kTraceRerun = -100;
hipError_t launch_wfa_affine_trace(const WfaAffTracePair *pairs, uint32_t n, const uint8_t *qs,
                                   const uint8_t *ds, const WfaAffParams &prm, bool wide,
                                   bool rerun, uint32_t grid, uint32_t *next, uint8_t *codes,
                                   int32_t *status, hipStream_t stream);
// Walk + replay of every pair of the chunk (after its fills): CIGAR words at
// cig_off, their count in cigar_len[p.out]; status SALN_OK or not.
hipError_t launch_wfa_affine_walk(const WfaAffTracePair *pairs, uint32_t n, const uint8_t *qs,
                                  const uint8_t *ds, const WfaAffParams &prm, uint8_t *codes,
                                  int32_t *status, uint32_t *cigar, uint32_t *cigar_len,
                                  hipStream_t stream);

}  // namespace saln
