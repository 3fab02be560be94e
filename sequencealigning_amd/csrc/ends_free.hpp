// Ends-free engine (include/saln.h, saln_ends_free_*): what the host file
// (ends_free_host.cpp) and the kernels (ends_free_kernels.hip,
// ends_free_long_kernels.hip) share.  Device side: ends_free_dev.hpp has what
// the fills and the walk share (the trace code), ends_free_fill.hpp the fill
// itself, which both fill kernels are built from.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "saln.h"

namespace saln {

// One pair of a launch.  code_off / cig_off: the pair's trace codes (bytes)
// and CIGAR word area (words) in the chunk's workspaces; out: its record in
// the results array.
struct EfPair {
    uint64_t q_off, d_off, code_off, cig_off;
    uint32_t lq, ld, out, row_bytes;
};
static_assert(sizeof(EfPair) == 48, "EfPair layout");

struct EfScoring {
    int32_t match, mismatch, open, extend;
};

// The run-time mode as a compile-time constant: f(std::integral_constant<int,
// SALN_MODE_...>{}) for the engine's four modes, hipErrorInvalidValue for
// anything else.  Every kernel template's instances are picked through it.
template <class F>
hipError_t ef_with_mode(int32_t mode, F &&f) {
    switch (mode) {
        case SALN_MODE_LOCAL: return f(std::integral_constant<int, SALN_MODE_LOCAL>{});
        case SALN_MODE_OVERLAP: return f(std::integral_constant<int, SALN_MODE_OVERLAP>{});
        case SALN_MODE_SEMI_GLOBAL: return f(std::integral_constant<int, SALN_MODE_SEMI_GLOBAL>{});
        case SALN_MODE_EXTEND: return f(std::integral_constant<int, SALN_MODE_EXTEND>{});
        default: return hipErrorInvalidValue;
    }
}

// A run-time flag as a compile-time constant, in ef_with_mode's style:
// f(std::bool_constant<flag>{}).
template <class F>
hipError_t ef_with_flag(bool flag, F &&f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

// Scoring under a substitution matrix (saln_sub_matrix, saln_ends_free_sub_*):
// one device block per batch or plan, which the fills with kSub copy into LDS
// once per workgroup.
//   bytes 0 .. 255   code[]: byte -> symbol, every entry < n_sym <= 32
//   then 32 rows (db symbol) of kEfSubStride bytes: score[db][query] in columns
//   0 .. 31 and the pad column kEfSubPad.
// Invariant: the pad column is strictly negative in every row (kEfSubPadScore).
// Pad columns past the query take part in local's running best without a
// mask; that is safe only because a pad cell's M = P(i-1, j-1) + s lies
// strictly below a P of the pair, hence below some real M or at most 0, which
// needs s < 0 whatever the matrix holds (extension's tracker, without the
// floor, rests on the same column: ef_row in ends_free_fill.hpp has the
// argument).  Entries outside n_sym x n_sym are
// never indexed (code[] is total and checked on the host) and hold the pad
// score too.
// Stride: the lanes of a group stand on different rows, so their row bases
// differ.  A 32-byte stride would put row r on bank 8 r mod 32, four distinct
// bases for 32 rows; 36 bytes (9 dwords, odd) puts the 32 rows on 32 distinct
// banks.
constexpr uint32_t kEfSubSyms = 32, kEfSubPad = 32, kEfSubStride = 36;
constexpr int8_t kEfSubPadScore = -1;
constexpr uint32_t kEfSubCodeBytes = 256;
constexpr uint32_t kEfSubBytes = kEfSubCodeBytes + kEfSubSyms * kEfSubStride;  // 1,408
static_assert(kEfSubPad < kEfSubStride && kEfSubBytes % 16 == 0, "table layout");

// Query classes: one pair per group of `lanes` lanes, `cols` query columns per
// lane, the whole query in one chunk (the i32 lane classes of the NW table).
struct EfClass {
    int32_t lanes, cols;
};
constexpr int kEfClasses = 4;
constexpr EfClass kEfClass[kEfClasses] = {{16, 10}, {16, 16}, {64, 8}, {64, 16}};
constexpr uint64_t kEfMaxQ = 1024;   // longest query (kEfClass's widest class)
constexpr uint64_t kEfMaxDb = 65000; // longest db: a group's db row is staged in LDS

// The class a query of len_q columns runs in (-1: above kEfMaxQ).  The one
// place the decision is made: saln_ends_free_pair_geometry, the code sizes
// and the launches all ask it.
inline int ef_class_of(uint64_t len_q) {
    for (int c = 0; c < kEfClasses; ++c)
        if (len_q <= (uint64_t)kEfClass[c].lanes * (uint64_t)kEfClass[c].cols) return c;
    return -1;
}

// Bytes of one code row of a pair (4 bits per cell): the lanes that hold a
// query column store cols / 2 bytes each.
inline uint32_t ef_row_bytes(uint64_t len_q) {
    const int c = ef_class_of(len_q);
    if (c < 0 || len_q == 0) return 0;
    const uint64_t k = (uint64_t)kEfClass[c].cols;
    return (uint32_t)((len_q + k - 1) / k * (k / 2));
}

// The chunked fill (ends_free_long_kernels.hip, saln_ends_free_long_*): the
// 64 x 16 class run over chunks of kEfChunkCols query columns, the db read as
// it goes.  It takes the pairs the classes refuse.
constexpr int kEfLongClass = kEfClasses;
constexpr uint64_t kEfChunkCols = 1024;
static_assert(kEfChunkCols == kEfMaxQ, "a chunk is the widest class");

// The fill a pair runs in: its class, kEfLongClass, or -1 (refused).  long_ok:
// the caller is a saln_ends_free_long_* entry point.  The one place the
// decision is made: saln_ends_free_long_pair_path, the code sizes and the
// launches all ask it.
inline int ef_path_of(uint64_t len_q, uint64_t len_db, bool long_ok) {
    if (len_q <= kEfMaxQ && len_db <= kEfMaxDb) return ef_class_of(len_q);
    return long_ok ? kEfLongClass : -1;
}

// Bytes of one code row under the chunked fill: 8 per lane that holds a column.
inline uint64_t ef_long_row_bytes(uint64_t len_q) { return (len_q + 15) / 16 * 8; }
inline uint64_t ef_path_row_bytes(int path, uint64_t len_q) {
    return path == kEfLongClass ? ef_long_row_bytes(len_q) : ef_row_bytes(len_q);
}

// Boundary workspace of the chunked fill.  Every wave of a launch owns one
// slot, a column of 8 bytes per row of the launch's longest db, and takes
// pairs from a counter; a launch runs min(pairs, kEfLongWaves,
// kEfLongWorkspace / slot bytes) waves and at least one, so the workspace
// stays within kEfLongWorkspace however large the batch is, except for a
// single db whose column alone exceeds it.
constexpr uint64_t kEfLongWorkspace = 256ull << 20;
constexpr uint32_t kEfLongWaves = 4096;
inline uint32_t ef_long_slots(uint64_t count, uint64_t ld_max) {
    const uint64_t fit = kEfLongWorkspace / (8 * (ld_max ? ld_max : 1));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({count, kEfLongWaves, fit}));
}

// The same for the chunked X-drop fill (ends_free_xdrop_long_kernels.hip,
// saln_ends_free_xdrop_long_*): an entry also holds B, 16 bytes per row, so
// half as many slots fit the same kEfLongWorkspace.
constexpr uint32_t kEfXdropBndBytes = 16;
inline uint32_t ef_xdrop_long_slots(uint64_t count, uint64_t ld_max) {
    const uint64_t fit = kEfLongWorkspace / (kEfXdropBndBytes * (ld_max ? ld_max : 1));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({count, kEfLongWaves, fit}));
}

// Tiled replay traceback (ends_free_replay_kernels.hip, saln_ends_free_replay_*,
// DESIGN.md section 3e): what a pair of the chunked path keeps in place of its
// codes, from the pair's code_off on.  R: rows of a tile (a power of two).
//   cols   the boundary columns 0 .. chunks - 2 (column c: P(r, c0), I(r, c0 + 1)
//          of c0 = (c + 1) * 1024 for the rows 1 .. ld), ld int2 each
//   cps    the checkpoint rows 0 .. (ld - 1) / R - 1 (row R * (n + 1): P(r, j),
//          D(r + 1, j) of every column of every chunk), chunks * 1024 int2 each
//   tile   the codes of the tile in work, R rows of kEfTileRowBytes
// All three are multiples of 8 bytes.  A pair without a cell keeps nothing.
constexpr uint32_t kEfTileRowBytes = (uint32_t)(kEfChunkCols / 2);
struct EfReplayLayout {
    uint64_t cols, cps, tile, bytes;  // byte offsets of the parts, and the whole
};
__host__ __device__ inline EfReplayLayout ef_replay_layout(uint64_t lq, uint64_t ld, uint64_t R) {
    if (lq == 0 || ld == 0) return EfReplayLayout{0, 0, 0, 0};
    const uint64_t chunks = (lq + kEfChunkCols - 1) / kEfChunkCols;
    EfReplayLayout l;
    l.cols = 0;
    l.cps = (chunks - 1) * ld * 8;
    l.tile = l.cps + (ld - 1) / R * chunks * kEfChunkCols * 8;
    l.bytes = l.tile + R * kEfTileRowBytes;
    return l;
}
// The same for the X-drop extension (ends_free_xdrop_replay_kernels.hip,
// saln_ends_free_xdrop_replay_*): every entry also holds
// B, one int4 each, and a header per chunk tells which rows the chunk ran.
//   hdr    one int4 per chunk: (lo_c, z_c, Bs = B(lo_c - 1, .), 1), or all 0 for
//          a chunk that did not run
//   cols   the boundary columns 0 .. chunks - 2: (P(r, c0), I(r, c0 + 1),
//          B(r, c0), 0), the chunked X-drop fill's entries, ld each
//   cps    the checkpoint rows: (P(r, j), D(r + 1, j), B(r, j), 0), chunks * 1024 each
//   tile   the codes of the tile in work
// Only the rows lo_c .. z_c of a chunk that ran are written (columns: of chunk
// c's own window); everything else in the area is stale memory, and the tile
// fill reads nothing outside them.  All four are multiples of 16 bytes; the
// area itself starts 16-byte aligned (ef_align_batch).
struct EfXdropReplayLayout {
    uint64_t hdr, cols, cps, tile, bytes;
};
__host__ __device__ inline EfXdropReplayLayout ef_xdrop_replay_layout(uint64_t lq, uint64_t ld, uint64_t R) {
    if (lq == 0 || ld == 0) return EfXdropReplayLayout{0, 0, 0, 0, 0};
    const uint64_t chunks = (lq + kEfChunkCols - 1) / kEfChunkCols;
    EfXdropReplayLayout l;
    l.hdr = 0;
    l.cols = chunks * 16;
    l.cps = l.cols + (chunks - 1) * ld * kEfXdropBndBytes;
    l.tile = l.cps + (ld - 1) / R * chunks * kEfChunkCols * 16;
    l.bytes = l.tile + R * kEfTileRowBytes;
    return l;
}
inline bool ef_tile_rows_ok(int64_t R) {
    return R == 64 || R == 128 || R == 256 || R == 512 || R == 1024;
}

// The resumable walk's state of one pair between two launches.
struct EfWalkState {
    uint32_t i, j;      // the cell the walk stands on, or whose code it waits for
    uint32_t st, pend;  // state (0 M, 1 I, 2 D); the read still owed: kEfPend*
    uint32_t run, op;   // the open run of words
    uint32_t n, done;   // words written; 1: the record is final
};
static_assert(sizeof(EfWalkState) == 32, "EfWalkState layout");
constexpr uint32_t kEfPendNone = 0, kEfPendArg = 1, kEfPendIExt = 2, kEfPendDExt = 3;

// Dynamic LDS of a fill workgroup of `groups` lane groups: each group's db
// row, padded by `lanes` bytes on both sides (the skew reads past the ends).
inline uint64_t ef_lds_bytes(int cls, uint32_t groups, uint32_t ld_max) {
    return (uint64_t)groups * ((uint64_t)ld_max + 2u * (uint32_t)kEfClass[cls].lanes);
}

// The workgroup of a class fill whose longest db has ld_max rows: as many lane
// groups (of at most 256 lanes together) as 64 KB of LDS stage rows for.  The
// matrix block comes out of the same 64 KB; a single group's row of the
// longest dbs goes up to kEfSubBytes above them, far below a CU's LDS.  The
// one place the decision is made: saln_ends_free_fill_geometry and the launch
// both ask it.
struct EfFillGeometry {
    uint32_t groups;
    uint64_t lds_bytes;  // ef_lds_bytes of them: the launch's dynamic LDS
};
inline EfFillGeometry ef_fill_geometry(int cls, uint32_t ld_max, bool has_matrix) {
    const uint64_t budget = (64u << 10) - (has_matrix ? kEfSubBytes : 0u);
    uint32_t groups = 256u / (uint32_t)kEfClass[cls].lanes;
    while (groups > 1 && ef_lds_bytes(cls, groups, ld_max) > budget) --groups;
    return EfFillGeometry{groups, ef_lds_bytes(cls, groups, ld_max)};
}

// Every fill below takes `sub` after the scoring: nullptr runs the
// match / mismatch instances and reads sc whole; a device block of kEfSubBytes
// (above) runs the kSub instances, which read sc.open and sc.extend only.

// Fill of pairs[first .. first + count), all of class cls with dbs of at most
// ld_max rows.  mode: SALN_MODE_LOCAL, _SEMI_GLOBAL, _OVERLAP or _EXTEND (the
// host has checked it).  codes == nullptr: score only.  end_state (with codes): the
// state of each pair's end cell (0 M, 1 I), indexed like results; overlap's
// walk takes it from the end cell's own code instead.  xdrop: kEfNoXdrop, or
// X >= 0 with SALN_MODE_EXTEND: the X-drop instances (saln_ends_free_xdrop_*),
// which also leave their row-loop steps in the records' `reserved`.
constexpr int32_t kEfNoXdrop = -1;
hipError_t launch_ef_fill(int cls, int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                          uint32_t ld_max, const uint8_t *qs, const uint8_t *ds, EfScoring sc,
                          const uint8_t *sub, uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results,
                          hipStream_t s, int32_t xdrop = kEfNoXdrop);
// Chunked fill of pairs[first .. first + count) (any lengths): `slots` waves,
// each with slot_rows (>= the longest db) 8-byte entries of bnd, taking pairs
// from *counter, which the caller has zeroed on the stream.
hipError_t launch_ef_fill_long(int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                               const uint8_t *qs, const uint8_t *ds, EfScoring sc, const uint8_t *sub,
                               uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results, void *bnd,
                               uint64_t slot_rows, uint32_t slots, uint32_t *counter, hipStream_t s);
// Chunked X-drop extension fill (SALN_MODE_EXTEND, xdrop = X >= 0) of
// pairs[first .. first + count): as launch_ef_fill_long, with slot_rows entries
// of kEfXdropBndBytes per slot; leaves the pairs' row-loop steps, summed over
// the chunks they ran, in the records' `reserved`.
hipError_t launch_ef_xdrop_fill_long(const EfPair *pairs, uint32_t first, uint32_t count, const uint8_t *qs,
                                     const uint8_t *ds, EfScoring sc, const uint8_t *sub, int32_t xdrop,
                                     uint8_t *codes, uint8_t *end_state, saln_ends_free_result *results,
                                     void *bnd, uint64_t slot_rows, uint32_t slots, uint32_t *counter,
                                     hipStream_t s);
// The forward pass of the tiled replay: the chunked fill, score only, of
// pairs[first .. first + count), keeping each pair's boundary columns and
// checkpoint rows at area + code_off (ef_replay_layout with tile_rows) and its
// end state.  `slots` waves take pairs from *counter (zeroed on the stream).
hipError_t launch_ef_fill_keep(int32_t mode, const EfPair *pairs, uint32_t first, uint32_t count,
                               const uint8_t *qs, const uint8_t *ds, EfScoring sc, const uint8_t *sub,
                               uint8_t *area, uint32_t tile_rows, uint8_t *end_state,
                               saln_ends_free_result *results, uint32_t slots, uint32_t *counter, hipStream_t s);
// The replay's rounds over pairs[0 .. count), all of the chunked path, state
// and lens indexed like pairs.  Start: the walk up to its first code read.
// Tile: one wave per unfinished pair fills the tile of the cell it waits for.
// Walk: every unfinished pair walks inside that tile, and finishes (record,
// lens) or leaves it for a tile up or left.
hipError_t launch_ef_replay_start(int32_t mode, const EfPair *pairs, uint32_t count,
                                  const uint8_t *qs, const uint8_t *ds, const uint8_t *end_state,
                                  saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                                  EfWalkState *state, hipStream_t s);
hipError_t launch_ef_tile_fill(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                               const uint8_t *ds, EfScoring sc, const uint8_t *sub, uint8_t *area,
                               uint32_t tile_rows, const EfWalkState *state, hipStream_t s);
hipError_t launch_ef_tile_walk(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                               const uint8_t *ds, const uint8_t *area, uint32_t tile_rows,
                               saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                               EfWalkState *state, hipStream_t s);
// The X-drop forms of the forward pass and of the tile fill (SALN_MODE_EXTEND,
// xdrop = X >= 0; ends_free_xdrop_replay_kernels.hip): the area is
// ef_xdrop_replay_layout's, the records' `reserved` holds the forward pass's
// row-loop steps, and the walk is launch_ef_replay_start / launch_ef_tile_walk.
hipError_t launch_ef_xdrop_fill_keep(const EfPair *pairs, uint32_t first, uint32_t count, const uint8_t *qs,
                                     const uint8_t *ds, EfScoring sc, const uint8_t *sub, int32_t xdrop,
                                     uint8_t *area, uint32_t tile_rows, uint8_t *end_state,
                                     saln_ends_free_result *results, uint32_t slots, uint32_t *counter,
                                     hipStream_t s);
hipError_t launch_ef_xdrop_tile_fill(const EfPair *pairs, uint32_t count, const uint8_t *qs, const uint8_t *ds,
                                     EfScoring sc, const uint8_t *sub, int32_t xdrop, uint8_t *area,
                                     uint32_t tile_rows, const EfWalkState *state, hipStream_t s);
// Walk of pairs[0 .. count): one pair per lane, from the end cell the fill
// reported.  A pair's words end at words[cig_off + lq + ld), cigar_len of
// them (also in lens, indexed like pairs).
hipError_t launch_ef_walk(int32_t mode, const EfPair *pairs, uint32_t count, const uint8_t *qs,
                          const uint8_t *ds, const uint8_t *codes, const uint8_t *end_state,
                          saln_ends_free_result *results, uint32_t *words, uint32_t *lens,
                          hipStream_t s);
// Packs those words: pair k's lens[k] words to out[dst[k] ..).
hipError_t launch_ef_gather(const EfPair *pairs, uint32_t count, const uint32_t *words,
                            const uint32_t *lens, const uint64_t *dst, uint32_t *out,
                            hipStream_t s);

}  // namespace saln
