/*
 * saln — MI355X-native drop-in engine for the NW-affine (and WFA) hot path of
 * Qw11111111111/SequenceAligning.
 *
 * C ABI only: plain pointers, sizes and POD structs; no C++ or torch types.
 * Every entry point names the reference interface it replaces.  The
 * reference is Rust (src/main.rs dispatches to free functions), so the
 * binding a maintainer adds is an `extern "C"` block in Rust — see
 * INTEGRATION.md.
 *
 * Orientation (reference convention, needleman_wunsch_affine.rs:424-430):
 *   seq1 = query  -> y, columns, inner loop
 *   seq2 = db     -> x, rows,    outer loop
 */
#ifndef SALN_H
#define SALN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALN_ABI_VERSION 1

/* Mode — src/parse.rs:44-50 (declaration order Global, Local, SemiGlobal).
 * SALN_MODE_OVERLAP is this library's own (the ends-free engine, below): no
 * reference name, and 3 stays an unknown mode. */
typedef enum {
    SALN_MODE_GLOBAL = 0,
    SALN_MODE_LOCAL = 1,
    SALN_MODE_SEMI_GLOBAL = 2,
    SALN_MODE_OVERLAP = 4
} saln_mode;
/* Extension alignment of the ends-free engine (below): pinned at the origin,
 * free at its end.  A macro beside the enum, not a member of it: saln_mode
 * mirrors the reference's Mode plus overlap, and its list of members is
 * pinned as it stands.  Every `int32_t mode` of saln_ends_free_* takes it. */
#define SALN_MODE_EXTEND 8

/* Per-pair status and API return codes.  The reference returns
 * AlignerError values (src/errors.rs:7-15) or panics (aborting the whole
 * process, exit 101); this library never aborts and reports a status instead. */
typedef enum {
    SALN_OK = 0,
    SALN_NOT_IMPLEMENTED = 1,    /* AlignmentError("not implemented"): NW :433-434, WFA :26 */
    SALN_REF_PANIC_BOUNDARY = 2, /* NW traceback index panic, needleman_wunsch_affine.rs:299/:303 */
    SALN_REF_PANIC_TRIM = 3,     /* WFA Ocean::trim rotate_left panic, wfa.rs:577/:603 */
    SALN_REF_PANIC_SLICE = 4,    /* WFA rec_tr slice panic, wfa.rs:695-744 */
    SALN_NONCONVERGED = 5,       /* WFA score loop hit the caller's step cap (wfa.rs:28) */
    SALN_ENUM_CAP = 6,           /* NW co-optimal enumeration hit the caller's cap */
    SALN_SPAN_UNLINKED = 7,      /* saln_nw_spans_walk only: the speculative passes did not
                                    link; walk span by span (saln_nw_span_walk) */
    SALN_TRACE_CAP = 8,          /* saln_wfa_affine_align_batch, saln_ends_free_align_batch: the pair's trace codes alone
                                    exceed trace_budget_bytes; score only, no CIGAR */
    SALN_INTERNAL = 9,           /* saln_wfa_affine_align_batch: the trace pass disagreed with
                                    the score pass; saln_ends_free_replay_align_batch: a walk
                                    did not end within its rounds (internal inconsistency;
                                    never expected) */

    SALN_E_INVALID = -1,   /* bad argument */
    SALN_E_HIP = -2,       /* HIP runtime error (message: saln_last_error) */
    SALN_E_NO_DEVICE = -3, /* no gfx950 device / extension not usable */
    SALN_E_CAPACITY = -4,  /* caller buffer too small */
    SALN_E_IO = -5,        /* file could not be read */
    SALN_E_FASTA = -6,     /* AlignerError::FastaError (bad extension), parse.rs:55-60 */
    SALN_E_FASTA_CHARS = -7, /* AlignerError::CharError; records are still returned, parse.rs:92-97 */
    SALN_E_DEVICE_WAIT = -8  /* a kernel's inter-workgroup dependency wait gave up: the results
                                of the executes since the last status check are invalid
                                (saln_nw_plan_status; message: saln_last_error) */
} saln_status;

/* Device error flags (saln_nw_plan_status, saln_nw_avsa_status). */
#define SALN_FLAG_WAIT_TIMEOUT 1u  /* a column-stripe fill's wait for its left neighbour's
                                      boundary rows exceeded the plan's wait limit */
#define SALN_FLAG_SPEC_UNLINKED 2u /* tests only (option nw.spec_strict = 1): a speculative
                                      stripe walk fell back to the sequential walker */

/* ScoringScheme, needleman_wunsch_affine.rs:15-20 / :382-388.
 * NULL everywhere means the reference SCHEME {5, -4, -8, -6}.
 * The scheme only selects the kernel (packed int16 where the range guards
 * hold, int32 otherwise), never the result: the reference recurrences' with
 * these four values.  Checked against the CPU oracle for match and mismatch
 * of either sign and relative order, and gap_open and gap_extend of either
 * sign (a positive gap_extend runs on the int32 kernels).  A
 * pair so long, or penalties so large, that its scores could leave the
 * engine's int32 range is refused with SALN_E_INVALID by every entry point. */
typedef struct {
    int32_t match;      /* +5 */
    int32_t mismatch;   /* -4 */
    int32_t gap_open;   /* -8 (added once when a gap opens from M) */
    int32_t gap_extend; /* -6 (added for every gap column) */
} saln_nw_scoring;

/* Result of one NW pair (16 bytes). */
typedef struct {
    int32_t score;      /* max(M,I,D)[len_db][len_q], :247-250 (never printed by the reference) */
    int32_t status;     /* SALN_OK | SALN_REF_PANIC_BOUNDARY | SALN_NOT_IMPLEMENTED */
    uint32_t cigar_len; /* RLE ops written for the first printed alignment (0 if none) */
    uint8_t end_states; /* bit0 M, bit1 I, bit2 D: end states equal to score (:251-280) */
    uint8_t printed;    /* 1 if the reference prints at least one alignment block; 0 when
                           its DFS panics first or every co-optimal path is
                           sentinel-rooted (dropped silently, :172-216) */
    uint8_t flags;      /* bit 3: score-only result; bit 1: internal inconsistency
                           (never set); all other bits 0 */
    uint8_t reserved;
} saln_nw_result;

/* CIGAR words: (run_length << 4) | op, BAM op codes, forward order, db as
 * the reference sequence:  '=' 7 (M column, bases equal), 'X' 8 (M column,
 * bases differ), 'I' 1 (query base vs '-', I state), 'D' 2 ('-' vs db base,
 * D state).  A run never exceeds 2^28-1. */
#define SALN_CIGAR_EQ 7u
#define SALN_CIGAR_X 8u
#define SALN_CIGAR_I 1u
#define SALN_CIGAR_D 2u

/* ---------------------------------------------------------------- context */
typedef struct saln_context saln_context;

/* Creates a context bound to HIP device `device` (one stream per context;
 * reentrant per context, not shared across threads).  Fails with
 * SALN_E_NO_DEVICE if no gfx950 device is present: there is no CPU path.
 * Device blocks released by plans and host-buffer calls stay cached in the
 * context (up to 32 GiB, reused by later requests of up to twice the size)
 * until saln_context_destroy; an allocation that fails drops the cache and
 * retries once. */
int saln_context_create(int device, saln_context **out);
int saln_context_destroy(saln_context *ctx);
const char *saln_last_error(void);     /* thread-local message for the last error */
int saln_abi_version(void);

/* ---------------------------------------------------------------- options
 * Tuning knobs (kernel geometry and A/B variants), all with the product's
 * defaults.  No reference counterpart: the reference has no tuning (its
 * constants are compile-time, needleman_wunsch_affine.rs:15-20).  The engine
 * reads nothing from the process environment; these calls are the only way
 * to change what it runs.  Every option gives the same results (but one: a
 * narrower second ring of the corrected WFA returns -2 for pairs that a wider
 * one scores).  Names:
 * "nw.wide_min_pairs", "nw.rows_k", "nw.stripe_pk", "nw.spec",
 * "nw.spec_passes", "nw.spec_strict", "nw.avsa_narrow", "nw.rows_lone",
 * "nw.rows_xcd", "nw.avsa_profile", "nw.pk_tab", "nw.walk_waves",
 * "nw.timing_mode", "wfa2.seq_lds", "wfa2.w1", "wfa2.w2", "wfa.arena_mb",
 * "ends_free.tile_rows", "ends_free.score_i16", "host.timing",
 * "host.prefault_mb".
 * Two levels, no other shared state:
 *  - saln_option_*: the process registry, the default of every context;
 *  - saln_context_option_*: overrides of one context (its own thread's
 *    choices; another context is not affected).
 * A plan, all-vs-all handle, span or host-buffer call takes its context's
 * effective values when it is created (or called); a later change does not
 * reach it.  SALN_E_INVALID for an unknown name or a value out of range.
 * The two ring-width options of the corrected WFA are stored within 0..4096,
 * but that engine runs only 0, 512, 1024 and 2048 (see saln_wfa_affine_batch).
 * The tile-rows option of the ends-free replay traceback is stored within
 * 64..1024, but that entry point runs only 64, 128, 256, 512 and 1024 (see
 * saln_ends_free_replay_align_batch).
 * The score search's option (score_i16; default 1: the packed-i16 fill where
 * it fits; 0: the i32 fill for every pair) is stored within 0..2,
 * but the saln_ends_free_score_* entry points run only 0 and 1 and refuse any
 * other value with SALN_E_INVALID.
 * The arena option (MB, default 32768, minimum 1) bounds the tensor history
 * that one launch of the reference-semantics WFA (saln_wfa_*) keeps.  A lane
 * (one pair) of a pass with step cap s and width W holds S = s / 2 + 1 tensor
 * slots, S * 48 + S * 3 * W * 8 + S bytes.  A launch takes budget / that many
 * lanes, where the budget is the option's value or half of the free device
 * memory if that is less, but never fewer than 256 lanes (or the whole batch
 * if it is smaller); a batch with more pairs runs in several launches.  The
 * results do not depend on it. */
int saln_option_set(const char *name, int64_t value);
int saln_option_get(const char *name, int64_t *value, int64_t *default_value);
/* Name of option `index` (0, 1, ...; SALN_E_INVALID past the last). */
int saln_option_name(uint32_t index, const char **name);
/* Every option of the registry back to its default. */
int saln_options_reset(void);
/* One context's override; _get returns the context's effective value; _clear
 * drops one override (name) or all of them (name NULL). */
int saln_context_option_set(saln_context *ctx, const char *name, int64_t value);
int saln_context_option_get(saln_context *ctx, const char *name, int64_t *value);
int saln_context_option_clear(saln_context *ctx, const char *name);

/* ------------------------------------------------------- NW: per pair (drop-in)
 * Replaces `pub fn n_w_align(seq1: &Record, seq2: &Record, _verbose: bool,
 * mode: Mode) -> Result<()>` (needleman_wunsch_affine.rs:424-437).
 * q = seq1.seq (query), d = seq2.seq (db).  `verbose` is ignored, as in the
 * reference.  cigar (capacity cigar_cap words) may be NULL.
 * Returns SALN_OK or SALN_NOT_IMPLEMENTED (mode != GLOBAL, like :433-434) or
 * an SALN_E_* error; the per-pair outcome (incl. reference panics) is in
 * out->status. */
int saln_nw_align(saln_context *ctx, const uint8_t *q, uint64_t len_q, const uint8_t *d,
                  uint64_t len_db, int verbose, int32_t mode, const saln_nw_scoring *scoring,
                  saln_nw_result *out, uint32_t *cigar, uint64_t cigar_cap);

/* Text the reference prints for this pair (needleman_wunsch_affine.rs:281-286
 * with TraceBackInfo Display :390-411): every co-optimal alignment block in
 * the reference's DFS order, up to the first panic.  The nondeterministic
 * `{:#?}` timing line (:431) is not produced.  max_blocks = 0: unlimited.
 * *status: SALN_OK, SALN_REF_PANIC_BOUNDARY (the reference would abort after
 * the returned text) or SALN_ENUM_CAP.  out may be NULL to query *out_len. */
int saln_nw_render(saln_context *ctx, const uint8_t *q, uint64_t len_q, const uint8_t *d,
                   uint64_t len_db, int32_t mode, uint64_t max_blocks, char *out, uint64_t cap,
                   uint64_t *out_len, uint64_t *n_blocks, int32_t *status);

/* The same text for a batch, each pair computed once (the drop-in CLI and
 * hosts that print per pair).  Replaces the pair loop main.rs:61-74 with the
 * text every n_w_align call prints: one plan for all pairs (same CSR / pair
 * conventions as saln_nw_align_batch; NULL pair lists = all-vs-all, db outer).
 * The GPU walks each pair's first printed alignment and decides what the
 * reference DFS meets after it; pairs whose text that settles (no block,
 * exactly one block, or with max_blocks = 1 the first block and then the cap
 * or the panic) are rendered from that walk, the others by the reference DFS
 * on host threads over their parent codes.  The text stays in the
 * returned handle until saln_nw_text_free.  stop_at_panic = 1: pairs after
 * the first one whose traceback panics (REF_PANIC_BOUNDARY) are not rendered
 * - the reference aborts there (exit 101) - so saln_nw_text_count is that
 * pair's index + 1.  mode != GLOBAL: every pair SALN_NOT_IMPLEMENTED with no
 * text (main.rs:68-74 prints the error and goes on). */
typedef struct saln_nw_text saln_nw_text;
int saln_nw_render_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                         uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                         uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                         uint64_t n_pairs, int32_t mode, uint64_t max_blocks, int stop_at_panic,
                         saln_nw_text **out);
/* One pair in one call: saln_nw_render_batch of (q, d). */
int saln_nw_render_text(saln_context *ctx, const uint8_t *q, uint64_t len_q, const uint8_t *d,
                        uint64_t len_db, int32_t mode, uint64_t max_blocks, saln_nw_text **out);
uint64_t saln_nw_text_count(const saln_nw_text *t);
/* Of those pairs, the ones rendered from the GPU's walk alone (no parent-code
 * download, no host DFS). */
uint64_t saln_nw_text_gpu_decided(const saln_nw_text *t);
/* Pair `pair` (< count): its text (valid until free; not NUL-terminated), the
 * blocks printed, the render status (SALN_OK, SALN_REF_PANIC_BOUNDARY after
 * the text, SALN_ENUM_CAP, SALN_NOT_IMPLEMENTED), its saln_nw_result, and
 * its wall time (its DFS plus its share of the batch's device work).  Any
 * output pointer may be NULL. */
int saln_nw_text_get(const saln_nw_text *t, uint64_t pair, const char **text, uint64_t *len,
                     uint64_t *n_blocks, int32_t *status, saln_nw_result *result,
                     uint64_t *elapsed_ns);
void saln_nw_text_free(saln_nw_text *t);

/* Dense parent mask for parity checks: (len_db+1) x (len_q+1) bytes,
 * row-major over db.  Byte bits: 0-2 = {M,I,D} equal to max(M,I,D) at the
 * cell (so the M parent set of (x,y) is the byte of (x-1,y-1)), 3-4 = I
 * parents {extend I[x][y-1], open M[x][y-1]}, 5-6 = D parents {extend
 * D[x-1][y], open M[x-1][y]} (needleman_wunsch_affine.rs:96-153, boundary
 * parents :196,:208). */
int saln_nw_dense_mask(saln_context *ctx, const uint8_t *q, uint64_t len_q, const uint8_t *d,
                       uint64_t len_db, const saln_nw_scoring *scoring, uint8_t *out);

/* --------------------------------------------------------- NW: batched (host)
 * Replaces the pair loop `for d in db { for q in query { n_w_align(q, d) } }`
 * (main.rs:61-67).  Sequences are CSR: q_seq bytes with q_off[n_q+1].  Pair p
 * aligns query pair_q[p] against db pair_db[p]; if pair_q == pair_db == NULL,
 * all-vs-all in the reference order (db outer, query inner:
 * p = d * n_q + q).  cigar/cigar_off may be NULL; cigar_off[p] (words) must
 * leave room for len_q + len_db words per pair (saln_nw_cigar_offsets). */
int saln_nw_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                        uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                        uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                        uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                        saln_nw_result *results, uint32_t *cigar, const uint64_t *cigar_off);

/* -------------------------------------------------- NW: batched (device, plan)
 * For callers whose data is already resident in HBM (bench, multi-GPU
 * driver).  The plan is built once from host-side lengths; execute then only
 * launches kernels on `stream` (hipStream_t; NULL = the context's own
 * non-blocking stream; pass hipStreamLegacy for the legacy null stream).
 * Device buffers: q_seq/db_seq (same CSR byte layout as the host offsets
 * given to the plan), results[n_pairs], cigar[plan cigar words] (may be
 * NULL: traceback still runs, ops are not stored). */
typedef struct saln_nw_plan saln_nw_plan;

int saln_nw_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                        const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                        const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                        const saln_nw_scoring *scoring, saln_nw_plan **out);
/* The same plan storing the reference's full parent sets: one byte per cell
 * (7 parent bits: the {M,I,D} argmax set and the I / D extend/open parents,
 * needleman_wunsch_affine.rs:96-153 - what the all-blocks DFS :281-329
 * consumes), instead of the walk codes saln_nw_plan_create's fills store.
 * Execute fills, walks and writes the first printed CIGAR as before;
 * saln_nw_plan_dense_mask reads a pair's parent sets back. */
int saln_nw_plan_create_full(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                             const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                             const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                             const saln_nw_scoring *scoring, saln_nw_plan **out);
/* Pair `pair`'s parent sets from the last execute of a synchronous full plan
 * (waits for it), as saln_nw_dense_mask lays them out: (len_db+1) x (len_q+1)
 * bytes.  SALN_E_INVALID while the plan is score-only
 * (saln_nw_plan_set_score_only(plan, 1)): such executes store no codes, and
 * the workspace holds whatever an earlier execute left. */
int saln_nw_plan_dense_mask(saln_nw_plan *plan, uint64_t pair, uint8_t *out);
/* The 4-bit walk codes a (non-full) plan's short-query fills store for pair
 * `pair` (parity tests): len_db x len_q bytes, cell (i, j) at (i-1) len_q +
 * j-1, bits set when the parent is ABSENT - 0 argI, 1 argD (M's predecessor:
 * I / D in max(M, I, D) at (i, j), :120-153), 2 I-open (M(i, j) + open
 * among the maxima of I(i, j+1), :108-119), 3 D-open (the same for D(i+1,
 * j), :96-107); in the last row bit 3 of the end cell is argM.  Last
 * synchronous execute; SALN_E_INVALID for a pair stored otherwise, and
 * for every pair while the plan is score-only (its executes store no codes). */
int saln_nw_plan_walk_codes(saln_nw_plan *plan, uint64_t pair, uint8_t *out);
/* mask_bytes: HBM parent-mask workspace (owned by the plan);
 * cigar_words: required length of the device cigar buffer. */
int saln_nw_plan_info(const saln_nw_plan *plan, uint64_t *mask_bytes, uint64_t *cigar_words,
                      uint64_t *cells);
int saln_nw_cigar_offsets(const saln_nw_plan *plan, uint64_t *cigar_off /* n_pairs+1 */);
int saln_nw_execute(saln_nw_plan *plan, const uint8_t *d_q_seq, const uint8_t *d_db_seq,
                    saln_nw_result *d_results, uint32_t *d_cigar, void *stream);
/* Optional per-kernel timing of every execute while enabled: total_ms and
 * launches (one per execute) since it was enabled.  Names: "nw_fill" (the
 * fill kernels), "nw_traceback" (the walk kernels), "nw_execute" (fill begin
 * to walk end).  By default hipEvents are recorded on the launch streams
 * around the fill and the walk launches: a span runs from marker to marker,
 * launch latency included.  Under "nw.timing_mode" = 0 a pipelined plan of
 * packed fill variants that walks (not score-only) has its kernels stamp the
 * device's constant-rate wall clock themselves instead: a span runs from the first
 * workgroup's start to the last workgroup's end of those kernels (each
 * workgroup's first wave stamps), and the execute puts no timing event on
 * either stream.  Such plans serve two further names:
 * "nw_fill_gap" (fill begin of execute n+1 minus fill end of execute n, among
 * the executes between two reads) and "nw_handoff" (walk begin minus fill
 * end); they replace a kernel trace when the balance of the two kernels is
 * tuned.  Every other plan keeps the events under either value.  The stamps
 * are not the default because they cost the 150 x 150 pipelined step more
 * than the markers do. */
int saln_nw_plan_set_timing(saln_nw_plan *plan, int enable);
int saln_nw_plan_kernel_time(const saln_nw_plan *plan, const char *kernel, double *total_ms,
                             uint64_t *launches);
/* Pipelined mode: execute returns with the traceback still running on the
 * context's second stream, so the traceback of batch n overlaps the fill of
 * batch n+1 (the plan double-buffers its mask workspace).  Results of an
 * execute are complete only after saln_nw_plan_sync(plan, stream, ...) has
 * made `stream` wait for them; keep_latest = 1 leaves the most recent execute
 * pending (software pipelining). */
int saln_nw_plan_set_async(saln_nw_plan *plan, int enable);
/* Score-only mode (the all-vs-all C5 workload): no parent codes, no
 * traceback; results carry score and the reference's panic status
 * (end_states = printed = cigar_len = 0, flags bit 3 set). */
int saln_nw_plan_set_score_only(saln_nw_plan *plan, int enable);
int saln_nw_plan_sync(saln_nw_plan *plan, void *stream, int keep_latest);
/* The stream a pipelined plan's tracebacks run on (NULL: the context's
 * second stream), e.g. a CU-masked stream so that the walk of execute n and
 * the fill of execute n+1 use disjoint CUs (tools/cu_pipeline.py). */
int saln_nw_plan_set_tb_stream(saln_nw_plan *plan, void *stream);
/* Device-side status of the plan's executes.  Waits (host-blocking) for every
 * execute issued since the previous call, then returns the device error
 * flags they raised (SALN_FLAG_*) in *flags (may be NULL) and clears them:
 * read-and-clear, so each execute is reported exactly once.  Returns
 * SALN_E_DEVICE_WAIT when a flag is set, SALN_OK otherwise.  The host-buffer
 * entry points (saln_nw_align, saln_nw_align_batch, ...) check it themselves;
 * device-plan callers call it after their executes (the kernels cannot fail
 * a stream).  A column-stripe fill never hangs: its bounded wait sets the
 * flag and the launch drains with wrong values for that pair. */
int saln_nw_plan_status(saln_nw_plan *plan, uint32_t *flags);
/* Polls a column-stripe dependency wait may spend before it gives up
 * (default 2^24, each poll sleeping ~64 clocks).  Test hook: 0 makes any wait
 * that finds its row unpublished fail, which injects SALN_FLAG_WAIT_TIMEOUT. */
int saln_nw_plan_set_wait_limit(saln_nw_plan *plan, uint32_t polls);
/* Introspection for tests: what the next saln_nw_execute does with pair
 * `pair` (results index), from the code that launches it (no second copy of
 * the decision).  The launch-wide fields depend on the longest db among the
 * plan's pairs of the same variant, on the plan's mode (score-only, async)
 * and on the options the plan read at creation. */
typedef struct {
    int32_t variant;   /* fill variant number (nw_kernels.hip's; -1: a pair with an
                          empty side, which no fill runs) */
    int32_t packed;    /* 1: int16 halves, two pairs per lane group; 0: i32 lanes */
    int32_t rebase;    /* 1: the packed launch uses the rebasing int16 frame */
    int32_t table;     /* packed launch body: 0 generic, 2 table at scale 2, 4 table at
                          scale 4, 3 row profiles */
    int32_t stripe_pk; /* column-stripe pairs (variant 3): 1 packed stripes */
    int32_t rows_k;    /* column-stripe pairs: the row fill's columns per lane
                          (0: the skewed or the packed stripe fill) */
} saln_nw_pair_path;
int saln_nw_plan_pair_path(const saln_nw_plan *plan, uint64_t pair, saln_nw_pair_path *out);
/* Waits for the device, then returns the plan's blocks to its context. */
int saln_nw_plan_destroy(saln_nw_plan *plan);

/* ------------------------------------ NW: score-only all-vs-all (device, C5)
 * The pair loop `for d in db { for q in query { n_w_align(q, d) } }`
 * (main.rs:61-67) reduced to what a score-only caller keeps: for every pair
 * p = d * n_q + q (reference order) out[2p] = score, out[2p+1] = status
 * (SALN_OK | SALN_REF_PANIC_BOUNDARY).  No per-pair descriptors: short
 * queries (packed-i16 region) are grouped into length classes and every
 * class runs as one index space over (query, db record); other queries go
 * through an internal score-only plan.  q_off/db_off are host offsets; the
 * sequences and `out` (int32[2 * n_q * n_db]) live on the device. */
typedef struct saln_nw_avsa saln_nw_avsa;
int saln_nw_avsa_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                        const uint64_t *db_off, uint64_t n_db, int32_t mode,
                        const saln_nw_scoring *scoring, saln_nw_avsa **out);
int saln_nw_avsa_execute(saln_nw_avsa *a, const uint8_t *d_q_seq, const uint8_t *d_db_seq,
                         int32_t *d_out, void *stream);
/* cells = sum over all pairs of len_q * len_db; fallback_pairs = pairs that
 * take the plan path. */
int saln_nw_avsa_info(const saln_nw_avsa *a, uint64_t *cells, uint64_t *fallback_pairs);
/* Launch geometry of a packed query class (fill variant 4-8; include/saln.h
 * has no variant enum, the numbers are nw_kernels.hip's): the most pairs one
 * launch takes and the workgroups (256 threads) that launch has.  Introspection
 * for tests: blocks * 256 must stay a 32-bit work-item count. */
int saln_nw_avsa_launch_geometry(int variant, uint64_t *chunk_pairs, uint64_t *grid_blocks);
/* saln_nw_plan_status of the internal plan (SALN_OK without one); the packed
 * classes have no inter-workgroup waits. */
int saln_nw_avsa_status(saln_nw_avsa *a, uint32_t *flags);
int saln_nw_avsa_destroy(saln_nw_avsa *a);

/* ------------------------- NW: one long pair split by columns (multi-GPU, f3)
 * The fill loop of one pair (needleman_wunsch_affine.rs:217-236) and its
 * traceback (:242-334) cut into column spans, one per GPU (SURVEY.md §8(f)
 * #3): span r owns query columns col_lo+1 .. col_hi (col_lo a multiple of
 * 256), keeps only its part of the 1 B/cell parent mask, and runs the row
 * fill's column stripes over every db row.  Its first stripe takes the
 * boundary entering column col_lo+1 from the span's INBOX column, its last
 * stripe publishes the boundary leaving column col_hi into its OUTBOX column;
 * a caller moves outbox rows of span r into the inbox of span r+1 while both
 * fills run (RCCL send/recv per row band, or a device copy).  Boundary
 * columns hold one 8-byte element per db row r at element r (the engine's
 * internal (H, I) form; an unpublished row reads 0x80000000 in its low word),
 * saln_nw_span_boundary_elems elements per column.
 *
 * The traceback crosses the spans right to left: the span holding the end
 * cell walks from it (entry SALN_SPAN_END) until the walk leaves its first
 * column; its exit is the entry of the span to the left; the span where the
 * walk ends reports kind SALN_SPAN_EXIT + event.  Concatenating the spans'
 * op words in walk order (last span first, runs of one op merged at the
 * seams) and reversing gives the pair's CIGAR. */
typedef struct saln_nw_span saln_nw_span;
/* walk cursor kinds (entry / exit) */
#define SALN_SPAN_M 0         /* state known: M, I or D at (i, j) */
#define SALN_SPAN_I 1
#define SALN_SPAN_D 2
#define SALN_SPAN_VIA_M 3     /* arrived at (i, j) by a diagonal step: state = its argmax */
#define SALN_SPAN_VIA_I 4     /* arrived by a horizontal step: state from (i, j+1)'s I bits */
#define SALN_SPAN_END 5       /* the pair's end cell, first end state (the reference's order) */
#define SALN_SPAN_EXIT 8      /* exit: the walk ended; + 0 origin, + 1 panic, + 2 dead end */
typedef struct {
    int32_t i, j;   /* cell (db row, query column) */
    int32_t kind;   /* SALN_SPAN_* */
    uint32_t end_states; /* exit of the end cell's span: the end cell's state set
                            (bit0 M, bit1 I, bit2 D), else 0 */
} saln_nw_span_cursor;
/* Elements (8 bytes each) of one boundary column for a db of len_db rows. */
uint64_t saln_nw_span_boundary_elems(uint64_t len_db);
/* Boundary columns (stripes + 1) of the span col_lo+1 .. col_hi: the size of a
 * caller-owned d_boundary is cols * saln_nw_span_boundary_elems(len_db)
 * elements (host-only, no device needed).  device_cols: the query columns of
 * every span that fills on the same device at the same time (0: this span
 * alone); the stripe width follows from it (64 columns while each stripe
 * has a SIMD of its own, else 128). */
uint64_t saln_nw_span_boundary_cols(uint64_t col_lo, uint64_t col_hi, uint64_t device_cols);
/* d_boundary: caller-owned device buffer of (stripes + 1) boundary columns
 * (saln_nw_span_info), column 0 the inbox, the last column the outbox; NULL:
 * the span allocates it. */
int saln_nw_span_create(saln_context *ctx, uint64_t len_q, uint64_t len_db, uint64_t col_lo,
                        uint64_t col_hi, uint64_t device_cols, const saln_nw_scoring *scoring,
                        void *d_boundary, saln_nw_span **out);
int saln_nw_span_info(const saln_nw_span *s, uint64_t *mask_bytes, uint64_t *boundary_cols,
                      uint64_t *ops_cap);
/* Device addresses of the inbox (column 0) and outbox (last column). */
int saln_nw_span_boundary(const saln_nw_span *s, void **inbox, void **outbox);
/* Presets both boundary columns to "unpublished" on `stream`.  Must precede
 * any write into the inbox and the fill. */
int saln_nw_span_reset(saln_nw_span *s, void *stream);
/* Launches the span's fill (q / db: the whole pair's sequences on the
 * device).  A span with col_lo > 0 waits, row by row, for its inbox. */
int saln_nw_span_fill(saln_nw_span *s, const uint8_t *d_q, const uint8_t *d_db, void *stream);
/* Launches a one-wave kernel that returns once outbox rows row_lo .. row_hi
 * are published (bounded by the wait limit: then the timeout flag is set),
 * so work queued behind it on `stream` may read them. */
int saln_nw_span_watch(saln_nw_span *s, uint64_t row_lo, uint64_t row_hi, void *stream);
/* Walks this span from `entry` (host-blocking, after the fill completed);
 * ops (host, ops_cap words) receive the run words in walk order (back to
 * front); *exit the cursor where the walk left the span or ended. */
int saln_nw_span_walk(saln_nw_span *s, const uint8_t *d_q, const uint8_t *d_db,
                      const saln_nw_span_cursor *entry, saln_nw_span_cursor *exit, uint32_t *ops,
                      uint64_t ops_cap, uint64_t *n_ops, void *stream);
/* The span holding the end cell: score and panic status of the pair once the
 * fill queued on `stream` has finished (host-blocking; SALN_E_INVALID on
 * another span). */
int saln_nw_span_score(saln_nw_span *s, int32_t *score, int32_t *status, void *stream);
/* As saln_nw_plan_status / saln_nw_plan_set_wait_limit for the span's fill
 * and watch waits. */
int saln_nw_span_status(saln_nw_span *s, uint32_t *flags);
int saln_nw_span_set_wait_limit(saln_nw_span *s, uint32_t polls);
int saln_nw_span_destroy(saln_nw_span *s);
/* Spans of one pair on ONE device (tests, the single-GPU emulation of the
 * multi-GPU chain): queues on `stream` a one-wave kernel that copies src's
 * outbox rows row_lo .. row_hi into dst's inbox as they are published (64
 * rows per round). */
int saln_nw_span_forward(saln_nw_span *src, saln_nw_span *dst, uint64_t row_lo, uint64_t row_hi,
                         void *stream);
/* Compute units of the context's device, and a stream whose kernels run only
 * on CUs cu_lo .. cu_hi-1 (hipExtStreamCreateWithCUMask): one device split
 * into per-span partitions. */
/* The walk over all n spans of a pair on ONE device at once: every span's
 * speculative stripe passes run together over a shared record table, linked
 * on the host from the end cell to the walk's end.  Returns SALN_OK with the
 * pair's CIGAR in `ops` (forward order, runs of one op merged across the
 * spans' seams: the words saln_nw_align gives when the walk printed) and the
 * final exit, SALN_SPAN_UNLINKED when the passes do not link (walk span by
 * span with saln_nw_span_walk), or an error. */
int saln_nw_spans_walk(saln_nw_span *const *spans, uint32_t n, const uint8_t *d_q,
                       const uint8_t *d_db, saln_nw_span_cursor *exit, uint32_t *ops,
                       uint64_t ops_cap, uint64_t *n_ops, void *stream);
int saln_device_cu_count(saln_context *ctx, uint32_t *n);
/* A stream on mask bits [cu_lo, cu_hi).  Bit c is a CU of XCD c mod n_xcd
 * (measured, profiles/r04_cu_map.json), so a range of 8k bits is k CUs per
 * XCD.  Ranges shorter than the XCD count are refused (SALN_E_INVALID): an
 * XCD left without a bit runs unmasked. */
int saln_stream_create_cu_range(saln_context *ctx, uint32_t cu_lo, uint32_t cu_hi, void **stream);
int saln_stream_destroy(saln_context *ctx, void *stream);
/* A stream on an arbitrary CU mask (bit c of word c / 32 = CU c in the
 * runtime's mask order, hipExtStreamCreateWithCUMask; an XCD with no bit set
 * runs unmasked, see saln_stream_create_cu_range). */
int saln_stream_create_cu_mask(saln_context *ctx, const uint32_t *mask, uint32_t n_words,
                               void **stream);
/* Diagnostic: launches n_blocks one-wave workgroups on `stream` (e.g. a
 * CU-masked one) and returns, per workgroup, the HW_ID register of its wave
 * (gfx9 layout: CU 11:8, SH 12, SE 15:13) and its XCC_ID (host arrays of
 * n_blocks).  tools/cu_map.py derives the mask bit -> (XCD, SE, CU) order. */
int saln_device_cu_probe(saln_context *ctx, void *stream, uint32_t n_blocks, uint32_t *hw_id,
                         uint32_t *xcc_id);

/* ----------------------------------------------------------------------- WFA
 * Replaces `pub fn wfa_align(seq1: &Record, seq2: &Record, mode: Mode)`
 * (wfa.rs:23-42) with the reference's exact (quirky) semantics: wavefront
 * tensors built by WaveFrontTensor::new (:225-420), extension of the newest
 * M front only (:127-139, :467-488), Ocean::trim (:490-623), convergence on
 * the newest tensor at (len_db-1, len_q-1) (:180-191), and the greedy rec_tr
 * traceback (:654-853).  seq1 = query, seq2 = db.  The reference loops
 * forever when it never converges; max_steps bounds the expand loop
 * (status SALN_NONCONVERGED), and max_width bounds a wavefront's width
 * (also SALN_NONCONVERGED).  Rust panics are statuses:
 * SALN_REF_PANIC_TRIM (rotate_left / expect / unwrap in trim),
 * SALN_REF_PANIC_SLICE (slice indexing in rec_tr).
 *
 * The two caps.  Results equal the reference's until one of them binds:
 *  - step cap: the pair has made max_steps expand calls without converging.
 *    status SALN_NONCONVERGED, steps == max_steps, score == steps + 1 (every
 *    expand call pushed its tensor, and score is wfs.len()).
 *  - width cap: an expand call would build a tensor of more than max_width
 *    diagonals (hi - lo + 1 of the `lo/hi` line it prints; the line is still
 *    printed by saln_wfa_render).  status SALN_NONCONVERGED, steps counts
 *    the refused call, score == steps (its tensor was not pushed).
 * steps < max_steps tells the width cap from the step cap.  The tensor of
 * the k-th expand call is at most 2 * (k / 4) + 1 diagonals wide (integer
 * division: its sources lie 4, 6 and 8 calls back and each side grows by
 * one), so max_width >= 2 * (max_steps / 4) + 1 never binds; the default
 * width of 64 cannot bind for max_steps <= 127. */
typedef struct {
    int32_t score;        /* printed score: wfs.len() at convergence (:33-38) */
    int32_t status;       /* SALN_OK | SALN_NOT_IMPLEMENTED | SALN_REF_PANIC_* | SALN_NONCONVERGED */
    uint32_t steps;       /* Ocean::expand calls */
    uint32_t aln_len1;    /* bytes of Alignment.seq1 / seq2 (traceback output) */
    uint32_t aln_len2;
    int32_t conv_offset;  /* converged element (:640): offset, state (0 M, 1 D, 2 I), */
    uint8_t conv_state;   /*   parents (np entries, same codes)                      */
    uint8_t conv_np;
    uint8_t conv_parents[3];
    uint8_t reserved[3];
} saln_wfa_result;        /* 32 bytes */

/* Batched wfa_align over pairs (same pair conventions as
 * saln_nw_align_batch).  aln (optional): per pair 2*aln_cap bytes at
 * aln_off[p] (seq1 then seq2, in the reference's push order, i.e. reversed).
 * max_steps = 0 selects 64; max_width = 0 selects 64. */
int saln_wfa_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                         uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                         uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                         uint64_t n_pairs, int32_t mode, uint32_t max_steps, uint32_t max_width,
                         saln_wfa_result *results, uint8_t *aln, const uint64_t *aln_off,
                         uint32_t aln_cap);

/* Everything the reference prints to stdout for one wfa_align call (the
 * `lo/hi` lines, `converged with score`, the traceback's debug lines, the
 * alignment and its Debug dump), up to the point where it would panic. */
int saln_wfa_render(saln_context *ctx, const uint8_t *q, uint64_t len_q, const uint8_t *d,
                    uint64_t len_db, int32_t mode, uint32_t max_steps, uint32_t max_width,
                    char *out, uint64_t cap, uint64_t *out_len, saln_wfa_result *result);

/* The same text for every pair of a batch (pair conventions as
 * saln_wfa_align_batch), each pair computed once: one GPU run of the batch
 * with its step logs and alignment rows, then host rendering.  Replaces the
 * size-probe + render pair of saln_wfa_render calls per pair that the pair
 * loop main.rs:61-74 would otherwise make.  Large batches run in chunks of
 * at most ~1 GB of alignment rows and step logs each. */
typedef struct saln_wfa_text saln_wfa_text;
int saln_wfa_render_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                          uint64_t n_pairs, int32_t mode, uint32_t max_steps, uint32_t max_width,
                          saln_wfa_text **out);
uint64_t saln_wfa_text_count(const saln_wfa_text *t);
/* text points into the handle (not NUL-terminated; len bytes), valid until
 * saln_wfa_text_free. */
int saln_wfa_text_get(const saln_wfa_text *t, uint64_t pair, const char **text, uint64_t *len,
                      saln_wfa_result *result);
void saln_wfa_text_free(saln_wfa_text *t);

/* Device-resident WFA batch (configs[2] / C3 measurement): plan once from host
 * offsets and a pair list (NULL = all-vs-all, reference order), then execute
 * on device sequences (same CSR layout) into device results[n_pairs].  No
 * alignment rows.  With max_steps above 32, pairs that reach a 32-step first
 * pass are re-run with max_steps (saln_wfa_align_batch does the same); the
 * results equal a single pass at max_steps. */
typedef struct saln_wfa_plan saln_wfa_plan;
int saln_wfa_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                         const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                         const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                         uint32_t max_steps, uint32_t max_width, saln_wfa_plan **out);
int saln_wfa_execute(saln_wfa_plan *plan, const uint8_t *d_q_seq, const uint8_t *d_db_seq,
                     saln_wfa_result *d_results, void *stream);
int saln_wfa_plan_destroy(saln_wfa_plan *plan);

/* ------------------------------------------- corrected gap-affine WFA (new)
 * NOT a reference-parity path.  The reference's
 * wfa_align (src/wfa.rs:23-42, above) defines no output for realistic inputs
 * (Ocean::trim panics at s = 20).  These entry points compute
 * what a gap-affine WFA is meant to: the minimum penalty of a global
 * alignment, mismatch * #mismatches + sum(gap_open + gap_extend * len) over
 * gaps, with the reference's penalties (wfa.rs:14-21) by default.  The
 * checker is the Gotoh DP (oracle/refaffine.c).
 * scores[p] >= 0: the penalty; -1: above max_score (max_score <= 0: no cap);
 * -2: the wavefront grew past the second pass's ring: 2,048 diagonals with
 * the default penalties (i16 offsets; 1,024 when a sequence of the batch is
 * longer than 32,000 bases, which selects i32 offsets), fewer where the
 * penalties need more ring slots (saln_wfa_affine_plan_geometry reports the
 * widths).
 * Ring widths and LDS: a pass's rings take 768 + (RM + 2 RI) * W * (2 | 4)
 * bytes of LDS for W diagonals, RM = max(x, o+e) / g + 1 and RI = e / g + 1
 * slots (g = gcd(x, o+e, e); at most 16 each, else SALN_E_INVALID) and i16 |
 * i32 offsets.  No pass asks for more than the 65,536 bytes of a workgroup:
 * a pass whose rings do not fit at its width ("wfa2.w1" / "wfa2.w2", or the
 * default) runs the widest of 2,048, 1,024 and 512 diagonals that fits, and
 * penalties whose rings do not fit at 512 are refused (SALN_E_INVALID with a
 * message naming them).  The kernels run rings of 512, 1,024 and 2,048
 * diagonals only: with "wfa2.w1" or "wfa2.w2" at any other value but 0
 * (the default width) every plan, batch and geometry call returns
 * SALN_E_INVALID. */
typedef struct {
    int32_t mismatch;   /* x = 4 */
    int32_t gap_open;   /* o = 2 */
    int32_t gap_extend; /* e = 6 */
} saln_wfa_penalties;   /* NULL = the reference's {4, 2, 6} */

int saln_wfa_affine_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                          uint64_t n_pairs, const saln_wfa_penalties *pen, int32_t max_score,
                          int32_t *scores);
/* Device-resident form (configs[2] measurement with the corrected engine):
 * plan from host offsets and a pair list (NULL = all-vs-all, reference
 * order), execute on device sequences into device scores[n_pairs]. */
typedef struct saln_wfa_affine_plan saln_wfa_affine_plan;
int saln_wfa_affine_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                const uint32_t *pair_db, uint64_t n_pairs,
                                const saln_wfa_penalties *pen, int32_t max_score,
                                saln_wfa_affine_plan **out);
int saln_wfa_affine_execute(saln_wfa_affine_plan *plan, const uint8_t *d_q_seq,
                            const uint8_t *d_db_seq, int32_t *d_scores, void *stream);
int saln_wfa_affine_plan_destroy(saln_wfa_affine_plan *plan);

/* Alignment mode: the minimum penalty as above and one optimal alignment per
 * pair as CIGAR words ((run << 4) | op with SALN_CIGAR_EQ/X/I/D, forward
 * order, db as the reference sequence, like the NW paths).  Orientation: a
 * column of '-' against a db base (the WFA's I component, which advances the
 * db offset) is SALN_CIGAR_D; a query base against '-' (its D component) is
 * SALN_CIGAR_I.  Among co-optimal alignments the choice is fixed (M prefers
 * a mismatch, then the db-advancing gap, then the query-advancing gap; a gap
 * prefers extend over open), so a pair's words do not depend on the batch,
 * the chunk or the run. */
typedef struct {
    int32_t score;      /* as saln_wfa_affine_batch: the penalty, -1 or -2 */
    int32_t status;     /* SALN_OK | SALN_TRACE_CAP | SALN_INTERNAL */
    uint32_t cigar_len; /* CIGAR words (0: negative score, SALN_TRACE_CAP, or both sequences empty) */
    uint32_t reserved;
} saln_wfa_affine_result;   /* 16 bytes */

/* Same pair conventions and argument errors as saln_wfa_affine_batch.  Runs
 * the score passes, reads the scores back, then the trace fill and the walk
 * in chunks: pairs are packed greedily in pair order into chunks of at most
 * trace_budget_bytes of trace codes (saln_wfa_affine_trace_bytes each; 0
 * selects 1 GiB).  A pair with score -1 or -2 has status SALN_OK and no
 * words; a pair whose codes alone exceed the budget has its score, status
 * SALN_TRACE_CAP and no words.  A sequence longer than 2^28-1 bases is
 * refused.  The handle owns the words. */
typedef struct saln_wfa_affine_aln saln_wfa_affine_aln;
int saln_wfa_affine_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                uint64_t n_pairs, const saln_wfa_penalties *pen,
                                int32_t max_score, uint64_t trace_budget_bytes,
                                saln_wfa_affine_aln **out);
uint64_t saln_wfa_affine_aln_count(const saln_wfa_affine_aln *a);
/* res and cigar are optional.  cigar points into the handle, res->cigar_len
 * words, valid until saln_wfa_affine_aln_free; the words of consecutive pairs
 * are contiguous, in pair order. */
int saln_wfa_affine_aln_get(const saln_wfa_affine_aln *a, uint64_t pair,
                            saln_wfa_affine_result *res, const uint32_t **cigar);
void saln_wfa_affine_aln_free(saln_wfa_affine_aln *a);
/* Host only (no device needed): bytes of trace workspace of one pair with
 * this penalty (score >= 0), the one place the layout's size is computed:
 *   T = score / g (g = gcd(x, o+e, e)) steps;
 *   wt = the smallest power of two >= max(64, min(2*max(0,(score-o)/e) + 1,
 *        len_q + len_db + 1) + 2) diagonals per code row, 4 bits each;
 *   bytes = T * wt / 2 (codes) + T rounded up to 16 (the walk's op bytes);
 * 0 when a sequence is empty.  SALN_E_INVALID for a negative score or bad
 * penalties. */
int saln_wfa_affine_trace_bytes(const saln_wfa_penalties *pen, uint64_t len_q, uint64_t len_db,
                                int32_t score, uint64_t *bytes);
/* Host only (no device needed): the launch geometry a plan over pairs of
 * these lengths (len_q[k] x len_db[k]) takes with these penalties and the
 * process registry's options - the decision saln_wfa_affine_plan_create
 * makes (with its context's options).  out[0] is the first pass, out[1] the
 * second (the pairs whose wavefront outgrew the first ring).  seqcap: the
 * LDS bytes for a pair's staged sequences; a pair stages 2-bit codes when
 * 4 * ((a_q + len_q + 15) / 16 + (a_d + len_db + 15) / 16 + 4) <= seqcap
 * (a_*: the sequence's address & 15) and all its bytes are A, C, G, T; else
 * bytes when ((len_q + 47) & ~15) + len_db + 48 <= seqcap; else it reads
 * the sequences where they are.  SALN_E_INVALID as the plan: bad penalties,
 * a refused ring-width option, rings that do not fit LDS. */
typedef struct {
    int32_t ring_width;   /* diagonals per wavefront slot: 512, 1024 or 2048 */
    int32_t seqcap;       /* LDS bytes for staged sequences (0: none staged) */
    uint32_t lds_bytes;   /* dynamic LDS of a workgroup: rings + seqcap, <= 65,536 */
    int32_t i32_offsets;  /* 1: i32 wavefront offsets (a sequence above 32,000 bases) */
    uint32_t workgroups_per_cu; /* a launch of n pairs (a score pass, or a trace fill of one
                                 * chunk) runs min(n, workgroups_per_cu * CUs) one-wave
                                 * workgroups, which take the pairs from a counter */
} saln_wfa_affine_pass_geometry;   /* 20 bytes */
int saln_wfa_affine_plan_geometry(const saln_wfa_penalties *pen, const uint64_t *len_q,
                                  const uint64_t *len_db, uint64_t n_pairs,
                                  saln_wfa_affine_pass_geometry out[2]);

/* ------------------- ends-free alignment: local, semi-global and overlap (new)
 * NOT a reference-parity path.  The reference only declares the first two modes
 * (overlap, SALN_MODE_OVERLAP, has no reference name at all):
 * ScoreTensor::Local and ::SemiGlobal carry empty comments where the fill
 * should be (needleman_wunsch_affine.rs:238-239, :331-332) and n_w_align
 * answers "not implemented" (:433-434), which saln_nw_* and the CLI keep
 * doing.  These entry points compute what the two modes are meant to: Gotoh
 * affine-gap alignment with free ends, on the GPU (ends_free_kernels.hip),
 * checked against the plain model tests/ends_free_model.py.
 *
 * Orientation, CIGAR words and scoring as above: q = query = columns j
 * (length n), d = db = rows i (length m), the db is the reference sequence;
 * a gap of length L costs gap_open + L * gap_extend; bases compare as bytes.
 * This engine takes match > 0, mismatch < 0, gap_open <= 0, gap_extend < 0
 * and refuses a batch with a pair for which (n + m + 2) * max|parameter| >=
 * 2^30 (SALN_E_INVALID).  Gaps open from M only (an I run and a D run are
 * never adjacent), s(i, j) is match or mismatch of d[i-1] against q[j-1]:
 *   I(i,j) = max(I(i,j-1) + e, M(i,j-1) + o + e)      j >= 1
 *   D(i,j) = max(D(i-1,j) + e, M(i-1,j) + o + e)      i >= 1
 *   M(i,j) = s(i,j) + P(i-1,j-1)                      i, j >= 1
 *   P = max(M, I, D) (semi-global, overlap), max(0, M, I, D) (local);
 * everything no rule gives is -infinity.
 *  - SALN_MODE_SEMI_GLOBAL: the whole query against a free db substring.
 *    M(i,0) = 0 for every i (the start); M(0,j>0), I(i,0), D(i,0), D(0,j) are
 *    -infinity.  score = max over i in 0..m of max(M(i,n), I(i,n)); the
 *    smallest i wins a tie, M before I.  n = 0: score 0, no words, db_begin =
 *    db_end = 0.  m = 0: gap_open + n * gap_extend and the single word nI.
 *    q_begin = 0 and q_end = n always.
 *  - SALN_MODE_LOCAL: score = max(0, max over i, j of M(i,j)); the alignment
 *    begins and ends with an M column; the smallest i, then the smallest j,
 *    wins a tie.  Score 0: no words, all four coordinates 0.
 *  - SALN_MODE_OVERLAP (dovetail, all four ends free): a suffix of one
 *    sequence against a prefix of the other, or one sequence inside the
 *    other; no floor, no charge for the overhang on either sequence.
 *    M(i,0) = 0 for i in 0..m and M(0,j) = 0 for j in 0..n (every cell of row
 *    0 and column 0 is a free start); I(i,0), I(0,j), D(i,0), D(0,j) are
 *    -infinity; by the rules I(i,1) = o + e for i >= 1 (it opens from M(i,0))
 *    and D(1,j) = o + e for j >= 1 (it opens from M(0,j); semi-global's
 *    D(1,j) is -infinity).  The end candidates are the border cells (i,n),
 *    1 <= i <= m, and (m,j), 1 <= j <= n, each with the value P(i,j); score =
 *    max(0, the best candidate).  No strictly positive candidate (n = 0 and
 *    m = 0 included): the empty alignment, score 0, no words, all four
 *    coordinates 0 (local's convention).  Else the end cell is the candidate
 *    with the largest value, the smallest i, then the smallest j, winning a
 *    tie (a last-column cell above row m beats a last-row cell), and the end
 *    state is the first of M, I, D equal to P there.  At least one of
 *    q_begin and db_begin is 0, at least one of q_end = n and db_end = m
 *    holds.
 *  - SALN_MODE_EXTEND (the gapped extension of seed-and-extend: pinned at the
 *    origin, free at its end): the alignment starts at (0,0) and may stop at
 *    any cell, with no charge for what lies behind the stop.  P = max(M, I,
 *    D), no floor.  M(0,0) = 0 is the only start; I(0,j) = o + j e for j >= 1
 *    (semi-global's row 0) and D(i,0) = o + i e for i >= 1 (column 0 is a
 *    deletion run); M(i,0) for i > 0, M(0,j) for j > 0, I(i,0) and D(0,j) are
 *    -infinity, hence I(i,1) = -infinity for i >= 1 and D(1,j) = -infinity
 *    for j >= 1: nothing opens from a border gap.  score = max(0, max over
 *    i >= 1, j >= 1 of M(i,j)); the smallest i, then the smallest j, wins a
 *    tie (local's rule; ending in a gap is never better, e < 0).  No strictly
 *    positive M (n = 0 or m = 0 included): the empty alignment, score 0, no
 *    words, all four coordinates 0.  The walk starts in M at the end cell and
 *    goes back to (0,0): in M at (i,j) it emits '=' or 'X' and goes to
 *    (i-1,j-1); at (0,0) it stops, on row 0 with j > 0 it emits one run of j
 *    'I' and stops, on column 0 with i > 0 one run of i 'D' and stops, else
 *    the next state is the first of M, I, D equal to M(i,j) - s(i,j).
 *    q_begin = db_begin = 0 always; the '=', 'X', 'I' lengths sum to q_end
 *    and the '=', 'X', 'D' lengths to db_end.  Every cell is computed; the
 *    X-drop form, which prunes cells and stops the fill early, is
 *    saln_ends_free_xdrop_align_batch ("X-drop extension", below).
 * The walk's choice among co-optimal paths is fixed.  In M at (i,j): emit
 * '=' or 'X', v = M(i,j) - s(i,j), go to (i-1,j-1); local stops when v == 0,
 * semi-global on reaching column 0, overlap on reaching row 0 or column 0;
 * else the next state is the first of M, I, D whose value there equals v.
 * In I or D extend comes before open; overlap also stops after an 'I' that
 * reaches column 0 or a 'D' that reaches row 0 (gaps opened from the free
 * start).  A pair's words depend on nothing but the pair and the scoring.
 * Ranges are half-open and 0-based: the '=', 'X' and 'I' lengths sum to
 * q_end - q_begin, the '=', 'X' and 'D' lengths to db_end - db_begin.
 *
 * Limits: a query of at most 1,024 columns (one chunk of the lane fill;
 * saln_ends_free_pair_geometry reports its class) and a db of at most 65,000
 * rows (a group's db row is staged in LDS); a longer sequence makes the batch
 * SALN_E_INVALID with a message naming the limit.  Longer pairs:
 * saln_ends_free_long_align_batch, below, whose only limit is the range
 * guard. */
typedef struct {
    int32_t score, status;            /* SALN_OK | SALN_TRACE_CAP | SALN_INTERNAL (replay only) */
    int32_t q_begin, q_end, db_begin, db_end;   /* begins -1 when no walk ran */
    uint32_t cigar_len, reserved;     /* reserved: 0; saln_ends_free_xdrop_*: the fill's steps (below) */
} saln_ends_free_result;              /* 32 bytes */

/* Pair conventions and argument errors as saln_wfa_affine_align_batch (NULL
 * pair lists = all-vs-all, db outer).  mode: SALN_MODE_LOCAL,
 * SALN_MODE_SEMI_GLOBAL, SALN_MODE_OVERLAP or SALN_MODE_EXTEND;
 * SALN_MODE_GLOBAL is SALN_E_INVALID (use saln_nw_*), and so is every other
 * value.
 * want_cigar != 0: the fill stores 4-bit trace codes and the walk follows
 * them, in chunks: pairs are packed greedily in pair order into chunks of at
 * most trace_budget_bytes of codes (saln_ends_free_trace_bytes each; 0
 * selects 1 GiB).  A pair whose codes alone exceed the budget has its score
 * and end coordinates, status SALN_TRACE_CAP, begins -1 and no words.
 * want_cigar == 0 runs the fill only (no codes stored): score and ends, begins
 * -1, cigar_len 0.  The handle owns the words. */
typedef struct saln_ends_free_aln saln_ends_free_aln;
int saln_ends_free_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                               uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                               uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                               uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                               uint64_t trace_budget_bytes, int want_cigar,
                               saln_ends_free_aln **out);
uint64_t saln_ends_free_aln_count(const saln_ends_free_aln *a);
/* res and cigar are optional.  cigar points into the handle, res->cigar_len
 * words, valid until saln_ends_free_aln_free; the words of consecutive pairs
 * are contiguous, in pair order. */
int saln_ends_free_aln_get(const saln_ends_free_aln *a, uint64_t pair, saln_ends_free_result *res,
                           const uint32_t **cigar);
void saln_ends_free_aln_free(saln_ends_free_aln *a);

/* Device-resident score-only form: plan from host offsets and a pair list
 * (NULL = all-vs-all), execute on device sequences (same CSR layout) into
 * device results[n_pairs] (score, ends, begins -1).  Stream as the other
 * plans (NULL = the context's own stream). */
typedef struct saln_ends_free_plan saln_ends_free_plan;
int saln_ends_free_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                               const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                               const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                               const saln_nw_scoring *scoring, saln_ends_free_plan **out);
int saln_ends_free_execute(saln_ends_free_plan *plan, const uint8_t *d_q_seq,
                           const uint8_t *d_db_seq, saln_ends_free_result *d_results, void *stream);
int saln_ends_free_plan_destroy(saln_ends_free_plan *plan);

/* Host only (no device needed): bytes of trace codes of one pair, the one
 * place the size is computed: len_db rows of ceil(len_q / cols) * cols / 2
 * bytes (4 bits per cell; cols: the pair's class, below), rounded up to a
 * multiple of 8; 0 when a sequence is empty.  SALN_E_INVALID above the
 * engine's limits. */
int saln_ends_free_trace_bytes(uint64_t len_q, uint64_t len_db, uint64_t *bytes);
/* Host only: the class a query of len_q columns runs in: one pair per group
 * of *lanes lanes, *cols_per_lane query columns per lane (16 x 10, 16 x 16,
 * 64 x 8, 64 x 16: the smallest that holds the query).  SALN_E_INVALID above
 * 1,024 columns.  The launch code asks the same function. */
int saln_ends_free_pair_geometry(uint64_t len_q, uint32_t *lanes, uint32_t *cols_per_lane);
/* Host only: the workgroup of the class fill that runs queries of len_q
 * columns in a launch whose longest db has ld_max rows (a batch's pairs are
 * cut into launches by class and by the power-of-two bucket of the db length).
 * *groups: the lane groups, one pair each, of a workgroup: 256 / lanes of
 * them, lowered until their staged db rows, groups * (ld_max + 2 * lanes)
 * bytes, fit 64 KB; with has_matrix != 0 (the saln_ends_free_sub_* entry
 * points) 64 KB less the matrix's block of 1,408 bytes; never below 1.
 * *lds_bytes: those bytes of staged rows (the block not counted).  A workgroup
 * has *groups * lanes lanes.  SALN_E_INVALID for a NULL output, above 1,024
 * columns and above 65,000 rows.  The launch code asks the same function. */
int saln_ends_free_fill_geometry(uint64_t len_q, uint64_t ld_max, int has_matrix, uint32_t *groups,
                                 uint32_t *lds_bytes);

/* X-drop extension: SALN_MODE_EXTEND with one more rule and a parameter
 * xdrop = X >= 0.  Borders, recurrences, tie rules and the walk are
 * extension's.  Every cell (i,j), 0 <= i <= m, 0 <= j <= n, also carries
 * B(i,j): the largest P of an unpruned cell in its dominance region
 * {(i',j') : i' <= i, j' <= j}.
 *  - (0,0) has P = B = 0 and is never pruned.
 *  - Every other cell computes M, I, D by extension's recurrences from its
 *    neighbours' values after pruning; P = max(M, I, D) and Bin =
 *    max(B(i-1,j), B(i,j-1)), a B outside the matrix being -infinity.
 *  - The cell is pruned iff P < Bin - X (strict).  A pruned cell has M = I =
 *    D = -infinity for every successor, and B = Bin.  An unpruned cell keeps
 *    its values, and B = max(Bin, P).
 * B obeys the dependencies of the recurrence, so the tables, and with them the
 * record and the words, depend on nothing but the pair, the scoring and X:
 * not on the order in which cells are computed, not on the class geometry.
 * Consequences:
 *  - Row 0 and column 0 have closed forms: (0,j) is unpruned iff o + j e >=
 *    -X, (i,0) iff o + i e >= -X, and B is 0 there.
 *  - Score and end cell are extension's rule over the unpruned cells: max(0,
 *    max M(i,j), i, j >= 1), the smallest i, then the smallest j.  A pruned
 *    cell's M lies below Bin - X, hence below an unpruned M or 0: it never
 *    wins or ties.
 *  - The walk never reads a pruned cell: an unpruned cell's chosen
 *    predecessor holds a finite value.
 *  - The score is monotone in X and never above extension's.  With X >=
 *    2 (n + m + 2) max|parameter| nothing real is pruned: records (but
 *    `reserved`) and words equal saln_ends_free_align_batch's under
 *    SALN_MODE_EXTEND.
 *  - Early stop.  With L the last row that holds an unpruned cell, every cell
 *    below row L is pruned, and so is everything behind any fully pruned front
 *    of the fill; the fill leaves a pair as soon as its front is pruned.
 * Domain: xdrop >= 0, and the range guard becomes (n + m + 2) *
 * max|parameter| + xdrop < 2^30; outside it the batch is SALN_E_INVALID with a
 * message.  Limits (1,024 columns, 65,000 rows, a message naming the limit),
 * trace budget, chunking and SALN_TRACE_CAP are saln_ends_free_align_batch's:
 * codes stay sized for all m rows.  Arguments are validated before the device
 * is touched.
 * `reserved` of these entry points' records is a diagnostic: the number of
 * row-loop steps the pair's group of lanes ran.  Unlike the rest of the record
 * it depends on the class geometry (G lanes, saln_ends_free_pair_geometry):
 * reserved <= min(m, L) + G, the group voting after every step (G - 1 steps
 * of skew and the vote's one); 0 for a pair without a query column.  A plain
 * fill runs m + G - 1 steps.
 * The entry points are their plain counterparts without `mode` and with
 * xdrop; saln_ends_free_execute / _plan_destroy and saln_ends_free_aln_count /
 * _get / _free serve them unchanged.  Pairs above the limits:
 * saln_ends_free_xdrop_long_align_batch, below, and its tiled-replay form
 * saln_ends_free_xdrop_replay_align_batch. */
int saln_ends_free_xdrop_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                     uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                     uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                     uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                     uint64_t trace_budget_bytes, int want_cigar,
                                     saln_ends_free_aln **out);
int saln_ends_free_xdrop_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                     const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                     const uint32_t *pair_db, uint64_t n_pairs,
                                     const saln_nw_scoring *scoring, int32_t xdrop,
                                     saln_ends_free_plan **out);

/* X-drop extension of pairs of any length (ends_free_xdrop_long_kernels.hip).
 * saln_ends_free_xdrop_long_align_batch is saln_ends_free_long_align_batch
 * (below) without `mode` and with xdrop: the definition above, the long entry
 * point's arguments, code sizes (saln_ends_free_long_trace_bytes: all m rows),
 * trace budget, chunking and SALN_TRACE_CAP.  The only limit is the range
 * guard, (n + m + 2) * max|parameter| + xdrop < 2^30; a negative xdrop, a pair
 * outside the guard and a NULL matrix are SALN_E_INVALID with a message, before
 * the device is touched.  Records (all fields but `reserved`) and words depend
 * on the pair, the scoring and X alone: they are the class form's for every
 * pair both can run.
 *  - A pair within the class limits (saln_ends_free_long_pair_path: long_fill
 *    0) runs saln_ends_free_xdrop_align_batch's fill and reports its steps.
 *  - Every other pair runs the chunked X-drop fill: chunks of 1,024 query
 *    columns, left to right.  A chunk runs only the rows from its first to its
 *    last row that can hold an unpruned cell (from row 1 where row 0 is
 *    unpruned at its left edge, else from the first row whose cell in the
 *    column left of it is unpruned; at least down to the last row the chunk
 *    before ran), and the pair ends at the first chunk that nothing unpruned
 *    enters.  Codes of rows and chunks that did not run are not written; the
 *    walk never reads them.
 *  - `reserved`: the row-loop steps summed over the chunks the pair ran,
 *    saturating at 2^32 - 1: per chunk at most (its rows) + 63 + 1.
 *  - Workspace: per wave one boundary column of 16 bytes per db row (P, I and
 *    B of the next chunk's first column), at most 256 MiB per launch. */
int saln_ends_free_xdrop_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                          uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                          uint64_t trace_budget_bytes, int want_cigar,
                                          saln_ends_free_aln **out);

/* Pairs of any length (ends_free_long_kernels.hip, ends_free_long_host.cpp).
 * saln_ends_free_long_align_batch is saln_ends_free_align_batch without the
 * two length limits: the same arguments, modes, scoring domain, range guard,
 * pair conventions, want_cigar, trace_budget_bytes chunking, SALN_TRACE_CAP
 * meaning and handle (saln_ends_free_aln_count / _get / _free serve it).  The
 * only limit left is the range guard, (n + m + 2) * max|parameter| < 2^30.
 * A pair within the limits above (n <= 1,024 and m <= 65,000) runs the class
 * fills; every other pair runs the chunked fill: one pair per wave, the query
 * in chunks of 1,024 columns left to right, every db row in each chunk, the
 * last column of a chunk handed to the next through a boundary column in
 * device memory, the db read as the rows come.  The definitions above
 * (recurrences, tie rules, the walk's choices) are unchanged, so a pair's
 * record and words depend on nothing but the pair and the scoring, whichever
 * fill ran it.  A pair's codes are saln_ends_free_long_trace_bytes.
 * Boundary workspace: 8 * m bytes per pair in flight.  Every wave of a
 * chunked-fill launch owns one slot of 8 bytes per row of the launch's
 * longest db and takes pairs from a counter; a launch runs min(pairs, 4,096,
 * 256 MiB / slot bytes) waves and at least one, so the workspace stays within
 * 256 MiB however large the batch; a single db above 33,554,432 rows runs
 * alone in a slot of its own size. */
int saln_ends_free_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                    uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                    uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                    uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                                    uint64_t trace_budget_bytes, int want_cigar,
                                    saln_ends_free_aln **out);
/* Host only: bytes of trace codes of one pair under the long entry point, the
 * one place the long layout's size is computed (the batch's chunking asks
 * it).  A pair within the class limits: saln_ends_free_trace_bytes.  Every
 * other pair: len_db rows of ceil(len_q / 16) * 8 bytes, rounded up to a
 * multiple of 8; 0 when a sequence is empty.  SALN_E_INVALID as
 * saln_ends_free_long_pair_path. */
int saln_ends_free_long_trace_bytes(uint64_t len_q, uint64_t len_db, uint64_t *bytes);
/* Host only: the fill a pair takes under the long entry point; the launch
 * code asks the same function.  *long_fill: 1 the chunked fill, 0 a class
 * fill (saln_ends_free_pair_geometry tells which).  *chunks: the pair's
 * 1,024-column chunks; 1 for the class fills.  SALN_E_INVALID only where the
 * range guard cannot hold for any scoring: len_q + len_db + 2 >= 2^30. */
int saln_ends_free_long_pair_path(uint64_t len_q, uint64_t len_db, int32_t *long_fill,
                                  uint32_t *chunks);

/* Alignments of long pairs without their n x m codes: the tiled replay
 * traceback (ends_free_replay_kernels.hip, ends_free_replay_host.cpp).
 * saln_ends_free_replay_align_batch is saln_ends_free_long_align_batch with
 * another way to the words of a pair of the chunked fill: the same arguments,
 * handle, records and words, word for word.  A pair within the class limits
 * runs as under the other entry points.  A pair of the chunked fill is filled
 * score only, keeping the boundary column of every chunk and, after every
 * R-th db row, a checkpoint row (P and the next row's D of every column).
 * The walk then runs tile by tile, a tile being one 1,024-column chunk times
 * one block of R rows: a wave fills the tile's codes again from the checkpoint
 * row above it and the boundary column left of it, the pair's walk follows
 * them until it leaves the tile or ends, and the next round fills the tile it
 * left for.  The host queues chunks + row blocks - 1 rounds of the chunk's
 * largest pair, which is as many tiles as a walk can visit, and waits for
 * none; a pair unfinished after them has status SALN_INTERNAL and no words
 * (never expected).  R is option "ends_free.tile_rows": 64, 128, 256, 512 or
 * 1024 (the default); with any other value the batch is SALN_E_INVALID.  Every
 * allowed value gives the same results.
 * trace_budget_bytes bounds a chunk's sum of saln_ends_free_replay_bytes; a
 * pair whose footprint alone exceeds it gets score, ends, SALN_TRACE_CAP,
 * begins -1 and no words.  want_cigar == 0: as the long entry point. */
int saln_ends_free_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                      uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                      uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                      uint64_t n_pairs, int32_t mode, const saln_nw_scoring *scoring,
                                      uint64_t trace_budget_bytes, int want_cigar,
                                      saln_ends_free_aln **out);
/* Host only: the bytes one pair holds against trace_budget_bytes under the
 * replay entry point, the one place they are computed (the batch's chunking
 * asks it).  tile_rows: R, or 0 for the process registry's option value.  A pair
 * within the class limits: saln_ends_free_trace_bytes.  Every other pair, with
 * chunks = ceil(len_q / 1024): (chunks - 1) * len_db * 8 (boundary columns)
 * + floor((len_db - 1) / R) * chunks * 1024 * 8 (checkpoint rows)
 * + R * 512 (the tile in work); 0 when a sequence is empty.  SALN_E_INVALID as
 * saln_ends_free_long_pair_path, and for an R outside the five values. */
int saln_ends_free_replay_bytes(uint64_t len_q, uint64_t len_db, uint32_t tile_rows, uint64_t *bytes);

/* X-drop extension of long pairs with their CIGARs by tiled replay
 * (ends_free_xdrop_replay_kernels.hip, ends_free_replay_host.cpp).
 * saln_ends_free_xdrop_replay_align_batch is
 * saln_ends_free_xdrop_long_align_batch with another way to the words of a
 * pair of the chunked path: the same arguments, handle and refusals (a negative
 * xdrop, a pair outside the range guard with X, a NULL matrix), and option
 * "ends_free.tile_rows" outside 64, 128, 256, 512, 1024 is SALN_E_INVALID too;
 * all before the device is touched.  Records (all fields but `reserved`) and
 * words are the same, word for word.
 *  - A pair within the class limits runs the class X-drop fill and the
 *    ordinary walk, as under the other X-drop entry points, steps included.
 *  - A pair of the chunked path is filled score only by the keep form of the
 *    chunked X-drop fill.  Per chunk that ran it keeps a header (the window of
 *    rows lo_c .. z_c the chunk ran, and B above the window), the boundary
 *    column's entries (P, I, B) of those rows and, for every R-th db row inside
 *    the window, a checkpoint row (P, the next row's D, and B of every
 *    column).  Every chunk runs on until its last lane has run row max(last
 *    live row, lo_c), so every kept row of a window is whole.
 *  - The rounds are the replay's: a wave fills again the codes of the rows of
 *    one tile that lie inside the chunk's window, from the checkpoint row above
 *    them or, where the window starts in the tile, from the fill's own start,
 *    with the X-drop rule (B is part of the kept state, so the cells are the
 *    same integers); the extension walk follows them unchanged, since it never
 *    reads a pruned cell.  The tile fill reads no entry outside the windows
 *    the headers state: what lies there is stale memory.  chunks + row blocks
 *    - 1 rounds of the largest pair are queued and none is waited for; a pair
 *    unfinished after them has SALN_INTERNAL and no words (never expected).
 *  - `reserved`: the forward pass's row-loop steps, per chunk at most (its
 *    rows) + 63 + 1; the tile fills are not counted.  It need not equal the
 *    long entry point's value: the last chunk drains as the others do.
 *  - trace_budget_bytes bounds a chunk's sum of
 *    saln_ends_free_xdrop_replay_bytes; a pair whose footprint alone exceeds it
 *    gets score, ends, SALN_TRACE_CAP, begins -1 and no words.
 *  - want_cigar == 0: the long X-drop entry point's fill.
 * No boundary workspace: a pair's columns lie in its own footprint, and a
 * launch runs min(pairs, 4,096) waves. */
int saln_ends_free_xdrop_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                            uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                            uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                            uint64_t n_pairs, const saln_nw_scoring *scoring, int32_t xdrop,
                                            uint64_t trace_budget_bytes, int want_cigar,
                                            saln_ends_free_aln **out);
/* Host only: the bytes one pair holds against trace_budget_bytes under the
 * X-drop replay entry points, the one place they are computed (the batch's
 * chunking asks it).  tile_rows: R, or 0 for the process registry's option
 * value.  A pair within the class limits: saln_ends_free_trace_bytes.  Every
 * other pair, with chunks = ceil(len_q / 1024): chunks * 16 (a header per
 * chunk) + (chunks - 1) * len_db * 16 (boundary columns: P, I, B)
 * + floor((len_db - 1) / R) * chunks * 1024 * 16 (checkpoint rows: P, D, B)
 * + R * 512 (the tile in work); 0 when a sequence is empty.  The size is for
 * all rows: the windows are not known before the fill.  SALN_E_INVALID as
 * saln_ends_free_replay_bytes. */
int saln_ends_free_xdrop_replay_bytes(uint64_t len_q, uint64_t len_db, uint32_t tile_rows, uint64_t *bytes);

/* Ends-free alignment under a substitution matrix (protein scoring under a
 * BLOSUM or PAM style table, IUPAC nucleotide codes, transition /
 * transversion scoring).  Everything above stays as it is written: the
 * recurrences, the three modes, the tie rules, the walk's choices, the record,
 * the limits, the chunking and the handle.  Only s(i, j) changes:
 *   s(i, j) = score[code[d[i-1]]][code[q[j-1]]]
 * row: the db symbol, column: the query symbol.  The matrix need not be
 * symmetric.  '=' and 'X' in the words stay byte comparisons of d[i-1] and
 * q[j-1], whatever the two bytes score (two different bytes of one symbol are
 * 'X').  code is a total map of the 256 byte values into 0 .. n_sym - 1, so a
 * kernel never indexes outside the table, also under the device-resident plan
 * where the host does not see the sequences.
 * Domain: 1 <= n_sym <= 32, reserved all 0, every code[] entry < n_sym,
 * gap_open <= 0, gap_extend < 0 and at least one entry of
 * score[0 .. n_sym)[0 .. n_sym) > 0; anything else is SALN_E_INVALID with a
 * message.  Range guard: the engine's own, (n + m + 2) * max|parameter| < 2^30,
 * the parameters being gap_open, gap_extend and the entries inside n_sym x
 * n_sym.
 * On the device the table has one more column, which the pad columns behind a
 * query's end read; it is strictly negative in every row (the role mismatch < 0
 * plays under the scalar scoring: a pad cell then never holds local's best). */
typedef struct {
    uint8_t n_sym;            /* 1 .. 32 */
    uint8_t reserved[3];      /* 0 */
    int32_t gap_open, gap_extend;
    uint8_t code[256];        /* byte -> symbol, every entry < n_sym */
    int8_t  score[32][32];    /* [db symbol][query symbol]; entries at or above n_sym ignored */
} saln_sub_matrix;            /* 1,292 bytes */
/* Host only (no device needed): the domain rules above.  *max_abs (optional):
 * the largest magnitude among gap_open, gap_extend and the entries inside
 * n_sym x n_sym, what the range guard multiplies.  Every entry point below
 * calls it. */
int saln_sub_matrix_check(const saln_sub_matrix *m, int32_t *max_abs);
/* saln_ends_free_align_batch, saln_ends_free_long_align_batch and
 * saln_ends_free_replay_align_batch under a matrix (NULL: SALN_E_INVALID; there
 * is no default matrix).  Every other argument, the limits, the chunking,
 * SALN_TRACE_CAP and the handle (saln_ends_free_aln_count / _get / _free) as
 * there. */
int saln_ends_free_sub_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                   uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                   uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                   uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                   uint64_t trace_budget_bytes, int want_cigar,
                                   saln_ends_free_aln **out);
int saln_ends_free_sub_long_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                        uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                        uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                        uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                        uint64_t trace_budget_bytes, int want_cigar,
                                        saln_ends_free_aln **out);
int saln_ends_free_sub_replay_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                          uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                          uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                          uint64_t n_pairs, int32_t mode, const saln_sub_matrix *matrix,
                                          uint64_t trace_budget_bytes, int want_cigar,
                                          saln_ends_free_aln **out);
/* saln_ends_free_plan_create under a matrix: the device-resident score-only
 * form (the database-search shape).  The plan owns the table's device copy;
 * saln_ends_free_execute and saln_ends_free_plan_destroy serve it unchanged. */
int saln_ends_free_sub_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                   const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                   const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                   const saln_sub_matrix *matrix, saln_ends_free_plan **out);
/* The X-drop extension (above) under a matrix. */
int saln_ends_free_sub_xdrop_align_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off,
                                         uint64_t n_q, const uint8_t *db_seq, const uint64_t *db_off,
                                         uint64_t n_db, const uint32_t *pair_q, const uint32_t *pair_db,
                                         uint64_t n_pairs, const saln_sub_matrix *matrix, int32_t xdrop,
                                         uint64_t trace_budget_bytes, int want_cigar,
                                         saln_ends_free_aln **out);
int saln_ends_free_sub_xdrop_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                         const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                         const uint32_t *pair_db, uint64_t n_pairs,
                                         const saln_sub_matrix *matrix, int32_t xdrop,
                                         saln_ends_free_plan **out);
/* saln_ends_free_xdrop_long_align_batch (above) under a matrix. */
int saln_ends_free_sub_xdrop_long_align_batch(saln_context *ctx, const uint8_t *q_seq,
                                              const uint64_t *q_off, uint64_t n_q, const uint8_t *db_seq,
                                              const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                              const uint32_t *pair_db, uint64_t n_pairs,
                                              const saln_sub_matrix *matrix, int32_t xdrop,
                                              uint64_t trace_budget_bytes, int want_cigar,
                                              saln_ends_free_aln **out);
/* saln_ends_free_xdrop_replay_align_batch (above) under a matrix. */
int saln_ends_free_sub_xdrop_replay_align_batch(saln_context *ctx, const uint8_t *q_seq,
                                                const uint64_t *q_off, uint64_t n_q, const uint8_t *db_seq,
                                                const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                                const uint32_t *pair_db, uint64_t n_pairs,
                                                const saln_sub_matrix *matrix, int32_t xdrop,
                                                uint64_t trace_budget_bytes, int want_cigar,
                                                saln_ends_free_aln **out);

/* Score-only search (ends_free_score_kernels.hip, ends_free_score_host.cpp):
 * what does each of these pairs score?  The first step of a database search:
 * score many pairs, rank, then align the few that matter with the entry
 * points above.
 *  - scores[p] is exactly the `score` that saln_ends_free_align_batch gives
 *    pair p under the same mode and scoring.  Nothing else is reported: no end
 *    cell, no state.
 *  - Pair lists, argument errors and the four modes as there; SALN_MODE_GLOBAL
 *    and every other value are SALN_E_INVALID.  Limits are the class limits
 *    (1,024 columns, 65,000 rows, the same messages; no long form), and the
 *    range guard (n + m + 2) * max|parameter| < 2^30 stays in force.
 *    Arguments are validated before the device is touched.
 *  - A pair of SALN_MODE_LOCAL or SALN_MODE_SEMI_GLOBAL runs the packed fill,
 *    16-bit values and two pairs per lane group, when its values fit int16.
 *    With S+ the largest positive s(i, j) (match, or the matrix's largest
 *    entry, at least 0) and A the largest |parameter|, gaps included (what
 *    saln_sub_matrix_check yields), a pair of n columns and m rows is packed
 *    iff
 *        min(n, m) * S+ + 4 * A < 2^15                   both modes, and
 *        (n + 4) * A < 2^15                              semi-global.
 *    Every other pair, and every pair of SALN_MODE_OVERLAP and
 *    SALN_MODE_EXTEND, runs the i32 fill of saln_ends_free_plan_create.  The
 *    score does not depend on the path.  saln_ends_free_score_path is the one
 *    place the path is decided; the plan asks the same function.
 *  - Option "ends_free.score_i16": 1 (the default) as above, 0 the i32 fill
 *    for every pair; any other value makes these entry points SALN_E_INVALID.
 * saln_ends_free_score_batch: host sequences in, scores[n_pairs] (host) out. */
int saln_ends_free_score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                               const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                               const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                               const saln_nw_scoring *scoring, int32_t *scores);
int saln_ends_free_sub_score_batch(saln_context *ctx, const uint8_t *q_seq, const uint64_t *q_off, uint64_t n_q,
                                   const uint8_t *db_seq, const uint64_t *db_off, uint64_t n_db,
                                   const uint32_t *pair_q, const uint32_t *pair_db, uint64_t n_pairs,
                                   int32_t mode, const saln_sub_matrix *matrix, int32_t *scores);
/* Device-resident form: plan from host offsets and a pair list (NULL =
 * all-vs-all), execute on device sequences (same CSR layout) into device
 * d_scores[n_pairs], any number of times.  Stream as the other plans.  The
 * plan owns the workspace of its i32 pairs: its executes must not overlap. */
typedef struct saln_ends_free_score_plan saln_ends_free_score_plan;
int saln_ends_free_score_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                     const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                     const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                     const saln_nw_scoring *scoring, saln_ends_free_score_plan **out);
int saln_ends_free_sub_score_plan_create(saln_context *ctx, const uint64_t *q_off, uint64_t n_q,
                                         const uint64_t *db_off, uint64_t n_db, const uint32_t *pair_q,
                                         const uint32_t *pair_db, uint64_t n_pairs, int32_t mode,
                                         const saln_sub_matrix *matrix, saln_ends_free_score_plan **out);
int saln_ends_free_score_execute(saln_ends_free_score_plan *plan, const uint8_t *d_q_seq,
                                 const uint8_t *d_db_seq, int32_t *d_scores, void *stream);
/* How many of the plan's pairs run the packed fill and how many the i32 fill
 * (either output may be NULL). */
int saln_ends_free_score_plan_info(const saln_ends_free_score_plan *plan, uint64_t *packed_pairs,
                                   uint64_t *i32_pairs);
int saln_ends_free_score_plan_destroy(saln_ends_free_score_plan *plan);
/* Host only: *packed = 1 iff a pair of len_q columns and len_db rows runs the
 * packed fill under `mode` and a scoring with the given S+ (max_pos) and A
 * (max_abs), by the formula above (option "ends_free.score_i16" not counted).
 * SALN_E_INVALID for a mode outside the four, above 1,024 columns or 65,000
 * rows, for a negative max_pos or max_abs and for a NULL output. */
int saln_ends_free_score_path(uint64_t len_q, uint64_t len_db, int32_t mode, int32_t max_pos, int32_t max_abs,
                              int32_t *packed);
/* Host only: the workgroup of a packed launch, saln_ends_free_fill_geometry's
 * rule for groups that stage two db rows: *groups lane groups (two pairs
 * each), 256 / lanes of them, lowered until groups * 2 * (ld_max + 2 * lanes)
 * bytes fit 64 KB (less the matrix block's 1,408 bytes with has_matrix != 0);
 * never below 1.  *lds_bytes: those bytes.  Errors as there.  The launch code
 * asks the same function. */
int saln_ends_free_score_geometry(uint64_t len_q, uint64_t ld_max, int has_matrix, uint32_t *groups,
                                  uint32_t *lds_bytes);

/* --------------------------------------------------------------------- FASTA
 * Replaces `pub fn parse_fasta(path: PathBuf) -> Result<Records>`
 * (parse.rs:54-99): extension must be exactly fa|fasta|fna; '>' opens a record
 * whose name includes the '>'; bytes outside {A,G,C,T,N} in sequence lines are
 * dropped and reported (returns SALN_E_FASTA_CHARS with the records still
 * valid, like CharError{res,chars}). */
typedef struct saln_records saln_records;
int saln_parse_fasta(const char *path, saln_records **out, uint8_t *bad_chars, uint64_t bad_cap,
                     uint64_t *n_bad);
int saln_parse_fasta_buffer(const uint8_t *buf, uint64_t len, saln_records **out,
                            uint8_t *bad_chars, uint64_t bad_cap, uint64_t *n_bad);
uint64_t saln_records_count(const saln_records *r);
int saln_records_get(const saln_records *r, uint64_t i, const uint8_t **name, uint64_t *name_len,
                     const uint8_t **seq, uint64_t *seq_len);
void saln_records_free(saln_records *r);

#ifdef __cplusplus
}
#endif
#endif /* SALN_H */
