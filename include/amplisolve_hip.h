/*
 * include/amplisolve_hip.h -- C ABI of libamplisolve_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of AmpliSolve is its two command lines and their files
 * (SURVEY.md section 8b); the reference exposes no library interface.  This
 * header is the thin C ABI between the C++ host that re-states those command
 * lines (amplisolve_amd/csrc/host) and the hand-written HIP kernels that do the
 * per-position arithmetic.  Every entry point names the reference code it
 * replaces:
 *   EE:n = /root/reference/source_codes/AmpliSolveErrorEstimation.cpp:n
 *   VC:n = /root/reference/source_codes/AmpliSolveVariantCalling.cpp:n
 *
 * Conventions: C linkage, plain pointers and sizes, no exceptions across the
 * boundary.  Every call returns AMPLI_OK (0) or a negative AMPLI_E_* code;
 * ampli_last_error(ctx) gives the detail text.  A context is bound to one
 * device and one HIP stream; all work is enqueued on that stream and is
 * asynchronous unless stated.  The caller owns every buffer.  Pointers named
 * d_* are DEVICE pointers (hipMalloc / ampli_dev_alloc / a torch CUDA tensor).
 * There is no CPU fallback: without a GPU every compute entry point fails
 * with AMPLI_E_HIP.
 *
 * Record arrays (the "count SoA"):
 *   int32 recs[n_samples][R][8],  R = P + E, position index fastest-but-one,
 *   one 32-byte vector {Afw,Cfw,Gfw,Tfw,Ars,Crs,Grs,Trs} per (sample, record):
 *   a dense (position x strand x base) tensor per sample.  Xfw = X - Xrs
 *   (EE:1155-1158, VC:767-770), Xrs = the ASEQ reverse-strand column.
 *   Absent record (the sample's file has no line for the position):
 *   recs[..][0] == AMPLI_ABSENT.
 *   P = unique panel positions.  Record r < P is the first line of position r
 *   in the sample's file.  E = extra occurrences: a position covered by
 *   overlapping amplicons is listed again in every ASEQ file and each line is
 *   a record of its own (it counts in the quorum, the sums and the germ-max
 *   sequence).  Extras of position p are records P+dup_off[p] ..
 *   P+dup_off[p+1]-1 and are visited right after record (s,p) (file order);
 *   ext_pos[e] is the position of extra e.  E = 0: pass NULL for both.
 *   Samples are in the reference's visit order (EE:1081 / VC:672).
 *   Counts must be < 2^24 (AMPLI_E_RANGE is reported by the host packer).
 */
#ifndef AMPLISOLVE_HIP_H
#define AMPLISOLVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "amplisolve_types.h" /* the AMPLI_* constants and parameter structs named below that the host library shares */

#ifdef __cplusplus
extern "C" {
#endif

#define AMPLI_ABI_VERSION 5
#define AMPLI_ABSENT INT32_MIN
/* record layouts, same field order in all of them:
 *   AMPLI_RECORDS_I32  int32 recs[n_samples][R][8], 32 B per record, absent: recs[..][0] == INT32_MIN
 *   AMPLI_RECORDS_U24  8 x 24-bit little-endian fields, 24 B per record, absent: field 0 == 0xFFFFFF; for counts
 *                      <= 2^24 - 2, which is every count the fast kernels accept anyway (a quarter fewer HBM bytes)
 *   AMPLI_RECORDS_U16  uint16 recs[n_samples][R][8], 16 B per record, absent: recs[..][0] == 0xFFFF; for cohorts
 *                      whose every count is <= 65534 (half the HBM bytes) */
#define AMPLI_RECORDS_I32 0
#define AMPLI_RECORDS_U16 1
#define AMPLI_RECORDS_U24 2

#define AMPLI_OK 0
#define AMPLI_E_INVALID (-1)  /* bad argument */
#define AMPLI_E_HIP (-2)      /* HIP runtime error / no device */
#define AMPLI_E_NOMEM (-3)
#define AMPLI_E_ENVELOPE (-4) /* double accumulators left the exactness envelope */
#define AMPLI_E_CAPACITY (-5) /* compact call list overflowed; n_calls holds the needed size */
#define AMPLI_E_RANGE (-6)    /* a count does not fit the kernels' integer envelope */
#define AMPLI_E_COMM_TIMEOUT (-7) /* ampli_comm_create: ncclCommInitRank did not return in time.  A helper thread is still inside
                                   * RCCL on this device: the process MUST end now -- print, flush, _exit(1); do not destroy the
                                   * context, do not run static destructors, never re-exec */

/*
 * Output contracts.  What a call does to the caller's output buffers, whatever they held before -- none of them needs to be
 * zeroed unless a line below says "added to" or "OR-ed into" (tests/test_gpu_output_contracts.py hands every entry point
 * poisoned, fenced buffers and checks each line).  No call writes a byte outside the extents given here.
 *   (C1) call mask (ampli_poisson_call / _records / _blocks, ampli_loo_call_records): CLEARED AND FULLY OVERWRITTEN by the call,
 *        all [n_samples][P + E] bytes, in every mode, with and without position ranges, captured or not.
 *   (C2) the mask's pad bytes: the buffer is rounded up to a multiple of 4 bytes; the up to 3 bytes behind the last record may be
 *        zeroed by the call and mean nothing.  Nothing behind them is touched.
 *   (C3) dense outputs -- d_q, d_af, d_thr_loo; d_rate, d_code, d_thr, d_germ_val, d_germ_present of every ampli_error_* entry
 *        point that takes them; d_min_reads and d_status of ampli_limit_records; d_power and d_lod of ampli_power_records;
 *        d_recs16 / d_recs24 of ampli_records_pack16 / 24: FULLY OVERWRITTEN, every element (d_germ_val holds a value of no
 *        meaning where d_germ_present is 0; d_q holds -1 where a score was not evaluated).
 *   (C4) ADDED TO (zero them for a count of one call): d_callable_pos, d_callable_sample of ampli_loo_call_records; d_counts of
 *        ampli_limit_records and of ampli_power_records.
 *   (C5) OR-ED INTO (zero them first): every flag word -- d_flags of the ampli_error_* entry points and of ampli_loo_call_records,
 *        d_overflow of ampli_records_pack16 / 24, the flag word in the 64-byte tail of a slice block.  A call never clears a bit.
 *   (C6) the sliced exchange buffers d_sums / d_gm (ampli_error_reduce_sliced, ampli_error_reduce_records_sliced,
 *        ampli_acc_to_slices) and the slice block of ampli_error_finalize_slice: every entry of a position < P of the addressed
 *        batch is overwritten; entries of positions >= P (the tail of the last slice that holds positions, whole slices behind
 *        it), the other batches of a group and the 60 bytes behind a block's flag word are NEVER WRITTEN and never read.
 *   (C7) accumulator table: the eight planes are overwritten (accumulate == 0) or folded into (accumulate != 0) over their
 *        [..][P] extents; the PADDING between the planes and behind the last one, up to ampli_acc_bytes(P), is NEVER WRITTEN.
 *        gm_first, gm_first_af and gm_rest hold values of no meaning where gm_n says that no (no second) record qualified.
 *   (C8) call list: segment k is written from its start; an entry is written only at an index below both the segment's count and
 *        capacity / AMPLI_CALL_SHARDS.  Entries beyond the count are UNTOUCHED, and no segment is written past its end however
 *        far its counter runs beyond it.
 *   (C9) d_n_calls: the AMPLI_CALL_SHARDS counters (words k * AMPLI_CALL_COUNTER_STRIDE) are RESET BY THE CALL ITSELF, whatever
 *        they held -- with position ranges each range resets the shards dealt to it; the words between the counters mean nothing
 *        and may be zeroed.
 *   (C10) panel dispersion (tests/test_gpu_dispersion_contracts.py): d_x2 and d_rinv of ampli_dispersion_records are FULLY OVERWRITTEN
 *        (accumulate == 0) or ADDED TO (accumulate != 0) over their [2][4][P] extents; d_sample_x2, d_sample_expect and d_sample_terms
 *        are FULLY OVERWRITTEN, all n entries, or all three NULL; d_z, d_phi and d_status of ampli_dispersion_finalize are FULLY
 *        OVERWRITTEN; its d_counts[4] are ADDED TO.  The partials of the per-sample sums live in the context's workspace.
 *   (C11) sample identity (tests/test_gpu_concordance_contracts.py): d_planes of ampli_genotype_planes_records is FULLY OVERWRITTEN, every
 *        word of the chunk's [n_samples][6][W] rows, the bits at and beyond P zero; d_counts of ampli_concordance_pairs is FULLY
 *        OVERWRITTEN, all [n_a][n_b][5] counts (with d_planes_a == d_planes_b too).  Neither touches anything else; the planes are
 *        inputs of ampli_concordance_pairs and stay as they are.
 *   (C12) cross-sample contamination (tests/test_gpu_contamination_contracts.py): d_sums of ampli_contamination_records is FULLY
 *        OVERWRITTEN, all [recs->n_samples][n_b][9] sums, whatever it held and however many position slices the launch is cut into (the
 *        call clears it itself where slices are added into it).  Nothing else is written -- the other chunks' rows of a larger matrix
 *        included -- and the records and both plane sets stay as they are.  Plane rows at and beyond n_samples / n_b and plane words
 *        at and beyond W are never read.
 *   (C13) amplicon depth sums (tests/test_gpu_amplicon_contracts.py): d_sums of ampli_amplicon_depth_records is FULLY OVERWRITTEN, all
 *        [recs->n_samples][A][4] sums, with plain stores (one wave owns a cell: nothing is cleared, nothing is added to), empty lists
 *        included (four zeros).  Nothing else is written -- the other chunks' rows of a larger matrix included.  d_amp_off is read at
 *        [0, A], d_amp_pos at [0, W) at most, a record only at a listed position below P of a row below n_samples.
 *   (C14) amplicon reference: ampli_amplicon_reference FULLY OVERWRITES d_total [N], d_ref [A][2] and d_status [A] and writes nothing
 *        else; d_sums and d_use stay as they are.
 *   (C15) amplicon ratios: ampli_amplicon_ratio FULLY OVERWRITES d_total [S], d_centre [S], d_k [S], d_ratio [S][A] and d_z [S][A]
 *        (a NaN is the quiet NaN 0x7FF8000000000000) and writes nothing else; d_sums, d_use, d_ref and d_status stay as they are.
 *   (C16) substitution spectrum (tests/test_gpu_spectrum_contracts.py): d_sums of ampli_spectrum_records is FULLY OVERWRITTEN, all
 *        [recs->n_samples][C][9] sums, whatever it held and however many position segments the launch is cut into (the call clears it
 *        itself where segments are added into it); a class no position has gets nine zeros.  Nothing else is written -- the other
 *        chunks' rows of a larger matrix included.  d_ref_code and d_class are read at [0, P), a record only at a position below P
 *        whose reference code and class are valid, of a row below n_samples.
 *   (C17) panel-of-normals exceedance (tests/test_gpu_exceedance_contracts.py): ampli_exceedance_records with accumulate == 0 FULLY
 *        OVERWRITES d_elig, all [n_t][P] counts, and d_ge, all [n_t][P][4][2] cells, AMPLI_EXCEEDANCE_NA included, whatever they held;
 *        with accumulate != 0 it ADDS TO d_elig and to the evaluated cells of d_ge and writes NA to the others.  Nothing else is
 *        written.  d_ref_code is read at [0, P), a record only at a position below P of a row below n_t / n_n.
 *   (C18) overdispersion-aware calling (tests/test_gpu_overdispersion_contracts.py): d_s2 of ampli_overdispersion_records is FULLY
 *        OVERWRITTEN (accumulate == 0) or ADDED TO (accumulate != 0) over its [2][4][P] extent; d_omega of ampli_overdispersion_finalize
 *        is FULLY OVERWRITTEN, all [2][4][P] cells; d_q of ampli_nb_score_records is FULLY OVERWRITTEN, all [n_t][P][4][2] cells,
 *        AMPLI_NB_NA included, whatever it held.  Nothing else is written -- the other chunks' rows of a larger matrix included.  d_thr
 *        and d_omega are read at [0, 8 P) at most, d_ref_code at [0, P), a record only at a position below P of a row below n_t.
 *   (C19) paired comparison (tests/test_gpu_paired_contracts.py): d_s of ampli_pair_score_records is FULLY OVERWRITTEN, all
 *        [n_pairs][P][4][2] cells, AMPLI_PAIR_NA included, whatever it held.  Nothing else is written.  d_pairs is read at [0, 2 n_pairs),
 *        d_ref_code at [0, P), a record only at a position below P of a row that a pair names and that lies in its chunk.
 *   (C20) false-discovery control (tests/test_gpu_fdr_contracts.py): d_a [rows][P][4] and d_m [rows] of ampli_fdr_adjust are FULLY
 *        OVERWRITTEN, AMPLI_FDR_NA included, whatever they held; d_rank [rows][P][4] is FULLY OVERWRITTEN when it is not NULL.  d_work
 *        is written only inside its first work_bytes bytes (ampli_fdr_workspace_bytes(rows, P) of them are used).  d_s is read at
 *        [0, 8 rows P) and never written.  Nothing else is written.
 *   (C21) in-silico dilution (tests/test_gpu_dilution_contracts.py): d_out of ampli_dilute_records is FULLY OVERWRITTEN, all
 *        [n_mix][P][8] words, ABSENT records included, and d_flags is FULLY OVERWRITTEN, all [n_mix] words, whatever they held.  Nothing
 *        else is written.  d_mix is read at [0, n_mix), a record only at a position below P, of a row that a valid mixture names.
 *   (C22) tumour-informed monitoring (tests/test_gpu_monitor_contracts.py): d_sums and d_lambda of ampli_monitor_sums_records are FULLY
 *        OVERWRITTEN, all [recs->n_samples][L][6] sums and [recs->n_samples][L][2] doubles, with plain stores (one wave owns a cell:
 *        nothing is cleared, nothing is added to), empty lists included (zeros).  Nothing else is written -- the other chunks' rows of a
 *        larger matrix included.  d_list_off is read at [0, L], d_list_cell at [0, W) at most, d_ref_code at [0, P), d_thr at
 *        [0, 8 P), a record only at a listed position below P of a row below n_samples.
 *   (C23) monitoring controls: d_sums and d_lambda of ampli_monitor_control_records are FULLY OVERWRITTEN, all [n_pairs][R][6] sums and
 *        [n_pairs][R][2] doubles, the zeros of a pair whose row or list is out of range included.  Nothing else is written.  d_pairs
 *        is read at [0, 2 n_pairs), d_cand_off at [0, 5), d_cand_pos at [0, n_cand) at most, a record only at a drawn position below P
 *        of a row that a pair names and that lies in the chunk.
 *   (C24) monitoring scores: d_q of ampli_monitor_score is FULLY OVERWRITTEN, all [n_cells][2] scores, AMPLI_MON_NA included.  Nothing
 *        else is written; d_sums is read at [0, 6 n_cells) and d_lambda at [0, 2 n_cells).
 *   (C25) het-site reference (tests/test_gpu_allelic_contracts.py): ampli_hetsite_reference_records ADDS TO d_ref, all [3][6][P] cells
 *        and nothing else, with plain loads and stores (one lane owns a position: no atomics); the caller clears it once.  d_planes is
 *        read at [0, n_samples 6 W'), W' = ceil(P / 64), a record only at a position below P of a row below n_samples.
 *   (C26) allelic sites: d_q, d_km, d_v and d_code of ampli_allelic_site_records are FULLY OVERWRITTEN, all [n_samples][P] cells
 *        ([n_samples][P][2] words of d_km), untested cells included (AMPLI_AI_NA, zeros, 0.0, the status), every cell stored exactly
 *        once.  Nothing else is written -- the other chunks' rows of a larger plane included.  d_row_g is read at [0, n_samples),
 *        d_planes_g only at rows in [0, n_g), d_ref at [0, 18 P).
 *   (C27) allelic regions: d_sums of ampli_allelic_region_sums is FULLY OVERWRITTEN, all [S][R][5] sums, empty regions included
 *        (zeros).  Nothing else is written.  d_reg_off is read at [0, R], d_reg_pos at [0, W) at most, the site planes only at a
 *        listed position below P of a row below S.
 *   (C28) tumour fraction (tests/test_gpu_fraction_contracts.py): d_est and d_count of ampli_fraction_records are FULLY OVERWRITTEN, all
 *        [recs->n_samples][L][4] doubles and [recs->n_samples][L][2] counts, with plain stores (one wave owns a cell: nothing is
 *        cleared, nothing is added to), empty lists included (AMPLI_TF_NA and zeros).  Nothing else is written -- the other chunks' rows
 *        of a larger matrix included.  d_list_off is read at [0, L], d_list_cell and d_list_w at [0, W) at most, d_ref_code at [0, P),
 *        d_thr at [0, 8 P), a record only at a listed position below P of a row below n_samples.
 *   (C29) amplicon-resolved counting (tests/test_gpu_amplicon_count_contracts.py): ampli_pileup_amplicon_count ADDS TO d_counts inside
 *        [0, W) records, to d_amp_reads inside [0, A) pairs and, when it is not NULL, to the four words of d_stats (zero them for the
 *        counts of one call; batches of one file add up).  Nothing else is written.  d_lo, d_hi, d_reach are read at [0, A), d_amp_off
 *        at [0, A).
 *   (C30) amplicon layers: ampli_amplicon_layers FULLY OVERWRITES d_layers [L][P][8], d_layer_amp [L][P] and d_total [P][8] with plain
 *        stores (one lane owns the cells of a position: nothing is cleared, nothing is added to), positions under no amplicon included
 *        (absent-record markers, -1 and zeros).  Nothing else is written.  d_counts is read only at walk entries below W.
 *   (C31) read-level evidence (tests/test_gpu_evidence_contracts.py): ampli_pileup_evidence ADDS TO d_hist inside [0, P) positions and,
 *        when it is not NULL, to the two words of d_stats (zero them for the counts of one call; batches of one file add up).  Nothing
 *        else is written.
 *   (C32) evidence scores: ampli_evidence_score FULLY OVERWRITES d_int [P][3][3], d_med [P][3][2], d_z2 [P][3] and d_alt_used [P] with
 *        plain stores (one lane owns a cell: nothing is cleared, nothing is added to), untested cells included.  Nothing else is written,
 *        d_hist, d_ref_nt and d_alt_nt included.
 *   (C33) read-level phasing (tests/test_gpu_phase_contracts.py): ampli_pileup_phase ADDS TO d_table inside [0, P) keys and, when it is
 *        not NULL, to the three words of d_stats (zero them for the counts of one call; batches of one file add up).  A cell (i, k) with
 *        i + 1 + k >= P is never written.  Nothing else is written.
 *   (C34) phase scores: ampli_phase_score FULLY OVERWRITES d_int [Q][6], d_score [Q] and d_class [Q] with plain stores (one lane owns a
 *        pair: nothing is cleared, nothing is added to), untested pairs included (-1, 0, -1).  Nothing else is written, d_table,
 *        d_pair_cell and d_pair_nt included; d_table is read only at the cell of a tested pair.
 */
typedef struct ampli_ctx ampli_ctx;

int ampli_abi_version(void);
const char *ampli_strerror(int code);
/* number of HIP devices visible; 0 when there is none (never initialises a device) */
int ampli_device_count(void);
/* the same with the reason when the answer is not a count: the number of devices, or -1 with hipGetDeviceCount's error
 * name and text in msg (cap bytes) */
int ampli_device_probe(char *msg, size_t cap);

/* stream: the hipStream_t to enqueue on (e.g. torch's current stream); NULL is the
 * device's default (null) stream; AMPLI_STREAM_OWN lets the context create and own a
 * non-blocking stream (which does not synchronise with the null stream). */
#define AMPLI_STREAM_OWN ((void *)(intptr_t)-1)
int ampli_ctx_create(int device_ordinal, void *stream, ampli_ctx **out);
/* layout of every record array (d_recs / d_trecs) handed to this context from now on; results are identical */
int ampli_set_record_layout(ampli_ctx *ctx, int32_t layout);
/* device-side conversion 8 x int32 -> 8 x uint16 of n_records records; *d_overflow is OR-ed with 1 when a count does
 * not fit (the caller then stays with AMPLI_RECORDS_I32) */
int ampli_records_pack16(ampli_ctx *ctx, const int32_t *d_recs32, int64_t n_records, void *d_recs16, int32_t *d_overflow);
/* the same for the 24-byte layout (8 x 24 bits); overflow: a count above 2^24 - 2 */
int ampli_records_pack24(ampli_ctx *ctx, const int32_t *d_recs32, int64_t n_records, void *d_recs24, int32_t *d_overflow);
void ampli_ctx_destroy(ampli_ctx *ctx);
const char *ampli_last_error(ampli_ctx *ctx);
int ampli_sync(ampli_ctx *ctx);        /* hipStreamSynchronize */
void *ampli_stream(ampli_ctx *ctx);    /* the hipStream_t in use */

/* memory plumbing */
int ampli_pinned_alloc(size_t bytes, void **out);
int ampli_pinned_free(void *p);
/* pin (page-lock + map for the device) host memory the caller owns, e.g. a record buffer the parsers filled while the runtime
 * was still starting; p / bytes page aligned; ctx (may be NULL) names the device.  ampli_host_unregister before the memory is freed. */
int ampli_host_register(ampli_ctx *ctx, void *p, size_t bytes);
int ampli_host_unregister(void *p);
int ampli_dev_alloc(ampli_ctx *ctx, size_t bytes, void **d_out);
int ampli_dev_free(ampli_ctx *ctx, void *d_p);
int ampli_copy_h2d(ampli_ctx *ctx, void *d_dst, const void *src, size_t bytes); /* async */
int ampli_copy_d2h(ampli_ctx *ctx, void *dst, const void *d_src, size_t bytes); /* async */
int ampli_memset_d(ampli_ctx *ctx, void *d_dst, int byte, size_t bytes);        /* async */

/* events on the context's stream (HIP events; bench.py times kernels with these) */
int ampli_event_create(void **ev);
int ampli_event_destroy(void *ev);
int ampli_event_record(ampli_ctx *ctx, void *ev);
int ampli_event_sync(void *ev);                                         /* hipEventSynchronize */
int ampli_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms); /* synchronises on ev_stop */

/*
 * Accumulator table: what storeGermlineStatistics + the record loop of
 * estimateThresholds leave behind per (position, nucleotide), as planes with the
 * position index fastest.  All planes live in one buffer of ampli_acc_bytes(P)
 * bytes; ampli_acc_bind carves the pointers (buffer order: snt, srd, cnt, nrec, gm_n, gm_first_af, gm_rest,
 * gm_first).  The planes:
 *   snt  double [2][4][P]  sum of X_s + float(RD_s)*float(C) over qualifying records   (EE:1597,1599)
 *   srd  int64  [2][4][P]  sum of RD_s over qualifying records                         (EE:1598,1600)
 *   cnt  int32  [4][P]     qualifying records                                          (EE:1606)
 *   nrec int32  [P]        all records of the position = Value_Hash.count(key)         (EE:1659)
 *   gm_n int32  [4][P]     records qualifying for Germ_Max                             (EE:1251)
 *   gm_first    int32 [4][P]  global sample index of the first qualifying record (INT32_MAX: none; -1: unknown,
 *                             after a gathered merge -- bookkeeping only, last plane of the buffer)
 *   gm_first_af float [4][P]  its AF (the reference discards it, EE:1258-1261; kept to merge shards)
 *   gm_rest     float [4][P]  max AF over the later qualifying records (-inf: none)    (EE:1263-1270)
 * [2] = strand (0 forward, 1 reverse), [4] = nucleotide A,C,G,T.
 * snt|srd|cnt|nrec|gm_n are plain sums over samples: shards merge by addition
 * (RCCL all-reduce SUM per dtype); the gm_* triple merges in sample order
 * (ampli_acc_merge).
 */
typedef struct ampli_acc_table {
    int64_t P;
    double *snt;
    int64_t *srd;
    int32_t *cnt;
    int32_t *nrec;
    int32_t *gm_n;
    int32_t *gm_first;
    float *gm_first_af;
    float *gm_rest;
} ampli_acc_table;

size_t ampli_acc_bytes(int64_t P);
int ampli_acc_bind(void *base, int64_t P, ampli_acc_table *out);

/*
 * error_reduce -- replaces the per-line derivation of storeGermlineStatistics
 * (EE:1149-1232), its running Germ_Max (EE:1251-1296 + C/G/T clones) and the
 * gate/accumulate loop of estimateThresholds (EE:1565-1631 + clones) for S
 * samples.  first_sample = global index of sample 0 of this shard.
 * C, coverage_cutoff as the reference's C_value / coverage_cutoff after its
 * defaulting (EE:372-388).  d_acc: device table (fully overwritten).
 */
int ampli_error_reduce(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E,
                       const uint32_t *d_dup_off, int32_t S, int32_t first_sample, float C,
                       int32_t coverage_cutoff, const ampli_acc_table *d_acc);

/*
 * error_estimate -- error_reduce + error_finalize in one call for a panel that lives on ONE device (the
 * single-GPU command line): the merged per-position state is finalised in the reduce kernel's epilogue, so the
 * accumulator table never travels through HBM (d_acc may be NULL; pass a table to get it as well).  Outputs as
 * for ampli_error_finalize.  Falls back to reduce -> merge -> finalize internally when the sample axis has to be
 * split across workgroups (small panels).
 */
int ampli_error_estimate(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                         int32_t S, float C, int32_t coverage_cutoff, const ampli_acc_table *d_acc, float *d_rate,
                         uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags);

/*
 * A cohort on the device described explicitly -- what the streaming command lines use: a cohort is uploaded in
 * CHUNKS of consecutive samples (visit order) while the next chunk is still being parsed, each chunk in its own
 * buffers and, if need be, its own layout (24-byte records unless a count of the chunk needs int32).
 *   recs        DEVICE, primary records [n_samples][row_stride] in `layout`
 *   row_stride  records between the same position of consecutive samples; 0 = dense (P when `ext` is given, else
 *               P + E).  A padded stride keeps panels whose row is a large power of two off the same HBM channels.
 *   ext         DEVICE, extra-occurrence records [n_samples][ext_stride]; NULL = they follow the primaries inside
 *               each row (the dense interchange layout: recs + P records)
 *   ext_stride  0 = E
 *   E, dup_off [P+1] (error_reduce), ext_pos [E] (poisson_call): as in the classic entry points; a chunk may carry
 *               its own E / dup_off / ext_pos (slots for the multiplicities seen in ITS files)
 *   rd, rd_ext  optional RD column of irregular lines (below)
 */
typedef struct ampli_records {
    const void *recs;
    int64_t row_stride;
    const void *ext;
    int64_t ext_stride;
    int64_t E;
    const uint32_t *dup_off;
    const uint32_t *ext_pos;
    int32_t layout;
    int32_t n_samples;
    /* optional: the RD column of the lines whose RD differs from A+C+G+T (EE:1178-1181, VC:762-765).  The reference
     * goes on to use the column: as the denominator of the Germ_Max AF (EE:1229-1232) and, in the caller, in AF = X/RD
     * and in the forward depth RD - RD_reverse of the Poisson test (VC:814-817, VC:895).  DEVICE int32 rd [n_samples][P],
     * rd_ext [n_samples][E], AMPLI_ABSENT where the line is regular; NULL = every line of the cohort is regular (the
     * fast kernels; a cohort with an RD plane goes through the literal reduce kernel). */
    const int32_t *rd;
    const int32_t *rd_ext;
} ampli_records;

/*
 * error_reduce over one chunk (EE:1149-1296, EE:1565-1631 as ampli_error_reduce).  accumulate == 0: d_acc is
 * overwritten (first chunk); accumulate != 0: d_acc holds the state of the EARLIER samples and receives
 * d_acc (+) chunk -- sums add, the Germ_Max triple composes in sample order, so any chunking of the visit order
 * gives the table of the single pass.  With d_rate / d_code non-NULL the merged state is finalised in the same
 * launch (last chunk; outputs as ampli_error_finalize).  Fully asynchronous on the context's stream.
 */
/* `accumulate` is a set of bits (0 / 1 as before):
 *   AMPLI_REDUCE_ACCUMULATE  d_acc holds the state of the earlier samples (above)
 *   AMPLI_REDUCE_SUMMARY     the caller takes d_acc as STREAMING STATE, not as the bookkeeping of record: gm_n may then count a
 *                            chunk's qualifying records as none / one / two-or-more and gm_first may read -1 (unknown) -- what every
 *                            merge, the sliced store and finalize ask of them is kept, every other plane is exact.  That is what lets
 *                            the compact-state kernel (ampli_set_reduce_compact) carry a streamed uint16 cohort from chunk to chunk;
 *                            chunks that take the general kernel (other layouts, lines with their own RD column) leave exact planes
 *                            and the two compose in either order.  The command lines stream with this bit. */
#define AMPLI_REDUCE_ACCUMULATE 1
#define AMPLI_REDUCE_SUMMARY 2
int ampli_error_reduce_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t first_sample, float C,
                               int32_t coverage_cutoff, const ampli_acc_table *d_acc, int32_t accumulate, float *d_rate,
                               uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags);
/* The last chunk of a SHARD's streamed cohort (one process per GPU): d_acc (+) chunk goes straight into the slice-major
 * exchange buffers of the position-sliced merge below (what ampli_error_reduce_sliced writes for a resident shard), and into
 * d_acc as well when one is given.  d_acc may be NULL when the shard's cohort is this one chunk (accumulate == 0). */
int ampli_error_reduce_records_sliced(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t first_sample, float C,
                                      int32_t coverage_cutoff, const ampli_acc_table *d_acc, int32_t accumulate, int32_t n_slices,
                                      double *d_sums, float *d_gm);

/*
 * The eight threshold sums of d_acc (snt[2][4][P]) in the REFERENCE's own order of addition -- what estimateThresholds'
 * walk of `equal_range` (EE:1555-1606) amounts to with libstdc++: the last file of the visit order first, a position's later
 * lines of a file before its first one -- for cohorts outside the exactness envelope (ampli_error_finalize raised flag bit 0:
 * a sum's partial sums are no longer all exact, so the double depends on the order).  recs = one chunk; a cohort in several
 * chunks is walked from its LAST chunk (accumulate = 0) to its first (accumulate = 1).  Every other plane of d_acc is left as
 * an ordinary ampli_error_reduce_records pass wrote it (they do not depend on the order); ampli_error_finalize on the table then
 * gives the reference's rates (it raises flag bit 0 again: pass d_flags = NULL or ignore the bit).  One lane per position,
 * sequential over the samples: a fallback, not a fast path.
 */
int ampli_error_sums_inorder(ampli_ctx *ctx, const ampli_records *recs, int64_t P, float C, int32_t coverage_cutoff,
                             const ampli_acc_table *d_acc, int32_t accumulate);

/*
 * acc_merge -- ordered combine of nparts partial tables (parts[0] = earliest
 * samples) into d_dst (may alias parts[0]).  Sums add; the germ-max triple
 * composes as the reference's sequential state machine would.  This is the
 * local half of the multi-GPU merge and of in-GPU sample splitting.
 * Synchronises the stream: the list of the parts' pointers is uploaded from the caller's stack.
 */
int ampli_acc_merge(ampli_ctx *ctx, const ampli_acc_table *d_dst, const ampli_acc_table *d_parts,
                    int32_t nparts);

/* Byte regions of a table buffer for the multi-GPU merge: [0, sum_bytes) holds the planes that merge by
 * addition (snt | srd | cnt | nrec | gm_n; reduce each with its own dtype), [gm_offset, gm_offset+gm_bytes)
 * holds gm_n | gm_first_af | gm_rest, 48*P bytes (all-gather it BEFORE gm_n is reduced). */
int ampli_acc_regions(int64_t P, size_t *sum_bytes, size_t *gm_offset, size_t *gm_bytes);

/* The additive planes as ONE float64 buffer [snt 8P | srd 8P | cnt 4P | nrec P] (ampli_acc_packed_len(P) = 21*P
 * doubles) so that the shards merge with a single all-reduce (SUM); the integers are exact in a double. */
int64_t ampli_acc_packed_len(int64_t P);
int ampli_acc_pack(ampli_ctx *ctx, const ampli_acc_table *d_acc, double *d_packed);
int ampli_acc_unpack(ampli_ctx *ctx, const double *d_packed, const ampli_acc_table *d_acc);

/* Multi-GPU fast path (same results as reduce -> pack ... unpack -> gm_merge -> finalize, two launches fewer and no
 * table round trip): error_reduce_packed writes a shard's additive planes straight into the all-reduce buffer
 * (d_acc then only receives the germ-max planes, for the all-gather); error_finalize_merged finalises from the
 * all-reduced buffer and the gathered germ-max regions (rank order = sample order). */
int ampli_error_reduce_packed(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                              int32_t S, int32_t first_sample, float C, int32_t coverage_cutoff,
                              const ampli_acc_table *d_acc, double *d_packed);
int ampli_error_finalize_merged(ampli_ctx *ctx, int64_t P, const double *d_packed, const void *d_gm_regions,
                                int32_t nparts, float C, int32_t coverage_cutoff, float *d_rate, uint8_t *d_code,
                                float *d_thr, float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags);

/* Position-sliced merge (the default multi-GPU exchange; ~2.5x less xGMI traffic than all-reduce + all-gather of whole
 * tables).  With n ranks, rank k owns the positions [k*L, (k+1)*L), L = ampli_slice_len(P, n) (ceil(P/n) rounded up to
 * 64).  Per batch and rank:
 *   ampli_error_reduce_sliced   shard of the normal panel -> d_sums f64 [n][21][L] (planes snt 8 | srd 8 | cnt 4 | nrec 1,
 *                               exact integers in doubles) and d_gm f32 [n][8][L] (germ-max of the shard: first AF of
 *                               EE:1251-1261, -1 when no record qualified | max of the later ones, -inf when none);
 *                               entries of positions >= P are never written (allocate the buffers zeroed)
 *   reduce-scatter(SUM) of d_sums -> the rank's [21][L]; all-to-all of d_gm -> [n][8][L] (chunk k = rank k's pair)
 *   ampli_error_finalize_slice  quorum / rate / NaN / text round trip / Germ_Max sentinel (EE:1659-1714, EE:1260...) of
 *                               the slice, the germ-max pairs folded in rank order = sample order -> one block
 *   all-gather of the blocks    (block = rate f32[8][L] | thr f32[8][L] | germ_val f32[4][L] | code u8[4][L] |
 *                               germ_present u8[4][L] | 64-byte tail holding the int32 exactness flags of the slice; the flag word
 *                               is OR-ed into, like every flag of this library: allocate the block zeroed)
 *   ampli_error_table_unslice   blocks -> the plane-major error table ([2][4][P] ...) every other entry point uses;
 *                               ORs the blocks' flags into *d_flags
 * Results are bit-identical to ampli_error_estimate over all shards in order. */
/* Several independent batches can share ONE round of collectives (fewer, larger messages; fewer cross-stream waits):
 * with ampli_set_slice_group(ctx, G, g) the exchange buffers hold G batches per slice chunk -- d_sums
 * [n][G][21][L], d_gm [n][G][8][L], the reduce-scattered / all-to-all'ed / gathered buffers accordingly [G][21][L],
 * [n][G][8][L], [G][block], [n][G][block] -- and every call of the four entry points below (and of
 * ampli_poisson_call_blocks) addresses batch g of the group.  Default G = 1, g = 0. */
int ampli_set_slice_group(ampli_ctx *ctx, int32_t group_size, int32_t group_index);
int64_t ampli_slice_len(int64_t P, int32_t n_slices);
int ampli_slice_bytes(int64_t P, int32_t n_slices, size_t *sums_bytes, size_t *gm_bytes, size_t *block_bytes);
/* The sums' format (round 4).  AMPLI_SLICE_WIDE (default): the 21 planes above, 168 B per position.  AMPLI_SLICE_SLIM: 14 planes,
 * 112 B per position, the same ONE reduce-scatter of doubles: snt 8 | srd 4 (the two strands' depth sums of a nucleotide in one
 * double: forward + reverse * 2^26) | cnt0 + cnt1 * 2^17 + cnt2 * 2^34 | cnt3 + nrec * 2^17.  Adding doubles adds the fields
 * independently and exactly while every field's total stays below its width, so each of the n shards may use 1/n of a field's
 * range (depth sums < 2^26 / n, counts < 2^17 / n per position): ampli_error_reduce_sliced / ampli_acc_to_slices check that where
 * they pack and raise AMPLI_FLAG_SLICE_RANGE otherwise -- repeat the exchange in the wide format then.  The format applies to
 * every sliced entry point of the context (the [21] in the shapes above becomes ampli_slice_planes(format)); results are
 * bit-identical in both. */
#define AMPLI_SLICE_WIDE 0
#define AMPLI_SLICE_SLIM 1
int ampli_set_slice_format(ampli_ctx *ctx, int32_t format);
int32_t ampli_slice_planes(int32_t format);
int ampli_slice_bytes_fmt(int64_t P, int32_t n_slices, int32_t format, size_t *sums_bytes, size_t *gm_bytes, size_t *block_bytes);
int ampli_error_reduce_sliced(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                              int32_t S, int32_t first_sample, float C, int32_t coverage_cutoff, int32_t n_slices,
                              double *d_sums, float *d_gm);
/* a shard's accumulator table (e.g. built chunk by chunk with ampli_error_reduce_records) -> the slice-major exchange
 * buffers ampli_error_reduce_sliced would have written */
int ampli_acc_to_slices(ampli_ctx *ctx, const ampli_acc_table *d_acc, int32_t n_slices, double *d_sums, float *d_gm);
int ampli_error_finalize_slice(ampli_ctx *ctx, int64_t P, int32_t n_slices, int32_t slice_index,
                               const double *d_sum_slice, const float *d_gm_recv, float C, int32_t coverage_cutoff,
                               void *d_block);
int ampli_error_table_unslice(ampli_ctx *ctx, int64_t P, int32_t n_slices, const void *d_blocks, float *d_rate,
                              uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags);

/* gm_merge -- fold nparts gathered gm regions (region k = shard k, ascending sample order, laid out
 * back to back, gm_bytes each) into d_dst's germ-max planes.  The sequential state machine of
 * EE:1251-1271 composes over shards exactly as ampli_acc_merge does. */
int ampli_gm_merge(ampli_ctx *ctx, const ampli_acc_table *d_dst, const void *d_regions, int32_t nparts);

/*
 * error_finalize -- replaces the quorum/divide/NaN logic of estimateThresholds
 * (EE:1659-1714 + clones) and the Germ_Max sentinel rule (EE:1260,1318,1374,1431).
 *   d_rate [2][4][P] float : float(snt)/float(srd)                       (EE:1679-1680)
 *   d_code [4][P]    uint8 : 0 estimate, 1 below quorum (EE:1659), 2 NaN (EE:1682)
 *   d_thr  [2][4][P] float : the value AmpliSolveVariantCalling reads back from the table text:
 *                            stof(sprintf("%f", rate)) (EE:1704 -> VC:889-890), 0.01f for code != 0
 *                            (EE:2680-2684); computed in exact integer arithmetic on the device
 *   d_germ_val [4][P] float, d_germ_present [4][P] uint8 : Germ_Max cell (EE:2807-2849)
 *   d_flags [1] int32 : bit 0 set when a sum left the exactness envelope
 * Any output pointer except d_code/d_rate may be NULL.
 */
int ampli_error_finalize(ampli_ctx *ctx, const ampli_acc_table *d_acc, float C,
                         int32_t coverage_cutoff, float *d_rate, uint8_t *d_code, float *d_thr,
                         float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags);

/* one emitted call (VC:898 true): everything the post-call annotation needs of the record, so that the host does
 * not have to keep the record array once it is uploaded */
typedef struct ampli_call {
    int32_t sample;   /* index into the T axis of this launch */
    int32_t record;   /* r in [0, R) */
    int32_t alt;      /* 0..3 = A,C,G,T */
    int32_t rd;       /* the RD column of the line (== fw + bw unless the line was irregular, VC:762-765) */
    double q_fw, q_bw;            /* VC:895-896 */
    float af, af_fw, af_bw;       /* VC:772-817: the reported VAFs */
    int32_t k_fw, k_bw;           /* alt reads per strand (Xfw = X - Xrs, Xrs) */
    int32_t fw, bw;               /* strand depths: sums of the four forward / reverse counts (VC:760-761) */
    int32_t flags;                /* AMPLI_CALL_* */
} ampli_call; /* 64 bytes */

/* ampli_call.flags.  The device forms Q = -10 log10 p in fp64 with ROCm's exp / log, the reference in glibc's double and
 * x87 long double (VC:3866-3880): the two agree to ~1e-10, so a Q within 1e-6 of the gate Q >= 5 (VC:898) cannot be decided on
 * the device.  Such (record, alternative) pairs are put on the call list EITHER WAY with AMPLI_CALL_BORDERLINE set; the mask
 * bit follows the device's own value, and the host re-evaluates the pair with the reference's operation sequence before it
 * writes anything (csrc/host/annotate.cpp: score_reference_sequence).  None occurs on Toy_data or the synthetic panels. */
#define AMPLI_CALL_BORDERLINE 1 /* the distance: AMPLI_CALL_GATE_EPS of amplisolve_types.h */

#define AMPLI_CALL_SHARDS 32
#define AMPLI_CALL_COUNTER_STRIDE 16 /* uint64 words between shard counters: one 128-byte line each */
#define AMPLI_CALL_COUNTER_WORDS (AMPLI_CALL_SHARDS * AMPLI_CALL_COUNTER_STRIDE)

#define AMPLI_POISSON_FULL 0      /* evaluate all 6 scores of every record, as the reference does */
#define AMPLI_POISSON_PREFILTER 1 /* skip scores an exact bound proves < 5 (identical outputs) */

/*
 * poisson_call -- replaces the per-line core of callVariants (VC:752-898 and
 * its 11 clones) with mutationRulesPoissonQualityScore / kf_gammaq / kf_lgamma
 * (VC:3721-3884) for T tumour samples.
 *   d_thr [2][4][P] as produced by error_finalize or parsed from the table (std::stof, VC:889-890)
 *   d_ref_code [P]  0..3 = A,C,G,T; 255 = reference base not in ACGT -> record skipped (VC:3290)
 *   d_call_mask [T][R] uint8: bit a set = alt nucleotide a called at that record (4-byte aligned buffer,
 *     rounded up to a multiple of 4 bytes)
 *   d_calls / capacity / d_n_calls: optional compact list of emitted calls, kept as AMPLI_CALL_SHARDS independent
 *     segments so that appends do not serialise on one counter: segment k = entries [k*(capacity/SHARDS), ...),
 *     its fill count is d_n_calls[k*AMPLI_CALL_COUNTER_STRIDE] (a count above capacity/SHARDS means that segment
 *     overflowed: rerun with a larger capacity).  d_n_calls points to AMPLI_CALL_COUNTER_WORDS uint64 words; the
 *     call resets them itself.  Entries are unordered: sort by (sample, record, alt) for the reference's
 *     emission order.  d_n_calls without d_calls just counts.
 *   d_q [T][R][4][2] double, optional dense scores (Q_fw,Q_bw per nucleotide; -1 = not evaluated;
 *     requires mode FULL); d_af [T][R][4][3] float optional dense {AF, AF_fw, AF_bw}.
 * Count domain (ampli_poisson_call, _blocks and _records alike).  Admitted in the int32 layout: eight non-negative counts per
 *   record with FW + BW <= INT32_MAX (what the ASEQ parser admits), and ANY int32 in the RD column (ampli_records.rd / rd_ext).
 *   Inside it every kernel returns the reference's result: counts and depths of 2^24 and more are never skipped in fp32 (not
 *   exact floats) but scored; a forward depth RD - BW of 0 gives Q = 100, a negative one (as a negative threshold cell) NaN and
 *   no call; the lgamma table is indexed by 0 <= count <= 65536 only, every other count -- INT32_MAX included -- takes the
 *   function (tests/test_gpu_call_domain.py, tests/test_gpu_scorer_domain.py).  Outside it nothing is read or written out of
 *   bounds, and no more is promised: a negative count is scored by whatever the literal arithmetic gives (no count indexes
 *   anything but that table), and strand sums beyond INT32_MAX wrap as int32 sums do.
 */
int ampli_poisson_call(ampli_ctx *ctx, const int32_t *d_trecs, int64_t P, int64_t E,
                       const uint32_t *d_ext_pos, int32_t T, const float *d_thr,
                       const uint8_t *d_ref_code, int32_t coverage_cutoff, int32_t mode,
                       uint8_t *d_call_mask, ampli_call *d_calls, int64_t capacity,
                       unsigned long long *d_n_calls, double *d_q, float *d_af);
/* the same with the thresholds read straight from the all-gathered blocks of a position-sliced merge (d_blocks as
 * ampli_error_table_unslice takes them): spares the unslice launch when only the calls are wanted */
int ampli_poisson_call_blocks(ampli_ctx *ctx, const int32_t *d_trecs, int64_t P, int64_t E, const uint32_t *d_ext_pos,
                              int32_t T, const void *d_blocks, int32_t n_slices, const uint8_t *d_ref_code,
                              int32_t coverage_cutoff, int32_t mode, uint8_t *d_call_mask, ampli_call *d_calls,
                              int64_t capacity, unsigned long long *d_n_calls, double *d_q, float *d_af);

/* poisson_call over an explicitly described cohort / chunk (ampli_records above); d_call_mask is [n_samples][P + E] */
int ampli_poisson_call_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr,
                               const uint8_t *d_ref_code, int32_t coverage_cutoff, int32_t mode, uint8_t *d_call_mask,
                               ampli_call *d_calls, int64_t capacity, unsigned long long *d_n_calls, double *d_q, float *d_af);

/*
 * loo_call -- the leave-one-out check of the panel of normals: for every normal s of the chunk `recs` and every
 * position p, the calling gate of VC (poisson_call's: VC:752-898, VC:3290) on s's records at p (primary and extra occurrences)
 * against the thresholds of the error table that the cohort WITHOUT s gives (EE with C and coverage_cutoff over the other S-1
 * normals), with calling_cutoff as VC's coverage_cutoff.  What a normal is called for is a false call of the noise model.
 *   d_acc           the WHOLE cohort's accumulator table, reduced with the SAME C and coverage_cutoff as given here
 *                   (ampli_error_reduce_records over every chunk; AMPLI_REDUCE_SUMMARY is enough: snt / srd / cnt / nrec are exact;
 *                   a table of other parameters gives wrong thresholds and is not detected); the S-1 sums are the totals minus s's own contribution, which is
 *                   exact inside the exactness envelope only: *d_flags is OR-ed with 1 when a total is outside it (then the
 *                   results are not the reference's; the caller must refuse)
 *   recs            one resident chunk of that cohort (any layout, dup_off required when E > 0; rd / rd_ext as for error_reduce);
 *                   call once per chunk.  Samples are chunk-local everywhere below.
 *   d_call_mask     [n][P + E] uint8, bit a = alt a called at that record (4-byte aligned; cleared by the call)
 *   d_calls / capacity / d_n_calls   the compact list as for ampli_poisson_call, entries ampli_loo_call
 *   d_callable_pos  int32 [P], optional, ADDED to: records of the chunk at p with ref in ACGT, FW >= and BW >= calling_cutoff
 *   d_callable_sample int32 [n], optional, ADDED to: the same per sample
 *   d_thr_loo       float [n][2][4][P], optional dense S-1 thresholds (the text round trip; 0.01 where the estimate is missing)
 *   mode            AMPLI_POISSON_PREFILTER, or AMPLI_POISSON_FULL: every live pair scored by the drain's exact bound (same outputs)
 * The queue is poisson_call's: AMPLI_FLAG_QUEUE_OVERFLOW as there; ampli_set_queue_items or AMPLI_POISSON_FULL (sized for every
 * live pair of the worst shard) recover.
 */
typedef struct ampli_loo_call {
    ampli_call call;      /* as poisson_call's list entry; call.sample = the held-out row of the chunk */
    float thr_fw, thr_bw; /* the S-1 table's threshold of the pair's (position, alt): what VC would read back from the table text */
    int32_t code;         /* that table cell's code: 0 estimate (the text is %f of the rate), 1 below quorum, 2 NaN (the text is 0.01) */
    int32_t pad;
} ampli_loo_call;         /* 80 bytes */
int ampli_loo_call_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc, float C,
                           int32_t coverage_cutoff, int32_t calling_cutoff, const uint8_t *d_ref_code, int32_t mode,
                           uint8_t *d_call_mask, ampli_loo_call *d_calls, int64_t capacity, unsigned long long *d_n_calls,
                           int32_t *d_callable_pos, int32_t *d_callable_sample, float *d_thr_loo, int32_t *d_flags);

/*
 * limit_records -- per-sample detection limits of the calling gate.  For every record of the chunk `trecs` (any layout,
 * ext_pos required when E > 0, rd / rd_ext as for poisson_call) and every base nt other than the position's reference base: the
 * smallest alternative counts (forward, reverse) with which the gate of VC:898 -- FW >= and BW >= coverage_cutoff,
 * Q(k_fw, RD - BW, thr_fw) >= 5 and Q(k_bw, BW, thr_bw) >= 5 -- would pass on that line's own depths, each strand's count bounded
 * by the strand's reads.  Asynchronous on the context's stream.
 *   d_thr        float [2][4][P] as for ampli_poisson_call;  d_ref_code uint8 [P]
 *   d_levels     float [n_levels], 0 <= n_levels <= AMPLI_LIMIT_MAX_LEVELS (may be NULL when n_levels == 0)
 *   d_min_reads  int32 [n][P + E][4][2] (fw, bw), 8-byte aligned; 0 unless the status is OK
 *   d_status     uint8 [n][P + E][4]: AMPLI_LIMIT_* below in bits 0-2; AMPLI_LIMIT_CALLED: the gate passes on the observed counts
 *                (ampli_poisson_call's mask bit); AMPLI_LIMIT_RECHECK: the device's arithmetic does not decide this cell (a score
 *                within AMPLI_CALL_GATE_EPS of the gate, a strand mean that is not a positive finite number): status, counts and the
 *                called bit of the cell are to be settled by the host (ampli_host_limit_reads); its other bits are 0
 *   d_counts     int64 [n][6 + n_levels], ADDED to: lines with a reference code > 3 | pairs OK | LOWDEPTH | NOESTIMATE |
 *                UNREACHABLE | RECHECK (counted nowhere else) | per level: OK pairs with MinAF = float(min_fw + min_bw) / float(RD)
 *                <= level
 */
#define AMPLI_LIMIT_OK 0          /* both strands have a smallest passing count */
#define AMPLI_LIMIT_REF 1         /* the position's reference base */
#define AMPLI_LIMIT_NOREF 2       /* the reference code is not A, C, G or T: the line gives no pairs (VC:3290) */
#define AMPLI_LIMIT_LOWDEPTH 3    /* FW < coverage_cutoff or BW < coverage_cutoff */
#define AMPLI_LIMIT_NOESTIMATE 4  /* a strand's threshold is -1 (Q = -888, VC:3844-3849) */
#define AMPLI_LIMIT_UNREACHABLE 5 /* not even every read of a strand would pass */
#define AMPLI_LIMIT_ABSENT 6      /* the sample has no such line */
#define AMPLI_LIMIT_CALLED 0x40
#define AMPLI_LIMIT_RECHECK 0x80
#define AMPLI_LIMIT_MAX_LEVELS 8
#define AMPLI_LIMIT_COUNTERS 6
int ampli_limit_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                        int32_t coverage_cutoff, const float *d_levels, int32_t n_levels, int32_t *d_min_reads, uint8_t *d_status,
                        int64_t *d_counts);
/* scorer evaluations of the context's limit_records launches so far: out[0] strands searched, out[1] evaluations (bracket checks
 * included), out[2] the most evaluations of one strand; reset != 0 clears them.  Synchronises the stream. */
int ampli_limit_stats(ampli_ctx *ctx, uint64_t out[3], int32_t reset);

/*
 * power_records -- detection power and limit of detection of the calling gate.  For every cell (sample, record, base) of
 * the chunk `trecs` whose status is AMPLI_LIMIT_OK (AMPLI_LIMIT_RECHECK clear; AMPLI_LIMIT_CALLED is ignored) with minimum reads
 * 1 <= min_fw <= FW and 1 <= min_bw <= BW (FW, BW: the sums of the record's four forward / reverse counts):
 *   power(v) = P[Bin(FW, v) >= min_fw] * P[Bin(BW, v) >= min_bw]   -- a variant at allele fraction v turns each read of a strand into an
 *              alternative read independently, the depths stay as they are, background alternative reads are ignored (a lower bound)
 *   LoD      = the v in (0, 1] with power(v) = confidence
 * Every other cell gets power 0 and LoD 0 and is counted nowhere.  Asynchronous on the context's stream.
 *   d_min_reads int32 [n][P + E][4][2], d_status uint8 [n][P + E][4]: as ampli_limit_records writes them, RECHECK cells settled by the host
 *   d_levels    float [n_levels] allele fractions, 0 <= n_levels <= AMPLI_POWER_MAX_LEVELS (may be NULL when n_levels == 0)
 *   confidence  in [0.5, 0.99] (the stopping rule of the root search is sized for this range)
 *   d_power     float [n][P + E][4][n_levels], may be NULL;  d_lod float [n][P + E][4], may be NULL (then no root is searched)
 *   d_counts    int64 [n][1 + n_levels], 8-byte aligned, ADDED to: OK pairs | per level: OK pairs with power(level) >= confidence, compared
 *               in double before the power is rounded to float
 * The values are fp64 sums formed with the device's exp / log: within 1e-6 of the definition (tests/power_model.py), the LoD within
 * 1e-4 relative; not bit-identical between libm versions or with ampli_host_power_pair.
 */
#define AMPLI_POWER_MAX_LEVELS 8
int ampli_power_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const int32_t *d_min_reads, const uint8_t *d_status,
                        const float *d_levels, int32_t n_levels, float confidence, float *d_power, float *d_lod, int64_t *d_counts);
/* work of the context's power_records launches so far: out[0] tails evaluated, out[1] pmf terms summed, out[2] the most terms of one
 * tail; reset != 0 clears them.  Synchronises the stream. */
int ampli_power_stats(ampli_ctx *ctx, uint64_t out[3], int32_t reset);

/*
 * dispersion_records / dispersion_finalize -- per-position dispersion of the panel of normals and per-normal outlier scores.
 * A cell is (strand, base, position); its qualifying records are the ones the threshold sums count (cnt of the accumulator table: every
 * present record of every normal at the position, primary and extra occurrences, with FW >= and BW >= coverage_cutoff and both strand
 * fractions of the base <= 0.05).  With k_i the record's count of the base on the strand, d_i the strand's depth, n the number of
 * qualifying records, K = sum k_i, D = sum d_i and r = K / D:
 *   X2  = sum (k_i - r d_i)^2 / (r d_i)          Pearson's statistic against the pooled rate
 *   phi = X2 / (n - 1),  z = (X2 - (n - 1)) / sqrt(V),  V = 2 (n - 1) + (D sum 1/d_i - n^2 - 2 n + 2) / K   (Haldane's exact variance)
 * A cell with n < 2 or K < 2 is FEW: X2 = sum 1/d = z = phi = 0, and it contributes to no per-sample sum.
 *   d_acc0      the WHOLE cohort's table reduced with C = 0 and the same coverage_cutoff (ampli_error_reduce_records over every chunk,
 *               AMPLI_REDUCE_SUMMARY is enough): snt = K exactly, srd = D, cnt = n.  A table of other parameters is not detected.
 *   recs        one resident chunk of that cohort (any layout, dup_off required when E > 0, rd / rd_ext as for error_reduce); call once
 *               per chunk, accumulate != 0 from the second chunk on
 *   d_x2, d_rinv  double [2][4][P]: X2 and sum 1/d_i, overwritten (accumulate == 0) or ADDED to
 *   d_sample_x2, d_sample_expect double [n], d_sample_terms int64 [n]: OVERWRITTEN, chunk-local rows, all three NULL or none -- over the
 *               OK cells and the sample's qualifying records in them: sum (k - r d)^2 / (r d), sum (1 - d / D) (the null mean of the
 *               same terms) and the number of terms.  x2 / expect is about 1 for an ordinary normal.
 * ampli_dispersion_finalize, once every chunk has been added: d_z double, d_phi float, d_status uint8, each [2][4][P], overwritten --
 * status AMPLI_DISPERSION_OK or _FEW in bits 0-2, AMPLI_DISPERSION_HIGH where the cell is OK and z >= z_cutoff; d_counts int64 [4] ADDED
 * to: cells OK | cells FEW | cells HIGH | positions with a HIGH cell.
 * No floating-point atomics: the same inputs in the same chunks give the same bytes.  Asynchronous on the context's stream.
 */
int ampli_dispersion_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc0, int32_t coverage_cutoff,
                             double *d_x2, double *d_rinv, int32_t accumulate, double *d_sample_x2, double *d_sample_expect,
                             int64_t *d_sample_terms);
int ampli_dispersion_finalize(ampli_ctx *ctx, int64_t P, const ampli_acc_table *d_acc0, const double *d_x2, const double *d_rinv,
                              double z_cutoff, double *d_z, float *d_phi, uint8_t *d_status, int64_t *d_counts);

/*
 * genotype_planes_records / concordance_pairs -- sample identity: are two count files the same person.
 * The genotype of (sample, position) comes from the counts of the position's PRIMARY record alone (slot r < P): extra occurrences (ext,
 * E, dup_off, ext_pos) and the own-RD planes (rd, rd_ext) of `recs` are ignored, no reference base and no error table is read.  With
 * n_b = fw[b] + bw[b] and d = sum n_b (all products in int64), base b is ABSENT when 1000 n_b <= absent_max_pm d, HET when
 * het_min_pm d <= 1000 n_b <= het_max_pm d, HOM when 1000 n_b >= hom_min_pm d, else AMBIGUOUS; the position is VALID when the record is
 * present, d >= min_depth, no base is AMBIGUOUS and either one base is HOM and none HET or two are HET and none HOM.
 *   prm       min_depth >= 1 and 0 <= absent_max_pm < het_min_pm <= het_max_pm < hom_min_pm <= 1000 (library defaults 100 / 100 / 250 /
 *             750 / 900), else AMPLI_E_INVALID
 *   d_planes  uint64 [recs->n_samples][6][W], W = ampli_concordance_words(P) = ceil(P / 64), 8-byte aligned, OVERWRITTEN, all of it:
 *             plane 0 V (valid), 1-4 A, C, G, T (the base is HET or HOM), 5 H (the position is a het); every plane is 0 where V is 0;
 *             bit i of word w is position 64 w + i; bits at and beyond P are 0.  A streamed cohort encodes each chunk into its rows of
 *             one buffer: pass d_planes + first_sample * 6 * W.
 * ampli_concordance_pairs: for every pair (a, b) of two plane sets (or of one: d_planes_a == d_planes_b with n_a == n_b computes the
 * upper triangle and mirrors it) five int32 counts, summed over the words, with both = Va & Vb, diff = OR over the bases of Xa ^ Xb,
 * share = OR of Xa & Xb:
 *   d_counts  int32 [n_a][n_b][5], OVERWRITTEN: sites popcount(both) | match popcount(both & ~diff) | ibs0 popcount(both & ~share)
 *             (opposite homozygotes) | het_either popcount(both & (Ha | Hb)) | het_match popcount(both & ~diff & Ha)
 * On the diagonal of a set against itself sites is the sample's valid positions and het_either its het positions.  P < 2^31.
 * Integers only: the same inputs give the same bytes.  Both are asynchronous on the context's stream.  The relation of a pair is
 * decided on the host (ampli_host_concordance_relation, include/amplisolve_host.h).
 */
int64_t ampli_concordance_words(int64_t P);
int ampli_genotype_planes_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_genotype_params *prm, uint64_t *d_planes);
int ampli_concordance_pairs(ampli_ctx *ctx, int64_t P, const uint64_t *d_planes_a, int32_t n_a, const uint64_t *d_planes_b, int32_t n_b,
                            int32_t *d_counts);

/*
 * contamination_records -- cross-sample contamination: which file leaks into which, and how much.  The counts of every
 * recipient a of a resident chunk are weighed against the genotypes of every source b, for every ordered pair.  Of `recs` only the
 * primary record of each (sample, position) enters, as in ampli_genotype_planes_records; with n[Y] = fw[Y] + bw[Y] and d = sum n[Y]
 * in int64, an absent record counting as all zeros whatever the planes say.  With the plane bits of a and b at a position:
 *   homA = Va & ~Ha (a is validly homozygous for its one base X), o[Y] = homA & Vb & B_Y & ~A_Y (b carries a base that a does not),
 *   bg = homA & Vb & ~(o[A] | o[C] | o[G] | o[T]) (b has a's genotype)
 * nine int64 sums over the positions, in the order AMPLI_CONTAM_*:
 *   sites_hom  1 if any o[Y] & ~Hb      alt_hom  n[Y] of those Y                  depth_hom  d, once
 *   sites_het  1 if any o[Y] & Hb       alt_het  n[Y] of every such Y (1 or 2)    depth_het  d once per such Y
 *   sites_bg   1 if bg                  alt_bg   sum of n[Y] over the Y with ~A_Y depth_bg   d
 *   d_planes_a  uint64 [recs->n_samples][6][W]: the planes of THE CHUNK'S rows (ampli_genotype_planes_records), W = ceil(P / 64)
 *   d_planes_b  uint64 [n_b][6][W]: the planes of the sources; may be (or overlap) d_planes_a
 *   d_sums      int64 [recs->n_samples][n_b][9], 8-byte aligned, FULLY OVERWRITTEN (C12).  A streamed recipient set writes each chunk
 *               into its rows of one matrix: pass d_sums + first_sample * n_b * 9.
 * All sums are exact: with the 16- and 24-bit layouts d < 2^27 and every sum stays below 2^59 for any P < 2^31; with the int32 layout
 * d < 2^34, counted at most twice per position, and P >= 2^28 is refused with AMPLI_E_RANGE (no data-dependent check is made).
 * P >= 2^31 and n_b > 4194240 are AMPLI_E_RANGE too.  Integers only, and integer additions only where position slices meet: the
 * same inputs give the same bytes.  Asynchronous on the context's stream.  The estimate and the status of a pair are decided on the
 * host (ampli_host_contamination_estimate, include/amplisolve_host.h).
 */
int ampli_contamination_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes_a, const uint64_t *d_planes_b,
                                int32_t n_b, int64_t *d_sums);

/*
 * Amplicon coverage and copy ratio against the panel of normals (the definition, in plain numpy, is tests/amplicon_model.py).
 *
 * The amplicons are position lists, a CSR over the BED walk, IN DEVICE MEMORY: d_amp_off uint32 [A + 1], d_amp_pos uint32 [W] with
 * entries in [0, P).  Lists may overlap, be in any order, name a position several times, and be empty.  That d_amp_off is monotone
 * with d_amp_off[A] <= W and that the entries are below P is the caller's contract: the contents are NOT validated on the host
 * (Context.amplicon_depth and AmpliSolveAmpliconCoverage build them).  The kernel still addresses nothing outside: list bounds are cut
 * to [0, W] and an entry at or beyond P is skipped.
 *
 * amplicon_depth_records -- stage 1: for every sample s of the resident chunk and every amplicon a, four int64 sums over the entries p
 * of a's list, from the PRIMARY record of (s, p) only (slot p < P; extras and an RD plane have no effect), in the order AMPLI_AMP_*:
 *   PRESENT   += 1 where the record is present            DEPTH_FW += FW = fw[A] + fw[C] + fw[G] + fw[T]
 *   CALLABLE  += 1 where FW >= cutoff and BW >= cutoff     DEPTH_BW += BW, likewise
 * An absent record adds nothing.  A depth is below 2^27 with the 16- and 24-bit layouts and below 2^34 with int32 records, so with
 * W < 2^28 no sum can leave int64: W >= 2^28 is AMPLI_E_RANGE, and there is no data-dependent check.  P >= 2^31 and
 * n_samples > 2097120 are AMPLI_E_RANGE too.  AMPLI_E_INVALID: a null or misaligned pointer, P <= 0, A <= 0, W < 0, a negative
 * cut-off, broken records.  On every refusal the output is untouched.
 *   d_sums  int64 [recs->n_samples][A][4], 8-byte aligned, FULLY OVERWRITTEN with plain stores (C13).  A streamed cohort writes each
 *           chunk into its rows of one matrix: pass d_sums + first_sample * A * 4.
 * One form for every list length: a wave owns one amplicon and AMPLI_AMPLICON_STRIP consecutive rows; lists of up to 256 entries keep
 * their indices in registers, longer ones are walked in rounds of 64 by the same wave (nothing is cut across waves, no atomics).
 * Integers only: the same inputs give the same bytes.  Asynchronous on the context's stream.
 *
 * amplicon_reference -- stage 2a, from the sums of the N normals: d[n][a] = DEPTH_FW + DEPTH_BW; T[n] = sum of d[n][a] over use[a] != 0
 * (int64); normal n is included iff T[n] > 0 (N_eff of them); x[n][a] = (double)d / (double)T[n]; med[a] = the median of x over the
 * included normals, mad[a] = the median of |x - med[a]|; status[a] = AMPLI_AMPLICON_FEW if N_eff < min_normals, else _DARK if
 * med[a] == 0, else _OK.  The median of m values in ascending order v is v[(m-1)/2] (m odd), (v[m/2-1] + v[m/2]) * 0.5 (m even),
 * NaN (m == 0); it is found by selection on the bit patterns.
 *   d_total int64 [N], d_ref double [A][2] (med, mad), d_status uint8 [A]: FULLY OVERWRITTEN (C14).
 * AMPLI_E_INVALID: null or misaligned pointers, N <= 0, A <= 0, min_normals < 1.  AMPLI_E_RANGE: N > AMPLI_AMPLICON_MAX (what the
 * workgroup's LDS buffer holds).
 *
 * amplicon_ratio -- stage 2b, for any S samples (tumours, or the normals themselves) from their sums and a reference: T[s] as above;
 * r[s][a] = (d / T[s]) / med[a] where status[a] is OK and T[s] > 0, else NaN; K[s] = the number of amplicons with use[a] and OK
 * (0 where T[s] <= 0), centre[s] = the median of r[s][a] over them (NaN where K[s] == 0); ratio[s][a] = r[s][a] / centre[s];
 * z[s][a] = mad[a] > 0 ? ((ratio - 1.0) * med[a]) / (1.4826 * mad[a]) : NaN.  Every operation is an IEEE double operation in the
 * written order (the library is built with -ffp-contract=off): the results equal the numpy model's bit for bit.
 *   d_total int64 [S], d_centre double [S], d_k int32 [S], d_ratio, d_z double [S][A]: FULLY OVERWRITTEN (C15).
 * AMPLI_E_INVALID as above; AMPLI_E_RANGE: A > AMPLI_AMPLICON_MAX.  Both are asynchronous on the context's stream.
 */
int ampli_amplicon_depth_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t A, const uint32_t *d_amp_off,
                                 const uint32_t *d_amp_pos, int64_t W, int32_t coverage_cutoff, int64_t *d_sums);
int ampli_amplicon_reference(ampli_ctx *ctx, const int64_t *d_sums, int32_t N, int32_t A, const uint8_t *d_use, int32_t min_normals,
                             int64_t *d_total, double *d_ref, uint8_t *d_status);
int ampli_amplicon_ratio(ampli_ctx *ctx, const int64_t *d_sums, int32_t S, int32_t A, const uint8_t *d_use, const double *d_ref,
                         const uint8_t *d_status, int64_t *d_total, double *d_centre, int32_t *d_k, double *d_ratio, double *d_z);

/*
 * Substitution spectrum and strand asymmetry (the definition, in plain numpy, is tests/spectrum_model.py).
 *
 * spectrum_records -- for every sample s of the resident chunk and every class c < C, nine int64 sums over the positions p with
 * d_class[p] == c whose PRIMARY record (s, p) ENTERS (slot p < P; extras and an RD plane have no effect), in the order AMPLI_SPEC_*:
 *   SITES += 1        FW_A .. FW_T += fw[b]        BW_A .. BW_T += bw[b]        (the reference base's own counts included)
 * With FW = sum fw[b], BW = sum bw[b], n_b = fw[b] + bw[b] and d = FW + BW, all in int64, the record enters iff it is present,
 * d_ref_code[p] is 0..3 (A C G T) and d_class[p] < C, FW >= coverage_cutoff and BW >= coverage_cutoff, and 1000 n_b <= max_alt_pm d
 * for every base b other than the reference: the position is background for this file, not a germline or a clear somatic variant.
 * The gate is all or nothing per position; d == 0 passes its last clause and is stopped only by a positive cut-off.  This is
 * csrc/ampli_math.h's ampli_spectrum_enters, which the host library exports (ampli_host_spectrum_enters_batch).
 *   d_ref_code uint8 [P]; d_class uint8 [P]: a class in [0, C), or AMPLI_SPECTRUM_SKIP (255) -- any value at or above C skips the
 *           position: no bin at or beyond C is ever addressed; C in [1, AMPLI_SPECTRUM_MAX_CLASSES]
 *   d_sums  int64 [recs->n_samples][C][9], 8-byte aligned, FULLY OVERWRITTEN (C16).  A streamed cohort writes each chunk into its rows
 *           of one matrix: pass d_sums + first_sample * C * 9.
 * A field is below 2^24 with the 16- and 24-bit layouts and below 2^31 with int32 records, and P >= 2^31 is AMPLI_E_RANGE, so no sum
 * can leave int64 and there is no data-dependent check.  AMPLI_E_RANGE too: C > AMPLI_SPECTRUM_MAX_CLASSES.  AMPLI_E_INVALID: a null
 * pointer, a misaligned d_sums, P <= 0, C <= 0, a negative cut-off, max_alt_pm outside [0, 1000], broken records.  On every refusal
 * the output is untouched.
 * The form: a workgroup of four waves owns AMPLI_SPECTRUM_STRIP consecutive rows and one segment of the positions; its waves take
 * the segment's 64-position tiles in turn, and an entering lane adds its values into the workgroup's LDS bins [row][class][9] with
 * 64-bit LDS atomics.  With one segment the bins are stored; with several they are added with 64-bit integer atomics onto the
 * matrix the call cleared.  The segments: a launch without them is strips = ceil(n_samples / AMPLI_SPECTRUM_STRIP) workgroups;
 * while that is fewer than 8 per compute unit, the T = ceil(P / 64) tiles are cut into
 *   segments = ceil(T / tps), tps = max(16, ceil(T / want)), want = min(64, ceil(8 n_cu / strips))
 * -- so every panel of up to 1024 positions is one segment.  ampli_last_spectrum_segments: the number of the context's last launch
 * (as ampli_last_reduce_kernel; AMPLI_E_INVALID before the first).  Integers only: the same inputs give the same bytes, whatever
 * the order the segments arrive in.  Asynchronous on the context's stream.
 */
int ampli_spectrum_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint8_t *d_ref_code, const uint8_t *d_class, int32_t C,
                           int32_t coverage_cutoff, int32_t max_alt_pm, int64_t *d_sums);
int ampli_last_spectrum_segments(const ampli_ctx *ctx);

/*
 * Panel-of-normals exceedance (the definition, in plain numpy, is tests/exceedance_model.py): how many of the normals show
 * an allele at a position at the tumour's fraction or above.
 *
 * Inputs.  recs_t, a chunk of n_t "tumour" rows, and recs_n, a chunk of n_n "normal" rows: both ampli_records in any of the three
 * layouts, and the two may differ.  P, and d_ref_code uint8 [P].  normal_cutoff >= 0 and calling_cutoff >= 0.  first_t and first_n
 * (>= 0), the global indices of each chunk's first row.  skip_same_index (0 / not 0) and accumulate (0 / not 0).  Only the PRIMARY
 * record of (row, position) enters, slot r < P; extras and an RD plane have no effect.
 * Per record.  For strand st (0 forward, 1 reverse) x[st][b] is the count of base b and D[st] the sum of the strand's four counts,
 * all unsigned 64-bit; an absent record has no counts.
 * Eligible normal.  Normal s is eligible at p iff its record is present, D_s[0] >= normal_cutoff and D_s[1] >= normal_cutoff (the
 * two-strand depth clause of EE:1592), and not (skip_same_index and first_n + s == first_t + t).  There is no allele-fraction
 * clause: a germline-heterozygous normal is supposed to count.
 * Reaching.  Normal s reaches tumour t at (p, b, st) iff it is eligible and x_s[st][b] D_t[st] >= x_t[st][b] D_s[st]: x_s / D_s >=
 * x_t / D_t by cross-multiplication.  Both products are formed in unsigned 64 bits: a field is below 2^31 and a depth below 2^33,
 * so no product reaches 2^64.  x_t == 0 makes every eligible normal reach (an absent tumour record too, whose cells are NA anyway).
 * Outputs.
 *   d_elig uint16 [n_t][P]: the eligible normals for (t, p), whatever t's own record is.
 *   d_ge   uint16 [n_t][P][4][2], 16-byte aligned: per base b and strand, the number of normals that reach.  A cell is EVALUATED iff
 *          t's record is present, D_t[0] >= calling_cutoff and D_t[1] >= calling_cutoff, d_ref_code[p] is 0..3 and b is not
 *          d_ref_code[p]; every other cell holds AMPLI_EXCEEDANCE_NA (0xFFFF) on both strands.
 * accumulate == 0 overwrites every cell of both outputs.  accumulate != 0 adds this chunk's normals onto d_elig and onto the cells
 * this call's arguments make evaluated (modulo 2^16: what they held is taken as a count) and writes NA to the others: called with
 * the same tumours, reference codes and calling_cutoff, NA cells stay NA, and any chunking of the normals gives the bytes of the
 * single pass (C17).
 * Refusals, every output untouched.  AMPLI_E_RANGE: first_n + n_n > AMPLI_EXCEEDANCE_MAX_NORMALS (65534), so that no count can
 * reach the sentinel; P >= 2^31.  AMPLI_E_INVALID: a null pointer, a misaligned d_elig or d_ge, P <= 0, a negative cut-off or first
 * index, broken records (n_t or n_n < 1, an unknown layout, a row stride below P + E, misaligned records).
 * The form: a workgroup of four waves owns one 64-position tile and AMPLI_EXCEEDANCE_ROWS tumour rows, two per wave, a lane a
 * position; the normals pass through LDS in strips of AMPLI_EXCEEDANCE_STRIP decoded rows, the next strip's loads in flight while
 * this one is compared.  The normals are never split across workgroups: every (t, p) cell has exactly one owning lane per launch,
 * the accumulate form is a plain read-modify-write, there are no atomics and the bytes are the same in any launch order.
 * Integers only.  Asynchronous on the context's stream.
 */
int ampli_exceedance_records(ampli_ctx *ctx, const ampli_records *recs_t, const ampli_records *recs_n, int64_t P, const uint8_t *d_ref_code,
                             int32_t normal_cutoff, int32_t calling_cutoff, int64_t first_t, int64_t first_n, int32_t skip_same_index,
                             int32_t accumulate, uint16_t *d_elig, uint16_t *d_ge);

/*
 * Overdispersion-aware calling (the definition is tests/overdispersion_model.py): the dispersion omega of every cell of the
 * panel of normals, and the score of a tumour's cell under the negative binomial with the error table's own mean.
 *
 * The fit.  A cell is (strand, base, position).  Its qualifying records are dispersion's (above): the ones cnt of the accumulator table
 * counts, primary and extra occurrences, an RD plane honoured.  With n, K = sum k_i, D = sum d_i of the C = 0 table, X2 and the status
 * of ampli_dispersion_records / _finalize and S2 = sum d_i^2 over the same records:
 *   omega = (X2 - (n - 1)) D / (K (D - S2 / D))   where the status carries AMPLI_DISPERSION_HIGH and D - S2 / D > 0,
 *   omega = 0                                      everywhere else, and where the quotient is not above 0 (a negative z_cutoff).
 * A pre-test moment estimator: E[X2] = (n - 1) + omega r (D - S2 / D) under k_i ~ Poisson(lambda_i d_i), E lambda_i = r = K / D,
 * Var lambda_i = omega r^2.  A cell the panel cannot show to be overdispersed keeps the reference's Poisson model.
 *   ampli_overdispersion_records   one resident chunk (any layout, dup_off required when E > 0, rd / rd_ext as for error_reduce) into
 *               d_s2 double [2][4][P], overwritten (accumulate == 0) or ADDED to.  Squares and sums are integers (two 64-bit words per
 *               cell), converted once: exact whenever S2 < 2^53 -- every uint16 cohort -- and then the same for any chunking.  No
 *               atomics: the same inputs in the same chunks give the same bytes.  d_acc0 (the C = 0 table of P positions, as for
 *               ampli_dispersion_records) is checked and not read: S2 is formed for every cell, OK or not.
 *   ampli_overdispersion_finalize  d_x2 and d_status as ampli_dispersion_* left them, d_s2 complete: d_omega double [2][4][P], overwritten.
 *               A HIGH status comes from an OK cell (n >= 2, K >= 2) and that is assumed: planes that do not belong together (HIGH with
 *               K = 0) give an infinite or NaN omega, which ampli_nb_score_records answers with AMPLI_NB_NA.
 *
 * The score.  Only the PRIMARY record of (row, position) enters, slot r < P; extras and an RD plane have no effect.  For strand st
 * and base b: k = x[st][b], d = D_t[st] (the sum of the strand's four counts), e = d_thr[st][b][p], omega = d_omega[st][b][p] (d_omega ==
 * NULL: 0 everywhere).
 *   Q = AMPLI_NB_NA          for a negative, NaN or infinite omega; else
 *   Q = -888                 for e == -1 (VC:3844-3849); else
 *   Q = 0                    for k == 0; else, with e == 0 replaced by 0.0010008f (VC:3852-3856) and m = double(d) * double(e),
 *   p = P[X >= k], X negative binomial of mean m and variance m + omega m^2 (pmf(0) = (1 + m omega)^(-1 / omega), pmf(j + 1) / pmf(j)
 *       = (1 + j omega) / (j + 1) * m / (1 + m omega)); at omega = 0, and below 1e-290, the exact Poisson tail;
 *   Q = 0 for p >= 1, else (float)(-10 log10(max(p, 1e-10))).
 * p is the mathematical tail, NOT the reference's kf_gammaq with its 100-term cut-offs: at omega = 0 the score differs from
 * ampli_poisson_call's wherever those cut-offs bite.  |Q - exact| <= 1e-5 for m in [1e-3, 1e4], omega = 0 or in [1e-8, 1e4] and
 * k <= 10 m + 2; between 0 and 1e-8 the arithmetic is the same and so was the error where it was tested.  A sum has at most 2^20
 * terms: a tail that needs more (k beyond 2^20 with m omega beyond 26 000, csrc/ampli_math.h) gives AMPLI_NB_NA.
 *   d_q float [n_t][P][4][2], 16-byte aligned, fully overwritten.  A cell is EVALUATED iff t's record is present, D_t[0] >=
 *   calling_cutoff and D_t[1] >= calling_cutoff, d_ref_code[p] is 0..3 and b is not d_ref_code[p]; every other cell holds AMPLI_NB_NA
 *   (-1.0f) on both strands.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer (d_omega of ampli_nb_score_records may be NULL),
 * P <= 0, coverage_cutoff < 1, calling_cutoff < 0, a table that is not bound to P positions, broken records (n < 1, an unknown layout,
 * a row stride below P + E, misaligned records, E > 0 without dup_off for the fit).  AMPLI_E_RANGE: P >= 2^31.
 * The form: the S2 kernel has dispersion_stream_kernel's shape (a 64-position tile, four waves over the rows, LDS hand-over in wave
 * order); the score kernel gives a wave one tumour row of a tile, a lane a position, and walks the lane's six cells in one loop.
 * Asynchronous on the context's stream.
 */
int ampli_overdispersion_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc0, int32_t coverage_cutoff,
                                 double *d_s2, int32_t accumulate);
int ampli_overdispersion_finalize(ampli_ctx *ctx, int64_t P, const ampli_acc_table *d_acc0, const double *d_x2, const double *d_s2,
                                  const uint8_t *d_status, double *d_omega);
int ampli_nb_score_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr, const double *d_omega,
                           const uint8_t *d_ref_code, int32_t calling_cutoff, float *d_q);

/*
 * Paired comparison (the definition is tests/paired_model.py): two count files of one patient -- tumour and matched normal,
 * baseline and follow-up, two libraries of one sample -- tested against each other at every (pair, position, alternative base), per
 * read strand, with the exact conditional test of the 2 x 2 table (alternative reads, other reads) x (file a, file b).
 *
 * A pair is (row a of recs_a, row b of recs_b).  Only the PRIMARY record of (row, position) enters, slot r < P; extras and an RD plane
 * have no effect.  For strand st and base y: k_a = x_a[st][y], d_a = the sum of a's four counts on st, k_b and d_b likewise;
 * N = d_a + d_b, K = k_a + k_b, n = d_a, and X is hypergeometric: the number of alternative reads among a's n when K alternative reads
 * are dealt among N.  The side is decided in integers by c = k_a N - K n (= k_a d_b - k_b d_a: two products below 2^64):
 *   S = +0                      for K == 0 or c == 0; else
 *   S = +Q(P[X >= k_a])         for c > 0 (a's fraction is the higher),
 *   S = -Q(P[X <= k_a])         for c < 0,      Q(p) = (float)(-10 log10(max(p, 1e-10))), +0 for p >= 1; -0 is never stored.
 * Only the tail on the observation's own side of the mean is summed -- the short sum, never a complement.  |S - exact| <= 1e-5 for
 * every strand depth up to 2^31 - 1 (tests/test_paired_host.py); the sign, +0, +-100 beyond the clamp and NA are exact.  A sum has at
 * most 2^20 terms: a tail that needs more gives AMPLI_PAIR_NA (no int32 record does, csrc/ampli_math.h).
 *   d_s float [n_pairs][P][4][2], 16-byte aligned, fully overwritten.  A cell is EVALUATED iff both records are present, all four
 *   strand depths (a and b, forward and backward) are >= depth_cutoff, d_ref_code[p] is 0..3 and y is not d_ref_code[p]; every other
 *   cell holds AMPLI_PAIR_NA (-999.0f) on both strands.
 *   d_pairs int32 [n_pairs][2]: row in a, row in b.  recs_a and recs_b may be the same chunk, a row may occur in many pairs, and a pair
 *   of a row with itself is legal: +0 in every evaluated cell.  Row indices cannot be checked on the host without a copy: an index
 *   outside its chunk makes that pair all NA, and the kernel checks this before any load.
 * Conditional on K; the strands are tested independently; nothing is corrected for the number of cells.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer, P <= 0, n_pairs < 1, depth_cutoff < 0, broken
 * records (n < 1, an unknown layout, a row stride below P + E, misaligned records), chunks of different layouts.  AMPLI_E_RANGE:
 * P >= 2^31.
 * The form: a wave owns one pair of a 64-position tile, a lane a position, and walks the lane's six cells in one loop.  Asynchronous on
 * the context's stream.
 */
int ampli_pair_score_records(ampli_ctx *ctx, const ampli_records *recs_a, const ampli_records *recs_b, int64_t P,
                             const int32_t *d_pairs /* [n_pairs][2]: row in a, row in b */, int32_t n_pairs,
                             const uint8_t *d_ref_code, int32_t depth_cutoff, float *d_s /* [n_pairs][P][4][2] */);

/*
 * False-discovery control (the definition is tests/fdr_model.py): the Benjamini-Hochberg adjusted score of every cell of a
 * score plane d_s float [rows][P][4][2] (row, position, base, strand) -- the plane ampli_nb_score_records and ampli_pair_score_records
 * write.  A row is one file or one pair, and each row is adjusted on its own.
 *
 * Cell key, with s_f and s_b the two strand scores of cell (r, p, y):
 *   two_sided == 0 (the negative-binomial plane; AMPLI_NB_NA and -888 are negative): the cell is TESTED iff 0 <= s_f <= 100 and
 *     0 <= s_b <= 100; magnitude a = min(s_f, s_b), sign +.
 *   two_sided == 1 (the paired plane): TESTED iff -100 <= s_f <= 100 and -100 <= s_b <= 100; both > 0: a = min, sign +; both < 0:
 *     a = min(|s_f|, |s_b|), sign -; otherwise a = 0.
 *   Everything else is UNTESTED: a NaN, an infinity, any sentinel, anything beyond +-100.  A zero of either sign is a = 0 (-0.0f is not
 *   the largest key).  Inputs of magnitude below 2^-126 (denormals) are outside the contract: no scorer writes one.
 * p_cell = max(p_fw, p_bw) -- both strands must show the allele, as every gate here asks -- is a valid, conservative p-value; the
 * two-sided form doubles it, because the side was chosen by the data.
 *
 * Adjustment, in double.  m_r = the tested cells of row r, those with a = 0 included.  For a tested cell with a > 0:
 *   R = #{tested j of the row : a_j >= a}        (the largest rank among ties: equal keys get equal values)
 *   B = a - 10 log10(m_r / R) - (two_sided ? 10 log10 2 : 0)
 *   A = max(0, max{B_j : 0 < a_j <= a})           (BH's step-up minimum over the larger p, in score space: q = 10^(-A / 10))
 *   d_a float [rows][P][4], 16-byte aligned: sign * (float)A for a tested cell with a > 0; +0 where a = 0 or A = 0 (-0 is never
 *     stored); AMPLI_FDR_NA (-999.0f) where untested.
 *   d_m int32 [rows]: m_r.  A row with m_r = 0 is all NA.
 *   d_rank int32 [rows][P][4], 16-byte aligned, or NULL: R, and 0 where untested or a = 0.
 *   d_work: ampli_fdr_workspace_bytes(rows, P) bytes, 16-byte aligned (two key arrays of 4 P words, the digit histograms and the scans'
 *     block totals, per row); 0 from the query means rows < 1, P <= 0 or 4 P >= 2^31.
 * |A - model| <= 1e-5 (one float ulp at 100 is 7.6e-6; the double arithmetic under it adds less than 1e-12); m, R, the tested mask, the
 * sign, +0 and NA are exact.  The same plane gives the same bytes, alone or as one row of a batch.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer (d_rank may be NULL), rows < 1, P <= 0, two_sided
 * not 0 or 1, a workspace smaller than the query's.  AMPLI_E_RANGE: 4 P >= 2^31.
 * The form (csrc/ampli_fdr.hip): the keys' bit patterns and m; an LSD radix sort of each row's 4 P keys, 8 bits a pass, over tiles of
 * AMPLI_FDR_TILE_KEYS keys with a stable scatter; B at the first slot of each tie group and its running maximum by a two-level scan
 * (blocks of AMPLI_FDR_SCAN_BLOCK, whose totals one workgroup per row walks AMPLI_FDR_SCAN_BLOCK at a time); a binary search per cell.
 * No workgroup waits for another.  Asynchronous on the context's stream: m_r is read from device memory, nothing synchronises.
 */
#define AMPLI_FDR_TILE_KEYS 4096 /* keys of one sort tile: 1024 positions */
#define AMPLI_FDR_SCAN_BLOCK 512 /* elements of one scan block; one second-level step covers 512 * 512 keys = 65536 positions */
size_t ampli_fdr_workspace_bytes(int32_t rows, int64_t P);
int ampli_fdr_adjust(ampli_ctx *ctx, const float *d_s /* [rows][P][4][2] */, int32_t rows, int64_t P, int32_t two_sided, void *d_work,
                     size_t work_bytes, float *d_a /* [rows][P][4] */, int32_t *d_m /* [rows] */, int32_t *d_rank /* [rows][P][4] or NULL */);

/*
 * In-silico dilution (the definition is tests/dilution_model.py): read-level mixing of two count files.  32-bit integer
 * work only, so the device, the host library and the numpy model agree integer for integer.
 *   Generator.  Philox4x32-10 (Salmon et al., 2011).  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments W0 = 0x9E3779B9,
 *     W1 = 0xBB67AE85.  One round on counter (c0, c1, c2, c3) with key (k0, k1): (hi0, lo0) = M0 * c0 as a 64-bit product,
 *     (hi1, lo1) = M1 * c2; the new counter is (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0).  Ten rounds; the key is bumped by (W0, W1)
 *     after each round (the bump after the last round is dead).
 *   Thinning.  Thin(n, keep; key, p, f, side) = #{ i < n : word_i < keep }, compared as 64-bit unsigned, keep in [0, 2^32].  word_i is
 *     output word (i & 3) of Philox with counter (i >> 2, p, f | side << 3, 0) and key (low word, high word of the 64-bit key); p is the
 *     position index, f in 0..7 the record field, side 0 for file a and 1 for file b.  A read is word i of its field, kept with
 *     probability keep / 2^32, independently.  Exactly: keep = 2^32 keeps all, keep = 0 keeps none, Thin is non-decreasing in n and in
 *     keep -- so a series with one key is nested.
 *   Mixture.  {int32 row_a; int32 row_b; uint64 keep_a; uint64 keep_b; uint64 key}: out[f] = Thin(a[f], keep_a; key, p, f, 0) +
 *     Thin(b[f], keep_b; key, p, f, 1) over the PRIMARY records; row_b == -1 is pure down-sampling.  The output record is ABSENT
 *     (field 0 = AMPLI_ABSENT, the other seven 0) when a's record is absent, when b is named and its record is absent, or when a present
 *     input record holds a count outside [0, 2^24 - 2] (AMPLI_DILUTE_BAD_COUNT).  A mixture is all ABSENT with AMPLI_DILUTE_BAD_MIXTURE
 *     when a row is outside its chunk, a keep is above 2^32, row_b >= 0 without a chunk b, or row_b < -1.
 *   Fractions to thresholds.  keep = (uint64) floor(ldexp(x, 32) + 0.5), x a double in [0, 1]: IEEE operations, the same everywhere.
 *
 * ampli_dilute_records: d_mix, n_mix descriptors of 32 bytes in DEVICE memory, 8-byte aligned (like d_pairs of the paired comparison).
 * Only the PRIMARY record of (row, position) enters, slot r < P; extras and an RD plane have no effect.  recs_a and recs_b may be the
 * same chunk, different chunks, or chunks of different layouts; recs_b may be NULL when every mixture has row_b == -1.  A row may occur
 * in many mixtures.  [0, 2^24 - 2] is the range the fast kernels take: it bounds a list at 2^22 Philox blocks and keeps every output
 * below 2^25.  The mixture's faults are checked on the device before any record is loaded (they cannot be checked on the host without
 * a copy); both keeps are checked whether b is named or not.  A bad count in EITHER present input record raises the flag.
 *   d_out int32 [n_mix][P][8], 16-byte aligned: the AMPLI_RECORDS_I32 layout, dense, E = 0 -- every entry point takes it as an
 *     ampli_records as it stands (n_samples = n_mix), and so does ampli_records_pack16.
 *   d_flags int32 [n_mix]: AMPLI_DILUTE_BAD_COUNT | AMPLI_DILUTE_BAD_MIXTURE, 0 for a clean mixture.  The call clears it on the stream
 *     and the kernel ORs into it with at most one integer atomic per workgroup; OR is order-free.
 * No kernel reads another mixture's data: a mixture's bytes do not depend on the batch it is launched in, and the same inputs give the
 * same bytes.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer other than recs_b, P <= 0, n_mix < 1, broken
 * records (n < 1, an unknown layout, a row stride below P + E, misaligned records).  AMPLI_E_RANGE: P >= 2^31.
 * The form (csrc/ampli_dilution.hip): the grid is (position tiles, mixtures), at most 65 535 mixtures a launch; a wave owns one record
 * at a time, its 64 lanes deal out the record's Philox blocks, the per-field counts are added across the wave and one 32-byte record is
 * stored.  The 16 (side, field) lists of a record are walked one after the other (DESIGN 22 measures the alternative).  Asynchronous
 * on the context's stream.
 */
int ampli_dilute_records(ampli_ctx *ctx, const ampli_records *recs_a, const ampli_records *recs_b /* may be NULL */, int64_t P,
                         const ampli_dilute_mix *d_mix /* [n_mix] */, int32_t n_mix, int32_t *d_out /* [n_mix][P][8] */,
                         int32_t *d_flags /* [n_mix] */);

/*
 * Tumour-informed monitoring (the definition, in plain numpy, is tests/monitor_model.py): pooled evidence over the cells of
 * variant lists -- is a patient's tumour, known as a list of somatic variants, in this plasma sample at all?
 *   Lists.  A CSR IN DEVICE MEMORY: d_list_off uint32 [L + 1], d_list_cell uint32 [W], an entry c = 4 p + y (position index p below
 *     2^30, base y).  Lists may be empty, overlap and name a cell several times; a cell named twice counts twice.  An entry with
 *     p >= P is none.  Offsets are cut to [0, W]: the contents are not validated on the host and nothing outside is addressed.
 *   Evaluated entry of sample row s, from the PRIMARY record of (s, p) only (slot p < P; extras and an RD plane have no effect): the
 *     record is present; D_fw >= coverage_cutoff and D_bw >= coverage_cutoff, each the sum of the strand's four counts;
 *     d_ref_code[p] in 0..3 and y != it; e_fw = d_thr[0][y][p] and e_bw = d_thr[1][y][p] both finite and >= 0 (so not the -1 of
 *     VC:3844, "no estimate"); 1000 (k_fw + k_bw) <= max_vaf_pm (D_fw + D_bw) in int64, k the strand's count of base y (1000 switches
 *     this gate off; it keeps a germline or mislisted site from carrying a list on its own).  e == 0 is replaced by 0.0010008f
 *     (VC:3852-3856).
 *   Sums per (sample, list), in the order AMPLI_MON_*: N_EVAL, N_SEEN (evaluated entries with k_fw + k_bw >= 1), K_FW, K_BW, D_FW,
 *     D_BW, int64; and the doubles Lambda_fw, Lambda_bw, each the sum of (double)d_st * (double)e_st.  The order of the double additions
 *     is part of the definition: lane j of 64 takes the list's entries j, j + 64, ... in ascending order and adds each product to an
 *     accumulator that starts at +0.0 (an entry that is not evaluated adds nothing); the 64 accumulators are combined by the butterfly
 *     x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1.  Unfused IEEE operations: the model, the host library and the device agree bit
 *     for bit.  W >= 2^28 is AMPLI_E_RANGE, so no integer sum can leave int64 (a depth is below 2^34).
 *   Pooled score per strand: Q = (float)(-10 log10(max(p, 1e-10))), 0 for p >= 1, p = P[X >= K] for X Poisson of mean Lambda
 *     (ampli_nb_init at omega = 0 and its step loop, csrc/ampli_math.h).  K == 0 gives 0, Lambda == 0 with K > 0 gives 100,
 *     N_EVAL == 0 gives AMPLI_MON_NA for both strands; so does a tail beyond the term bound (csrc/ampli_math.h says when).
 *   Matched random controls, replicate r (global index) of list l: entry i (0-based within the list) at (p, y) with g = d_ref_code[p]
 *     becomes (p', y), p' = d_cand_pos[d_cand_off[g] + ((uint64(word) * m) >> 32)] with m = d_cand_off[g + 1] - d_cand_off[g] the
 *     candidates of g (d_cand_off uint32 [5], bounds cut to [0, n_cand]; d_cand_pos uint32 [n_cand], positions grouped by reference
 *     base) and word = output word 0 of Philox4x32-10 with counter (i, r, l, AMPLI_MON_CONTROL_TAG) and key (low word, high word of
 *     seed).  No control entry where p >= P, g > 3, m == 0 or p' >= P.  The multiply-high draw favours some candidates by less than
 *     m / 2^32.  A control list depends on (seed, l, r) only, never on the sample; its sums are formed exactly as above, from the
 *     thresholds and the reference base of p', max_vaf_pm included.
 *
 * ampli_monitor_sums_records: d_sums int64 [recs->n_samples][L][6] and d_lambda double [recs->n_samples][L][2], 8-byte aligned, FULLY
 *   OVERWRITTEN with plain stores (C22); a streamed cohort passes each chunk its rows of one matrix.  A wave owns one list and
 *   AMPLI_MON_STRIP consecutive rows; lists of up to 256 entries keep their cells and thresholds in registers (loaded once per wave),
 *   longer ones are walked in rounds of 64 by the same wave.
 * ampli_monitor_control_records: d_pairs int32 [n_pairs][2] (row of the chunk, list) in device memory; replicates first_rep ..
 *   first_rep + R - 1; d_sums int64 [n_pairs][R][6] and d_lambda double [n_pairs][R][2], FULLY OVERWRITTEN (C23).  A row or list index
 *   outside its range makes that pair's cells all zero (which scores as N_EVAL = 0); the index is checked before any list or record
 *   is loaded.  A wave owns one (pair, replicate): a replicate's cells do not depend on the batch it is computed in.
 * ampli_monitor_score: d_q float [n_cells][2] (fw, bw) from d_sums int64 [n_cells][6] and d_lambda double [n_cells][2], FULLY
 *   OVERWRITTEN (C24).  A lane per cell; the lane's two tails run in one loop.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer (prm is a host pointer), P <= 0, L < 1, W < 0,
 *   R < 1, n_pairs < 1, n_cells < 1, first_rep < 0, n_cand < 0, coverage_cutoff < 0, max_vaf_pm outside 0..1000, broken records.
 *   AMPLI_E_RANGE: P >= 2^31, W >= 2^28, n_samples > 2097120, n_cand >= 2^32, first_rep + R >= 2^31.
 * No LDS, no barrier, no atomics: the same inputs give the same bytes.  All three are asynchronous on the context's stream.  The
 * verdict, the excess fractions, the empirical p and the limit of detection are decided on the host (include/amplisolve_host.h).
 */
int ampli_monitor_sums_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                               const uint32_t *d_list_off, const uint32_t *d_list_cell, int32_t L, int64_t W, const ampli_monitor_params *prm,
                               int64_t *d_sums /* [n][L][6] */, double *d_lambda /* [n][L][2] */);
int ampli_monitor_control_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                  const uint32_t *d_list_off, const uint32_t *d_list_cell, int32_t L, int64_t W, const int32_t *d_pairs /* [n_pairs][2] */,
                                  int32_t n_pairs, const uint32_t *d_cand_off /* [5] */, const uint32_t *d_cand_pos /* [n_cand] */, int64_t n_cand,
                                  int32_t R, int32_t first_rep, uint64_t seed, const ampli_monitor_params *prm, int64_t *d_sums /* [n_pairs][R][6] */,
                                  double *d_lambda /* [n_pairs][R][2] */);
int ampli_monitor_score(ampli_ctx *ctx, const int64_t *d_sums, const double *d_lambda, int64_t n_cells, float *d_q /* [n_cells][2] */);

/*
 * Allelic imbalance at germline het sites, pooled per region (the definition, in plain numpy, is tests/allelic_model.py): the
 * companion of the copy ratio -- does a sample show the two alleles of its germline het sites in the share the panel of normals shows?
 *   Bases A, C, G, T = 0..3; pair code c = 0..5 for (lo, hi) = (A,C), (A,G), (A,T), (C,G), (C,T), (G,T).  A row of genotype planes
 *     (ampli_genotype_planes_records) is HET AT p WITH PAIR c when its V and H bits are set and exactly two of its A/C/G/T bits;
 *     anything else -- malformed planes included -- is not a het site.  Only the PRIMARY record of (row, p) enters (slot p < P; extras
 *     and an RD plane have no effect): k_lo = fw[lo] + bw[lo], k_hi likewise, m = k_lo + k_hi, in int64.
 *   Stage R.  d_ref int64 [3][6][P] (AMPLI_AI_REF_CNT, _LO, _HI): for every row of the chunk and every position where the row (row i of
 *     d_planes, the chunk's own planes [n][6][W']) is het with pair c, the record is present and m >= min_depth: CNT[c][p] += 1,
 *     LO[c][p] += k_lo, HI[c][p] += k_hi.  The call ADDS TO d_ref (C25): the caller clears it once, streamed chunks accumulate.
 *   Stage S.  Row s takes its germline from plane row g = d_row_g[s] of d_planes_g [n_g][6][W']; a g outside [0, n_g) means "none" and
 *     is never dereferenced.  Status of (s, p), the first rule that applies: AMPLI_AI_NOT_HET (g is none, or g is not het at p),
 *     _ABSENT (no record), _SHALLOW (m < min_depth), _DEEP (m > 2^31 - 1); then with c the pair of g at p: _TESTED_REF with
 *     v = (double)LO / (double)(LO + HI) if CNT[c][p] >= min_normals and LO > 0 and HI > 0; else _TESTED_HALF with v = 0.5 if
 *     half_fallback; else _NO_REFERENCE.  A tested cell: d = (double)k_lo - v (double)m, formed with two operations; d == 0: q = +0;
 *     d > 0: p = P[X >= k_lo], X ~ Bin(m, v); d < 0: p = P[X <= k_lo], taken as the upper tail of m - k_lo under 1.0 - v;
 *     q = (float)(-10 log10(max(min(1, 2 p), 1e-10))) signed by d, +0 where 2 p >= 1 - 1e-8, never -0, |q| <= 100; AMPLI_AI_NA where the tail
 *     is not computable within its term bound (csrc/ampli_math.h says when: no int32 record's).  Outputs, FULLY OVERWRITTEN for the
 *     chunk's rows (C26): d_q float [n][P] (AMPLI_AI_NA where untested), d_km int32 [n][P][2] = (k_lo, m) (zeros where untested),
 *     d_v double [n][P] (0.0 where untested), d_code uint8 [n][P] = status * 8 + pair (pair AMPLI_AI_NO_PAIR = 7 where there is none).
 *   Stage G.  Regions are a CSR IN DEVICE MEMORY as the amplicons of ampli_amplicon_depth_records: d_reg_off uint32 [R + 1],
 *     d_reg_pos uint32 [W]; they may overlap, repeat and be empty, an entry >= P is none, offsets are cut to [0, W].  Over the tested
 *     entries of a region (status >= AMPLI_AI_TESTED_REF and q != AMPLI_AI_NA), in the order AMPLI_AI_*: SITES += 1, SIG += 1 where
 *     |q| >= site_q, DEPTH += m, DEV16 += llrint(|(double)k_lo - v (double)m| 16.0), Q20 += llrint((double)|q| 1048576.0).  Integer
 *     additions only: order-free and exact.  d_sums int64 [S][R][5] is FULLY OVERWRITTEN (C27).
 * Launch shapes: R -- a workgroup per 64-position tile, its four waves take the rows w, w + 4, ...; S -- a wave per (tile, run of up
 * to 16 rows), all rows classified first, then all of a lane's tested cells in one loop of ampli_ai_step; G -- a wave per (region,
 * AMPLI_AI_STRIP rows).  No atomics: the same inputs give the same bytes.  All three are asynchronous on the context's stream.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer (prm is a host pointer), P <= 0, n_g < 1, S < 1,
 *   R < 1, W < 0, min_depth < 1, min_normals < 1, half_fallback not 0 / 1, site_q < 0 or NaN, broken records.  AMPLI_E_RANGE:
 *   P >= 2^31; P >= 2^28 with int32 records (R); n_samples > 4194240 (S); S > 2097120, W >= 2^27 (G).
 * The verdict of a region is decided on the host (ampli_host_allelic_region_verdict, include/amplisolve_host.h).
 */
int ampli_hetsite_reference_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes /* [n][6][W'] */,
                                    int32_t min_depth, int64_t *d_ref /* [3][6][P] */);
int ampli_allelic_site_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes_g /* [n_g][6][W'] */, int32_t n_g,
                               const int32_t *d_row_g /* [n] */, const int64_t *d_ref /* [3][6][P] */, const ampli_allelic_params *prm,
                               float *d_q /* [n][P] */, int32_t *d_km /* [n][P][2] */, double *d_v /* [n][P] */, uint8_t *d_code /* [n][P] */);
int ampli_allelic_region_sums(ampli_ctx *ctx, const float *d_q, const int32_t *d_km, const double *d_v, const uint8_t *d_code, int32_t S, int64_t P,
                              int32_t R, const uint32_t *d_reg_off /* [R + 1] */, const uint32_t *d_reg_pos /* [W] */, int64_t W, double site_q,
                              int64_t *d_sums /* [S][R][5] */);

/*
 * Tumour fraction per (sample, list) (the definition, in plain numpy, is tests/fraction_model.py): how much of a patient's
 * tumour is in this plasma sample, and within what bounds -- the score estimate of f and its Rao score interval.
 *   Lists.  The CSR of ampli_monitor_sums_records IN DEVICE MEMORY (d_list_off uint32 [L + 1], d_list_cell uint32 [W], an entry
 *     c = 4 p + y) and d_list_w float32 [W], the weight a of every entry: the variant's allele fraction per unit of tumour fraction, for
 *     example its tissue VAF divided by the purity.  A cell named twice counts twice; an entry with p >= P is none; offsets are cut to
 *     [0, W].  W >= 2^28 is AMPLI_E_RANGE.
 *   Evaluated entry of a row: exactly the rule of ampli_monitor_sums_records (PRIMARY record only, both strand depths >=
 *     coverage_cutoff, the max_vaf_pm cap, a reference base in 0..3 that y differs from, both thresholds finite and >= 0, e == 0
 *     replaced by 0.0010008f), and a weight that is finite, > 0 and <= 1.  It gives two cells, fw then bw, each with its count k of
 *     base y, its strand's depth d and its threshold e as doubles, a = (double)w and ad = a * d.  A cell is modelled as a Poisson
 *     count of mean d (e + f a): f is the fraction ABOVE THE TABLE'S RATES.
 *   Score and information at f; the operation sequence is part of the definition.  Per cell r = e + f * a; g = a / r; U += g * k - ad;
 *     I += g * ad.  Lane j of 64 takes the list's entries j, j + 64, ... in ascending order, fw before bw, into two accumulators that
 *     start at +0.0 (an entry that is not evaluated adds nothing); the 64 pairs are combined by x += x[lane ^ off] for off = 32, 16,
 *     8, 4, 2, 1.  T(f) = U * |U| / I.  Unfused IEEE operations, a correctly rounded division: the model, the host library and the
 *     device agree bit for bit.
 *   Values per (sample, list), in the order AMPLI_TF_*.  N_EVAL == 0 or I(0) <= 0: all four are AMPLI_TF_NA.  Every bisection takes
 *     AMPLI_TF_ITERS steps mid = 0.5 * (lo + hi) and gives 0.5 * (lo + hi).
 *     F_HAT: 0 if U(0) <= 0; 1 if U(1) >= 0; else on [0, 1] with U(mid) > 0 ? lo = mid : hi = mid.
 *     F_LO:  0 if T(0) <= z2; else on [0, F_HAT] with T(mid) > z2 ? lo = mid : hi = mid (T need not be monotone there in contrived
 *            lists: the bisection's result is the definition).
 *     F_HI:  0 if F_HAT == 0 and -T(0) >= z2; 1 if -T(1) < z2; else on [F_HAT, 1] with -T(mid) < z2 ? lo = mid : hi = mid.
 *     T0:    T(0), the signed squared score at zero.
 *   Counts per (sample, list): N_EVAL, the evaluated entries, and N_SEEN, those of them with k_fw + k_bw >= 1.
 *
 * ampli_fraction_records: d_est double [recs->n_samples][L][AMPLI_TF_VALS] and d_count int64 [recs->n_samples][L][AMPLI_TF_COUNTS],
 *   8-byte aligned, FULLY OVERWRITTEN with plain stores (C28); a streamed cohort passes each chunk its rows of one matrix.  A wave owns
 *   one list and 8 consecutive rows; lists of up to 256 entries keep their entries and the row's cells in registers, an evaluation of
 *   the sums is then one division per cell and the butterfly; longer lists are gathered again for each of the up to 182 evaluations
 *   (slow).  L == 0 writes nothing and succeeds.
 * Refusals, every output untouched.  AMPLI_E_INVALID: a null or misaligned pointer (prm is a host pointer), P <= 0, L < 0, W < 0,
 *   coverage_cutoff < 0, max_vaf_pm outside 0..1000, z2 not finite or <= 0, broken records.  AMPLI_E_RANGE: P >= 2^31, W >= 2^28,
 *   n_samples > 2097120.
 * No LDS, no barrier, no atomics: the same inputs give the same bytes.  Asynchronous on the context's stream.  The verdict of a
 * (sample, list) and the change between two draws are decided on the host (include/amplisolve_host.h).
 */
int ampli_fraction_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                           const uint32_t *d_list_off, const uint32_t *d_list_cell, const float *d_list_w, int32_t L, int64_t W,
                           const ampli_fraction_params *prm, double *d_est /* [n][L][4]: F_HAT, F_LO, F_HI, T0 */,
                           int64_t *d_count /* [n][L][2]: N_EVAL, N_SEEN */);

/* free and total bytes of the context's device (hipMemGetInfo), for callers that keep a whole cohort resident */
int ampli_mem_info(ampli_ctx *ctx, size_t *free_bytes, size_t *total_bytes);

/* Asynchronous drain (opt-in).  In prefilter mode poisson_call is two kernels; the second (the dense drain of the
 * queued survivors) is one fp64 scorer chain long and independent of what the caller enqueues next.  With
 * ampli_set_async_drain(ctx, 1) it runs on a side stream of the context: the call mask, the call list and
 * d_n_calls of a poisson_call are then complete only after ampli_wait_calls (the context's stream waits, the host
 * does not block), ampli_sync, ampli_copy_d2h, ampli_ctx_flags or the next ampli_poisson_call; the outputs must
 * stay untouched until then (the queued items carry their own thresholds and depths). */
int ampli_set_async_drain(ampli_ctx *ctx, int32_t on);
int ampli_wait_calls(ampli_ctx *ctx);

/* hipGraph capture of a sequence of calls on the context's stream (small, launch-bound panels).  The context must
 * own a real stream (AMPLI_STREAM_OWN or a non-null stream) and the sequence must have run once (workspaces warm).
 * ampli_graph_end returns a hipGraphExec_t as an opaque pointer; launch it any number of times. */
int ampli_graph_begin(ampli_ctx *ctx);
int ampli_graph_end(ampli_ctx *ctx, void **graph_exec);
int ampli_graph_launch(ampli_ctx *ctx, void *graph_exec);
int ampli_graph_destroy(void *graph_exec);

/*
 * Native transport of the multi-GPU merge (one process per GPU, no Python): RCCL over xGMI, bound at run time
 * (librccl.so is only loaded when a communicator is created).  Rendezvous through a file every rank can see: rank 0
 * removes whatever file of that name a dead run left behind and writes its ncclUniqueId there, tagged with the world size,
 * the launch's AMPLISOLVE_JOB_NONCE (optional; any integer the launcher gives every rank) and the time; the others wait up
 * to timeout_s for a file that carries THEIR world size and nonce and is not older than the job, and ncclCommInitRank
 * itself is bounded by timeout_s as well (RCCL has no timeout of its own): a missing rank or a stale file ends in
 * AMPLI_E_HIP (no usable id file) or AMPLI_E_COMM_TIMEOUT (the init itself timed out: the caller must _exit, see the
 * code's comment) with a message, never in a hang.  A rank above 0 reads the file once more 0.25 s after accepting it and
 * takes the newer one, so a relaunch right after a crash does not pick up the dead run's id in the moment before rank 0
 * replaces it (without a nonce that window cannot be closed completely: give every launch its AMPLISOLVE_JOB_NONCE).  Collectives are enqueued on the context's
 * stream; the *_i32 / *_i64 helpers take HOST values and synchronise.  Buffer shapes as in "Position-sliced merge".
 */
typedef struct ampli_comm ampli_comm;
int ampli_comm_create(ampli_ctx *ctx, int32_t rank, int32_t world, const char *id_file, int32_t timeout_s, ampli_comm **out);
void ampli_comm_destroy(ampli_comm *c);
int ampli_comm_reduce_scatter_f64(ampli_comm *c, const double *d_send /*[world][count]*/, double *d_recv /*[count]*/, int64_t count);
int ampli_comm_all_to_all_f32(ampli_comm *c, const float *d_send /*[world][count]*/, float *d_recv /*[world][count]*/, int64_t count);
int ampli_comm_all_gather_bytes(ampli_comm *c, const void *d_send /*[bytes]*/, void *d_recv /*[world][bytes]*/, int64_t bytes);
int ampli_comm_all_reduce_max_i32(ampli_comm *c, int32_t *values /*host, in place*/, int32_t n);
int ampli_comm_exclusive_sum_i64(ampli_comm *c, int64_t mine, int64_t *before);
int ampli_comm_barrier(ampli_comm *c);

/* scalar scorer on the device for known-answer tests: q[i] = score(k[i], rd[i], err[i]),
 * p[i] = 1 - kf_gammaq(k, rd*err) (VC:3834-3884).  Either output may be NULL. */
int ampli_score_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err,
                      int64_t n, double *d_q, double *d_p);
/* the scorer of the all-scores mode (AMPLI_POISSON_FULL) for the same tests: the integer-count form of the same recipe --
 * lgamma from a table of the Lanczos form's own values, division-free series and continued fraction (csrc/ampli_math.h,
 * ampli_poisson_score_dense); q[i] equals ampli_score_batch's to rounding (~1e-13 relative on p) */
int ampli_score_dense_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err, int64_t n, double *d_q);
/* the scorer of the prefilter mode's drain for the same tests: one strand of a queued item, a count k against a mean
 * m = rd * err with 0 < m < k (the series branch, division-free, lgamma(k + 1) from the same table; csrc/ampli_math.h,
 * ampli_drain_p): p[i] and q[i] = Q of it, as ampli_host_drain_score_batch.  Outside 0 < m < k the result is whatever that
 * arithmetic gives (the drain never asks).  Either output may be NULL. */
int ampli_drain_score_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err, int64_t n, double *d_q,
                            double *d_p);
/* text round trip on the device for known-answer tests: out[i] = stof(sprintf("%f", in[i])) */
int ampli_roundtrip_batch(ampli_ctx *ctx, const float *d_in, int64_t n, float *d_out);

/* deterministic synthetic panel generated in HBM: fills recs[n_samples][P][8]
 * for samples [first_sample, first_sample+n_samples) of panel `seed`; tumour != 0 spikes SNVs.
 * Bit-identical to ampli_synth_record() on the host (amplisolve_amd/csrc/ampli_synth.h).
 * n_samples > 65535 is AMPLI_E_RANGE (one grid row per sample): fill a larger panel in parts. */
int ampli_synth_fill(ampli_ctx *ctx, int32_t *d_recs, int64_t P, int32_t n_samples,
                     int32_t first_sample, uint64_t seed, int32_t depth, int32_t tumour);
int ampli_synth_ref(ampli_ctx *ctx, uint8_t *d_ref_code, int64_t P, uint64_t seed);

/*
 * Upstream of the path: alignments -> per-position counts, i.e. what ASEQ's PILEUP mode / the reference's binary-only
 * computeCounts produce (/root/reference/Execution_examples.md:16-46: vcf= bam= mbq= mrq= mdc=).  d_bam: the UNCOMPRESSED BAM
 * alignment records (the host inflates the BGZF blocks); d_rec_off[i]: byte offset of record i's block_size field, every listed
 * record lying completely inside d_bam with a CIGAR that matches its l_seq (the host checks), and the buffer readable for 16 bytes
 * behind the last record (the kernel copies whole 16-byte pieces; d_bam itself 16-byte aligned); d_rec_off must be ASCENDING (a
 * workgroup takes the bytes of its consecutive records from its first and its last offset; bytes between records are skipped);
 * d_keys[P]: the panel's unique
 * positions as (BAM reference id << 32 | 1-based position), ascending.  d_counts int32 [P][8] = {A,C,G,T, Ars,Crs,Grs,Trs} is
 * ACCUMULATED into (zero it first; batches of one file add up).  Kept reads: mapped, not secondary / QC-fail / duplicate,
 * MAPQ >= mrq; counted bases: M / = / X columns, A/C/G/T, base quality >= mbq.  d_stats (optional, 2 words, accumulated):
 * reads kept, bases counted.  AMPLI_E_INVALID, before anything is launched: a d_bam that is not 16-byte aligned, or d_rec_off, d_keys,
 * d_stats (8 bytes) or d_counts (4 bytes) below the alignment of its type.  The three walks below and the two gathers refuse typed
 * pointers below their natural alignment in the same way.
 */
int ampli_pileup_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P,
                       int32_t mbq, int32_t mrq, int32_t *d_counts, uint64_t *d_stats);

/*
 * Indel counting over the same alignment records: per panel position and read strand, how many reads show an insertion, a
 * deletion or neither at the junction behind that position, written into the record slots every other entry point reads.  The stream
 * contract is ampli_pileup_count's (d_bam, d_rec_off ascending, 16-byte alignment, 16 readable bytes behind the last record, d_keys).
 *
 * Kept reads are exactly those of ampli_pileup_count: placed, none of the flags 0x4 / 0x100 / 0x200 / 0x400, and MAPQ >= mrq.
 * Effective operations: a read's CIGAR is taken with every operation of length 0 and every P operation removed.  What remains are the
 * read's effective operations.
 * Junction p is the boundary between reference positions p and p + 1 (1-based).  p must be a panel key.  p + 1 need not be.
 * Observing a junction: a read observes junction p when its base at p lies in an M, = or X column and that base's quality is >= mbq.
 * There is no condition on the base's letter.  The next effective column or operation must be one of these:
 *   another M / = / X column at p + 1, in the same operation or the next one          slot 0, A ("reference junction")
 *   one I of length L >= 1, followed directly by an M / = / X operation                slot 1, C (insertion)
 *   one D of length L >= 1, followed directly by an M / = / X operation                slot 2, G (deletion)
 * Anything else leaves the junction unobserved by that read, and it is counted nowhere.  That covers the read's last aligned column, a
 * soft or hard clip, an N, I then D, D then I, two I, and an indel that opens or closes the alignment.
 * Reverse-strand reads (flag 0x10) also add to slot + 4.  Slots 3 and 7 (T) are never written.  So per position A + C + G is the number
 * of kept reads that observed the junction, and the record's depth is what the existing gates expect it to be.
 *
 * State machine: the definition is a state machine over the effective operations and needs no look-ahead.  Its state is "previous
 * effective operation was a match run, ending at column p with query index q" plus at most one pending indel.
 *   A match run first settles what is pending: the pending event at its anchor, or a reference junction between two adjacent match runs.
 *   It then counts its own len - 1 inner junctions as reference junctions.
 *   I or D behind a match run with nothing pending becomes pending.
 *   Every other case clears both states.
 *
 * d_counts int32 [P][8] is ACCUMULATED into.  d_lengths (optional, may be NULL) int32 [P][2][AMPLI_INDEL_LEN_BINS] is accumulated into:
 * kind 0 is insertion and kind 1 is deletion, the bin is min(L, 32) - 1, both strands are pooled, and over the bins of a kind the sum
 * equals slot 1 (kind 0) or slot 2 (kind 1).  d_stats (optional, 2 words, accumulated): reads kept, junctions counted over all three
 * slots.  Bad arguments give AMPLI_E_INVALID ("bad argument").  n_reads == 0 or P == 0 is a no-op that returns AMPLI_OK.
 * Limits: events are taken where the aligner placed them (no left-alignment), the inserted bases are not recorded, all lengths at a
 * junction share one count, complex events (I next to D) are ignored.
 */
int ampli_pileup_indel_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P,
                             int32_t mbq, int32_t mrq, int32_t *d_counts, int32_t *d_lengths, uint64_t *d_stats);

/*
 * Amplicon-resolved counting over the same alignment records: every kept read is assigned to the amplicon it came from and
 * counted there only, so that a position under two amplicons keeps two records.  The stream contract is ampli_pileup_count's (d_bam,
 * d_rec_off; this kernel reads the records straight from global memory and needs neither ascending offsets nor the 16 bytes behind).
 *
 * Amplicons.  There are A intervals on the BAM's references, 1-based and inclusive.  They are given as keys
 * lo[a] = ref_id << 32 | first and hi[a] = ref_id << 32 | last.  They are sorted by lo ascending, then hi ascending.  The host sorts
 * them and keeps the permutation back to BED order.  Intervals may overlap, nest and repeat.  reach[a] = max(hi[0..a]).  It is
 * monotone, so the candidates of a read form a contiguous index range even with nested amplicons.  amp_off[a] is the exclusive prefix
 * sum of the lengths last - first + 1, and W = amp_off[A].  Walk entry w = amp_off[a] + (x - first[a]) is the cell "position x as seen
 * by amplicon a".  This is the same order as DESIGN 16's amp_off / amp_pos CSR for BED rows.
 * Kept reads.  These are exactly the reads ampli_pileup_count keeps: the read is placed; none of the flags 0x4 / 0x100 / 0x200 / 0x400
 * is set; MAPQ >= mrq.
 * Span.  span_first = pos + 1.  span_last = pos + R, where R is the sum of the lengths of the read's M = X D N operations.  A read with
 * R = 0 is unassigned.
 * Overlap.  The overlap of a read with amplicon a is the number of reference positions in both intervals on the same reference.  It is
 * 0 if there are none.
 * Assignment.
 *   1. The read belongs to the amplicon of largest overlap.
 *   2. Among ties, it belongs to the amplicon with the smallest anchor distance: |span_first - first[a]| for a forward read;
 *      |span_last - last[a]| for a read with flag 0x10.  Amplicon reads start at their amplicon's own end.
 *   3. Among ties still, it belongs to the lowest index a in the sorted order.
 *   4. The assignment stands only if overlap >= 1 and overlap x 100 >= min_overlap x (span_last - span_first + 1).  The arithmetic is
 *      int64 integer arithmetic.  min_overlap is an integer in [1, 100] and defaults to 50.
 *   5. Otherwise the read is off-target.  It is counted in the statistics and nowhere else.
 * Counting.  For a read assigned to a, every M / = / X column adds 1 to counts[w][nt] when all of these hold: its reference position x
 * satisfies first[a] <= x <= last[a]; its base is A/C/G/T; its base quality is >= mbq.  A reverse read also adds 1 to
 * counts[w][4 + nt].  A column outside the amplicon's interval is clipped.  It is counted in no cell and tallied in the statistics
 * (whatever its base and its quality).
 * Outputs.  d_counts: int32 [W][8], accumulated into.  d_amp_reads: int64 [A][2], assigned forward and reverse reads, accumulated.
 * d_stats: optional (may be NULL), uint64 [4], accumulated.  Its four words are reads kept, reads assigned, bases counted and bases
 * clipped.  d_amp_off is read at [0, A); W is passed beside it.
 * Refusals.  AMPLI_E_RANGE: W >= 2^31; more than 2^31 - 1 read groups.  AMPLI_E_INVALID: min_overlap outside [1, 100]; a null required
 * pointer; negative sizes.  A = 0 or n_reads = 0 is a successful no-op.
 * Stated limits.  A read is assigned from its alignment alone, not from its primer sequence.  A chimeric read is given to its larger
 * part.  An amplicon wholly inside another wins only reads that fit it better by the anchor rule.
 */
int ampli_pileup_amplicon_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_lo,
                                const uint64_t *d_hi, const uint64_t *d_reach, const int64_t *d_amp_off, int64_t A, int64_t W, int32_t mbq,
                                int32_t mrq, int32_t min_overlap, int32_t *d_counts, int64_t *d_amp_reads, uint64_t *d_stats);
/*
 * Layers (a gather over the counts of ampli_pileup_amplicon_count).  For every listed panel position d_keys[p] (reference id
 * << 32 | 1-based position; any order, repeats allowed), take the amplicons that cover it, in sorted order.  Layer l < L is the record
 * of the l-th covering amplicon.  Where there is none, it is the project's absent-record marker: slot 0 = INT32_MIN, the rest 0.
 * d_layers: int32 [L][P][8].  d_layer_amp: int32 [L][P], that amplicon's sorted index, or -1.  d_total: int32 [P][8], the sum over ALL
 * covering amplicons, including those beyond L.  Every output cell has one owner and is overwritten, not accumulated.  A position under
 * no amplicon gets zeros in d_total.  d_counts, d_layers and d_total are 16-byte aligned (the gather loads and stores int4; anything else
 * is AMPLI_E_INVALID).  L = 0 gives the totals alone (d_layers and d_layer_amp may then be NULL).
 * Refusals as above (AMPLI_E_RANGE: W >= 2^31; AMPLI_E_INVALID: a null required pointer, negative sizes).  A = 0 or P = 0 is a
 * successful no-op.  Layer order is genomic and not biological.
 */
int ampli_amplicon_layers(ampli_ctx *ctx, const int32_t *d_counts, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_reach,
                          const int64_t *d_amp_off, int64_t A, int64_t W, const uint64_t *d_keys, int64_t P, int32_t L, int32_t *d_layers,
                          int32_t *d_layer_amp, int32_t *d_total);

/*
 * Read-level evidence over the same alignment records: what the reads behind a count looked like.  The stream contract is
 * ampli_pileup_count's (d_bam, d_rec_off, d_keys; this kernel reads the records straight from global memory and needs neither ascending
 * offsets nor the 16 bytes behind).
 *
 * Counted column.  A counted column is exactly a column that ampli_pileup_count adds to counts[p][nt]: the read is kept (placed, none of
 * the flags 0x4 / 0x100 / 0x200 / 0x400, MAPQ >= mrq); it is an M / = / X column whose reference position is the panel key d_keys[p]; its
 * base is A/C/G/T; its quality is >= mbq.  The effective operations are those of ampli_pileup_indel_count: zero-length operations and P
 * are dropped.
 * Bins.  Every counted column adds 1 to three bins of d_hist, int32 [P][4][AMPLI_EVIDENCE_METRICS][AMPLI_EVIDENCE_BINS] in the order
 * (position, nt, metric, bin).  Strands are pooled.  d_hist is ACCUMULATED into.
 *   AMPLI_EVIDENCE_BQ   bin min(q, 63), q the column's quality byte
 *   AMPLI_EVIDENCE_MQ   bin min(mapq >> 2, 63)
 *   AMPLI_EVIDENCE_POS  bin min(d, 63) with d = min(i, l_seq - 1 - i), i the column's 0-based index into the record's SEQ: soft-clipped
 *                       and inserted bases in front of the column count towards i, hard clips and deletions do not
 * Invariant.  For every position, nt and metric the sum over the 64 bins equals counts[p][nt] of ampli_pileup_count over the same records,
 * mbq and mrq.
 * d_stats (optional, may be NULL) uint64 [2], accumulated: reads kept, columns counted.  Bad arguments give AMPLI_E_INVALID ("bad
 * argument"), more than 2^31 - 1 read groups AMPLI_E_RANGE.  n_reads == 0 or P == 0 is a no-op that returns AMPLI_OK.
 * Stated limits.  MAPQ is seen only at or above mrq and qualities only at or above mbq (that is what makes the invariant hold); strands
 * are pooled; POS is the distance to the nearer end of the stored sequence, not to the primer.
 */
int ampli_pileup_evidence(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P,
                          int32_t mbq, int32_t mrq, int32_t *d_hist, uint64_t *d_stats);
/*
 * The rank-sum score of alt reads against ref reads, one cell per (position, metric) of d_hist.  d_ref_nt, d_alt_nt: int8 [P].
 * An alt of -1 means "choose": the non-reference nt with the largest total count (over its BQ bins), ties to the lowest index.  A ref
 * outside 0 .. 3 leaves the position's cells untested, and so does an alt outside -1 .. 3 or equal to ref; a side without a usable nt reads
 * as an empty histogram.
 * With a_b and r_b the alt and ref histograms of the metric, n1 = sum a_b, n2 = sum r_b, N = n1 + n2, t_b = a_b + r_b:
 *   1. U2 = sum_b a_b (2 R_<b + r_b) with R_<b = sum_{c<b} r_c, int64: twice the Mann-Whitney U of alt over ref, ties counted half.
 *   2. D = U2 - n1 n2, int64.
 *   3. Medians: the smallest b with 2 cum_b >= n, per side; -1 when n = 0.
 *   4. In doubles, nothing contracted: Td = sum_b ascending ((double)t_b x (double)t_b x (double)t_b - (double)t_b), Nd = (double)N,
 *      c = (Nd + 1.0) - Td / (Nd x (Nd - 1.0)), v = (double)n1 x (double)n2 x c.
 *   5. z2 = 3.0 x (double)D x (double)D / v, negated when D < 0: the signed square of the tie-corrected normal score without continuity
 *      correction.  A negative value means the alt reads rank below the ref reads.
 * Every operation is one IEEE + - x / in this order; no sqrt, erfc or log runs on the device.
 * Untested cells: n1 = 0, n2 = 0, N >= 2^30 (keeps U2 < 2^63) or !(v > 0) (all reads in one bin).  Such a cell gets u2 = -1 and z2 = 0; its
 * counts and medians are still written.
 * Outputs, every cell with one owner and overwritten: d_int int64 [P][3][3] = n_ref, n_alt, u2; d_med int32 [P][3][2] = med_ref, med_alt;
 * d_z2 double [P][3]; d_alt_used int8 [P], the alt nt that was used, or -1.  A null pointer or P < 0 gives AMPLI_E_INVALID ("bad
 * argument"), P == 0 is a no-op.  The score is a normal approximation: report it only from a few reads a side (computeReadEvidence: min_alt).
 */
int ampli_evidence_score(ampli_ctx *ctx, const int32_t *d_hist, int64_t P, const int8_t *d_ref_nt, const int8_t *d_alt_nt, int64_t *d_int,
                         int32_t *d_med, double *d_z2, int8_t *d_alt_used);

/*
 * Read-level phasing over the same alignment records: which alleles a read shows at two listed positions at once.  The stream
 * contract is ampli_pileup_evidence's (d_bam, d_rec_off, d_keys ascending; the records are read straight from global memory), and so are
 * the kept-read filter and the effective operations.  The context is the LAST parameter of this entry point and of ampli_phase_score.
 *
 * Covered key.  A key is covered by a kept read iff it is on the read's reference and its position lies in [pos + 1, pos + L], L the summed
 * length of the read's effective M = X D N operations.  The keys a read covers are a contiguous range of the list.
 * State of a read at a covered key.  0 .. 3 = A C G T where the key falls on an M / = / X column whose base is A/C/G/T with quality >= mbq:
 * exactly a counted column of ampli_pileup_evidence.  AMPLI_PHASE_OTHER (4) otherwise: a base below mbq, a non-ACGT base, a key inside a
 * D or an N.
 * Output.  d_table is int32 [P][K][5][5], K = AMPLI_PHASE_PARTNERS, in the order (key i, partner k, state at key i, state at key
 * i + 1 + k), and is ACCUMULATED into.  Every kept read adds 1 to d_table[i][k][s_i][s_j] for every two keys i < j = i + 1 + k <= i + K that
 * it both covers.  Cells with i + 1 + k >= P are never written.
 * d_stats (optional, may be NULL) uint64 [3], accumulated: reads kept, reads covering at least two keys, cells incremented.
 * Invariant.  Take a pair cell (i, k) where every kept read that covers one of the two keys covers both.  Then for s <= 3 the sum over t of
 * d_table[i][k][s][t] equals counts[i][s] of ampli_pileup_count (its slots 0 .. 3: both strands pooled) over the same records, mbq and
 * mrq, and the sum over s of d_table[i][k][s][t] equals counts[j][t] for t <= 3.
 * Bad arguments and alignments (8 bytes: d_rec_off, d_keys, d_stats; 4 bytes: d_table) give AMPLI_E_INVALID ("bad argument"), more than
 * 2^31 - 1 read groups AMPLI_E_RANGE.  n_reads == 0 or P == 0 is a no-op that returns AMPLI_OK.
 * Stated limits.  Records are counted, not fragments: overlapping mates count twice, as in computeCounts.  Only the next K listed keys are
 * partners: pairs further apart in the list are never counted.  Strands are pooled.  An insertion has no key.
 */
int ampli_pileup_phase(const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P, int32_t mbq, int32_t mrq,
                       int32_t *d_table, uint64_t *d_stats, ampli_ctx *ctx);
/*
 * The pair score over the joint table: are the alts of two listed keys on the same reads?  The alleles are chosen here, not in
 * the walk.  d_pair_cell: int64 [Q], each i K + k (the pair of key i and key j = i + 1 + k); d_pair_nt: int8 [Q][4], each ref_i, alt_i,
 * ref_j, alt_j in 0 .. 3 = A C G T.  min_alt >= 1; min_share in 0 .. 100 (per cent).  The context is the LAST parameter.
 * Counts, from the pair's 5 x 5 cell (the first letter is the state at key i): n_rr, n_ra, n_ar, n_aa its four corners; n_joint the sum
 * of all 25; n_other = n_joint - the four corners.
 * Score = ampli_pair_score_records' exact conditional test of the 2 x 2 table with k_a = n_aa, d_a = n_aa + n_ar, k_b = n_ra,
 * d_b = n_ra + n_rr: positive when alt at j is commoner among the reads that show alt at i -- the two are linked in cis --, negative when
 * it is rarer, +0 without a difference.
 * Class, a bit mask.  With m = n_aa + n_ar + n_ra a group x is present iff x >= min_alt and 100 x >= min_share m, compared in int64.
 * Bit 0: aa, bit 1: ar, bit 2: ra.
 * Untested pairs: a pair cell outside [0, P K) or with i + 1 + k >= P; any nt outside 0 .. 3; ref == alt on either side.  Such a pair gets
 * class -1 and score 0, and its counts are written as -1; d_table is not read for it.
 * Outputs, each cell with one owner and overwritten: d_int int64 [Q][6] = rr, ra, ar, aa, joint, other; d_score float [Q]; d_class int32
 * [Q].  A null pointer, P < 0, Q < 0, a min_alt or min_share outside its range or a misaligned pointer (8 bytes: d_pair_cell, d_int; 4 bytes:
 * d_table, d_score, d_class) gives AMPLI_E_INVALID ("bad argument"), more than 2^31 - 1 groups of 256 pairs AMPLI_E_RANGE.  Q == 0 is a no-op.
 */
int ampli_phase_score(const int32_t *d_table, int64_t P, const int64_t *d_pair_cell, const int8_t *d_pair_nt, int64_t Q, int32_t min_alt, int32_t min_share,
                      int64_t *d_int, float *d_score, int32_t *d_class, ampli_ctx *ctx);

/* tuning knobs.  reduce_sample_splits: 0 = automatic.  reduce_general: 0 = the fast error_reduce kernel
 * (valid while every strand depth is < 2^22; it raises AMPLI_FLAG_RERUN_GENERAL otherwise), 1 = the literal
 * kernel that follows the reference operation by operation for any depth (slower).  reduce_lane_groups: lane
 * groups per wave of error_reduce (1, 2 or 4; 0 = automatic: 1 unless the panel is too small to fill the chip). */
int ampli_set_tuning(ampli_ctx *ctx, int32_t reduce_sample_splits, int32_t reduce_general, int32_t reduce_lane_groups);
/* error_reduce with a compact per-position state (96 VGPRs: five waves per SIMD instead of four) -- error_reduce_u16_kernel for
 * uint16 records (at most 4096 samples per launch) and, since round 5, error_reduce_u24_kernel for 24-bit records (at most 4092
 * samples; a covered record with RD >= 2^22 raises AMPLI_FLAG_RERUN_GENERAL like the fast general kernel): taken by
 * ampli_error_estimate / ampli_error_reduce_records(_sliced) / ampli_error_reduce_sliced when on != 0 (the default) and the launch
 * has the shape they cover -- fast kernel, one lane group, one sample split, and either no accumulator table (finalize fused, or
 * the shard's sums straight into the sliced exchange buffers) or a table the caller takes as streaming state
 * (AMPLI_REDUCE_SUMMARY).  Positions listed more than once (E > 0) are served: their tiles go to the general kernel over a list.
 * Every other launch takes the general kernel.  Same results, bit for bit.  on = 2: the uint16 form only (A/B runs). */
int ampli_set_reduce_compact(ampli_ctx *ctx, int32_t on);
/* Which kernel the context's latest error_reduce launch was: 0 = error_reduce_kernel (general), 1 = error_reduce_u16_kernel,
 * 2 = error_reduce_u24_kernel (compact state); AMPLI_E_INVALID before the first launch.  For tests and the bench line, which name the kernel they measured. */
int ampli_last_reduce_kernel(const ampli_ctx *ctx);

/*
 * Position ranges on concurrent streams (round 5).  A resident panel is rarely a whole number of rounds of workgroups (config 3:
 * 1563 tiles of 64 positions on 1280 resident workgroups of error_reduce), and a launch's partly filled last round runs at a
 * fraction of the chip.  With n_ranges > 1 (at most 4) ampli_error_estimate / ampli_error_reduce_records and ampli_poisson_call /
 * _records (prefilter mode) cut the panel into n tile-aligned ranges of positions, each on a stream the context owns (the
 * context's own stream only forks into them and joins them), each range's poisson_call behind its own error_estimate (a position's
 * thresholds are all a record of that position needs).  Over BACK-TO-BACK passes on independent batches one range's poisson_call
 * and another's error_reduce then fill each other's thin rounds (config 3: 0.143-0.155 -> 0.132-0.139 ms per pass; more than two
 * ranges buy nothing more); a single pass gains nothing -- the
 * join at its end costs what the overlap inside it saves -- so the command lines do not use it.  Outputs are the same arrays,
 * bit for bit; the call list's shards are dealt to the ranges (range k appends to shards [32 k / n, 32 (k + 1) / n)), so a shard
 * fills n times faster than without ranges.
 * Semantics: the section opens at the first such call (the ranges' streams wait for everything enqueued on the context's stream
 * so far) and CLOSES -- the context's stream waits for every range -- at the next call of any other entry point on the context
 * (ampli_sync, copies, ampli_event_record, ampli_ctx_flags, every other kernel, ampli_stream), or at ampli_ranges_join.  While
 * it is open the caller must not enqueue work of its own that writes the ranges' inputs or reads their outputs.  Launches outside
 * the shape (positions listed more than once, another record layout than the compact kernel's for error_estimate, the all-scores
 * mode, a panel of fewer than 2 n tiles, P + E not a multiple of 4 for poisson_call, stream capture) simply run unsplit, after a join.
 */
int ampli_set_ranges(ampli_ctx *ctx, int32_t n_ranges);
int ampli_ranges_join(ampli_ctx *ctx);
/* 1 when ampli_set_ranges saw every pair of the ranges' streams run concurrently; 0 when it could not find streams on different
 * hardware queues (HIP deals streams to a few queues by rules of its own: ampli_set_ranges probes each new stream against the earlier
 * ranges' with a short sleeping kernel and replaces one that shares a queue) -- results are the same either way, the overlap is not. */
int ampli_ranges_concurrent(const ampli_ctx *ctx);
/* An event (ampli_event_create) on range `range`'s stream WITHOUT closing the section: events recorded before and after a call
 * bracket that range's share of it -- the kernels' durations under the overlap the ranges exist for.  (ampli_event_record is an
 * ordinary call: it closes the section first and records on the context's stream.) */
int ampli_range_event_record(ampli_ctx *ctx, int32_t range, void *ev);

/* poisson_call (prefilter mode) launch shape; 0 = default for each.  rows_per_wave: tumour rows one wave streams
 * (a workgroup = 4 waves over one 64-record tile and 4 * rows_per_wave rows).  drain_blocks_per_shard: workgroups per
 * queue shard in the drain launch.  Results do not depend on either. */
int ampli_set_poisson_tuning(ampli_ctx *ctx, int32_t rows_per_wave, int32_t drain_blocks_per_shard);

/* Minimum capacity (items of 40 B) of the prefilter queue of ampli_poisson_call; default T*R/4, at least 65536. */
int ampli_set_queue_items(ampli_ctx *ctx, int64_t items);

/* Flags raised by kernels of this context since the last clear (synchronises the stream). */
#define AMPLI_FLAG_QUEUE_OVERFLOW 4 /* poisson_call (prefilter) ran out of queue space: masks/calls incomplete, raise
                                       ampli_set_queue_items (or use AMPLI_POISSON_FULL) and rerun */
#define AMPLI_FLAG_SLICE_RANGE 8 /* sliced exchange in the slim format: a shard's value does not fit its share of a packed field; repeat
                                  * the exchange with ampli_set_slice_format(ctx, AMPLI_SLICE_WIDE) */
#define AMPLI_FLAG_RERUN_GENERAL 2 /* error_reduce met a depth >= 2^22: its table is invalid, rerun with reduce_general = 1 */
int ampli_ctx_flags(ampli_ctx *ctx, int32_t *out, int32_t clear);

#ifdef __cplusplus
}
#endif
#endif /* AMPLISOLVE_HIP_H */
