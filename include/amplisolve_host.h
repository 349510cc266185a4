/*
 * include/amplisolve_host.h -- C ABI of libamplisolve_host.so: the C++ host
 * side of the two AmpliSolve command lines (argv, BED / FASTA / .PILEUP.ASEQ /
 * error-table parsing, the SoA packer, the writers).  The executables
 * AmpliSolveErrorEstimation / AmpliSolveVariantCalling are thin mains over
 * this library; tests drive the same entry points through ctypes.
 *
 * The host library holds NO arithmetic of the hot path: sums, rates, p-values
 * and the call gate come from libamplisolve_hip.so (include/amplisolve_hip.h),
 * which it loads at run time and without which every pipeline entry point
 * fails with AMPLI_E_HIP.
 *   EE:n = /root/reference/source_codes/AmpliSolveErrorEstimation.cpp:n
 *   VC:n = /root/reference/source_codes/AmpliSolveVariantCalling.cpp:n
 */
#ifndef AMPLISOLVE_HOST_H
#define AMPLISOLVE_HOST_H
#include <stddef.h>
#include <stdint.h>
#include "amplisolve_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic panels: bit-identical to ampli_synth_fill on the device ---- */
int ampli_host_synth_fill(int32_t *recs /*[n_samples][P][8]*/, int64_t P, int32_t n_samples,
                          int32_t first_sample, uint64_t seed, int32_t depth, int32_t tumour);
int ampli_host_synth_ref(uint8_t *ref_code /*[P]*/, int64_t P, uint64_t seed);

/* the same panel as files: BED + "chrom pos base" table, and one .PILEUP.ASEQ per sample (<dir>/<prefix>NNNNN.PILEUP.ASEQ)
 * with exactly the counts ampli_host_synth_fill / ampli_synth_fill produce; returns the bytes of text written (< 0: error) */
int ampli_host_synth_write_panel(const char *bed_path, const char *refbases_path, int64_t P, uint64_t seed);
int64_t ampli_host_synth_write_aseq(const char *dir, const char *prefix, int64_t P, int32_t n_samples, int32_t first_sample,
                                    uint64_t seed, int32_t depth, int32_t tumour, int32_t n_threads);

/* ---- scalar helpers of csrc/ampli_math.h compiled for the host (formatting, unit checks) ---- */
void ampli_host_text_roundtrip_batch(const float *in, int64_t n, float *out);
int32_t ampli_host_af_limit(int32_t d);
void ampli_host_af_limit_batch(const int32_t *d, int64_t n, int32_t *out);
void ampli_host_af_limit_f32_batch(const int32_t *d, int64_t n, int32_t *out); /* ampli_af_limit_f32((float)d[i]) */
int ampli_host_prefilter_nocall(int32_t k, int32_t rd, float err);
int ampli_host_prefilter_skip_f32(int32_t k, int32_t rd, float err); /* the streaming kernel's fp32 form */
/* the all-scores mode's scorer (ampli_poisson_score_dense, csrc/ampli_math.h) on the host, lgamma computed: Q */
void ampli_host_dense_score_batch(const int32_t *k, const int32_t *rd, const float *err, int64_t n, double *q);
/* the drain kernel's scorer (division-free series, csrc/ampli_math.h) for items with k > rd*err > 0: Q and p */
void ampli_host_drain_score_batch(const int32_t *k, const int32_t *rd, const float *err, int64_t n, double *q, double *p);
/* the same two with kf_lgamma at the integers read from a table of AMPLI_LGTAB entries, as the kernels read it: the table is
 * filled once, by the host's own ampli_kf_lgamma; the results carry the same bits as the two above for every int32 input */
void ampli_host_dense_score_table_batch(const int32_t *k, const int32_t *rd, const float *err, int64_t n, double *q);
void ampli_host_drain_score_table_batch(const int32_t *k, const int32_t *rd, const float *err, int64_t n, double *q, double *p);

/* ---- panel + cohort: BED (or error table) + a directory of .PILEUP.ASEQ packed into the record SoA ---- */
typedef struct ampli_host_cohort ampli_host_cohort;
const char *ampli_host_last_error(void);
/* bed_or_table: BED panel (EE:615-650) or, with is_error_table != 0, a positionSpecificNoise table (VC:430-576).
 * Reference bases from refbases_file ("chrom pos base" lines, EE:963) or from a FASTA (+ optional .fai);
 * aseq_dir may be NULL (panel only).  Samples come out in the reference's visit order (EE:1081 / VC:672). */
int ampli_host_cohort_load(const char *bed_or_table, int is_error_table, const char *refbases_file, const char *fasta,
                           const char *aseq_dir, int n_threads, int keep_line_no, ampli_host_cohort **out);
/* the same for shard shard_index of shard_count: only that contiguous range of the visit order is parsed (one process per
 * GPU; the ranges are those of amplisolve_amd/dist.py::shard_range).  first_sample = visit-order index of its sample 0 */
int ampli_host_cohort_load_shard(const char *bed_or_table, int is_error_table, const char *refbases_file, const char *fasta,
                                 const char *aseq_dir, int n_threads, int keep_line_no, int32_t shard_index, int32_t shard_count,
                                 ampli_host_cohort **out);
int32_t ampli_host_cohort_first_sample(const ampli_host_cohort *h);
int32_t ampli_host_cohort_total_samples(const ampli_host_cohort *h);
void ampli_host_cohort_free(ampli_host_cohort *h);
int64_t ampli_host_cohort_P(const ampli_host_cohort *h);
int64_t ampli_host_cohort_E(const ampli_host_cohort *h);
int32_t ampli_host_cohort_S(const ampli_host_cohort *h);
int64_t ampli_host_cohort_walk_len(const ampli_host_cohort *h);      /* BED-walk rows incl. repeated positions */
const int32_t *ampli_host_cohort_recs(const ampli_host_cohort *h);    /* [S][P+E][8] */
const uint32_t *ampli_host_cohort_dup_off(const ampli_host_cohort *h);/* [P+1] */
const uint32_t *ampli_host_cohort_ext_pos(const ampli_host_cohort *h);/* [E] */
const int32_t *ampli_host_cohort_line_no(const ampli_host_cohort *h); /* [S][P+E] or NULL */
/* lines whose RD column is not A+C+G+T: *n entries of four 32-bit words {sample, record slot, occurrence, RD column} */
const uint32_t *ampli_host_cohort_irregular(const ampli_host_cohort *h, int64_t *n);
const uint8_t *ampli_host_cohort_ref_code(const ampli_host_cohort *h);/* [P] */
const uint8_t *ampli_host_cohort_dup_flag(const ampli_host_cohort *h);/* [P] */
const char *ampli_host_cohort_sample_name(const ampli_host_cohort *h, int32_t s);
void ampli_host_cohort_stats(const ampli_host_cohort *h, int64_t *lines, int64_t *offpanel, int64_t *irregular, int64_t *malformed);
int ampli_host_position(const ampli_host_cohort *h, int64_t p, char *chrom_out, int chrom_cap, int32_t *coord);
/* sample names of the .ASEQ files of dir in visit order, newline separated; returns the count */
int ampli_host_sample_order(const char *dir, char *out, int64_t cap);

/* ---- the cohort as the command lines see it: a stream of chunks of consecutive samples, already in the device record
 * layout (what ampli_records of include/amplisolve_hip.h describes).  The callback gets one chunk at a time, in visit
 * order, while the next ones are being parsed; its pointers are valid until it returns.  layout: the narrowest the chunk's
 * counts fit -- AMPLI_RECORDS_U16 (every count <= 65534), AMPLI_RECORDS_U24 (<= 2^24 - 2) or AMPLI_RECORDS_I32; the
 * environment variable AMPLISOLVE_RECORDS = u16 | u24 | i32 sets the narrowest the packer may choose.  prim [n][P] records, ext [n][E] records (E, dup_off,
 * ext_pos are the CHUNK's own); line_prim / line_ext with keep_line_no; irregular: n_irregular x {sample in chunk, record
 * slot, occurrence, RD column} for lines with RD != A+C+G+T.  A negative strand count (reverse above total) or a count
 * beyond int32 ends the stream with AMPLI_E_RANGE.  Return non-zero from the callback to stop. */
typedef int (*ampli_host_chunk_fn)(void *user, int32_t first_sample, int32_t n_samples, int32_t layout, int64_t P, int64_t E,
                                   const void *prim, const void *ext, const uint32_t *dup_off, const uint32_t *ext_pos,
                                   const int32_t *line_prim, const int32_t *line_ext, const uint32_t *irregular, int64_t n_irregular);
int ampli_host_stream_chunks(const ampli_host_cohort *panel, const char *aseq_dir, int n_threads, int keep_line_no,
                             int64_t chunk_bytes, ampli_host_chunk_fn fn, void *user);

/* ---- the error table on disk (EE:2546-2944 writer, VC:430-576 reader) ---- */
int ampli_host_write_error_table(const ampli_host_cohort *h, const float *rate /*[2][4][P]*/, const uint8_t *code /*[4][P]*/,
                                 const float *germ_val /*[4][P]*/, const uint8_t *germ_present /*[4][P]*/, const char *path);
int ampli_host_read_error_table(const char *path, ampli_host_cohort **out, float *thr_out /*[2][4][P]*/, int64_t thr_capacity);
/* the same reader, also writing the by-product file storeInputFile writes (VC:437-441, 571: `chrom \t position \t. ...` per
 * data row, repeated rows included; dummy_vcf NULL or "" = none) */
int ampli_host_read_error_table_vcf(const char *path, const char *dummy_vcf, ampli_host_cohort **out, float *thr_out, int64_t thr_capacity);
/* a table read that way, cell by cell as the caller keeps it -- what storeInputFile puts into its four maps (VC:505-560;
 * the FIRST row of a repeated position wins): which = 0 reference cell (ReferenceBase_Hash), 1..4 threshold cell of A/C/G/T
 * (Thresholds_Hash_Analytic), 5..8 germ-max cell of A/C/G/T (Germline_Max_Hash).  NULL for a panel that did not come from a
 * table or an index out of range; the pointer lives as long as the cohort. */
const char *ampli_host_table_cell(const ampli_host_cohort *h, int64_t p, int32_t which);

/* ---- sequence context of a call (post-call annotation, VC:3307-3718): the 10 reference bases before and after position p
 * of the panel as find_kmer_down / find_kmer_up spell them (a position outside the panel is "-|", or a bare "-" at the
 * offsets -6, -3, -1 and +10) and homopolymerTest's flag for the substituted base `sub`.  down / up: caller's buffers of
 * cap bytes (a cell of a table can be up to 49 characters, so 10 of them need <= 512).  Returns the flag (0 / 1), < 0 on error. */
int ampli_host_context(const ampli_host_cohort *h, int64_t p, char sub, char *down, char *up, int32_t cap);

/* ---- the two command lines as functions (need libamplisolve_hip.so + a GPU) ---- */
int ampli_host_run_error_estimation(const char *panel_design, const char *reference_genome, const char *germline_dir,
                                    const char *C_value, const char *coverage_cutoff, const char *default_error,
                                    const char *output_dir, const char *refbases_file /* NULL: read the FASTA */);
int ampli_host_run_variant_calling(const char *error_file, const char *tumour_dir, const char *output_dir,
                                   const char *coverage_cutoff, const char *p_value);

/* ---- the same command lines as one shard of a multi-process (one process per GPU) run ----
 * Samples shard by contiguous ranges of the visit order (shard k of n takes what amplisolve_amd/dist.py::shard_range
 * gives it); every collective step is a callback, so the transport (torch.distributed over RCCL in
 * amplisolve_amd/multi.py; gloo in the tests) stays outside this library.  Device work is enqueued on the device's
 * default stream and the callbacks must be ordered with it.  Results are byte-identical to the one-process run.
 *   error estimation: position-sliced merge of include/amplisolve_hip.h -- ee_buffers is called once P is known and
 *   returns six DEVICE buffers sized by ampli_slice_bytes(P, count): [0] sums (zeroed), [1] gm, [2] sum_slice,
 *   [3] gm_recv, [4] block (zeroed), [5] blocks; ee_exchange = reduce-scatter SUM [0]->[2] + all-to-all [1]->[3];
 *   ee_gather = all-gather [4]->[5]; or_flags = bitwise OR of a host int over the shards.  Shard 0 writes the files.
 *   variant calling: tumour files are independent; rows_before = exclusive prefix sum of the emitted rows (the
 *   reference's Summary stream changes its float precision after the first row ever written, VC:1066); barrier; shard 0
 *   then assembles Summary_Variant_Info.txt from the shards' parts. */
typedef struct ampli_host_shard {
    int32_t index, count;
    void *user;
    int (*ee_buffers)(void *user, int64_t P, void **d_bufs /*[6]*/);
    int (*ee_exchange)(void *user);
    int (*ee_gather)(void *user);
    int (*or_flags)(void *user, int32_t *flags);
    int (*rows_before)(void *user, int64_t mine, int64_t *before);
    int (*barrier)(void *user);
} ampli_host_shard;
int ampli_host_run_error_estimation_sharded(const char *panel_design, const char *reference_genome, const char *germline_dir,
                                            const char *C_value, const char *coverage_cutoff, const char *default_error,
                                            const char *output_dir, const char *refbases_file, const ampli_host_shard *shard);
int ampli_host_run_variant_calling_sharded(const char *error_file, const char *tumour_dir, const char *output_dir,
                                           const char *coverage_cutoff, const char *p_value, const ampli_host_shard *shard);

/* ---- upstream of the two programs: BAM -> <out_dir>/<bam name without .bam>.PILEUP.ASEQ, i.e. computeCounts / ASEQ PILEUP mode
 * (/root/reference/Execution_examples.md:16-46: vcf= bam= threads= mbq= mrq= mdc= out=; the reference ships it as a binary without
 * source, so parity is unpinned -- DESIGN.md).  The host inflates the BGZF blocks (threads), the device decodes the alignment
 * records and counts (ampli_pileup_count); needs libamplisolve_hip.so + a GPU.  stats (optional) [4]: alignment records, reads
 * kept, bases counted, lines written. */
int ampli_host_compute_counts(const char *vcf, const char *bam, const char *out_dir, int32_t threads, int32_t mbq, int32_t mrq, int32_t mdc,
                              int64_t *stats);
/* computeIndelCounts: the same walk with ampli_pileup_indel_count per batch -> <out_dir>/<bam name>.INDEL.PILEUP.ASEQ (ref A,
 * A = reference junctions, C = insertions, G = deletions behind the position) and <out_dir>/<bam name>.INDEL.LENGTHS.txt, and, when refbases
 * is not NULL or empty, the `chrom pos A` table at that path.  A failure leaves no output file behind.  stats (optional) [4]: alignment
 * records, reads kept, junctions counted, lines written. */
int ampli_host_compute_indel_counts(const char *vcf, const char *bam, const char *out_dir, const char *refbases, int32_t threads, int32_t mbq,
                                    int32_t mrq, int32_t mdc, int64_t *stats);
/* computeAmpliconCounts: the same walk with ampli_pileup_amplicon_count per batch and one ampli_amplicon_layers behind it ->
 * <out_dir>/<bam name>.AMPLICON.PILEUP.ASEQ, .AMPLICON.READS.txt, .AMPLICON.OVERLAPS.txt and, when layers_dir is not NULL or empty (and differs
 * from out_dir), <layers_dir>/<bam name>.AMP1.PILEUP.ASEQ, .AMP2.PILEUP.ASEQ and <bam name>.pairs.txt.  bed: the panel's amplicons.  Bad numbers
 * (min_overlap outside 1 .. 100) and unreadable inputs are refused before the device is opened; a failure leaves no output file behind.
 * stats (optional) [6]: alignment records, reads kept, reads assigned, bases counted, bases clipped, lines written. */
int ampli_host_compute_amplicon_counts(const char *vcf, const char *bam, const char *bed, const char *out_dir, const char *layers_dir, int32_t threads,
                                       int32_t mbq, int32_t mrq, int32_t mdc, int32_t min_overlap, int64_t *stats);
/* The amplicons of a BED file as ampli_pileup_amplicon_count takes them (no GPU).  ref_names: the BAM header's reference names in
 * the order of their ids, separated by '\n'.  A row enters iff its chromosome is among them and 1 <= start <= end.  Sorted by lo, then hi (ties
 * in BED order): lo, hi, reach [cap], amp_off [cap + 1] (amp_off[A] = W), row_of [cap] (sorted index -> BED row, 0-based); *n_rows (optional): the
 * rows of the file.  Returns A >= 0, or a negative code: AMPLI_E_RANGE when A > cap or W >= 2^31, AMPLI_E_INVALID for a bad argument or file. */
int64_t ampli_host_amplicon_arrays(const char *bed, const char *ref_names, int64_t cap, uint64_t *lo, uint64_t *hi, uint64_t *reach, int64_t *amp_off,
                                   int32_t *row_of, int64_t *n_rows);
/* computeReadEvidence: the same walk with ampli_pileup_evidence per batch and one ampli_evidence_score over the listed lines ->
 * <out_dir>/<bam name>.EVIDENCE.txt (chr pos ref alt n_ref n_alt, per metric med_ref med_alt z, the verdict) and <out_dir>/<bam name>
 * .EVIDENCE.HIST.txt.  vcf: the calls (chr pos id ref alt; an alt of . takes the non-reference base with the most reads).  min_alt >= 1: the
 * reads either allele needs for a verdict; z_min > 0: the score from which a metric is flagged.  Bad numbers and unreadable inputs are refused
 * before the device is opened; a failure leaves no output file behind.  stats (optional) [4]: alignment records, reads kept, columns counted,
 * lines written. */
int ampli_host_compute_read_evidence(const char *vcf, const char *bam, const char *out_dir, int32_t threads, int32_t mbq, int32_t mrq, int32_t min_alt,
                                     double z_min, int64_t *stats);
/* ampli_evidence_score on the host (no GPU): the same planes -- hist int32 [P][4][3][64], ref_nt and alt_nt int8 [P] -- through the same
 * arithmetic (ampli_ev_* of csrc/ampli_math.h), so out_int [P][3][3], out_med [P][3][2], out_z2 [P][3] and alt_used [P] equal the device's bit
 * for bit.  Returns 0, or AMPLI_E_INVALID for a null pointer or P < 0. */
int ampli_host_evidence_score(const int32_t *hist, int64_t P, const int8_t *ref_nt, const int8_t *alt_nt, int64_t *out_int, int32_t *out_med,
                              double *out_z2, int8_t *alt_used);
/* computePhasing: the same walk with ampli_pileup_phase per batch and one ampli_phase_score over every formed pair of listed lines ->
 * <out_dir>/<bam name>.PHASE.txt (chr posA refA altA posB refB altB n_joint n_rr n_ra n_ar n_aa n_other exp_aa score verdict, one line per two
 * listed lines on one chromosome at most max_dist apart) and <out_dir>/<bam name>.PHASE.MNV.txt (chains of 2 or 3 consecutive positions that are
 * CIS in pairs).  vcf: the calls (chr pos id ref alt).  min_alt >= 1 and min_share in 0 .. 100: when a group of reads is present; q_min > 0: the
 * score CIS and NESTED_* need; max_dist >= 1.  Bad numbers and unreadable inputs are refused before the device is opened; a failure leaves no
 * output file behind.  stats (optional) [6]: alignment records, reads kept, reads covering at least two keys, cells incremented, pairs written,
 * chains written. */
int ampli_host_compute_phasing(const char *vcf, const char *bam, const char *out_dir, int32_t threads, int32_t mbq, int32_t mrq, int32_t min_alt,
                               int32_t min_share, double q_min, int32_t max_dist, int64_t *stats);
/* ampli_phase_score on the host (no GPU): the same table -- int32 [P][8][5][5] --, pair_cell int64 [Q] and pair_nt int8 [Q][4] through the same
 * arithmetic (ampli_ph_* of csrc/ampli_math.h): out_int [Q][6] and out_class [Q] equal the device's, out_score [Q] to the rounding of the two
 * math libraries.  Returns 0, or AMPLI_E_INVALID for a null pointer, P < 0, Q < 0, min_alt < 1 or min_share outside 0 .. 100. */
int ampli_host_phase_score(const int32_t *table, int64_t P, const int64_t *pair_cell, const int8_t *pair_nt, int64_t Q, int32_t min_alt, int32_t min_share,
                           int64_t *out_int, float *out_score, int32_t *out_class);
/* What computePhasing does behind its walk, from host arrays (no GPU): the pairs of the L listed lines (list: "chr \t pos \t ref \t alt \n" per
 * line; key_index [L]: each line's index into the table's keys, -1 for an unknown chromosome), ampli_host_phase_score over the formed ones, the
 * verdicts, the chains, and the two files <out_dir>/<name>.PHASE.txt and <name>.PHASE.MNV.txt.  stats (optional) [3]: pairs written, pairs
 * scored, chains written.  Returns 0 or a negative code. */
int ampli_host_phase_files(const char *list, const int64_t *key_index, int64_t L, const int32_t *table, int64_t P, int32_t min_alt, int32_t min_share,
                           double q_min, int64_t max_dist, const char *out_dir, const char *name, int64_t *stats);
/* the container only (no GPU): stats[4] = alignment records, uncompressed bytes, reference sequences, malformed records (complete
 * records whose CIGAR does not add up to their l_seq or whose fields overrun their block: counted and skipped).  Bytes behind the
 * last complete record -- a truncated or desynchronised stream -- are an error (AMPLI_E_INVALID), not a count: since round 3 the call
 * fails instead of reporting them in stats[3]. */
int ampli_host_bam_scan(const char *bam, int32_t threads, int64_t *stats);

/* the decision guard of the variant-calling command line for calls within 1e-6 of a gate (AMPLI_CALL_BORDERLINE): Q by the
 * reference's own operation sequence (VC:3834-3884: double kf_gammaq, long double log10); *ge5 / *lt20 = the comparisons of
 * VC:898 / VC:1023 made in long double */
double ampli_host_guard_score(int32_t k, int32_t rd, float err, int32_t *ge5, int32_t *lt20);

/* Detection limit of the calling gate for one strand, the literal definition: the smallest k in 1 .. bound with
 * Q(k, depth, thr) >= 5 in the reference's own operation sequence (as ampli_host_guard_score), scanning upwards from k = 1.
 * Returns -1 when thr == -1 (no estimate), 0 when no such k exists (also for depth <= 0).  Settles the cells ampli_limit_records
 * marks AMPLI_LIMIT_RECHECK. */
int32_t ampli_host_limit_reads(int32_t depth, float thr, int32_t bound);
/* the same count by the search the kernel runs (csrc/ampli_math.h: seeded walk and bracket check, fp64 with the host's libm), or -2
 * where that arithmetic does not decide (the kernel's RECHECK); *evals (optional) = scorer evaluations spent */
int32_t ampli_host_limit_search(int32_t depth, float thr, int32_t bound, int32_t *evals);

/* Detection power, the code of csrc/ampli_math.h that limit_power_kernel runs, compiled for the host.
 * ampli_host_binom_tail: P[Bin(n, v) >= k] in fp64; *terms (optional) = pmf terms formed (0: decided without a sum).
 * ampli_host_power_pair: one OK pair -- power[l] = tail(FW, min_fw, levels[l]) * tail(BW, min_bw, levels[l]) and, when lod is not NULL,
 * *lod = the allele fraction at which the power is `confidence` (*iters, optional: evaluations of the root search).  Returns 0, or
 * AMPLI_E_INVALID unless 1 <= min reads <= the strand's reads, n_levels in 0 .. 8 and confidence in [0.5, 0.99]. */
double ampli_host_binom_tail(int32_t n, int32_t k, double v, int32_t *terms);
int ampli_host_power_pair(int32_t FW, int32_t min_fw, int32_t BW, int32_t min_bw, const float *levels, int32_t n_levels, float confidence,
                          double *power, double *lod, int32_t *iters);

/* Panel dispersion: the finalize arithmetic of one cell (csrc/ampli_math.h, ampli_dispersion_cell -- what
 * dispersion_finalize_kernel runs) over `count` cells: n qualifying records, K alternative reads, D depth, X2 and sum 1/d -> z, phi
 * and the status (AMPLI_DISPERSION_OK / _FEW, AMPLI_DISPERSION_HIGH where z >= z_cutoff). */
void ampli_host_dispersion_cell_batch(const int32_t *n, const double *K, const double *D, const double *x2, const double *rinv, int64_t count,
                                      double z_cutoff, double *z, float *phi, uint8_t *status);

/* Sample identity: the genotype of `count` records (int32 [count][8], absent: field 0 == INT32_MIN) as the six plane bits
 * AMPLI_GENO_V | _A | _C | _G | _T | _H of include/amplisolve_types.h -- csrc/ampli_math.h's ampli_genotype_classify, what
 * genotype_planes_kernel runs.  Returns 0, or AMPLI_E_INVALID (-1) with nothing written when prm breaks its inequalities. */
int ampli_host_genotype_classify_batch(const int32_t *recs, int64_t count, const struct ampli_genotype_params *prm, uint8_t *bits);
/* the relation of a pair of samples from two of its counts: AMPLI_RELATION_UNDETERMINED when het_either < min_sites, else _SAME when
 * (double)het_match >= same_fraction * (double)het_either, else _DIFFERENT */
int ampli_host_concordance_relation(int32_t het_either, int32_t het_match, int32_t min_sites, double same_fraction);
/* Cross-sample contamination: fraction, its standard error and the background rate e of one ordered pair from its nine
 * sums (order AMPLI_CONTAM_* of include/amplisolve_types.h) -- csrc/ampli_math.h's ampli_contamination_estimate, in double, unfused.
 * fraction and se are NaN where the pair has no depth on an informative site; any of the three pointers may be NULL.  Returns
 * AMPLI_CONTAM_STATUS_UNDETERMINED when sites_hom + sites_het < min_sites, else _CONTAMINATED when fraction >= min_fraction, else
 * _CLEAN; AMPLI_E_INVALID (-1) when sums is NULL. */
int ampli_host_contamination_estimate(const int64_t *sums, int64_t min_sites, double min_fraction, double *fraction, double *se, double *background);
/* Amplicon copy ratio: csrc/ampli_math.h's functions, in double, unfused.  _median: the median of the m values of v that
 * are not NaN (signed values; v is not changed), NaN if there is none or v is NULL.  _z: mad > 0 ? ((ratio - 1.0) * med) / (1.4826 * mad)
 * : NaN.  _share: (double)d / (double)total.  _gene_status: AMPLI_GENE_GAIN / _LOSS / _NEUTRAL (include/amplisolve_types.h). */
double ampli_host_amplicon_median(const double *v, int64_t m);
/* the BED rows (with the amplicon id of column 4 and the gene of column 6, "." where missing) and the position index of a panel as text,
 * for tests: "R chrom start end name gene" per row, "W" + the walk, "D" + the dup flags, "P" + chrom:coord per position.  Returns the
 * bytes needed, the NUL included (the text is cut at cap - 1), or a negative AMPLI_E_* code. */
int64_t ampli_host_panel_describe(const char *bed_path, char *out, int64_t cap);
double ampli_host_amplicon_z(double ratio, double med, double mad);
double ampli_host_amplicon_share(int64_t d, int64_t total);
int ampli_host_amplicon_gene_status(int64_t n, double median_ratio, double median_z, int64_t min_amplicons, double gain_ratio, double loss_ratio,
                                    double z_cutoff);

/* Substitution spectrum (the definition is tests/spectrum_model.py): csrc/ampli_math.h's functions, integers and unfused doubles.
 * _enters_batch: the gate of `count` records (int32 [count][8], absent: field 0 == INT32_MIN) with their positions' reference codes and
 *   classes (uint8 [count] each) -- ampli_spectrum_enters, what spectrum_kernel runs -- as 0 / 1 in enters.  Returns 0, or
 *   AMPLI_E_INVALID (-1) with nothing written for a null pointer, count < 0, C outside [1, 128], a negative cut-off or max_alt_pm
 *   outside [0, 1000].
 * _class: 16 r + 4 l + t, 64 + r where a neighbour's code is not 0..3, 255 where r is not.
 * _fold: the sums of S samples, int64 [S][68][9] (the command line's classes), into alt and dep int64 [S][2][13] (strand, type; type 12
 *   is ALL), sites int64 [S][13] and the 96 channels ctx_alt, ctx_dep int64 [S][96] (both may be NULL).
 * _score: the reference from the first N samples (the normals) and the score of all S: ref double [13][4] = med, mad, med_a, mad_a;
 *   n_eff int32 [13]; status uint8 [13] (AMPLI_SPECTRUM_REF_*); rate2, ratio, z, asym, za double [S][13]; flag uint8 [S][13]
 *   (AMPLI_SPECTRUM_OK, _LOW_SITES, _NO_REFERENCE, _ELEVATED, _ASYMMETRIC of include/amplisolve_types.h).  Returns 0, or AMPLI_E_INVALID
 *   for a null pointer, S <= 0 or N outside [0, S]. */
int ampli_host_spectrum_enters_batch(const int32_t *recs, int64_t count, const uint8_t *ref_code, const uint8_t *cls, int32_t C, int32_t coverage_cutoff,
                                     int32_t max_alt_pm, uint8_t *enters);
int ampli_host_spectrum_class(int32_t r, int32_t l, int32_t t);
int ampli_host_spectrum_fold(const int64_t *sums, int64_t S, int64_t *alt, int64_t *dep, int64_t *sites, int64_t *ctx_alt, int64_t *ctx_dep);
int ampli_host_spectrum_score(const int64_t *alt, const int64_t *dep, const int64_t *sites, int64_t S, int64_t N, const ampli_spectrum_params *prm,
                              double *ref, int32_t *n_eff, uint8_t *status, double *rate2, double *ratio, double *z, double *asym, double *za,
                              uint8_t *flag);

/* Panel-of-normals exceedance (the definition is tests/exceedance_model.py): csrc/ampli_math.h's ampli_exceedance_candidate
 * on `count` cells, integers only.  x and depth uint64 [count][2]: the tumour's reads of the cell's base and its depth per strand
 * (forward, reverse); elig uint16 [count]: the eligible normals of the cell's (row, position); ge uint16 [count][2]: the cell's two
 * counts of ampli_exceedance_records.  A cell is a candidate (1 in candidate, else 0) iff neither count is AMPLI_EXCEEDANCE_NA (0xFFFF),
 * x[0] >= min_alt_reads and x[1] >= min_alt_reads, 1000 (x[0] + x[1]) >= min_vaf_pm (depth[0] + depth[1]), elig >= min_normals, and
 * ge[0] <= max_normals and ge[1] <= max_normals: the per-strand rule.  Returns 0, or AMPLI_E_INVALID (-1) with nothing written for a
 * null pointer, count < 0, a negative parameter or min_vaf_pm above 1000. */
int ampli_host_exceedance_candidate_batch(const uint64_t *x, const uint64_t *depth, const uint16_t *elig, const uint16_t *ge, int64_t count,
                                          const ampli_exceedance_params *prm, uint8_t *candidate);

/* Overdispersion-aware calling (the definition is tests/overdispersion_model.py): csrc/ampli_math.h's functions, in double,
 * unfused -- what overdispersion_finalize_kernel and nb_score_kernel run.
 * _overdispersion_cell_batch: omega of `count` cells from dispersion's status and X2, the cell's n, K, D and S2 = sum d_i^2:
 *   (X2 - (n - 1)) D / (K (D - S2 / D)) where the status carries AMPLI_DISPERSION_HIGH, D - S2 / D > 0 and the quotient is above 0,
 *   else 0.
 * _nb_score_batch: Q of n (k, d, e, omega) quadruples, omega == NULL meaning 0 everywhere: AMPLI_NB_NA (-1) for a negative, NaN or
 *   infinite omega, else -888 for e == -1, else 0 for k == 0, else with m = double(d) * double(e == 0 ? 0.0010008f : e) and p =
 *   P[X >= k] under the negative binomial of mean m and variance m + omega m^2 (the Poisson law at omega = 0): 0 for p >= 1, else
 *   (float)(-10 log10(max(p, 1e-10))).  The mathematical tail, not the reference's kf_gammaq; AMPLI_NB_NA too where the tail needs
 *   more than 2^20 terms (csrc/ampli_math.h says when).  Returns 0, or AMPLI_E_INVALID (-1) with nothing written for a null k, d, e
 *   or q or n < 1.
 * _nb_tail: p itself (a NaN beyond the term bound); *terms (optional) = pmf terms formed. */
void ampli_host_overdispersion_cell_batch(const uint8_t *status, const int32_t *n, const double *K, const double *D, const double *x2, const double *s2,
                                          int64_t count, double *omega);
int ampli_host_nb_score_batch(const int32_t *k, const int32_t *d, const float *e, const double *omega, int64_t n, float *q);
double ampli_host_nb_tail(double k, double m, double omega, int32_t *terms);

/* Paired comparison (the definition is tests/paired_model.py): csrc/ampli_math.h's functions, in double, unfused -- what
 * paired_score_kernel runs.
 * _pair_score_batch: the signed score S of n strand cells, file a with k_a alternative reads among d_a, file b with k_b among d_b.
 *   N = d_a + d_b, K = k_a + k_b, X hypergeometric (the alternative reads among a's d_a when K are dealt among N), c = k_a N - K d_a:
 *   +0 for K == 0 or c == 0; c > 0: +Q(P[X >= k_a]); c < 0: -Q(P[X <= k_a]); Q(p) = (float)(-10 log10(max(p, 1e-10))), +0 for
 *   p >= 1; -0 is never written.  AMPLI_PAIR_NA (-999) where the tail needs more than 2^20 terms (no int32 cell does).  Returns 0, or
 *   AMPLI_E_INVALID (-1) with nothing written for a null pointer, n < 1 or a cell outside 0 <= k <= d.
 * _hyper_tail: the tail itself, from k upwards (up != 0) or downwards, for 0 < n < N, 0 <= K <= N and k in the support on the far
 *   side of the mean from the direction's start (the sum runs away from the mean: a k on the near side gives 1); exactly 0 where the
 *   first term already bounds the tail below 1e-10; a NaN beyond the term bound or for arguments outside these; *terms (optional) = pmf
 *   terms formed. */
int ampli_host_pair_score_batch(const int32_t *k_a, const int32_t *d_a, const int32_t *k_b, const int32_t *d_b, int64_t n, float *s);
double ampli_host_hyper_tail(int64_t N, int64_t K, int64_t n, int64_t k, int32_t up, int32_t *terms);

/* False-discovery control (the definition is tests/fdr_model.py): what ampli_fdr_adjust computes, from the same text
 * (csrc/ampli_math.h: ampli_fdr_key, ampli_fdr_value, ampli_fdr_store) with std::sort in place of the device sort.
 * _fdr_rows: s float [rows][P][4][2]; a float [rows][P][4] (sign * A, +0, AMPLI_FDR_NA = -999 where untested), m int32 [rows] (the tested
 *   cells of each row), rank int32 [rows][P][4] or NULL (R, 0 where untested or a = 0).  Each row on its own.  Returns 0,
 *   AMPLI_E_INVALID (-1) for a null pointer, rows < 1, P <= 0 or two_sided not 0 or 1, AMPLI_E_RANGE (-6) for 4 P >= 2^31. */
int ampli_host_fdr_rows(const float *s, int32_t rows, int64_t P, int32_t two_sided, float *a, int32_t *m, int32_t *rank);

/* In-silico dilution (the definition is tests/dilution_model.py): csrc/ampli_math.h's functions, the text dilute_kernel runs,
 * so that every integer is pinned without a GPU.  The definition in full stands in include/amplisolve_hip.h (ampli_dilute_records).
 * _philox4x32_10: Philox4x32-10 of counter ctr[4] and key key[2] into out[4].
 * _thin: Thin(n, keep; key, p, field, side) = #{ i < n : word_i < keep }, word_i = output word (i & 3) of Philox with counter
 *   (i >> 2, p, field | side << 3, 0) and key (low word, high word); -1 for n < 0, keep above 2^32, field outside 0..7 or side outside 0..1.
 * _dilute_keep: (uint64) floor(ldexp(x, 32) + 0.5); x outside [0, 1] (a NaN included) gives UINT64_MAX, which every entry refuses.
 * _dilute_records: ampli_dilute_records over int32 records on the host.  recs_a int32 [n_a][stride_a][8] and recs_b (NULL with n_b = 0
 *   when there is no chunk b) [n_b][stride_b][8], strides in records (0 = P), of which the first P records of a row enter; mix [n_mix];
 *   out int32 [n_mix][P][8] and flags int32 [n_mix], both fully overwritten.  Returns 0, or AMPLI_E_INVALID (-1) with nothing written
 *   for a null pointer other than recs_b, P <= 0, n_mix < 1, n_a < 1, n_b < 0, a stride below P, AMPLI_E_RANGE (-6) for P >= 2^31. */
void ampli_host_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out);
int64_t ampli_host_thin(int64_t n, uint64_t keep, uint64_t key, uint32_t p, int32_t field, int32_t side);
uint64_t ampli_host_dilute_keep(double x);
int ampli_host_dilute_records(const int32_t *recs_a, int32_t n_a, int64_t stride_a, const int32_t *recs_b, int32_t n_b, int64_t stride_b, int64_t P,
                              const ampli_dilute_mix *mix, int32_t n_mix, int32_t *out, int32_t *flags);

/* Tumour-informed monitoring (the definition is tests/monitor_model.py): csrc/ampli_math.h's functions in the order of the
 * definition, so that every integer, every double and every score is pinned without a GPU.  The definition in full stands in
 * include/amplisolve_hip.h (ampli_monitor_sums_records).
 * _monitor_sums, _monitor_controls, _monitor_score: the three device entry points over int32 records on the host.  recs int32
 *   [n][stride][8], stride in records (0 = P), of which the first P records of a row enter; the other arrays as on the device.  The
 *   outputs are fully overwritten.  Returns 0, or AMPLI_E_INVALID (-1) / AMPLI_E_RANGE (-6) with nothing written where the device
 *   entry point refuses.
 * _monitor_control_draw: the index among m candidates that entry i of list l takes in replicate r: (uint64(word) * m) >> 32, word =
 *   output word 0 of Philox4x32-10 with counter (i, r, l, AMPLI_MON_CONTROL_TAG) and key (low word, high word of seed).
 * _monitor_verdict: AMPLI_MON_NOT_EVALUABLE if n_eval < min_variants; else AMPLI_MON_DETECTED iff n_seen >= min_seen and q_fw >= q_min
 *   and q_bw >= q_min (the float scores widened to double); else AMPLI_MON_NOT_DETECTED.
 * _monitor_excess: the pooled excess fraction of a strand, max(0, ((double)K - Lambda) / (double)D); 0 for D <= 0.
 * _monitor_count_ge: n_ge = the controls r < R whose min(ctl_q[r][0], ctl_q[r][1]) >= min(obs_fw, obs_bw); -1 for a null pointer or R < 0.
 * _monitor_empirical_p: (1 + n_ge) / (R + 1).
 * _monitor_lod_reads: the smallest K >= floor(Lambda) + 1 whose pooled score reaches q_min, walking upwards one count at a time for at
 *   most AMPLI_MON_LOD_MAX_EVALS evaluations; 0 where none is found within them, q_min is above 100 or Lambda is outside [0, 2^52);
 *   *evals (optional) = evaluations made.
 * _monitor_lod: the pooled limit of detection, the larger of the strands' (K_min - Lambda) / D; -1 where a strand has no K_min or D <= 0. */
int ampli_host_monitor_sums(const int32_t *recs, int32_t n, int64_t stride, int64_t P, const float *thr, const uint8_t *ref_code, const uint32_t *list_off,
                            const uint32_t *list_cell, int32_t L, int64_t W, const ampli_monitor_params *prm, int64_t *sums, double *lambda);
int ampli_host_monitor_controls(const int32_t *recs, int32_t n, int64_t stride, int64_t P, const float *thr, const uint8_t *ref_code,
                                const uint32_t *list_off, const uint32_t *list_cell, int32_t L, int64_t W, const int32_t *pairs, int32_t n_pairs,
                                const uint32_t *cand_off, const uint32_t *cand_pos, int64_t n_cand, int32_t R, int32_t first_rep, uint64_t seed,
                                const ampli_monitor_params *prm, int64_t *sums, double *lambda);
int ampli_host_monitor_score(const int64_t *sums, const double *lambda, int64_t n_cells, float *q);
uint32_t ampli_host_monitor_control_draw(uint32_t i, uint32_t r, uint32_t l, uint64_t seed, uint32_t m);
int ampli_host_monitor_verdict(int64_t n_eval, int64_t n_seen, float q_fw, float q_bw, int64_t min_variants, int64_t min_seen, double q_min);
double ampli_host_monitor_excess(int64_t K, double lam, int64_t D);
int64_t ampli_host_monitor_count_ge(float obs_fw, float obs_bw, const float *ctl_q, int64_t R);
double ampli_host_monitor_empirical_p(int64_t n_ge, int64_t R);
int64_t ampli_host_monitor_lod_reads(double lam, double q_min, int32_t *evals);
double ampli_host_monitor_lod(double lam_fw, double lam_bw, int64_t D_fw, int64_t D_bw, double q_min);

/* Allelic imbalance at germline het sites (the definition is tests/allelic_model.py, in full in include/amplisolve_hip.h):
 * csrc/ampli_math.h's functions, so that every status, share and score is pinned without a GPU.
 * _allelic_site_batch: the site stage for n cells given apart: pair (the germline's pair code 0..5, anything else: not het), present,
 *   the reads k_lo and k_hi of the pair's two bases, and the reference's CNT, LO and HI of (pair, position).  q, km [n][2], v and code
 *   as ampli_allelic_site_records stores them; terms (optional) = pmf terms formed per cell.  Returns 0, or -1 with nothing written
 *   for a null pointer, n < 0 or parameters the device entry point refuses.
 * _allelic_pair: the pair code of six plane bits (V, A, C, G, T, H = bits 0..5), -1 where the bits are not a het site.
 * _allelic_site_sums: what a tested cell adds to DEV16 and Q20 of a region.
 * _allelic_region_verdict: AMPLI_AI_FEW if SITES < max(min_sites, 1); else X = (ln 10 / 5) (Q20 / 2^20), p = kf_gammaq(SITES, X / 2)
 *   (Fisher's combination: chi-square with 2 SITES degrees of freedom), *Q = 0 for p >= 1, -10 log10(p) for p > 1e-30, else 300;
 *   *imbalance = DEV16 / (16 DEPTH); AMPLI_AI_IMBALANCED iff *Q >= q_min and *imbalance >= min_imbalance, else AMPLI_AI_BALANCED.  *Q is
 *   NaN for FEW, *imbalance NaN where DEPTH is 0.  -1 for a null pointer. */
int ampli_host_allelic_site_batch(int64_t n, const int32_t *pair, const uint8_t *present, const int64_t *k_lo, const int64_t *k_hi, const int64_t *cnt,
                                  const int64_t *lo, const int64_t *hi, const ampli_allelic_params *prm, float *q, int32_t *km, double *v, uint8_t *code,
                                  int32_t *terms);
int ampli_host_allelic_pair(uint32_t plane_bits);
int ampli_host_allelic_site_sums(float q, int32_t k_lo, int32_t m, double v, int64_t *dev16, int64_t *q20);
int ampli_host_allelic_region_verdict(const int64_t *sums /* [5] */, int64_t min_sites, double q_min, double min_imbalance, double *Q, double *imbalance);

/* Tumour fraction per (sample, list) (the definition is tests/fraction_model.py, in full in include/amplisolve_hip.h):
 * csrc/ampli_math.h's functions in the order of the definition, so that every double is pinned without a GPU.
 * _fraction: the device entry point over int32 records on the host.  recs int32 [n][stride][8], stride in records (0 = P), of which
 *   the first P records of a row enter; the other arrays as on the device.  est [n][L][AMPLI_TF_VALS] and count [n][L][AMPLI_TF_COUNTS]
 *   are fully overwritten.  Returns 0, or AMPLI_E_INVALID (-1) / AMPLI_E_RANGE (-6) with nothing written where the device entry point
 *   refuses.
 * _fraction_verdict: AMPLI_TF_NOT_EVALUABLE if n_eval < min_variants or the values are AMPLI_TF_NA (f_hat < 0); else AMPLI_TF_QUANTIFIED if
 *   f_lo > 0; else AMPLI_TF_BELOW, and F_HI is the reportable upper bound.
 * _fraction_change: from draw A to draw B of one list, a and b the draws' four values: AMPLI_TF_CHANGE_NOT_EVALUABLE if either verdict is
 *   AMPLI_TF_NOT_EVALUABLE; else AMPLI_TF_RISING if F_LO_B > F_HI_A; else AMPLI_TF_FALLING if F_HI_B < F_LO_A; else AMPLI_TF_STABLE.
 *   *ratio = F_HAT_B / F_HAT_A, AMPLI_TF_NA where either draw is not evaluable or F_HAT_A is 0.  -1 for a null pointer. */
int ampli_host_fraction(const int32_t *recs, int32_t n, int64_t stride, int64_t P, const float *thr, const uint8_t *ref_code, const uint32_t *list_off,
                        const uint32_t *list_cell, const float *list_w, int32_t L, int64_t W, const ampli_fraction_params *prm, double *est, int64_t *count);
int ampli_host_fraction_verdict(int64_t n_eval, double f_hat, double f_lo, int64_t min_variants);
int ampli_host_fraction_change(int32_t verdict_a, const double *a /* [4] */, int32_t verdict_b, const double *b /* [4] */, double *ratio);

/* two-sided Fisher exact test of the post-call annotation (VC:3797-3814; own pmf, parity unpinned vs Boost) */
double ampli_host_fisher(int a, int b, int c, int d);
/* the same sum with every term taken from the log-gamma form (slow; the check of the recurrence ampli_host_fisher walks) */
double ampli_host_fisher_direct(int a, int b, int c, int d);

#ifdef __cplusplus
}
#endif
#endif
