/*
 * include/amplisolve_types.h -- the constants and plain structs that more than one of include/amplisolve_hip.h (the kernels' C ABI),
 * include/amplisolve_host.h (the host library's C ABI) and amplisolve_amd/csrc/ampli_math.h (the scalar arithmetic that the kernels
 * and the host library both compile) needs.  Each is defined here and nowhere else; all three include this header.  Plain C, no
 * functions, nothing but <stddef.h> and <stdint.h>.  What a value means in full stands with the entry point that takes or writes it,
 * in include/amplisolve_hip.h; DESIGN n names the section of DESIGN.md.
 */
#ifndef AMPLISOLVE_TYPES_H
#define AMPLISOLVE_TYPES_H

#include <stddef.h>
#include <stdint.h>

/* The calling gate (ampli_poisson_call, ampli_limit_records): a score within this distance of the gate Q >= 5 is not decided by the
 * device's arithmetic but handed to the host (AMPLI_CALL_BORDERLINE, AMPLI_LIMIT_RECHECK). */
#define AMPLI_CALL_GATE_EPS 1e-6

/* Panel dispersion: the status of a cell, OK or FEW in bits 0-2, HIGH where the cell is OK and z >= z_cutoff. */
#define AMPLI_DISPERSION_OK 0
#define AMPLI_DISPERSION_FEW 1
#define AMPLI_DISPERSION_HIGH 0x40

/* Sample identity: the per-mille bounds of the genotype classes -- min_depth >= 1 and 0 <= absent_max_pm < het_min_pm <=
 * het_max_pm < hom_min_pm <= 1000 --, the six plane bits of a (sample, position) -- bit k is plane k of uint64 planes[sample][6][W] --
 * and the relation of a pair of samples. */
typedef struct ampli_genotype_params {
    int32_t min_depth, absent_max_pm, het_min_pm, het_max_pm, hom_min_pm;
} ampli_genotype_params;
#define AMPLI_GENO_V 1
#define AMPLI_GENO_A 2
#define AMPLI_GENO_C 4
#define AMPLI_GENO_G 8
#define AMPLI_GENO_T 16
#define AMPLI_GENO_H 32
#define AMPLI_GENO_PLANES 6
#define AMPLI_RELATION_UNDETERMINED 0
#define AMPLI_RELATION_SAME 1
#define AMPLI_RELATION_DIFFERENT 2

/* Cross-sample contamination: the order of the nine int64 sums of an ordered pair, and the pair's status. */
#define AMPLI_CONTAM_SITES_HOM 0
#define AMPLI_CONTAM_ALT_HOM 1
#define AMPLI_CONTAM_DEPTH_HOM 2
#define AMPLI_CONTAM_SITES_HET 3
#define AMPLI_CONTAM_ALT_HET 4
#define AMPLI_CONTAM_DEPTH_HET 5
#define AMPLI_CONTAM_SITES_BG 6
#define AMPLI_CONTAM_ALT_BG 7
#define AMPLI_CONTAM_DEPTH_BG 8
#define AMPLI_CONTAM_SUMS 9
#define AMPLI_CONTAM_STATUS_UNDETERMINED 0
#define AMPLI_CONTAM_STATUS_CLEAN 1
#define AMPLI_CONTAM_STATUS_CONTAMINATED 2

/* Amplicon coverage and copy ratio: the order of the four int64 sums of a (sample, amplicon), the status of an amplicon
 * of the reference, the launch bounds, and the status of a gene. */
#define AMPLI_AMP_PRESENT 0
#define AMPLI_AMP_DEPTH_FW 1
#define AMPLI_AMP_DEPTH_BW 2
#define AMPLI_AMP_CALLABLE 3
#define AMPLI_AMP_SUMS 4
#define AMPLI_AMPLICON_OK 0
#define AMPLI_AMPLICON_FEW 1
#define AMPLI_AMPLICON_DARK 2
#define AMPLI_AMPLICON_MAX 4096 /* N of amplicon_reference, A of amplicon_ratio: 32 KB of LDS */
#define AMPLI_AMPLICON_STRIP 8  /* rows per wave of amplicon_depth_kernel */
#define AMPLI_GENE_NEUTRAL 0
#define AMPLI_GENE_GAIN 1
#define AMPLI_GENE_LOSS 2

/* Substitution spectrum: the order of the nine int64 sums of a (sample, class), the class axis, the folded types and
 * channels, the flag of a (sample, type), the status of a type's reference, and the parameters of the score. */
#define AMPLI_SPEC_SITES 0
#define AMPLI_SPEC_FW_A 1
#define AMPLI_SPEC_FW_C 2
#define AMPLI_SPEC_FW_G 3
#define AMPLI_SPEC_FW_T 4
#define AMPLI_SPEC_BW_A 5
#define AMPLI_SPEC_BW_C 6
#define AMPLI_SPEC_BW_G 7
#define AMPLI_SPEC_BW_T 8
#define AMPLI_SPEC_SUMS 9
#define AMPLI_SPECTRUM_MAX_CLASSES 128
#define AMPLI_SPECTRUM_STRIP 4    /* rows per workgroup of spectrum_kernel */
#define AMPLI_SPECTRUM_SKIP 255
#define AMPLI_SPECTRUM_CLASSES 68 /* the command line's classes: 64 trinucleotide contexts and 4 edge classes */
#define AMPLI_SPECTRUM_TYPES 13   /* twelve strand-resolved substitution types and ALL */
#define AMPLI_SPECTRUM_ALL 12
#define AMPLI_SPECTRUM_CHANNELS 96
#define AMPLI_SPECTRUM_OK 0
#define AMPLI_SPECTRUM_LOW_SITES 1
#define AMPLI_SPECTRUM_NO_REFERENCE 2
#define AMPLI_SPECTRUM_ELEVATED 3
#define AMPLI_SPECTRUM_ASYMMETRIC 4
#define AMPLI_SPECTRUM_REF_OK 0
#define AMPLI_SPECTRUM_REF_FEW 1
typedef struct ampli_spectrum_params {
    int64_t min_sites, min_normals;
    double excess_ratio, z_cutoff, asym_delta;
} ampli_spectrum_params;

/* Panel-of-normals exceedance: the sentinel of a cell that is not evaluated, the bound that keeps a count below it, the
 * launch shape, and the candidate rule's parameters (every count >= 0, min_vaf_pm at most 1000). */
#define AMPLI_EXCEEDANCE_NA 0xFFFF
#define AMPLI_EXCEEDANCE_MAX_NORMALS 65534
#define AMPLI_EXCEEDANCE_STRIP 8 /* normal rows decoded into LDS at a time */
#define AMPLI_EXCEEDANCE_ROWS 8  /* tumour rows per workgroup of exceedance_kernel */
typedef struct ampli_exceedance_params {
    int64_t min_alt_reads, min_vaf_pm, min_normals, max_normals;
} ampli_exceedance_params;

/* The score planes' sentinels of a cell that is not evaluated or not tested: the negative-binomial score, the paired
 * comparison, the adjusted score of false-discovery control. */
#define AMPLI_NB_NA (-1.0f)
#define AMPLI_PAIR_NA (-999.0f)
#define AMPLI_FDR_NA (-999.0f)

/* In-silico dilution: one mixture -- out = Thin(row_a, keep_a) + Thin(row_b, keep_b), row_b == -1 for pure down-sampling,
 * a keep in [0, 2^32] -- the flag bits of a mixture, and the largest count an input record may hold.  The layout is the one the
 * kernel, the host library and the bindings share. */
typedef struct ampli_dilute_mix {
    int32_t row_a, row_b;
    uint64_t keep_a, keep_b, key;
} ampli_dilute_mix;
#define AMPLI_DILUTE_BAD_COUNT 1
#define AMPLI_DILUTE_BAD_MIXTURE 2
#define AMPLI_DILUTE_MAX_COUNT 16777214 /* 2^24 - 2 */
#ifdef __cplusplus
static_assert(sizeof(ampli_dilute_mix) == 32 && offsetof(ampli_dilute_mix, row_a) == 0 && offsetof(ampli_dilute_mix, row_b) == 4 &&
                  offsetof(ampli_dilute_mix, keep_a) == 8 && offsetof(ampli_dilute_mix, keep_b) == 16 && offsetof(ampli_dilute_mix, key) == 24,
              "ampli_dilute_mix is {int32 row_a; int32 row_b; uint64 keep_a; uint64 keep_b; uint64 key}, 32 bytes");
static_assert(AMPLI_DILUTE_BAD_COUNT == 1 && AMPLI_DILUTE_BAD_MIXTURE == 2 && AMPLI_DILUTE_MAX_COUNT == (1 << 24) - 2, "the flag bits and the count range");
#endif

/* Tumour-informed monitoring: the order of the six int64 sums of a (sample, list), the score of a cell without an evaluated
 * entry (outside [0, 100]; a tail that is not computable within its term bound gets it too), the verdict of a (sample, list), the rows
 * a wave of monitor_sums_kernel owns, the tag in the fourth counter word of a control draw, the bound of the limit-of-detection walk,
 * and the gates of an evaluated entry (coverage_cutoff >= 0, 0 <= max_vaf_pm <= 1000; 1000 switches the allele-fraction gate off). */
#define AMPLI_MON_N_EVAL 0
#define AMPLI_MON_N_SEEN 1
#define AMPLI_MON_K_FW 2
#define AMPLI_MON_K_BW 3
#define AMPLI_MON_D_FW 4
#define AMPLI_MON_D_BW 5
#define AMPLI_MON_SUMS 6
#define AMPLI_MON_NA (-1.0f)
#define AMPLI_MON_NOT_EVALUABLE 0
#define AMPLI_MON_NOT_DETECTED 1
#define AMPLI_MON_DETECTED 2
#define AMPLI_MON_STRIP 8
#define AMPLI_MON_CONTROL_TAG 0x4D4F4E31u /* "MON1" */
#define AMPLI_MON_LOD_MAX_EVALS 4096
typedef struct ampli_monitor_params {
    int32_t coverage_cutoff, max_vaf_pm;
} ampli_monitor_params;

/* Allelic imbalance at germline het sites: the three int64 planes of the het-site reference [3][6][P], the status of a
 * (sample, position) -- stored as status * 8 + pair code, the pair code 7 where there is none --, the score of a cell that is not
 * tested (a tail that is not computable within its term bound gets it too), the order of the five int64 sums of a (sample, region),
 * the rows a wave of allelic_region_kernel owns, the verdict of a region, and the parameters of the site stage (min_depth >= 1,
 * min_normals >= 1, half_fallback 0 / 1). */
#define AMPLI_AI_REF_CNT 0
#define AMPLI_AI_REF_LO 1
#define AMPLI_AI_REF_HI 2
#define AMPLI_AI_REF_PLANES 3
#define AMPLI_AI_PAIRS 6
#define AMPLI_AI_NO_PAIR 7
#define AMPLI_AI_NOT_HET 0
#define AMPLI_AI_ABSENT 1
#define AMPLI_AI_SHALLOW 2
#define AMPLI_AI_DEEP 3
#define AMPLI_AI_NO_REFERENCE 4
#define AMPLI_AI_TESTED_REF 5
#define AMPLI_AI_TESTED_HALF 6
#define AMPLI_AI_NA (-999.0f)
#define AMPLI_AI_SITES 0
#define AMPLI_AI_SIG 1
#define AMPLI_AI_DEPTH 2
#define AMPLI_AI_DEV16 3
#define AMPLI_AI_Q20 4
#define AMPLI_AI_SUMS 5
#define AMPLI_AI_STRIP 8
#define AMPLI_AI_FEW 0
#define AMPLI_AI_BALANCED 1
#define AMPLI_AI_IMBALANCED 2
typedef struct ampli_allelic_params {
    int32_t min_depth, min_normals, half_fallback;
} ampli_allelic_params;

/* Tumour fraction per (sample, list): the order of the four doubles of a (sample, list) -- the score estimate, the two ends of
 * its Rao score interval and the signed squared score at zero --, the order of the two int64 counts, the value of all four doubles where
 * nothing can be estimated, the steps of every bisection, the verdict of a (sample, list), the change between two draws of one list, and
 * the parameters: the gates of an evaluated entry as ampli_monitor_params has them, and z2, the squared normal quantile of the interval
 * (finite and > 0; AMPLI_TF_Z2_95 is the default). */
#define AMPLI_TF_F_HAT 0
#define AMPLI_TF_F_LO 1
#define AMPLI_TF_F_HI 2
#define AMPLI_TF_T0 3
#define AMPLI_TF_VALS 4
#define AMPLI_TF_N_EVAL 0
#define AMPLI_TF_N_SEEN 1
#define AMPLI_TF_COUNTS 2
#define AMPLI_TF_NA (-1.0)
#define AMPLI_TF_ITERS 60
#define AMPLI_TF_Z2_90 2.705543
#define AMPLI_TF_Z2_95 3.841459
#define AMPLI_TF_Z2_99 6.634897
#define AMPLI_TF_NOT_EVALUABLE 0
#define AMPLI_TF_BELOW 1
#define AMPLI_TF_QUANTIFIED 2
#define AMPLI_TF_CHANGE_NOT_EVALUABLE 0
#define AMPLI_TF_STABLE 1
#define AMPLI_TF_RISING 2
#define AMPLI_TF_FALLING 3
typedef struct ampli_fraction_params {
    int32_t coverage_cutoff, max_vaf_pm;
    double z2;
} ampli_fraction_params;

/* Indel counting from alignments: the length bins per (position, kind) of ampli_pileup_indel_count's second output, kind 0 =
 * insertion, kind 1 = deletion; an event of length L falls into bin min(L, AMPLI_INDEL_LEN_BINS) - 1, so the last bin holds L >= 32. */
#define AMPLI_INDEL_LEN_BINS 32

/* Read-level evidence from alignments: ampli_pileup_evidence's histograms are int32 [P][4][AMPLI_EVIDENCE_METRICS]
 * [AMPLI_EVIDENCE_BINS] in the order (position, nt, metric, bin); the metrics are the base quality of the counted column, the MAPQ of its
 * read (in steps of 4) and the column's distance to the nearer end of the stored sequence, each clamped into the last bin. */
#define AMPLI_EVIDENCE_METRICS 3
#define AMPLI_EVIDENCE_BINS 64
#define AMPLI_EVIDENCE_BQ 0
#define AMPLI_EVIDENCE_MQ 1
#define AMPLI_EVIDENCE_POS 2

/* Read-level phasing from alignments: ampli_pileup_phase's joint table is int32 [P][AMPLI_PHASE_PARTNERS][AMPLI_PHASE_STATES]
 * [AMPLI_PHASE_STATES] in the order (key i, partner k, state at key i, state at key i + 1 + k): a key is paired with the next
 * AMPLI_PHASE_PARTNERS listed keys; a read's state at a key it covers is 0 .. 3 = A C G T for a counted column and AMPLI_PHASE_OTHER for
 * everything else (a base below mbq, a non-ACGT base, a key inside a deletion or a reference skip). */
#define AMPLI_PHASE_PARTNERS 8
#define AMPLI_PHASE_STATES 5
#define AMPLI_PHASE_OTHER 4

#endif /* AMPLISOLVE_TYPES_H */
