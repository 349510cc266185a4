// amplisolve_amd/csrc/host/host.hpp -- C++ host side of the two AmpliSolve command lines.
//
// Parsers, panel index, SoA packer, table reader/writer, annotation and the
// pipelines that call libamplisolve_hip.so.  No arithmetic of the hot path
// lives here.  EE:n / VC:n cite /root/reference/source_codes/AmpliSolve{ErrorEstimation,VariantCalling}.cpp.
#pragma once
#include <cstdint>
#include <iosfwd>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/amplisolve_hip.h"
#include "../../../include/amplisolve_host.h"

namespace ampli {

struct BedRow {
    std::string chrom;
    int start = -1, end = -1;
    std::string name = ".", gene = "."; // columns 4 and 6 (the amplicon's id and its gene); "." where the row has no such column
};

// The panel: unique positions in order of first appearance in the BED walk
// (rows in file order, start..end inclusive, 1-based: EE:633-649, EE:2595-2606).
struct Panel {
    std::vector<BedRow> rows;
    std::vector<std::string> chroms;                  // chrom id -> name
    std::unordered_map<std::string, int> chrom_id;    // name -> id
    std::vector<int32_t> pos_chrom, pos_coord;        // per unique position p
    std::vector<uint32_t> walk;                       // BED walk (duplicates repeated) -> p
    std::unordered_map<uint64_t, uint32_t> index;     // (chrom id << 32 | coord) -> p
    std::vector<std::string> ref_base;                // per p, as read (case preserved)
    std::vector<uint8_t> ref_code;                    // 0..3 = A,C,G,T (exact, upper case), 255 otherwise
    std::vector<uint8_t> dup;                         // per p: listed more than once (EE:657-664)
    // error-table columns, when the panel was loaded from positionSpecificNoise_*.txt (VC:430-576): the file's text with
    // every cell NUL-terminated in place, and per unique position the offsets of its 4 threshold + 4 germ-max cells
    std::string table_text;
    std::vector<uint32_t> cell_off[8];
    bool from_table() const { return !cell_off[0].empty() || (!table_text.empty() && pos_coord.empty()); }
    const char *thr_cell(int nt, int64_t p) const { return table_text.data() + cell_off[nt][(size_t)p]; }      // Thresholds_Hash_Analytic (VC:519-538)
    const char *germ_cell(int nt, int64_t p) const { return table_text.data() + cell_off[4 + nt][(size_t)p]; } // Germline_Max_Hash (VC:541-560)

    int64_t P() const { return (int64_t)pos_coord.size(); }
    int find(const std::string &chrom, int coord) const;
    int add_position(const std::string &chrom, int coord);
    int add_position_id(int chrom_id_, int coord); // the chromosome is already in `chroms`
    void set_ref(uint32_t p, const std::string &base);
};

// A line whose RD column differs from A+C+G+T (EE:1178-1181, VC:762-765).  The reference keeps using the column:
// as the denominator of the Germ_Max AF (EE:1229-1232) and, in the caller, as RD in AF = X/RD and in the forward depth
// RD - RD_reverse of the Poisson test (VC:814-817, VC:895).  Sparse side list next to the dense records.
struct Irregular {
    uint32_t sample;     // sample index inside the cohort / chunk
    uint32_t record;     // record slot in [0, P+E)
    uint32_t occurrence; // which line of that position in the file (0 = the primary record)
    int32_t rd;          // the RD column
};

// A directory of .PILEUP.ASEQ files packed into the record SoA of include/amplisolve_hip.h
struct Cohort {
    std::vector<std::string> paths;   // in visit order (EE:1081 / VC:672)
    std::vector<std::string> names;   // sample names (EE:831)
    int64_t P = 0, E = 0;
    int32_t *recs = nullptr;          // [S][P+E][8], pinned when the HIP library is loaded
    bool pinned = false;
    std::vector<uint32_t> dup_off;    // [P+1]
    std::vector<uint32_t> ext_pos;    // [E]
    std::vector<int32_t> line_no;     // [S][P+E] data-line index inside the sample's file, -1 absent
    std::vector<Irregular> irregular; // lines with RD != A+C+G+T
    int64_t n_lines = 0, n_offpanel = 0, n_irregular = 0, n_malformed = 0;
    int first_sample = 0, total_samples = 0; // this cohort = samples [first_sample, first_sample + S()) of the directory's visit order
    ~Cohort();
    int S() const { return (int)paths.size(); }
    int64_t R() const { return P + E; }
};

struct Error {
    int code;
    std::string msg;
};

// One upload unit of a streamed cohort: consecutive samples of the visit order, records already in the layout the
// kernels read (24-byte records; int32 when a count of the chunk needs it), extras in their own array with the
// chunk's own slot layout (ampli_records of include/amplisolve_hip.h describes exactly this).
struct Chunk {
    int slot = 0, index = 0;       // ring slot; chunk number
    int first = 0, n = 0;          // samples [first, first + n) of the stream's file list
    bool last = false;
    int layout = AMPLI_RECORDS_U24;
    int64_t P = 0, E = 0;
    void *prim = nullptr;          // [n][P] records; page-aligned host memory the parsers fill BEFORE the HIP runtime is up,
    size_t prim_cap = 0;           // pinned late (pin(): hipHostRegister) by the consumer once there is a context
    bool prim_pinned = false;
    void *ext = nullptr;           // [n][E] records
    size_t ext_cap = 0;
    bool ext_pinned = false;
    void pin(ampli_ctx *ctx);      // register prim / ext with the runtime if they are not yet (no-op without the HIP library)
    std::vector<uint32_t> dup_off; // [P+1]
    std::vector<uint32_t> ext_pos; // [E]
    std::vector<int32_t> line_prim, line_ext; // [n][P], [n][E] data-line index inside the sample's file (-1 absent); variant calling only
    std::vector<Irregular> irregular;
    int64_t n_lines = 0, n_offpanel = 0, n_irregular = 0, n_malformed = 0;
    Chunk() = default;
    Chunk(const Chunk &) = delete;
    Chunk &operator=(const Chunk &) = delete;
    ~Chunk();
};

// The cohort as a stream of chunks: a producer thread (with n_threads parser workers) fills a small ring of page-aligned
// buffers ahead of the consumer (they need no HIP call, so parsing starts while the runtime is still coming up; the
// consumer pins a buffer the first time it uploads from it), so parsing of chunk k+1 overlaps the upload and the kernels of chunk k and the host
// never holds more than n_slots chunks (replaces the parse loops of EE:1100-1149 / VC:699-752).
class ChunkStream {
public:
    ChunkStream(const Panel &panel, std::vector<std::pair<std::string, std::string>> files, int n_threads, bool keep_line_no,
                size_t chunk_bytes, int n_slots);
    ~ChunkStream();
    ChunkStream(const ChunkStream &) = delete;
    ChunkStream &operator=(const ChunkStream &) = delete;
    Chunk *next();            // next chunk in order, nullptr after the last; rethrows the producer's Error
    void release(Chunk *c);   // the chunk's buffers may be refilled
    void shutdown();          // stop the producer and free the ring now (the destructor does the same)
    void abandon();           // stop the producer and LEAVE the ring's buffers to the end of the process (a command line about to exit:
                              //  unpinning and unmapping half a gigabyte beside the writers costs them more than the exit does)
    int samples_per_chunk() const;
    int chunks() const;
    double parse_seconds() const; // producer time spent parsing so far
private:
    struct Impl;
    Impl *im;
};

// ---- pipeline.cpp: where a command line's wall time goes (printed with AMPLISOLVE_TIMING) ----
// Named spans, summed per name, from any thread.  `critical` spans lie on the main thread's path, so they add up to the
// wall time; the others (side-thread context start-up, parser threads) are reported as overlapped work beside them.
struct PhaseClock {
    static double now();                                   // seconds, steady clock
    static void add(const char *name, double seconds, bool critical);
    struct Scope {
        const char *name;
        bool critical;
        double t0;
        Scope(const char *n, bool c = true) : name(n), critical(c), t0(now()) {}
        ~Scope() { add(name, now() - t0, critical); }
    };
    static void reset();
    static void report(std::ostream &os, double wall);     // "TIMING2 <name> <seconds> critical|overlapped" lines + the unattributed rest
};
// ---- panel.cpp ----
void panel_from_bed(const std::string &bed_path, Panel &out);                   // throws Error
std::vector<BedRow> bed_rows(const std::string &bed_path);                      // the rows alone, as Panel::rows keeps them; throws Error
void panel_load_refbases_file(Panel &p, const std::string &path);               // chrom pos base per line (EE:963)
void panel_load_fasta(Panel &p, const std::string &fasta_path);                 // replaces `samtools faidx` (EE:644)
void panel_write_interm_files(const Panel &p, const std::string &dir, int seed);// EE:601, 657-664
// ---- aseq.cpp ----
std::vector<std::pair<std::string, std::string>> list_count_files(const std::string &dir, const std::string &list_file); // EE:552-559, 794-841
std::vector<std::pair<std::string, std::string>> shard_of_files(const std::vector<std::pair<std::string, std::string>> &files, int shard_index,
                                                                int shard_count, int *first);
size_t record_bytes(int layout);
void fill_absent(int layout, char *dst, size_t n_records);
void record_unpack(int layout, const char *src, int32_t rec[8]); // one packed record -> the eight int32 counts (absent: rec[0] = AMPLI_ABSENT)
// shard_index / shard_count: keep only that contiguous range of the visit order (multi-process runs)
void cohort_load(const Panel &panel, const std::string &dir, const std::string &list_file, int n_threads, bool keep_line_no,
                 bool print_irregular, Cohort &out, int shard_index = 0, int shard_count = 1);
// ---- table.cpp ----
std::string format_rate_cell(uint8_t code, float r_fw, float r_bw, bool is_ref);  // EE:1704, 2670-2688
std::string format_germ_cell(uint8_t present, float v);                           // EE:2807-2849
void write_error_table(const Panel &panel, const float *rate, const uint8_t *code, const float *germ_val,
                       const uint8_t *germ_present, const std::string &path);
void write_error_table_default(const Panel &panel, float default_error, const std::string &path); // EE:2948-3043
void panel_from_error_table(const std::string &path, const std::string &dummy_vcf, Panel &out, std::vector<float> &thr); // VC:430-576
// ---- hip_loader.cpp ----
struct HipApi; // function pointers of libamplisolve_hip.so
const HipApi *hip_api(std::string *why = nullptr); // nullptr when the library cannot be loaded
// ---- pipeline.cpp (what the commands share; its internal declarations: pipeline.hpp) ----
// one process per GPU without Python: this process is shard `rank` of `world`, the exchange steps go over RCCL
// (ampli_comm_* of include/amplisolve_hip.h); rank 0 publishes the communicator id in id_file
struct NativeDist {
    int rank = 0, world = 1;
    std::string id_file;
    int timeout_s = 120;
};
// AMPLISOLVE_WORLD_SIZE / AMPLISOLVE_RANK / AMPLISOLVE_ID_FILE / AMPLISOLVE_RCCL_TIMEOUT (the executables' multi-GPU mode)
NativeDist native_dist_from_env(const std::string &output_dir);
// threads for a loop over n independent rows: one per `grain` rows, at most 16 and the machine's own, capped by AMPLISOLVE_THREADS
int row_threads(size_t n, size_t grain);
// the arguments of run_error_estimation (run_ee.cpp) and run_variant_calling (run_vc.cpp)
struct EeArgs {
    std::string panel_design, reference_genome, germline_dir, output_dir;
    std::string C_value = "0.002", coverage_cutoff = "100", default_error = "0.01";
    std::string refbases_file; // test hook: skip the FASTA, read chrom/pos/base lines
    const ampli_host_shard *shard = nullptr; // one shard of a multi-process run (include/amplisolve_host.h)
    NativeDist native;                       // or: one shard with the library's own RCCL transport (shard == nullptr)
    bool process_ends = false;               // the caller is an executable that exits right after: big buffers are left to the exit
};
struct VcArgs {
    std::string error_file, tumour_dir, output_dir, coverage_cutoff = "100", p_value = "0.05";
    const ampli_host_shard *shard = nullptr;
    NativeDist native;
    bool process_ends = false;
};
// ---- bam.cpp ----
// computeCounts: one BAM file -> <out_dir>/<name>.PILEUP.ASEQ
struct CcArgs {
    std::string vcf, bam, out_dir;
    int threads = 4, mbq = 20, mrq = 20, mdc = 20; // Execution_examples.md:46 recommends 20-20-20
    int64_t *stats = nullptr;                      // optional [4]: records, reads kept, bases counted, lines written
    std::string *error = nullptr;
};
int run_compute_counts(const CcArgs &a);
// ---- run_ci.cpp ----
// computeIndelCounts: one BAM file -> <out_dir>/<name>.INDEL.PILEUP.ASEQ + <name>.INDEL.LENGTHS.txt (+ the table at refbases)
struct CiArgs {
    std::string vcf, bam, out_dir, refbases; // refbases: optional path of the `chrom pos A` table for AMPLISOLVE_REFBASES_FILE
    int threads = 4, mbq = 20, mrq = 20, mdc = 20;
    int64_t *stats = nullptr; // optional [4]: records, reads kept, junctions counted, lines written
    std::string *error = nullptr;
};
int run_compute_indel_counts(const CiArgs &a);
// ---- run_ca.cpp ----
// The amplicons of a BED file as ampli_pileup_amplicon_count takes them: the rows whose chromosome is among ref_names and
// whose interval is 1 <= start <= end < 2^31, as keys sorted by lo, then hi (ties in BED order), with reach, the walk offsets and the
// permutation back to BED order.  A row that is left out keeps sorted_of_row = -1: it is still reported, with zeros.
struct AmpliconArrays {
    std::vector<uint64_t> lo, hi, reach; // [A]: ref_id << 32 | first, ref_id << 32 | last, max(hi[0..a])
    std::vector<int64_t> amp_off;        // [A + 1]: exclusive prefix sum of the lengths
    std::vector<int32_t> row_of;         // [A]: sorted index -> BED row
    std::vector<int32_t> sorted_of_row;  // [rows]: BED row -> sorted index, or -1
    int64_t A() const { return (int64_t)lo.size(); }
    int64_t W() const { return amp_off.empty() ? 0 : amp_off.back(); }
    // the sorted indices [first, last] among which the amplicons over `key` lie (those with hi[a] >= key); empty when first > last
    void candidates(uint64_t key, int64_t &first, int64_t &last) const;
};
AmpliconArrays amplicon_arrays(const std::vector<BedRow> &rows, const std::vector<std::string> &ref_names); // Error{AMPLI_E_RANGE}: W >= 2^31
// computeAmpliconCounts: one BAM file -> <out_dir>/<name>.AMPLICON.PILEUP.ASEQ, .AMPLICON.READS.txt, .AMPLICON.OVERLAPS.txt and,
// with layers_dir, <layers_dir>/<name>.AMP1.PILEUP.ASEQ, .AMP2.PILEUP.ASEQ and <name>.pairs.txt.  The numbers as the command line gives them.
struct CaArgs {
    std::string vcf, bam, bed, out_dir, layers_dir;
    std::string threads = "4", mbq = "20", mrq = "20", mdc = "20", min_overlap = "50";
    int64_t *stats = nullptr; // optional [6]: records, reads kept, reads assigned, bases counted, bases clipped, lines written
    std::string *error = nullptr;
};
int run_compute_amplicon_counts(const CaArgs &a);
// what the device computed for one file, on the host, and the writer of the command's files from it (no device: tools/amplicon_count_sanitize.cpp)
struct AmpliconCounts {
    std::vector<int32_t> counts;               // [W][8]
    std::vector<int64_t> amp_reads;            // [A][2]
    uint64_t stats[4] = {0, 0, 0, 0};          // reads kept, reads assigned, bases counted, bases clipped
    std::vector<uint64_t> keys;                // [n]: the listed positions with a known chromosome, in the list's order
    std::vector<int32_t> layers, layer_amp, total; // [2][n][8], [2][n], [n][8] over `keys`
};
struct AmpliconListed { // one listed position: what the ASEQ line prints, and its index into AmpliconCounts::keys (-1: unknown chromosome)
    std::string chrom, id, ref, alt;
    int64_t pos = 0, slot = -1;
};
// returns the lines written to <name>.AMPLICON.PILEUP.ASEQ; every file under a temporary name, renamed into place at the end
int64_t write_amplicon_files(const std::string &out_dir, const std::string &layers_dir, const std::string &name, const std::vector<BedRow> &rows,
                             const AmpliconArrays &amps, const std::vector<AmpliconListed> &listed, const AmpliconCounts &c, int mdc);
// ---- run_re.cpp ----
// computeReadEvidence: one BAM file and a list of calls -> <out_dir>/<name>.EVIDENCE.txt + <name>.EVIDENCE.HIST.txt.  The numbers
// as the command line gives them.
struct ReArgs {
    std::string vcf, bam, out_dir;
    std::string threads = "4", mbq = "20", mrq = "20", min_alt = "4", z_min = "3";
    int64_t *stats = nullptr; // optional [4]: records, reads kept, columns counted, lines written
    std::string *error = nullptr;
};
int run_compute_read_evidence(const ReArgs &a);
// the nt code of a listed allele: 0 .. 3 for one of A C G T (either case), -1 for "." where `choose` allows it, -2 for anything else
int evidence_nt(const std::string &allele, bool choose);
// the score of ampli_evidence_score on the host (ampli_ev_* of csrc/ampli_math.h): the same planes, the same bits
void evidence_score_host(const int32_t *hist, int64_t P, const int8_t *ref_nt, const int8_t *alt_nt, int64_t *o_int, int32_t *o_med, double *o_z2, int8_t *alt_used);
// one listed line with the planes of its position, and the writer of the command's two files from host arrays alone (no device:
// tools/evidence_sanitize.cpp); returns the lines written to <name>.EVIDENCE.txt; both files under temporary names, renamed at the end
struct EvidenceListed {
    std::string chrom, ref, alt;
    int64_t pos = 0;
};
int64_t write_evidence_files(const std::string &out_dir, const std::string &name, const std::vector<EvidenceListed> &listed, const int32_t *hist /* [L][4][3][64] */,
                             const int64_t *v_int /* [L][3][3] */, const int32_t *v_med /* [L][3][2] */, const double *v_z2 /* [L][3] */,
                             const int8_t *ref_nt, const int8_t *alt_used /* [L] */, int64_t min_alt, double z_min);
// ---- run_ph.cpp ----
// computePhasing: one BAM file and a list of calls -> <out_dir>/<name>.PHASE.txt + <name>.PHASE.MNV.txt.  The numbers as the
// command line gives them.
struct PhArgs {
    std::string vcf, bam, out_dir;
    std::string threads = "4", mbq = "20", mrq = "20", min_alt = "4", min_share = "10", q_min = "13", max_dist = "200";
    int64_t *stats = nullptr; // optional [6]: records, reads kept, reads covering two keys, cells incremented, pairs written, MNV lines written
    std::string *error = nullptr;
};
int run_compute_phasing(const PhArgs &a);
// the score of ampli_phase_score on the host (ampli_ph_* of csrc/ampli_math.h): the same table, the same integers
void phase_score_host(const int32_t *table, int64_t P, const int64_t *pair_cell, const int8_t *pair_nt, int64_t Q, int32_t min_alt, int32_t min_share, int64_t *o_int,
                      float *o_score, int32_t *o_class);
// one listed line and its index into the sorted keys (-1: unknown chromosome); one pair of listed lines a, b (indices into the list)
struct PhaseListed {
    std::string chrom, ref, alt;
    int64_t pos = 0, key_index = -1;
};
struct PhasePair {
    int64_t a = 0, b = 0;
    int64_t slot = -1; // its index among the formed pairs (the rows of the score's outputs), -1: NOT_FORMED
    std::string verdict;
    int64_t n_aa = 0;
};
// every two listed lines a, b with a key on one chromosome and 0 < pos_b - pos_a <= max_dist, in the order (key of a, key of b, list order);
// pair_cell / pair_nt: the formed ones (key indices at most AMPLI_PHASE_PARTNERS apart) as ampli_phase_score takes them
std::vector<PhasePair> phase_pairs(const std::vector<PhaseListed> &listed, int64_t max_dist, std::vector<int64_t> &pair_cell, std::vector<int8_t> &pair_nt);
// the verdict of a formed pair from its class and score
const char *phase_verdict(int32_t cls, float score, double q_min);
// chains of 2 or 3 lines at consecutive positions, every two of them CIS, grown greedily in (key, list) order; a line is in at most one
std::vector<std::vector<int64_t>> phase_chains(const std::vector<PhaseListed> &listed, const std::vector<PhasePair> &pairs);
// sets the pairs' verdicts and writes the command's two files from host arrays alone (no device: tools/phase_sanitize.cpp); returns the
// lines written to <name>.PHASE.txt, *mnv (optional) those of <name>.PHASE.MNV.txt; both files under temporary names, renamed at the end
int64_t write_phase_files(const std::string &out_dir, const std::string &name, const std::vector<PhaseListed> &listed, std::vector<PhasePair> &pairs,
                          const int64_t *v_int /* [Q][6] */, const float *v_score /* [Q] */, const int32_t *v_class /* [Q] */, double q_min, int64_t *mnv);
// BGZF + BAM structure only (no GPU): stats[4] = alignment records, uncompressed bytes, references, malformed records
void bam_scan(const std::string &bam, int n_threads, int64_t stats[4]);
// ---- pipeline.cpp ----
// End of a command line: all outputs are written and closed.  Flushes stdio / iostreams and leaves with _exit(status), i.e.
// without the static destructors and atexit handlers of the HIP runtime (queue / signal / pool teardown that only serves a
// process that lives on; the driver reclaims everything at exit either way).  AMPLISOLVE_EXIT=orderly returns instead.
void finish_process(int status);
// ---- run_ee.cpp, run_vc.cpp, and the project's own commands: every other run_*.cpp (what those share: command.hpp; their
// main(): command_main of main_args.hpp over the Args struct's fields) ----
int run_error_estimation(const EeArgs &a);
int run_variant_calling(const VcArgs &a);
// AmpliSolveLeaveOneOut (loo_main.cpp): C_value is one value or a comma-separated list; exit status 0 / 1
struct LooArgs {
    std::string panel_design, reference_genome, germline_dir, C_value = "0.002", coverage_cutoff = "100", calling_cutoff = "100", output_dir;
    std::string refbases_file;
};
int run_leave_one_out(const LooArgs &a);
// AmpliSolveDetectionLimit (dl_main.cpp): levels is one allele fraction or a comma-separated list of up to 8; exit status 0 / 1
struct DlArgs {
    std::string error_file, tumour_dir, output_dir, coverage_cutoff = "100", levels;
};
int run_detection_limits(const DlArgs &a);
// AmpliSolveDetectionPower (dp_main.cpp): levels as above, confidence a probability in [0.5, 0.99]; exit status 0 / 1
struct DpArgs {
    std::string error_file, tumour_dir, output_dir, coverage_cutoff = "100", levels, confidence = "0.95";
};
int run_detection_power(const DpArgs &a);
// AmpliSolvePanelDispersion (pd_main.cpp): z_cutoff is the z-score from which a cell is flagged HIGH; exit status 0 / 1
struct PdArgs {
    std::string panel_design, reference_genome, germline_dir, coverage_cutoff = "100", z_cutoff = "4", output_dir;
    std::string refbases_file;
};
int run_panel_dispersion(const PdArgs &a);
// AmpliSolveSampleConcordance (sc_main.cpp, run_sc.cpp): are the count files who they say they are.  tumour_dir "-" = the
// normals only; min_depth, min_sites integers >= 1, same_fraction in (0, 1]; exit status 0 / 1
struct ScArgs {
    std::string panel_design, germline_dir, tumour_dir = "-", min_depth = "100", min_sites = "20", same_fraction = "0.8", output_dir;
};
int run_sample_concordance(const ScArgs &a);

// AmpliSolveContamination (ct_main.cpp, run_ct.cpp): which count file leaks into which, and how much.  tumour_dir "-" = the
// normals only; min_depth, min_sites integers >= 1, min_fraction in (0, 1]; exit status 0 / 1
struct CtArgs {
    std::string panel_design, germline_dir, tumour_dir = "-", output_dir, min_depth = "100", min_sites = "20", min_fraction = "0.005";
};
int run_contamination(const CtArgs &a);

// AmpliSolveAmpliconCoverage (ac_main.cpp, run_ac.cpp): which amplicons failed, and where the copy number is off against
// the panel of normals.  tumour_dir "-" = the normals only; exclude_chrom: a comma list of chromosomes left out of library size and
// centring, "-" = none; coverage_cutoff an integer >= 0, min_normals and min_amplicons integers >= 1, z_cutoff >= 0, gain_ratio > 1,
// loss_ratio in (0, 1); exit status 0 / 1
struct AcArgs {
    std::string panel_design, germline_dir, tumour_dir = "-", output_dir, coverage_cutoff = "100", min_normals = "5", min_amplicons = "3",
                z_cutoff = "3", gain_ratio = "1.3", loss_ratio = "0.7", exclude_chrom = "chrX,chrY";
};
int run_amplicon_coverage(const AcArgs &a);

// AmpliSolveSubstitutionSpectrum (ss_main.cpp, run_ss.cpp): which kind of error a file makes more of than the panel of
// normals does, per strand-resolved substitution type and per read strand.  tumour_dir "-" = the normals only; coverage_cutoff an
// integer >= 0, max_alt_pm an integer in [0, 1000], min_sites and min_normals integers >= 1, excess_ratio > 1, z_cutoff >= 0,
// asym_delta in [0, 1]; refbases_file: a chrom / pos / base table instead of the FASTA; exit status 0 / 1
struct SsArgs {
    std::string panel_design, reference_genome, germline_dir, tumour_dir = "-", output_dir, coverage_cutoff = "100", max_alt_pm = "30",
                min_sites = "200", min_normals = "5", excess_ratio = "3", z_cutoff = "10", asym_delta = "0.15", refbases_file;
};
int run_substitution_spectrum(const SsArgs &a);

// AmpliSolveNormalExceedance (ex_main.cpp, run_ex.cpp): how many normals of the panel show an allele at a tumour's fraction
// or above, and which cells top (nearly) all of them on both strands.  tumour_dir "-" = the normals against themselves, each without
// its own file; coverage_cutoff, calling_cutoff, min_alt_reads and min_normals integers >= 0, min_vaf_pm an integer in [0, 1000],
// max_normals an integer in [0, 65534]; refbases_file: a chrom / pos / base table instead of the FASTA; exit status 0 / 1
struct ExArgs {
    std::string panel_design, reference_genome, germline_dir, tumour_dir = "-", output_dir, coverage_cutoff = "100", calling_cutoff = "100",
                min_alt_reads = "3", min_vaf_pm = "0", min_normals = "10", max_normals = "0", refbases_file;
};
int run_normal_exceedance(const ExArgs &a);
// AmpliSolveOverdispersedCalling (od_main.cpp, run_od.cpp): the dispersion omega of every cell of the panel, every tumour cell
// scored under the Poisson law and under the negative binomial, and the cells that pass the first at q_min and not the second.  C_value
// in [0, 1], coverage_cutoff an integer >= 1, calling_cutoff an integer >= 0, z_cutoff a number, q_min in (0, 100]; refbases_file: a
// chrom / pos / base table instead of the FASTA; exit status 0 / 1
struct OdArgs {
    std::string panel_design, reference_genome, germline_dir, tumour_dir, C_value = "0.002", coverage_cutoff = "100", calling_cutoff = "100",
                z_cutoff = "4", q_min = "13", output_dir, refbases_file;
};
int run_overdispersed_calling(const OdArgs &a);
// AmpliSolvePairedComparison (pc_main.cpp, run_pc.cpp): the exact conditional test of two count files of sample_dir at every
// cell, for every pair of the list `pairs` (nameA<TAB>nameB per line, the names as the Summary names samples), and the verdict of
// every cell whose pooled VAF reaches min_vaf in either file.  depth_cutoff an integer >= 0, q_min in (0, 100], min_vaf in [0, 1];
// refbases_file: a chrom / pos / base table instead of the FASTA; exit status 0 / 1
struct PcArgs {
    std::string panel_design, reference_genome, sample_dir, pairs, depth_cutoff = "100", q_min = "13", min_vaf = "0.005", output_dir, refbases_file;
};
int run_paired_comparison(const PcArgs &a);
// ---- run_di.cpp ----
// AmpliSolveInSilicoDilution (di_main.cpp, run_di.cpp): a dilution series over the files of sample_dir -- every line of `mixtures`
// (source<TAB>diluent or -<TAB>fraction[<TAB>scale]) mixed `replicates` times read by read, gated with the table's thresholds, the share of
// the source's called cells still called beside the predicted power.  replicates in 1 .. 2^20 - 1, seed an unsigned 64-bit integer,
// coverage_cutoff >= 1, confidence in [0.5, 0.99], write_counts 0 or 1; exit status 0 / 1
struct DiArgs {
    std::string error_file, sample_dir, mixtures, replicates = "8", seed = "1", coverage_cutoff = "100", confidence = "0.95", write_counts = "0", output_dir;
};
int run_insilico_dilution(const DiArgs &a);
// AmpliSolveVariantMonitoring (mo_main.cpp, run_mo.cpp): tumour-informed monitoring.  `variants` lists
// list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line, `assign` sample<TAB>list per line ("-": no assignment); the panel, the thresholds and
// the reference bases come from the error table alone.  Every file of sample_dir against every list (Monitoring_Matrix.txt), every
// assigned pair with its limit of detection, `controls` matched random lists and the list's detections among the samples not assigned
// to it (Monitoring_Own.txt), Monitoring_Summary.txt.  coverage_cutoff >= 0, q_min in (0, 100], min_variants >= 1, min_seen >= 0,
// max_vaf in [0, 1] (the gate in per mille, rounded), controls >= 0, seed an unsigned 64-bit integer; exit status 0 / 1
struct MoArgs {
    std::string error_file, sample_dir, variants, assign = "-", coverage_cutoff = "100", q_min = "20", min_variants = "5", min_seen = "2", max_vaf = "1",
                controls = "100", seed = "1", output_dir;
};
int run_variant_monitoring(const MoArgs &a);
// AmpliSolveTumourFraction (tf_main.cpp, run_tf.cpp): the tumour fraction of every (sample, list) with its score interval, the
// assigned pairs, and the change between consecutive draws of one list.  variants carries a sixth column, the weight; confidence is one of
// 0.90, 0.95, 0.99.  Fraction_Matrix.txt, Fraction_Own.txt, Fraction_Change.txt, Fraction_Summary.txt; exit status 0 / 1
struct TfArgs {
    std::string error_file, sample_dir, variants, assign = "-", coverage_cutoff = "100", min_variants = "5", max_vaf = "1", confidence = "0.95", output_dir;
};
int run_tumour_fraction(const TfArgs &a);
// AmpliSolveAllelicImbalance (ai_main.cpp, run_ai.cpp): the allelic balance at germline het sites, pooled per gene.  The het-site
// reference from the normals; every file of tumour_dir (or, with "-", the normals again: the null calibration) at the het sites of its own
// genotype or of the normal that `pairs` names (tumourName<TAB>normalName per line, or "self"); one region per gene string of the BED and
// ALL.  Allelic_Reference.txt, Allelic_Sites.txt, Allelic_Genes.txt, Allelic_Summary.txt.  min_depth >= 1, min_normals >= 1, site_q in
// [0, 100], min_sites >= 1, q_min in [0, 300], min_imbalance in [0, 1]; exit status 0 / 1
struct AiArgs {
    std::string panel_design, germline_dir, tumour_dir, pairs = "self", output_dir, min_depth = "100", min_normals = "5", site_q = "20", min_sites = "3",
                q_min = "20", min_imbalance = "0.02";
};
int run_allelic_imbalance(const AiArgs &a);
// ---- annotate.cpp ----
double fisher_two_sided(int a, int b, int c, int d);                            // VC:3797-3814 (own hypergeometric pmf)
double fisher_two_sided_direct(int a, int b, int c, int d);                     // the same, every term from log-gamma (check)
long double score_reference_sequence(int k, int rd, float err);                 // VC:3834-3884, for calls within rounding of a gate
// detection limit of one strand by the literal scan: the smallest k in 1 .. bound with score_reference_sequence(k, depth,
// thr) >= 5, scanning upwards from k = 1; -1 when thr == -1 (no estimate), 0 when there is none (also depth <= 0)
int limit_reads_literal(int depth, float thr, int bound);
// one (line, base) pair by the literal scan and the gate on the observed counts: status AMPLI_LIMIT_*, min reads (0 unless OK)
struct PairLimit { int status, min_fw, min_bw; bool called; };
PairLimit limit_pair_literal(const int32_t rec[8], int rd, int nt, float thr_fw, float thr_bw, int cov);
std::string kmer_down(const Panel &p, const std::string &chrom, int pos);       // VC:3307-3458
std::string kmer_up(const Panel &p, const std::string &chrom, int pos);         // VC:3461-3613
int homopolymer_test(const std::string &down, const std::string &up, char sub); // VC:3615-3718
// ---- run_fd.cpp ----
// AmpliSolveFalseDiscovery (fd_main.cpp, run_fd.cpp): every tumour cell scored with the exact Poisson tail against the panel's
// own error table, the Benjamini-Hochberg adjusted score of every cell per file, and the cells whose adjusted score reaches
// -10 log10(fdr).  C_value in [0, 1], coverage_cutoff an integer >= 1, calling_cutoff an integer >= 0, fdr in (0, 1), q_min in (0, 100]
// (the raw per-strand gate the listing is compared with); refbases_file: a chrom / pos / base table instead of the FASTA; exit status 0 / 1
struct FdArgs {
    std::string panel_design, reference_genome, germline_dir, tumour_dir, C_value = "0.002", coverage_cutoff = "100", calling_cutoff = "100", fdr = "0.05",
                q_min = "13", output_dir, refbases_file;
};
int run_false_discovery(const FdArgs &a);

} // namespace ampli
