// amplisolve_amd/csrc/host/command.hpp -- what the project's own commands (every run_*.cpp but run_ee.cpp / run_vc.cpp) share: how a
// value is parsed and refused, the frame of a command, its inputs, the two ways a cohort goes over the device (streamed, resident)
// and how the files are written.  command.cpp; internal to those files.
#pragma once
#include <climits>
#include <initializer_list>
#include <string_view>

#include "pipeline.hpp"

namespace ampli {

// ---- values: a refused one throws Error{AMPLI_E_INVALID, "<what> must be ..., got '<s>'"} ----
int parse_int(const std::string &s, const char *what, long lo, long hi = INT_MAX); // a whole decimal integer in [lo, hi]
double parse_number(const std::string &s, const char *what, const char *range_text, bool (*ok)(double)); // finite, and ok(v)
std::string num(const char *fmt, double x); // the one printf format of each kind of number; NA for a NaN

// ---- the frame ----
void require_single_gpu(const char *program); // refuses AMPLISOLVE_WORLD_SIZE > 1
// body() inside the commands' one error frame: what it throws becomes "<program> failed: <why>" on stdout and status 1
int run_command(const char *program, const std::function<int()> &body);
// mkdir -p output_dir, then the files in the order given: a command that writes here, at its end, leaves nothing behind when it refuses
void write_files(const std::string &output_dir, std::initializer_list<std::pair<const char *, std::string_view>> files);

// ---- the device's memory ----
size_t device_free_bytes(Dev &dev);
void require_fits(size_t needed, size_t reserve, size_t free_bytes, const std::string &message); // Error{AMPLI_E_NOMEM, message} unless it fits

// ---- the inputs of a command over the normals and the tumours of a panel ----
using FileSet = std::vector<std::pair<std::string, std::string>>; // (path, sample name) in visit order: list_count_files
struct CohortInputs {
    Panel panel;
    FileSet sets[2]; // the normals, the tumours (none with tumour_dir "-")
    int n_normals = 0, n_tumours = 0;
    int64_t P = 0;
    std::vector<std::string> names; // the normals', then the tumours'
};
// In this order: the BED, the reference bases (reference_genome == nullptr: none are needed; else refbases_file, or the FASTA when that
// is empty), the normals' files, the tumours' unless tumour_dir is "-", "the panel has no positions", and with require_normals "no
// count files in <germline_dir>".  Throws Error.
void load_cohort(CohortInputs &in, const std::string &panel_design, const std::string *reference_genome, const std::string &refbases_file,
                 const std::string &germline_dir, const std::string &tumour_dir, bool require_normals);

// ---- streamed: records never stay on the device ----
// The normals (first_set = 0) and then the tumours, each in its visit order, through the one `slot`: fn(records, chunk, first) issues the
// chunk's work, `first` being the index of the chunk's first file among the normals followed by the tumours; then the device is waited
// for and the chunk's buffers go back to the parsers.  first_set = 1: the tumours only.
using ChunkFn = std::function<void(const ampli_records &r, Chunk &c, int first)>;
void for_each_chunk(Dev &dev, const CohortInputs &in, DevSlot &slot, const ChunkFn &fn, int first_set = 0);

// ---- the variant lists and assignments of the monitoring commands (run_mo.cpp) ----
// list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line, with <TAB>weight in (0, 1] where `weighted`, as a CSR of cells 4 p + y in the order of
// the lines (w is empty unless weighted); and sample<TAB>list per line, or "-" for none, as (file index, list index).  Both refuse what
// they cannot read, with the line's number.
struct VariantLists {
    std::vector<std::string> names;  // in the order of their first line
    std::vector<uint32_t> off, cell; // the CSR: a list's entries in the order of its lines
    std::vector<float> w;            // the entries' weights
};
VariantLists read_variant_lists(const std::string &path, const Panel &panel, bool weighted);
std::vector<std::pair<int, int>> read_assignments(const std::string &path, const FileSet &files, const VariantLists &lists, const std::string &sample_dir);

// ---- resident: every chunk of `files` stays on the device ----
struct Resident {
    ampli_records r;
    int first, n; // files [first, first + n) of `files`
};
// Every chunk into a DevSlot of its own (returned, in chunk order).  A chunk counts its records plus aux_bytes_per_record for each of
// them; before the sum and `reserve` pass free_bytes: Error{AMPLI_E_NOMEM, "<what>: ... needed so far, ... bytes free"}.  on_chunk sees
// the uploaded chunk before its host buffers go back to the parsers: the place to keep what the command needs of it.
std::vector<DevSlot> upload_resident(Dev &dev, const Panel &panel, const FileSet &files, bool keep_line_no, size_t aux_bytes_per_record, size_t reserve,
                                     size_t free_bytes, const char *what, const std::function<void(const Resident &, Chunk &)> &on_chunk);

} // namespace ampli
