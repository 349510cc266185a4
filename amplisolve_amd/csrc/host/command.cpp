// amplisolve_amd/csrc/host/command.cpp -- what the project's own twelve commands share (command.hpp)
#include "command.hpp"

namespace ampli {

int parse_int(const std::string &s, const char *what, const long lo, const long hi)
{
    char *end = nullptr;
    const long v = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || *end || v < lo || v > hi) {
        const std::string range = hi == INT_MAX ? ">= " + std::to_string(lo) : "in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
        throw Error{AMPLI_E_INVALID, std::string(what) + " must be an integer " + range + ", got '" + s + "'"};
    }
    return (int)v;
}

double parse_number(const std::string &s, const char *what, const char *range_text, bool (*ok)(double))
{
    char *end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (s.empty() || *end || !std::isfinite(v) || !ok(v))
        throw Error{AMPLI_E_INVALID, std::string(what) + " must be a number " + range_text + ", got '" + s + "'"};
    return v;
}

std::string num(const char *fmt, const double x)
{
    if (std::isnan(x)) return "NA";
    char b[64];
    snprintf(b, sizeof b, fmt, x);
    return b;
}

void require_single_gpu(const char *program)
{
    if (const char *e = getenv("AMPLISOLVE_WORLD_SIZE"))
        if (atoi(e) > 1) throw Error{AMPLI_E_INVALID, std::string(program) + " runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported"};
}

int run_command(const char *program, const std::function<int()> &body)
{
    try {
        return body();
    } catch (const Error &e) {
        return fail_line(program, e.msg);
    } catch (const std::exception &e) {
        return fail_line(program, e.what());
    }
}

void write_files(const std::string &output_dir, std::initializer_list<std::pair<const char *, std::string_view>> files)
{
    mkdir_p(output_dir);
    for (const auto &f : files) std::ofstream(output_dir + "/" + f.first) << f.second;
}

size_t device_free_bytes(Dev &dev)
{
    size_t free_b = 0, total_b = 0;
    dev.check(dev.api->mem_info(dev.ctx, &free_b, &total_b), "ampli_mem_info");
    return free_b;
}

void require_fits(const size_t needed, const size_t reserve, const size_t free_bytes, const std::string &message)
{
    if (needed + reserve > free_bytes) throw Error{AMPLI_E_NOMEM, message};
}

void load_cohort(CohortInputs &in, const std::string &panel_design, const std::string *reference_genome, const std::string &refbases_file,
                 const std::string &germline_dir, const std::string &tumour_dir, const bool require_normals)
{
    panel_from_bed(panel_design, in.panel); // without reference bases the packer still keys a line by chromosome and coordinate
    if (reference_genome) {
        if (!refbases_file.empty()) panel_load_refbases_file(in.panel, refbases_file);
        else panel_load_fasta(in.panel, *reference_genome);
    }
    in.sets[0] = list_count_files(germline_dir, std::string());
    if (tumour_dir != "-") in.sets[1] = list_count_files(tumour_dir, std::string());
    in.n_normals = (int)in.sets[0].size();
    in.n_tumours = (int)in.sets[1].size();
    in.P = in.panel.P();
    if (in.P <= 0) throw Error{AMPLI_E_INVALID, "the panel has no positions"};
    if (require_normals && in.n_normals <= 0) throw Error{AMPLI_E_INVALID, "no count files in " + germline_dir};
    for (const FileSet &set : in.sets)
        for (const auto &f : set) in.names.push_back(f.second);
}

void for_each_chunk(Dev &dev, const CohortInputs &in, DevSlot &slot, const ChunkFn &fn, const int first_set)
{
    for (int set = first_set; set < 2; ++set) {
        if (in.sets[set].empty()) continue;
        const int base = set ? in.n_normals : 0;
        const std::unique_ptr<ChunkStream> cs = open_stream(in.panel, in.sets[set], false);
        for (Chunk *c; (c = next_chunk(*cs)) != nullptr;) {
            const ampli_records r = upload_chunk(dev, slot, *c, false);
            fn(r, *c, base + c->first);
            dev.sync(); // the chunk's host buffers go back to the parsers, its device buffers to the next chunk
            cs->release(c);
        }
    }
}

std::vector<DevSlot> upload_resident(Dev &dev, const Panel &panel, const FileSet &files, const bool keep_line_no, const size_t aux_bytes_per_record,
                                     const size_t reserve, const size_t free_bytes, const char *what, const std::function<void(const Resident &, Chunk &)> &on_chunk)
{
    std::vector<DevSlot> slots;
    slots.reserve(4096);
    size_t resident_bytes = 0;
    const std::unique_ptr<ChunkStream> cs = open_stream(panel, files, keep_line_no);
    for (Chunk *c; (c = next_chunk(*cs)) != nullptr;) {
        const size_t records = (size_t)c->n * (size_t)(panel.P() + c->E);
        resident_bytes += records * record_bytes(c->layout) + records * aux_bytes_per_record;
        require_fits(resident_bytes, reserve, free_bytes, std::string(what) + ": " + std::to_string(resident_bytes + reserve) +
                                                              " bytes of records and buffers needed so far, " + std::to_string(free_bytes) + " bytes free");
        slots.emplace_back();
        const Resident x{upload_chunk(dev, slots.back(), *c, false), c->first, c->n};
        on_chunk(x, *c);
        dev.sync(); // the chunk's host buffers go back to the parsers
        cs->release(c);
    }
    return slots;
}

} // namespace ampli
