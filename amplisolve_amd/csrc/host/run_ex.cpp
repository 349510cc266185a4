// amplisolve_amd/csrc/host/run_ex.cpp -- run_normal_exceedance, one of the project's own command lines
// AmpliSolveNormalExceedance: for every cell (file, position, alternative base) of the tumours, how many normals of the
// panel show the allele at the file's fraction or above on each strand, and which cells are candidates: enough reads on both strands,
// enough eligible normals, and at most max_normals of them reaching on either strand.  Every chunk of the normals stays resident on
// the device; the tumours stream chunk by chunk, each against every resident chunk into the same two count arrays (the first
// overwrites, the others accumulate); the candidate rule (ampli_exceedance_candidate, ampli_math.h) and the four files here.
// tumour_dir=- runs the normals against themselves, each without its own file: the leave-self-out false-candidate rate of the panel.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

namespace {

struct ExResident : Resident { // a chunk of the normals that stays on the device; with tumour_dir=- also the host's copy of its primary records
    int layout;
    std::vector<char> prim;
};

std::string per_1000(const long long c, const long long e)
{
    char b[64];
    snprintf(b, sizeof b, "%.4f", e ? 1000.0 * (double)c / (double)e : 0.0);
    return b;
}

} // namespace

int run_normal_exceedance(const ExArgs &a)
{
    return run_command("AmpliSolveNormalExceedance", [&]() -> int {
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 0);
        const int call_cov = parse_int(a.calling_cutoff, "calling_cutoff", 0);
        ampli_exceedance_params prm;
        prm.min_alt_reads = parse_int(a.min_alt_reads, "min_alt_reads", 0);
        prm.min_vaf_pm = parse_int(a.min_vaf_pm, "min_vaf_pm", 0, 1000);
        prm.min_normals = parse_int(a.min_normals, "min_normals", 0);
        prm.max_normals = parse_int(a.max_normals, "max_normals", 0, AMPLI_EXCEEDANCE_MAX_NORMALS);
        require_single_gpu("AmpliSolveNormalExceedance");
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveNormalExceedance: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("the normals themselves")) << ", coverage_cutoff " << cov << ", calling_cutoff " << call_cov
                  << ", min_alt_reads " << prm.min_alt_reads << ", min_vaf_pm " << prm.min_vaf_pm << ", min_normals " << prm.min_normals << ", max_normals "
                  << prm.max_normals << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, &a.reference_genome, a.refbases_file, a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const int n_normals = in.n_normals, n_tumours = in.n_tumours;
        const int64_t P = in.P;
        if (n_normals > AMPLI_EXCEEDANCE_MAX_NORMALS)
            throw Error{AMPLI_E_RANGE, "a panel of at most " + std::to_string(AMPLI_EXCEEDANCE_MAX_NORMALS) + " normals is supported, " + a.germline_dir + " has " +
                                           std::to_string(n_normals)};
        const FileSet &files = in.sets[with_tumours ? 1 : 0]; // the files under test
        const int F = (int)files.size();
        Dev &dev = dev_async.get();
        // every chunk of the normals stays resident: refuse before the device runs out (beside them one chunk of tumours and its counts)
        std::vector<ExResident> res;
        upload_resident(dev, panel, in.sets[0], false, 5, (size_t)1 << 30, device_free_bytes(dev), "the normals do not fit the device",
                        [&](const Resident &x, Chunk &c) {
                            res.push_back(ExResident{x, c.layout, {}});
                            if (!with_tumours) res.back().prim.assign((const char *)c.prim, (const char *)c.prim + (size_t)c.n * (size_t)P * record_bytes(c.layout));
                        });
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());

        std::string candidates = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tAF\tElig\tGE_fw\tGE_rs\n";
        std::vector<long long> evaluated_of((size_t)F, 0), candidates_of((size_t)F, 0), cand_pos((size_t)P * 4, 0);
        std::vector<uint16_t> elig_all((size_t)F * (size_t)P);
        DevBuf b_elig, b_ge;
        std::vector<uint16_t> elig, ge;
        char b[512];
        // one chunk of the files under test: its counts against every resident chunk, then the candidate rule on the host
        auto test_chunk = [&](const ampli_records &tr, const int first, const int n, const int layout, const char *prim) {
            const size_t cells = (size_t)n * (size_t)P;
            uint16_t *d_elig = (uint16_t *)b_elig.ensure(dev, cells * sizeof(uint16_t));
            uint16_t *d_ge = (uint16_t *)b_ge.ensure(dev, cells * 8 * sizeof(uint16_t));
            for (size_t k = 0; k < res.size(); ++k)
                dev.check(dev.api->exceedance_records(dev.ctx, &tr, &res[k].r, P, d_ref, cov, call_cov, (with_tumours ? n_normals : 0) + first, res[k].first,
                                                      with_tumours ? 0 : 1, k ? 1 : 0, d_elig, d_ge),
                          "ampli_exceedance_records");
            elig.resize(cells);
            ge.resize(cells * 8);
            dev.download(elig.data(), (const uint16_t *)d_elig, cells);
            dev.download(ge.data(), (const uint16_t *)d_ge, cells * 8);
            dev.sync();
            const size_t rb = record_bytes(layout);
            for (int s = 0; s < n; ++s) {
                const size_t f = (size_t)(first + s);
                std::copy(elig.begin() + (size_t)s * P, elig.begin() + (size_t)(s + 1) * P, elig_all.begin() + f * (size_t)P);
                for (int64_t p = 0; p < P; ++p) {
                    const size_t cell = (size_t)s * (size_t)P + (size_t)p;
                    const uint16_t *g = ge.data() + cell * 8;
                    int32_t rec[8];
                    bool have = false;
                    for (int y = 0; y < 4; ++y) {
                        if (g[2 * y] == AMPLI_EXCEEDANCE_NA) continue;
                        ++evaluated_of[f];
                        if (!have) { record_unpack(layout, prim + cell * rb, rec); have = true; }
                        const uint64_t d_fw = (uint64_t)rec[0] + (uint64_t)rec[1] + (uint64_t)rec[2] + (uint64_t)rec[3];
                        const uint64_t d_bw = (uint64_t)rec[4] + (uint64_t)rec[5] + (uint64_t)rec[6] + (uint64_t)rec[7];
                        const uint64_t x_fw = (uint64_t)rec[y], x_bw = (uint64_t)rec[4 + y];
                        if (!ampli_exceedance_candidate(x_fw, x_bw, d_fw, d_bw, elig[cell], g[2 * y], g[2 * y + 1], &prm)) continue;
                        ++candidates_of[f];
                        ++cand_pos[(size_t)p * 4 + y];
                        const uint64_t d = d_fw + d_bw;
                        char af[64] = "NA";
                        if (d) snprintf(af, sizeof af, "%.6f", (double)(x_fw + x_bw) / (double)d);
                        snprintf(b, sizeof b, "\t%d\t%c->%c\t%llu\t%llu\t%llu\t%llu\t%s\t%u\t%u\t%u\n", panel.pos_coord[(size_t)p], "ACGT"[panel.ref_code[(size_t)p]],
                                 "ACGT"[y], (unsigned long long)x_fw, (unsigned long long)x_bw, (unsigned long long)d_fw, (unsigned long long)d_bw, af,
                                 (unsigned)elig[cell], (unsigned)g[2 * y], (unsigned)g[2 * y + 1]);
                        candidates += files[f].second + "\t" + panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + b;
                    }
                }
            }
        };
        if (with_tumours) {
            DevSlot slot;
            for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &c, int) { test_chunk(r, c.first, c.n, c.layout, (const char *)c.prim); }, 1);
        } else {
            for (const ExResident &x : res) test_chunk(x.r, x.first, x.n, x.layout, x.prim.data());
        }

        // Exceedance_Samples.txt, Exceedance_Positions.txt, Exceedance_Summary.txt
        std::string samples = "sample\tEvaluated\tCandidates\tCandidates_per_1000\n";
        long long evaluated = 0, n_candidates = 0;
        for (int f = 0; f < F; ++f) {
            samples += files[(size_t)f].second + "\t" + std::to_string(evaluated_of[(size_t)f]) + "\t" + std::to_string(candidates_of[(size_t)f]) + "\t" +
                       per_1000(candidates_of[(size_t)f], evaluated_of[(size_t)f]) + "\n";
            evaluated += evaluated_of[(size_t)f];
            n_candidates += candidates_of[(size_t)f];
        }
        std::string positions = "chrom\tposition\treference\tMedianElig\tCand_A\tCand_C\tCand_G\tCand_T\n";
        std::vector<uint16_t> col((size_t)F);
        long long with_reference = 0;
        for (int64_t p = 0; p < P; ++p) {
            std::string median = "NA"; // the median of the files' eligible normals: the mean of the two middle ones when F is even
            if (F > 0) {
                for (int f = 0; f < F; ++f) col[(size_t)f] = elig_all[(size_t)f * (size_t)P + (size_t)p];
                std::sort(col.begin(), col.end());
                snprintf(b, sizeof b, "%.1f", ((double)col[(size_t)(F - 1) / 2] + (double)col[(size_t)F / 2]) / 2.0);
                median = b;
            }
            with_reference += panel.ref_code[(size_t)p] <= 3 ? 1 : 0;
            positions += panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + "\t" + std::to_string(panel.pos_coord[(size_t)p]) + "\t" + panel.ref_base[(size_t)p] + "\t" +
                         median;
            for (int y = 0; y < 4; ++y) positions += "\t" + std::to_string(cand_pos[(size_t)p * 4 + y]);
            positions += "\n";
        }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\npositions=%lld\npositions_with_reference=%lld\ncoverage_cutoff=%d\ncalling_cutoff=%d\nmin_alt_reads=%lld\n"
                 "min_vaf_pm=%lld\nmin_normals=%lld\nmax_normals=%lld\nskip_same_index=%d\nevaluated=%lld\ncandidates=%lld\ncandidates_per_1000=%s\n",
                 n_normals, n_tumours, (long long)P, with_reference, cov, call_cov, (long long)prm.min_alt_reads, (long long)prm.min_vaf_pm,
                 (long long)prm.min_normals, (long long)prm.max_normals, with_tumours ? 0 : 1, evaluated, n_candidates, per_1000(n_candidates, evaluated).c_str());
        write_files(a.output_dir, {{"Exceedance_Candidates.txt", candidates}, {"Exceedance_Samples.txt", samples}, {"Exceedance_Positions.txt", positions},
                                   {"Exceedance_Summary.txt", b}});
        std::cout << F << " files against " << n_normals << " normals, " << P << " positions: " << n_candidates << " candidates in " << evaluated
                  << " evaluated cells" << std::endl;
        return 0;
    });
}

} // namespace ampli
