// amplisolve_amd/csrc/host/run_ct.cpp -- run_contamination, one of the project's own command lines
// AmpliSolveContamination: which count file of a run leaks into which, and how much.  Every file of the normals and the
// tumours is a recipient and a source: the counts of a recipient are weighed on the device against the genotype bit planes of every
// source, and the fraction of an ordered pair is estimated here from the pair's nine sums.  Two passes over the files: the first
// encodes every chunk into its rows of the one resident plane buffer (as AmpliSolveSampleConcordance does), the second streams
// every chunk again and fills its rows of the resident N x N x 9 matrix.  Records never stay on the device.
#include "pipeline.hpp"

#include <cmath>

#include "../ampli_math.h"

namespace ampli {

namespace {

// a whole decimal integer >= 1
int parse_count(const std::string &s, const char *what)
{
    char *end = nullptr;
    const long v = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || *end || v < 1 || v > 0x7FFFFFFFl) throw Error{AMPLI_E_INVALID, std::string(what) + " must be an integer >= 1, got '" + s + "'"};
    return (int)v;
}

// "%.5f", or NA for the NaN of a pair without depth
std::string f5(double x)
{
    if (std::isnan(x)) return "NA";
    char b[64];
    snprintf(b, sizeof b, "%.5f", x);
    return b;
}

} // namespace

int run_contamination(const CtArgs &a)
{
    try {
        ampli_genotype_params prm{100, 100, 250, 750, 900};
        prm.min_depth = parse_count(a.min_depth, "min_depth");
        const int min_sites = parse_count(a.min_sites, "min_sites");
        char *end = nullptr;
        const double min_fraction = std::strtod(a.min_fraction.c_str(), &end);
        if (a.min_fraction.empty() || *end || !(min_fraction > 0.0 && min_fraction <= 1.0))
            throw Error{AMPLI_E_INVALID, "min_fraction must be a number in (0, 1], got '" + a.min_fraction + "'"};
        if (const char *e = getenv("AMPLISOLVE_WORLD_SIZE"))
            if (atoi(e) > 1) throw Error{AMPLI_E_INVALID, "AmpliSolveContamination runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported"};
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveContamination: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("none")) << ", min_depth " << prm.min_depth << ", min_sites " << min_sites
                  << ", min_fraction " << min_fraction << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        Panel panel;
        panel_from_bed(a.panel_design, panel); // no reference base is needed: the packer keys a line by chromosome and coordinate
        std::vector<std::pair<std::string, std::string>> sets[2];
        sets[0] = list_count_files(a.germline_dir, std::string());
        if (with_tumours) sets[1] = list_count_files(a.tumour_dir, std::string());
        const int n_normals = (int)sets[0].size(), n_tumours = (int)sets[1].size(), N = n_normals + n_tumours;
        const int64_t P = panel.P();
        if (P <= 0) throw Error{AMPLI_E_INVALID, "the panel has no positions"};
        const size_t W = (size_t)((P + 63) / 64);
        Dev &dev = dev_async.get();
        size_t free_b = 0, total_b = 0;
        dev.check(dev.api->mem_info(dev.ctx, &free_b, &total_b), "ampli_mem_info");
        // what stays resident: the planes and the N x N x 9 matrix of sums; beside them one chunk of records at a time
        const size_t plane_bytes = (size_t)N * AMPLI_GENO_PLANES * W * 8, sum_bytes = (size_t)N * (size_t)N * AMPLI_CONTAM_SUMS * sizeof(int64_t);
        const size_t reserve = (size_t)1 << 30;
        if (plane_bytes + sum_bytes + reserve > free_b)
            throw Error{AMPLI_E_NOMEM, "the samples do not fit the device: " + std::to_string(plane_bytes) + " bytes of genotype planes and " +
                                           std::to_string(sum_bytes) + " bytes of pair sums for " + std::to_string(N) + " samples, " +
                                           std::to_string(reserve) + " bytes kept for the streamed records, " + std::to_string(free_b) + " bytes free"};
        uint64_t *d_planes = dev.alloc<uint64_t>((size_t)N * AMPLI_GENO_PLANES * W);
        int64_t *d_sums = dev.alloc<int64_t>((size_t)N * (size_t)N * AMPLI_CONTAM_SUMS);
        // normals, then tumours, each in its visit order, twice: 1. encode the chunk into its rows of the planes; 2. once every source
        // is encoded, the chunk's recipients against all N sources into its rows of the matrix
        std::vector<std::string> names;
        DevSlot slot;
        for (int pass = 0; pass < 2; ++pass) {
            int base = 0;
            for (int set = 0; set < 2; ++set) {
                if (sets[set].empty()) continue;
                const std::unique_ptr<ChunkStream> cs = open_stream(panel, sets[set], false);
                for (Chunk *c; (c = next_chunk(*cs)) != nullptr;) {
                    const ampli_records r = upload_chunk(dev, slot, *c, false);
                    uint64_t *rows = d_planes + (size_t)(base + c->first) * AMPLI_GENO_PLANES * W;
                    if (pass == 0)
                        dev.check(dev.api->genotype_planes_records(dev.ctx, &r, P, &prm, rows), "ampli_genotype_planes_records");
                    else
                        dev.check(dev.api->contamination_records(dev.ctx, &r, P, rows, d_planes, N,
                                                                 d_sums + (size_t)(base + c->first) * (size_t)N * AMPLI_CONTAM_SUMS),
                                  "ampli_contamination_records");
                    dev.sync(); // the chunk's host buffers go back to the parsers, its device buffers to the next chunk
                    cs->release(c);
                }
                if (pass == 0)
                    for (const auto &f : sets[set]) names.push_back(f.second);
                base += (int)sets[set].size();
            }
        }
        std::vector<int64_t> sums((size_t)N * (size_t)N * AMPLI_CONTAM_SUMS);
        if (N > 0) dev.download(sums.data(), (const int64_t *)d_sums, sums.size());
        dev.sync();
        auto at = [&](int i, int j) { return sums.data() + ((size_t)i * (size_t)N + (size_t)j) * AMPLI_CONTAM_SUMS; };
        struct Est { double fraction, se, e; int status; };
        auto est = [&](int i, int j) {
            Est x;
            x.status = ampli_contamination_estimate(at(i, j), min_sites, min_fraction, &x.fraction, &x.se, &x.e);
            return x;
        };
        static const char *const kStatus[3] = {"UNDETERMINED", "CLEAN", "CONTAMINATED"};
        // the three files
        char b[768];
        std::string samples = "Sample\tSet\tHomSites\tBackground\tSource\tSites\tFraction\tSE\tStatus\n";
        std::string pairs = "Recipient\tSource\tSitesHom\tAltHom\tDepthHom\tSitesHet\tAltHet\tDepthHet\tSitesBg\tAltBg\tDepthBg\tFraction\tSE\n";
        long long by_status[3] = {0, 0, 0};
        for (int i = 0; i < N; ++i) {
            int best = -1;
            double best_rank = 0;
            for (int j = 0; j < N; ++j) {
                const Est x = est(i, j);
                if (j != i) {
                    ++by_status[x.status];
                    if (x.status == AMPLI_CONTAM_STATUS_CONTAMINATED) {
                        const int64_t *s = at(i, j);
                        snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t", (long long)s[0], (long long)s[1], (long long)s[2],
                                 (long long)s[3], (long long)s[4], (long long)s[5], (long long)s[6], (long long)s[7], (long long)s[8]);
                        pairs += names[(size_t)i] + "\t" + names[(size_t)j] + b + f5(x.fraction) + "\t" + f5(x.se) + "\n";
                    }
                }
                if (x.status == AMPLI_CONTAM_STATUS_UNDETERMINED) continue;
                const double rank = std::isnan(x.fraction) ? -1.0 : x.fraction; // a pair without depth ranks last
                if (best < 0 || rank > best_rank) { best = j; best_rank = rank; } // the first source in order wins a tie
            }
            snprintf(b, sizeof b, "\t%c\t%lld\t%.6f\t", i < n_normals ? 'N' : 'T', (long long)at(i, i)[AMPLI_CONTAM_SITES_BG], est(i, i).e);
            samples += names[(size_t)i] + b;
            if (best < 0) {
                samples += "NA\tNA\tNA\tNA\tUNDETERMINED\n";
            } else {
                const Est x = est(i, best);
                snprintf(b, sizeof b, "\t%lld\t", (long long)(at(i, best)[AMPLI_CONTAM_SITES_HOM] + at(i, best)[AMPLI_CONTAM_SITES_HET]));
                samples += names[(size_t)best] + b + f5(x.fraction) + "\t" + f5(x.se) + "\t" + kStatus[x.status] + "\n";
            }
        }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\nmin_depth=%d\nabsent_max_pm=%d\nhet_min_pm=%d\nhet_max_pm=%d\nhom_min_pm=%d\nmin_sites=%d\nmin_fraction=%g\n"
                 "pairs_contaminated=%lld\npairs_clean=%lld\npairs_undetermined=%lld\n",
                 n_normals, n_tumours, prm.min_depth, prm.absent_max_pm, prm.het_min_pm, prm.het_max_pm, prm.hom_min_pm, min_sites, min_fraction,
                 by_status[AMPLI_CONTAM_STATUS_CONTAMINATED], by_status[AMPLI_CONTAM_STATUS_CLEAN], by_status[AMPLI_CONTAM_STATUS_UNDETERMINED]);
        mkdir_p(a.output_dir);
        std::ofstream(a.output_dir + "/Contamination_Samples.txt") << samples;
        std::ofstream(a.output_dir + "/Contamination_Pairs.txt") << pairs;
        std::ofstream(a.output_dir + "/Contamination_Summary.txt") << b;
        std::cout << N << " samples: " << by_status[AMPLI_CONTAM_STATUS_CONTAMINATED] << " ordered pairs CONTAMINATED, "
                  << by_status[AMPLI_CONTAM_STATUS_CLEAN] << " CLEAN, " << by_status[AMPLI_CONTAM_STATUS_UNDETERMINED] << " UNDETERMINED" << std::endl;
        return 0;
    } catch (const Error &e) {
        return fail_line("AmpliSolveContamination", e.msg);
    } catch (const std::exception &e) {
        return fail_line("AmpliSolveContamination", e.what());
    }
}

} // namespace ampli
