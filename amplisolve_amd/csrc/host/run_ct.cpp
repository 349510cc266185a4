// amplisolve_amd/csrc/host/run_ct.cpp -- run_contamination, one of the project's own command lines
// AmpliSolveContamination: which count file of a run leaks into which, and how much.  Every file of the normals and the
// tumours is a recipient and a source: the counts of a recipient are weighed on the device against the genotype bit planes of every
// source, and the fraction of an ordered pair is estimated here from the pair's nine sums.  Two passes over the files: the first
// encodes every chunk into its rows of the one resident plane buffer (as AmpliSolveSampleConcordance does), the second streams
// every chunk again and fills its rows of the resident N x N x 9 matrix.  Records never stay on the device.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

int run_contamination(const CtArgs &a)
{
    return run_command("AmpliSolveContamination", [&]() -> int {
        const char *const kFraction = "%.5f"; // NA for the NaN of a pair without depth
        ampli_genotype_params prm{100, 100, 250, 750, 900};
        prm.min_depth = parse_int(a.min_depth, "min_depth", 1);
        const int min_sites = parse_int(a.min_sites, "min_sites", 1);
        const double min_fraction = parse_number(a.min_fraction, "min_fraction", "in (0, 1]", [](double v) { return v > 0.0 && v <= 1.0; });
        require_single_gpu("AmpliSolveContamination");
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveContamination: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("none")) << ", min_depth " << prm.min_depth << ", min_sites " << min_sites
                  << ", min_fraction " << min_fraction << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, nullptr, std::string(), a.germline_dir, a.tumour_dir, false);
        const std::vector<std::string> &names = in.names;
        const int n_normals = in.n_normals, n_tumours = in.n_tumours, N = n_normals + n_tumours;
        const int64_t P = in.P;
        const size_t W = (size_t)((P + 63) / 64);
        Dev &dev = dev_async.get();
        const size_t free_b = device_free_bytes(dev);
        // what stays resident: the planes and the N x N x 9 matrix of sums; beside them one chunk of records at a time
        const size_t plane_bytes = (size_t)N * AMPLI_GENO_PLANES * W * 8, sum_bytes = (size_t)N * (size_t)N * AMPLI_CONTAM_SUMS * sizeof(int64_t);
        const size_t reserve = (size_t)1 << 30;
        require_fits(plane_bytes + sum_bytes, reserve, free_b,
                     "the samples do not fit the device: " + std::to_string(plane_bytes) + " bytes of genotype planes and " + std::to_string(sum_bytes) +
                         " bytes of pair sums for " + std::to_string(N) + " samples, " + std::to_string(reserve) +
                         " bytes kept for the streamed records, " + std::to_string(free_b) + " bytes free");
        uint64_t *d_planes = dev.alloc<uint64_t>((size_t)N * AMPLI_GENO_PLANES * W);
        int64_t *d_sums = dev.alloc<int64_t>((size_t)N * (size_t)N * AMPLI_CONTAM_SUMS);
        // normals, then tumours, each in its visit order, twice: 1. encode the chunk into its rows of the planes; 2. once every source
        // is encoded, the chunk's recipients against all N sources into its rows of the matrix
        DevSlot slot;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            dev.check(dev.api->genotype_planes_records(dev.ctx, &r, P, &prm, d_planes + (size_t)first * AMPLI_GENO_PLANES * W), "ampli_genotype_planes_records");
        });
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            dev.check(dev.api->contamination_records(dev.ctx, &r, P, d_planes + (size_t)first * AMPLI_GENO_PLANES * W, d_planes, N,
                                                     d_sums + (size_t)first * (size_t)N * AMPLI_CONTAM_SUMS),
                      "ampli_contamination_records");
        });
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
                        pairs += names[(size_t)i] + "\t" + names[(size_t)j] + b + num(kFraction, x.fraction) + "\t" + num(kFraction, x.se) + "\n";
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
                samples += names[(size_t)best] + b + num(kFraction, x.fraction) + "\t" + num(kFraction, x.se) + "\t" + kStatus[x.status] + "\n";
            }
        }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\nmin_depth=%d\nabsent_max_pm=%d\nhet_min_pm=%d\nhet_max_pm=%d\nhom_min_pm=%d\nmin_sites=%d\nmin_fraction=%g\n"
                 "pairs_contaminated=%lld\npairs_clean=%lld\npairs_undetermined=%lld\n",
                 n_normals, n_tumours, prm.min_depth, prm.absent_max_pm, prm.het_min_pm, prm.het_max_pm, prm.hom_min_pm, min_sites, min_fraction,
                 by_status[AMPLI_CONTAM_STATUS_CONTAMINATED], by_status[AMPLI_CONTAM_STATUS_CLEAN], by_status[AMPLI_CONTAM_STATUS_UNDETERMINED]);
        write_files(a.output_dir, {{"Contamination_Samples.txt", samples}, {"Contamination_Pairs.txt", pairs}, {"Contamination_Summary.txt", b}});
        std::cout << N << " samples: " << by_status[AMPLI_CONTAM_STATUS_CONTAMINATED] << " ordered pairs CONTAMINATED, "
                  << by_status[AMPLI_CONTAM_STATUS_CLEAN] << " CLEAN, " << by_status[AMPLI_CONTAM_STATUS_UNDETERMINED] << " UNDETERMINED" << std::endl;
        return 0;
    });
}

} // namespace ampli
