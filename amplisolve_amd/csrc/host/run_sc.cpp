// amplisolve_amd/csrc/host/run_sc.cpp -- run_sample_concordance, one of the project's own command lines
// AmpliSolveSampleConcordance: every count file of the normals and the tumours is encoded into genotype bit planes from
// its counts alone (no reference genome, no error table), every pair of files is compared on the device, and the relation of a pair --
// the same person, different people, too few het sites to tell -- is decided here from two of the pair's five counts.  The cohorts
// are streamed: a chunk is uploaded, encoded straight into its rows of the one resident plane buffer and released; records never
// stay on the device.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

int run_sample_concordance(const ScArgs &a)
{
    return run_command("AmpliSolveSampleConcordance", [&]() -> int {
        ampli_genotype_params prm{100, 100, 250, 750, 900};
        prm.min_depth = parse_int(a.min_depth, "min_depth", 1);
        const int min_sites = parse_int(a.min_sites, "min_sites", 1);
        const double same_fraction = parse_number(a.same_fraction, "same_fraction", "in (0, 1]", [](double v) { return v > 0.0 && v <= 1.0; });
        require_single_gpu("AmpliSolveSampleConcordance");
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveSampleConcordance: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("none")) << ", min_depth " << prm.min_depth << ", min_sites " << min_sites
                  << ", same_fraction " << same_fraction << ", output " << a.output_dir << std::endl;
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
        // what stays resident: the planes and the N x N count matrix; beside them one chunk of records at a time
        const size_t plane_bytes = (size_t)N * AMPLI_GENO_PLANES * W * 8, count_bytes = (size_t)N * (size_t)N * 5 * sizeof(int32_t);
        const size_t reserve = (size_t)1 << 30;
        require_fits(plane_bytes + count_bytes, reserve, free_b,
                     "the samples do not fit the device: " + std::to_string(plane_bytes) + " bytes of genotype planes and " + std::to_string(count_bytes) +
                         " bytes of pair counts for " + std::to_string(N) + " samples, " + std::to_string(reserve) +
                         " bytes kept for the streamed records, " + std::to_string(free_b) + " bytes free");
        uint64_t *d_planes = dev.alloc<uint64_t>((size_t)N * AMPLI_GENO_PLANES * W);
        int32_t *d_counts = dev.alloc<int32_t>((size_t)N * (size_t)N * 5);
        // 1. normals, then tumours, each in its visit order: upload, encode into the chunk's rows, release
        DevSlot slot;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            dev.check(dev.api->genotype_planes_records(dev.ctx, &r, P, &prm, d_planes + (size_t)first * AMPLI_GENO_PLANES * W), "ampli_genotype_planes_records");
        });
        // 2. every pair at once, the relations here
        dev.check(dev.api->concordance_pairs(dev.ctx, P, d_planes, N, d_planes, N, d_counts), "ampli_concordance_pairs");
        std::vector<int32_t> cnt((size_t)N * (size_t)N * 5);
        dev.download(cnt.data(), (const int32_t *)d_counts, cnt.size());
        dev.sync();
        auto at = [&](int i, int j) { return cnt.data() + ((size_t)i * (size_t)N + (size_t)j) * 5; };
        auto relation = [&](int i, int j) { return ampli_concordance_relation(at(i, j)[3], at(i, j)[4], min_sites, same_fraction); };
        static const char *const kRelation[3] = {"UNDETERMINED", "SAME", "DIFFERENT"};
        // 3. the three files
        char b[512];
        std::string samples = "Sample\tSet\tValidSites\tHetSites\tSamePartners\tNearest\tNearestHetEither\tNearestHetMatch\tNearestConcordance\n";
        for (int i = 0; i < N; ++i) {
            int same = 0, best = -1;
            for (int j = 0; j < N; ++j) {
                if (j == i) continue;
                const int rel = relation(i, j);
                same += rel == AMPLI_RELATION_SAME ? 1 : 0;
                if (rel == AMPLI_RELATION_UNDETERMINED) continue;
                // the largest het_match / het_either, compared as fractions of integers; the first in order wins a tie
                if (best < 0 || (int64_t)at(i, j)[4] * at(i, best)[3] > (int64_t)at(i, best)[4] * at(i, j)[3]) best = j;
            }
            snprintf(b, sizeof b, "\t%c\t%d\t%d\t%d\t", i < n_normals ? 'N' : 'T', at(i, i)[0], at(i, i)[3], same);
            samples += names[(size_t)i] + b;
            if (best < 0) {
                samples += "NA\tNA\tNA\tNA\n";
            } else {
                snprintf(b, sizeof b, "\t%d\t%d\t%.4f\n", at(i, best)[3], at(i, best)[4], (double)at(i, best)[4] / (double)at(i, best)[3]);
                samples += names[(size_t)best] + b;
            }
        }
        std::string pairs = "SampleA\tSampleB\tSites\tMatch\tIBS0\tHetEither\tHetMatch\tConcordance\tRelation\n";
        long long by_relation[3] = {0, 0, 0};
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) {
                const int rel = relation(i, j);
                ++by_relation[rel];
                if (rel == AMPLI_RELATION_DIFFERENT) continue;
                const int32_t *c = at(i, j);
                char conc[64] = "NA";
                if (c[3] > 0) snprintf(conc, sizeof conc, "%.4f", (double)c[4] / (double)c[3]);
                snprintf(b, sizeof b, "\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n", c[0], c[1], c[2], c[3], c[4], conc, kRelation[rel]);
                pairs += names[(size_t)i] + "\t" + names[(size_t)j] + b;
            }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\nmin_depth=%d\nabsent_max_pm=%d\nhet_min_pm=%d\nhet_max_pm=%d\nhom_min_pm=%d\nmin_sites=%d\nsame_fraction=%g\n"
                 "pairs_same=%lld\npairs_different=%lld\npairs_undetermined=%lld\n",
                 n_normals, n_tumours, prm.min_depth, prm.absent_max_pm, prm.het_min_pm, prm.het_max_pm, prm.hom_min_pm, min_sites, same_fraction,
                 by_relation[AMPLI_RELATION_SAME], by_relation[AMPLI_RELATION_DIFFERENT], by_relation[AMPLI_RELATION_UNDETERMINED]);
        write_files(a.output_dir, {{"Concordance_Samples.txt", samples}, {"Concordance_Pairs.txt", pairs}, {"Concordance_Summary.txt", b}});
        std::cout << N << " samples: " << by_relation[AMPLI_RELATION_SAME] << " pairs SAME, " << by_relation[AMPLI_RELATION_DIFFERENT] << " DIFFERENT, "
                  << by_relation[AMPLI_RELATION_UNDETERMINED] << " UNDETERMINED" << std::endl;
        return 0;
    });
}

} // namespace ampli
