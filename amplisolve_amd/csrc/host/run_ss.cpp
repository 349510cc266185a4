// amplisolve_amd/csrc/host/run_ss.cpp -- run_substitution_spectrum, one of the project's own command lines
// AmpliSolveSubstitutionSpectrum: which kind of error a count file makes more of than the panel of normals does -- per
// strand-resolved substitution type its rate over the file's background positions against the normals' median, and the share of the
// forward strand in it.  One pass over the normals and then over the tumours: every chunk's primary records are binned by the
// trinucleotide class of their position into its rows of the one resident S x 68 x 9 matrix; one download; the folds, the reference,
// the scores and the four files here.  Records never stay on the device.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

namespace {

const char *const kRate = "%.6e", *const kRatio = "%.5f", *const kZ = "%.3f";
const char kNt[] = "ACGT";

std::string type_name(const int ty)
{
    if (ty == AMPLI_SPECTRUM_ALL) return "ALL";
    const int r = ty / 3, k = ty % 3, y = k < r ? k : k + 1;
    return std::string(1, kNt[r]) + ">" + kNt[y];
}

std::string channel_name(const int ch)
{
    const int sub = ch / 16, l = (ch / 4) % 4, t = ch % 4, r = sub >= 3 ? 3 : 1, k = sub % 3, y = k < r ? k : k + 1;
    return std::string(1, kNt[l]) + "[" + kNt[r] + ">" + kNt[y] + "]" + kNt[t];
}

} // namespace

int run_substitution_spectrum(const SsArgs &a)
{
    return run_command("AmpliSolveSubstitutionSpectrum", [&]() -> int {
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 0);
        const int max_alt_pm = parse_int(a.max_alt_pm, "max_alt_pm", 0, 1000);
        ampli_spectrum_params prm;
        prm.min_sites = parse_int(a.min_sites, "min_sites", 1);
        prm.min_normals = parse_int(a.min_normals, "min_normals", 1);
        prm.excess_ratio = parse_number(a.excess_ratio, "excess_ratio", "> 1", [](double v) { return v > 1.0; });
        prm.z_cutoff = parse_number(a.z_cutoff, "z_cutoff", ">= 0", [](double v) { return v >= 0.0; });
        prm.asym_delta = parse_number(a.asym_delta, "asym_delta", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        require_single_gpu("AmpliSolveSubstitutionSpectrum");
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveSubstitutionSpectrum: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("none")) << ", coverage_cutoff " << cov << ", max_alt_pm " << max_alt_pm << ", min_sites "
                  << prm.min_sites << ", min_normals " << prm.min_normals << ", excess_ratio " << prm.excess_ratio << ", z_cutoff " << prm.z_cutoff
                  << ", asym_delta " << prm.asym_delta << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, &a.reference_genome, a.refbases_file, a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const std::vector<std::string> &names = in.names;
        const int n_normals = in.n_normals, n_tumours = in.n_tumours, S = n_normals + n_tumours;
        const int64_t P = in.P;
        // the class of every position from the panel's own reference bases: the lookup kmer_down / kmer_up use, upper-cased
        const int C = AMPLI_SPECTRUM_CLASSES;
        std::vector<uint8_t> cls((size_t)P);
        long long census[3] = {0, 0, 0}; // trinucleotide, edge, skipped
        std::vector<uint8_t> used((size_t)C, 0);
        for (int64_t p = 0; p < P; ++p) {
            const std::string &chrom = panel.chroms[(size_t)panel.pos_chrom[(size_t)p]];
            const int coord = panel.pos_coord[(size_t)p];
            auto code = [&](const int x) {
                const int i = panel.find(chrom, x);
                return i < 0 ? 255u : ampli_spectrum_base_code(panel.ref_base[(size_t)i].c_str());
            };
            const uint32_t c = ampli_spectrum_class(panel.ref_code[(size_t)p], code(coord - 1), code(coord + 1));
            cls[(size_t)p] = (uint8_t)c;
            ++census[c < 64 ? 0 : (c < (uint32_t)C ? 1 : 2)];
            if (c < (uint32_t)C) used[c] = 1;
        }
        int classes_used = 0;
        for (const uint8_t u : used) classes_used += u;
        Dev &dev = dev_async.get();
        const size_t free_b = device_free_bytes(dev);
        // what stays resident: the sums of every (sample, class) and the two byte arrays; beside them one chunk of records
        const size_t cells = (size_t)S * (size_t)C * AMPLI_SPEC_SUMS;
        const size_t resident = cells * sizeof(int64_t) + 2 * (size_t)P;
        const size_t reserve = (size_t)1 << 30;
        require_fits(resident, reserve, free_b,
                     "the samples do not fit the device: " + std::to_string(resident) + " bytes of class sums for " + std::to_string(S) + " samples, " +
                         std::to_string(reserve) + " bytes kept for the streamed records, " + std::to_string(free_b) + " bytes free");
        int64_t *d_sums = dev.alloc<int64_t>(cells);
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
        const uint8_t *d_cls = dev.upload(cls.data(), cls.size());
        DevSlot slot;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            dev.check(dev.api->spectrum_records(dev.ctx, &r, P, d_ref, d_cls, C, cov, max_alt_pm, d_sums + (size_t)first * (size_t)C * AMPLI_SPEC_SUMS),
                      "ampli_spectrum_records");
        });
        std::vector<int64_t> sums(cells);
        dev.download(sums.data(), (const int64_t *)d_sums, sums.size());
        dev.sync();
        // stage 2: folds, reference and scores
        const int T = AMPLI_SPECTRUM_TYPES, CH = AMPLI_SPECTRUM_CHANNELS;
        std::vector<int64_t> alt((size_t)S * 2 * T), dep((size_t)S * 2 * T), sites((size_t)S * T), ctx_alt((size_t)S * CH), ctx_dep((size_t)S * CH);
        for (int s = 0; s < S; ++s)
            ampli_spectrum_fold(sums.data() + (size_t)s * C * AMPLI_SPEC_SUMS, alt.data() + (size_t)s * 2 * T, dep.data() + (size_t)s * 2 * T,
                                sites.data() + (size_t)s * T, ctx_alt.data() + (size_t)s * CH, ctx_dep.data() + (size_t)s * CH);
        std::vector<double> tmp((size_t)n_normals + 1), ref((size_t)T * 4), rate2((size_t)S * T), ratio((size_t)S * T), z((size_t)S * T), asym((size_t)S * T),
            za((size_t)S * T);
        std::vector<int32_t> n_eff((size_t)T);
        std::vector<uint8_t> status((size_t)T), flag((size_t)S * T);
        ampli_spectrum_score(alt.data(), dep.data(), sites.data(), S, n_normals, &prm, tmp.data(), ref.data(), n_eff.data(), status.data(), rate2.data(),
                             ratio.data(), z.data(), asym.data(), za.data(), flag.data());
        static const char *const kRef[2] = {"OK", "FEW"};
        static const char *const kFlag[5] = {"OK", "LOW_SITES", "NO_REFERENCE", "ELEVATED", "ASYMMETRIC"};
        char b[1024];
        // Spectrum_Reference.txt: one row per type
        std::string reference = "Type\tNeff\tMedian\tMAD\tMedianAsym\tMADAsym\tStatus\n";
        for (int ty = 0; ty < T; ++ty) {
            const double *r = ref.data() + 4 * (size_t)ty;
            reference += type_name(ty) + "\t" + std::to_string(n_eff[(size_t)ty]) + "\t" + num(kRate, r[0]) + "\t" + num(kRate, r[1]) + "\t" + num(kRatio, r[2]) +
                         "\t" + num(kRatio, r[3]) + "\t" + kRef[status[(size_t)ty]] + "\n";
        }
        // Spectrum_Samples.txt: one row per (sample, type); Spectrum_Contexts.txt: one per (sample, channel)
        std::string samples = "Sample\tSet\tType\tSites\tAltFw\tDepthFw\tAltBw\tDepthBw\tRate\tRatio\tZ\tAsym\tZAsym\tFlag\n";
        std::string contexts = "Sample\tSet\tChannel\tAlt\tDepth\tRate\n";
        std::string summary_rows = "Sample\tSet\tSitesA\tSitesC\tSitesG\tSitesT\tNotOK\n";
        long long by_flag[5] = {0, 0, 0, 0, 0};
        for (int s = 0; s < S; ++s) {
            const std::string who = names[(size_t)s] + (s < n_normals ? "\tN\t" : "\tT\t");
            const int64_t *al = alt.data() + (size_t)s * 2 * T, *de = dep.data() + (size_t)s * 2 * T, *si = sites.data() + (size_t)s * T;
            std::string bad;
            for (int ty = 0; ty < T; ++ty) {
                const size_t i = (size_t)s * T + ty;
                snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t", (long long)si[ty], (long long)al[ty], (long long)de[ty], (long long)al[T + ty],
                         (long long)de[T + ty]);
                samples += who + type_name(ty) + b + num(kRate, rate2[i]) + "\t" + num(kRatio, ratio[i]) + "\t" + num(kZ, z[i]) + "\t" + num(kRatio, asym[i]) +
                           "\t" + num(kZ, za[i]) + "\t" + kFlag[flag[i]] + "\n";
                ++by_flag[flag[i]];
                if (flag[i] != AMPLI_SPECTRUM_OK) bad += (bad.empty() ? "" : ",") + type_name(ty) + ":" + kFlag[flag[i]];
            }
            for (int ch = 0; ch < CH; ++ch) {
                const int64_t ca = ctx_alt[(size_t)s * CH + ch], cd = ctx_dep[(size_t)s * CH + ch];
                snprintf(b, sizeof b, "\t%lld\t%lld\t", (long long)ca, (long long)cd);
                contexts += who + channel_name(ch) + b + num(kRate, cd > 0 ? (double)ca / (double)cd : (double)NAN) + "\n";
            }
            snprintf(b, sizeof b, "%lld\t%lld\t%lld\t%lld\t", (long long)si[0], (long long)si[3], (long long)si[6], (long long)si[9]);
            summary_rows += who + b + (bad.empty() ? std::string("-") : bad) + "\n";
        }
        // Spectrum_Summary.txt
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\npositions=%lld\ncoverage_cutoff=%d\nmax_alt_pm=%d\nmin_sites=%lld\nmin_normals=%lld\nexcess_ratio=%g\nz_cutoff=%g\n"
                 "asym_delta=%g\npositions_trinucleotide=%lld\npositions_edge=%lld\npositions_skipped=%lld\nclasses_used=%d\n",
                 n_normals, n_tumours, (long long)P, cov, max_alt_pm, (long long)prm.min_sites, (long long)prm.min_normals, prm.excess_ratio, prm.z_cutoff,
                 prm.asym_delta, census[0], census[1], census[2], classes_used);
        write_files(a.output_dir, {{"Spectrum_Reference.txt", reference}, {"Spectrum_Samples.txt", samples}, {"Spectrum_Contexts.txt", contexts},
                                   {"Spectrum_Summary.txt", b + summary_rows}});
        std::cout << S << " samples, " << P << " positions in " << classes_used << " classes: " << by_flag[AMPLI_SPECTRUM_ELEVATED] << " (sample, type) ELEVATED, "
                  << by_flag[AMPLI_SPECTRUM_ASYMMETRIC] << " ASYMMETRIC, " << by_flag[AMPLI_SPECTRUM_LOW_SITES] << " LOW_SITES, "
                  << by_flag[AMPLI_SPECTRUM_NO_REFERENCE] << " NO_REFERENCE" << std::endl;
        return 0;
    });
}

} // namespace ampli
