// amplisolve_amd/csrc/host/run_ac.cpp -- run_amplicon_coverage, one of the project's own command lines
// AmpliSolveAmpliconCoverage: which amplicons of the design failed, in the panel of normals or in one file, and where a
// file's copy number is off.  One pass over the normals and then over the tumours: every chunk's primary records are summed along the
// amplicons' position lists into its rows of the one resident S x A x 4 matrix; then the reference from the normals' rows and the
// ratios of all rows, both on the device; the gene level and the four files here.  Records never stay on the device.
#include "command.hpp"

#include <map>

#include "../ampli_math.h"

namespace ampli {

namespace {

const char *const kShare = "%.6e", *const kRatio = "%.5f", *const kZ = "%.3f", *const kFraction = "%.4f";

} // namespace

int run_amplicon_coverage(const AcArgs &a)
{
    return run_command("AmpliSolveAmpliconCoverage", [&]() -> int {
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 0);
        const int min_normals = parse_int(a.min_normals, "min_normals", 1);
        const int min_amplicons = parse_int(a.min_amplicons, "min_amplicons", 1);
        const double z_cutoff = parse_number(a.z_cutoff, "z_cutoff", ">= 0", [](double v) { return v >= 0.0; });
        const double gain_ratio = parse_number(a.gain_ratio, "gain_ratio", "> 1", [](double v) { return v > 1.0; });
        const double loss_ratio = parse_number(a.loss_ratio, "loss_ratio", "in (0, 1)", [](double v) { return v > 0.0 && v < 1.0; });
        if (a.exclude_chrom.empty()) throw Error{AMPLI_E_INVALID, "exclude_chrom must be a comma list of chromosomes or -, got ''"};
        std::vector<std::string> excluded;
        if (a.exclude_chrom != "-") {
            size_t at = 0;
            while (at <= a.exclude_chrom.size()) {
                const size_t comma = std::min(a.exclude_chrom.find(',', at), a.exclude_chrom.size());
                if (comma > at) excluded.push_back(a.exclude_chrom.substr(at, comma - at));
                at = comma + 1;
            }
        }
        require_single_gpu("AmpliSolveAmpliconCoverage");
        const bool with_tumours = a.tumour_dir != "-";
        std::cout << "AmpliSolveAmpliconCoverage: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("none")) << ", coverage_cutoff " << cov << ", min_normals " << min_normals
                  << ", min_amplicons " << min_amplicons << ", z_cutoff " << z_cutoff << ", gain_ratio " << gain_ratio << ", loss_ratio " << loss_ratio
                  << ", exclude_chrom " << a.exclude_chrom << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, nullptr, std::string(), a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const std::vector<std::string> &names = in.names;
        const int n_normals = in.n_normals, n_tumours = in.n_tumours, S = n_normals + n_tumours;
        const int64_t P = in.P;
        // the amplicons' lists: a BED row's walk entries whose position is listed once in the BED -- a position under two overlapping
        // amplicons carries both amplicons' reads and would count towards neither cleanly -- or all its entries if none is left
        const int A = (int)panel.rows.size();
        std::vector<uint32_t> amp_off(1, 0u), amp_pos;
        std::vector<uint8_t> use((size_t)A, 1);
        size_t wo = 0;
        for (int i = 0; i < A; ++i) {
            const BedRow &r = panel.rows[(size_t)i];
            const size_t len = r.end >= r.start ? (size_t)((int64_t)r.end - r.start + 1) : 0;
            const size_t before = amp_pos.size();
            for (size_t k = 0; k < len; ++k)
                if (!panel.dup[panel.walk[wo + k]]) amp_pos.push_back(panel.walk[wo + k]);
            if (amp_pos.size() == before) amp_pos.insert(amp_pos.end(), panel.walk.begin() + (long)wo, panel.walk.begin() + (long)(wo + len));
            wo += len;
            amp_off.push_back((uint32_t)amp_pos.size());
            for (const std::string &x : excluded)
                if (x == r.chrom) use[(size_t)i] = 0;
        }
        const int64_t W = (int64_t)amp_pos.size();
        if (A > AMPLI_AMPLICON_MAX || n_normals > AMPLI_AMPLICON_MAX)
            throw Error{AMPLI_E_RANGE, "at most " + std::to_string(AMPLI_AMPLICON_MAX) + " amplicons and as many normals are supported, got " +
                                           std::to_string(A) + " amplicons and " + std::to_string(n_normals) + " normals"};
        Dev &dev = dev_async.get();
        const size_t free_b = device_free_bytes(dev);
        // what stays resident: the sums, the ratios and z of every (sample, amplicon), and the lists; beside them one chunk of records
        const size_t cells = (size_t)S * (size_t)A;
        const size_t resident = cells * (AMPLI_AMP_SUMS * sizeof(int64_t) + 2 * sizeof(double)) + (size_t)(W + A + 1) * sizeof(uint32_t);
        const size_t reserve = (size_t)1 << 30;
        require_fits(resident, reserve, free_b,
                     "the samples do not fit the device: " + std::to_string(resident) + " bytes of amplicon sums and ratios for " + std::to_string(S) +
                         " samples and " + std::to_string(A) + " amplicons, " + std::to_string(reserve) + " bytes kept for the streamed records, " +
                         std::to_string(free_b) + " bytes free");
        int64_t *d_sums = dev.alloc<int64_t>(cells * AMPLI_AMP_SUMS);
        const uint32_t *d_off = dev.upload(amp_off.data(), amp_off.size());
        const uint32_t *d_pos = dev.upload(amp_pos.data(), amp_pos.size());
        const uint8_t *d_use = dev.upload(use.data(), use.size());
        DevSlot slot;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            dev.check(dev.api->amplicon_depth_records(dev.ctx, &r, P, A, d_off, d_pos, W, cov, d_sums + (size_t)first * (size_t)A * AMPLI_AMP_SUMS),
                      "ampli_amplicon_depth_records");
        });
        int64_t *d_total_n = dev.alloc<int64_t>((size_t)n_normals), *d_total = dev.alloc<int64_t>((size_t)S);
        double *d_ref = dev.alloc<double>((size_t)A * 2), *d_centre = dev.alloc<double>((size_t)S);
        uint8_t *d_status = dev.alloc<uint8_t>((size_t)A);
        int32_t *d_k = dev.alloc<int32_t>((size_t)S);
        double *d_ratio = dev.alloc<double>(cells), *d_z = dev.alloc<double>(cells);
        dev.check(dev.api->amplicon_reference(dev.ctx, d_sums, n_normals, A, d_use, min_normals, d_total_n, d_ref, d_status), "ampli_amplicon_reference");
        dev.check(dev.api->amplicon_ratio(dev.ctx, d_sums, S, A, d_use, d_ref, d_status, d_total, d_centre, d_k, d_ratio, d_z), "ampli_amplicon_ratio");
        std::vector<int64_t> sums(cells * AMPLI_AMP_SUMS), total((size_t)S);
        std::vector<double> ref((size_t)A * 2), centre((size_t)S), ratio(cells), z(cells);
        std::vector<uint8_t> status((size_t)A);
        std::vector<int32_t> kk((size_t)S);
        dev.download(sums.data(), (const int64_t *)d_sums, sums.size());
        dev.download(total.data(), (const int64_t *)d_total, total.size());
        dev.download(ref.data(), (const double *)d_ref, ref.size());
        dev.download(centre.data(), (const double *)d_centre, centre.size());
        dev.download(status.data(), (const uint8_t *)d_status, status.size());
        dev.download(kk.data(), (const int32_t *)d_k, kk.size());
        dev.download(ratio.data(), (const double *)d_ratio, ratio.size());
        dev.download(z.data(), (const double *)d_z, z.size());
        dev.sync();
        auto cell = [&](int s, int i) { return sums.data() + ((size_t)s * (size_t)A + (size_t)i) * AMPLI_AMP_SUMS; };
        auto len_of = [&](int i) { return (int64_t)(amp_off[(size_t)i + 1] - amp_off[(size_t)i]); };
        int n_eff = 0;
        for (int n = 0; n < n_normals; ++n) n_eff += total[(size_t)n] > 0 ? 1 : 0;
        static const char *const kStatus[3] = {"OK", "FEW", "DARK"};
        static const char *const kGene[3] = {"NEUTRAL", "GAIN", "LOSS"};
        char b[1024];
        // Amplicon_Reference.txt: one row per amplicon
        std::string reference = "Chrom\tStart\tEnd\tAmplicon\tGene\tPositions\tStatus\tNeff\tMedian\tMAD\tCallable\n";
        long long by_status[3] = {0, 0, 0};
        for (int i = 0; i < A; ++i) {
            const BedRow &r = panel.rows[(size_t)i];
            ++by_status[status[(size_t)i]];
            int64_t callable = 0;
            for (int n = 0; n < n_normals; ++n) callable += cell(n, i)[AMPLI_AMP_CALLABLE];
            const int64_t len = len_of(i);
            const double fraction = len > 0 ? (double)callable / (double)((int64_t)n_normals * len) : (double)NAN;
            snprintf(b, sizeof b, "\t%d\t%d\t", r.start, r.end);
            reference += r.chrom + b + r.name + "\t" + r.gene + "\t" + std::to_string(len) + "\t" + kStatus[status[(size_t)i]] + "\t" + std::to_string(n_eff) +
                         "\t" + num(kShare, ref[2 * (size_t)i]) + "\t" + num(kShare, ref[2 * (size_t)i + 1]) + "\t" + num(kFraction, fraction) + "\n";
        }
        // Amplicon_Ratios.txt: one row per (sample, amplicon)
        std::string ratios = "Sample\tSet\tAmplicon\tGene\tPresent\tDepthFw\tDepthBw\tCallable\tRatio\tZ\n";
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < A; ++i) {
                const int64_t *c = cell(s, i);
                snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t", (long long)c[AMPLI_AMP_PRESENT], (long long)c[AMPLI_AMP_DEPTH_FW],
                         (long long)c[AMPLI_AMP_DEPTH_BW], (long long)c[AMPLI_AMP_CALLABLE]);
                ratios += names[(size_t)s] + (s < n_normals ? "\tN\t" : "\tT\t") + panel.rows[(size_t)i].name + "\t" + panel.rows[(size_t)i].gene + b +
                          num(kRatio, ratio[(size_t)s * (size_t)A + (size_t)i]) + "\t" + num(kZ, z[(size_t)s * (size_t)A + (size_t)i]) + "\n";
            }
        // Amplicon_Genes.txt: per (sample, gene) over the gene's OK amplicons; the tumours' GAIN and LOSS rows, or every row of the normals
        std::map<std::string, std::vector<int>> genes; // in the order of the gene strings' bytes
        for (int i = 0; i < A; ++i) {
            std::vector<int> &g = genes[panel.rows[(size_t)i].gene];
            if (status[(size_t)i] == AMPLI_AMPLICON_OK) g.push_back(i);
        }
        std::string gene_rows = "Sample\tSet\tGene\tAmplicons\tMedianRatio\tMedianZ\tStatus\n";
        long long gains = 0, losses = 0;
        std::vector<double> vr, vz;
        for (int s = with_tumours ? n_normals : 0; s < S; ++s)
            for (const auto &g : genes) {
                vr.clear();
                vz.clear();
                for (const int i : g.second) {
                    vr.push_back(ratio[(size_t)s * (size_t)A + (size_t)i]);
                    vz.push_back(z[(size_t)s * (size_t)A + (size_t)i]);
                }
                const int64_t n = (int64_t)g.second.size();
                const double mr = ampli_amplicon_median(vr.data(), n), mz = ampli_amplicon_median(vz.data(), n);
                const int st = ampli_amplicon_gene_status(n, mr, mz, min_amplicons, gain_ratio, loss_ratio, z_cutoff);
                gains += st == AMPLI_GENE_GAIN;
                losses += st == AMPLI_GENE_LOSS;
                if (with_tumours && st == AMPLI_GENE_NEUTRAL) continue;
                gene_rows += names[(size_t)s] + (s < n_normals ? "\tN\t" : "\tT\t") + g.first + "\t" + std::to_string(n) + "\t" + num(kRatio, mr) + "\t" +
                             num(kZ, mz) + "\t" + kGene[st] + "\n";
            }
        // Amplicon_Summary.txt
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\namplicons=%d\ncoverage_cutoff=%d\nmin_normals=%d\nmin_amplicons=%d\nz_cutoff=%g\ngain_ratio=%g\nloss_ratio=%g\n"
                 "exclude_chrom=%s\nn_eff=%d\namplicons_ok=%lld\namplicons_few=%lld\namplicons_dark=%lld\ngenes_gain=%lld\ngenes_loss=%lld\n",
                 n_normals, n_tumours, A, cov, min_normals, min_amplicons, z_cutoff, gain_ratio, loss_ratio, a.exclude_chrom.substr(0, 400).c_str(), n_eff,
                 by_status[AMPLI_AMPLICON_OK], by_status[AMPLI_AMPLICON_FEW], by_status[AMPLI_AMPLICON_DARK], gains, losses);
        std::string summary = b;
        summary += "Sample\tSet\tTotal\tCentre\tK\tBelowCallable\n";
        for (int s = 0; s < S; ++s) {
            int below = 0; // amplicons with a position of the list that is not callable in this file
            for (int i = 0; i < A; ++i) below += cell(s, i)[AMPLI_AMP_CALLABLE] < len_of(i) ? 1 : 0;
            summary += names[(size_t)s] + (s < n_normals ? "\tN\t" : "\tT\t") + std::to_string((long long)total[(size_t)s]) + "\t" +
                       num(kRatio, centre[(size_t)s]) + "\t" + std::to_string(kk[(size_t)s]) + "\t" + std::to_string(below) + "\n";
        }
        write_files(a.output_dir,
                    {{"Amplicon_Reference.txt", reference}, {"Amplicon_Ratios.txt", ratios}, {"Amplicon_Genes.txt", gene_rows}, {"Amplicon_Summary.txt", summary}});
        std::cout << S << " samples, " << A << " amplicons: " << by_status[AMPLI_AMPLICON_OK] << " OK, " << by_status[AMPLI_AMPLICON_FEW] << " FEW, "
                  << by_status[AMPLI_AMPLICON_DARK] << " DARK; " << gains << " (sample, gene) GAIN, " << losses << " LOSS" << std::endl;
        return 0;
    });
}

} // namespace ampli
