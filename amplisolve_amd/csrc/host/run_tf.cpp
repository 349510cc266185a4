// amplisolve_amd/csrc/host/run_tf.cpp -- run_tumour_fraction, one of the project's own command lines
// AmpliSolveTumourFraction: how much of a patient's tumour a plasma sample holds, within what bounds, and whether it changed
// since the last draw.  `variants` lists list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt<TAB>weight per line and `assign` sample<TAB>list per
// line ("-": none); both are read and checked against the error table and sample_dir before the device is opened (the readers are
// run_mo.cpp's).  The panel, the thresholds and the reference bases come from the error table alone.  The lists, the weights, the
// thresholds and the reference bases stay resident; the files stream chunk by chunk, each chunk writing its rows of one matrix
// (ampli_fraction_records), so chunking changes no byte.  Verdict and change are csrc/ampli_math.h's.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

namespace {

const char *tf_verdict_name(const int v) { return v == AMPLI_TF_QUANTIFIED ? "QUANTIFIED" : v == AMPLI_TF_BELOW ? "BELOW" : "NOT_EVALUABLE"; }

const char *tf_change_name(const int v)
{
    return v == AMPLI_TF_RISING ? "RISING" : v == AMPLI_TF_FALLING ? "FALLING" : v == AMPLI_TF_STABLE ? "STABLE" : "NOT_EVALUABLE";
}

// a value of the four, AMPLI_TF_NA as NA
std::string tf_num(const double x) { return x == AMPLI_TF_NA ? std::string("NA") : num("%.6g", x); }

} // namespace

int run_tumour_fraction(const TfArgs &a)
{
    return run_command("AmpliSolveTumourFraction", [&]() -> int {
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 0);
        const int min_variants = parse_int(a.min_variants, "min_variants", 1);
        const double max_vaf = parse_number(a.max_vaf, "max_vaf", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        const int max_vaf_pm = (int)std::floor(max_vaf * 1000.0 + 0.5);
        const double confidence = parse_number(a.confidence, "confidence", "among 0.90, 0.95, 0.99", [](double v) { return v == 0.90 || v == 0.95 || v == 0.99; });
        const double z2 = confidence == 0.90 ? AMPLI_TF_Z2_90 : confidence == 0.95 ? AMPLI_TF_Z2_95 : AMPLI_TF_Z2_99;
        require_single_gpu("AmpliSolveTumourFraction");
        // everything the command can refuse on its own is refused before the device is opened
        CohortInputs in;
        std::vector<float> thr;
        panel_from_error_table(a.error_file, std::string(), in.panel, thr);
        const Panel &panel = in.panel;
        const int64_t P = panel.P();
        if (P <= 0) throw Error{AMPLI_E_INVALID, "the panel has no positions"};
        in.sets[1] = list_count_files(a.sample_dir, std::string());
        const FileSet &files = in.sets[1];
        const int F = (int)files.size();
        if (F == 0) throw Error{AMPLI_E_INVALID, "no count files in " + a.sample_dir};
        in.n_tumours = F;
        in.P = P;
        const VariantLists lists = read_variant_lists(a.variants, panel, true);
        const std::vector<std::pair<int, int>> own = read_assignments(a.assign, files, lists, a.sample_dir);
        const int L = (int)lists.names.size();
        const int64_t W = (int64_t)lists.cell.size();
        std::cout << "AmpliSolveTumourFraction: table " << a.error_file << ", files " << a.sample_dir << ", variants " << a.variants << " (" << L << " lists, " << W
                  << " entries), assign " << a.assign << " (" << own.size() << " pairs), coverage_cutoff " << cov << ", min_variants " << min_variants
                  << ", max_vaf_pm " << max_vaf_pm << ", confidence " << num("%.2f", confidence) << " (z2 " << z2 << "), output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        Dev &dev = dev_async.get();

        // resident: thresholds, reference bases, the lists and their weights
        const float *d_thr = dev.upload(thr.data(), thr.size());
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
        const uint32_t *d_off = dev.upload(lists.off.data(), lists.off.size());
        const uint32_t *d_cell = dev.upload(lists.cell.data(), lists.cell.size());
        const float *d_w = dev.upload(lists.w.data(), lists.w.size());
        const ampli_fraction_params prm = {cov, max_vaf_pm, z2};

        const size_t cells = (size_t)F * (size_t)L;
        std::vector<double> est(cells * AMPLI_TF_VALS);
        std::vector<int64_t> count(cells * AMPLI_TF_COUNTS);
        require_fits(cells * (AMPLI_TF_VALS + AMPLI_TF_COUNTS) * 8 + 4096, (size_t)64 << 20, device_free_bytes(dev),
                     "the matrix of " + std::to_string(F) + " files x " + std::to_string(L) + " lists does not fit the device");
        DevBuf b_est, b_count;
        double *d_est = (double *)b_est.ensure(dev, cells * AMPLI_TF_VALS * 8);
        int64_t *d_count = (int64_t *)b_count.ensure(dev, cells * AMPLI_TF_COUNTS * 8);
        DevSlot slot;
        int chunks = 0;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &c, int first) {
            ++chunks;
            (void)c;
            dev.check(dev.api->fraction_records(dev.ctx, &r, P, d_thr, d_ref, d_off, d_cell, d_w, L, W, &prm, d_est + (size_t)first * L * AMPLI_TF_VALS,
                                                d_count + (size_t)first * L * AMPLI_TF_COUNTS), "ampli_fraction_records");
        }, 1);
        dev.download(est.data(), (const double *)d_est, est.size());
        dev.download(count.data(), (const int64_t *)d_count, count.size());
        dev.sync();

        // the texts
        std::vector<int> verdict(cells);
        char b[768];
        const auto row = [&](const size_t cell) {
            const double *v = est.data() + cell * AMPLI_TF_VALS;
            snprintf(b, sizeof b, "\t%lld\t%lld\t%s\t%s\t%s\t%s\t%s", (long long)count[cell * 2], (long long)count[cell * 2 + 1], tf_num(v[AMPLI_TF_F_HAT]).c_str(),
                     tf_num(v[AMPLI_TF_F_LO]).c_str(), tf_num(v[AMPLI_TF_F_HI]).c_str(),
                     v[AMPLI_TF_F_HAT] == AMPLI_TF_NA ? "NA" : num("%.6g", v[AMPLI_TF_T0]).c_str(), tf_verdict_name(verdict[cell]));
            return files[cell / (size_t)L].second + "\t" + lists.names[cell % (size_t)L] + b;
        };
        const std::string head = "sample\tlist\tN_eval\tN_seen\tF_hat\tF_lo\tF_hi\tT0\tVerdict";
        std::string matrix = head + "\n";
        long long matrix_quantified = 0;
        for (size_t cell = 0; cell < cells; ++cell) {
            const double *v = est.data() + cell * AMPLI_TF_VALS;
            verdict[cell] = ampli_tf_verdict(count[cell * 2 + AMPLI_TF_N_EVAL], v[AMPLI_TF_F_HAT], v[AMPLI_TF_F_LO], min_variants);
            matrix_quantified += verdict[cell] == AMPLI_TF_QUANTIFIED;
            matrix += row(cell) + "\n";
        }
        std::string own_text = head + "\n";
        long long own_verdicts[3] = {0, 0, 0};
        for (const auto &o : own) {
            const size_t cell = (size_t)o.first * L + (size_t)o.second;
            ++own_verdicts[verdict[cell]];
            own_text += row(cell) + "\n";
        }
        // consecutive lines of assign that name the same list are consecutive draws of one patient
        std::string change_text = "list\tsample_a\tsample_b\tF_hat_a\tF_lo_a\tF_hi_a\tF_hat_b\tF_lo_b\tF_hi_b\tRatio\tChange\n";
        long long changes[4] = {0, 0, 0, 0};
        for (size_t k = 1; k < own.size(); ++k) {
            if (own[k].second != own[k - 1].second) continue;
            const size_t ca = (size_t)own[k - 1].first * L + (size_t)own[k].second, cb = (size_t)own[k].first * L + (size_t)own[k].second;
            const double *va = est.data() + ca * AMPLI_TF_VALS, *vb = est.data() + cb * AMPLI_TF_VALS;
            double ratio;
            const int ch = ampli_tf_change(verdict[ca], va, verdict[cb], vb, &ratio);
            ++changes[ch];
            change_text += lists.names[(size_t)own[k].second] + "\t" + files[(size_t)own[k - 1].first].second + "\t" + files[(size_t)own[k].first].second + "\t" +
                           tf_num(va[AMPLI_TF_F_HAT]) + "\t" + tf_num(va[AMPLI_TF_F_LO]) + "\t" + tf_num(va[AMPLI_TF_F_HI]) + "\t" + tf_num(vb[AMPLI_TF_F_HAT]) + "\t" +
                           tf_num(vb[AMPLI_TF_F_LO]) + "\t" + tf_num(vb[AMPLI_TF_F_HI]) + "\t" + tf_num(ratio) + "\t" + tf_change_name(ch) + "\n";
        }
        snprintf(b, sizeof b,
                 "samples=%d\nlists=%d\nentries=%lld\npositions=%lld\nassigned_pairs=%zu\ncoverage_cutoff=%d\nmin_variants=%d\nmax_vaf_pm=%d\nconfidence=%.2f\n"
                 "z2=%g\nmatrix_quantified=%lld\nown_quantified=%lld\nown_below=%lld\nown_not_evaluable=%lld\nchanges=%lld\nrising=%lld\nfalling=%lld\nstable=%lld\n"
                 "change_not_evaluable=%lld\n",
                 F, L, (long long)W, (long long)P, own.size(), cov, min_variants, max_vaf_pm, confidence, z2, matrix_quantified, own_verdicts[AMPLI_TF_QUANTIFIED],
                 own_verdicts[AMPLI_TF_BELOW], own_verdicts[AMPLI_TF_NOT_EVALUABLE], changes[0] + changes[1] + changes[2] + changes[3], changes[AMPLI_TF_RISING],
                 changes[AMPLI_TF_FALLING], changes[AMPLI_TF_STABLE], changes[AMPLI_TF_CHANGE_NOT_EVALUABLE]);
        write_files(a.output_dir, {{"Fraction_Matrix.txt", matrix}, {"Fraction_Own.txt", own_text}, {"Fraction_Change.txt", change_text}, {"Fraction_Summary.txt", b}});
        std::cout << F << " files in " << chunks << " chunks x " << L << " lists, " << own.size() << " assigned pairs, " << P << " positions: "
                  << own_verdicts[AMPLI_TF_QUANTIFIED] << " own pairs quantified, " << changes[AMPLI_TF_RISING] << " rising and " << changes[AMPLI_TF_FALLING]
                  << " falling of " << changes[0] + changes[1] + changes[2] + changes[3] << " changes" << std::endl;
        return 0;
    });
}

} // namespace ampli
