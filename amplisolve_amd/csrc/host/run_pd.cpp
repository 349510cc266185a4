// amplisolve_amd/csrc/host/run_pd.cpp -- run_panel_dispersion, one of the project's own command lines
// AmpliSolvePanelDispersion: per (position, base, strand) of the panel of normals, Pearson's statistic of the qualifying
// records' alternative counts against the pooled rate the error table would use, its z-score under Haldane's exact moments, and per
// normal its share of the statistic against the null mean.  The cohort is loaded and streamed as run_loo.cpp does: every chunk stays
// resident on the device; pass 1 is the reduce with C = 0 over the chunks (the totals), pass 2 one dispersion launch per chunk.
#include "command.hpp"

namespace ampli {

int run_panel_dispersion(const PdArgs &a)
{
    return run_command("AmpliSolvePanelDispersion", [&]() -> int {
        int cov = std::atoi(a.coverage_cutoff.c_str());
        if (cov <= 0) cov = 100; // EE:380-388
        char *end = nullptr;
        const double z_cutoff = std::strtod(a.z_cutoff.c_str(), &end);
        if (a.z_cutoff.empty() || *end || !std::isfinite(z_cutoff)) throw Error{AMPLI_E_INVALID, "z_cutoff must be a number, got '" + a.z_cutoff + "'"};
        require_single_gpu("AmpliSolvePanelDispersion");
        std::cout << "AmpliSolvePanelDispersion: panel " << a.panel_design << ", normals " << a.germline_dir << ", coverage_cutoff " << cov
                  << ", z_cutoff " << z_cutoff << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        Panel panel;
        panel_from_bed(a.panel_design, panel);
        if (!a.refbases_file.empty()) panel_load_refbases_file(panel, a.refbases_file);
        else panel_load_fasta(panel, a.reference_genome);
        const auto files = list_count_files(a.germline_dir, std::string());
        const int S = (int)files.size();
        if (S == 0) throw Error{AMPLI_E_INVALID, "no count files in " + a.germline_dir};
        const int64_t P = panel.P();
        Dev &dev = dev_async.get();
        const size_t free_b = device_free_bytes(dev);
        // every chunk stays resident: refuse before the device runs out (the records, plus the table, the planes and the partials)
        std::vector<Resident> res;
        upload_resident(dev, panel, files, false, 4, dev.api->acc_bytes(P) + (size_t)P * 8 * 30 + ((size_t)64 << 20), free_b,
                        "the cohort does not fit the device", [&](const Resident &x, Chunk &) { res.push_back(x); });
        void *d_accbuf = dev.alloc<char>(dev.api->acc_bytes(P));
        ampli_acc_table acc{};
        dev.check(dev.api->acc_bind(d_accbuf, P, &acc), "ampli_acc_bind");
        const size_t cells = (size_t)P * 8;
        double *d_x2 = dev.alloc<double>(cells), *d_rinv = dev.alloc<double>(cells), *d_z = dev.alloc<double>(cells);
        float *d_phi = dev.alloc<float>(cells);
        uint8_t *d_status = dev.alloc<uint8_t>(cells);
        int64_t *d_counts = dev.alloc<int64_t>(4);
        double *d_sx = dev.alloc<double>((size_t)S), *d_se = dev.alloc<double>((size_t)S);
        int64_t *d_st = dev.alloc<int64_t>((size_t)S);
        // 1. the whole cohort's totals: with C = 0 snt is K exactly, srd is D, cnt is n; the general kernel where a depth asks for it
        for (int attempt = 0; attempt < 2; ++attempt) {
            for (size_t k = 0; k < res.size(); ++k)
                dev.check(dev.api->error_reduce_records(dev.ctx, &res[k].r, P, res[k].first, 0.0f, cov, &acc, (k ? AMPLI_REDUCE_ACCUMULATE : 0) | AMPLI_REDUCE_SUMMARY,
                                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "ampli_error_reduce_records");
            if (!(dev.flags() & AMPLI_FLAG_RERUN_GENERAL)) break;
            dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning");
        }
        // 2. one dispersion launch per resident chunk, then the finalize
        for (size_t k = 0; k < res.size(); ++k)
            dev.check(dev.api->dispersion_records(dev.ctx, &res[k].r, P, &acc, cov, d_x2, d_rinv, k ? 1 : 0, d_sx + res[k].first, d_se + res[k].first,
                                                  d_st + res[k].first), "ampli_dispersion_records");
        dev.check(dev.api->memset_d(dev.ctx, d_counts, 0, sizeof(int64_t) * 4), "memset");
        dev.check(dev.api->dispersion_finalize(dev.ctx, P, &acc, d_x2, d_rinv, z_cutoff, d_z, d_phi, d_status, d_counts), "ampli_dispersion_finalize");
        std::vector<double> snt(cells), x2(cells), z(cells), sx((size_t)S), se((size_t)S);
        std::vector<int64_t> srd(cells), st((size_t)S), counts(4);
        std::vector<int32_t> cnt((size_t)P * 4);
        std::vector<float> phi(cells);
        std::vector<uint8_t> status(cells);
        dev.download(snt.data(), (const double *)acc.snt, cells);
        dev.download(srd.data(), (const int64_t *)acc.srd, cells);
        dev.download(cnt.data(), (const int32_t *)acc.cnt, (size_t)P * 4);
        dev.download(x2.data(), (const double *)d_x2, cells);
        dev.download(z.data(), (const double *)d_z, cells);
        dev.download(phi.data(), (const float *)d_phi, cells);
        dev.download(status.data(), (const uint8_t *)d_status, cells);
        dev.download(counts.data(), (const int64_t *)d_counts, 4);
        dev.download(sx.data(), (const double *)d_sx, (size_t)S);
        dev.download(se.data(), (const double *)d_se, (size_t)S);
        dev.download(st.data(), (const int64_t *)d_st, (size_t)S);
        dev.sync();
        // 3. the three files
        std::string cellsf = "Chrom\tPosition\tRef\tBase\tStrand\tN\tAltReads\tDepth\tX2\tPhi\tZ\tFlag\n";
        char b[512];
        for (int64_t p = 0; p < P; ++p)
            for (int nt = 0; nt < 4; ++nt)
                for (int s = 0; s < 2; ++s) {
                    const size_t o = (size_t)(s * 4 + nt) * (size_t)P + (size_t)p;
                    if ((status[o] & 7) != AMPLI_DISPERSION_OK) continue;
                    snprintf(b, sizeof b, "\t%c\t%c\t%d\t%lld\t%lld\t%.6f\t%.4f\t%.4f\t%s\n", "ACGT"[nt], s ? '-' : '+', cnt[(size_t)nt * P + p],
                             (long long)snt[o], (long long)srd[o], x2[o], (double)phi[o], z[o], status[o] & AMPLI_DISPERSION_HIGH ? "HIGH" : ".");
                    cellsf += panel.chroms[panel.pos_chrom[p]] + "\t" + std::to_string(panel.pos_coord[p]) + "\t" + panel.ref_base[p] + b;
                }
        std::string samples = "Sample\tTerms\tX2\tExpected\tRatio\n";
        for (int s = 0; s < S; ++s) {
            char ratio[64] = "NA";
            if (se[(size_t)s] != 0) snprintf(ratio, sizeof ratio, "%.4f", sx[(size_t)s] / se[(size_t)s]);
            snprintf(b, sizeof b, "\t%lld\t%.6f\t%.6f\t%s\n", (long long)st[(size_t)s], sx[(size_t)s], se[(size_t)s], ratio);
            samples += files[(size_t)s].second + b;
        }
        snprintf(b, sizeof b, "normals=%d\ncoverage_cutoff=%d\nz_cutoff=%g\ncells_ok=%lld\ncells_few=%lld\ncells_high=%lld\npositions_high=%lld\n", S, cov,
                 z_cutoff, (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3]);
        write_files(a.output_dir, {{"panelDispersion.txt", cellsf}, {"panelDispersion_samples.txt", samples}, {"panelDispersion_summary.txt", b}});
        std::cout << counts[0] << " cells OK, " << counts[1] << " with too few reads or records, " << counts[2] << " HIGH at " << counts[3] << " positions"
                  << std::endl;
        return 0;
    });
}

} // namespace ampli
