// amplisolve_amd/csrc/host/run_od.cpp -- run_overdispersed_calling, one of the project's own command lines
// AmpliSolveOverdispersedCalling: the dispersion omega of every cell of the panel of normals, and every tumour cell scored
// twice with the panel's own error table -- under the Poisson law (omega = 0 everywhere) and under the negative binomial with the
// fitted omega -- to say which cells that pass the Poisson gate at q_min no longer pass.  The normals stay resident on the device, as
// in run_pd.cpp: the reduce with C_value and its finalize (the table), the reduce with C = 0 (the totals), dispersion's two calls
// (X2, status) and the two of the fit (S2, omega).  The tumours stream chunk by chunk; each chunk is scored twice and both arrays come
// down.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

int run_overdispersed_calling(const OdArgs &a)
{
    return run_command("AmpliSolveOverdispersedCalling", [&]() -> int {
        const double C_value = parse_number(a.C_value, "C_value", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 1);
        const int call_cov = parse_int(a.calling_cutoff, "calling_cutoff", 0);
        char *end = nullptr;
        const double z_cutoff = std::strtod(a.z_cutoff.c_str(), &end); // as AmpliSolvePanelDispersion takes it
        if (a.z_cutoff.empty() || *end || !std::isfinite(z_cutoff)) throw Error{AMPLI_E_INVALID, "z_cutoff must be a number, got '" + a.z_cutoff + "'"};
        const double q_min = parse_number(a.q_min, "q_min", "in (0, 100]", [](double v) { return v > 0.0 && v <= 100.0; });
        require_single_gpu("AmpliSolveOverdispersedCalling");
        std::cout << "AmpliSolveOverdispersedCalling: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours " << a.tumour_dir << ", C_value "
                  << C_value << ", coverage_cutoff " << cov << ", calling_cutoff " << call_cov << ", z_cutoff " << z_cutoff << ", q_min " << q_min << ", output "
                  << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, &a.reference_genome, a.refbases_file, a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const int64_t P = in.P;
        const FileSet &files = in.sets[1];
        const int F = (int)files.size();
        Dev &dev = dev_async.get();
        // every chunk of the normals stays resident: refuse before the device runs out (beside them two tables, the planes, one chunk of tumours)
        std::vector<Resident> res;
        upload_resident(dev, panel, in.sets[0], false, 4, 2 * dev.api->acc_bytes(P) + (size_t)P * 8 * 60 + ((size_t)1 << 30), device_free_bytes(dev),
                        "the normals do not fit the device", [&](const Resident &x, Chunk &) { res.push_back(x); });
        const size_t cells = (size_t)P * 8;
        ampli_acc_table acc{}, acc0{};
        dev.check(dev.api->acc_bind(dev.alloc<char>(dev.api->acc_bytes(P)), P, &acc), "ampli_acc_bind");
        dev.check(dev.api->acc_bind(dev.alloc<char>(dev.api->acc_bytes(P)), P, &acc0), "ampli_acc_bind");
        float *d_rate = dev.alloc<float>(cells), *d_thr = dev.alloc<float>(cells), *d_germ = dev.alloc<float>((size_t)P * 4);
        uint8_t *d_code = dev.alloc<uint8_t>((size_t)P * 4), *d_gp = dev.alloc<uint8_t>((size_t)P * 4), *d_status = dev.alloc<uint8_t>(cells);
        int32_t *d_flags = dev.alloc<int32_t>(16);
        double *d_x2 = dev.alloc<double>(cells), *d_rinv = dev.alloc<double>(cells), *d_z = dev.alloc<double>(cells), *d_s2 = dev.alloc<double>(cells),
               *d_omega = dev.alloc<double>(cells);
        float *d_phi = dev.alloc<float>(cells);
        int64_t *d_counts = dev.alloc<int64_t>(4);
        // 1. the table of the whole panel (thr), 2. its totals with C = 0; the general kernel where a depth asks for it
        for (int attempt = 0; attempt < 2; ++attempt) {
            for (size_t k = 0; k < res.size(); ++k) {
                dev.check(dev.api->error_reduce_records(dev.ctx, &res[k].r, P, res[k].first, (float)C_value, cov, &acc, k ? AMPLI_REDUCE_ACCUMULATE : 0, nullptr,
                                                        nullptr, nullptr, nullptr, nullptr, nullptr), "ampli_error_reduce_records");
                dev.check(dev.api->error_reduce_records(dev.ctx, &res[k].r, P, res[k].first, 0.0f, cov, &acc0, (k ? AMPLI_REDUCE_ACCUMULATE : 0) | AMPLI_REDUCE_SUMMARY,
                                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "ampli_error_reduce_records");
            }
            if (!(dev.flags() & AMPLI_FLAG_RERUN_GENERAL)) break;
            dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning");
        }
        dev.check(dev.api->memset_d(dev.ctx, d_flags, 0, sizeof(int32_t) * 16), "memset");
        dev.check(dev.api->error_finalize(dev.ctx, &acc, (float)C_value, cov, d_rate, d_code, d_thr, d_germ, d_gp, d_flags), "ampli_error_finalize");
        // 3. dispersion's two calls, 4. the two of the fit
        for (size_t k = 0; k < res.size(); ++k) {
            dev.check(dev.api->dispersion_records(dev.ctx, &res[k].r, P, &acc0, cov, d_x2, d_rinv, k ? 1 : 0, nullptr, nullptr, nullptr), "ampli_dispersion_records");
            dev.check(dev.api->overdispersion_records(dev.ctx, &res[k].r, P, &acc0, cov, d_s2, k ? 1 : 0), "ampli_overdispersion_records");
        }
        dev.check(dev.api->memset_d(dev.ctx, d_counts, 0, sizeof(int64_t) * 4), "memset");
        dev.check(dev.api->dispersion_finalize(dev.ctx, P, &acc0, d_x2, d_rinv, z_cutoff, d_z, d_phi, d_status, d_counts), "ampli_dispersion_finalize");
        dev.check(dev.api->overdispersion_finalize(dev.ctx, P, &acc0, d_x2, d_s2, d_status, d_omega), "ampli_overdispersion_finalize");
        std::vector<double> snt(cells), x2(cells), z(cells), omega(cells);
        std::vector<int64_t> srd(cells);
        std::vector<int32_t> cnt((size_t)P * 4);
        dev.download(snt.data(), (const double *)acc0.snt, cells);
        dev.download(srd.data(), (const int64_t *)acc0.srd, cells);
        dev.download(cnt.data(), (const int32_t *)acc0.cnt, (size_t)P * 4);
        dev.download(x2.data(), (const double *)d_x2, cells);
        dev.download(z.data(), (const double *)d_z, cells);
        dev.download(omega.data(), (const double *)d_omega, cells);
        dev.sync();
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());

        // Overdispersed_Cells.txt: every cell with omega > 0
        char b[512];
        std::string cellsf = "chrom\tposition\tref\tbase\tstrand\tN\tAltReads\tDepth\tX2\tZ\tOmega\n";
        long long cells_fitted = 0;
        for (int64_t p = 0; p < P; ++p)
            for (int nt = 0; nt < 4; ++nt)
                for (int s = 0; s < 2; ++s) {
                    const size_t o = (size_t)(s * 4 + nt) * (size_t)P + (size_t)p;
                    if (!(omega[o] > 0.0)) continue;
                    ++cells_fitted;
                    snprintf(b, sizeof b, "\t%c\t%c\t%d\t%lld\t%lld\t%.6f\t%.4f\t%.6g\n", "ACGT"[nt], s ? '-' : '+', cnt[(size_t)nt * P + p], (long long)snt[o],
                             (long long)srd[o], x2[o], z[o], omega[o]);
                    cellsf += panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + "\t" + std::to_string(panel.pos_coord[(size_t)p]) + "\t" + panel.ref_base[(size_t)p] + b;
                }

        // the tumours: each chunk scored twice, both arrays down, the gate at q_min on the host
        std::string calls = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tQ0_fw\tQ0_rs\tOmega_fw\tOmega_rs\tQ_fw\tQ_rs\tVerdict\n";
        std::vector<long long> evaluated_of((size_t)F, 0), poisson_of((size_t)F, 0), kept_of((size_t)F, 0);
        DevBuf b_q0, b_q;
        std::vector<float> q0, q;
        DevSlot slot;
        int tumour_chunks = 0;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &c, int) {
            ++tumour_chunks;
            const size_t n_q = (size_t)c.n * (size_t)P * 8;
            float *d_q0 = (float *)b_q0.ensure(dev, n_q * sizeof(float)), *d_q = (float *)b_q.ensure(dev, n_q * sizeof(float));
            dev.check(dev.api->nb_score_records(dev.ctx, &r, P, d_thr, nullptr, d_ref, call_cov, d_q0), "ampli_nb_score_records");
            dev.check(dev.api->nb_score_records(dev.ctx, &r, P, d_thr, d_omega, d_ref, call_cov, d_q), "ampli_nb_score_records");
            q0.resize(n_q);
            q.resize(n_q);
            dev.download(q0.data(), (const float *)d_q0, n_q);
            dev.download(q.data(), (const float *)d_q, n_q);
            dev.sync();
            const size_t rb = record_bytes(c.layout);
            for (int s = 0; s < c.n; ++s) {
                const size_t f = (size_t)(c.first + s);
                for (int64_t p = 0; p < P; ++p) {
                    const size_t cell = (size_t)s * (size_t)P + (size_t)p;
                    for (int y = 0; y < 4; ++y) {
                        const float *g0 = q0.data() + cell * 8 + 2 * y, *g = q.data() + cell * 8 + 2 * y;
                        if (g0[0] == AMPLI_NB_NA) continue; // not evaluated: with omega == NULL nothing else gives NA on the forward strand
                        ++evaluated_of[f];
                        if (!((double)g0[0] >= q_min && (double)g0[1] >= q_min)) continue;
                        ++poisson_of[f];
                        const bool kept = (double)g[0] >= q_min && (double)g[1] >= q_min;
                        kept_of[f] += kept ? 1 : 0;
                        int32_t rec[8];
                        record_unpack(c.layout, (const char *)c.prim + cell * rb, rec);
                        const long long d_fw = (long long)rec[0] + rec[1] + rec[2] + rec[3], d_bw = (long long)rec[4] + rec[5] + rec[6] + rec[7];
                        const size_t o_fw = (size_t)y * (size_t)P + (size_t)p, o_bw = (size_t)(4 + y) * (size_t)P + (size_t)p;
                        snprintf(b, sizeof b, "\t%d\t%c->%c\t%d\t%d\t%lld\t%lld\t%.4f\t%.4f\t%.6g\t%.6g\t%.4f\t%.4f\t%s\n", panel.pos_coord[(size_t)p],
                                 "ACGT"[panel.ref_code[(size_t)p]], "ACGT"[y], rec[y], rec[4 + y], d_fw, d_bw, (double)g0[0], (double)g0[1], omega[o_fw], omega[o_bw],
                                 (double)g[0], (double)g[1], kept ? "KEPT" : "DROPPED");
                        calls += files[f].second + "\t" + panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + b;
                    }
                }
            }
        }, 1);

        std::string samples = "sample\tEvaluated\tPoisson\tKept\tDropped\n";
        long long evaluated = 0, n_poisson = 0, n_kept = 0;
        for (int f = 0; f < F; ++f) {
            samples += files[(size_t)f].second + "\t" + std::to_string(evaluated_of[(size_t)f]) + "\t" + std::to_string(poisson_of[(size_t)f]) + "\t" +
                       std::to_string(kept_of[(size_t)f]) + "\t" + std::to_string(poisson_of[(size_t)f] - kept_of[(size_t)f]) + "\n";
            evaluated += evaluated_of[(size_t)f];
            n_poisson += poisson_of[(size_t)f];
            n_kept += kept_of[(size_t)f];
        }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\npositions=%lld\nC_value=%g\ncoverage_cutoff=%d\ncalling_cutoff=%d\nz_cutoff=%g\nq_min=%g\ncells_fitted=%lld\n"
                 "evaluated=%lld\npoisson=%lld\nkept=%lld\ndropped=%lld\n",
                 in.n_normals, in.n_tumours, (long long)P, C_value, cov, call_cov, z_cutoff, q_min, cells_fitted, evaluated, n_poisson, n_kept, n_poisson - n_kept);
        write_files(a.output_dir, {{"Overdispersed_Calls.txt", calls}, {"Overdispersed_Cells.txt", cellsf}, {"Overdispersed_Samples.txt", samples},
                                   {"Overdispersed_Summary.txt", b}});
        std::cout << F << " tumours in " << tumour_chunks << " chunks against " << in.n_normals << " normals in " << res.size() << " chunks, " << P
                  << " positions: " << cells_fitted << " overdispersed cells, " << n_poisson
                  << " cells pass the Poisson gate, " << n_poisson - n_kept << " of them dropped" << std::endl;
        return 0;
    });
}

} // namespace ampli
