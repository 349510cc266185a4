// amplisolve_amd/csrc/host/run_loo.cpp -- run_leave_one_out, one of the project's own command lines
// AmpliSolveLeaveOneOut: for every normal of germline_dir, the calling gate on its own file against the error table of the
// other S-1 normals, for each C of a list.  Every chunk of the cohort stays resident on the device; per C one reduce over the chunks,
// one leave-one-out launch per chunk, the emitted pairs re-scored with the reference's operation sequence, three files.
#include "command.hpp"

namespace ampli {

namespace {
struct LooRow : CallBase { long double q_fw, q_bw; float thr_fw, thr_bw; int code; };
struct LooResident : Resident { // a chunk that stays on the device, with what maps its records back to lines and positions (record_line)
    int64_t P, E;
    std::vector<uint32_t> ext_pos;
    std::vector<int32_t> line_prim, line_ext;
};
std::string thr_text(float thr, int code)
{
    if (code) return "0.01"; // EE:2680-2684
    char b[64];
    snprintf(b, sizeof b, "%f", thr); // EE:1704: the table's text of the rate, which reads back as thr
    return b;
}
} // namespace

int run_leave_one_out(const LooArgs &a)
{
    return run_command("AmpliSolveLeaveOneOut", [&]() -> int {
        std::vector<float> Cs;
        {
            std::stringstream ss(a.C_value);
            for (std::string t; std::getline(ss, t, ',');) {
                float c = (float)std::atof(t.c_str());
                Cs.push_back(c <= 0 ? 0.002f : c); // EE:372-388
            }
            if (Cs.empty()) Cs.push_back(0.002f);
        }
        int cov = std::atoi(a.coverage_cutoff.c_str());
        if (cov <= 0) cov = 100; // EE:380-388
        int call_cov = std::atoi(a.calling_cutoff.c_str());
        if (call_cov <= 0) call_cov = 100; // VC:262-275
        require_single_gpu("AmpliSolveLeaveOneOut");
        std::cout << "AmpliSolveLeaveOneOut: panel " << a.panel_design << ", normals " << a.germline_dir << ", coverage_cutoff " << cov
                  << ", calling_cutoff " << call_cov << ", output " << a.output_dir << std::endl;
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
        // every chunk stays resident: refuse before the device runs out (the records, plus the table, masks and lists the passes add)
        std::vector<LooResident> res;
        std::vector<DevSlot> slots =
            upload_resident(dev, panel, files, true, 5, dev.api->acc_bytes(P) + ((size_t)64 << 20), free_b, "the cohort does not fit the device",
                            [&](const Resident &x, Chunk &c) { res.push_back(LooResident{x, P, c.E, c.ext_pos, c.line_prim, c.line_ext}); });
        uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
        void *d_accbuf = dev.alloc<char>(dev.api->acc_bytes(P));
        ampli_acc_table acc{};
        dev.check(dev.api->acc_bind(d_accbuf, P, &acc), "ampli_acc_bind");
        int32_t *d_cpos = dev.alloc<int32_t>((size_t)P), *d_csam = dev.alloc<int32_t>((size_t)S), *d_flags = dev.alloc<int32_t>(1);
        unsigned long long *d_n = alloc_call_counters(dev);
        mkdir_p(a.output_dir);
        struct Out { std::string calls, positions, samples, line; };
        std::vector<Out> outs;
        for (const float C : Cs) {
            // 1. the whole cohort's sums (streaming state is enough: snt / srd / cnt / nrec are exact), the general kernel where a depth asks for it
            for (int attempt = 0; attempt < 2; ++attempt) {
                for (size_t k = 0; k < res.size(); ++k)
                    dev.check(dev.api->error_reduce_records(dev.ctx, &res[k].r, P, res[k].first, C, cov, &acc,
                                                            (k ? AMPLI_REDUCE_ACCUMULATE : 0) | AMPLI_REDUCE_SUMMARY, nullptr, nullptr, nullptr,
                                                            nullptr, nullptr, nullptr), "ampli_error_reduce_records");
                if (!(dev.flags() & AMPLI_FLAG_RERUN_GENERAL)) break;
                dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning");
            }
            dev.check(dev.api->memset_d(dev.ctx, d_cpos, 0, sizeof(int32_t) * (size_t)P), "memset");
            dev.check(dev.api->memset_d(dev.ctx, d_csam, 0, sizeof(int32_t) * (size_t)S), "memset");
            dev.check(dev.api->memset_d(dev.ctx, d_flags, 0, sizeof(int32_t)), "memset");
            // 2. one leave-one-out launch per resident chunk
            std::vector<LooRow> rows;
            for (size_t k = 0; k < res.size(); ++k) {
                const LooResident &x = res[k];
                const int64_t R = P + x.E;
                uint8_t *d_mask = (uint8_t *)slots[k].mask.ensure(dev, (size_t)x.n * R + 4);
                std::vector<int32_t> cpos_before((size_t)P);
                const char *why = collect_calls<ampli_loo_call>(
                    dev, x.n, R, d_n,
                    [&](ampli_loo_call *d_calls, int64_t cap, int) {
                        // the callable counts are added to: a repeated attempt must not count twice
                        dev.download(cpos_before.data(), d_cpos, (size_t)P);
                        dev.sync();
                        dev.check(dev.api->loo_call_records(dev.ctx, &x.r, P, &acc, C, cov, call_cov, d_ref, AMPLI_POISSON_PREFILTER, d_mask, d_calls, cap, d_n,
                                                            d_cpos, d_csam + x.first, nullptr, d_flags), "ampli_loo_call_records");
                    },
                    [&] {
                        dev.h2d(d_cpos, cpos_before.data(), sizeof(int32_t) * (size_t)P);
                        dev.check(dev.api->memset_d(dev.ctx, d_csam + x.first, 0, sizeof(int32_t) * (size_t)x.n), "memset");
                        dev.sync();
                    },
                    [&](const ampli_loo_call &lc) { rows.push_back(LooRow{call_base(x, lc.call), 0, 0, lc.thr_fw, lc.thr_bw, lc.code}); });
                if (why) throw Error{AMPLI_E_CAPACITY, "the leave-one-out pass did not complete: call list or queue still overflowing"};
            }
            int32_t env = 0;
            dev.download(&env, d_flags, 1);
            dev.sync();
            if (env & 1) { // outside the exactness envelope the S-1 sums are not the totals minus one sample: refuse before writing anything
                std::vector<double> snt((size_t)P * 8);
                dev.download(snt.data(), acc.snt, snt.size());
                dev.sync();
                int ex = 0;
                const float pmin = (float)cov * C;
                (void)frexpf(pmin > 0 ? pmin : 1.0f, &ex);
                const double limit = std::ldexp(1.0, ex - 24) * 9007199254740992.0 * 0.5; // envelope_limit
                int64_t bad = 0;
                for (int64_t p = 0; p < P; ++p) {
                    bool b = false;
                    for (int j = 0; j < 8; ++j) b |= !(snt[(size_t)j * P + p] < limit);
                    bad += b ? 1 : 0;
                }
                throw Error{AMPLI_E_ENVELOPE, "the threshold sums of " + std::to_string(bad) + " position(s) are outside the exactness envelope at C=" +
                                                  std::to_string(C) + ", coverage_cutoff=" + std::to_string(cov) +
                                                  ": leave-one-out is not supported there (DESIGN 10); no file was written"};
            }
            // 3. every emitted pair re-scored with the reference's operation sequence and its own S-1 thresholds (VC:895-898)
            std::vector<LooRow> kept;
            for (LooRow &r : rows) {
                r.q_fw = score_reference_sequence(r.k_fw, r.rd - r.bw, r.thr_fw);
                r.q_bw = score_reference_sequence(r.k_bw, r.bw, r.thr_bw);
                if (r.q_fw >= 5 && r.q_bw >= 5) kept.push_back(r);
            }
            std::sort(kept.begin(), kept.end(), EmissionOrder{});
            std::vector<int32_t> cpos((size_t)P), csam((size_t)S);
            dev.download(cpos.data(), d_cpos, cpos.size());
            dev.download(csam.data(), d_csam, csam.size());
            dev.sync();
            // 4. the three files (text first, written once every C has passed its checks)
            char cb[32];
            snprintf(cb, sizeof cb, "%.4f", C);
            Out o;
            std::ostringstream calls, positions, samples;
            calls << std::setprecision(4);
            calls << "sample\tchrom\tposition\tsubstitution\tRD\tFW\tBW\tAF\tXfw\tXrs\tAF_fw\tAF_bw\tQ_fw\tQ_bw\tThr_fw\tThr_bw\n";
            std::vector<int64_t> calls_pos((size_t)P * 4, 0), calls_sam((size_t)S, 0);
            for (const LooRow &r : kept) {
                calls << files[(size_t)r.sample].second << "\t" << panel.chroms[panel.pos_chrom[r.p]] << "\t" << panel.pos_coord[r.p] << "\t"
                      << "ACGT"[panel.ref_code[r.p]] << "->" << "ACGT"[r.alt] << "\t" << r.rd << "\t" << r.fw << "\t" << r.bw << "\t" << r.af << "\t"
                      << r.k_fw << "\t" << r.k_bw << "\t" << r.af_fw << "\t" << r.af_bw << "\t" << (double)r.q_fw << "\t" << (double)r.q_bw << "\t"
                      << thr_text(r.thr_fw, r.code) << "\t" << thr_text(r.thr_bw, r.code) << "\n";
                ++calls_pos[(size_t)r.p * 4 + r.alt];
                ++calls_sam[(size_t)r.sample];
            }
            positions << "chrom\tposition\treference\tduplicate\tCallable\tCalls_A\tCalls_C\tCalls_G\tCalls_T\n";
            int64_t n_callable = 0, multi = 0;
            for (int64_t p = 0; p < P; ++p) {
                positions << panel.chroms[panel.pos_chrom[p]] << "\t" << panel.pos_coord[p] << "\t" << panel.ref_base[p] << (panel.dup[p] ? "\tYES" : "\tNO")
                          << "\t" << cpos[(size_t)p];
                for (int nt = 0; nt < 4; ++nt) positions << "\t" << calls_pos[(size_t)p * 4 + nt];
                positions << "\n";
                n_callable += cpos[(size_t)p];
            }
            // positions called in >= 2 normals
            {
                std::vector<int> last((size_t)P, -1), cnt((size_t)P, 0);
                for (const LooRow &r : kept)
                    if (last[(size_t)r.p] != r.sample) { last[(size_t)r.p] = r.sample; ++cnt[(size_t)r.p]; }
                for (int64_t p = 0; p < P; ++p) multi += cnt[(size_t)p] >= 2 ? 1 : 0;
            }
            samples << "sample\tCallable\tCalls\tCalls_per_1000\n";
            for (int s = 0; s < S; ++s) {
                char per[64];
                snprintf(per, sizeof per, "%.4f", csam[(size_t)s] ? 1000.0 * (double)calls_sam[(size_t)s] / (double)csam[(size_t)s] : 0.0);
                samples << files[(size_t)s].second << "\t" << csam[(size_t)s] << "\t" << calls_sam[(size_t)s] << "\t" << per << "\n";
            }
            o.calls = calls.str(); o.positions = positions.str(); o.samples = samples.str();
            o.line = std::string("C=") + cb + ": " + std::to_string(kept.size()) + " calls in " + std::to_string(n_callable) + " callable records, " +
                     std::to_string(multi) + " positions called in >= 2 normals";
            outs.push_back(std::move(o));
        }
        for (size_t i = 0; i < Cs.size(); ++i) {
            char cb[32];
            snprintf(cb, sizeof cb, "%.4f", Cs[i]);
            const std::string base = a.output_dir + "/leaveOneOut_" + cb;
            std::ofstream(base + "_calls.txt") << outs[i].calls;
            std::ofstream(base + "_positions.txt") << outs[i].positions;
            std::ofstream(base + "_samples.txt") << outs[i].samples;
            std::cout << outs[i].line << std::endl;
        }
        return 0;
    });
}

} // namespace ampli
