// amplisolve_amd/csrc/host/run_fd.cpp -- run_false_discovery, one of the project's own command lines
// AmpliSolveFalseDiscovery: every tumour cell scored with the exact Poisson tail (ampli_nb_score_records with omega NULL)
// against the panel's own error table, the Benjamini-Hochberg adjusted score of every cell per file (ampli_fdr_adjust), and the cells
// whose adjusted score A reaches a_min = -10 log10(fdr) -- beside what the raw per-strand gate at q_min lets through, so that the
// difference between the two is a number.  The normals stay resident for the table, as in run_od.cpp's step 1; the tumours stream
// chunk by chunk; a chunk's rows are adjusted in batches whose workspace fits the device beside 64 MiB of reserve.  The scores come
// down with the adjusted values: FDR_Samples.txt counts the raw gate in every file, listed cells or not.
#include "command.hpp"

#include "../ampli_math.h"

namespace ampli {

int run_false_discovery(const FdArgs &a)
{
    return run_command("AmpliSolveFalseDiscovery", [&]() -> int {
        const double C_value = parse_number(a.C_value, "C_value", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 1);
        const int call_cov = parse_int(a.calling_cutoff, "calling_cutoff", 0);
        const double fdr = parse_number(a.fdr, "fdr", "in (0, 1)", [](double v) { return v > 0.0 && v < 1.0; });
        const double q_min = parse_number(a.q_min, "q_min", "in (0, 100]", [](double v) { return v > 0.0 && v <= 100.0; });
        require_single_gpu("AmpliSolveFalseDiscovery");
        (void)list_count_files(a.tumour_dir, std::string()); // an empty tumour directory is refused before the device is opened
        const double a_min = -10.0 * log10(fdr);
        long batch_rows_env = 0; // AMPLISOLVE_FDR_BATCH_ROWS: rows of one ampli_fdr_adjust call at most (tests; 0 = what fits)
        if (const char *e = getenv("AMPLISOLVE_FDR_BATCH_ROWS")) batch_rows_env = parse_int(e, "AMPLISOLVE_FDR_BATCH_ROWS", 1);
        std::cout << "AmpliSolveFalseDiscovery: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours " << a.tumour_dir << ", C_value "
                  << C_value << ", coverage_cutoff " << cov << ", calling_cutoff " << call_cov << ", fdr " << fdr << " (A >= " << num("%.6g", a_min) << "), q_min "
                  << q_min << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, &a.reference_genome, a.refbases_file, a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const int64_t P = in.P;
        const FileSet &files = in.sets[1];
        const int F = (int)files.size();
        Dev &dev = dev_async.get();
        if (P >= ((int64_t)1 << 29)) throw Error{AMPLI_E_RANGE, "the panel has 2^29 positions or more: a file's cells cannot be ranked in 32 bits"};
        const size_t cells = (size_t)P * 8;
        ampli_acc_table acc{};
        float *d_thr = nullptr;
        {
            // the table of the whole panel, as run_od.cpp's step 1: the normals resident, the general kernel where a depth asks for it
            std::vector<Resident> res;
            const std::vector<DevSlot> slots = upload_resident(dev, panel, in.sets[0], false, 4, dev.api->acc_bytes(P) + (size_t)P * 8 * 12 + ((size_t)1 << 30),
                                                               device_free_bytes(dev), "the normals do not fit the device",
                                                               [&](const Resident &x, Chunk &) { res.push_back(x); });
            dev.check(dev.api->acc_bind(dev.alloc<char>(dev.api->acc_bytes(P)), P, &acc), "ampli_acc_bind");
            float *d_rate = dev.alloc<float>(cells), *d_germ = dev.alloc<float>((size_t)P * 4);
            d_thr = dev.alloc<float>(cells);
            uint8_t *d_code = dev.alloc<uint8_t>((size_t)P * 4), *d_gp = dev.alloc<uint8_t>((size_t)P * 4);
            int32_t *d_flags = dev.alloc<int32_t>(16);
            for (int attempt = 0; attempt < 2; ++attempt) {
                for (size_t k = 0; k < res.size(); ++k)
                    dev.check(dev.api->error_reduce_records(dev.ctx, &res[k].r, P, res[k].first, (float)C_value, cov, &acc, k ? AMPLI_REDUCE_ACCUMULATE : 0, nullptr,
                                                            nullptr, nullptr, nullptr, nullptr, nullptr), "ampli_error_reduce_records");
                if (!(dev.flags() & AMPLI_FLAG_RERUN_GENERAL)) break;
                dev.check(dev.api->set_tuning(dev.ctx, 0, 1, 0), "ampli_set_tuning");
            }
            dev.check(dev.api->memset_d(dev.ctx, d_flags, 0, sizeof(int32_t) * 16), "memset");
            dev.check(dev.api->error_finalize(dev.ctx, &acc, (float)C_value, cov, d_rate, d_code, d_thr, d_germ, d_gp, d_flags), "ampli_error_finalize");
            dev.sync();
        }
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());

        std::string calls = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tQ_fw\tQ_rs\tKey\tA\tq\tRank\tRawGate\n";
        std::vector<long long> tested_of((size_t)F, 0), raw_of((size_t)F, 0), adj_of((size_t)F, 0), raw_only_of((size_t)F, 0);
        std::vector<double> min_key_of((size_t)F, NAN);
        DevBuf b_q, b_a, b_m, b_rank, b_work;
        std::vector<float> q, adj;
        std::vector<int32_t> m, rank;
        DevSlot slot;
        char b[512];
        int tumour_chunks = 0, batches = 0;
        long largest_batch = 0;
        const size_t row_work = dev.api->fdr_workspace_bytes(1, P);
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &c, int) {
            ++tumour_chunks;
            const size_t n_cells = (size_t)c.n * (size_t)P * 4;
            float *d_q = (float *)b_q.ensure(dev, n_cells * 2 * sizeof(float)), *d_a = (float *)b_a.ensure(dev, n_cells * sizeof(float));
            int32_t *d_m = (int32_t *)b_m.ensure(dev, (size_t)c.n * sizeof(int32_t)), *d_rank = (int32_t *)b_rank.ensure(dev, n_cells * sizeof(int32_t));
            dev.check(dev.api->nb_score_records(dev.ctx, &r, P, d_thr, nullptr, d_ref, call_cov, d_q), "ampli_nb_score_records");
            // rows per call: what the device has left beside the reserve (and beside the workspace already held), or fewer when asked
            long rows = c.n;
            if (batch_rows_env) rows = std::min<long>(rows, batch_rows_env);
            if ((size_t)rows * row_work > b_work.cap) {
                const size_t free_b = device_free_bytes(dev) + b_work.cap, reserve = (size_t)64 << 20;
                require_fits(row_work, reserve, free_b, "the workspace of one file's false-discovery adjustment (" + std::to_string(row_work) +
                                                            " bytes) does not fit the device beside the scores");
                rows = std::min<long>(rows, (long)((free_b - reserve) / row_work));
            }
            void *d_work = b_work.ensure(dev, (size_t)rows * row_work);
            for (long r0 = 0; r0 < c.n; r0 += rows) {
                const long nr = std::min<long>(rows, c.n - r0);
                ++batches;
                largest_batch = std::max(largest_batch, nr);
                dev.check(dev.api->fdr_adjust(dev.ctx, d_q + (size_t)r0 * (size_t)P * 8, (int32_t)nr, P, 0, d_work, (size_t)rows * row_work,
                                              d_a + (size_t)r0 * (size_t)P * 4, d_m + r0, d_rank + (size_t)r0 * (size_t)P * 4), "ampli_fdr_adjust");
            }
            q.resize(n_cells * 2);
            adj.resize(n_cells);
            rank.resize(n_cells);
            m.resize((size_t)c.n);
            dev.download(q.data(), (const float *)d_q, n_cells * 2);
            dev.download(adj.data(), (const float *)d_a, n_cells);
            dev.download(rank.data(), (const int32_t *)d_rank, n_cells);
            dev.download(m.data(), (const int32_t *)d_m, (size_t)c.n);
            dev.sync();
            const size_t rb = record_bytes(c.layout);
            for (int s = 0; s < c.n; ++s) {
                const size_t f = (size_t)(c.first + s);
                tested_of[f] = m[(size_t)s];
                for (int64_t p = 0; p < P; ++p) {
                    const size_t cell = (size_t)s * (size_t)P + (size_t)p;
                    for (int y = 0; y < 4; ++y) {
                        const float *g = q.data() + cell * 8 + 2 * y;
                        const float A = adj[cell * 4 + (size_t)y];
                        if (A == AMPLI_FDR_NA) continue;
                        const bool raw = (double)g[0] >= q_min && (double)g[1] >= q_min, found = (double)A >= a_min;
                        raw_of[f] += raw ? 1 : 0;
                        raw_only_of[f] += raw && !found ? 1 : 0;
                        if (!found) continue;
                        ++adj_of[f];
                        const double key = (double)(g[0] < g[1] ? g[0] : g[1]);
                        if (!(min_key_of[f] <= key)) min_key_of[f] = key;
                        int32_t rec[8];
                        record_unpack(c.layout, (const char *)c.prim + cell * rb, rec);
                        const long long d_fw = (long long)rec[0] + rec[1] + rec[2] + rec[3], d_bw = (long long)rec[4] + rec[5] + rec[6] + rec[7];
                        snprintf(b, sizeof b, "\t%d\t%c->%c\t%d\t%d\t%lld\t%lld\t%.6f\t%.6f\t%.6f\t%.6f\t%.6g\t%d\t%s\n", panel.pos_coord[(size_t)p],
                                 "ACGT"[panel.ref_code[(size_t)p]], "ACGT"[y], rec[y], rec[4 + y], d_fw, d_bw, (double)g[0], (double)g[1], key, (double)A,
                                 pow(10.0, -(double)A / 10.0), rank[cell * 4 + (size_t)y], raw ? "PASS" : "FAIL");
                        calls += files[f].second + "\t" + panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + b;
                    }
                }
            }
        }, 1);

        std::string samples = "sample\tTested\tRawGate\tAdjusted\tRawOnly\tMinKey\n";
        long long tested = 0, n_raw = 0, n_adj = 0, n_raw_only = 0;
        for (int f = 0; f < F; ++f) {
            const size_t i = (size_t)f;
            samples += files[i].second + "\t" + std::to_string(tested_of[i]) + "\t" + std::to_string(raw_of[i]) + "\t" + std::to_string(adj_of[i]) + "\t" +
                       std::to_string(raw_only_of[i]) + "\t" + num("%.6f", min_key_of[i]) + "\n";
            tested += tested_of[i];
            n_raw += raw_of[i];
            n_adj += adj_of[i];
            n_raw_only += raw_only_of[i];
        }
        snprintf(b, sizeof b,
                 "normals=%d\ntumours=%d\npositions=%lld\nC_value=%g\ncoverage_cutoff=%d\ncalling_cutoff=%d\nfdr=%g\na_min=%.6g\nq_min=%g\ntested=%lld\n"
                 "raw_gate=%lld\nadjusted=%lld\nraw_only=%lld\n",
                 in.n_normals, in.n_tumours, (long long)P, C_value, cov, call_cov, fdr, a_min, q_min, tested, n_raw, n_adj, n_raw_only);
        write_files(a.output_dir, {{"FDR_Calls.txt", calls}, {"FDR_Samples.txt", samples}, {"FDR_Summary.txt", b}});
        std::cout << F << " tumours in " << tumour_chunks << " chunks against " << in.n_normals << " normals, " << P << " positions: adjusted in " << batches
                  << " batches of at most " << largest_batch << " rows (AMPLISOLVE_FDR_BATCH_ROWS), " << tested << " cells tested, " << n_raw
                  << " pass the raw gate, " << n_adj << " pass at fdr " << fdr << ", " << n_raw_only << " pass the raw gate only" << std::endl;
        return 0;
    });
}

} // namespace ampli
