// amplisolve_amd/csrc/host/run_di.cpp -- run_insilico_dilution, one of the project's own command lines
// AmpliSolveInSilicoDilution: an in-silico dilution series.  `mixtures` lists source<TAB>diluent<TAB>fraction[<TAB>scale] per
// line, the names as the Summary names samples, diluent "-" for none; the list is read and checked against sample_dir before the
// device is opened.  Every chunk of sample_dir stays resident; the gate's verdict on the files themselves (ampli_limit_records) gives
// the truth cells of a line -- called in the source and not in the diluent; every line is mixed `replicates` times
// (ampli_dilute_records) in batches, each batch is gated by ampli_limit_records with the table's thresholds, RECHECK cells are settled
// by the host as run_dl.cpp does, and the share of the truth cells still called stands beside the predicted power
// (ampli_power_lod at the expected fraction, on each replicate's own depths and limits).  The two columns are reported side by side;
// nothing here asserts that they agree.
#include "command.hpp"

#include <cerrno>
#include <map>

#include "../ampli_math.h"
#include "../ampli_synth.h"

namespace ampli {

namespace {

struct DiLine {
    int a, b; // files of sample_dir in visit order; b = -1: no diluent
    double fraction, scale;
    uint64_t keep_a, keep_b;
    int line; // of the mixtures file
};

double di_number(const std::string &s, const int line, const char *what, const char *range, bool (*ok)(double))
{
    char *end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (s.empty() || *end || !std::isfinite(v) || !ok(v))
        throw Error{AMPLI_E_INVALID, "mixtures: line " + std::to_string(line) + ": " + what + " must be a number " + range + ", got '" + s + "'"};
    return v;
}

std::vector<DiLine> read_mixtures(const std::string &path, const FileSet &files, const std::string &sample_dir)
{
    std::ifstream f(path);
    if (!f) throw Error{AMPLI_E_INVALID, "mixtures: cannot read '" + path + "'"};
    std::map<std::string, int> index;
    for (size_t i = 0; i < files.size(); ++i) index.emplace(files[i].second, (int)i);
    std::vector<DiLine> out;
    std::string line;
    for (int n = 1; std::getline(f, line); ++n) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::vector<std::string> t;
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            t.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        if (t.size() < 3 || t.size() > 4 || t[0].empty() || t[1].empty())
            throw Error{AMPLI_E_INVALID, "mixtures: line " + std::to_string(n) + " of '" + path + "' is not source<TAB>diluent<TAB>fraction[<TAB>scale]"};
        DiLine d;
        d.line = n;
        d.fraction = di_number(t[2], n, "fraction", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        d.scale = t.size() == 4 ? di_number(t[3], n, "scale", "in (0, 1]", [](double v) { return v > 0.0 && v <= 1.0; }) : 1.0;
        if (t[0] == t[1]) throw Error{AMPLI_E_INVALID, "mixtures: line " + std::to_string(n) + " dilutes '" + t[0] + "' with itself"};
        int idx[2] = {-1, -1};
        for (int k = 0; k < 2; ++k) {
            if (k == 1 && t[1] == "-") continue;
            const auto it = index.find(t[(size_t)k]);
            if (it == index.end())
                throw Error{AMPLI_E_INVALID, "mixtures: line " + std::to_string(n) + " names '" + t[(size_t)k] + "', which is no count file of " + sample_dir};
            idx[k] = it->second;
        }
        d.a = idx[0];
        d.b = idx[1];
        d.keep_a = ampli_dilute_keep(d.fraction * d.scale);          // each product rounded once, in double
        d.keep_b = ampli_dilute_keep((1.0 - d.fraction) * d.scale);
        out.push_back(d);
    }
    if (out.empty()) throw Error{AMPLI_E_INVALID, "mixtures: '" + path + "' lists no mixture"};
    return out;
}

struct DiResident : Resident {
    ampli_records prim; // the chunk's primary records alone: E = 0, no RD plane
};

// the gate's verdict on n rows of primary records: called[row][p][nt], and with `limits` the settled status and minimum reads
struct DiGate {
    std::vector<uint8_t> status;  // [n][P][4], RECHECK settled
    std::vector<int32_t> min_reads; // [n][P][4][2]
};

} // namespace

int run_insilico_dilution(const DiArgs &a)
{
    return run_command("AmpliSolveInSilicoDilution", [&]() -> int {
        const int replicates = parse_int(a.replicates, "replicates", 1, (1 << 20) - 1);
        uint64_t seed = 0;
        {
            char *end = nullptr;
            errno = 0;
            seed = std::strtoull(a.seed.c_str(), &end, 10);
            if (a.seed.empty() || *end || errno || a.seed.find_first_not_of("0123456789") != std::string::npos)
                throw Error{AMPLI_E_INVALID, "seed must be an unsigned 64-bit integer, got '" + a.seed + "'"};
        }
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 1);
        const double conf = parse_number(a.confidence, "confidence", "in [0.5, 0.99]", [](double v) { return v >= 0.5 && v <= 0.99; });
        const int write_counts = parse_int(a.write_counts, "write_counts", 0, 1);
        require_single_gpu("AmpliSolveInSilicoDilution");
        const FileSet files = list_count_files(a.sample_dir, std::string());
        const std::vector<DiLine> lines = read_mixtures(a.mixtures, files, a.sample_dir);
        long batch_cap = 0; // AMPLISOLVE_DILUTION_BATCH: mixtures of one batch at most (tests; 0 = what 256 MiB hold)
        if (const char *e = getenv("AMPLISOLVE_DILUTION_BATCH")) batch_cap = std::atol(e);
        std::cout << "AmpliSolveInSilicoDilution: table " << a.error_file << ", files " << a.sample_dir << ", mixtures " << a.mixtures << " (" << lines.size()
                  << " lines), replicates " << replicates << ", seed " << seed << ", coverage_cutoff " << cov << ", confidence " << conf << ", output "
                  << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        Panel panel;
        std::vector<float> thr;
        panel_from_error_table(a.error_file, std::string(), panel, thr);
        const int64_t P = panel.P();
        if (P <= 0) throw Error{AMPLI_E_INVALID, "the panel has no positions"};
        const int F = (int)files.size();
        Dev &dev = dev_async.get();
        std::vector<DiResident> res;
        std::vector<int32_t> recs((size_t)F * (size_t)P * 8); // every file's primary records, as int32
        const std::vector<DevSlot> slots =
            upload_resident(dev, panel, files, false, 0, (size_t)1 << 30, device_free_bytes(dev), "the files do not fit the device", [&](const Resident &x, Chunk &c) {
                DiResident d{x, x.r};
                d.prim.row_stride = x.r.row_stride > 0 ? x.r.row_stride : (x.r.ext ? P : P + x.r.E);
                d.prim.ext = nullptr; d.prim.ext_stride = 0; d.prim.E = 0; d.prim.dup_off = nullptr; d.prim.ext_pos = nullptr; d.prim.rd = nullptr; d.prim.rd_ext = nullptr;
                res.push_back(d);
                const size_t rb = record_bytes(c.layout);
                for (int s = 0; s < c.n; ++s)
                    for (int64_t p = 0; p < P; ++p)
                        record_unpack(c.layout, (const char *)c.prim + ((size_t)s * (size_t)P + (size_t)p) * rb, recs.data() + ((size_t)(c.first + s) * (size_t)P + (size_t)p) * 8);
            });
        const float *d_thr = dev.upload(thr.data(), thr.size());
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
        std::vector<int> chunk_of((size_t)F, -1);
        for (size_t k = 0; k < res.size(); ++k)
            for (int s = 0; s < res[k].n; ++s) chunk_of[(size_t)(res[k].first + s)] = (int)k;

        // one ampli_limit_records over n rows of primary records, its RECHECK cells settled by the literal scan (run_dl.cpp)
        DevBuf b_min, b_status, b_counts;
        int64_t n_recheck = 0;
        const auto gate = [&](const ampli_records &r, const int n, const int32_t *rows /* [n][P][8] */, DiGate &g) {
            const size_t cells = (size_t)n * (size_t)P * 4;
            int32_t *d_min = (int32_t *)b_min.ensure(dev, cells * 8);
            uint8_t *d_status = (uint8_t *)b_status.ensure(dev, cells);
            int64_t *d_counts = (int64_t *)b_counts.ensure(dev, (size_t)n * AMPLI_LIMIT_COUNTERS * 8);
            dev.check(dev.api->memset_d(dev.ctx, d_counts, 0, (size_t)n * AMPLI_LIMIT_COUNTERS * 8), "memset");
            dev.check(dev.api->limit_records(dev.ctx, &r, P, d_thr, d_ref, cov, nullptr, 0, d_min, d_status, d_counts), "ampli_limit_records");
            g.status.resize(cells);
            g.min_reads.resize(cells * 2);
            dev.download(g.min_reads.data(), (const int32_t *)d_min, cells * 2);
            dev.download(g.status.data(), (const uint8_t *)d_status, cells);
            dev.sync();
            for (size_t cell = 0; cell < cells; ++cell) {
                if (!(g.status[cell] & AMPLI_LIMIT_RECHECK)) continue;
                const size_t rp = cell / 4, p = rp % (size_t)P;
                const int nt = (int)(cell & 3);
                const int32_t *rec = rows + rp * 8;
                const int rd = rec[0] + rec[1] + rec[2] + rec[3] + rec[4] + rec[5] + rec[6] + rec[7];
                const PairLimit h = limit_pair_literal(rec, rd, nt, thr[(size_t)nt * P + p], thr[(size_t)(4 + nt) * P + p], cov);
                g.status[cell] = (uint8_t)(h.status | (h.called ? AMPLI_LIMIT_CALLED : 0));
                g.min_reads[cell * 2] = h.min_fw;
                g.min_reads[cell * 2 + 1] = h.min_bw;
                ++n_recheck;
            }
        };

        // the files themselves: called[file][p][nt]
        std::vector<uint8_t> called((size_t)F * (size_t)P * 4, 0);
        for (const DiResident &r : res) {
            DiGate g;
            gate(r.prim, r.n, recs.data() + (size_t)r.first * (size_t)P * 8, g);
            for (size_t c = 0; c < g.status.size(); ++c) called[(size_t)r.first * (size_t)P * 4 + c] = (g.status[c] & AMPLI_LIMIT_CALLED) ? 1 : 0;
        }

        // a batch: at most 256 MiB of mixtures, at least one, beside 64 MiB of reserve
        const size_t mix_bytes = (size_t)P * 32;
        size_t per_batch = std::max<size_t>(1, ((size_t)256 << 20) / mix_bytes);
        if (batch_cap > 0) per_batch = std::min(per_batch, (size_t)batch_cap);
        per_batch = std::min(per_batch, (size_t)replicates);
        require_fits(per_batch * (mix_bytes + (size_t)P * 4 * 9 + 64) + 4096, (size_t)64 << 20, device_free_bytes(dev),
                     "a batch of " + std::to_string(per_batch) + " mixtures does not fit the device beside the files");
        DevBuf b_mix, b_out, b_flags;
        std::vector<ampli_dilute_mix> mix;
        std::vector<int32_t> out, flags;
        std::string variants = "source\tdiluent\tfraction\tscale\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tVAF\tv_exp\treplicates\tdetected\trate\tpredicted\n";
        std::string per_line = "source\tdiluent\tfraction\tscale\ttruth_cells\tmean_rate\tmean_predicted\tnovel_mean\tnovel_max\tdepth_fw\tdepth_bw\tflagged_records\n";
        long long tot_truth = 0, tot_detected = 0, tot_novel = 0, tot_flagged = 0;
        int batches = 0;
        char b[512];
        if (write_counts) mkdir_p(a.output_dir + "/mixtures");
        for (size_t li = 0; li < lines.size(); ++li) {
            const DiLine &L = lines[li];
            const int32_t *ra = recs.data() + (size_t)L.a * (size_t)P * 8, *rb = L.b >= 0 ? recs.data() + (size_t)L.b * (size_t)P * 8 : nullptr;
            const uint8_t *ca = called.data() + (size_t)L.a * (size_t)P * 4, *cb = L.b >= 0 ? called.data() + (size_t)L.b * (size_t)P * 4 : nullptr;
            std::vector<size_t> truth; // cells p * 4 + nt
            for (size_t c = 0; c < (size_t)P * 4; ++c)
                if (ca[c] && !(cb && cb[c])) truth.push_back(c);
            std::vector<int> detected(truth.size(), 0);
            std::vector<double> predicted(truth.size(), 0.0), v_exp(truth.size(), 0.0);
            for (size_t t = 0; t < truth.size(); ++t) {
                const size_t p = truth[t] / 4;
                const int nt = (int)(truth[t] & 3);
                const int32_t *x = ra + p * 8, *y = rb ? rb + p * 8 : nullptr;
                const bool yb = y && y[0] != AMPLI_ABSENT;
                const double ka = (double)((int64_t)x[nt] + x[4 + nt]), Da = (double)((int64_t)x[0] + x[1] + x[2] + x[3] + x[4] + x[5] + x[6] + x[7]);
                const double kb = yb ? (double)((int64_t)y[nt] + y[4 + nt]) : 0.0;
                const double Db = yb ? (double)((int64_t)y[0] + y[1] + y[2] + y[3] + y[4] + y[5] + y[6] + y[7]) : 0.0;
                const double den = Da * (double)L.keep_a + Db * (double)L.keep_b;
                v_exp[t] = den > 0.0 ? (ka * (double)L.keep_a + kb * (double)L.keep_b) / den : 0.0;
            }
            long long novel_sum = 0, novel_max = 0, flagged = 0, present_records = 0;
            double depth_fw = 0.0, depth_bw = 0.0;
            const DiResident &Ra = res[(size_t)chunk_of[(size_t)L.a]];
            const DiResident *Rb = L.b >= 0 ? &res[(size_t)chunk_of[(size_t)L.b]] : nullptr;
            for (int r0 = 0; r0 < replicates; r0 += (int)per_batch) {
                const int nb = std::min((int)per_batch, replicates - r0);
                ++batches;
                mix.resize((size_t)nb);
                for (int i = 0; i < nb; ++i) {
                    const uint64_t rep = (uint64_t)(r0 + i);
                    const uint64_t key = ampli_splitmix64(seed ^ ampli_splitmix64(((uint64_t)L.a << 40) ^ ((uint64_t)(L.b + 1) << 20) ^ rep));
                    mix[(size_t)i] = ampli_dilute_mix{L.a - Ra.first, Rb ? L.b - Rb->first : -1, L.keep_a, L.keep_b, key};
                }
                ampli_dilute_mix *d_mix = (ampli_dilute_mix *)b_mix.ensure(dev, (size_t)nb * sizeof(ampli_dilute_mix));
                int32_t *d_out = (int32_t *)b_out.ensure(dev, (size_t)nb * mix_bytes);
                int32_t *d_flags = (int32_t *)b_flags.ensure(dev, (size_t)nb * 4);
                dev.h2d(d_mix, mix.data(), (size_t)nb * sizeof(ampli_dilute_mix));
                dev.check(dev.api->dilute_records(dev.ctx, &Ra.prim, Rb ? &Rb->prim : nullptr, P, d_mix, nb, d_out, d_flags), "ampli_dilute_records");
                out.resize((size_t)nb * (size_t)P * 8);
                flags.resize((size_t)nb);
                dev.download(out.data(), (const int32_t *)d_out, out.size());
                dev.download(flags.data(), (const int32_t *)d_flags, flags.size());
                ampli_records mr{};
                mr.recs = d_out; mr.layout = AMPLI_RECORDS_I32; mr.n_samples = nb;
                DiGate g;
                gate(mr, nb, out.data(), g); // synchronises: out and flags are down
                for (int i = 0; i < nb; ++i) {
                    const int32_t *o = out.data() + (size_t)i * (size_t)P * 8;
                    const uint8_t *st = g.status.data() + (size_t)i * (size_t)P * 4;
                    const int32_t *mr2 = g.min_reads.data() + (size_t)i * (size_t)P * 8;
                    long long novel = 0;
                    for (int64_t p = 0; p < P; ++p) {
                        const int32_t *x = o + p * 8;
                        if (x[0] == AMPLI_ABSENT) {
                            if (flags[(size_t)i] && ra[p * 8] != AMPLI_ABSENT && !(rb && rb[p * 8] == AMPLI_ABSENT)) ++flagged; // absent for a bad count
                            continue;
                        }
                        ++present_records;
                        depth_fw += (double)((int64_t)x[0] + x[1] + x[2] + x[3]);
                        depth_bw += (double)((int64_t)x[4] + x[5] + x[6] + x[7]);
                        for (int nt = 0; nt < 4; ++nt)
                            if ((st[p * 4 + nt] & AMPLI_LIMIT_CALLED) && !ca[p * 4 + nt] && !(cb && cb[p * 4 + nt])) ++novel;
                    }
                    novel_sum += novel;
                    novel_max = std::max(novel_max, novel);
                    for (size_t t = 0; t < truth.size(); ++t) {
                        const size_t c = truth[t], p = c / 4;
                        if (st[c] & AMPLI_LIMIT_CALLED) ++detected[t];
                        if ((st[c] & 7) == AMPLI_LIMIT_OK && v_exp[t] > 0.0) {
                            const int32_t *x = o + p * 8;
                            const int FW = x[0] + x[1] + x[2] + x[3], BW = x[4] + x[5] + x[6] + x[7];
                            const float level = (float)v_exp[t];
                            double pw = 0.0;
                            ampli_power_lod(FW, mr2[c * 2], BW, mr2[c * 2 + 1], &level, 1, conf, &pw, nullptr, nullptr, nullptr);
                            predicted[t] += pw;
                        }
                    }
                    if (write_counts) {
                        snprintf(b, sizeof b, "/mixtures/L%03zu_R%04d.PILEUP.ASEQ", li + 1, r0 + i);
                        std::ofstream f(a.output_dir + b);
                        f << "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n";
                        for (int64_t p = 0; p < P; ++p) {
                            const int32_t *x = o + p * 8;
                            if (x[0] == AMPLI_ABSENT) continue;
                            const int64_t tA = (int64_t)x[0] + x[4], tC = (int64_t)x[1] + x[5], tG = (int64_t)x[2] + x[6], tT = (int64_t)x[3] + x[7];
                            f << panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] << "\t" << panel.pos_coord[(size_t)p] << "\t.\t.\t.\t.\t" << tA << "\t" << tC << "\t" << tG
                              << "\t" << tT << "\t" << tA + tC + tG + tT << "\t" << x[4] << "\t" << x[5] << "\t" << x[6] << "\t" << x[7] << "\n";
                        }
                        f.close();
                        if (f.fail()) throw Error{AMPLI_E_INVALID, std::string("could not write ") + b};
                    }
                }
            }
            const std::string head = files[(size_t)L.a].second + "\t" + (L.b >= 0 ? files[(size_t)L.b].second : std::string("-")) + "\t" + num("%g", L.fraction) + "\t" +
                                     num("%g", L.scale);
            double rate_sum = 0.0, pred_sum = 0.0;
            for (size_t t = 0; t < truth.size(); ++t) {
                const size_t p = truth[t] / 4;
                const int nt = (int)(truth[t] & 3);
                const int32_t *x = ra + p * 8;
                const long long FW = (long long)x[0] + x[1] + x[2] + x[3], BW = (long long)x[4] + x[5] + x[6] + x[7];
                const double rate = (double)detected[t] / (double)replicates, pred = predicted[t] / (double)replicates;
                rate_sum += rate;
                pred_sum += pred;
                tot_detected += detected[t];
                snprintf(b, sizeof b, "\t%d\t%c->%c\t%d\t%d\t%lld\t%lld\t%.6f\t%.6f\t%d\t%d\t%.6f\t%.6f\n", panel.pos_coord[p], "ACGT"[panel.ref_code[p]], "ACGT"[nt], x[nt],
                         x[4 + nt], FW, BW, FW + BW ? (double)((long long)x[nt] + x[4 + nt]) / (double)(FW + BW) : 0.0, v_exp[t], replicates, detected[t], rate, pred);
                variants += head + "\t" + panel.chroms[(size_t)panel.pos_chrom[p]] + b;
            }
            const double nt_ = (double)truth.size();
            snprintf(b, sizeof b, "\t%zu\t%s\t%s\t%.6f\t%lld\t%.2f\t%.2f\t%lld\n", truth.size(), num("%.6f", truth.empty() ? NAN : rate_sum / nt_).c_str(),
                     num("%.6f", truth.empty() ? NAN : pred_sum / nt_).c_str(), (double)novel_sum / (double)replicates, novel_max,
                     present_records ? depth_fw / (double)present_records : 0.0, present_records ? depth_bw / (double)present_records : 0.0, flagged);
            per_line += head + b;
            tot_truth += (long long)truth.size();
            tot_novel += novel_sum;
            tot_flagged += flagged;
        }
        snprintf(b, sizeof b, "lines=%zu\nmixtures=%lld\npositions=%lld\nreplicates=%d\nseed=%llu\ncoverage_cutoff=%d\nconfidence=%g\ntruth_cells=%lld\ndetected=%lld\n"
                              "novel=%lld\nflagged_records=%lld\n",
                 lines.size(), (long long)lines.size() * replicates, (long long)P, replicates, (unsigned long long)seed, cov, conf, tot_truth, tot_detected, tot_novel, tot_flagged);
        write_files(a.output_dir, {{"Dilution_Variants.txt", variants}, {"Dilution_Lines.txt", per_line}, {"Dilution_Summary.txt", b}});
        std::cout << lines.size() << " lines x " << replicates << " replicates of " << F << " files in " << res.size() << " chunks, " << batches << " batches, " << P
                  << " positions: " << tot_truth << " truth cells, " << tot_detected << " detections, " << tot_novel << " novel cells, " << n_recheck
                  << " cells settled on the host" << std::endl;
        return 0;
    });
}

} // namespace ampli
