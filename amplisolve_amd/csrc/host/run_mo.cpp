// amplisolve_amd/csrc/host/run_mo.cpp -- run_variant_monitoring, one of the project's own command lines
// AmpliSolveVariantMonitoring: tumour-informed monitoring.  `variants` lists list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line
// and `assign` sample<TAB>list per line ("-": none); both are read and checked against the error table and sample_dir before the device
// is opened.  The panel, the thresholds and the reference bases come from the error table alone, as in run_vc.cpp.  The lists, the
// thresholds, the reference bases and the candidates of the control draw stay resident; the files stream chunk by chunk: every chunk's
// sums and scores against every list (ampli_monitor_sums_records, ampli_monitor_score), and for the assigned pairs whose file the chunk
// holds the control replicates in batches (ampli_monitor_control_records), each batch scored on the device and counted on the host.
// Verdict, excess fraction, limit of detection and empirical p are csrc/ampli_math.h's.
#include "command.hpp"

#include <cerrno>
#include <map>

#include "../ampli_math.h"

namespace ampli {

namespace {

std::vector<std::string> mo_fields(std::string line)
{
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::vector<std::string> t;
    for (size_t at = 0;;) {
        const size_t tab = line.find('\t', at);
        t.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
        if (tab == std::string::npos) break;
        at = tab + 1;
    }
    return t;
}

} // namespace

// list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line, and <TAB>weight where `weighted`; refuses a line of another shape (an empty one too), a
// position that is not a whole positive number, a variant off the panel, a ref that is not the table's base, an alt that is no base or
// is the ref, a weight that is not a number in (0, 1], an empty file
VariantLists read_variant_lists(const std::string &path, const Panel &panel, const bool weighted)
{
    std::ifstream f(path);
    if (!f) throw Error{AMPLI_E_INVALID, "variants: cannot read '" + path + "'"};
    std::map<std::string, int> index;
    std::vector<std::vector<uint32_t>> cells;
    std::vector<std::vector<float>> weights;
    VariantLists out;
    std::string line;
    for (int n = 1; std::getline(f, line); ++n) {
        const std::vector<std::string> t = mo_fields(line);
        const std::string at = "variants: line " + std::to_string(n);
        if (t.size() != (weighted ? 6u : 5u) || t[0].empty() || t[1].empty())
            throw Error{AMPLI_E_INVALID, at + " of '" + path + "' is not list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt" + (weighted ? "<TAB>weight" : "")};
        char *end = nullptr;
        errno = 0;
        const long pos = std::strtol(t[2].c_str(), &end, 10);
        if (t[2].empty() || *end || errno || pos <= 0 || pos > INT_MAX || t[2].find_first_not_of("0123456789") != std::string::npos)
            throw Error{AMPLI_E_INVALID, at + ": pos must be a whole positive number, got '" + t[2] + "'"};
        const size_t ref = t[3].size() == 1 ? std::string("ACGT").find(t[3][0]) : std::string::npos;
        const size_t alt = t[4].size() == 1 ? std::string("ACGT").find(t[4][0]) : std::string::npos;
        if (ref == std::string::npos || alt == std::string::npos) throw Error{AMPLI_E_INVALID, at + ": ref and alt must each be one of A, C, G, T, got '" + t[3] + "' and '" + t[4] + "'"};
        if (ref == alt) throw Error{AMPLI_E_INVALID, at + ": alt equals ref ('" + t[3] + "')"};
        float w = 1.0f;
        if (weighted) {
            errno = 0;
            w = std::strtof(t[5].c_str(), &end);
            if (t[5].empty() || *end || errno || t[5].find_first_not_of("0123456789.eE+-") != std::string::npos || !ampli_tf_weight_ok(w))
                throw Error{AMPLI_E_INVALID, at + ": weight must be a number in (0, 1], got '" + t[5] + "'"};
        }
        const int p = panel.find(t[1], (int)pos);
        if (p < 0) throw Error{AMPLI_E_INVALID, at + ": " + t[1] + ":" + t[2] + " is not a position of the error table"};
        if (panel.ref_code[(size_t)p] != (uint8_t)ref)
            throw Error{AMPLI_E_INVALID, at + ": ref '" + t[3] + "' is not the table's base '" + panel.ref_base[(size_t)p] + "' at " + t[1] + ":" + t[2]};
        if (p >= (1 << 30)) throw Error{AMPLI_E_RANGE, at + ": the position index does not fit a list entry"};
        const auto it = index.emplace(t[0], (int)out.names.size());
        if (it.second) { out.names.push_back(t[0]); cells.emplace_back(); weights.emplace_back(); }
        cells[(size_t)it.first->second].push_back((uint32_t)p * 4u + (uint32_t)alt);
        weights[(size_t)it.first->second].push_back(w);
    }
    if (out.names.empty()) throw Error{AMPLI_E_INVALID, "variants: '" + path + "' lists no variant"};
    out.off.push_back(0);
    for (size_t l = 0; l < cells.size(); ++l) {
        out.cell.insert(out.cell.end(), cells[l].begin(), cells[l].end());
        if (weighted) out.w.insert(out.w.end(), weights[l].begin(), weights[l].end());
        out.off.push_back((uint32_t)out.cell.size());
    }
    if (out.cell.size() >= ((size_t)1 << 28)) throw Error{AMPLI_E_RANGE, "variants: more than 2^28 - 1 entries"};
    return out;
}

// sample<TAB>list per line, or "-" for none; refuses a line of another shape, an unknown sample or list
std::vector<std::pair<int, int>> read_assignments(const std::string &path, const FileSet &files, const VariantLists &lists, const std::string &sample_dir)
{
    std::vector<std::pair<int, int>> out;
    if (path == "-") return out;
    std::ifstream f(path);
    if (!f) throw Error{AMPLI_E_INVALID, "assign: cannot read '" + path + "'"};
    std::map<std::string, int> sample, list;
    for (size_t i = 0; i < files.size(); ++i) sample.emplace(files[i].second, (int)i);
    for (size_t i = 0; i < lists.names.size(); ++i) list.emplace(lists.names[i], (int)i);
    std::string line;
    for (int n = 1; std::getline(f, line); ++n) {
        const std::vector<std::string> t = mo_fields(line);
        const std::string at = "assign: line " + std::to_string(n);
        if (t.size() != 2 || t[0].empty() || t[1].empty()) throw Error{AMPLI_E_INVALID, at + " of '" + path + "' is not sample<TAB>list"};
        const auto s = sample.find(t[0]);
        if (s == sample.end()) throw Error{AMPLI_E_INVALID, at + " names '" + t[0] + "', which is no count file of " + sample_dir};
        const auto l = list.find(t[1]);
        if (l == list.end()) throw Error{AMPLI_E_INVALID, at + " names '" + t[1] + "', which is no list of the variants file"};
        out.emplace_back(s->second, l->second);
    }
    return out;
}

namespace {

const char *mo_verdict_name(const int v) { return v == AMPLI_MON_DETECTED ? "DETECTED" : v == AMPLI_MON_NOT_DETECTED ? "NOT_DETECTED" : "NOT_EVALUABLE"; }

} // namespace

int run_variant_monitoring(const MoArgs &a)
{
    return run_command("AmpliSolveVariantMonitoring", [&]() -> int {
        const int cov = parse_int(a.coverage_cutoff, "coverage_cutoff", 0);
        const double q_min = parse_number(a.q_min, "q_min", "in (0, 100]", [](double v) { return v > 0.0 && v <= 100.0; });
        const int min_variants = parse_int(a.min_variants, "min_variants", 1);
        const int min_seen = parse_int(a.min_seen, "min_seen", 0);
        const double max_vaf = parse_number(a.max_vaf, "max_vaf", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        const int max_vaf_pm = (int)std::floor(max_vaf * 1000.0 + 0.5);
        const int R = parse_int(a.controls, "controls", 0, (1 << 30));
        uint64_t seed = 0;
        {
            char *end = nullptr;
            errno = 0;
            seed = std::strtoull(a.seed.c_str(), &end, 10);
            if (a.seed.empty() || *end || errno || a.seed.find_first_not_of("0123456789") != std::string::npos)
                throw Error{AMPLI_E_INVALID, "seed must be an unsigned 64-bit integer, got '" + a.seed + "'"};
        }
        require_single_gpu("AmpliSolveVariantMonitoring");
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
        const VariantLists lists = read_variant_lists(a.variants, panel, false);
        const std::vector<std::pair<int, int>> own = read_assignments(a.assign, files, lists, a.sample_dir);
        const int L = (int)lists.names.size();
        const int64_t W = (int64_t)lists.cell.size();
        long batch_cap = 0; // AMPLISOLVE_MONITOR_BATCH: control replicates of one batch at most (tests; 0 = what 64 MiB hold)
        if (const char *e = getenv("AMPLISOLVE_MONITOR_BATCH")) batch_cap = std::atol(e);
        std::cout << "AmpliSolveVariantMonitoring: table " << a.error_file << ", files " << a.sample_dir << ", variants " << a.variants << " (" << L << " lists, " << W
                  << " entries), assign " << a.assign << " (" << own.size() << " pairs), coverage_cutoff " << cov << ", q_min " << q_min << ", min_variants "
                  << min_variants << ", min_seen " << min_seen << ", max_vaf_pm " << max_vaf_pm << ", controls " << R << ", seed " << seed << ", output "
                  << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        Dev &dev = dev_async.get();

        // resident: thresholds, reference bases, the lists, the candidates of the control draw (every position, grouped by reference base)
        std::vector<uint32_t> cand_off(5, 0), cand_pos;
        for (uint32_t g = 0; g < 4; ++g) {
            for (int64_t p = 0; p < P; ++p)
                if (panel.ref_code[(size_t)p] == g) cand_pos.push_back((uint32_t)p);
            cand_off[g + 1] = (uint32_t)cand_pos.size();
        }
        const int64_t n_cand = (int64_t)cand_pos.size();
        if (cand_pos.empty()) cand_pos.push_back(0);
        const float *d_thr = dev.upload(thr.data(), thr.size());
        const uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
        const uint32_t *d_off = dev.upload(lists.off.data(), lists.off.size());
        const uint32_t *d_cell = dev.upload(lists.cell.data(), lists.cell.size());
        const uint32_t *d_cand_off = dev.upload(cand_off.data(), cand_off.size());
        const uint32_t *d_cand_pos = dev.upload(cand_pos.data(), cand_pos.size());
        const ampli_monitor_params prm = {cov, max_vaf_pm};

        const size_t cells = (size_t)F * (size_t)L;
        std::vector<int64_t> sums(cells * AMPLI_MON_SUMS);
        std::vector<double> lam(cells * 2);
        std::vector<float> q(cells * 2);
        std::vector<long long> n_ge(own.size(), 0);
        DevBuf b_sums, b_lam, b_q, b_pairs, b_cs, b_cl, b_cq;
        std::vector<int32_t> pairs;
        std::vector<size_t> pair_own;
        std::vector<float> cq;
        DevSlot slot;
        int chunks = 0, batches = 0;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &c, int first) {
            ++chunks;
            const size_t n_c = (size_t)c.n * (size_t)L;
            int64_t *d_sums = (int64_t *)b_sums.ensure(dev, n_c * AMPLI_MON_SUMS * 8);
            double *d_lam = (double *)b_lam.ensure(dev, n_c * 16);
            float *d_q = (float *)b_q.ensure(dev, n_c * 8);
            dev.check(dev.api->monitor_sums_records(dev.ctx, &r, P, d_thr, d_ref, d_off, d_cell, L, W, &prm, d_sums, d_lam), "ampli_monitor_sums_records");
            dev.check(dev.api->monitor_score(dev.ctx, d_sums, d_lam, (int64_t)n_c, d_q), "ampli_monitor_score");
            dev.download(sums.data() + (size_t)first * L * AMPLI_MON_SUMS, (const int64_t *)d_sums, n_c * AMPLI_MON_SUMS);
            dev.download(lam.data() + (size_t)first * L * 2, (const double *)d_lam, n_c * 2);
            dev.download(q.data() + (size_t)first * L * 2, (const float *)d_q, n_c * 2);
            dev.sync();
            // the assigned pairs whose file this chunk holds: their control replicates in batches
            pairs.clear();
            pair_own.clear();
            for (size_t k = 0; k < own.size(); ++k)
                if (own[k].first >= first && own[k].first < first + c.n) {
                    pairs.push_back(own[k].first - first);
                    pairs.push_back(own[k].second);
                    pair_own.push_back(k);
                }
            const size_t np = pair_own.size();
            if (!np || R == 0) return;
            size_t per_batch = std::max<size_t>(1, ((size_t)64 << 20) / (np * 72));
            if (batch_cap > 0) per_batch = std::min(per_batch, (size_t)batch_cap);
            per_batch = std::min(per_batch, (size_t)R);
            require_fits(np * per_batch * 72 + np * 8 + 4096, (size_t)64 << 20, device_free_bytes(dev),
                         "a batch of " + std::to_string(per_batch) + " control replicates of " + std::to_string(np) + " pairs does not fit the device");
            int32_t *d_pairs = (int32_t *)b_pairs.ensure(dev, np * 8);
            dev.h2d(d_pairs, pairs.data(), np * 8);
            for (int r0 = 0; r0 < R; r0 += (int)per_batch) {
                const int nb = std::min((int)per_batch, R - r0);
                ++batches;
                const size_t n_k = np * (size_t)nb;
                int64_t *d_cs = (int64_t *)b_cs.ensure(dev, n_k * AMPLI_MON_SUMS * 8);
                double *d_cl = (double *)b_cl.ensure(dev, n_k * 16);
                float *d_cq = (float *)b_cq.ensure(dev, n_k * 8);
                dev.check(dev.api->monitor_control_records(dev.ctx, &r, P, d_thr, d_ref, d_off, d_cell, L, W, d_pairs, (int32_t)np, d_cand_off, d_cand_pos, n_cand, nb,
                                                           r0, seed, &prm, d_cs, d_cl), "ampli_monitor_control_records");
                dev.check(dev.api->monitor_score(dev.ctx, d_cs, d_cl, (int64_t)n_k, d_cq), "ampli_monitor_score");
                cq.resize(n_k * 2);
                dev.download(cq.data(), (const float *)d_cq, n_k * 2);
                dev.sync();
                for (size_t k = 0; k < np; ++k) {
                    const float *o = q.data() + ((size_t)own[pair_own[k]].first * L + (size_t)own[pair_own[k]].second) * 2;
                    const float obs = o[0] < o[1] ? o[0] : o[1];
                    for (int i = 0; i < nb; ++i) {
                        const float *g = cq.data() + (k * (size_t)nb + (size_t)i) * 2;
                        n_ge[pair_own[k]] += (g[0] < g[1] ? g[0] : g[1]) >= obs ? 1 : 0;
                    }
                }
            }
        }, 1);

        // the texts
        std::vector<uint8_t> assigned(cells, 0);
        for (const auto &o : own) assigned[(size_t)o.first * L + (size_t)o.second] = 1;
        std::vector<int> verdict(cells);
        std::vector<long long> other(L, 0);
        char b[768];
        const auto row = [&](const size_t cell) {
            const int64_t *s = sums.data() + cell * AMPLI_MON_SUMS;
            snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%.6f\t%.6f\t%.4f\t%.4f\t%.6g\t%.6g\t%s", (long long)s[0], (long long)s[1], (long long)s[2],
                     (long long)s[3], (long long)s[4], (long long)s[5], lam[cell * 2], lam[cell * 2 + 1], (double)q[cell * 2], (double)q[cell * 2 + 1],
                     ampli_mon_excess(s[AMPLI_MON_K_FW], lam[cell * 2], s[AMPLI_MON_D_FW]), ampli_mon_excess(s[AMPLI_MON_K_BW], lam[cell * 2 + 1], s[AMPLI_MON_D_BW]),
                     mo_verdict_name(verdict[cell]));
            return files[cell / (size_t)L].second + "\t" + lists.names[cell % (size_t)L] + b;
        };
        const std::string head = "sample\tlist\tN_eval\tN_seen\tK_fw\tK_bw\tD_fw\tD_bw\tLambda_fw\tLambda_bw\tQ_fw\tQ_bw\tExcess_fw\tExcess_bw\tVerdict";
        std::string matrix = head + "\n";
        long long matrix_detected = 0, cross_detected = 0;
        for (size_t cell = 0; cell < cells; ++cell) {
            const int64_t *s = sums.data() + cell * AMPLI_MON_SUMS;
            verdict[cell] = ampli_mon_verdict(s[AMPLI_MON_N_EVAL], s[AMPLI_MON_N_SEEN], q[cell * 2], q[cell * 2 + 1], min_variants, min_seen, q_min);
            if (verdict[cell] == AMPLI_MON_DETECTED) {
                ++matrix_detected;
                if (!assigned[cell]) { ++other[cell % (size_t)L]; ++cross_detected; }
            }
            matrix += row(cell) + "\n";
        }
        std::string own_text = head + "\tLoD\tN_ge\tControls\tEmpirical_p\tOther_detected\n";
        long long own_verdicts[3] = {0, 0, 0};
        for (size_t k = 0; k < own.size(); ++k) {
            const size_t cell = (size_t)own[k].first * L + (size_t)own[k].second;
            const int64_t *s = sums.data() + cell * AMPLI_MON_SUMS;
            ++own_verdicts[verdict[cell]];
            const double lod = ampli_mon_lod(lam[cell * 2], lam[cell * 2 + 1], s[AMPLI_MON_D_FW], s[AMPLI_MON_D_BW], q_min);
            own_text += row(cell);
            snprintf(b, sizeof b, "\t%s\t%lld\t%d\t%.6g\t%lld\n", lod < 0.0 ? "NA" : num("%.6g", lod).c_str(), n_ge[k], R, ampli_mon_empirical_p(n_ge[k], R),
                     other[(size_t)own[k].second]);
            own_text += b;
        }
        snprintf(b, sizeof b,
                 "samples=%d\nlists=%d\nentries=%lld\npositions=%lld\nassigned_pairs=%zu\ncoverage_cutoff=%d\nq_min=%g\nmin_variants=%d\nmin_seen=%d\nmax_vaf_pm=%d\n"
                 "controls=%d\nseed=%llu\nmatrix_detected=%lld\nown_detected=%lld\nown_not_detected=%lld\nown_not_evaluable=%lld\ncross_detected=%lld\n",
                 F, L, (long long)W, (long long)P, own.size(), cov, q_min, min_variants, min_seen, max_vaf_pm, R, (unsigned long long)seed, matrix_detected,
                 own_verdicts[AMPLI_MON_DETECTED], own_verdicts[AMPLI_MON_NOT_DETECTED], own_verdicts[AMPLI_MON_NOT_EVALUABLE], cross_detected);
        write_files(a.output_dir, {{"Monitoring_Matrix.txt", matrix}, {"Monitoring_Own.txt", own_text}, {"Monitoring_Summary.txt", b}});
        std::cout << F << " files in " << chunks << " chunks x " << L << " lists, " << own.size() << " assigned pairs x " << R << " controls in " << batches
                  << " batches, " << P << " positions: " << own_verdicts[AMPLI_MON_DETECTED] << " own pairs detected, " << cross_detected
                  << " detections of a list in a sample not assigned to it" << std::endl;
        return 0;
    });
}

} // namespace ampli
