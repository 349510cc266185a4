// amplisolve_amd/csrc/host/run_dp.cpp -- run_detection_power, one of the project's own command lines
// AmpliSolveDetectionPower: for every line of every tumour file and every base other than the reference base, the probability
// that a variant at each given allele fraction passes the calling gate on that line's own depths, and the allele fraction that passes
// with the given confidence (the limit of detection).  Streams as run_detection_limits does: one ampli_limit_records per chunk, the
// cells the device leaves open (RECHECK) settled by the literal scan, the settled cells uploaded again, one ampli_power_records; one
// file per tumour file and a summary.  The probabilities are the device's: 28 M pairs at config 3 are not scored twice.
#include <algorithm>

#include "command.hpp"

namespace ampli {

namespace {
const char *dp_name(int status)
{
    return status == AMPLI_LIMIT_OK ? "OK" : status == AMPLI_LIMIT_LOWDEPTH ? "LOWDEPTH" : status == AMPLI_LIMIT_NOESTIMATE ? "NOESTIMATE" : "UNREACHABLE";
}
struct DpCounts { int64_t lines = 0, pairs = 0, ok = 0; double median_lod = 0; std::vector<int64_t> lev; };
} // namespace

int run_detection_power(const DpArgs &a)
{
    return run_command("AmpliSolveDetectionPower", [&]() -> int {
        int cov = std::atoi(a.coverage_cutoff.c_str());
        if (cov <= 0) cov = 100; // VC:262-275
        std::vector<float> levels;
        std::vector<std::string> level_text;
        {
            std::stringstream ss(a.levels);
            for (std::string t; std::getline(ss, t, ',');) {
                char *end = nullptr;
                const float v = std::strtof(t.c_str(), &end);
                if (t.empty() || end == t.c_str() || *end || !(v > 0 && v <= 1)) throw Error{AMPLI_E_INVALID, "levels: '" + t + "' is not an allele fraction in (0, 1]"};
                levels.push_back(v);
                level_text.push_back(t);
            }
            if (levels.empty() || levels.size() > AMPLI_POWER_MAX_LEVELS) throw Error{AMPLI_E_INVALID, "levels: one to 8 allele fractions are required"};
        }
        float conf = 0;
        {
            char *end = nullptr;
            conf = std::strtof(a.confidence.c_str(), &end);
            if (a.confidence.empty() || end == a.confidence.c_str() || *end || !(conf >= 0.5f && conf <= 0.99f))
                throw Error{AMPLI_E_INVALID, "confidence: '" + a.confidence + "' is not a probability in [0.5, 0.99]"};
        }
        const int L = (int)levels.size(), NC = 1 + L, NLC = AMPLI_LIMIT_COUNTERS;
        require_single_gpu("AmpliSolveDetectionPower");
        std::cout << "AmpliSolveDetectionPower: table " << a.error_file << ", tumours " << a.tumour_dir << ", coverage_cutoff " << cov << ", confidence "
                  << conf << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start(); // beside the reading of the error table
        mkdir_p(a.output_dir);
        Panel panel;
        std::vector<float> thr;
        panel_from_error_table(a.error_file, std::string(), panel, thr); // VC:320
        const auto files = list_count_files(a.tumour_dir, std::string());
        const int T = (int)files.size();
        if (T == 0) throw Error{AMPLI_E_INVALID, "no count files in " + a.tumour_dir};
        const int64_t P = panel.P();
        std::vector<DpCounts> tot((size_t)T);
        int64_t n_recheck = 0;
        {
            const std::unique_ptr<ChunkStream> cs = open_stream(panel, files, true);
            Dev &dev = dev_async.get();
            float *d_thr = dev.upload(thr.data(), thr.size());
            uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
            float *d_levels = dev.upload(levels.data(), levels.size());
            DevSlot dslots[kDevSlots];
            DevBuf d_min_b, d_status_b, d_lcounts_b, d_power_b, d_lod_b, d_counts_b;
            std::vector<int32_t> min_reads;
            std::vector<uint8_t> status;
            std::vector<float> power, lod;
            std::vector<int64_t> counts;
            for (Chunk *c; (c = cs->next()) != nullptr;) {
                const ampli_records r = upload_chunk(dev, dslots[c->slot % kDevSlots], *c, true);
                const int64_t R = P + c->E;
                const size_t cells = (size_t)c->n * (size_t)R * 4;
                int32_t *d_min = (int32_t *)d_min_b.ensure(dev, cells * 8);
                uint8_t *d_status = (uint8_t *)d_status_b.ensure(dev, cells);
                int64_t *d_lcounts = (int64_t *)d_lcounts_b.ensure(dev, (size_t)c->n * NLC * 8);
                float *d_power = (float *)d_power_b.ensure(dev, cells * (size_t)L * 4);
                float *d_lod = (float *)d_lod_b.ensure(dev, cells * 4);
                int64_t *d_counts = (int64_t *)d_counts_b.ensure(dev, (size_t)c->n * NC * 8);
                dev.check(dev.api->memset_d(dev.ctx, d_lcounts, 0, (size_t)c->n * NLC * 8), "memset");
                dev.check(dev.api->memset_d(dev.ctx, d_counts, 0, (size_t)c->n * NC * 8), "memset");
                dev.check(dev.api->limit_records(dev.ctx, &r, P, d_thr, d_ref, cov, nullptr, 0, d_min, d_status, d_lcounts), "ampli_limit_records");
                min_reads.resize(cells * 2);
                status.resize(cells);
                dev.download(min_reads.data(), d_min, cells * 2);
                dev.download(status.data(), d_status, cells);
                dev.sync();
                // the RD column of the lines that carry their own (VC:762-765)
                std::unordered_map<uint64_t, int32_t> own_rd;
                for (const Irregular &x : c->irregular) own_rd[(uint64_t)x.sample * (uint64_t)R + (uint64_t)x.record] = x.rd;
                const size_t rb = record_bytes(c->layout);
                auto unpack = [&](int i, int64_t rr, int32_t rec[8]) {
                    record_unpack(c->layout, rr < P ? (const char *)c->prim + ((size_t)i * P + rr) * rb
                                                    : (const char *)c->ext + ((size_t)i * c->E + (rr - P)) * rb, rec);
                };
                // settle what the device left open, then hand the settled cells back
                int64_t open_cells = 0;
                for (size_t cell = 0; cell < cells; ++cell) {
                    if (!(status[cell] & AMPLI_LIMIT_RECHECK)) continue;
                    const int nt = (int)(cell & 3);
                    const int64_t rr = (int64_t)((cell >> 2) % (size_t)R);
                    const int i = (int)((cell >> 2) / (size_t)R);
                    const int64_t p = record_position(*c, rr);
                    int32_t rec[8];
                    unpack(i, rr, rec);
                    const auto it = own_rd.find((uint64_t)i * (uint64_t)R + (uint64_t)rr);
                    const int RD = it != own_rd.end() ? it->second : rec[0] + rec[1] + rec[2] + rec[3] + rec[4] + rec[5] + rec[6] + rec[7];
                    const PairLimit h = limit_pair_literal(rec, RD, nt, thr[(size_t)nt * P + p], thr[(size_t)(4 + nt) * P + p], cov);
                    status[cell] = (uint8_t)(h.status | (h.called ? AMPLI_LIMIT_CALLED : 0));
                    min_reads[cell * 2] = h.min_fw;
                    min_reads[cell * 2 + 1] = h.min_bw;
                    ++open_cells;
                }
                if (open_cells) {
                    dev.check(dev.api->copy_h2d(dev.ctx, d_min, min_reads.data(), cells * 8), "copy_h2d");
                    dev.check(dev.api->copy_h2d(dev.ctx, d_status, status.data(), cells), "copy_h2d");
                }
                n_recheck += open_cells;
                dev.check(dev.api->power_records(dev.ctx, &r, P, d_min, d_status, d_levels, L, conf, d_power, d_lod, d_counts), "ampli_power_records");
                power.resize(cells * (size_t)L);
                lod.resize(cells);
                counts.resize((size_t)c->n * NC);
                dev.download(power.data(), d_power, power.size());
                dev.download(lod.data(), d_lod, lod.size());
                dev.download(counts.data(), d_counts, counts.size());
                dev.sync();
                for (int i = 0; i < c->n; ++i) {
                    const int t = c->first + i;
                    DpCounts &tc = tot[(size_t)t];
                    std::vector<std::pair<int, int64_t>> order; // (line in the file, record)
                    for (int64_t rr = 0; rr < R; ++rr) {
                        const int line = record_line(*c, i, rr);
                        if (line >= 0) order.emplace_back(line, rr);
                    }
                    std::sort(order.begin(), order.end());
                    tc.lines = (int64_t)order.size();
                    tc.ok = counts[(size_t)i * NC];
                    tc.lev.assign(counts.begin() + (size_t)i * NC + 1, counts.begin() + (size_t)(i + 1) * NC);
                    std::vector<float> lods;
                    std::ostringstream out;
                    out.precision(8); // a float's digits
                    out << "Chrom\tPosition\tRef\tAlt\tRD_fw\tRD_bw\tMinReads_fw\tMinReads_bw\tStatus\tLoD";
                    for (const std::string &s : level_text) out << "\tPower@" << s;
                    out << "\n";
                    for (const auto &lr : order) {
                        const int64_t rr = lr.second;
                        const int64_t p = record_position(*c, rr);
                        const int ref = panel.ref_code[(size_t)p];
                        if (ref > 3) continue; // VC:3290: the line gives no pairs
                        int32_t rec[8];
                        unpack(i, rr, rec);
                        const int FW = rec[0] + rec[1] + rec[2] + rec[3], BW = rec[4] + rec[5] + rec[6] + rec[7];
                        const std::string &chrom = panel.chroms[panel.pos_chrom[p]];
                        for (int nt = 0; nt < 4; ++nt) {
                            if (nt == ref) continue;
                            const size_t cell = ((size_t)i * (size_t)R + (size_t)rr) * 4 + nt;
                            const int st = status[cell] & 7;
                            ++tc.pairs;
                            out << chrom << "\t" << panel.pos_coord[p] << "\t" << "ACGT"[ref] << "\t" << "ACGT"[nt] << "\t" << FW << "\t" << BW << "\t";
                            if (st == AMPLI_LIMIT_OK) {
                                out << min_reads[cell * 2] << "\t" << min_reads[cell * 2 + 1] << "\tOK\t" << lod[cell];
                                for (int l = 0; l < L; ++l) out << "\t" << power[cell * (size_t)L + l];
                                lods.push_back(lod[cell]);
                            } else {
                                out << ".\t.\t" << dp_name(st) << "\t.";
                                for (int l = 0; l < L; ++l) out << "\t.";
                            }
                            out << "\n";
                        }
                    }
                    if ((int64_t)lods.size() != tc.ok) throw Error{AMPLI_E_INVALID, "detection power: the device's counter of OK pairs and its cells differ"};
                    if (!lods.empty()) { // the lower median
                        std::nth_element(lods.begin(), lods.begin() + (lods.size() - 1) / 2, lods.end());
                        tc.median_lod = lods[(lods.size() - 1) / 2];
                    }
                    std::ofstream f(a.output_dir + "/" + files[(size_t)t].second + "_detection_power.txt");
                    f << out.str();
                    f.close();
                    if (f.fail()) throw Error{AMPLI_E_INVALID, "could not write the detection power of " + files[(size_t)t].second};
                }
                cs->release(c);
            }
        }
        std::ofstream sum(a.output_dir + "/Summary_Detection_Power.txt");
        sum << "Filename\tLines\tPairs\tOK\tMedianLoD";
        for (const std::string &s : level_text) sum << "\tPower@" << s << ">=" << conf;
        sum << "\n";
        for (int t = 0; t < T; ++t) {
            const DpCounts &c = tot[(size_t)t];
            sum << files[(size_t)t].second << "\t" << c.lines << "\t" << c.pairs << "\t" << c.ok << "\t";
            if (c.ok) sum << c.median_lod; else sum << ".";
            for (int l = 0; l < L; ++l) sum << "\t" << c.lev[(size_t)l];
            sum << "\n";
        }
        sum.close();
        if (sum.fail()) throw Error{AMPLI_E_INVALID, "could not write Summary_Detection_Power.txt"};
        std::cout << "AmpliSolveDetectionPower: " << T << " files, " << n_recheck << " cells settled on the host" << std::endl;
        return 0;
    });
}

} // namespace ampli
