// amplisolve_amd/csrc/host/run_dl.cpp -- run_detection_limits, one of the project's own command lines
// AmpliSolveDetectionLimit: for every line of every tumour file and every base other than the reference base, the smallest
// alternative counts with which the calling gate would pass on that line's own depths.  The error table and the tumour files are read
// and streamed exactly as run_variant_calling does; one ampli_limit_records per chunk; the cells the device leaves open (RECHECK) are
// settled by the literal scan; one file per tumour file and a summary.
#include "command.hpp"

namespace ampli {

namespace {
struct DlCounts { int64_t lines = 0, noref = 0, st[4] = {0, 0, 0, 0}; std::vector<int64_t> lev; }; // st: OK, LOWDEPTH, NOESTIMATE, UNREACHABLE
int dl_slot(int status) { return status == AMPLI_LIMIT_OK ? 0 : status == AMPLI_LIMIT_LOWDEPTH ? 1 : status == AMPLI_LIMIT_NOESTIMATE ? 2 : 3; }
const char *dl_name(int status)
{
    return status == AMPLI_LIMIT_OK ? "OK" : status == AMPLI_LIMIT_LOWDEPTH ? "LOWDEPTH" : status == AMPLI_LIMIT_NOESTIMATE ? "NOESTIMATE" : "UNREACHABLE";
}
} // namespace

int run_detection_limits(const DlArgs &a)
{
    return run_command("AmpliSolveDetectionLimit", [&]() -> int {
        int cov = std::atoi(a.coverage_cutoff.c_str());
        if (cov <= 0) cov = 100; // VC:262-275
        std::vector<float> levels;
        {
            std::stringstream ss(a.levels);
            for (std::string t; std::getline(ss, t, ',');) {
                char *end = nullptr;
                const float v = std::strtof(t.c_str(), &end);
                if (t.empty() || end == t.c_str() || *end || !(v > 0 && v <= 1)) throw Error{AMPLI_E_INVALID, "levels: '" + t + "' is not an allele fraction in (0, 1]"};
                levels.push_back(v);
            }
            if (levels.empty() || levels.size() > AMPLI_LIMIT_MAX_LEVELS) throw Error{AMPLI_E_INVALID, "levels: one to 8 allele fractions are required"};
        }
        const int L = (int)levels.size(), NC = AMPLI_LIMIT_COUNTERS + L;
        require_single_gpu("AmpliSolveDetectionLimit");
        const char *ve = getenv("AMPLISOLVE_LIMIT_VERIFY");
        const bool verify_all = ve && std::string(ve) == "all";
        std::cout << "AmpliSolveDetectionLimit: table " << a.error_file << ", tumours " << a.tumour_dir << ", coverage_cutoff " << cov << ", output "
                  << a.output_dir << std::endl;
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
        std::vector<DlCounts> tot((size_t)T);
        int64_t n_recheck = 0, n_verified = 0, n_diff = 0;
        {
            const std::unique_ptr<ChunkStream> cs = open_stream(panel, files, true);
            Dev &dev = dev_async.get();
            float *d_thr = dev.upload(thr.data(), thr.size());
            uint8_t *d_ref = dev.upload(panel.ref_code.data(), panel.ref_code.size());
            float *d_levels = dev.upload(levels.data(), levels.size());
            DevSlot dslots[kDevSlots];
            DevBuf d_min_b, d_status_b, d_counts_b;
            std::vector<int32_t> min_reads;
            std::vector<uint8_t> status;
            std::vector<int64_t> counts;
            for (Chunk *c; (c = cs->next()) != nullptr;) {
                const ampli_records r = upload_chunk(dev, dslots[c->slot % kDevSlots], *c, true);
                const int64_t R = P + c->E;
                const size_t cells = (size_t)c->n * (size_t)R * 4;
                int32_t *d_min = (int32_t *)d_min_b.ensure(dev, cells * 8);
                uint8_t *d_status = (uint8_t *)d_status_b.ensure(dev, cells);
                int64_t *d_counts = (int64_t *)d_counts_b.ensure(dev, (size_t)c->n * NC * 8);
                dev.check(dev.api->memset_d(dev.ctx, d_counts, 0, (size_t)c->n * NC * 8), "memset");
                dev.check(dev.api->limit_records(dev.ctx, &r, P, d_thr, d_ref, cov, d_levels, L, d_min, d_status, d_counts), "ampli_limit_records");
                min_reads.resize(cells * 2);
                status.resize(cells);
                counts.resize((size_t)c->n * NC);
                dev.download(min_reads.data(), d_min, cells * 2);
                dev.download(status.data(), d_status, cells);
                dev.download(counts.data(), d_counts, counts.size());
                dev.sync();
                // the RD column of the lines that carry their own (VC:762-765)
                std::unordered_map<uint64_t, int32_t> own_rd;
                for (const Irregular &x : c->irregular) own_rd[(uint64_t)x.sample * (uint64_t)R + (uint64_t)x.record] = x.rd;
                const size_t rb = record_bytes(c->layout);
                for (int i = 0; i < c->n; ++i) {
                    const int t = c->first + i;
                    DlCounts &tc = tot[(size_t)t];
                    tc.lev.assign((size_t)L, 0);
                    DlCounts host; // VERIFY=all: every counter from the host's own cells
                    host.lev.assign((size_t)L, 0);
                    std::vector<std::pair<int, int64_t>> order; // (line in the file, record)
                    for (int64_t rr = 0; rr < R; ++rr) {
                        const int line = record_line(*c, i, rr);
                        if (line >= 0) order.emplace_back(line, rr);
                    }
                    std::sort(order.begin(), order.end());
                    const int64_t *dc = counts.data() + (size_t)i * NC;
                    tc.lines = (int64_t)order.size();
                    tc.noref = dc[0];
                    for (int k = 0; k < 4; ++k) tc.st[k] = dc[1 + k];
                    for (int l = 0; l < L; ++l) tc.lev[(size_t)l] = dc[AMPLI_LIMIT_COUNTERS + l];
                    int64_t seen_recheck = 0;
                    std::ostringstream out;
                    out << "Chrom\tPosition\tRef\tAlt\tRD\tRD_fw\tRD_bw\tThr_fw\tThr_bw\tMinReads_fw\tMinReads_bw\tMinAF\tStatus\tReads_fw\tReads_bw\tCalled\n";
                    for (const auto &lr : order) {
                        const int64_t rr = lr.second;
                        const int64_t p = record_position(*c, rr);
                        const int ref = panel.ref_code[(size_t)p];
                        if (ref > 3) { ++host.noref; continue; } // VC:3290: the line gives no pairs
                        int32_t rec[8];
                        record_unpack(c->layout, rr < P ? (const char *)c->prim + ((size_t)i * P + rr) * rb
                                                        : (const char *)c->ext + ((size_t)i * c->E + (rr - P)) * rb, rec);
                        const int FW = rec[0] + rec[1] + rec[2] + rec[3], BW = rec[4] + rec[5] + rec[6] + rec[7];
                        const auto it = own_rd.find((uint64_t)i * (uint64_t)R + (uint64_t)rr);
                        const int RD = it != own_rd.end() ? it->second : FW + BW;
                        const std::string &chrom = panel.chroms[panel.pos_chrom[p]];
                        for (int nt = 0; nt < 4; ++nt) {
                            if (nt == ref) continue;
                            const size_t cell = ((size_t)i * (size_t)R + (size_t)rr) * 4 + nt;
                            const float th_fw = thr[(size_t)nt * P + p], th_bw = thr[(size_t)(4 + nt) * P + p];
                            PairLimit pl{status[cell] & 7, min_reads[cell * 2], min_reads[cell * 2 + 1], (status[cell] & AMPLI_LIMIT_CALLED) != 0};
                            const bool recheck = (status[cell] & AMPLI_LIMIT_RECHECK) != 0;
                            if (recheck || verify_all) {
                                const PairLimit h = limit_pair_literal(rec, RD, nt, th_fw, th_bw, cov);
                                if (recheck) {
                                    ++seen_recheck;
                                    pl = h;
                                    ++tc.st[dl_slot(pl.status)];
                                } else {
                                    ++n_verified;
                                    if (h.status != pl.status || h.min_fw != pl.min_fw || h.min_bw != pl.min_bw || h.called != pl.called) {
                                        if (++n_diff <= 10)
                                            std::cout << "VERIFY: " << files[(size_t)t].second << " " << chrom << ":" << panel.pos_coord[p] << " " << "ACGT"[nt]
                                                      << " device " << dl_name(pl.status) << " " << pl.min_fw << "/" << pl.min_bw << " called " << pl.called
                                                      << ", host " << dl_name(h.status) << " " << h.min_fw << "/" << h.min_bw << " called " << h.called << std::endl;
                                    }
                                }
                            }
                            const float min_af = pl.status == AMPLI_LIMIT_OK ? (float)(pl.min_fw + pl.min_bw) / (float)RD : 0.0f; // as VC:814-817
                            if (pl.status == AMPLI_LIMIT_OK)
                                for (int l = 0; l < L; ++l) {
                                    if (recheck && min_af <= levels[(size_t)l]) ++tc.lev[(size_t)l];
                                    if (min_af <= levels[(size_t)l]) ++host.lev[(size_t)l];
                                }
                            ++host.st[dl_slot(pl.status)];
                            out << chrom << "\t" << panel.pos_coord[p] << "\t" << "ACGT"[ref] << "\t" << "ACGT"[nt] << "\t" << RD << "\t" << FW << "\t" << BW
                                << "\t" << th_fw << "\t" << th_bw << "\t";
                            if (pl.status == AMPLI_LIMIT_OK) out << pl.min_fw << "\t" << pl.min_bw << "\t" << min_af;
                            else out << ".\t.\t.";
                            out << "\t" << dl_name(pl.status) << "\t" << rec[nt] << "\t" << rec[4 + nt] << "\t" << (pl.called ? "YES" : "NO") << "\n";
                        }
                    }
                    if (seen_recheck != dc[5]) throw Error{AMPLI_E_INVALID, "detection limits: the device's RECHECK counter and its cells differ"};
                    n_recheck += seen_recheck;
                    if (verify_all) {
                        bool same = host.noref == tc.noref;
                        for (int k = 0; k < 4; ++k) same = same && host.st[k] == tc.st[k];
                        for (int l = 0; l < L; ++l) same = same && host.lev[(size_t)l] == tc.lev[(size_t)l];
                        if (!same) {
                            ++n_diff;
                            std::cout << "VERIFY: the counters of " << files[(size_t)t].second << " differ from the host's" << std::endl;
                        }
                    }
                    std::ofstream f(a.output_dir + "/" + files[(size_t)t].second + "_detection_limits.txt");
                    f << out.str();
                    f.close();
                    if (f.fail()) throw Error{AMPLI_E_INVALID, "could not write the detection limits of " + files[(size_t)t].second};
                }
                cs->release(c);
            }
        }
        std::ofstream sum(a.output_dir + "/Summary_Detection_Limits.txt");
        sum << "Filename\tLines\tNoRefLines\tPairs\tOK\tLOWDEPTH\tNOESTIMATE\tUNREACHABLE";
        for (float v : levels) sum << "\tMinAF<=" << v;
        sum << "\n";
        for (int t = 0; t < T; ++t) {
            const DlCounts &c = tot[(size_t)t];
            sum << files[(size_t)t].second << "\t" << c.lines << "\t" << c.noref << "\t" << c.st[0] + c.st[1] + c.st[2] + c.st[3];
            for (int k = 0; k < 4; ++k) sum << "\t" << c.st[k];
            for (int l = 0; l < L; ++l) sum << "\t" << c.lev[(size_t)l];
            sum << "\n";
        }
        sum.close();
        if (sum.fail()) throw Error{AMPLI_E_INVALID, "could not write Summary_Detection_Limits.txt"};
        std::cout << "AmpliSolveDetectionLimit: " << T << " files, " << n_recheck << " cells settled on the host";
        if (verify_all) std::cout << ", " << n_verified << " cells verified, " << n_diff << " differences";
        std::cout << std::endl;
        if (n_diff) throw Error{AMPLI_E_INVALID, "AMPLISOLVE_LIMIT_VERIFY=all: device and host differ"};
        return 0;
    });
}

} // namespace ampli
