// amplisolve_amd/csrc/host/run_re.cpp -- computeReadEvidence: one BAM file and a list of calls -> what the reads behind every
// call looked like.  The walk over the file is computeCounts' (walk_bam, bam_walk.hpp); what is launched per batch is
// ampli_pileup_evidence, and behind the walk one ampli_evidence_score over the listed lines.  Written:
//   <out>/<bam name>.EVIDENCE.txt        chr pos ref alt n_ref n_alt, then per metric (BQ, MQ, POS) med_ref med_alt z, then the verdict; one
//                                        line per listed line, in the list's order (no header line)
//   <out>/<bam name>.EVIDENCE.HIST.txt   chr pos nt metric bin count per non-zero bin of the ref and alt alleles of every listed line
// Both files are written under a temporary name and renamed into place once both are complete: a failure leaves none behind.
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <iostream>

#include "../ampli_math.h"
#include "bam_walk.hpp"
#include "command.hpp"

namespace ampli {

namespace {
constexpr size_t EV_CELLS = 4 * AMPLI_EVIDENCE_METRICS * AMPLI_EVIDENCE_BINS; // counters of one position
const char *const EV_METRIC[AMPLI_EVIDENCE_METRICS] = {"BQ", "MQ", "POS"};
const char *const EV_FLAG[AMPLI_EVIDENCE_METRICS] = {"LOW_BQ", "LOW_MQ", "READ_END"};
} // namespace

int evidence_nt(const std::string &allele, bool choose)
{
    if (allele.size() != 1) return -2;
    switch (allele[0]) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    case '.': return choose ? -1 : -2;
    default: return -2;
    }
}

void evidence_score_host(const int32_t *hist, int64_t P, const int8_t *ref_nt, const int8_t *alt_nt, int64_t *o_int, int32_t *o_med, double *o_z2, int8_t *alt_used)
{
    for (int64_t p = 0; p < P; ++p) {
        const int32_t *h = hist + (size_t)p * EV_CELLS;
        const int ref = ref_nt[p];
        const int alt = ampli_ev_alt(h, ref, alt_nt[p]);
        for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) {
            const int32_t *a = alt >= 0 ? h + (alt * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS : nullptr;
            const int32_t *r = ref >= 0 && ref <= 3 ? h + (ref * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS : nullptr;
            const size_t cell = (size_t)p * AMPLI_EVIDENCE_METRICS + m;
            ampli_ev_cell(a, r, o_int + cell * 3, o_med + cell * 2, o_z2 + cell);
        }
        alt_used[p] = (int8_t)alt;
    }
}

int64_t write_evidence_files(const std::string &out_dir, const std::string &name, const std::vector<EvidenceListed> &listed, const int32_t *hist,
                             const int64_t *v_int, const int32_t *v_med, const double *v_z2, const int8_t *ref_nt, const int8_t *alt_used, int64_t min_alt,
                             double z_min)
{
    const std::string ev_path = out_dir + "/" + name + ".EVIDENCE.txt", hist_path = out_dir + "/" + name + ".EVIDENCE.HIST.txt";
    TempFiles tmp;
    FILE *o = tmp.open(ev_path);
    int64_t written = 0;
    for (size_t l = 0; l < listed.size(); ++l) {
        const auto &v = listed[l];
        const int64_t *vi = v_int + l * AMPLI_EVIDENCE_METRICS * 3;
        const bool usable = alt_used[l] >= 0;
        const char alt_text[2] = {usable ? "ACGT"[alt_used[l]] : '.', 0};
        fprintf(o, "%s\t%lld\t%s\t%s\t%lld\t%lld", v.chrom.c_str(), (long long)v.pos, v.ref.c_str(), usable ? alt_text : v.alt.c_str(), (long long)vi[0], (long long)vi[1]);
        std::string flags;
        for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) {
            const size_t cell = l * AMPLI_EVIDENCE_METRICS + m;
            fprintf(o, "\t%d\t%d", v_med[cell * 2], v_med[cell * 2 + 1]);
            if (v_int[cell * 3 + 2] < 0) { // an untested cell: no score, no flag
                fputs("\t.", o);
                continue;
            }
            const double z2 = v_z2[cell];
            fprintf(o, "\t%.4f", z2 < 0.0 ? -std::sqrt(-z2) : std::sqrt(z2));
            if (z2 <= -(z_min * z_min)) flags += (flags.empty() ? "" : ",") + std::string(EV_FLAG[m]);
        }
        const bool tested = usable && vi[1] >= min_alt && vi[0] >= min_alt;
        fprintf(o, "\t%s\n", !tested ? "UNTESTED" : flags.empty() ? "PASS" : flags.c_str());
        ++written;
    }
    tmp.close(o, ev_path);
    // the bins behind every line: its ref allele, then its alt allele
    o = tmp.open(hist_path);
    for (size_t l = 0; l < listed.size(); ++l) {
        const auto &v = listed[l];
        const int side[2] = {ref_nt[l] >= 0 && ref_nt[l] <= 3 ? ref_nt[l] : -1, alt_used[l]};
        for (const int nt : side) {
            if (nt < 0) continue;
            for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m)
                for (int b = 0; b < AMPLI_EVIDENCE_BINS; ++b) {
                    const int32_t n = hist[l * EV_CELLS + ((size_t)nt * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS + b];
                    if (n) fprintf(o, "%s\t%lld\t%c\t%s\t%d\t%d\n", v.chrom.c_str(), (long long)v.pos, "ACGT"[nt], EV_METRIC[m], b, n);
                }
        }
    }
    tmp.close(o, hist_path);
    tmp.commit();
    return written;
}

int run_compute_read_evidence(const ReArgs &a)
{
    try {
        if (a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) throw Error{AMPLI_E_INVALID, "vcf=, bam= and out= are required"};
        // refused before the device is opened: bad numbers, unreadable inputs (walk_bam opens vcf and bam again, with the same words)
        const int threads = parse_int(a.threads, "threads", 1, 1024), mbq = parse_int(a.mbq, "mbq", 0, 255), mrq = parse_int(a.mrq, "mrq", 0, 255);
        const int min_alt = parse_int(a.min_alt, "min_alt", 1);
        const double z_min = parse_number(a.z_min, "z_min", "> 0", [](double v) { return v > 0.0; });
        for (const std::string *path : {&a.vcf, &a.bam})
            if (access(path->c_str(), R_OK) != 0) throw Error{AMPLI_E_INVALID, "cannot open " + *path};

        BamDevice dev;
        int32_t *d_hist = nullptr;
        uint64_t *d_stats = nullptr;
        BamSink sink;
        sink.panel = [&](BamDevice &d, int64_t P) {
            d_hist = (int32_t *)d.alloc((size_t)P * EV_CELLS * sizeof(int32_t));
            d_stats = (uint64_t *)d.alloc(16);
            d.check(d.api->memset_d(d.ctx, d_hist, 0, (size_t)P * EV_CELLS * sizeof(int32_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_stats, 0, 16), "ampli_memset_d");
        };
        sink.batch = [&](BamDevice &d, const uint8_t *d_bam, const uint64_t *d_off, int64_t n_reads, const uint64_t *d_keys, int64_t P) {
            d.check(d.api->pileup_evidence(d.ctx, d_bam, d_off, n_reads, d_keys, P, mbq, mrq, d_hist, d_stats), "ampli_pileup_evidence");
        };
        const BamWalk w = walk_bam(a.vcf, a.bam, threads, dev, sink);
        const HipApi *api = dev.api;
        const size_t P = (size_t)w.P, L = w.lines.size();

        std::vector<int32_t> hist(P * EV_CELLS, 0);
        uint64_t st[2] = {0, 0};
        if (P > 0) {
            dev.check(api->copy_d2h(dev.ctx, hist.data(), d_hist, hist.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, st, d_stats, 16), "ampli_copy_d2h");
        }
        dev.check(api->sync(dev.ctx), "ampli_sync");
        // the planes in the list's order -- a position listed twice twice, an unknown chromosome as zeros -- with the alleles of every line
        std::vector<EvidenceListed> listed(L);
        std::vector<int32_t> lhist(L * EV_CELLS, 0);
        std::vector<int8_t> ref_nt(L), alt_nt(L), alt_used(L, (int8_t)-1);
        for (size_t l = 0; l < L; ++l) {
            const auto &v = w.lines[l];
            listed[l].chrom = v.chrom; listed[l].ref = v.ref; listed[l].alt = v.alt; listed[l].pos = v.pos;
            ref_nt[l] = (int8_t)evidence_nt(v.ref, false);
            alt_nt[l] = (int8_t)evidence_nt(v.alt, true);
            if (v.key_index >= 0) std::copy_n(&hist[(size_t)v.key_index * EV_CELLS], EV_CELLS, &lhist[l * EV_CELLS]);
        }
        std::vector<int64_t> v_int(L * AMPLI_EVIDENCE_METRICS * 3, 0);
        std::vector<int32_t> v_med(L * AMPLI_EVIDENCE_METRICS * 2, 0);
        std::vector<double> v_z2(L * AMPLI_EVIDENCE_METRICS, 0.0);
        {
            int32_t *d_lhist = (int32_t *)dev.alloc(lhist.size() * sizeof(int32_t));
            int8_t *d_ref = (int8_t *)dev.alloc(L), *d_alt = (int8_t *)dev.alloc(L), *d_used = (int8_t *)dev.alloc(L);
            int64_t *d_int = (int64_t *)dev.alloc(v_int.size() * sizeof(int64_t));
            int32_t *d_med = (int32_t *)dev.alloc(v_med.size() * sizeof(int32_t));
            double *d_z2 = (double *)dev.alloc(v_z2.size() * sizeof(double));
            dev.check(api->copy_h2d(dev.ctx, d_lhist, lhist.data(), lhist.size() * sizeof(int32_t)), "ampli_copy_h2d");
            dev.check(api->copy_h2d(dev.ctx, d_ref, ref_nt.data(), L), "ampli_copy_h2d");
            dev.check(api->copy_h2d(dev.ctx, d_alt, alt_nt.data(), L), "ampli_copy_h2d");
            dev.check(api->evidence_score(dev.ctx, d_lhist, (int64_t)L, d_ref, d_alt, d_int, d_med, d_z2, d_used), "ampli_evidence_score");
            dev.check(api->copy_d2h(dev.ctx, v_int.data(), d_int, v_int.size() * sizeof(int64_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, v_med.data(), d_med, v_med.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, v_z2.data(), d_z2, v_z2.size() * sizeof(double)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, alt_used.data(), d_used, L), "ampli_copy_d2h");
            dev.check(api->sync(dev.ctx), "ampli_sync");
        }

        std::string base = a.bam;
        const size_t sl = base.rfind('/');
        if (sl != std::string::npos) base = base.substr(sl + 1);
        if (base.size() > 4 && base.compare(base.size() - 4, 4, ".bam") == 0) base.resize(base.size() - 4);
        const int64_t written = write_evidence_files(a.out_dir, base, listed, lhist.data(), v_int.data(), v_med.data(), v_z2.data(), ref_nt.data(), alt_used.data(),
                                                     min_alt, z_min);
        std::cout << "computeReadEvidence (MI355X-native build): " << a.bam << "\n\t" << w.n_records << " alignment records (" << w.malformed << " malformed), "
                  << st[0] << " kept (mrq " << mrq << "), " << st[1] << " columns counted (mbq " << mbq << ") over " << L << " listed lines\n\t" << written
                  << " lines (min_alt " << min_alt << ", z_min " << a.z_min << ") written to " << a.out_dir << "/" << base << ".EVIDENCE.txt" << std::endl;
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING total " << w.seconds() << " inflate " << w.t_inflate << " (" << w.threads << " threads, " << w.total_bytes << " bytes) device_wait "
                      << w.t_wait << std::endl;
        if (a.stats) { a.stats[0] = w.n_records; a.stats[1] = (int64_t)st[0]; a.stats[2] = (int64_t)st[1]; a.stats[3] = written; }
        return 0;
    } catch (const Error &e) {
        std::cout << "computeReadEvidence: " << e.msg << std::endl;
        if (a.error) *a.error = e.msg;
        return e.code ? e.code : -1;
    }
}

} // namespace ampli
