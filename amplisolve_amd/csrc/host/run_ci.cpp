// amplisolve_amd/csrc/host/run_ci.cpp -- computeIndelCounts: one BAM file -> count files of indel junctions that every
// command reads as it reads substitution counts.  The walk over the file is computeCounts' (walk_bam, bam_walk.hpp); what is launched per
// batch is ampli_pileup_indel_count.  Written:
//   <out>/<bam name>.INDEL.PILEUP.ASEQ   the 15 ASEQ columns, ref A, alt ., A = reference junctions, C = insertions, G = deletions, T = 0
//   <out>/<bam name>.INDEL.LENGTHS.txt   chr pos kind len count per non-zero length bin (no header line)
//   the table at refbases= (optional)    chrom pos A per listed position: what the commands take as AMPLISOLVE_REFBASES_FILE
// Every file is written under a temporary name and renamed into place once all of them are complete: a failure leaves none behind.
#include <unistd.h>

#include <cstdio>
#include <iostream>

#include "bam_walk.hpp"

namespace ampli {

int run_compute_indel_counts(const CiArgs &a)
{
    try {
        if (a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) throw Error{AMPLI_E_INVALID, "vcf=, bam= and out= are required"};
        for (const std::string *path : {&a.vcf, &a.bam}) // refused before the device is opened (walk_bam opens both again, with the same words)
            if (access(path->c_str(), R_OK) != 0) throw Error{AMPLI_E_INVALID, "cannot open " + *path};
        BamDevice dev;
        int32_t *d_counts = nullptr, *d_lengths = nullptr;
        uint64_t *d_stats = nullptr;
        const size_t bins = 2 * AMPLI_INDEL_LEN_BINS;
        BamSink sink;
        sink.panel = [&](BamDevice &d, int64_t P) {
            d_counts = (int32_t *)d.alloc((size_t)P * 8 * sizeof(int32_t));
            d_lengths = (int32_t *)d.alloc((size_t)P * bins * sizeof(int32_t));
            d_stats = (uint64_t *)d.alloc(16);
            d.check(d.api->memset_d(d.ctx, d_counts, 0, (size_t)P * 8 * sizeof(int32_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_lengths, 0, (size_t)P * bins * sizeof(int32_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_stats, 0, 16), "ampli_memset_d");
        };
        sink.batch = [&](BamDevice &d, const uint8_t *d_bam, const uint64_t *d_off, int64_t n_reads, const uint64_t *d_keys, int64_t P) {
            d.check(d.api->pileup_indel_count(d.ctx, d_bam, d_off, n_reads, d_keys, P, a.mbq, a.mrq, d_counts, d_lengths, d_stats), "ampli_pileup_indel_count");
        };
        const BamWalk w = walk_bam(a.vcf, a.bam, a.threads, dev, sink);
        const HipApi *api = dev.api;
        const int64_t P = w.P;

        std::vector<int32_t> counts((size_t)P * 8, 0), lengths((size_t)P * bins, 0);
        uint64_t st[2] = {0, 0};
        if (P > 0) {
            dev.check(api->copy_d2h(dev.ctx, counts.data(), d_counts, counts.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, lengths.data(), d_lengths, lengths.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, st, d_stats, 16), "ampli_copy_d2h");
        }
        dev.check(api->sync(dev.ctx), "ampli_sync");

        std::string base = a.bam;
        const size_t sl = base.rfind('/');
        if (sl != std::string::npos) base = base.substr(sl + 1);
        if (base.size() > 4 && base.compare(base.size() - 4, 4, ".bam") == 0) base.resize(base.size() - 4);
        const std::string out_path = a.out_dir + "/" + base + ".INDEL.PILEUP.ASEQ", len_path = a.out_dir + "/" + base + ".INDEL.LENGTHS.txt";
        TempFiles tmp;
        // one line per listed position whose depth A + C + G reaches mdc, in the list's order
        FILE *o = tmp.open(out_path);
        fputs("chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n", o);
        int64_t written = 0;
        for (const auto &v : w.lines) {
            static const int32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int32_t *c = v.key_index >= 0 ? &counts[(size_t)v.key_index * 8] : zero;
            const long long rd = (long long)c[0] + c[1] + c[2];
            if (rd < a.mdc) continue;
            fprintf(o, "%s\t%lld\t%s\t.\tA\t.\t%d\t%d\t%d\t%d\t%lld\t%d\t%d\t%d\t%d\n", v.chrom.c_str(), (long long)v.pos, v.id.c_str(), c[0], c[1], c[2], c[3], rd,
                    c[4], c[5], c[6], c[7]);
            ++written;
        }
        tmp.close(o, out_path);
        // one line per non-zero length bin, in the list's order, each position once
        o = tmp.open(len_path);
        std::vector<char> seen((size_t)P, 0);
        for (const auto &v : w.lines) {
            if (v.key_index < 0 || seen[(size_t)v.key_index]) continue;
            seen[(size_t)v.key_index] = 1;
            for (int kind = 0; kind < 2; ++kind)
                for (int b = 0; b < AMPLI_INDEL_LEN_BINS; ++b) {
                    const int32_t n = lengths[((size_t)v.key_index * 2 + kind) * AMPLI_INDEL_LEN_BINS + b];
                    if (n) fprintf(o, "%s\t%lld\t%s\t%d\t%d\n", v.chrom.c_str(), (long long)v.pos, kind ? "DEL" : "INS", b + 1, n);
                }
        }
        tmp.close(o, len_path);
        if (!a.refbases.empty()) { // chrom pos A per listed position (several runs of one batch write the same content)
            o = tmp.open(a.refbases);
            for (const auto &v : w.lines) fprintf(o, "%s\t%lld\tA\n", v.chrom.c_str(), (long long)v.pos);
            tmp.close(o, a.refbases);
        }
        tmp.commit();
        std::cout << "computeIndelCounts (MI355X-native build): " << a.bam << "\n\t" << w.n_records << " alignment records (" << w.malformed << " malformed), "
                  << st[0] << " kept (mrq " << a.mrq << "), " << st[1] << " junctions counted (mbq " << a.mbq << ") over " << w.lines.size()
                  << " listed positions\n\t" << written << " lines with depth >= " << a.mdc << " written to " << out_path << "\n\tlengths written to " << len_path
                  << std::endl;
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING total " << w.seconds() << " inflate " << w.t_inflate << " (" << w.threads << " threads, " << w.total_bytes << " bytes) device_wait "
                      << w.t_wait << std::endl;
        if (a.stats) { a.stats[0] = w.n_records; a.stats[1] = (int64_t)st[0]; a.stats[2] = (int64_t)st[1]; a.stats[3] = written; }
        return 0;
    } catch (const Error &e) {
        std::cout << "computeIndelCounts: " << e.msg << std::endl;
        if (a.error) *a.error = e.msg;
        return e.code ? e.code : -1;
    }
}

} // namespace ampli
