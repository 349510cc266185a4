// amplisolve_amd/csrc/host/run_ca.cpp -- computeAmpliconCounts: one BAM file -> count files that keep which amplicon a read
// came from.  The walk over the file is computeCounts' (walk_bam, bam_walk.hpp); what is launched per batch is
// ampli_pileup_amplicon_count, and behind the walk one ampli_amplicon_layers over the listed positions.  Written:
//   <out>/<bam name>.AMPLICON.PILEUP.ASEQ     the 15 ASEQ columns per listed position: the sum over the amplicons that cover it, every read
//                                              counted inside its own amplicon only
//   <out>/<bam name>.AMPLICON.READS.txt       chrom start end name gene reads_fw reads_rev per BED row, then #kept #assigned #off_target
//                                              #bases_counted #bases_clipped
//   <out>/<bam name>.AMPLICON.OVERLAPS.txt    chr pos name A C G T Ars Crs Grs Trs per listed position under >= 2 amplicons and covering amplicon
//   <layers>/<bam name>.AMP1.PILEUP.ASEQ, .AMP2.PILEUP.ASEQ, <bam name>.pairs.txt (with layers=): the first and the second covering
//                                              amplicon as count files, and the pair list AmpliSolvePairedComparison takes
// Every file is written under a temporary name and renamed into place once all of them are complete: a failure leaves none behind.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <numeric>

#include "bam_walk.hpp"
#include "command.hpp"

namespace ampli {

AmpliconArrays amplicon_arrays(const std::vector<BedRow> &rows, const std::vector<std::string> &ref_names)
{
    std::unordered_map<std::string, int> rid;
    for (size_t i = 0; i < ref_names.size(); ++i) rid.emplace(ref_names[i], (int)i); // the first of a repeated name, as walk_bam takes it
    AmpliconArrays out;
    out.sorted_of_row.assign(rows.size(), -1);
    std::vector<uint64_t> lo, hi;
    std::vector<int32_t> row;
    for (size_t r = 0; r < rows.size(); ++r) {
        const auto it = rid.find(rows[r].chrom);
        if (it == rid.end() || rows[r].start < 1 || rows[r].end < rows[r].start) continue; // (int: end < 2^31)
        lo.push_back(((uint64_t)(uint32_t)it->second << 32) | (uint64_t)rows[r].start);
        hi.push_back(((uint64_t)(uint32_t)it->second << 32) | (uint64_t)rows[r].end);
        row.push_back((int32_t)r);
    }
    std::vector<size_t> order(lo.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lo[x] != lo[y] ? lo[x] < lo[y] : hi[x] < hi[y]; });
    out.amp_off.push_back(0);
    for (size_t a = 0; a < order.size(); ++a) {
        const size_t k = order[a];
        out.lo.push_back(lo[k]);
        out.hi.push_back(hi[k]);
        out.reach.push_back(a ? std::max(out.reach[a - 1], hi[k]) : hi[k]);
        out.amp_off.push_back(out.amp_off.back() + (int64_t)(hi[k] - lo[k]) + 1);
        out.row_of.push_back(row[k]);
        out.sorted_of_row[(size_t)row[k]] = (int32_t)a;
        if (out.amp_off.back() > 0x7fffffffll) throw Error{AMPLI_E_RANGE, "the amplicons of the BED file cover 2^31 positions or more"};
    }
    return out;
}

void AmpliconArrays::candidates(uint64_t key, int64_t &first, int64_t &last) const
{
    first = (int64_t)(std::lower_bound(reach.begin(), reach.end(), key) - reach.begin());
    last = (int64_t)(std::upper_bound(lo.begin(), lo.end(), key) - lo.begin()) - 1;
}

namespace {

const char *ASEQ_HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n";

// one count file: the listed positions whose record `rec(v)` exists (not nullptr) and reaches mdc; returns the lines written
template <class F> int64_t write_aseq(TempFiles &tmp, const std::string &path, const std::vector<AmpliconListed> &listed, int mdc, F &&rec)
{
    FILE *o = tmp.open(path);
    fputs(ASEQ_HEADER, o);
    int64_t written = 0;
    for (const auto &v : listed) {
        const int32_t *c = rec(v);
        if (!c) continue;
        const long long rd = (long long)c[0] + c[1] + c[2] + c[3];
        if (rd < mdc) continue;
        fprintf(o, "%s\t%lld\t%s\t.\t%s\t%s\t%d\t%d\t%d\t%d\t%lld\t%d\t%d\t%d\t%d\n", v.chrom.c_str(), (long long)v.pos, v.id.c_str(), v.ref.c_str(), v.alt.c_str(),
                c[0], c[1], c[2], c[3], rd, c[4], c[5], c[6], c[7]);
        ++written;
    }
    tmp.close(o, path);
    return written;
}

} // namespace

int64_t write_amplicon_files(const std::string &out_dir, const std::string &layers_dir, const std::string &name, const std::vector<BedRow> &rows,
                             const AmpliconArrays &amps, const std::vector<AmpliconListed> &listed, const AmpliconCounts &c, int mdc)
{
    static const int32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t n = c.keys.size();
    TempFiles tmp;
    // the clipped totals: a count file like any other
    const int64_t written = write_aseq(tmp, out_dir + "/" + name + ".AMPLICON.PILEUP.ASEQ", listed, mdc,
                                       [&](const AmpliconListed &v) { return v.slot >= 0 ? &c.total[(size_t)v.slot * 8] : zero; });
    // the reads of every BED row, in BED order
    const std::string reads_path = out_dir + "/" + name + ".AMPLICON.READS.txt";
    FILE *o = tmp.open(reads_path);
    for (size_t r = 0; r < rows.size(); ++r) {
        const int32_t a = amps.sorted_of_row[r];
        fprintf(o, "%s\t%d\t%d\t%s\t%s\t%lld\t%lld\n", rows[r].chrom.c_str(), rows[r].start, rows[r].end, rows[r].name.c_str(), rows[r].gene.c_str(),
                a >= 0 ? (long long)c.amp_reads[(size_t)a * 2] : 0ll, a >= 0 ? (long long)c.amp_reads[(size_t)a * 2 + 1] : 0ll);
    }
    fprintf(o, "#kept\t%llu\n#assigned\t%llu\n#off_target\t%llu\n#bases_counted\t%llu\n#bases_clipped\t%llu\n", (unsigned long long)c.stats[0],
            (unsigned long long)c.stats[1], (unsigned long long)(c.stats[0] - c.stats[1]), (unsigned long long)c.stats[2], (unsigned long long)c.stats[3]);
    tmp.close(o, reads_path);
    // every listed position under two or more amplicons, one line per covering amplicon in sorted order
    const std::string over_path = out_dir + "/" + name + ".AMPLICON.OVERLAPS.txt";
    o = tmp.open(over_path);
    std::vector<int64_t> cover;
    for (const auto &v : listed) {
        if (v.slot < 0) continue;
        const uint64_t key = c.keys[(size_t)v.slot];
        int64_t first, last;
        amps.candidates(key, first, last);
        cover.clear();
        for (int64_t a = first; a <= last; ++a)
            if (amps.hi[(size_t)a] >= key) cover.push_back(a);
        if (cover.size() < 2) continue;
        for (const int64_t a : cover) {
            const int32_t *r = &c.counts[(size_t)(amps.amp_off[(size_t)a] + (int64_t)(key - amps.lo[(size_t)a])) * 8];
            fprintf(o, "%s\t%lld\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", v.chrom.c_str(), (long long)v.pos, rows[(size_t)amps.row_of[(size_t)a]].name.c_str(), r[0], r[1],
                    r[2], r[3], r[4], r[5], r[6], r[7]);
        }
    }
    tmp.close(o, over_path);
    if (!layers_dir.empty()) { // layers 0 and 1 as count files, where the layer has an amplicon, and the pair list of the two
        for (int l = 0; l < 2; ++l)
            write_aseq(tmp, layers_dir + "/" + name + ".AMP" + std::to_string(l + 1) + ".PILEUP.ASEQ", listed, mdc, [&](const AmpliconListed &v) {
                return v.slot >= 0 && c.layer_amp[(size_t)l * n + (size_t)v.slot] >= 0 ? &c.layers[((size_t)l * n + (size_t)v.slot) * 8] : nullptr;
            });
        const std::string pairs_path = layers_dir + "/" + name + ".pairs.txt";
        o = tmp.open(pairs_path);
        fprintf(o, "%s.AMP1\t%s.AMP2\n", name.c_str(), name.c_str());
        tmp.close(o, pairs_path);
    }
    tmp.commit();
    return written;
}

int run_compute_amplicon_counts(const CaArgs &a)
{
    try {
        if (a.vcf.empty() || a.bam.empty() || a.bed.empty() || a.out_dir.empty()) throw Error{AMPLI_E_INVALID, "vcf=, bam=, bed= and out= are required"};
        // refused before the device is opened: bad numbers, unreadable inputs (walk_bam opens vcf and bam again, with the same words)
        const int threads = parse_int(a.threads, "threads", 1, 1024), mbq = parse_int(a.mbq, "mbq", 0, 255), mrq = parse_int(a.mrq, "mrq", 0, 255);
        const int mdc = parse_int(a.mdc, "mdc", 0), min_overlap = parse_int(a.min_overlap, "min_overlap", 1, 100);
        if (!a.layers_dir.empty() && a.layers_dir == a.out_dir) throw Error{AMPLI_E_INVALID, "layers= must differ from out=: the commands take every *.ASEQ file of a directory"};
        for (const std::string *path : {&a.vcf, &a.bam, &a.bed})
            if (access(path->c_str(), R_OK) != 0) throw Error{AMPLI_E_INVALID, "cannot open " + *path};
        const std::vector<BedRow> rows = bed_rows(a.bed); // (not the Panel: the command needs no position index)

        BamDevice dev;
        AmpliconArrays amps;
        uint64_t *d_lo = nullptr, *d_hi = nullptr, *d_reach = nullptr, *d_stats = nullptr;
        int64_t *d_amp_off = nullptr, *d_amp_reads = nullptr;
        int32_t *d_counts = nullptr;
        BamSink sink;
        sink.header = [&](const std::vector<std::string> &ref_names) { amps = amplicon_arrays(rows, ref_names); };
        sink.panel = [&](BamDevice &d, int64_t) {
            const size_t A = (size_t)amps.A(), W = (size_t)amps.W();
            if (A == 0) return;
            const auto up = [&](const void *src, size_t bytes) {
                void *p = d.alloc(bytes);
                d.check(d.api->copy_h2d(d.ctx, p, src, bytes), "ampli_copy_h2d");
                return p;
            };
            d_lo = (uint64_t *)up(amps.lo.data(), A * 8);
            d_hi = (uint64_t *)up(amps.hi.data(), A * 8);
            d_reach = (uint64_t *)up(amps.reach.data(), A * 8);
            d_amp_off = (int64_t *)up(amps.amp_off.data(), (A + 1) * 8);
            d_counts = (int32_t *)d.alloc(W * 8 * sizeof(int32_t));
            d_amp_reads = (int64_t *)d.alloc(A * 2 * sizeof(int64_t));
            d_stats = (uint64_t *)d.alloc(32);
            d.check(d.api->memset_d(d.ctx, d_counts, 0, W * 8 * sizeof(int32_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_amp_reads, 0, A * 2 * sizeof(int64_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_stats, 0, 32), "ampli_memset_d");
        };
        sink.batch = [&](BamDevice &d, const uint8_t *d_bam, const uint64_t *d_off, int64_t n_reads, const uint64_t *, int64_t) {
            if (!d_counts) return;
            d.check(d.api->pileup_amplicon_count(d.ctx, d_bam, d_off, n_reads, d_lo, d_hi, d_reach, d_amp_off, amps.A(), amps.W(), mbq, mrq, min_overlap, d_counts,
                                                 d_amp_reads, d_stats),
                    "ampli_pileup_amplicon_count");
        };
        const BamWalk w = walk_bam(a.vcf, a.bam, threads, dev, sink);
        const HipApi *api = dev.api;

        // the listed positions with a known chromosome, in the list's order (repeats stay): the gather's keys
        std::unordered_map<std::string, int> rid;
        for (size_t i = 0; i < w.ref_names.size(); ++i) rid.emplace(w.ref_names[i], (int)i);
        AmpliconCounts c;
        std::vector<AmpliconListed> listed;
        for (const auto &v : w.lines) {
            AmpliconListed l;
            l.chrom = v.chrom; l.id = v.id; l.ref = v.ref; l.alt = v.alt; l.pos = v.pos;
            if (v.key_index >= 0) {
                l.slot = (int64_t)c.keys.size();
                c.keys.push_back(((uint64_t)(uint32_t)rid.at(v.chrom) << 32) | (uint64_t)v.pos);
            }
            listed.push_back(l);
        }
        const size_t n = c.keys.size(), A = (size_t)amps.A(), W = (size_t)amps.W();
        c.counts.assign(W * 8, 0);
        c.amp_reads.assign(A * 2, 0);
        c.layers.assign(2 * n * 8, 0);
        for (size_t i = 0; i < 2 * n; ++i) c.layers[i * 8] = AMPLI_ABSENT;
        c.layer_amp.assign(2 * n, -1);
        c.total.assign(n * 8, 0);
        if (d_counts && n > 0) {
            uint64_t *d_keys = (uint64_t *)dev.alloc(n * 8);
            int32_t *d_layers = (int32_t *)dev.alloc(2 * n * 8 * sizeof(int32_t)), *d_layer_amp = (int32_t *)dev.alloc(2 * n * sizeof(int32_t));
            int32_t *d_total = (int32_t *)dev.alloc(n * 8 * sizeof(int32_t));
            dev.check(api->copy_h2d(dev.ctx, d_keys, c.keys.data(), n * 8), "ampli_copy_h2d");
            dev.check(api->amplicon_layers(dev.ctx, d_counts, d_lo, d_hi, d_reach, d_amp_off, amps.A(), amps.W(), d_keys, (int64_t)n, 2, d_layers, d_layer_amp, d_total),
                      "ampli_amplicon_layers");
            dev.check(api->copy_d2h(dev.ctx, c.counts.data(), d_counts, c.counts.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, c.amp_reads.data(), d_amp_reads, c.amp_reads.size() * sizeof(int64_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, c.stats, d_stats, 32), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, c.layers.data(), d_layers, c.layers.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, c.layer_amp.data(), d_layer_amp, c.layer_amp.size() * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, c.total.data(), d_total, c.total.size() * sizeof(int32_t)), "ampli_copy_d2h");
        }
        dev.check(api->sync(dev.ctx), "ampli_sync");

        std::string base = a.bam;
        const size_t sl = base.rfind('/');
        if (sl != std::string::npos) base = base.substr(sl + 1);
        if (base.size() > 4 && base.compare(base.size() - 4, 4, ".bam") == 0) base.resize(base.size() - 4);
        const int64_t written = write_amplicon_files(a.out_dir, a.layers_dir, base, rows, amps, listed, c, mdc);
        std::cout << "computeAmpliconCounts (MI355X-native build): " << a.bam << "\n\t" << w.n_records << " alignment records (" << w.malformed << " malformed), "
                  << c.stats[0] << " kept (mrq " << mrq << "), " << c.stats[1] << " assigned to " << A << " of " << rows.size() << " BED rows (min_overlap "
                  << min_overlap << "), " << c.stats[2] << " bases counted (mbq " << mbq << "), " << c.stats[3] << " clipped, over " << listed.size()
                  << " listed positions\n\t" << written << " lines with depth >= " << mdc << " written to " << a.out_dir << "/" << base << ".AMPLICON.PILEUP.ASEQ"
                  << std::endl;
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING total " << w.seconds() << " inflate " << w.t_inflate << " (" << w.threads << " threads, " << w.total_bytes << " bytes) device_wait "
                      << w.t_wait << std::endl;
        if (a.stats) {
            a.stats[0] = w.n_records;
            for (int i = 0; i < 4; ++i) a.stats[1 + i] = (int64_t)c.stats[i];
            a.stats[5] = written;
        }
        return 0;
    } catch (const Error &e) {
        std::cout << "computeAmpliconCounts: " << e.msg << std::endl;
        if (a.error) *a.error = e.msg;
        return e.code ? e.code : -1;
    }
}

} // namespace ampli
