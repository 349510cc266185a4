// amplisolve_amd/csrc/host/run_ph.cpp -- computePhasing: one BAM file and a list of calls -> do nearby calls share their reads.
// The walk over the file is computeCounts' (walk_bam, bam_walk.hpp); what is launched per batch is ampli_pileup_phase, and behind the walk
// one ampli_phase_score over every formed pair of listed lines.  Written:
//   <out>/<bam name>.PHASE.txt       chr posA refA altA posB refB altB n_joint n_rr n_ra n_ar n_aa n_other exp_aa score verdict; one line per
//                                    pair of listed lines at most max_dist apart, in the order (key of A, key of B, list order); no header line
//   <out>/<bam name>.PHASE.MNV.txt   chr pos ref_string alt_string reads per chain of 2 or 3 lines at consecutive positions that are CIS in pairs
// Both files are written under a temporary name and renamed into place once both are complete: a failure leaves none behind.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <map>
#include <tuple>

#include "../ampli_math.h"
#include "bam_walk.hpp"
#include "command.hpp"

namespace ampli {

namespace {
constexpr size_t PH_CELLS = (size_t)AMPLI_PHASE_PARTNERS * AMPLI_PHASE_STATES * AMPLI_PHASE_STATES; // counters of one key
} // namespace

void phase_score_host(const int32_t *table, int64_t P, const int64_t *pair_cell, const int8_t *pair_nt, int64_t Q, int32_t min_alt, int32_t min_share, int64_t *o_int,
                      float *o_score, int32_t *o_class)
{
    for (int64_t q = 0; q < Q; ++q) ampli_ph_cell(table, P, pair_cell[q], pair_nt + q * 4, min_alt, min_share, o_int + q * 6, o_score + q, o_class + q);
}

std::vector<PhasePair> phase_pairs(const std::vector<PhaseListed> &listed, int64_t max_dist, std::vector<int64_t> &pair_cell, std::vector<int8_t> &pair_nt)
{
    // the lines with a key, by (key, list order): on one chromosome that is by position
    std::vector<int64_t> order;
    for (size_t l = 0; l < listed.size(); ++l)
        if (listed[l].key_index >= 0) order.push_back((int64_t)l);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return listed[x].key_index < listed[y].key_index; });
    std::vector<PhasePair> pairs;
    pair_cell.clear();
    pair_nt.clear();
    for (size_t i = 0; i < order.size(); ++i) {
        const PhaseListed &la = listed[order[i]];
        for (size_t j = i + 1; j < order.size(); ++j) {
            const PhaseListed &lb = listed[order[j]];
            if (lb.key_index == la.key_index) continue;                    // the same position: no pair
            if (lb.chrom != la.chrom || lb.pos - la.pos > max_dist) break; // sorted by key: nothing nearer follows
            PhasePair p;
            p.a = order[i];
            p.b = order[j];
            pairs.push_back(p);
        }
    }
    const auto rank = [&](const PhasePair &p) { return std::make_tuple(listed[p.a].key_index, listed[p.b].key_index, p.a, p.b); };
    std::sort(pairs.begin(), pairs.end(), [&](const PhasePair &x, const PhasePair &y) { return rank(x) < rank(y); });
    for (PhasePair &p : pairs) {
        const PhaseListed &la = listed[p.a], &lb = listed[p.b];
        if (lb.key_index - la.key_index > AMPLI_PHASE_PARTNERS) continue; // NOT_FORMED: the table has no cell for it
        p.slot = (int64_t)pair_cell.size();
        pair_cell.push_back(la.key_index * AMPLI_PHASE_PARTNERS + (lb.key_index - la.key_index - 1));
        for (const std::string *s : {&la.ref, &la.alt, &lb.ref, &lb.alt}) pair_nt.push_back((int8_t)evidence_nt(*s, false));
    }
    return pairs;
}

const char *phase_verdict(int32_t cls, float score, double q_min)
{
    switch (cls) {
    case 1: return (double)score >= q_min ? "CIS" : "UNRESOLVED";
    case 3: return (double)score >= q_min ? "NESTED_B" : "UNRESOLVED";
    case 5: return (double)score >= q_min ? "NESTED_A" : "UNRESOLVED";
    case 6: return "TRANS";
    case 7: return "MIXED";
    default: return "UNTESTED"; // -1, and 0, 2, 4: one of the variants has no reads among the joint ones
    }
}

std::vector<std::vector<int64_t>> phase_chains(const std::vector<PhaseListed> &listed, const std::vector<PhasePair> &pairs)
{
    std::map<std::pair<int64_t, int64_t>, bool> cis;
    for (const PhasePair &p : pairs) cis[{p.a, p.b}] = p.verdict == "CIS";
    const auto linked = [&](int64_t a, int64_t b) {
        const auto it = cis.find({a, b});
        return it != cis.end() && it->second;
    };
    std::vector<int64_t> order;
    for (size_t l = 0; l < listed.size(); ++l)
        if (listed[l].key_index >= 0) order.push_back((int64_t)l);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return listed[x].key_index < listed[y].key_index; });
    std::vector<char> used(listed.size(), 0);
    std::vector<std::vector<int64_t>> chains;
    // the first unused line one position behind `last` on its chromosome that is CIS with every member of the chain, -1: none
    const auto next = [&](const std::vector<int64_t> &chain) -> int64_t {
        const PhaseListed &last = listed[chain.back()];
        for (const int64_t l : order) {
            if (used[l] || listed[l].chrom != last.chrom || listed[l].pos != last.pos + 1) continue;
            bool all = true;
            for (const int64_t m : chain) all = all && linked(m, l);
            if (all) return l;
        }
        return -1;
    };
    for (const int64_t a : order) {
        if (used[a]) continue;
        std::vector<int64_t> chain{a};
        while (chain.size() < 3) {
            const int64_t l = next(chain);
            if (l < 0) break;
            chain.push_back(l);
        }
        if (chain.size() < 2) continue;
        for (const int64_t m : chain) used[m] = 1;
        chains.push_back(chain);
    }
    return chains;
}

int64_t write_phase_files(const std::string &out_dir, const std::string &name, const std::vector<PhaseListed> &listed, std::vector<PhasePair> &pairs,
                          const int64_t *v_int, const float *v_score, const int32_t *v_class, double q_min, int64_t *mnv)
{
    const std::string ph_path = out_dir + "/" + name + ".PHASE.txt", mnv_path = out_dir + "/" + name + ".PHASE.MNV.txt";
    TempFiles tmp;
    FILE *o = tmp.open(ph_path);
    int64_t written = 0;
    for (PhasePair &p : pairs) {
        const PhaseListed &a = listed[p.a], &b = listed[p.b];
        fprintf(o, "%s\t%lld\t%s\t%s\t%lld\t%s\t%s", a.chrom.c_str(), (long long)a.pos, a.ref.c_str(), a.alt.c_str(), (long long)b.pos, b.ref.c_str(), b.alt.c_str());
        if (p.slot < 0 || v_class[p.slot] < 0) { // no cell, or no usable alleles: no counts, no score
            p.verdict = p.slot < 0 ? "NOT_FORMED" : "UNTESTED";
            p.n_aa = 0;
            fprintf(o, "\t.\t.\t.\t.\t.\t.\t.\t.\t%s\n", p.verdict.c_str());
        } else {
            const int64_t *v = v_int + p.slot * 6; // rr, ra, ar, aa, joint, other
            p.verdict = phase_verdict(v_class[p.slot], v_score[p.slot], q_min);
            p.n_aa = v[3];
            fprintf(o, "\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld", (long long)v[4], (long long)v[0], (long long)v[1], (long long)v[2], (long long)v[3], (long long)v[5]);
            const int64_t four = v[0] + v[1] + v[2] + v[3];
            if (four > 0) fprintf(o, "\t%.2f", (double)(v[3] + v[2]) * (double)(v[3] + v[1]) / (double)four);
            else fputs("\t.", o);
            fprintf(o, "\t%.4f\t%s\n", (double)v_score[p.slot], p.verdict.c_str());
        }
        ++written;
    }
    tmp.close(o, ph_path);
    o = tmp.open(mnv_path);
    std::map<std::pair<int64_t, int64_t>, int64_t> n_aa;
    for (const PhasePair &p : pairs) n_aa[{p.a, p.b}] = p.n_aa;
    int64_t chains_written = 0;
    for (const std::vector<int64_t> &chain : phase_chains(listed, pairs)) {
        std::string ref, alt;
        int64_t reads = INT64_MAX;
        for (size_t i = 0; i < chain.size(); ++i) {
            ref += listed[chain[i]].ref;
            alt += listed[chain[i]].alt;
            for (size_t j = i + 1; j < chain.size(); ++j) reads = std::min(reads, n_aa[{chain[i], chain[j]}]);
        }
        fprintf(o, "%s\t%lld\t%s\t%s\t%lld\n", listed[chain[0]].chrom.c_str(), (long long)listed[chain[0]].pos, ref.c_str(), alt.c_str(), (long long)reads);
        ++chains_written;
    }
    tmp.close(o, mnv_path);
    tmp.commit();
    if (mnv) *mnv = chains_written;
    return written;
}

int run_compute_phasing(const PhArgs &a)
{
    try {
        if (a.vcf.empty() || a.bam.empty() || a.out_dir.empty()) throw Error{AMPLI_E_INVALID, "vcf=, bam= and out= are required"};
        // refused before the device is opened: bad numbers, unreadable inputs (walk_bam opens vcf and bam again, with the same words)
        const int threads = parse_int(a.threads, "threads", 1, 1024), mbq = parse_int(a.mbq, "mbq", 0, 255), mrq = parse_int(a.mrq, "mrq", 0, 255);
        const int min_alt = parse_int(a.min_alt, "min_alt", 1), min_share = parse_int(a.min_share, "min_share", 0, 100);
        const double q_min = parse_number(a.q_min, "q_min", "> 0", [](double v) { return v > 0.0; });
        const int max_dist = parse_int(a.max_dist, "max_dist", 1);
        for (const std::string *path : {&a.vcf, &a.bam})
            if (access(path->c_str(), R_OK) != 0) throw Error{AMPLI_E_INVALID, "cannot open " + *path};

        BamDevice dev;
        int32_t *d_table = nullptr;
        uint64_t *d_stats = nullptr;
        BamSink sink;
        sink.panel = [&](BamDevice &d, int64_t P) {
            d_table = (int32_t *)d.alloc((size_t)P * PH_CELLS * sizeof(int32_t));
            d_stats = (uint64_t *)d.alloc(24);
            d.check(d.api->memset_d(d.ctx, d_table, 0, (size_t)P * PH_CELLS * sizeof(int32_t)), "ampli_memset_d");
            d.check(d.api->memset_d(d.ctx, d_stats, 0, 24), "ampli_memset_d");
        };
        sink.batch = [&](BamDevice &d, const uint8_t *d_bam, const uint64_t *d_off, int64_t n_reads, const uint64_t *d_keys, int64_t P) {
            d.check(d.api->pileup_phase(d_bam, d_off, n_reads, d_keys, P, mbq, mrq, d_table, d_stats, d.ctx), "ampli_pileup_phase");
        };
        const BamWalk w = walk_bam(a.vcf, a.bam, threads, dev, sink);
        const HipApi *api = dev.api;
        uint64_t st[3] = {0, 0, 0};
        if (w.P > 0) dev.check(api->copy_d2h(dev.ctx, st, d_stats, 24), "ampli_copy_d2h");
        dev.check(api->sync(dev.ctx), "ampli_sync");

        std::vector<PhaseListed> listed(w.lines.size());
        for (size_t l = 0; l < listed.size(); ++l) {
            const auto &v = w.lines[l];
            listed[l].chrom = v.chrom; listed[l].ref = v.ref; listed[l].alt = v.alt; listed[l].pos = v.pos; listed[l].key_index = v.key_index;
        }
        std::vector<int64_t> pair_cell;
        std::vector<int8_t> pair_nt;
        std::vector<PhasePair> pairs = phase_pairs(listed, max_dist, pair_cell, pair_nt);
        const size_t Q = pair_cell.size();
        std::vector<int64_t> v_int(Q * 6, 0);
        std::vector<float> v_score(Q, 0.0f);
        std::vector<int32_t> v_class(Q, 0);
        if (Q > 0) { // all formed pairs through one ampli_phase_score over the table where the walk left it
            int64_t *d_cell = (int64_t *)dev.alloc(Q * sizeof(int64_t)), *d_int = (int64_t *)dev.alloc(Q * 6 * sizeof(int64_t));
            int8_t *d_nt = (int8_t *)dev.alloc(Q * 4);
            float *d_score = (float *)dev.alloc(Q * sizeof(float));
            int32_t *d_class = (int32_t *)dev.alloc(Q * sizeof(int32_t));
            dev.check(api->copy_h2d(dev.ctx, d_cell, pair_cell.data(), Q * sizeof(int64_t)), "ampli_copy_h2d");
            dev.check(api->copy_h2d(dev.ctx, d_nt, pair_nt.data(), Q * 4), "ampli_copy_h2d");
            dev.check(api->phase_score(d_table, w.P, d_cell, d_nt, (int64_t)Q, min_alt, min_share, d_int, d_score, d_class, dev.ctx), "ampli_phase_score");
            dev.check(api->copy_d2h(dev.ctx, v_int.data(), d_int, Q * 6 * sizeof(int64_t)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, v_score.data(), d_score, Q * sizeof(float)), "ampli_copy_d2h");
            dev.check(api->copy_d2h(dev.ctx, v_class.data(), d_class, Q * sizeof(int32_t)), "ampli_copy_d2h");
            dev.check(api->sync(dev.ctx), "ampli_sync");
        }

        std::string base = a.bam;
        const size_t sl = base.rfind('/');
        if (sl != std::string::npos) base = base.substr(sl + 1);
        if (base.size() > 4 && base.compare(base.size() - 4, 4, ".bam") == 0) base.resize(base.size() - 4);
        int64_t mnv = 0;
        const int64_t written = write_phase_files(a.out_dir, base, listed, pairs, v_int.data(), v_score.data(), v_class.data(), q_min, &mnv);
        std::cout << "computePhasing (MI355X-native build): " << a.bam << "\n\t" << w.n_records << " alignment records (" << w.malformed << " malformed), " << st[0]
                  << " kept (mrq " << mrq << "), " << st[1] << " over two or more of " << listed.size() << " listed lines, " << st[2] << " cells counted (mbq " << mbq
                  << ")\n\t" << written << " pairs (" << Q << " scored; min_alt " << min_alt << ", min_share " << min_share << ", q_min " << a.q_min << ", max_dist "
                  << max_dist << ") written to " << a.out_dir << "/" << base << ".PHASE.txt, " << mnv << " chains to " << base << ".PHASE.MNV.txt" << std::endl;
        if (getenv("AMPLISOLVE_TIMING"))
            std::cerr << "TIMING total " << w.seconds() << " inflate " << w.t_inflate << " (" << w.threads << " threads, " << w.total_bytes << " bytes) device_wait "
                      << w.t_wait << std::endl;
        if (a.stats) {
            a.stats[0] = w.n_records; a.stats[1] = (int64_t)st[0]; a.stats[2] = (int64_t)st[1]; a.stats[3] = (int64_t)st[2]; a.stats[4] = written; a.stats[5] = mnv;
        }
        return 0;
    } catch (const Error &e) {
        std::cout << "computePhasing: " << e.msg << std::endl;
        if (a.error) *a.error = e.msg;
        return e.code ? e.code : -1;
    }
}

} // namespace ampli
