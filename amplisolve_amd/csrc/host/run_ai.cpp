// amplisolve_amd/csrc/host/run_ai.cpp -- run_allelic_imbalance, one of the project's own command lines
// AmpliSolveAllelicImbalance: the allelic balance of every file at the het sites of its germline, pooled per gene.  Pass 1
// streams the normals: every chunk is encoded into its rows of the resident genotype planes and added to the het-site reference.
// Pass 2 streams the tumours (tumour_dir "-": the normals again, the null calibration): every chunk is encoded too, takes its germline
// from its own planes or from the normal that `pairs` names, and fills its rows of the resident site planes.  Then the region sums on
// the device -- one region per gene string and ALL -- and the verdicts and the four files here.  Records never stay on the device.
#include "command.hpp"

#include <map>
#include <set>

#include "../ampli_math.h"

namespace ampli {

namespace {

const char *const kScore = "%.4f", *const kShare = "%.5f";
const char *const kPair[AMPLI_AI_PAIRS] = {"A/C", "A/G", "A/T", "C/G", "C/T", "G/T"};
const char *const kVerdict[3] = {"FEW", "BALANCED", "IMBALANCED"};

// tumourName<TAB>normalName per line, read before the device is opened; an empty line is skipped
std::vector<std::pair<std::string, std::string>> read_pairs(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw Error{AMPLI_E_INVALID, "cannot read pairs file " + path};
    std::vector<std::pair<std::string, std::string>> out;
    std::set<std::string> seen;
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || tab == 0 || tab + 1 >= line.size() || line.find('\t', tab + 1) != std::string::npos)
            throw Error{AMPLI_E_INVALID, "pairs line " + std::to_string(no) + " must be tumourName<TAB>normalName, got '" + line + "'"};
        const std::string t = line.substr(0, tab), n = line.substr(tab + 1);
        if (!seen.insert(t).second) throw Error{AMPLI_E_INVALID, "pairs line " + std::to_string(no) + " names " + t + " a second time"};
        out.emplace_back(t, n);
    }
    return out;
}

} // namespace

int run_allelic_imbalance(const AiArgs &a)
{
    return run_command("AmpliSolveAllelicImbalance", [&]() -> int {
        ampli_allelic_params prm{100, 5, 1};
        prm.min_depth = parse_int(a.min_depth, "min_depth", 1);
        prm.min_normals = parse_int(a.min_normals, "min_normals", 1);
        const double site_q = parse_number(a.site_q, "site_q", "in [0, 100]", [](double v) { return v >= 0.0 && v <= 100.0; });
        const int min_sites = parse_int(a.min_sites, "min_sites", 1);
        const double q_min = parse_number(a.q_min, "q_min", "in [0, 300]", [](double v) { return v >= 0.0 && v <= 300.0; });
        const double min_imbalance = parse_number(a.min_imbalance, "min_imbalance", "in [0, 1]", [](double v) { return v >= 0.0 && v <= 1.0; });
        if (a.pairs.empty()) throw Error{AMPLI_E_INVALID, "pairs must be a file or self, got ''"};
        std::vector<std::pair<std::string, std::string>> pairs;
        if (a.pairs != "self") pairs = read_pairs(a.pairs);
        require_single_gpu("AmpliSolveAllelicImbalance");
        const bool with_tumours = a.tumour_dir != "-";
        if (!pairs.empty()) { // the names, against the directories' listings: refused before the device is opened
            const FileSet normals = list_count_files(a.germline_dir, std::string());
            const FileSet files = with_tumours ? list_count_files(a.tumour_dir, std::string()) : normals;
            auto has = [](const FileSet &set, const std::string &name) {
                for (const auto &f : set)
                    if (f.second == name) return true;
                return false;
            };
            for (const auto &pr : pairs) {
                if (!has(files, pr.first))
                    throw Error{AMPLI_E_INVALID, "pairs names '" + pr.first + "', which is no count file of " + (with_tumours ? a.tumour_dir : a.germline_dir)};
                if (!has(normals, pr.second)) throw Error{AMPLI_E_INVALID, "pairs names the normal '" + pr.second + "', which is no count file of " + a.germline_dir};
            }
        }
        ampli_genotype_params geno{100, 100, 250, 750, 900};
        geno.min_depth = prm.min_depth;
        std::cout << "AmpliSolveAllelicImbalance: panel " << a.panel_design << ", normals " << a.germline_dir << ", tumours "
                  << (with_tumours ? a.tumour_dir : std::string("the normals again")) << ", pairs " << a.pairs << ", min_depth " << prm.min_depth
                  << ", min_normals " << prm.min_normals << ", site_q " << site_q << ", min_sites " << min_sites << ", q_min " << q_min << ", min_imbalance "
                  << min_imbalance << ", output " << a.output_dir << std::endl;
        DevAsync dev_async;
        dev_async.start();
        CohortInputs in;
        load_cohort(in, a.panel_design, nullptr, std::string(), a.germline_dir, a.tumour_dir, true);
        const Panel &panel = in.panel;
        const int n_normals = in.n_normals, S2 = with_tumours ? in.n_tumours : in.n_normals, base2 = with_tumours ? n_normals : 0;
        const int64_t P = in.P;
        const size_t W = (size_t)((P + 63) / 64);
        if (S2 <= 0) throw Error{AMPLI_E_INVALID, "no count files in " + a.tumour_dir};
        // the germline row of every file of pass 2: its own planes (rows n_normals ..) or the planes of the normal that `pairs` names
        std::vector<int32_t> row_g((size_t)S2);
        for (int s = 0; s < S2; ++s) row_g[(size_t)s] = n_normals + s;
        for (const auto &pr : pairs) {
            int t = -1, n = -1;
            for (int s = 0; s < S2; ++s)
                if (in.names[(size_t)(base2 + s)] == pr.first) t = s;
            for (int s = 0; s < n_normals; ++s)
                if (in.names[(size_t)s] == pr.second) n = s;
            if (t < 0) throw Error{AMPLI_E_INVALID, "pairs names " + pr.first + ", which is not a sample of " + (with_tumours ? a.tumour_dir : a.germline_dir)};
            if (n < 0) throw Error{AMPLI_E_INVALID, "pairs names the normal " + pr.second + ", which is not a sample of " + a.germline_dir};
            row_g[(size_t)t] = n;
        }
        // the regions: one per gene string (BED column 6) -- the unique positions of the gene's rows, in walk order -- and ALL
        std::map<std::string, std::vector<uint32_t>> genes; // in the order of the gene strings' bytes
        {
            std::map<std::string, std::vector<uint8_t>> seen;
            size_t wo = 0;
            for (const BedRow &r : panel.rows) {
                const size_t len = r.end >= r.start ? (size_t)((int64_t)r.end - r.start + 1) : 0;
                std::vector<uint32_t> &g = genes[r.gene];
                std::vector<uint8_t> &sn = seen[r.gene];
                if (sn.empty()) sn.assign((size_t)P, 0);
                for (size_t k = 0; k < len; ++k) {
                    const uint32_t p = panel.walk[wo + k];
                    if (!sn[p]) { sn[p] = 1; g.push_back(p); }
                }
                wo += len;
            }
        }
        std::vector<std::string> reg_names;
        std::vector<uint32_t> reg_off(1, 0u), reg_pos;
        for (const auto &g : genes) {
            reg_names.push_back(g.first);
            reg_pos.insert(reg_pos.end(), g.second.begin(), g.second.end());
            reg_off.push_back((uint32_t)reg_pos.size());
        }
        reg_names.push_back("ALL");
        for (int64_t p = 0; p < P; ++p) reg_pos.push_back((uint32_t)p);
        reg_off.push_back((uint32_t)reg_pos.size());
        const int R = (int)reg_names.size();
        const int64_t RW = (int64_t)reg_pos.size();
        Dev &dev = dev_async.get();
        const size_t free_b = device_free_bytes(dev);
        // what stays resident: the planes of the normals and of pass 2, the reference, the site planes and the sums; beside them one chunk
        const size_t n_g = (size_t)n_normals + (size_t)S2, cells = (size_t)S2 * (size_t)P;
        const size_t plane_bytes = n_g * AMPLI_GENO_PLANES * W * 8, ref_bytes = (size_t)AMPLI_AI_REF_PLANES * AMPLI_AI_PAIRS * (size_t)P * 8;
        const size_t site_bytes = cells * (sizeof(float) + 2 * sizeof(int32_t) + sizeof(double) + 1);
        const size_t sum_bytes = (size_t)S2 * (size_t)R * AMPLI_AI_SUMS * 8 + (size_t)(RW + R + 1) * 4;
        const size_t reserve = (size_t)1 << 30;
        require_fits(plane_bytes + ref_bytes + site_bytes + sum_bytes, reserve, free_b,
                     "the samples do not fit the device: " + std::to_string(plane_bytes) + " bytes of genotype planes, " + std::to_string(ref_bytes) +
                         " bytes of het-site reference, " + std::to_string(site_bytes) + " bytes of site planes and " + std::to_string(sum_bytes) +
                         " bytes of region sums and lists for " + std::to_string(n_normals) + " normals and " + std::to_string(S2) + " files, " +
                         std::to_string(reserve) + " bytes kept for the streamed records, " + std::to_string(free_b) + " bytes free");
        uint64_t *d_planes = dev.alloc<uint64_t>(n_g * AMPLI_GENO_PLANES * W);
        int64_t *d_ref = dev.alloc<int64_t>(ref_bytes / 8);
        dev.check(dev.api->memset_d(dev.ctx, d_ref, 0, ref_bytes), "memset");
        float *d_q = dev.alloc<float>(cells);
        int32_t *d_km = dev.alloc<int32_t>(cells * 2);
        double *d_v = dev.alloc<double>(cells);
        uint8_t *d_code = dev.alloc<uint8_t>(cells);
        int64_t *d_sums = dev.alloc<int64_t>((size_t)S2 * (size_t)R * AMPLI_AI_SUMS);
        const uint32_t *d_off = dev.upload(reg_off.data(), reg_off.size());
        const uint32_t *d_pos = dev.upload(reg_pos.data(), reg_pos.size());
        const int32_t *d_row_g = dev.upload(row_g.data(), row_g.size());
        DevSlot slot;
        // pass 1: the normals alone
        const FileSet tumours = in.sets[1];
        in.sets[1].clear();
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            uint64_t *pl = d_planes + (size_t)first * AMPLI_GENO_PLANES * W;
            dev.check(dev.api->genotype_planes_records(dev.ctx, &r, P, &geno, pl), "ampli_genotype_planes_records");
            dev.check(dev.api->hetsite_reference_records(dev.ctx, &r, P, pl, prm.min_depth, d_ref), "ampli_hetsite_reference_records");
        });
        // pass 2: the tumours alone (`first` counts from n_normals), or the normals again
        in.sets[1] = tumours;
        for_each_chunk(dev, in, slot, [&](const ampli_records &r, Chunk &, const int first) {
            const size_t s = (size_t)(first - base2);
            dev.check(dev.api->genotype_planes_records(dev.ctx, &r, P, &geno, d_planes + ((size_t)n_normals + s) * AMPLI_GENO_PLANES * W),
                      "ampli_genotype_planes_records");
            dev.check(dev.api->allelic_site_records(dev.ctx, &r, P, d_planes, (int32_t)n_g, d_row_g + s, d_ref, &prm, d_q + s * (size_t)P,
                                                    d_km + s * (size_t)P * 2, d_v + s * (size_t)P, d_code + s * (size_t)P),
                      "ampli_allelic_site_records");
        }, with_tumours ? 1 : 0);
        dev.check(dev.api->allelic_region_sums(dev.ctx, d_q, d_km, d_v, d_code, S2, P, R, d_off, d_pos, RW, site_q, d_sums), "ampli_allelic_region_sums");
        std::vector<int64_t> ref(ref_bytes / 8), sums((size_t)S2 * (size_t)R * AMPLI_AI_SUMS);
        std::vector<float> q(cells);
        std::vector<int32_t> km(cells * 2);
        std::vector<double> v(cells);
        std::vector<uint8_t> code(cells);
        dev.download(ref.data(), (const int64_t *)d_ref, ref.size());
        dev.download(sums.data(), (const int64_t *)d_sums, sums.size());
        dev.download(q.data(), (const float *)d_q, q.size());
        dev.download(km.data(), (const int32_t *)d_km, km.size());
        dev.download(v.data(), (const double *)d_v, v.size());
        dev.download(code.data(), (const uint8_t *)d_code, code.size());
        dev.sync();
        char b[1024];
        auto where = [&](int64_t p) { return panel.chroms[(size_t)panel.pos_chrom[(size_t)p]] + "\t" + std::to_string(panel.pos_coord[(size_t)p]); };
        // Allelic_Reference.txt: the cells with CNT > 0
        std::string reference = "Chrom\tPosition\tPair\tNormals\tLo\tHi\tShare\n";
        long long ref_cells = 0, ref_usable = 0;
        const size_t plane = (size_t)AMPLI_AI_PAIRS * (size_t)P;
        for (int64_t p = 0; p < P; ++p)
            for (int c = 0; c < AMPLI_AI_PAIRS; ++c) {
                const size_t at = (size_t)c * (size_t)P + (size_t)p;
                const int64_t cnt = ref[AMPLI_AI_REF_CNT * plane + at], lo = ref[AMPLI_AI_REF_LO * plane + at], hi = ref[AMPLI_AI_REF_HI * plane + at];
                if (cnt <= 0) continue;
                ++ref_cells;
                ref_usable += cnt >= prm.min_normals && lo > 0 && hi > 0 ? 1 : 0;
                snprintf(b, sizeof b, "\t%s\t%lld\t%lld\t%lld\t", kPair[c], (long long)cnt, (long long)lo, (long long)hi);
                reference += where(p) + b + num(kShare, lo + hi > 0 ? (double)lo / (double)(lo + hi) : (double)NAN) + "\n";
            }
        // Allelic_Sites.txt: every tested site
        std::string sites = "Sample\tChrom\tPosition\tPair\tReference\tKlo\tM\tExpected\tObserved\tQ\n";
        long long tested = 0, tested_half = 0, significant = 0;
        for (int s = 0; s < S2; ++s)
            for (int64_t p = 0; p < P; ++p) {
                const size_t at = (size_t)s * (size_t)P + (size_t)p;
                const int status = code[at] >> 3;
                if (status < AMPLI_AI_TESTED_REF) continue;
                ++tested;
                tested_half += status == AMPLI_AI_TESTED_HALF;
                significant += q[at] != AMPLI_AI_NA && (double)fabsf(q[at]) >= site_q;
                snprintf(b, sizeof b, "\t%s\t%s\t%d\t%d\t", kPair[code[at] & 7], status == AMPLI_AI_TESTED_REF ? "NORMALS" : "HALF", km[2 * at], km[2 * at + 1]);
                sites += in.names[(size_t)(base2 + s)] + "\t" + where(p) + b + num(kShare, v[at]) + "\t" +
                         num(kShare, (double)km[2 * at] / (double)km[2 * at + 1]) + "\t" + num(kScore, q[at] == AMPLI_AI_NA ? (double)NAN : (double)q[at]) + "\n";
            }
        // Allelic_Genes.txt: every (sample, region)
        std::string gene_rows = "Sample\tRegion\tSites\tSignificant\tDepth\tDev16\tQ20\tQ\tImbalance\tVerdict\tFractionIfCopyNeutralLOH\tFractionIfSingleCopyLoss\n";
        long long by_verdict[3] = {0, 0, 0};
        for (int s = 0; s < S2; ++s)
            for (int r = 0; r < R; ++r) {
                const int64_t *x = sums.data() + ((size_t)s * (size_t)R + (size_t)r) * AMPLI_AI_SUMS;
                double Q, imb;
                const int verdict = ampli_ai_region_verdict(x, min_sites, q_min, min_imbalance, &Q, &imb);
                ++by_verdict[verdict];
                snprintf(b, sizeof b, "\t%lld\t%lld\t%lld\t%lld\t%lld\t", (long long)x[0], (long long)x[1], (long long)x[2], (long long)x[3], (long long)x[4]);
                gene_rows += in.names[(size_t)(base2 + s)] + "\t" + reg_names[(size_t)r] + b + num(kScore, Q) + "\t" + num(kShare, imb) + "\t" + kVerdict[verdict] +
                             "\t" + num(kShare, std::isnan(imb) ? imb : ampli_ai_fraction_cnloh(imb)) + "\t" +
                             num(kShare, std::isnan(imb) ? imb : ampli_ai_fraction_loss(imb)) + "\n";
            }
        // Allelic_Summary.txt
        const long long regions_tested = by_verdict[AMPLI_AI_BALANCED] + by_verdict[AMPLI_AI_IMBALANCED];
        snprintf(b, sizeof b,
                 "normals=%d\nfiles=%d\nmode=%s\npairs=%zu\npositions=%lld\nregions=%d\nmin_depth=%d\nmin_normals=%d\nsite_q=%g\nmin_sites=%d\nq_min=%g\n"
                 "min_imbalance=%g\nreference_cells=%lld\nreference_cells_usable=%lld\nsites_tested=%lld\nsites_tested_half=%lld\nsites_significant=%lld\n"
                 "regions_few=%lld\nregions_balanced=%lld\nregions_imbalanced=%lld\nshare_flagged=%s\n",
                 n_normals, S2, with_tumours ? "tumours" : "null_calibration", pairs.size(), (long long)P, R, prm.min_depth, prm.min_normals, site_q, min_sites,
                 q_min, min_imbalance, ref_cells, ref_usable, tested, tested_half, significant, by_verdict[AMPLI_AI_FEW], by_verdict[AMPLI_AI_BALANCED],
                 by_verdict[AMPLI_AI_IMBALANCED],
                 num(kShare, regions_tested > 0 ? (double)by_verdict[AMPLI_AI_IMBALANCED] / (double)regions_tested : (double)NAN).c_str());
        std::string summary = b;
        summary += "Sample\tGermline\n";
        for (int s = 0; s < S2; ++s)
            summary += in.names[(size_t)(base2 + s)] + "\t" + (row_g[(size_t)s] < n_normals ? in.names[(size_t)row_g[(size_t)s]] : std::string("self")) + "\n";
        write_files(a.output_dir,
                    {{"Allelic_Reference.txt", reference}, {"Allelic_Sites.txt", sites}, {"Allelic_Genes.txt", gene_rows}, {"Allelic_Summary.txt", summary}});
        std::cout << S2 << " files, " << R << " regions: " << by_verdict[AMPLI_AI_IMBALANCED] << " (file, region) IMBALANCED, " << by_verdict[AMPLI_AI_BALANCED]
                  << " BALANCED, " << by_verdict[AMPLI_AI_FEW] << " FEW" << std::endl;
        return 0;
    });
}

} // namespace ampli
