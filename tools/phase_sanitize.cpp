// tools/phase_sanitize.cpp -- the host side of computePhasing under AddressSanitizer + UBSan: the host scorer (phase_score_host
// over ampli_ph_* of csrc/ampli_math.h), the pair builder, the chain builder and the writers of the command's two files, in a stand-alone
// program over the host library's sources, run once on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/phase_sanitize \
//       tools/phase_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/phase_sanitize
// A few hundred random joint tables -- empty cells, single corners, counts up to 2^31 - 1, lists with positions listed twice, unknown
// chromosomes, unusable alleles, pairs beyond K keys and beyond max_dist -- in heap buffers of exactly the sizes the contract names (a read
// or a store past either end is a report) go through the builders and the scorer; their outputs are checked against the definition's
// invariants.  Then they go through write_phase_files; the files are read back and their line counts checked, and a directory that cannot
// be written to must leave nothing.
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>

#include "../amplisolve_amd/csrc/host/host.hpp"

using namespace ampli;

static uint64_t rng_state = 0x0123456789ABCDEFull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

static long lines_of(const std::string &path)
{
    std::ifstream in(path);
    if (!in) return -1;
    long n = 0;
    std::string l;
    while (std::getline(in, l)) ++n;
    return n;
}

static int entries(const std::string &dir)
{
    DIR *d = opendir(dir.c_str());
    if (!d) return -1;
    int n = 0;
    while (dirent *e = readdir(d))
        if (e->d_name[0] != '.') ++n;
    closedir(d);
    return n;
}

int main()
{
    constexpr int K = AMPLI_PHASE_PARTNERS, S = AMPLI_PHASE_STATES, PAIR = S * S;
    static const int32_t depths[] = {0, 0, 1, 3, 10, 40, 300, 5000, 200000, 0x7fffffff};
    static const char *const alleles[] = {"A", "C", "G", "T", "a", "t", "AT", "N", ".", ""};
    char dir_t[] = "/tmp/phase_sanitize_XXXXXX";
    CHECK(mkdtemp(dir_t) != nullptr);
    const std::string dir = dir_t;
    long tables = 0, scored = 0, not_formed = 0, chains_seen = 0, classes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int round = 0; round < 300; ++round) {
        // a list: positions on two known chromosomes and an unknown one, some listed twice, in any order
        const int64_t P = 1 + (int64_t)(rnd() % 40);
        const bool planted = round % 4 == 0; // every line A > C and every cell 300 reads with the ref at both keys, 40 with the alt at both: CIS throughout
        std::vector<int64_t> key_pos(P);
        std::vector<int> key_chr(P);
        for (int64_t i = 0; i < P; ++i) {
            key_chr[i] = i < P / 2 ? 0 : 1;
            key_pos[i] = (i && key_chr[i] == key_chr[i - 1] ? key_pos[i - 1] : 100) + 1 + (int64_t)(rnd() % (round % 3 ? 3 : 40));
        }
        std::vector<PhaseListed> listed;
        for (int64_t i = 0; i < P; ++i)
            for (int rep = 0; rep < (rnd() % 5 == 0 ? 2 : 1); ++rep) {
                PhaseListed v;
                v.chrom = key_chr[i] ? "chr8" : "chr1";
                v.pos = key_pos[i];
                v.key_index = i;
                v.ref = planted ? "A" : alleles[rnd() % (rnd() % 4 ? 4 : 10)];
                v.alt = planted ? "C" : alleles[rnd() % (rnd() % 4 ? 4 : 10)];
                listed.push_back(v);
            }
        for (int u = 0; u < (int)(rnd() % 3); ++u) {
            PhaseListed v;
            v.chrom = "chrUn_a_rather_long_name_of_a_contig_that_is_not_in_the_header";
            v.pos = 100 + (int64_t)(rnd() % 50);
            v.ref = "A"; v.alt = "C";
            listed.push_back(v);
        }
        for (size_t i = listed.size(); i > 1; --i) std::swap(listed[i - 1], listed[rnd() % i]);
        // the table, in a buffer of exactly P K 25 words
        std::vector<int32_t> table((size_t)P * K * PAIR, 0);
        for (int64_t i = 0; i < P; ++i)
            for (int k = 0; k < K && i + 1 + k < P; ++k) {
                const int32_t depth = depths[rnd() % (round < 250 ? 9 : 10)];
                const int filled = 1 + (int)(rnd() % 6);
                for (int f = 0; f < filled && !planted; ++f) table[((size_t)i * K + k) * PAIR + rnd() % PAIR] = depth / filled;
                if (planted) { table[((size_t)i * K + k) * PAIR] = 300; table[((size_t)i * K + k) * PAIR + S + 1] = 40; }
            }
        const int64_t max_dist = 1 + (int64_t)(rnd() % 60);
        std::vector<int64_t> pair_cell;
        std::vector<int8_t> pair_nt;
        std::vector<PhasePair> pairs = phase_pairs(listed, max_dist, pair_cell, pair_nt);
        const size_t Q = pair_cell.size();
        CHECK(pair_nt.size() == Q * 4);
        std::set<std::pair<int64_t, int64_t>> seen;
        size_t formed = 0;
        for (size_t x = 0; x < pairs.size(); ++x) {
            const PhasePair &p = pairs[x];
            const PhaseListed &la = listed[p.a], &lb = listed[p.b];
            CHECK(la.key_index >= 0 && lb.key_index > la.key_index && la.chrom == lb.chrom && lb.pos - la.pos > 0 && lb.pos - la.pos <= max_dist);
            CHECK(seen.insert({p.a, p.b}).second);
            if (x) CHECK(std::make_pair(listed[pairs[x - 1].a].key_index, listed[pairs[x - 1].b].key_index) <= std::make_pair(la.key_index, lb.key_index));
            if (lb.key_index - la.key_index <= K) {
                CHECK(p.slot == (int64_t)formed && pair_cell[formed] == la.key_index * K + (lb.key_index - la.key_index - 1));
                ++formed;
            } else {
                CHECK(p.slot == -1);
                ++not_formed;
            }
        }
        CHECK(formed == Q);
        // the scorer, its outputs in buffers of exactly Q 6, Q and Q
        const int32_t min_alt = 1 + (int32_t)(rnd() % 6), min_share = (int32_t)(rnd() % 101);
        std::vector<int64_t> v_int(Q * 6, 7);
        std::vector<float> v_score(Q, 7.0f);
        std::vector<int32_t> v_class(Q, 7);
        phase_score_host(table.data(), P, pair_cell.data(), pair_nt.data(), (int64_t)Q, min_alt, min_share, v_int.data(), v_score.data(), v_class.data());
        for (size_t q = 0; q < Q; ++q) {
            const int64_t *v = &v_int[q * 6];
            CHECK(v_class[q] >= -1 && v_class[q] <= 7 && std::isfinite(v_score[q]) && v_score[q] >= -100.0f && v_score[q] <= 100.0f);
            ++classes[v_class[q] + 1];
            if (v_class[q] < 0) {
                CHECK(v[0] == -1 && v[1] == -1 && v[2] == -1 && v[3] == -1 && v[4] == -1 && v[5] == -1 && v_score[q] == 0.0f);
                continue;
            }
            CHECK(v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[3] >= 0 && v[5] >= 0 && v[4] == v[0] + v[1] + v[2] + v[3] + v[5]);
            if (v[3] * v[0] > v[2] * v[1]) CHECK(v_score[q] >= 0.0f); // (counts below 2^31: the products stay inside int64)
            if (v[3] * v[0] < v[2] * v[1]) CHECK(v_score[q] <= 0.0f);
            if ((v_class[q] & 1) != 0) CHECK(v[3] >= min_alt);
            if ((v_class[q] & 2) != 0) CHECK(v[2] >= min_alt);
            if ((v_class[q] & 4) != 0) CHECK(v[1] >= min_alt);
            ++scored;
        }
        // a pair cell and an nt outside their ranges read nothing
        if (Q > 0) {
            const int64_t bad_cell[4] = {-1, P * K, P * K + 7, (P - 1) * K};
            const int8_t ok_nt[16] = {0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1};
            int64_t o_int[24];
            float o_score[4];
            int32_t o_class[4];
            phase_score_host(table.data(), P, bad_cell, ok_nt, 4, min_alt, min_share, o_int, o_score, o_class);
            for (int q = 0; q < 4; ++q) CHECK(o_class[q] == -1 && o_int[q * 6] == -1 && o_score[q] == 0.0f);
        }
        // the writers
        const double q_min = round % 2 ? 13.0 : 0.5;
        int64_t mnv = -1;
        const int64_t written = write_phase_files(dir, "S", listed, pairs, v_int.data(), v_score.data(), v_class.data(), q_min, &mnv);
        CHECK(written == (int64_t)pairs.size() && lines_of(dir + "/S.PHASE.txt") == (long)pairs.size() && lines_of(dir + "/S.PHASE.MNV.txt") == (long)mnv && entries(dir) == 2);
        std::vector<char> used(listed.size(), 0);
        const std::vector<std::vector<int64_t>> chains = phase_chains(listed, pairs);
        CHECK((int64_t)chains.size() == mnv);
        for (const auto &chain : chains) {
            CHECK(chain.size() == 2 || chain.size() == 3);
            for (size_t i = 0; i < chain.size(); ++i) {
                CHECK(!used[chain[i]]);
                used[chain[i]] = 1;
                if (i) CHECK(listed[chain[i]].pos == listed[chain[i - 1]].pos + 1 && listed[chain[i]].chrom == listed[chain[0]].chrom);
            }
            ++chains_seen;
        }
        for (const PhasePair &p : pairs) CHECK(!p.verdict.empty() && (p.slot >= 0) == (p.verdict != "NOT_FORMED"));
        ++tables;
    }
    CHECK(scored > 1000);
    CHECK(not_formed > 50);
    CHECK(chains_seen > 20);
    for (int c = 0; c < 9; ++c) CHECK(classes[c] > 0);
    // Q = 0 touches nothing; an empty list writes two empty files; a directory that cannot be written to leaves nothing
    phase_score_host(nullptr, 0, nullptr, nullptr, 0, 4, 10, nullptr, nullptr, nullptr);
    std::vector<PhasePair> none;
    int64_t mnv = -1;
    CHECK(write_phase_files(dir, "E", {}, none, nullptr, nullptr, nullptr, 13.0, &mnv) == 0 && mnv == 0);
    CHECK(lines_of(dir + "/E.PHASE.txt") == 0 && lines_of(dir + "/E.PHASE.MNV.txt") == 0 && entries(dir) == 4);
    bool refused = false;
    try {
        write_phase_files(dir + "/missing", "S", {}, none, nullptr, nullptr, nullptr, 13.0, nullptr);
    } catch (const Error &) {
        refused = true;
    }
    CHECK(refused && entries(dir) == 4);
    CHECK(strcmp(phase_verdict(-1, 50.0f, 13.0), "UNTESTED") == 0 && strcmp(phase_verdict(1, 13.0f, 13.0), "CIS") == 0 && strcmp(phase_verdict(1, 12.99f, 13.0), "UNRESOLVED") == 0 &&
          strcmp(phase_verdict(3, 20.0f, 13.0), "NESTED_B") == 0 && strcmp(phase_verdict(5, 20.0f, 13.0), "NESTED_A") == 0 && strcmp(phase_verdict(6, -100.0f, 13.0), "TRANS") == 0 &&
          strcmp(phase_verdict(7, 0.0f, 13.0), "MIXED") == 0 && strcmp(phase_verdict(2, 99.0f, 13.0), "UNTESTED") == 0);
    for (const char *f : {"/S.PHASE.txt", "/S.PHASE.MNV.txt", "/E.PHASE.txt", "/E.PHASE.MNV.txt"}) unlink((dir + f).c_str());
    rmdir(dir.c_str());
    printf("phase_sanitize: %ld tables, %ld scored pairs, %ld pairs not formed, %ld chains, files written %ld times: clean\n", tables, scored, not_formed, chains_seen, tables);
    return 0;
}
