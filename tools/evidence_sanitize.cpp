// tools/evidence_sanitize.cpp -- the host side of computeReadEvidence under AddressSanitizer + UBSan: the host scorer
// (evidence_score_host over ampli_ev_* of csrc/ampli_math.h) and the writer of the command's two files, in a stand-alone program over the
// host library's sources, run once on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/evidence_sanitize \
//       tools/evidence_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/evidence_sanitize
// A few hundred random histogram planes -- empty sides, single bins, depths up to 2^29 a bin (N at and beyond 2^30, where U2 would leave
// int64), alleles inside and outside their ranges -- in heap buffers of exactly the sizes the contract names (a read or a store past either
// end is a report) go through the scorer; its outputs are checked against the definition's invariants.  Then the planes go through
// write_evidence_files; the files are read back and their line counts checked, and a directory that cannot be written to must leave nothing.
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
    const size_t L = 300, CELLS = 4 * AMPLI_EVIDENCE_METRICS * AMPLI_EVIDENCE_BINS;
    std::vector<int32_t> hist(L * CELLS, 0), med(L * AMPLI_EVIDENCE_METRICS * 2, 7);
    std::vector<int8_t> ref(L), alt(L), used(L, 7);
    std::vector<int64_t> ints(L * AMPLI_EVIDENCE_METRICS * 3, 7);
    std::vector<double> z2(L * AMPLI_EVIDENCE_METRICS, 7.0);
    static const int32_t depths[] = {0, 1, 3, 10, 40, 300, 5000, 200000, 1 << 29, 0x7fffffff};
    for (size_t l = 0; l < L; ++l) {
        for (int nt = 0; nt < 4; ++nt) {
            const int32_t depth = depths[rnd() % (l < 250 ? 8 : 10)];
            for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) {
                const int nb = 1 + (int)(rnd() % 6);
                for (int k = 0; k < nb; ++k) hist[l * CELLS + ((size_t)nt * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS + rnd() % AMPLI_EVIDENCE_BINS] = depth / nb;
            }
        }
        ref[l] = (int8_t)((int)(rnd() % 7) - 2);
        alt[l] = (int8_t)((int)(rnd() % 8) - 3);
    }
    evidence_score_host(hist.data(), (int64_t)L, ref.data(), alt.data(), ints.data(), med.data(), z2.data(), used.data());
    long tested = 0;
    for (size_t l = 0; l < L; ++l) {
        const bool ref_ok = ref[l] >= 0 && ref[l] <= 3;
        CHECK(used[l] >= -1 && used[l] <= 3 && (used[l] < 0 || (ref_ok && used[l] != ref[l])));
        if (alt[l] >= 0 && alt[l] <= 3 && ref_ok && alt[l] != ref[l]) CHECK(used[l] == alt[l]);
        if (alt[l] == -1 && ref_ok) CHECK(used[l] >= 0);
        for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) {
            const size_t c = l * AMPLI_EVIDENCE_METRICS + m;
            const int64_t n_ref = ints[c * 3], n_alt = ints[c * 3 + 1], u2 = ints[c * 3 + 2];
            CHECK(n_ref >= 0 && n_alt >= 0 && (ref_ok || n_ref == 0) && (used[l] >= 0 || n_alt == 0));
            CHECK((med[c * 2] == -1) == (n_ref == 0) && (med[c * 2 + 1] == -1) == (n_alt == 0) && med[c * 2] < AMPLI_EVIDENCE_BINS && med[c * 2 + 1] < AMPLI_EVIDENCE_BINS);
            CHECK(std::isfinite(z2[c]));
            if (u2 < 0) {
                CHECK(u2 == -1 && z2[c] == 0.0);
            } else {
                CHECK(n_ref > 0 && n_alt > 0 && n_ref + n_alt < (1ll << 30) && u2 <= 2 * n_ref * n_alt);
                CHECK((z2[c] < 0.0) == (u2 < n_ref * n_alt) && (z2[c] > 0.0) == (u2 > n_ref * n_alt));
                ++tested;
            }
        }
    }
    CHECK(tested > 100);
    evidence_score_host(hist.data(), 0, ref.data(), alt.data(), ints.data(), med.data(), z2.data(), used.data()); // P = 0: nothing is touched

    // the writers, from host arrays alone
    char dir_t[] = "/tmp/evidence_sanitize_XXXXXX";
    CHECK(mkdtemp(dir_t) != nullptr);
    const std::string dir = dir_t;
    std::vector<EvidenceListed> listed(L);
    for (size_t l = 0; l < L; ++l) {
        listed[l].chrom = l % 17 ? "chr1" : "chrUn_a_rather_long_name_of_a_contig_that_is_not_in_the_header";
        listed[l].pos = 1 + (int64_t)(rnd() % 100000);
        listed[l].ref = ref[l] >= 0 && ref[l] <= 3 ? std::string(1, "ACGT"[ref[l]]) : "AT";
        listed[l].alt = alt[l] >= 0 && alt[l] <= 3 ? std::string(1, "ACGT"[alt[l]]) : alt[l] == -1 ? "." : "GATTACA";
    }
    for (const double z_min : {0.5, 3.0, 1e6}) {
        const int64_t written = write_evidence_files(dir, "S", listed, hist.data(), ints.data(), med.data(), z2.data(), ref.data(), used.data(), 4, z_min);
        CHECK(written == (int64_t)L && lines_of(dir + "/S.EVIDENCE.txt") == (long)L && lines_of(dir + "/S.EVIDENCE.HIST.txt") > (long)L && entries(dir) == 2);
    }
    CHECK(write_evidence_files(dir, "E", {}, hist.data(), ints.data(), med.data(), z2.data(), ref.data(), used.data(), 1, 3.0) == 0);
    CHECK(lines_of(dir + "/E.EVIDENCE.txt") == 0 && lines_of(dir + "/E.EVIDENCE.HIST.txt") == 0 && entries(dir) == 4);
    bool refused = false;
    try {
        write_evidence_files(dir + "/missing", "S", listed, hist.data(), ints.data(), med.data(), z2.data(), ref.data(), used.data(), 4, 3.0);
    } catch (const Error &) {
        refused = true;
    }
    CHECK(refused && entries(dir) == 4);
    CHECK(evidence_nt("A", false) == 0 && evidence_nt("t", true) == 3 && evidence_nt(".", true) == -1 && evidence_nt(".", false) == -2 && evidence_nt("", true) == -2 &&
          evidence_nt("AC", true) == -2 && evidence_nt("N", false) == -2);
    for (const char *f : {"/S.EVIDENCE.txt", "/S.EVIDENCE.HIST.txt", "/E.EVIDENCE.txt", "/E.EVIDENCE.HIST.txt"}) unlink((dir + f).c_str());
    rmdir(dir.c_str());
    printf("evidence_sanitize: %zu planes scored (%ld tested cells), files written three times: clean\n", L, tested);
    return 0;
}
