// tools/amplicon_count_sanitize.cpp -- the host side of computeAmpliconCounts under AddressSanitizer + UBSan: the builder of
// the sorted amplicon arrays and the writers of the command's files, in a stand-alone program over the host library's sources, run once
// on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/amplicon_count_sanitize \
//       tools/amplicon_count_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/amplicon_count_sanitize
// Random BED rows -- nested, repeated, on unknown chromosomes, with start 0, end < start and of length 1 -- go through amplicon_arrays;
// its outputs are checked against the definition (sorted, reach monotone, prefix sums, the permutation both ways).  Then counts of
// exactly the sizes the contract names (heap buffers: a read past either end is a report) go through write_amplicon_files with and
// without layers, listed positions repeated and on unknown chromosomes; the files are read back and their line counts checked, and a
// directory that cannot be written to must leave nothing behind.
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
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
    char tmpl[] = "/tmp/amplicon_count_sanitize.XXXXXX";
    const char *root = mkdtemp(tmpl);
    CHECK(root != nullptr);
    const std::string out = std::string(root) + "/out", lay = std::string(root) + "/layers";
    CHECK(mkdir(out.c_str(), 0700) == 0 && mkdir(lay.c_str(), 0700) == 0);
    const std::vector<std::string> refs = {"chr1", "chr8", "chrX", "chr1"}; // a repeated name: the first id wins
    const char *chroms[] = {"chr1", "chr8", "chrX", "chr22", "chrom"};
    long amplicons = 0, files = 0, overlap_lines = 0;
    for (int round = 0; round < 200; ++round) {
        std::vector<BedRow> rows(rnd() % 40);
        for (auto &r : rows) {
            r.chrom = chroms[rnd() % 5];
            r.start = rnd() % 12 == 0 ? (int)(rnd() % 3) - 1 : 100 + (int)(rnd() % 400);
            r.end = rnd() % 10 == 0 ? r.start - (int)(rnd() % 3) : r.start + (int)(rnd() % 150);
            if (rnd() % 8 == 0 && &r != &rows[0]) r = rows[0];
            r.name = "amp" + std::to_string(&r - &rows[0]);
        }
        const AmpliconArrays a = amplicon_arrays(rows, refs);
        const size_t A = (size_t)a.A();
        amplicons += (long)A;
        CHECK(a.hi.size() == A && a.reach.size() == A && a.amp_off.size() == A + 1 && a.row_of.size() == A && a.sorted_of_row.size() == rows.size());
        size_t known = 0;
        for (size_t r = 0; r < rows.size(); ++r) {
            const bool in = rows[r].chrom != "chr22" && rows[r].chrom != "chrom" && rows[r].start >= 1 && rows[r].end >= rows[r].start;
            known += in;
            CHECK((a.sorted_of_row[r] >= 0) == in);
            if (in) CHECK(a.row_of[(size_t)a.sorted_of_row[r]] == (int32_t)r);
        }
        CHECK(known == A && a.amp_off[0] == 0);
        for (size_t i = 0; i < A; ++i) {
            CHECK(a.lo[i] <= a.hi[i] && (a.lo[i] >> 32) == (a.hi[i] >> 32) && (a.lo[i] >> 32) < 3);
            CHECK(a.amp_off[i + 1] - a.amp_off[i] == (int64_t)(a.hi[i] - a.lo[i]) + 1);
            CHECK(a.reach[i] >= a.hi[i] && (i == 0 || a.reach[i] >= a.reach[i - 1]));
            if (i) CHECK(a.lo[i - 1] < a.lo[i] || (a.lo[i - 1] == a.lo[i] && (a.hi[i - 1] < a.hi[i] || (a.hi[i - 1] == a.hi[i] && a.row_of[i - 1] < a.row_of[i]))));
        }
        // listed positions: around the amplicons, repeated, and on an unknown chromosome
        AmpliconCounts c;
        std::vector<AmpliconListed> listed(rnd() % 300);
        for (auto &v : listed) {
            v.chrom = chroms[rnd() % 4];
            v.pos = 90 + (int64_t)(rnd() % 600);
            v.id = ".";
            v.ref = "A";
            v.alt = ".";
            const int id = v.chrom == "chr1" ? 0 : v.chrom == "chr8" ? 1 : v.chrom == "chrX" ? 2 : -1;
            if (id >= 0) {
                v.slot = (int64_t)c.keys.size();
                c.keys.push_back(((uint64_t)id << 32) | (uint64_t)v.pos);
            }
        }
        const size_t n = c.keys.size(), W = (size_t)a.W();
        c.counts.resize(W * 8);
        for (auto &x : c.counts) x = (int32_t)(rnd() % 50);
        c.amp_reads.resize(A * 2);
        for (auto &x : c.amp_reads) x = (int64_t)(rnd() % 1000);
        c.stats[0] = 5000; c.stats[1] = 4000; c.stats[2] = 400000; c.stats[3] = 777;
        c.layers.assign(2 * n * 8, 0);
        c.layer_amp.assign(2 * n, -1);
        c.total.assign(n * 8, 0);
        long want_overlap = 0, want_amp2 = 0;
        for (size_t p = 0; p < n; ++p) { // the gather, on the host
            int64_t first, last;
            a.candidates(c.keys[p], first, last);
            CHECK(first >= 0 && last < (int64_t)A);
            int l = 0;
            for (int64_t i = first; i <= last; ++i) {
                if (a.hi[(size_t)i] < c.keys[p]) continue;
                CHECK(a.lo[(size_t)i] <= c.keys[p]);
                const int32_t *r = &c.counts[(size_t)(a.amp_off[(size_t)i] + (int64_t)(c.keys[p] - a.lo[(size_t)i])) * 8];
                for (int f = 0; f < 8; ++f) c.total[p * 8 + f] += r[f];
                if (l < 2) {
                    std::copy(r, r + 8, &c.layers[((size_t)l * n + p) * 8]);
                    c.layer_amp[(size_t)l * n + p] = (int32_t)i;
                }
                ++l;
            }
            for (int k = l; k < 2; ++k) c.layers[((size_t)k * n + p) * 8] = AMPLI_ABSENT;
            if (l >= 2) { want_overlap += l; ++want_amp2; }
        }
        const bool with_layers = round % 2 == 0;
        const int64_t written = write_amplicon_files(out, with_layers ? lay : "", "S" + std::to_string(round), rows, a, listed, c, 0);
        const std::string base = out + "/S" + std::to_string(round);
        CHECK(written == (int64_t)listed.size() && lines_of(base + ".AMPLICON.PILEUP.ASEQ") == 1 + (long)listed.size());
        CHECK(lines_of(base + ".AMPLICON.READS.txt") == (long)rows.size() + 5 && lines_of(base + ".AMPLICON.OVERLAPS.txt") == want_overlap);
        if (with_layers) CHECK(lines_of(lay + "/S" + std::to_string(round) + ".AMP2.PILEUP.ASEQ") == 1 + want_amp2 && lines_of(lay + "/S" + std::to_string(round) + ".pairs.txt") == 1);
        overlap_lines += want_overlap;
        files += with_layers ? 6 : 3;
        CHECK(write_amplicon_files(out, "", "S" + std::to_string(round), rows, a, listed, c, 1 << 30) == 0); // over the files of the first call: the header alone
        CHECK(lines_of(base + ".AMPLICON.PILEUP.ASEQ") == 1);
        // a layers directory that does not exist: refused, and nothing new is left in out
        const int before = entries(out);
        bool threw = false;
        try {
            write_amplicon_files(out, std::string(root) + "/missing", "T", rows, a, listed, c, 0);
        } catch (const Error &) {
            threw = true;
        }
        CHECK(threw && entries(out) == before);
    }
    // W >= 2^31 is refused by the builder
    {
        std::vector<BedRow> rows(2);
        rows[0].chrom = rows[1].chrom = "chr1";
        rows[0].start = rows[1].start = 1;
        rows[0].end = rows[1].end = 0x7fffffff / 2 + 1;
        bool threw = false;
        try {
            amplicon_arrays(rows, refs);
        } catch (const Error &e) {
            threw = e.code == AMPLI_E_RANGE;
        }
        CHECK(threw);
        CHECK(amplicon_arrays({}, refs).A() == 0 && amplicon_arrays(rows, {}).A() == 0 && amplicon_arrays(rows, {}).sorted_of_row.size() == 2);
    }
    CHECK(system(("rm -r " + std::string(root)).c_str()) == 0);
    printf("amplicon_count_sanitize: %ld amplicons, %ld files, %ld overlap lines: clean\n", amplicons, files, overlap_lines);
    return 0;
}
