// tools/dilution_sanitize.cpp -- ampli_host_dilute_records under AddressSanitizer + UBSan: a stand-alone program over the
// host library's sources, run once on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/dilution_sanitize \
//       tools/dilution_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/dilution_sanitize
// Random records with every edge of the definition -- absent records, counts on the block and lane-stride edges, 2^24 - 2, 2^24 - 1, a
// negative count, thresholds 0, 1, 2^32 - 1, 2^32 and beyond, rows outside their chunk, no chunk b, padded strides -- in heap buffers of
// exactly the size the contract names, so that a read or a write past either end is a report.  Every output is checked against Thin
// called cell by cell.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/amplisolve_hip.h"
#include "../include/amplisolve_host.h"

static uint64_t rng_state = 0x0123456789ABCDEFull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int main()
{
    const int32_t edges[] = {0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 2000, 65534, AMPLI_DILUTE_MAX_COUNT, AMPLI_DILUTE_MAX_COUNT + 1, -1, INT32_MAX};
    const uint64_t keeps[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, UINT64_MAX, 0x80000000ull, 429496730ull};
    long checked = 0, absent = 0, bad_count = 0, bad_mix = 0;
    for (int round = 0; round < 40; ++round) {
        const int64_t P = 1 + (int64_t)(rnd() % 70);
        const int32_t n_a = 1 + (int32_t)(rnd() % 4), n_b = (int32_t)(rnd() % 4), n_mix = 1 + (int32_t)(rnd() % 12);
        const int64_t sa = P + (int64_t)(rnd() % 3), sb = P + (int64_t)(rnd() % 3);
        std::vector<int32_t> A((size_t)n_a * sa * 8), B((size_t)n_b * sb * 8);
        for (std::vector<int32_t> *v : {&A, &B})
            for (size_t r = 0; r < v->size() / 8; ++r) {
                int32_t *rec = v->data() + r * 8;
                const bool deep = rnd() % 400 == 0; // a few long cells only: the program draws every read
                for (int f = 0; f < 8; ++f) {
                    int32_t e = edges[rnd() % (sizeof edges / sizeof *edges)];
                    if (e == AMPLI_DILUTE_MAX_COUNT && !deep) e = (int32_t)(rnd() % 3000);
                    rec[f] = rnd() % 3 ? (int32_t)(rnd() % 3000) : e;
                }
                if (rnd() % 8 == 0) rec[0] = AMPLI_ABSENT;
            }
        std::vector<ampli_dilute_mix> mix((size_t)n_mix);
        for (ampli_dilute_mix &m : mix) {
            m.row_a = rnd() % 10 ? (int32_t)(rnd() % (uint64_t)n_a) : (int32_t)(rnd() % 7) - 3 + (rnd() % 2 ? n_a : 0);
            m.row_b = rnd() % 3 == 0 ? -1 : (rnd() % 10 && n_b ? (int32_t)(rnd() % (uint64_t)n_b) : (int32_t)(rnd() % 9) - 4 + n_b);
            m.keep_a = rnd() % 2 ? keeps[rnd() % 8] : rnd() >> 32;
            m.keep_b = rnd() % 2 ? keeps[rnd() % 8] : rnd() >> 32;
            m.key = rnd();
        }
        std::vector<int32_t> out((size_t)n_mix * P * 8, 0x5A5A5A5A), flags((size_t)n_mix, 0x5A5A5A5A);
        const int rc = ampli_host_dilute_records(A.data(), n_a, sa, n_b ? B.data() : nullptr, n_b, sb, P, mix.data(), n_mix, out.data(), flags.data());
        if (rc != 0) { printf("round %d: rc %d\n", round, rc); return 1; }
        for (int32_t m = 0; m < n_mix; ++m) {
            const ampli_dilute_mix &x = mix[(size_t)m];
            const bool ok = x.row_a >= 0 && x.row_a < n_a && x.keep_a <= 0x100000000ull && x.keep_b <= 0x100000000ull && x.row_b >= -1 && (x.row_b == -1 || x.row_b < n_b);
            int flag = ok ? 0 : AMPLI_DILUTE_BAD_MIXTURE;
            bad_mix += !ok;
            for (int64_t p = 0; p < P; ++p) {
                const int32_t *o = out.data() + ((size_t)m * P + p) * 8;
                bool present = ok;
                const int32_t *a = nullptr, *b = nullptr;
                if (ok) {
                    bool bad = false;
                    a = A.data() + ((size_t)x.row_a * sa + p) * 8;
                    if (x.row_b >= 0) b = B.data() + ((size_t)x.row_b * sb + p) * 8;
                    for (const int32_t *r : {a, b}) {
                        if (!r) continue;
                        if (r[0] == AMPLI_ABSENT) { present = false; continue; }
                        for (int f = 0; f < 8; ++f) bad = bad || r[f] < 0 || r[f] > AMPLI_DILUTE_MAX_COUNT;
                    }
                    if (bad) { flag |= AMPLI_DILUTE_BAD_COUNT; present = false; ++bad_count; }
                }
                absent += !present;
                for (int f = 0; f < 8; ++f) {
                    int64_t want = f == 0 ? (int64_t)AMPLI_ABSENT : 0;
                    if (present) want = ampli_host_thin(a[f], x.keep_a, x.key, (uint32_t)p, f, 0) + (b ? ampli_host_thin(b[f], x.keep_b, x.key, (uint32_t)p, f, 1) : 0);
                    if (o[f] != want) { printf("round %d mixture %d position %lld field %d: %d, expected %lld\n", round, m, (long long)p, f, o[f], (long long)want); return 1; }
                    ++checked;
                }
            }
            if (flags[(size_t)m] != flag) { printf("round %d mixture %d: flags %d, expected %d\n", round, m, flags[(size_t)m], flag); return 1; }
        }
    }
    // the refusals write nothing
    int32_t rec[8] = {1, 2, 3, 4, 5, 6, 7, 8}, o[8] = {0}, fl = 0;
    ampli_dilute_mix one = {0, -1, 5, 5, 1};
    if (ampli_host_dilute_records(nullptr, 1, 0, nullptr, 0, 0, 1, &one, 1, o, &fl) != -1 || ampli_host_dilute_records(rec, 1, 0, nullptr, 1, 0, 1, &one, 1, o, &fl) != -1 ||
        ampli_host_dilute_records(rec, 1, 0, nullptr, 0, 0, 0, &one, 1, o, &fl) != -1 || ampli_host_dilute_records(rec, 1, 0, nullptr, 0, 0, 1, &one, 0, o, &fl) != -1) {
        printf("a refusal did not refuse\n");
        return 1;
    }
    printf("clean: %ld output words checked, %ld absent records, %ld records with a bad count, %ld bad mixtures\n", checked, absent, bad_count, bad_mix);
    return 0;
}
