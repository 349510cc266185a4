// tools/fraction_sanitize.cpp -- the host library's tumour-fraction exports under AddressSanitizer + UBSan: a stand-alone
// program over the host library's sources, run once on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/fraction_sanitize \
//       tools/fraction_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/fraction_sanitize
// Random panels with every edge of the definition -- absent records, int32 fields of 2^30 and 2^31 - 1, thresholds of -1, 0, NaN and
// infinity, weights of NaN, infinity, 0, negative and above 1, reference codes above 3, entries at and beyond P, offsets that run
// backwards and beyond W, padded strides, L = 0 -- in heap buffers of exactly the size the contract names, so that a read or a write past
// either end is a report.  Every value is checked against its range and the order F_LO <= F_HAT <= F_HI, a second call against the
// first (the same bytes), the verdict and the change against their codes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/amplisolve_hip.h"
#include "../include/amplisolve_host.h"

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

int main()
{
    const int32_t counts[] = {0, 1, 2, 50, 99, 100, 101, 400, 65534, 1 << 24, 1 << 30, INT32_MAX};
    const float thrs[] = {1e-3f, 2e-4f, 5e-3f, 0.0f, -1.0f, NAN, INFINITY, -0.5f, 1.0f};
    const float weights[] = {0.5f, 0.2f, 1.0f, 0.05f, NAN, INFINITY, 0.0f, -0.0f, -0.3f, 1.5f, 1e-30f};
    const double z2s[] = {AMPLI_TF_Z2_90, AMPLI_TF_Z2_95, AMPLI_TF_Z2_99};
    long cells = 0, evaluated = 0, na = 0, quantified = 0;
    for (int round = 0; round < 60; ++round) {
        const int64_t P = 1 + (int64_t)(rnd() % 90);
        const int32_t n = 1 + (int32_t)(rnd() % 5), L = (int32_t)(rnd() % 8);
        const int64_t stride = P + (int64_t)(rnd() % 3);
        std::vector<int32_t> recs((size_t)n * stride * 8);
        for (size_t r = 0; r < recs.size() / 8; ++r) {
            if (rnd() % 2) { // plasma-like: a deep reference base and a few alternative reads
                for (int f = 0; f < 8; ++f) recs[r * 8 + f] = (int32_t)(rnd() % 4 ? rnd() % 6 : 0);
                recs[r * 8 + rnd() % 4] = 2500 + (int32_t)(rnd() % 1000);
                recs[r * 8 + 4 + rnd() % 4] = 2500 + (int32_t)(rnd() % 1000);
            } else
                for (int f = 0; f < 8; ++f) recs[r * 8 + f] = counts[rnd() % (rnd() % 4 ? 9 : 12)];
            if (rnd() % 9 == 0) recs[r * 8] = INT32_MIN;
        }
        std::vector<float> thr((size_t)8 * P);
        for (float &e : thr) e = thrs[rnd() % (rnd() % 3 ? 3 : 9)];
        std::vector<uint8_t> ref((size_t)P);
        for (uint8_t &g : ref) g = rnd() % 12 ? (uint8_t)(rnd() % 4) : (uint8_t)(rnd() % 2 ? 4 : 255);
        // lists: mostly monotone offsets, sometimes running backwards or beyond W
        const int64_t W = (int64_t)(rnd() % 400);
        std::vector<uint32_t> off((size_t)L + 1), cell((size_t)(W ? W : 1));
        std::vector<float> w(cell.size());
        for (uint32_t &c : cell) c = rnd() % 6 ? (uint32_t)(rnd() % (4 * P)) : (uint32_t)(4 * (P + rnd() % 5) + rnd() % 4);
        for (float &x : w) x = weights[rnd() % (rnd() % 3 ? 4 : 11)];
        if (rnd() % 8 == 0) cell[0] = 0xFFFFFFFFu;
        off[0] = 0;
        for (int32_t l = 1; l <= L; ++l) off[l] = (uint32_t)((int64_t)W * l / L);
        if (rnd() % 4 == 0) off[(size_t)(rnd() % (L + 1))] = (uint32_t)(W + rnd() % 50);
        if (rnd() % 4 == 0) off[(size_t)(rnd() % (L + 1))] = 0;
        const ampli_fraction_params prm = {(int32_t)(rnd() % 3 ? 100 : rnd() % 2 ? 0 : 30000), (int32_t)(rnd() % 2 ? 1000 : rnd() % 1001), z2s[rnd() % 3]};

        std::vector<double> est((size_t)n * L * AMPLI_TF_VALS, -7.0), est2(est);
        std::vector<int64_t> count((size_t)n * L * AMPLI_TF_COUNTS, -7), count2(count);
        // exactly-sized outputs; with L == 0 they are empty and a valid pointer is still required
        double none_e = 0.0;
        int64_t none_c = 0;
        double *pe = est.empty() ? &none_e : est.data(), *pe2 = est2.empty() ? &none_e : est2.data();
        int64_t *pc = count.empty() ? &none_c : count.data(), *pc2 = count2.empty() ? &none_c : count2.data();
        CHECK(ampli_host_fraction(recs.data(), n, stride, P, thr.data(), ref.data(), off.data(), cell.data(), w.data(), L, W, &prm, pe, pc) == 0);
        CHECK(ampli_host_fraction(recs.data(), n, stride, P, thr.data(), ref.data(), off.data(), cell.data(), w.data(), L, W, &prm, pe2, pc2) == 0);
        CHECK(est.empty() || memcmp(est.data(), est2.data(), est.size() * sizeof(double)) == 0);
        CHECK(count == count2);
        for (size_t i = 0; i < (size_t)n * L; ++i) {
            ++cells;
            const double *v = &est[i * AMPLI_TF_VALS];
            const int64_t ne = count[i * 2], ns = count[i * 2 + 1];
            CHECK(ne >= ns && ns >= 0);
            evaluated += ne;
            if (ne == 0) CHECK(v[AMPLI_TF_F_HAT] == AMPLI_TF_NA);
            if (v[AMPLI_TF_F_HAT] == AMPLI_TF_NA) {
                CHECK(v[AMPLI_TF_F_LO] == AMPLI_TF_NA && v[AMPLI_TF_F_HI] == AMPLI_TF_NA && v[AMPLI_TF_T0] == AMPLI_TF_NA);
                ++na;
            } else {
                CHECK(v[AMPLI_TF_F_LO] >= 0.0 && v[AMPLI_TF_F_LO] <= v[AMPLI_TF_F_HAT] && v[AMPLI_TF_F_HAT] <= v[AMPLI_TF_F_HI] && v[AMPLI_TF_F_HI] <= 1.0);
                CHECK(!std::isnan(v[AMPLI_TF_T0]));
                CHECK((v[AMPLI_TF_F_LO] > 0.0) == (v[AMPLI_TF_T0] > prm.z2));
            }
            const int verdict = ampli_host_fraction_verdict(ne, v[AMPLI_TF_F_HAT], v[AMPLI_TF_F_LO], 3);
            CHECK(verdict >= AMPLI_TF_NOT_EVALUABLE && verdict <= AMPLI_TF_QUANTIFIED);
            quantified += verdict == AMPLI_TF_QUANTIFIED;
            if (i > 0) {
                const double *u = &est[(i - 1) * AMPLI_TF_VALS];
                const int before = ampli_host_fraction_verdict(count[(i - 1) * 2], u[AMPLI_TF_F_HAT], u[AMPLI_TF_F_LO], 3);
                double ratio = -7.0;
                const int ch = ampli_host_fraction_change(before, u, verdict, v, &ratio);
                CHECK(ch >= AMPLI_TF_CHANGE_NOT_EVALUABLE && ch <= AMPLI_TF_FALLING);
                CHECK(ratio == AMPLI_TF_NA || ratio >= 0.0);
            }
        }
    }
    // refusals write nothing
    {
        const int32_t rec[8] = {3000, 9, 0, 0, 2900, 8, 0, 0};
        const float thr[8] = {1e-3f, 1e-3f, 1e-3f, 1e-3f, 1e-3f, 1e-3f, 1e-3f, 1e-3f}, w[1] = {0.4f};
        const uint8_t ref[1] = {0};
        const uint32_t off[2] = {0, 1}, cell[1] = {1};
        double est[4] = {-7, -7, -7, -7};
        int64_t count[2] = {-7, -7};
        ampli_fraction_params bad = {100, 1000, 0.0};
        CHECK(ampli_host_fraction(rec, 1, 0, 1, thr, ref, off, cell, w, 1, 1, &bad, est, count) == -1 && est[0] == -7 && count[0] == -7);
        bad.z2 = NAN;
        CHECK(ampli_host_fraction(rec, 1, 0, 1, thr, ref, off, cell, w, 1, 1, &bad, est, count) == -1 && est[0] == -7);
        bad.z2 = AMPLI_TF_Z2_95;
        CHECK(ampli_host_fraction(rec, 1, 0, 1, thr, ref, off, cell, w, -1, 1, &bad, est, count) == -1 && est[0] == -7);
        CHECK(ampli_host_fraction(rec, 1, 0, 1, thr, ref, off, cell, w, 1, 1ll << 28, &bad, est, count) == -6 && est[0] == -7);
        CHECK(ampli_host_fraction(rec, 1, 0, 1, thr, ref, off, cell, w, 1, 1, &bad, est, count) == 0 && count[0] == 1 && count[1] == 1);
        CHECK(est[AMPLI_TF_F_HAT] > 0.0 && est[AMPLI_TF_F_HAT] < 0.01 && est[AMPLI_TF_F_HI] > est[AMPLI_TF_F_HAT]);
    }
    printf("fraction_sanitize: %ld cells, %ld evaluated entries, %ld cells NA, %ld quantified: clean\n", cells, evaluated, na, quantified);
    return 0;
}
