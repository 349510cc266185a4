// tools/monitor_sanitize.cpp -- the host library's monitoring exports under AddressSanitizer + UBSan: a stand-alone program
// over the host library's sources, run once on the CPU, not part of the suite.  From the repository's root:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -o /tmp/monitor_sanitize \
//       tools/monitor_sanitize.cpp $(ls amplisolve_amd/csrc/host/*.cpp | grep -v _main.cpp) -ldl -lz && /tmp/monitor_sanitize
// Random panels with every edge of the definition -- absent records, int32 fields of 2^30 and 2^31 - 1, thresholds of -1, 0, NaN and
// infinity, reference codes above 3, entries at and beyond P, offsets that run backwards and beyond W, empty candidate classes, drawn
// positions beyond P, pair indices out of range, padded strides -- in heap buffers of exactly the size the contract names, so that a
// read or a write past either end is a report.  The controls of a whole call are checked against the same call cut in two batches, the
// sums against the sums of the list read backwards (the integers agree whatever the order), the scores against their range.
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
    long cells = 0, evaluated = 0, na = 0;
    for (int round = 0; round < 60; ++round) {
        const int64_t P = 1 + (int64_t)(rnd() % 90);
        const int32_t n = 1 + (int32_t)(rnd() % 5), L = 1 + (int32_t)(rnd() % 7);
        const int64_t stride = P + (int64_t)(rnd() % 3);
        std::vector<int32_t> recs((size_t)n * stride * 8);
        for (size_t r = 0; r < recs.size() / 8; ++r) {
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
        for (uint32_t &c : cell) c = rnd() % 6 ? (uint32_t)(rnd() % (4 * P)) : (uint32_t)(4 * (P + rnd() % 5) + rnd() % 4);
        if (rnd() % 8 == 0) cell[0] = 0xFFFFFFFFu;
        off[0] = 0;
        for (int32_t l = 1; l <= L; ++l) off[l] = (uint32_t)((int64_t)W * l / L);
        if (rnd() % 4 == 0) off[(size_t)(rnd() % (L + 1))] = (uint32_t)(W + rnd() % 50);
        if (rnd() % 4 == 0) off[(size_t)(rnd() % (L + 1))] = 0;
        const ampli_monitor_params prm = {(int32_t)(rnd() % 3 ? 100 : rnd() % 2 ? 0 : 30000), (int32_t)(rnd() % 2 ? 1000 : rnd() % 1001)};

        std::vector<int64_t> sums((size_t)n * L * AMPLI_MON_SUMS, -1);
        std::vector<double> lam((size_t)n * L * 2, -1.0);
        CHECK(ampli_host_monitor_sums(recs.data(), n, stride, P, thr.data(), ref.data(), off.data(), cell.data(), L, W, &prm, sums.data(), lam.data()) == 0);
        // the same lists read backwards: the integers do not depend on the order of the entries
        std::vector<uint32_t> rev_off((size_t)L + 1), rev_cell;
        rev_off[0] = 0;
        for (int32_t l = 0; l < L; ++l) {
            const uint32_t w = (uint32_t)W, a = off[l] < w ? off[l] : w, b_ = off[l + 1] < w ? off[l + 1] : w, b = b_ < a ? a : b_;
            for (uint32_t e = b; e > a; --e) rev_cell.push_back(cell[e - 1]);
            rev_off[l + 1] = (uint32_t)rev_cell.size();
        }
        const int64_t rev_W = (int64_t)rev_cell.size();
        if (rev_cell.empty()) rev_cell.push_back(0);
        std::vector<int64_t> sums2(sums.size(), -1);
        std::vector<double> lam2(lam.size(), -1.0);
        CHECK(ampli_host_monitor_sums(recs.data(), n, stride, P, thr.data(), ref.data(), rev_off.data(), rev_cell.data(), L, rev_W, &prm, sums2.data(),
                                      lam2.data()) == 0);
        CHECK(sums == sums2);
        for (size_t i = 0; i < lam.size(); ++i) CHECK(lam[i] >= 0.0 && std::fabs(lam[i] - lam2[i]) <= 1e-12 * lam[i]);
        std::vector<float> q((size_t)n * L * 2, -7.0f);
        CHECK(ampli_host_monitor_score(sums.data(), lam.data(), (int64_t)n * L, q.data()) == 0);
        for (size_t i = 0; i < (size_t)n * L; ++i) {
            ++cells;
            evaluated += sums[i * 6];
            CHECK(sums[i * 6] >= sums[i * 6 + 1] && sums[i * 6 + 1] >= 0);
            for (int st = 0; st < 2; ++st) {
                const float v = q[2 * i + st];
                if (sums[i * 6] == 0) { CHECK(v == AMPLI_MON_NA); ++na; }
                else CHECK(v == AMPLI_MON_NA || (v >= 0.0f && v <= 100.0f));
                (void)ampli_host_monitor_excess(sums[i * 6 + 2 + st], lam[2 * i + st], sums[i * 6 + 4 + st]);
            }
            (void)ampli_host_monitor_verdict(sums[i * 6], sums[i * 6 + 1], q[2 * i], q[2 * i + 1], 3, 1, 20.0);
        }

        // controls: candidates grouped by base, sometimes a class emptied, sometimes positions beyond P among them
        std::vector<uint32_t> cand_off(5, 0), cand_pos;
        for (uint32_t g = 0; g < 4; ++g) {
            if (rnd() % 5)
                for (int64_t p = 0; p < P; ++p)
                    if (ref[(size_t)p] == g) cand_pos.push_back(rnd() % 40 ? (uint32_t)p : (uint32_t)(P + rnd() % 3));
            cand_off[g + 1] = (uint32_t)cand_pos.size();
        }
        const int64_t n_cand = (int64_t)cand_pos.size();
        if (rnd() % 6 == 0) cand_off[4] += 7; // beyond n_cand: cut
        if (cand_pos.empty()) cand_pos.push_back(0);
        const int32_t n_pairs = 1 + (int32_t)(rnd() % 5), R = 2 + (int32_t)(rnd() % 6), first = (int32_t)(rnd() % 1000);
        std::vector<int32_t> pairs((size_t)n_pairs * 2);
        for (int32_t k = 0; k < n_pairs; ++k) {
            pairs[2 * k] = rnd() % 6 ? (int32_t)(rnd() % n) : (rnd() % 2 ? n : -1);
            pairs[2 * k + 1] = rnd() % 6 ? (int32_t)(rnd() % L) : (rnd() % 2 ? L : -1);
        }
        const uint64_t seed = rnd();
        std::vector<int64_t> cs((size_t)n_pairs * R * AMPLI_MON_SUMS, -1);
        std::vector<double> cl((size_t)n_pairs * R * 2, -1.0);
        CHECK(ampli_host_monitor_controls(recs.data(), n, stride, P, thr.data(), ref.data(), off.data(), cell.data(), L, W, pairs.data(), n_pairs, cand_off.data(),
                                          cand_pos.data(), n_cand, R, first, seed, &prm, cs.data(), cl.data()) == 0);
        const int32_t R1 = 1 + (int32_t)(rnd() % (R - 1));
        for (int part = 0; part < 2; ++part) { // two batches equal one call
            const int32_t r0 = part ? R1 : 0, rn = part ? R - R1 : R1;
            std::vector<int64_t> ps((size_t)n_pairs * rn * AMPLI_MON_SUMS, -1);
            std::vector<double> pl((size_t)n_pairs * rn * 2, -1.0);
            CHECK(ampli_host_monitor_controls(recs.data(), n, stride, P, thr.data(), ref.data(), off.data(), cell.data(), L, W, pairs.data(), n_pairs,
                                              cand_off.data(), cand_pos.data(), n_cand, rn, first + r0, seed, &prm, ps.data(), pl.data()) == 0);
            for (int32_t k = 0; k < n_pairs; ++k)
                for (int32_t r = 0; r < rn; ++r) {
                    CHECK(memcmp(&ps[((size_t)k * rn + r) * 6], &cs[((size_t)k * R + r0 + r) * 6], 6 * sizeof(int64_t)) == 0);
                    CHECK(memcmp(&pl[((size_t)k * rn + r) * 2], &cl[((size_t)k * R + r0 + r) * 2], 2 * sizeof(double)) == 0);
                }
        }
        std::vector<float> cq((size_t)n_pairs * R * 2);
        CHECK(ampli_host_monitor_score(cs.data(), cl.data(), (int64_t)n_pairs * R, cq.data()) == 0);
        for (int32_t k = 0; k < n_pairs; ++k) {
            const int64_t n_ge = ampli_host_monitor_count_ge(q[0], q[1], cq.data() + (size_t)k * R * 2, R);
            CHECK(n_ge >= 0 && n_ge <= R);
            const double pe = ampli_host_monitor_empirical_p(n_ge, R);
            CHECK(pe > 0.0 && pe <= 1.0);
        }
    }
    int32_t evals = 0;
    CHECK(ampli_host_monitor_lod_reads(10.0, 20.0, &evals) == 19 && evals == 9);
    CHECK(ampli_host_monitor_lod_reads(1e6, 100.0, &evals) == 0 && evals == AMPLI_MON_LOD_MAX_EVALS);
    CHECK(ampli_host_monitor_lod(10.0, 2.5, 1000, 500, 20.0) > 0.0 && ampli_host_monitor_lod(10.0, 2.5, 0, 500, 20.0) == -1.0);
    for (uint32_t m : {1u, 2u, 3u, 1000u, 0xFFFFFFFFu})
        for (int i = 0; i < 1000; ++i) CHECK(ampli_host_monitor_control_draw((uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd(), rnd(), m) < m);
    printf("monitor_sanitize: %ld cells, %ld evaluated entries, %ld scores NA: clean\n", cells, evaluated, na);
    return 0;
}
