// tests/csrc/scorer_domain_main.cpp -- a stand-alone host program (tests/test_scorer_domain_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the table-backed forms of the scorers of csrc/ampli_math.h against their no-table
// forms, over the index arithmetic's whole domain.  A heap table of exactly AMPLI_LGTAB entries, filled by ampli_kf_lgamma as the
// device fills its own, so that an index outside 0 .. AMPLI_LGTAB - 1 is a heap overflow the sanitizer sees; the no-table form
// (NULL, 0) calls the function.  Both must return the same bits at every point.  Exit status: 0 = equal everywhere.
#include <cinttypes>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../amplisolve_amd/csrc/ampli_math.h"

namespace {

const double *g_tab = nullptr;
long g_points = 0, g_bad = 0;

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

void report(const char *what, int32_t k, int32_t rd, float err, double with_table, double without)
{
    if (++g_bad <= 20) fprintf(stderr, "%s differs: k=%" PRId32 " rd=%" PRId32 " err=%.9g: table %.17g, function %.17g\n", what, k, rd, (double)err, with_table, without);
}

// ampli_drain_p (where the drain would ask: any mean; the arithmetic is total) and ampli_poisson_score_dense at one point
void check(int32_t k, int32_t rd, float err)
{
    ++g_points;
    const double m = (double)rd * err; // VC:3864
    const double a = ampli_drain_p(k, m, g_tab, AMPLI_LGTAB), b = ampli_drain_p(k, m, nullptr, 0);
    if (!same_bits(a, b)) report("ampli_drain_p", k, rd, err, a, b);
    const double c = ampli_poisson_score_dense(k, rd, err, g_tab, AMPLI_LGTAB), d = ampli_poisson_score_dense(k, rd, err, nullptr, 0);
    if (!same_bits(c, d)) report("ampli_poisson_score_dense", k, rd, err, c, d);
}

} // namespace

int main()
{
    double *tab = (double *)malloc(sizeof(double) * AMPLI_LGTAB);
    if (!tab) return 2;
    for (int i = 0; i < AMPLI_LGTAB; ++i) tab[i] = ampli_kf_lgamma((double)i);
    g_tab = tab;

    // every table index and the first ones beyond it: n = 0 .. AMPLI_LGTAB + 2 as the count, against means on both sides of it
    // (series: lgamma(n + 1); continued fraction and its closed form: lgamma(n)) and against the special errors
    for (int32_t n = 0; n <= AMPLI_LGTAB + 2; ++n) {
        const int32_t below = n > 600 ? 4 * (n - 536) : (n > 1 ? 2 * n : 1); // m = n - 536 (0.25) or n / 2
        check(n, below, 0.25f);
        check(n, 4 * n + 400, 0.25f); // m = n + 100: the fraction's side
        check(n, 1000 * n + 1500, 0.002f);
        check(n, n, 0.0f);
        check(n, n, -1.0f);
        if (!same_bits(ampli_lgamma_int(n, tab, AMPLI_LGTAB), ampli_kf_lgamma((double)n))) report("ampli_lgamma_int", n, 0, 0, 0, 0);
    }
    // the table's end at a threshold of 0.25, both sides of the mean (tests/scorer_grids.py, table_end_points)
    {
        const int32_t dm[] = {-536, -300, -100, 100, 536};
        for (int32_t k = 65534; k <= 65538; ++k)
            for (int32_t d : dm) check(k, 4 * (k + d), 0.25f);
    }
    // counts and depths at and beyond 2^24 up to INT32_MAX against six errors (edge_points)
    {
        const int32_t big[] = {(1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 30, INT32_MAX - 1, INT32_MAX};
        const float errs[] = {1e-5f, 0.002f, 0.0f, 0.25f, 0.9f, -1.0f};
        for (int32_t k : big)
            for (int32_t rd : big)
                for (float e : errs) check(k, rd, e);
        // and counts next to the mean of those depths, where p is neither 0 nor 1
        for (int32_t rd : big)
            for (float e : errs) {
                if (e < 0) continue;
                const double m = (double)rd * (e == 0 ? 0.0010008f : e), dks[] = {-1, 0, 1, 3, floor(3 * sqrt(m))};
                for (double dk : dks) check((int32_t)fmin(floor(m) + dk, (double)INT32_MAX), rd, e);
            }
    }
    // both sides of the closed form's bound z < 838860.8 with k = 1 .. 5
    {
        const struct { float err; int32_t rd_lo; } hb[] = {{0.25f, 3355443}, {0.5f, 1677721}, {0.05f, 16777215}};
        for (const auto &h : hb)
            for (int32_t rd = h.rd_lo - 1; rd <= h.rd_lo + 2; ++rd)
                for (int32_t k = 1; k <= 5; ++k) check(k, rd, h.err);
    }
    // k = 0, rd = 0, negative counts, negative depths, negative errors
    {
        const float errs[] = {0.002f, 0.0f, 0.25f, -1.0f, -0.002f, -0.25f, -1e-5f};
        const int32_t rds[] = {0, 1, 500, 100000, 1 << 24, INT32_MAX, -1, -500, -(1 << 24), INT32_MIN};
        const int32_t ks[] = {0, 1, 2, 5, 77, 300, 65536, 65537, 1 << 24, INT32_MAX, -1, -2, -77, -65537, -(1 << 24), INT32_MIN + 1, INT32_MIN};
        for (int32_t k : ks)
            for (int32_t rd : rds)
                for (float e : errs) check(k, rd, e);
    }
    // the detection limit's walk reads the same table through ampli_drain_p: the largest strands
    {
        int32_t ev_a = 0, ev_b = 0;
        const int32_t depths[] = {1000, 70000, 1 << 24, INT32_MAX};
        for (int32_t d : depths) {
            const int32_t a = ampli_limit_reads(d, 0.25f, d, tab, AMPLI_LGTAB, &ev_a), b = ampli_limit_reads(d, 0.25f, d, nullptr, 0, &ev_b);
            ++g_points;
            if (a != b || ev_a != ev_b) report("ampli_limit_reads", d, d, 0.25f, (double)a, (double)b);
        }
    }
    free(tab);
    printf("%ld points, %ld differences\n", g_points, g_bad);
    return g_bad ? 1 : 0;
}
