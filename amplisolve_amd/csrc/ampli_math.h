// amplisolve_amd/csrc/ampli_math.h
//
// Scalar arithmetic of the hot path, shared by the HIP kernels (device) and by
// the C++ host (formatting / CPU-side unit checks of the same code).  Each
// function names the reference lines whose result it must reproduce:
//   EE:n = source_codes/AmpliSolveErrorEstimation.cpp:n, VC:n = source_codes/AmpliSolveVariantCalling.cpp:n
#ifndef AMPLI_MATH_H
#define AMPLI_MATH_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/amplisolve_types.h"

#if defined(__HIPCC__)
#define AMPLI_FN __host__ __device__ __forceinline__
#else
#define AMPLI_FN static inline
#endif

// ---------------------------------------------------------------------------
// AF gate.  The reference computes af = float(x)/float(d), widens it to double
// and tests af <= 0.05 (EE:1229,1251 and EE:1592-1595).  0.05 (double) lies
// strictly between the adjacent floats f0 = 13421772*2^-28 and f1 = f0 + 2^-28,
// so the test is RN(x/d) <= f0.  With round-to-nearest-even and f0's even
// significand that is x/d <= (f0+f1)/2 = 26843545 * 2^-29, i.e. for exactly
// representable x, d (< 2^24):   x <= floor(d * 26843545 / 2^29).
// One 64-bit multiply per (record, strand) instead of one IEEE division per
// (record, strand, nucleotide).  d == 0 gives limit 0; callers AND the gate
// with d >= coverage_cutoff >= 1 as the reference does, which also removes
// the 0/0 = NaN case.
// ---------------------------------------------------------------------------
#define AMPLI_AF_MID_NUM 26843545ull
#define AMPLI_AF_MID_SHIFT 29
#define AMPLI_COUNT_LIMIT (1 << 24)

// floor(d * 26843545 / 2^29) = floor(d * (26843545 * 8) / 2^32): the high half of ONE 32 x 32-bit multiply (v_mul_hi_u32)
// instead of a 64-bit multiply-add and a 64-bit shift; 26843545 * 8 < 2^32, so the identity holds for every uint32 d.
#define AMPLI_AF_MID_NUM8 214748360u
AMPLI_FN int32_t ampli_af_limit(int32_t d)
{
    return (int32_t)(((uint64_t)(uint32_t)d * AMPLI_AF_MID_NUM8) >> 32);
}

// The same integer as one fp32 multiply and a truncation, for 0 <= d < 2^24 (d exact in fp32): 0x1.999998p-5 is the float just
// below 0.05, and the rounding error of the product never carries it across an integer that the exact quotient d * 26843545 / 2^29
// has not crossed (tests/test_math_host.py compares every d).  Full rate on the GPU where v_mul_hi_u32 takes four passes; the
// float of d is needed by the callers anyway.  Negative d (an absent record's sentinel sum) gives a value <= 0: callers mask it.
AMPLI_FN int32_t ampli_af_limit_f32(float d_as_float)
{
    return (int32_t)(d_as_float * 0x1.999998p-5f);
}

// literal form, for operands outside the exact-float range and for tests
AMPLI_FN int ampli_af_gate_fp(int32_t x, int32_t d)
{
    double af = (double)((float)x / (float)d);
    return af <= 0.05;
}

// ---------------------------------------------------------------------------
// stof(sprintf("%f", r)): the rate as AmpliSolveVariantCalling reads it back
// from the error table (EE:1704 -> VC:887-890), in exact integer arithmetic.
//   "%f" prints round-half-even(r * 10^6) / 10^6 (glibc rounds the exact binary
//   value); r = m * 2^e with m < 2^24, so m * 10^6 < 2^44 fits an int64.
//   For r >= 16 the float spacing (>= 2^-19) exceeds 2 * 5e-7, so the nearest
//   float to the printed decimal is r itself.  Below 16, N < 2^24 and 10^6 are
//   both exact floats and the correctly rounded fp32 quotient N / 10^6 is the
//   float nearest to the printed decimal, which is what strtof returns.
// ---------------------------------------------------------------------------
AMPLI_FN float ampli_text_roundtrip(float r)
{
    uint32_t bits;
    memcpy(&bits, &r, 4);
    const uint32_t sign = bits & 0x80000000u;
    const uint32_t ex = (bits >> 23) & 0xFF;
    uint32_t man = bits & 0x7FFFFFu;
    if (ex == 0xFF) return r; // inf / nan: not produced by the reference's finalize (NaN is caught before)
    float a = fabsf(r);
    if (a >= 16.0f) return r;
    int e2;
    if (ex == 0) {
        e2 = -149;
    } else {
        man |= 0x800000u;
        e2 = (int)ex - 150;
    }
    // a = man * 2^e2, e2 <= -20 here
    const uint64_t A = (uint64_t)man * 1000000ull;
    const int k = -e2;
    uint64_t N;
    if (k >= 45) {
        N = 0; // A < 2^44 <= 2^(k-1): rounds to 0
    } else {
        const uint64_t q = A >> k, rem = A & ((1ull << k) - 1), half = 1ull << (k - 1);
        N = q + ((rem > half) || (rem == half && (q & 1)));
    }
    float out = (float)(uint32_t)N / 1000000.0f;
    uint32_t ob;
    memcpy(&ob, &out, 4);
    ob |= sign; // "-0.000000" parses to -0.0f
    memcpy(&out, &ob, 4);
    return out;
}

// ---------------------------------------------------------------------------
// Poisson scorer: kf_lgamma / _kf_gammap / _kf_gammaq / kf_gammaq as adopted by
// the reference from samtools kfunc.c (VC:3721-3830), including the 99-step
// caps, KF_GAMMA_EPS 1e-14 and KF_TINY 1e-290 (VC:149-150).
// ---------------------------------------------------------------------------
AMPLI_FN double ampli_kf_lgamma(double z)
{
    double x = 0;
    x += 0.1659470187408462e-06 / (z + 7);
    x += 0.9934937113930748e-05 / (z + 6);
    x -= 0.1385710331296526 / (z + 5);
    x += 12.50734324009056 / (z + 4);
    x -= 176.6150291498386 / (z + 3);
    x += 771.3234287757674 / (z + 2);
    x -= 1259.139216722289 / (z + 1);
    x += 676.5203681218835 / z;
    x += 0.9999999999995183;
    return log(x) - 5.58106146679532777 - z + (z - 0.5) * log(z + 6.5);
}

AMPLI_FN double ampli_kf_gammap_series(double s, double z)
{
    double sum = 1., x = 1.;
    for (int k = 1; k < 100; ++k) {
        x *= z / (s + k);
        sum += x;
        if (x / sum < 1e-14) break;
    }
    return exp(s * log(z) - z - ampli_kf_lgamma(s + 1.) + log(sum));
}

AMPLI_FN double ampli_kf_gammaq_cf(double s, double z)
{
    double f = 1. + z - s, C = f, D = 0.;
    for (int j = 1; j < 100; ++j) {
        const double a = j * (s - j), b = (j << 1) + 1 + z - s;
        D = b + a * D;
        if (D < 1e-290) D = 1e-290;
        C = b + a / C;
        if (C < 1e-290) C = 1e-290;
        D = 1. / D;
        const double d = C * D;
        f *= d;
        if (fabs(d - 1.) < 1e-14) break;
    }
    return exp(s * log(z) - z - ampli_kf_lgamma(s) - log(f));
}

// The same series without its 99 divisions, for the dense drain of the prefilter queue (z < s there):
//   sum_{n=0}^{99} z^n / ((s+1)...(s+n)) = A_99 / D_99,   A_n = A_{n-1} (s+n) + z^n,   D_n = D_{n-1} (s+n),
// one fused multiply-add per term on the critical path instead of an IEEE division (~10 dependent operations), every
// term positive (no cancellation), A / D in [1, 100]; A, D and z^n are rescaled by an exact power of two every 16 terms
// ((s+n)^16 < 2^500 for every int32 count).  Differences from ampli_kf_gammap_series: (i) rounding, ~1e-14 relative;
// (ii) the reference stops at the first term with x/sum < 1e-14 -- the terms it leaves out add < ~1e-13 of the sum
// (this form stops, between runs of 16 terms, only once a term is below 2^-60 of the sum).
// Both are eight orders of magnitude inside the 1e-6 tolerance on p.  What is NOT optional is the cap at n = 99:
// for z close to s the series has not converged by then and the truncation is part of the reference's result.
AMPLI_FN double ampli_kf_gammap_series_nodiv(double s, double z)
{
    double A = 1., D = 1., zp = 1., t = s;
    // terms 1..99 as six runs of 16 and one of 3; the rescale sits BETWEEN the runs so that a run is four
    // operations per term and nothing else
    for (int blk = 0; blk < 7; ++blk) {
        const int len = blk < 6 ? 16 : 3;
        for (int i = 0; i < len; ++i) {
            t += 1.;
            zp *= z;
            A = fma(A, t, zp);
            D *= t;
        }
        // z < s: every further term is smaller than the last one (zp / D), so once that is below 2^-60 of the sum the
        // at most 83 terms still to come cannot change the double any more
        if (zp < A * 8.673617379884035e-19) break;
        int e;
        (void)frexp(D, &e);
        A = ldexp(A, -e); D = ldexp(D, -e); zp = ldexp(zp, -e);
    }
    return exp(s * log(z) - z - ampli_kf_lgamma(s + 1.) + log(A / D)); // VC:3793
}

AMPLI_FN double ampli_kf_gammaq(double s, double z)
{
    return (z <= 1. || z < s) ? 1. - ampli_kf_gammap_series(s, z) : ampli_kf_gammaq_cf(s, z);
}

// p as formed at VC:3858-3865 (before the clamp); err already != -1
AMPLI_FN double ampli_poisson_p(int32_t k, int32_t rd, float err)
{
    if (err == 0) err = 0.0010008f; // VC:3852-3856 (double literal narrowed to float)
    if (k == 0) return 1.0;         // VC:3858-3861
    const double m = (double)rd * err; // VC:3864: double * float
    return 1 - ampli_kf_gammaq((double)k, m);
}

// Q = -10 log10 p with the reference's clamps (VC:3844-3880).  The reference
// takes the final log10 in long double; fp64 differs by < 1e-14 relative.
AMPLI_FN double ampli_q_from_p(double p)
{
    if (p < 0.0000000001) return 100.0; // -10*log10l(1e-10), (double) of which is 100
    if (p == 1) return 0.0;
    return -10 * log10(p);
}

AMPLI_FN double ampli_poisson_score(int32_t k, int32_t rd, float err)
{
    if (err == -1) return -888.0; // VC:3844-3849
    return ampli_q_from_p(ampli_poisson_p(k, rd, err));
}

// ---------------------------------------------------------------------------
// The all-scores mode's scorer (round 4): the same Q as ampli_poisson_score, to rounding, for what that mode feeds it --
// s = k is always an INTEGER count -- at about a third of the instructions:
//   * kf_lgamma(s), kf_lgamma(s + 1) come from a table of the Lanczos form's own values at the integers (lgtab[n] =
//     ampli_kf_lgamma(n), filled by the same function on the same device, so bit-identical to calling it; NULL or an index
//     beyond ntab: the function itself): 8 divisions + 2 logarithms less per score;
//   * the series branch is the division-free form of the drain kernel (ampli_kf_gammap_series_nodiv);
//   * the continued fraction (VC:3733-3752) is evaluated through its convergents, f_j = A_j / B_j with
//       A_j = b_j A_{j-1} + a_j A_{j-2},  B_j = b_j B_{j-1} + a_j B_{j-2},  a_j = j (s - j),  b_j = 2j + 1 + z - s
//     (modified Lentz keeps C_j = A_j / A_{j-1} and D_j = B_{j-1} / B_j and pays two divisions per step; the product of the
//     C_j D_j it accumulates IS A_j / B_j).  The reference leaves the loop once |C_j D_j - 1| < 1e-14 or after 99 steps, and
//     for an integer s at j = s at the latest (a_s = 0 makes the step the identity); all three exits are kept.  In this
//     branch z > s >= 1, so every a_j up to the exit and every b_j is positive and the KF_TINY guards never fire;
//   * log(sum) / log(f) are not taken: the prefactor exp(s log z - z - lgamma) is multiplied / divided instead.
// Differences from the literal scorer: rounding (~1e-13 relative on p, measured in tests/test_math_host.py); the contract
// is 1e-6, and a Q within 1e-6 of a gate is re-decided by the host in the reference's own arithmetic either way.
// That the table gives the function's bits is asserted on the host: tests/csrc/scorer_domain_main.cpp (under the address and
// undefined-behaviour sanitizers) and tests/test_math_host.py run the table and the no-table form of every scorer below over the
// int32 domain and compare bits.  The index arithmetic is free of overflow: the index is compared as an unsigned number, so a
// negative one takes the function, and k + 1 is never formed as an int -- ampli_lgamma_int_next takes k and adds inside
// ((double)k + 1. is exact for every int32 k; at INT32_MAX the int sum wrapped to INT32_MIN and passed the signed guard it had).
// ---------------------------------------------------------------------------
#define AMPLI_LGTAB 65537 // entries of the table (why this many: ampli_internal.h)
AMPLI_FN double ampli_lgamma_int(int n, const double *lgtab, int ntab)
{
    return (lgtab && (unsigned)n < (unsigned)ntab) ? lgtab[n] : ampli_kf_lgamma((double)n);
}

// kf_lgamma(k + 1) for an int32 k
AMPLI_FN double ampli_lgamma_int_next(int k, const double *lgtab, int ntab)
{
    return (lgtab && ntab > 0 && (unsigned)k < (unsigned)(ntab - 1)) ? lgtab[k + 1] : ampli_kf_lgamma((double)k + 1.);
}

// P(s, z) by the series, z <= s (the branch kf_gammaq takes for z <= 1 or z < s), prefactor given
AMPLI_FN double ampli_gammap_series_int(double s, double z, double prefactor /* exp(s log z - z - lgamma(s + 1)) */)
{
    double A = 1., D = 1., zp = 1., t = s;
    for (int blk = 0; blk < 7; ++blk) {
        const int len = blk < 6 ? 16 : 3;
        for (int i = 0; i < len; ++i) {
            t += 1.;
            zp *= z;
            A = fma(A, t, zp);
            D *= t;
        }
        if (zp < A * 8.673617379884035e-19) break; // see ampli_kf_gammap_series_nodiv
        int e;
        (void)frexp(D, &e);
        A = ldexp(A, -e); D = ldexp(D, -e); zp = ldexp(zp, -e);
    }
    return prefactor * (A / D);
}

// Q(s, z) by the continued fraction for an integer s = k, z > s, prefactor given
AMPLI_FN double ampli_gammaq_cf_int(int k, double z, double prefactor /* exp(s log z - z - lgamma(s)) */)
{
    const double s = (double)k;
    double A1 = 1. + z - s, A2 = 1., B1 = 1., B2 = 0.; // f_0 = b_0; A_{-1} = 1, B_{-1} = 0, B_0 = 1
    const int J = k - 1 < 99 ? k - 1 : 99;             // j = s is the identity step; the reference's cap is j < 100
    for (int j = 1; j <= J; ++j) {
        const double a = (double)j * (s - j), b = (double)((j << 1) + 1) + z - s;
        const double A0 = fma(b, A1, a * A2), B0 = fma(b, B1, a * B2);
        const double num = A0 * B1, den = A1 * B0; // C_j D_j = num / den, both positive
        A2 = A1; A1 = A0; B2 = B1; B1 = B0;
        if (fabs(num - den) < 1e-14 * den) break;
        if ((j & 7) == 0) { // a, b < 2^33: eight steps stay far inside the double range
            int e;
            (void)frexp(A1, &e);
            A1 = ldexp(A1, -e); A2 = ldexp(A2, -e); B1 = ldexp(B1, -e); B2 = ldexp(B2, -e);
        }
    }
    return prefactor * B1 / A1; // exp(...) / f, f = A_j / B_j  (VC:3751)
}

// Q(k, z) for an integer k in 1 .. AMPLI_HORNER_K on the continued fraction's side (z > k), round 5.  For an integer s the
// fraction of VC:3733-3752 ends at j = s (a_s = 0: the step is the identity) and its value there is a rational function,
//   f = z^k / H_k(z),   H_k(z) = sum_{i<k} z^i (k-1)! / i!   (H_1 = 1, H_{j+1} = j H_j + z^j),
// so exp(s log z - z - lgamma(s)) / f  =  exp(-z - lgamma(k)) H_k(z): the Poisson sum e^-z sum_{i<k} z^i / i! with the
// reference's own lgamma (the table of its Lanczos values).  One exp and k - 1 FMAs -- no log z, no division, no convergence
// test; the reference's early exit (|C_j D_j - 1| < 1e-14) leaves out steps that change f by < 1e-14 each.  Within 1e-13
// relative of the literal scorer (tests/test_math_host.py).  K = 4 covers 96 % of the scores on that side of a ctDNA-like panel
// (config 3: all-scores mode 0.55 ms; K = 16: 0.58 ms -- a wave runs the longest loop of its lanes; H_16 would still be far
// from overflow for z < 2^24 x 0.05, the bound kept below).
#define AMPLI_HORNER_K 4
AMPLI_FN double ampli_gammaq_horner_int(int k, double z, double lgk /* lgamma(k) */)
{
    double H = 1., zp = 1.;
    for (int j = 1; j < k; ++j) {
        zp *= z;
        H = fma((double)j, H, zp);
    }
    return exp(-z - lgk) * H;
}

// p of a count k > 0 against an effective error (neither -1 nor 0): VC:3864-3865 through the forms above
AMPLI_FN double ampli_poisson_p_dense(int32_t k, int32_t rd, float err, const double *lgtab, int ntab)
{
    if (k < 0) return 1 - ampli_kf_gammaq((double)k, (double)rd * err); // not a count: the literal path
    const double s = (double)k, z = (double)rd * err; // VC:3864: double * float
    if (z <= 1. || z < s) { // VC:3728
        if (!(z > 0)) return 1 - ampli_kf_gammaq(s, z); // z <= 0 or NaN: whatever the literal arithmetic gives
        const double P = ampli_gammap_series_int(s, z, exp(s * log(z) - z - ampli_lgamma_int_next(k, lgtab, ntab)));
        return 1 - (1. - P); // VC:3865 on top of VC:3728
    }
    if (k <= AMPLI_HORNER_K && z < 838860.8) return 1 - ampli_gammaq_horner_int(k, z, ampli_lgamma_int(k, lgtab, ntab));
    return 1 - ampli_gammaq_cf_int(k, z, exp(s * log(z) - z - ampli_lgamma_int(k, lgtab, ntab)));
}

// The drain kernel's scorer since round 6: p of a queued item -- an integer count k against a mean 0 < m < k, i.e. always the
// series branch of kf_gammaq (VC:3728) -- in the all-scores mode's form: kf_lgamma(k + 1) from the table of its own values, the
// prefactor multiplied by the series' sum instead of adding its logarithm.  A wave of the drain is bound by the length of ONE
// instruction stream (a pass is ~1500 dependent fp64 instructions at ~8 cycles): this form has a third fewer.
AMPLI_FN double ampli_drain_p(int32_t k, double m, const double *lgtab, int ntab)
{
    const double s = (double)k;
    const double P = ampli_gammap_series_int(s, m, exp(s * log(m) - m - ampli_lgamma_int_next(k, lgtab, ntab)));
    return 1 - (1. - P); // VC:3865 on top of VC:3728
}

AMPLI_FN double ampli_poisson_score_dense(int32_t k, int32_t rd, float err, const double *lgtab, int ntab)
{
    if (err == -1) return -888.0;   // VC:3844-3849
    if (err == 0) err = 0.0010008f; // VC:3852-3856
    if (k == 0) return 0.0;         // VC:3858-3861: p = 1 -> Q = 0 (VC:3873-3876)
    return ampli_q_from_p(ampli_poisson_p_dense(k, rd, err, lgtab, ntab));
}

// Exact-decision bound used by AMPLI_POISSON_PREFILTER: when k <= m the
// reference's own scorer returns Q < 5 (P(X >= k) > 0.31 for k <= mean; checked
// exhaustively against the scorer incl. its iteration caps in
// tests/test_math_host.py), so VC:898 is false whatever the other strand says.
// err == -1 gives Q = -888 < 5 as well.
AMPLI_FN int ampli_prefilter_nocall(int32_t k, int32_t rd, float err)
{
    if (err == -1) return 1;
    if (err == 0) err = 0.0010008f;
    if (k == 0) return 1;
    const double m = (double)rd * err;
    return (double)k <= m;
}

// Conservative fp32 form of the bound above, used by the streaming kernel: with err_eff = ampli_effective_err(err)
// and c = float(rd) * 0.999999f,   float(k) <= c * err_eff   implies   k <= rd * err   (k, rd < 2^24 are exact
// floats; two roundings of at most 2^-24 each cannot undo the factor 1 - 1e-6), so every record it skips would be
// skipped by ampli_prefilter_nocall too.  What it does not skip is scored exactly; nothing is decided in fp32.
AMPLI_FN float ampli_effective_err(float err)
{
    if (err == 0.0f) return 0.0010008f; // VC:3852-3856
    if (err == -1.0f) return INFINITY;  // VC:3844-3849: Q = -888
    return err;
}

AMPLI_FN int ampli_prefilter_skip_f32(int32_t k, int32_t rd, float err_eff)
{
    if ((uint32_t)rd >= (uint32_t)AMPLI_COUNT_LIMIT || (uint32_t)k >= (uint32_t)AMPLI_COUNT_LIMIT) return 0;
    const float c = (float)rd * 0.999999f;
    return (float)k <= c * err_eff;
}

// ---------------------------------------------------------------------------
// Detection limit of the calling gate: the smallest count k in 1 .. bound of one strand with Q(k, depth, thr) >= 5
// (VC:898 with VC:3834-3884), found without scanning from k = 1:
//   * nothing passes at k <= m = depth * thr (ampli_prefilter_nocall's bound), so the walk starts at floor(m) + 1 or, for larger
//     means up to AMPLI_LIMIT_SEED_MAX_M, at floor(m + 0.4 sqrt(m + 1)) -- the first passing count was never seen below
//     m + 0.45 sqrt(m + 1) there (tests/test_limit_host.py re-asserts both on random strands).  For much larger means the 99-term
//     cap of the series (VC:3783) cuts p short and the first passing count comes back to floor(m) + 1: no seed there;
//   * every candidate lies above m, i.e. on the series branch of kf_gammaq (VC:3728): ampli_drain_p evaluates it;
//   * the answer k is only given with its bracket: Q(k) >= 5 and (k == 1 or k - 1 <= m or Q(k - 1) < 5), every Q decided outside
//     the band of AMPLI_LIMIT_BAND around the gate.  A seed that turns out to pass walks DOWN until the bracket closes.
// Whatever this arithmetic cannot decide -- a Q inside the band, a mean that is not a positive finite number, a walk longer than
// AMPLI_LIMIT_MAX_EVALS -- is AMPLI_LIMK_RECHECK: the host settles it with the literal scan (ampli_host_limit_reads).
// One ampli_limit_step is ONE scorer evaluation, so that a kernel can run the steps of several strands in a single loop.
// ---------------------------------------------------------------------------
#define AMPLI_LIMIT_BAND AMPLI_CALL_GATE_EPS // one band for the search and for the call list
#define AMPLI_LIMIT_MAX_EVALS 128       // the longest walk seen on 200 000 random strands is 26 evaluations from floor(m) + 1
#define AMPLI_LIMK_PENDING (-3)        // the search goes on
#define AMPLI_LIMK_RECHECK (-2)        // not decided here
#define AMPLI_LIMK_NOESTIMATE (-1)     // thr == -1: Q = -888 for every count (VC:3844-3849)
#define AMPLI_LIMK_UNREACHABLE 0       // no count in 1 .. bound passes
#define AMPLI_LIMIT_SEED 0.4
#define AMPLI_LIMIT_SEED_MAX_M 1024.0   // beyond: the series is cut at 99 terms long before it converges and the first passing count falls back towards m

typedef struct {
    double m;      // depth * thr (VC:3864)
    int32_t k;     // the candidate
    int32_t bound; // the strand's reads: no more than these can be alternative
    int32_t below; // k - 1 is known not to pass (k == 1, k - 1 <= m, or evaluated)
    int32_t down;  // k has passed: the evaluation in hand is the bracket check of k - 1
    int32_t evals;
    int32_t res;   // AMPLI_LIMIT_* or the smallest passing count
} ampli_limit_search;

AMPLI_FN void ampli_limit_init(ampli_limit_search *s, int32_t depth, float thr, int32_t bound)
{
    s->m = 0; s->k = 0; s->bound = bound; s->below = 1; s->down = 0; s->evals = 0; s->res = AMPLI_LIMK_PENDING;
    if (thr == -1) { s->res = AMPLI_LIMK_NOESTIMATE; return; }
    if (thr == 0) thr = 0.0010008f;                                      // VC:3852-3856
    if (depth <= 0 || bound < 1) { s->res = AMPLI_LIMK_UNREACHABLE; return; }
    const double m = (double)depth * thr;                                // VC:3864: double * float
    if (!(m > 0 && m < 2147483000.0)) { s->res = AMPLI_LIMK_RECHECK; return; } // negative, NaN, infinite or beyond an int count
    s->m = m;
    const int32_t k0 = (int32_t)floor(m) + 1;
    if (k0 > bound) { s->res = AMPLI_LIMK_UNREACHABLE; return; }        // every k <= bound is <= m
    int32_t k = m <= AMPLI_LIMIT_SEED_MAX_M ? (int32_t)floor(m + AMPLI_LIMIT_SEED * sqrt(m + 1.)) : k0;
    if (k < k0) k = k0;
    if (k > bound) k = bound;
    s->k = k;
    s->below = k == k0;                                                  // k - 1 = floor(m) <= m (k0 == 1: k == 1)
}

AMPLI_FN void ampli_limit_step(ampli_limit_search *s, const double *lgtab, int ntab)
{
    const int32_t kk = s->down ? s->k - 1 : s->k;                        // m < kk always
    const double q = ampli_q_from_p(ampli_drain_p(kk, s->m, lgtab, ntab));
    ++s->evals;
    if (!(q < 5.0 - AMPLI_LIMIT_BAND) && !(q >= 5.0 + AMPLI_LIMIT_BAND)) { s->res = AMPLI_LIMK_RECHECK; return; } // in the band, or NaN
    const int pass = q >= 5.0;
    if (s->down) {
        if (!pass) { s->res = s->k; return; }
        --s->k;                                                          // the seed was above the limit: one down
        if ((double)(s->k - 1) <= s->m) { s->res = s->k; return; }       // also k == 1
    } else if (pass) {
        if (s->below) { s->res = s->k; return; }
        s->down = 1;
    } else {
        s->below = 1;
        if (s->k >= s->bound) { s->res = AMPLI_LIMK_UNREACHABLE; return; }
        ++s->k;
    }
    if (s->evals >= AMPLI_LIMIT_MAX_EVALS) s->res = AMPLI_LIMK_RECHECK;
}

// the whole search of one strand (host, tests, and lanes that own a single strand)
AMPLI_FN int32_t ampli_limit_reads(int32_t depth, float thr, int32_t bound, const double *lgtab, int ntab, int32_t *evals)
{
    ampli_limit_search s;
    ampli_limit_init(&s, depth, thr, bound);
    while (s.res == AMPLI_LIMK_PENDING) ampli_limit_step(&s, lgtab, ntab);
    if (evals) *evals = s.evals;
    return s.res;
}

// ---------------------------------------------------------------------------
// Detection power: the probability that a variant at allele fraction v gives at least k alternative reads among the n
// reads of a strand, tail(n, k, v) = P[Bin(n, v) >= k], in fp64 for n up to 2^31, and the allele fraction at which both strands
// together reach a confidence c.
//   * One term of the pmf is formed in closed form -- the saddle-point form, whose large parts cancel analytically:
//       ln pmf(j) = 1/2 ln(n / (2 pi j (n - j))) + d(n) - d(j) - d(n - j) - D(j),   D(j) = n KL(j/n || v),
//     d(x) = ln x! - ((x + 1/2) ln x - x + 1/2 ln 2 pi), the error of Stirling's formula.  (lgamma differences are useless here: at
//     2^30 one lgamma carries an absolute error of 4e-6, whichever function computes it.)
//   * D(j) is also Chernoff's exponent: P[X >= k] <= exp(-D(k)) for k >= n v and P[X <= k - 1] <= exp(-D(k - 1)) for k - 1 <= n v.
//     Beyond AMPLI_TAIL_CUT = 20 the tail is within e^-20 = 2.1e-9 of 0 or of 1 and is returned as that: no sum.
//   * Otherwise the pmf is summed AWAY from the mean with the term recurrence, from k upwards when k > n v, else from k - 1 downwards
//     (the complement).  The ratio of consecutive terms is below one from the first step and falls from step to step, so what is left
//     after a term t with next ratio r is below t r / (1 - r): the sum ends once that is below AMPLI_TAIL_EPS.  That happens within
//     about 6.7 standard deviations of the mean; with the cut above no sum starts farther than 6.4 from it on the other side, but sums
//     never cross the mean, so a tail costs at most AMPLI_TAIL_TERMS(n v (1 - v)) terms (asserted in tests/test_power_host.py).
// One ampli_tail_step is a short run of terms, so that a kernel can run the tails of a lane in a single loop (as ampli_limit_step).
// ---------------------------------------------------------------------------
#define AMPLI_TAIL_CUT 20.0
#define AMPLI_TAIL_EPS 1e-11
#define AMPLI_TAIL_RUN 8                 // terms per ampli_tail_step
#define AMPLI_TAIL_MAX_TERMS (1 << 19)   // never reached for n < 2^31 (8 sqrt(2^31 / 4) + 64 = 185 000): the loop's own bound
#define AMPLI_TAIL_TERMS(var) (8.0 * sqrt(var) + 64.0)

// d(x) for an integer x >= 1: the asymptotic series from 16 on (next term 1 / (1188 x^9) < 2e-14), below it from x! itself
AMPLI_FN double ampli_stirling_err(double x)
{
    if (x >= 16.0) {
        const double r = 1.0 / (x * x);
        return (1.0 / 12 - (1.0 / 360 - (1.0 / 1260 - 1.0 / 1680 * r) * r) * r) / x;
    }
    double f = 1.0;
    for (double i = 2.0; i <= x; i += 1.0) f *= i; // 15! < 2^53: exact
    return log(f) - ((x + 0.5) * log(x) - x + 0.918938533204672742);
}

// x ln(x / m) + m - x >= 0 for x >= 0, m > 0: m ((1 + t) log1p(t) - t) with t = (x - m) / m; the rounding error is ~1e-16 |x - m|
AMPLI_FN double ampli_bd0(double x, double m)
{
    if (x <= 0.0) return m;
    const double t = (x - m) / m;
    return m * ((1.0 + t) * log1p(t) - t);
}

// ln pmf(j) of Bin(n, v) for 0 <= j <= n, 0 < v < 1; *dev = D(j)
AMPLI_FN double ampli_binom_logpmf(double n, double j, double v, double *dev)
{
    if (j <= 0.0) { const double d = -n * log1p(-v); *dev = d; return -d; }
    if (j >= n) { const double d = -n * log(v); *dev = d; return -d; }
    const double D = ampli_bd0(j, n * v) + ampli_bd0(n - j, n * (1.0 - v));
    *dev = D;
    return 0.5 * log(n / (6.283185307179586477 * j * (n - j))) + ampli_stirling_err(n) - ampli_stirling_err(j) - ampli_stirling_err(n - j) - D;
}

typedef struct {
    double n, j;     // reads; index of the latest term
    double t, sum;   // the latest term; the terms so far
    double odds;     // v / (1 - v) going up, its inverse going down
    double pmf_k;    // pmf(k): d tail / d ln v = k pmf(k)
    double res;      // the tail, once live == 0
    int32_t up;      // the sum is the tail (from k upwards) / its complement (from k - 1 downwards)
    int32_t terms;   // pmf terms formed, the first one included
    int32_t live;
} ampli_tail_sum;

AMPLI_FN void ampli_tail_init(ampli_tail_sum *s, int32_t n_reads, int32_t k, double v)
{
    s->terms = 0; s->live = 0; s->pmf_k = 0; s->up = 1; s->n = (double)n_reads; s->j = 0; s->t = 0; s->sum = 0; s->odds = 0;
    if (k > n_reads || !(v > 0.0)) { s->res = 0.0; return; }
    if (k <= 0 || v >= 1.0) { s->res = 1.0; return; }
    const double n = (double)n_reads, kk = (double)k, o = v / (1.0 - v);
    double D;
    s->terms = 1;
    if (kk > n * v) {
        const double p = exp(ampli_binom_logpmf(n, kk, v, &D));
        s->pmf_k = p;
        if (D > AMPLI_TAIL_CUT) { s->res = 0.0; return; }
        s->j = kk; s->t = s->sum = p; s->odds = o; s->up = 1;
    } else {
        const double p = exp(ampli_binom_logpmf(n, kk - 1.0, v, &D));
        s->pmf_k = p * ((n - kk + 1.0) / kk) * o;
        if (D > AMPLI_TAIL_CUT) { s->res = 1.0; return; }
        s->j = kk - 1.0; s->t = s->sum = p; s->odds = 1.0 / o; s->up = 0;
    }
    s->live = 1;
}

AMPLI_FN void ampli_tail_step(ampli_tail_sum *s)
{
    double j = s->j, t = s->t, sum = s->sum;
    const double n = s->n, o = s->odds;
    int live = 1, terms = s->terms;
    for (int i = 0; i < AMPLI_TAIL_RUN; ++i) {
        // the ratio to the next term away from the mean; 0 at the end of the support
        const double r = s->up ? (n - j) / (j + 1.0) * o : j / (n - j + 1.0) * o;
        if (!(t * r >= AMPLI_TAIL_EPS * (1.0 - r)) || terms >= AMPLI_TAIL_MAX_TERMS) { live = 0; break; }
        t *= r;
        sum += t;
        j += s->up ? 1.0 : -1.0;
        ++terms;
    }
    s->j = j; s->t = t; s->sum = sum; s->terms = terms; s->live = live;
    if (!live) s->res = s->up ? (sum < 1.0 ? sum : 1.0) : (sum < 1.0 ? 1.0 - sum : 0.0);
}

// tail(n, k, v); *terms (optional) = pmf terms formed, *pmf_k (optional) = pmf(k)
AMPLI_FN double ampli_binom_tail(int32_t n, int32_t k, double v, int32_t *terms, double *pmf_k)
{
    ampli_tail_sum s;
    ampli_tail_init(&s, n, k, v);
    while (s.live) ampli_tail_step(&s);
    if (terms) *terms = s.terms;
    if (pmf_k) *pmf_k = s.pmf_k;
    return s.res;
}

// power(v) = tail(FW, k_fw, v) tail(BW, k_bw, v) and its derivative in ln v, one unit of work per ampli_power_advance: a tail's start
// (if it is due), one run of its terms and, when that run ends the tail, the change of strand.  A tail of up to AMPLI_TAIL_RUN + 1 terms
// is therefore ONE unit; a longer one takes one more unit per further run.  Returns 1 when pw / dpw are those of v.
typedef struct {
    ampli_tail_sum ts;
    double v, tail_fw, d_fw; // d_fw = k_fw pmf(k_fw)
    double pw, dpw;
    int32_t FW, BW, k_fw, k_bw;
    int32_t strand, start;
    uint32_t n_tails, n_terms, max_terms; // of every tail since ampli_power_begin
} ampli_power_eval;

AMPLI_FN void ampli_power_begin(ampli_power_eval *e, int32_t FW, int32_t k_fw, int32_t BW, int32_t k_bw)
{
    e->FW = FW; e->BW = BW; e->k_fw = k_fw; e->k_bw = k_bw;
    e->v = 0; e->tail_fw = 0; e->d_fw = 0; e->pw = 0; e->dpw = 0; e->strand = 0; e->start = 0;
    e->n_tails = e->n_terms = e->max_terms = 0;
    e->ts.live = 0;
}

AMPLI_FN void ampli_power_at(ampli_power_eval *e, double v)
{
    e->v = v; e->strand = 0; e->start = 1;
}

AMPLI_FN int ampli_power_advance(ampli_power_eval *e)
{
    if (e->start) {
        ampli_tail_init(&e->ts, e->strand ? e->BW : e->FW, e->strand ? e->k_bw : e->k_fw, e->v);
        e->start = 0;
    }
    if (e->ts.live) {
        ampli_tail_step(&e->ts);
        if (e->ts.live) return 0;
    }
    ++e->n_tails;
    e->n_terms += (uint32_t)e->ts.terms;
    if ((uint32_t)e->ts.terms > e->max_terms) e->max_terms = (uint32_t)e->ts.terms;
    if (e->strand == 0) {
        e->tail_fw = e->ts.res; e->d_fw = (double)e->k_fw * e->ts.pmf_k;
        e->strand = 1; e->start = 1;
        return 0;
    }
    e->pw = e->tail_fw * e->ts.res;
    e->dpw = e->d_fw * e->ts.res + e->tail_fw * ((double)e->k_bw * e->ts.pmf_k);
    return 1;
}

// LoD(c): the root of power(v) = c in x = ln v by Newton's step, kept inside a bracket [lo, hi] with power(e^lo) < c <= power(e^hi)
// and replaced by a bisection when it leaves the bracket or does not halve the step (rtsafe).  The bracket starts at [ln 1e-12, 0]:
// power(1) = 1, and power(1e-12) <= P[X >= 1] <= 2^31 1e-12 < 0.5.  The search ends once |power - c| <= AMPLI_LOD_FTOL -- with d power /
// d ln v >= 0.046 at the root for c <= 0.99 that is 2.2e-7 of ln v -- or once the bracket is narrower than AMPLI_LOD_XTOL, and after
// AMPLI_LOD_MAX_ITERS evaluations at the latest (35 bisections close the bracket; a Newton step in between at most doubles that).
#define AMPLI_LOD_FTOL 1e-8
#define AMPLI_LOD_XTOL 1e-9
#define AMPLI_LOD_MAX_ITERS 96

typedef struct {
    double lo, hi, x, dx, dx_old, c;
    int32_t iters, done;
} ampli_lod_search;

// returns the first allele fraction to evaluate: where the more demanding strand expects its minimum reads and a standard deviation more
AMPLI_FN double ampli_lod_begin(ampli_lod_search *s, int32_t FW, int32_t k_fw, int32_t BW, int32_t k_bw, double c)
{
    s->lo = -27.631021115928547; s->hi = 0.0; s->c = c; s->iters = 0; s->done = 0;
    const double a = ((double)k_fw + sqrt((double)k_fw)) / (double)FW, b = ((double)k_bw + sqrt((double)k_bw)) / (double)BW;
    double v = a > b ? a : b;
    if (!(v < 0.99)) v = 0.99;
    s->x = log(v);
    s->dx = s->dx_old = s->hi - s->lo;
    return v;
}

// power and its derivative at e^x are in: returns the next allele fraction, or sets done (the LoD is then e^x)
AMPLI_FN double ampli_lod_update(ampli_lod_search *s, double pw, double dpw)
{
    const double f = pw - s->c;
    ++s->iters;
    if (f < 0.0) s->lo = s->x; else s->hi = s->x;
    if (fabs(f) <= AMPLI_LOD_FTOL || s->iters >= AMPLI_LOD_MAX_ITERS) { s->done = 1; return exp(s->x); }
    if (s->hi - s->lo <= AMPLI_LOD_XTOL) { s->done = 1; s->x = 0.5 * (s->lo + s->hi); return exp(s->x); }
    double xn = s->x - f / dpw;
    if (!(dpw > 0.0) || !(xn > s->lo && xn < s->hi) || fabs(2.0 * f) > fabs(s->dx_old * dpw)) xn = 0.5 * (s->lo + s->hi);
    s->dx_old = s->dx;
    s->dx = xn - s->x;
    s->x = xn;
    return exp(xn);
}

// the whole of one pair (host, tests): power[l] at levels[l], *lod = LoD(c) when lod is not NULL; stats[3] (optional) += tails, terms, max
AMPLI_FN void ampli_power_lod(int32_t FW, int32_t k_fw, int32_t BW, int32_t k_bw, const float *levels, int32_t n_levels, double c,
                              double *power, double *lod, int32_t *iters, uint64_t *stats)
{
    ampli_power_eval e;
    ampli_power_begin(&e, FW, k_fw, BW, k_bw);
    for (int l = 0; l < n_levels; ++l) {
        ampli_power_at(&e, (double)levels[l]);
        while (!ampli_power_advance(&e)) {}
        power[l] = e.pw;
    }
    if (iters) *iters = 0;
    if (lod) {
        ampli_lod_search s;
        double v = ampli_lod_begin(&s, FW, k_fw, BW, k_bw, c);
        while (!s.done) {
            ampli_power_at(&e, v);
            while (!ampli_power_advance(&e)) {}
            v = ampli_lod_update(&s, e.pw, e.dpw);
        }
        *lod = v;
        if (iters) *iters = s.iters;
    }
    if (stats) { stats[0] += e.n_tails; stats[1] += e.n_terms; if (e.max_terms > stats[2]) stats[2] = e.max_terms; }
}

// ---------------------------------------------------------------------------
// Dispersion of the panel of normals.  One cell = (position, base, strand) with its n qualifying records (the records
// the threshold sums count), K = sum of their alternative counts, D = sum of their strand depths, X2 = Pearson's statistic of the
// counts against the pooled rate K / D, and rinv = sum of 1 / d_i.  Given K the counts are multinomial with cell probabilities
// d_i / D under the pooled rate; Haldane's exact moments of X2 are then mean n - 1 and variance
//   V = 2 (n - 1) + (D rinv - n^2 - 2 n + 2) / K   (>= n - 1 whenever K >= 2),
// which hold where the expected counts are far below 1 and the chi-square table does not.
//   z = (X2 - (n - 1)) / sqrt(V), phi = X2 / (n - 1).
// Returns the status: AMPLI_DISPERSION_FEW (n < 2 or K < 2: z = phi = 0), else AMPLI_DISPERSION_OK, with AMPLI_DISPERSION_HIGH
// where z >= z_cutoff.  The finalize kernel and ampli_host_dispersion_cell_batch both run this text.
// ---------------------------------------------------------------------------
AMPLI_FN uint8_t ampli_dispersion_cell(int32_t n, double K, double D, double x2, double rinv, double z_cutoff, double *z, float *phi)
{
    *z = 0.0;
    *phi = 0.0f;
    if (n < 2 || !(K >= 2.0)) return AMPLI_DISPERSION_FEW;
    const double nn = (double)n, nm1 = nn - 1.0;
    const double V = 2.0 * nm1 + (D * rinv - (nn * nn + 2.0 * nn - 2.0)) / K;
    const double zz = (x2 - nm1) / sqrt(V);
    *z = zz;
    *phi = (float)(x2 / nm1);
    return zz >= z_cutoff ? AMPLI_DISPERSION_HIGH : AMPLI_DISPERSION_OK;
}

// ---------------------------------------------------------------------------
// Sample identity: the genotype of one (sample, position) from its counts alone, as six plane bits, and the relation of
// a pair of samples from the pair's counts.  Only the PRIMARY record of a position enters (slot r < P): extra occurrences (ext,
// dup_off, ext_pos) and the own-RD planes (rd, rd_ext) are ignored.  No reference base, no error table.
//   n_b = fw[b] + bw[b], d = sum n_b; with the per-mille bounds of ampli_genotype_params base b is
//     ABSENT 1000 n_b <= absent_max_pm d | HET het_min_pm d <= 1000 n_b <= het_max_pm d | HOM 1000 n_b >= hom_min_pm d | else AMBIGUOUS
//   VALID: present, d >= min_depth, no AMBIGUOUS base, and one HOM with no HET or two HET with no HOM.
// Every product is formed in int64: an int32-layout record may hold counts near 2^31 (n_b < 2^33, d < 2^35, 1000 d < 2^45).
// Returns the bits AMPLI_GENO_V | _A | _C | _G | _T (the base is HET or HOM) | _H (the position is a het); 0 unless VALID.  Bit k is
// plane k of the device's uint64 planes[sample][6][W].  genotype_planes_kernel and ampli_host_genotype_classify_batch run this text.
// ---------------------------------------------------------------------------
// min_depth >= 1 and 0 <= absent_max_pm < het_min_pm <= het_max_pm < hom_min_pm <= 1000
AMPLI_FN int ampli_genotype_params_ok(const ampli_genotype_params *q)
{
    return q->min_depth >= 1 && q->absent_max_pm >= 0 && q->absent_max_pm < q->het_min_pm && q->het_min_pm <= q->het_max_pm &&
           q->het_max_pm < q->hom_min_pm && q->hom_min_pm <= 1000;
}
AMPLI_FN uint32_t ampli_genotype_classify(const int32_t fw[4], const int32_t bw[4], int present, const ampli_genotype_params *q)
{
    int64_t n[4], d = 0;
    for (int b = 0; b < 4; ++b) {
        n[b] = (int64_t)fw[b] + (int64_t)bw[b];
        d += n[b];
    }
    const int64_t lim_abs = (int64_t)q->absent_max_pm * d, lim_het_lo = (int64_t)q->het_min_pm * d, lim_het_hi = (int64_t)q->het_max_pm * d,
                  lim_hom = (int64_t)q->hom_min_pm * d;
    uint32_t bits = 0;
    int n_het = 0, n_hom = 0, n_amb = 0;
    for (int b = 0; b < 4; ++b) {
        const int64_t k = 1000 * n[b];
        const int absent = k <= lim_abs, het = k >= lim_het_lo && k <= lim_het_hi, hom = k >= lim_hom;
        n_het += het;
        n_hom += hom;
        n_amb += !(absent || het || hom);
        bits |= (het || hom) ? 2u << b : 0u;
    }
    const int valid = present && d >= (int64_t)q->min_depth && n_amb == 0 && ((n_hom == 1 && n_het == 0) || (n_het == 2 && n_hom == 0));
    return valid ? (bits | AMPLI_GENO_V | (n_het == 2 ? AMPLI_GENO_H : 0u)) : 0u;
}
// the relation of a pair from its het_either and het_match counts: positions where both samples are homozygous for the same base
// (nearly every panel position) never enter the deciding ratio
AMPLI_FN int ampli_concordance_relation(int32_t het_either, int32_t het_match, int32_t min_sites, double same_fraction)
{
    if (het_either < min_sites) return AMPLI_RELATION_UNDETERMINED;
    return (double)het_match >= same_fraction * (double)het_either ? AMPLI_RELATION_SAME : AMPLI_RELATION_DIFFERENT;
}

// ---------------------------------------------------------------------------
// Cross-sample contamination: the fraction of recipient a's reads that come from source b, from the nine int64 sums of
// the ordered pair (contamination_kernel, index order AMPLI_CONTAM_*).  At a position where a is validly homozygous for X and b
// carries a base Y that a does not, a fraction c of b's reads shows n[Y] = c d reads where b is homozygous and c d / 2 where b is
// heterozygous for Y; the sequencing error puts e d reads on each other base, e measured on the positions where b has a's genotype:
//   alt = s1 + s4, slots = s2 + s5, den = s2 + s5 / 2, e = s7 / (3 s8), fraction = max(0, (alt - e slots) / den), se = sqrt(alt) / den.
// In double, in exactly this order.  num is NOT fused: the host library and the kernels' unit are both built with -ffp-contract=off
// (build.py), so that alt - e * slots is a rounded product and a rounded difference on every compiler -- the numpy model
// (tests/contamination_model.py) computes it that way, and tests/test_contamination_host.py compares the two bit for bit.
// fraction and se are NaN where den == 0.  The status: UNDETERMINED while s0 + s3 < min_sites, else CONTAMINATED where
// fraction >= min_fraction (never for a NaN), else CLEAN.
// ---------------------------------------------------------------------------
AMPLI_FN int ampli_contamination_estimate(const int64_t s[AMPLI_CONTAM_SUMS], int64_t min_sites, double min_fraction, double *fraction, double *se,
                                          double *background)
{
    const double alt = (double)(s[AMPLI_CONTAM_ALT_HOM] + s[AMPLI_CONTAM_ALT_HET]);
    const double slots = (double)(s[AMPLI_CONTAM_DEPTH_HOM] + s[AMPLI_CONTAM_DEPTH_HET]);
    const double den = (double)s[AMPLI_CONTAM_DEPTH_HOM] + 0.5 * (double)s[AMPLI_CONTAM_DEPTH_HET];
    const double e = s[AMPLI_CONTAM_DEPTH_BG] > 0 ? (double)s[AMPLI_CONTAM_ALT_BG] / (3.0 * (double)s[AMPLI_CONTAM_DEPTH_BG]) : 0.0;
    const double prod = e * slots;
    const double num = alt - prod;
    const double q = num / den;
    const double f = den > 0 ? (q > 0.0 ? q : 0.0) : (double)NAN;
    if (fraction) *fraction = f;
    if (se) *se = den > 0 ? sqrt(alt) / den : (double)NAN;
    if (background) *background = e;
    if (s[AMPLI_CONTAM_SITES_HOM] + s[AMPLI_CONTAM_SITES_HET] < min_sites) return AMPLI_CONTAM_STATUS_UNDETERMINED;
    return f >= min_fraction ? AMPLI_CONTAM_STATUS_CONTAMINATED : AMPLI_CONTAM_STATUS_CLEAN;
}

// ---------------------------------------------------------------------------
// Amplicon coverage and copy ratio (the definition is tests/amplicon_model.py).  Every value is an IEEE double + - x / in the
// written order, unfused (-ffp-contract=off in both libraries), so that the kernels, the host library and the numpy model agree bit
// for bit.
//   share   x = (double)d / (double)T                       d = DEPTH_FW + DEPTH_BW of one (sample, amplicon), T its sample's total
//   median  of m values in ascending order v: m odd v[(m-1)/2], m even (v[m/2-1] + v[m/2]) * 0.5, m == 0 NaN -- ONE function
//           (ampli_amplicon_median_pick) applied to the two middle values, however they were selected: by a bitwise search on the bit
//           patterns in the kernels (non-negative values), by ampli_amplicon_median here (signed values, a plain selection; NaNs are
//           dropped first, and m counts what is left)
//   z       mad > 0 ? ((ratio - 1.0) * med) / (1.4826 * mad) : NaN
//   gene    GAIN if n >= min_amplicons, median ratio >= gain_ratio and median z >= z_cutoff; LOSS if n >= min_amplicons, median ratio
//           <= loss_ratio and median z <= -z_cutoff; else NEUTRAL (a NaN median compares false: NEUTRAL)
// ---------------------------------------------------------------------------
AMPLI_FN double ampli_amplicon_share(int64_t d, int64_t total) { return (double)d / (double)total; }

AMPLI_FN double ampli_amplicon_median_pick(double lo, double hi, int64_t m)
{
    if (m <= 0) return (double)NAN;
    return (m & 1) ? hi : (lo + hi) * 0.5;
}

// the k-th smallest (k from 0) of v[0 .. m), none of them NaN; v is reordered (Hoare's selection, ordinary comparisons)
AMPLI_FN double ampli_amplicon_select(double *v, int64_t m, int64_t k)
{
    int64_t lo = 0, hi = m - 1;
    while (lo < hi) {
        const double pivot = v[lo + (hi - lo) / 2];
        int64_t i = lo, j = hi;
        while (i <= j) {
            while (v[i] < pivot) ++i;
            while (pivot < v[j]) --j;
            if (i <= j) {
                const double t = v[i];
                v[i] = v[j];
                v[j] = t;
                ++i;
                --j;
            }
        }
        if (k <= j) hi = j;
        else if (k >= i) lo = i;
        else break;
    }
    return v[k];
}

// the median of the values of v[0 .. m) that are not NaN (signed values; v is reordered); NaN if there is none
AMPLI_FN double ampli_amplicon_median(double *v, int64_t m)
{
    int64_t c = 0;
    for (int64_t i = 0; i < m; ++i)
        if (v[i] == v[i]) v[c++] = v[i];
    if (c == 0) return (double)NAN;
    const double hi = ampli_amplicon_select(v, c, c / 2);
    const double lo = (c & 1) ? hi : ampli_amplicon_select(v, c, c / 2 - 1);
    return ampli_amplicon_median_pick(lo, hi, c);
}

AMPLI_FN double ampli_amplicon_z(double ratio, double med, double mad)
{
    if (!(mad > 0.0)) return (double)NAN;
    const double num = (ratio - 1.0) * med;
    const double den = 1.4826 * mad;
    return num / den;
}

AMPLI_FN int ampli_amplicon_gene_status(int64_t n, double median_ratio, double median_z, int64_t min_amplicons, double gain_ratio, double loss_ratio,
                                        double z_cutoff)
{
    if (n >= min_amplicons && median_ratio >= gain_ratio && median_z >= z_cutoff) return AMPLI_GENE_GAIN;
    if (n >= min_amplicons && median_ratio <= loss_ratio && median_z <= -z_cutoff) return AMPLI_GENE_LOSS;
    return AMPLI_GENE_NEUTRAL;
}

// ---------------------------------------------------------------------------
// Substitution spectrum and strand asymmetry (the definition is tests/spectrum_model.py).
//
// Stage 1, integers (spectrum_kernel and ampli_host_spectrum_enters_batch run ampli_spectrum_enters): the PRIMARY record of (sample,
// position) enters iff it is present, the position's reference code is 0..3 and its class is below C, FW >= cutoff and BW >= cutoff,
// and every base b other than the reference has 1000 n_b <= max_alt_pm d (n_b = fw[b] + bw[b], d = FW + BW, all in int64: an int32
// record may hold counts near 2^31).  d == 0 passes the last clause and is stopped only by a positive cut-off.  An entering record
// adds 1 and its eight counts to the nine sums of (sample, class), index order AMPLI_SPEC_*.
//
// Stage 2, on the host, every operation one IEEE double operation in the written order (unfused, -ffp-contract=off):
//   classes of the command line  16 r + 4 l + t with r the reference code and l, t the codes of the panel's own reference bases at
//           coordinate - 1 / + 1 of the same chromosome; 64 + r where a neighbour is missing or not A/C/G/T; 255 where r is not 0..3
//   types   ty = 3 r + k, k counting the alternatives in A,C,G,T order without r; type 12 (ALL) pools the twelve
//   fold    ALT[st][ty] = sum over the classes with that r of count[st][y]; DEP[st][ty] = sum over them of the four counts of strand
//           st (the same for the three types of one r); SITES[ty] likewise; ALL: the sums over every class
//   rates   rate[st] = DEP[st] > 0 ? ALT[st] / DEP[st] : NaN; rate2 = DEP_fw + DEP_bw > 0 ? (ALT_fw + ALT_bw) / (DEP_fw + DEP_bw) : NaN;
//           asym = rate_fw + rate_bw > 0 ? rate_fw / (rate_fw + rate_bw) : NaN
//   reference, per type, from the normals with SITES >= min_sites (N_eff of them): med, mad of rate2 and med_a, mad_a of asym by
//           ampli_amplicon_median (NaNs dropped); FEW if N_eff < min_normals
//   score   ratio = med > 0 ? rate2 / med : NaN; z = mad > 0 ? (rate2 - med) / (1.4826 mad) : NaN; za likewise from asym
//   flag    LOW_SITES if SITES < min_sites, else NO_REFERENCE if FEW, else ELEVATED if ratio >= excess_ratio and z >= z_cutoff, else
//           ASYMMETRIC if |za| >= z_cutoff and |asym - med_a| >= asym_delta, else OK; a comparison with NaN is false
//   96 channels  the classes below 64 folded onto a pyrimidine reference base (r in {A, G}: r' = 3 - r, l' = 3 - t, t' = 3 - l,
//           y' = 3 - y), both strands summed: channel 16 sub + 4 l' + t', sub = (r' == T ? 3 : 0) + k' -- C>A C>G C>T T>A T>C T>G
// ---------------------------------------------------------------------------

// the gate of one record, without a branch on the data: every clause is evaluated and the results are and-ed
AMPLI_FN int ampli_spectrum_enters(const int32_t fw[4], const int32_t bw[4], int present, uint32_t ref, uint32_t cls, int32_t C, int32_t cutoff,
                                   int32_t max_alt_pm)
{
    int64_t n[4], FW = 0, BW = 0;
    for (int b = 0; b < 4; ++b) {
        n[b] = (int64_t)fw[b] + (int64_t)bw[b];
        FW += (int64_t)fw[b];
        BW += (int64_t)bw[b];
    }
    const int64_t lim = (int64_t)max_alt_pm * (FW + BW);
    int ok = present != 0 && ref <= 3u && cls < (uint32_t)C && FW >= (int64_t)cutoff && BW >= (int64_t)cutoff;
    for (int b = 0; b < 4; ++b) ok &= ((uint32_t)b == ref) | (1000 * n[b] <= lim);
    return ok;
}

// the code of one reference-base string as a neighbour sees it: upper-cased, one of A C G T, else 255
AMPLI_FN uint32_t ampli_spectrum_base_code(const char *s)
{
    if (!s || !s[0] || s[1]) return 255u;
    const char c = (char)(s[0] >= 'a' && s[0] <= 'z' ? s[0] - 'a' + 'A' : s[0]);
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 255u;
}

// the class of a position from its reference code and its neighbours' codes (255: no such neighbour, or not A/C/G/T)
AMPLI_FN uint32_t ampli_spectrum_class(uint32_t r, uint32_t l, uint32_t t)
{
    if (r > 3u) return AMPLI_SPECTRUM_SKIP;
    return (l <= 3u && t <= 3u) ? 16u * r + 4u * l + t : 64u + r;
}

// the index of alternative y among A,C,G,T without r (y != r)
AMPLI_FN int ampli_spectrum_alt_index(int r, int y) { return y < r ? y : y - 1; }

// the sums of one sample, int64 [68][9], folded: alt, dep [2][13], sites [13], and the 96 channels (ctx_alt, ctx_dep; both may be NULL)
AMPLI_FN void ampli_spectrum_fold(const int64_t *sums, int64_t *alt, int64_t *dep, int64_t *sites, int64_t *ctx_alt, int64_t *ctx_dep)
{
    const int T = AMPLI_SPECTRUM_TYPES;
    for (int i = 0; i < 2 * T; ++i) alt[i] = dep[i] = 0;
    for (int i = 0; i < T; ++i) sites[i] = 0;
    if (ctx_alt && ctx_dep)
        for (int i = 0; i < AMPLI_SPECTRUM_CHANNELS; ++i) ctx_alt[i] = ctx_dep[i] = 0;
    for (int c = 0; c < AMPLI_SPECTRUM_CLASSES; ++c) {
        const int64_t *v = sums + (size_t)c * AMPLI_SPEC_SUMS;
        const int r = c < 64 ? c >> 4 : c - 64;
        int64_t depth[2];
        for (int st = 0; st < 2; ++st) {
            depth[st] = v[1 + 4 * st] + v[2 + 4 * st] + v[3 + 4 * st] + v[4 + 4 * st];
            for (int k = 0; k < 3; ++k) dep[st * T + 3 * r + k] += depth[st];
            dep[st * T + AMPLI_SPECTRUM_ALL] += depth[st];
            for (int y = 0; y < 4; ++y) {
                if (y == r) continue;
                alt[st * T + 3 * r + ampli_spectrum_alt_index(r, y)] += v[1 + 4 * st + y];
                alt[st * T + AMPLI_SPECTRUM_ALL] += v[1 + 4 * st + y];
            }
        }
        for (int k = 0; k < 3; ++k) sites[3 * r + k] += v[AMPLI_SPEC_SITES];
        sites[AMPLI_SPECTRUM_ALL] += v[AMPLI_SPEC_SITES];
        if (c >= 64 || !ctx_alt || !ctx_dep) continue;
        const int l = (c >> 2) & 3, t = c & 3, pyr = r == 1 || r == 3;
        const int r2 = pyr ? r : 3 - r, l2 = pyr ? l : 3 - t, t2 = pyr ? t : 3 - l;
        for (int y = 0; y < 4; ++y) {
            if (y == r) continue;
            const int y2 = pyr ? y : 3 - y;
            const int ch = 16 * ((r2 == 3 ? 3 : 0) + ampli_spectrum_alt_index(r2, y2)) + 4 * l2 + t2;
            ctx_alt[ch] += v[1 + y] + v[5 + y];
            ctx_dep[ch] += depth[0] + depth[1];
        }
    }
}

// the rates of one (sample, type) from its strand sums
AMPLI_FN void ampli_spectrum_rates(int64_t alt_fw, int64_t dep_fw, int64_t alt_bw, int64_t dep_bw, double *rate_fw, double *rate_bw, double *rate2,
                                   double *asym)
{
    const double rf = dep_fw > 0 ? (double)alt_fw / (double)dep_fw : (double)NAN;
    const double rb = dep_bw > 0 ? (double)alt_bw / (double)dep_bw : (double)NAN;
    const double sum = rf + rb;
    *rate_fw = rf;
    *rate_bw = rb;
    *rate2 = dep_fw + dep_bw > 0 ? (double)(alt_fw + alt_bw) / (double)(dep_fw + dep_bw) : (double)NAN;
    *asym = sum > 0.0 ? rf / sum : (double)NAN;
}

// (x - med) / (1.4826 mad), NaN unless mad > 0
AMPLI_FN double ampli_spectrum_z(double x, double med, double mad)
{
    if (!(mad > 0.0)) return (double)NAN;
    const double num = x - med;
    const double den = 1.4826 * mad;
    return num / den;
}

AMPLI_FN int ampli_spectrum_flag(int64_t sites, int few, double ratio, double z, double asym, double med_a, double za, const ampli_spectrum_params *q)
{
    if (sites < q->min_sites) return AMPLI_SPECTRUM_LOW_SITES;
    if (few) return AMPLI_SPECTRUM_NO_REFERENCE;
    if (ratio >= q->excess_ratio && z >= q->z_cutoff) return AMPLI_SPECTRUM_ELEVATED;
    if (fabs(za) >= q->z_cutoff && fabs(asym - med_a) >= q->asym_delta) return AMPLI_SPECTRUM_ASYMMETRIC;
    return AMPLI_SPECTRUM_OK;
}

// The score of S samples, the first N of them the normals, from their folds alt, dep int64 [S][2][13] and sites int64 [S][13].
// tmp: N doubles of scratch.  ref double [13][4] = med, mad, med_a, mad_a; n_eff int32 [13]; status uint8 [13] (AMPLI_SPECTRUM_REF_*);
// rate2, ratio, z, asym, za double [S][13]; flag uint8 [S][13] (AMPLI_SPECTRUM_OK ...).
AMPLI_FN void ampli_spectrum_score(const int64_t *alt, const int64_t *dep, const int64_t *sites, int64_t S, int64_t N, const ampli_spectrum_params *q,
                                   double *tmp, double *ref, int32_t *n_eff, uint8_t *status, double *rate2, double *ratio, double *z, double *asym,
                                   double *za, uint8_t *flag)
{
    const int T = AMPLI_SPECTRUM_TYPES;
    for (int64_t s = 0; s < S; ++s)
        for (int ty = 0; ty < T; ++ty) {
            const int64_t *a = alt + s * 2 * T, *d = dep + s * 2 * T;
            double rf, rb;
            ampli_spectrum_rates(a[ty], d[ty], a[T + ty], d[T + ty], &rf, &rb, &rate2[s * T + ty], &asym[s * T + ty]);
        }
    for (int ty = 0; ty < T; ++ty) {
        double *r = ref + 4 * ty;
        for (int pass = 0; pass < 2; ++pass) { // rate2, then asym
            const double *x = pass ? asym : rate2;
            int64_t m = 0;
            for (int64_t n = 0; n < N; ++n)
                if (sites[n * T + ty] >= q->min_sites) tmp[m++] = x[n * T + ty];
            if (!pass) n_eff[ty] = (int32_t)m;
            const double med = ampli_amplicon_median(tmp, m);
            m = 0;
            for (int64_t n = 0; n < N; ++n)
                if (sites[n * T + ty] >= q->min_sites) tmp[m++] = fabs(x[n * T + ty] - med);
            r[2 * pass] = med;
            r[2 * pass + 1] = ampli_amplicon_median(tmp, m);
        }
        status[ty] = (uint8_t)((int64_t)n_eff[ty] < q->min_normals ? AMPLI_SPECTRUM_REF_FEW : AMPLI_SPECTRUM_REF_OK);
        for (int64_t s = 0; s < S; ++s) {
            const int64_t i = s * T + ty;
            ratio[i] = r[0] > 0.0 ? rate2[i] / r[0] : (double)NAN;
            z[i] = ampli_spectrum_z(rate2[i], r[0], r[1]);
            za[i] = ampli_spectrum_z(asym[i], r[2], r[3]);
            flag[i] = (uint8_t)ampli_spectrum_flag(sites[i], status[ty] == AMPLI_SPECTRUM_REF_FEW, ratio[i], z[i], asym[i], r[2], za[i], q);
        }
    }
}

// ---------------------------------------------------------------------------
// Panel-of-normals exceedance (the definition is tests/exceedance_model.py): the candidate rule on top of the counts of
// ampli_exceedance_records.  Integers only.  A cell (tumour row, position, base) with the tumour's alt reads x[st] and depths D[st]
// per strand, the position's eligible normals and the cell's two counts ge[st] is a candidate iff it is evaluated (neither count is
// AMPLI_EXCEEDANCE_NA) and
//   x[0] >= min_alt_reads and x[1] >= min_alt_reads, 1000 (x[0] + x[1]) >= min_vaf_pm (D[0] + D[1]), elig >= min_normals,
//   ge[0] <= max_normals and ge[1] <= max_normals
// -- the PER-STRAND rule: at most max_normals normals reach on the forward strand and at most max_normals on the reverse.  ("No
// normal reaches on both strands at once" is a different, far weaker rule and is not this one.)  A field is below 2^31 and a depth
// below 2^33, min_vaf_pm at most 1000: no product leaves unsigned 64 bits.
// ---------------------------------------------------------------------------
// every count >= 0 and min_vaf_pm at most 1000
AMPLI_FN int ampli_exceedance_params_ok(const ampli_exceedance_params *q)
{
    return q->min_alt_reads >= 0 && q->min_vaf_pm >= 0 && q->min_vaf_pm <= 1000 && q->min_normals >= 0 && q->max_normals >= 0;
}
AMPLI_FN int ampli_exceedance_candidate(uint64_t x_fw, uint64_t x_bw, uint64_t d_fw, uint64_t d_bw, uint32_t elig, uint32_t ge_fw, uint32_t ge_bw,
                                        const ampli_exceedance_params *q)
{
    const int evaluated = ge_fw != AMPLI_EXCEEDANCE_NA && ge_bw != AMPLI_EXCEEDANCE_NA;
    const int reads = x_fw >= (uint64_t)q->min_alt_reads && x_bw >= (uint64_t)q->min_alt_reads;
    const int vaf = 1000ull * (x_fw + x_bw) >= (uint64_t)q->min_vaf_pm * (d_fw + d_bw);
    const int normals = (int64_t)elig >= q->min_normals;
    const int top = (int64_t)ge_fw <= q->max_normals && (int64_t)ge_bw <= q->max_normals;
    return evaluated & reads & vaf & normals & top;
}

// ---------------------------------------------------------------------------
// Overdispersion-aware calling (the definition is tests/overdispersion_model.py).
//
// The fit.  A cell (strand, base, position) of the panel with its n qualifying records (dispersion's set), K = sum k_i, D = sum d_i,
// S2 = sum d_i^2, Pearson's X2 and dispersion's status.  Under k_i ~ Poisson(lambda_i d_i), E lambda_i = r, Var lambda_i = omega r^2:
//   E[X2] = (n - 1) + omega r (D - S2 / D),  so  omega = (X2 - (n - 1)) D / (K (D - S2 / D))
// where the status carries AMPLI_DISPERSION_HIGH and D - S2 / D > 0; every other cell, and a quotient that is not above 0 (a negative
// z_cutoff), has omega = 0: the reference's Poisson model.  A HIGH status comes from an OK cell, so n >= 2 and K >= 2 are assumed: planes that
// do not belong together (HIGH with K = 0) give an infinite or NaN omega, which the score answers with AMPLI_NB_NA.  Five roundings and the subtraction: within 16 * 2^-53 * omega * (2 + S2 /
// (D^2 - S2)) of the exact quotient of the same X2.
//
// The score.  p = P[X >= k] for X negative binomial with mean m = double(d) * double(e) and variance m + omega m^2:
//   pmf(0) = (1 + m omega)^(-1 / omega),  pmf(j + 1) / pmf(j) = (1 + j omega) / (j + 1) * m / (1 + m omega);
// omega = 0 is the Poisson law itself, and omega below AMPLI_NB_POISSON_BELOW is taken as 0.  This is the mathematical tail: it is NOT
// the reference's kf_gammaq with its 100-term cut-offs, and at omega = 0 it differs from ampli_poisson_score wherever those cut-offs bite.
//   * ONE term starts a sum, in the saddle-point form (as ampli_binom_logpmf): with s = 1 / omega, N = j + s, a = 1 + m omega,
//       ln pmf(j) = -1/2 ln(2 pi j (1 + j omega)) + d(N) - d(j) - d(s) - bd0(j, N m omega / a) - bd0(s, N / a),
//     d = Stirling's error and both deviances taken from the difference (j - m) / a, which is formed without cancellation: no lgamma
//     difference at large s, and pmf(0) is never the start of a sum that goes up, so it cannot underflow one.
//   * k > m, upwards from k: every later ratio is below rb = max(the next ratio, m omega / a) < 1, so what is left after a term t with
//     next ratio r is below t r / (1 - rb); the sum ends once that is below AMPLI_NB_EPS of the sum (RELATIVE: p is wanted down to
//     1e-10).  That takes at most AMPLI_NB_TERMS_UP(m, omega) terms.  A first term below e^-80 ends the tail at once: it is below
//     5e-31 and returned as 0.
//   * otherwise, and where k terms are fewer than that bound, the complement: downwards from k - 1, to 0 or -- for omega < 1, where the
//     ratios fall on the way down -- until what is left is below AMPLI_NB_EPS_DOWN.  A complement that comes out below AMPLI_NB_SWITCH
//     has lost digits to 1 - sum and is summed again upwards where AMPLI_NB_TERMS_UP(m, omega) <= AMPLI_NB_MAX_TERMS.
//   * no sum is longer than AMPLI_NB_MAX_TERMS terms, a tail never more than twice that (asserted in tests/test_overdispersion_host.py).
//     A tail that would need more -- k > 2^20 with 40 (1 + m omega) > 2^20, or omega >= 1 with k - 1 <= m beyond 2^20 -- is a NaN and
//     its score AMPLI_NB_NA.  A complement below AMPLI_NB_SWITCH whose upward sum does not fit (m omega > 26 000 and k in the hundreds
//     of thousands) keeps its lost digits.
// |Q - exact| <= 1e-5 for m in [1e-3, 1e4], omega = 0 or in [1e-8, 1e4] and k <= 10 m + 2 (tests/test_overdispersion_host.py); the same
// arithmetic, and on the samples tested the same bound, between 0 and 1e-8.
// One ampli_nb_step is a short run of terms, so that a kernel runs the tails of a lane in a single loop (as ampli_tail_step).
// ---------------------------------------------------------------------------
#define AMPLI_NB_POISSON_BELOW 1e-290
#define AMPLI_NB_EPS 1e-9
#define AMPLI_NB_EPS_DOWN 1e-18
#define AMPLI_NB_SWITCH 1e-4
#define AMPLI_NB_LOG_FLOOR (-80.0)       // an upward sum whose first term is below e^-80 is 0
#define AMPLI_NB_RUN 8                   // terms per ampli_nb_step
#define AMPLI_NB_MAX_TERMS (1 << 20)     // of one sum: the loop's own bound
#define AMPLI_NB_TERMS_UP(m, w) (8.0 * sqrt((m) + (w) * (m) * (m)) + 40.0 * (1.0 + (m) * (w)) + 64.0)

AMPLI_FN double ampli_overdispersion_cell(uint8_t status, int32_t n, double K, double D, double x2, double s2)
{
    if (!(status & AMPLI_DISPERSION_HIGH)) return 0.0;
    const double den = D - s2 / D;
    if (!(den > 0.0)) return 0.0;
    const double w = (x2 - ((double)n - 1.0)) * D / (K * den);
    return w > 0.0 ? w : 0.0;
}

// d(x) for a real x > 0
AMPLI_FN double ampli_stirling_err_real(double x)
{
    if (x >= 16.0) {
        const double r = 1.0 / (x * x);
        return (1.0 / 12 - (1.0 / 360 - (1.0 / 1260 - 1.0 / 1680 * r) * r) * r) / x;
    }
    return lgamma(x + 1.0) - ((x + 0.5) * log(x) - x + 0.918938533204672742);
}

// x ln(x / mu) + mu - x for x, mu > 0 with diff = x - mu given
AMPLI_FN double ampli_bd0_diff(double x, double mu, double diff)
{
    if (fabs(diff) < 0.1 * mu) {
        const double t = diff / mu;
        return mu * ((1.0 + t) * log1p(t) - t);
    }
    return x * log(x / mu) - diff;
}

// ln pmf(j), j >= 0 an integer, m > 0, w >= 0
AMPLI_FN double ampli_nb_logpmf(double j, double m, double w)
{
    if (!(w >= AMPLI_NB_POISSON_BELOW)) {
        if (j <= 0.0) return -m;
        return -0.5 * log(6.283185307179586477 * j) - ampli_stirling_err_real(j) - ampli_bd0_diff(j, m, j - m);
    }
    const double mw = m * w, a = 1.0 + mw;
    if (j <= 0.0) return -log1p(mw) / w;
    const double s = 1.0 / w, N = j + s, delta = (j - m) / a;
    return -0.5 * log(6.283185307179586477 * j * (1.0 + j * w)) + ampli_stirling_err_real(N) - ampli_stirling_err_real(j) - ampli_stirling_err_real(s) -
           ampli_bd0_diff(j, N * mw / a, delta) - ampli_bd0_diff(s, N / a, -delta);
}

typedef struct {
    double k, m, w;  // the tail's count, mean and omega
    double qq, lim;  // m / (1 + m omega); m omega / (1 + m omega), the limit of the ratios going up
    double j, t, sum; // index of the latest term; the term; the terms so far
    double res;      // the tail, once live == 0 (a NaN: not computable within the bound)
    int32_t up;      // the sum is the tail (from k upwards) / its complement (from k - 1 downwards)
    int32_t retry;   // a complement below AMPLI_NB_SWITCH is summed again upwards
    int32_t terms;   // pmf terms formed in this sum, the first one included
    int32_t total;   // ... in every sum of this tail
    int32_t live;
} ampli_nb_sum;

AMPLI_FN void ampli_nb_start(ampli_nb_sum *s, int up)
{
    const double j = up ? s->k : s->k - 1.0;
    const double lp = ampli_nb_logpmf(j, s->m, s->w);
    s->up = up; s->j = j; s->terms = 1; s->total += 1; s->live = 1;
    s->t = s->sum = exp(lp);
    // upwards what follows the first term is below t / (1 - rb) <= t (1 + m omega) <= 2.7e4 t: a tail below 5e-31 is returned as 0, and
    // no sum starts among the denormals, where the terms cannot fall any more
    if (up && !(lp >= AMPLI_NB_LOG_FLOOR)) { s->res = 0.0; s->live = 0; }
    if (!up && j > s->m && lp < -600.0) { s->res = 0.0; s->live = 0; } // far above the mean: the terms below would all be lost
}

AMPLI_FN void ampli_nb_init(ampli_nb_sum *s, double k, double m, double w)
{
    s->k = k; s->m = m; s->w = w; s->qq = 0; s->lim = 0; s->j = 0; s->t = 0; s->sum = 0; s->res = 0;
    s->up = 0; s->retry = 0; s->terms = 0; s->total = 0; s->live = 0;
    if (k <= 0.0) { s->res = 1.0; return; }
    if (!(m > 0.0)) { s->res = 0.0; return; }
    if (!(w >= AMPLI_NB_POISSON_BELOW)) s->w = w = 0.0;
    const double a = 1.0 + m * w, est_up = AMPLI_NB_TERMS_UP(m, w);
    s->qq = m / a; s->lim = m * w / a;
    const int up_ok = k > m && est_up <= (double)AMPLI_NB_MAX_TERMS;
    if (up_ok && est_up < k) { ampli_nb_start(s, 1); return; }
    if (!up_ok && k > (double)AMPLI_NB_MAX_TERMS && w >= 1.0) { s->res = NAN; return; }
    s->retry = up_ok;
    ampli_nb_start(s, 0);
}

AMPLI_FN void ampli_nb_step(ampli_nb_sum *s)
{
    double j = s->j, t = s->t, sum = s->sum;
    const double w = s->w, qq = s->qq, lim = s->lim;
    int terms = s->terms, end = 0; // 1: the sum is complete, 2: the bound
    for (int i = 0; i < AMPLI_NB_RUN; ++i) {
        double r;
        if (s->up) {
            r = (1.0 + j * w) / (j + 1.0) * qq;
            const double rb = r > lim ? r : lim;
            if (!(t * r > AMPLI_NB_EPS * sum * (1.0 - rb))) { end = 1; break; }
        } else {
            if (j <= 0.0) { end = 1; break; }
            r = j / ((1.0 + (j - 1.0) * w) * qq);
            if (w < 1.0 && r < 1.0 && t * r < AMPLI_NB_EPS_DOWN * (1.0 - r)) { end = 1; break; }
        }
        if (terms >= AMPLI_NB_MAX_TERMS) { end = 2; break; }
        t *= r;
        sum += t;
        j += s->up ? 1.0 : -1.0;
        ++terms;
    }
    s->total += terms - s->terms;
    s->j = j; s->t = t; s->sum = sum; s->terms = terms;
    if (!end) return;
    s->live = 0;
    if (end == 2) { s->res = NAN; return; }
    if (s->up) { s->res = sum < 1.0 ? sum : 1.0; return; }
    s->res = sum < 1.0 ? 1.0 - sum : 0.0;
    if (s->retry && s->res < AMPLI_NB_SWITCH) { s->retry = 0; ampli_nb_start(s, 1); }
}

// Q of a tail: 0 for p >= 1, -10 log10(max(p, 1e-10)) as a float, AMPLI_NB_NA for a NaN
AMPLI_FN float ampli_nb_q_from_p(double p)
{
    if (p != p) return AMPLI_NB_NA;
    if (p >= 1.0) return 0.0f;
    return (float)(-10.0 * log10(p > 1e-10 ? p : 1e-10));
}

// what a score needs before its sum: returns 1 with *s ready for ampli_nb_step while s->live, else 0 with *q the score.  k alternative
// reads of d on the strand, e the table's threshold (-1: Q = -888; 0: 0.0010008f, VC:3844-3856); a negative, NaN or infinite omega
// gives AMPLI_NB_NA.
AMPLI_FN int ampli_nb_score_begin(ampli_nb_sum *s, int32_t k, int32_t d, float e, double w, float *q)
{
    s->live = 0; s->total = 0;
    if (!(w >= 0.0) || w > 1.79769313486231570815e308) { *q = AMPLI_NB_NA; return 0; }
    if (e == -1.0f) { *q = -888.0f; return 0; }
    if (e == 0.0f) e = 0.0010008f;
    if (k == 0) { *q = 0.0f; return 0; }
    ampli_nb_init(s, (double)k, (double)d * (double)e, w);
    if (!s->live) { *q = ampli_nb_q_from_p(s->res); return 0; }
    return 1;
}

// the whole of one score (host, tests); *terms (optional) = pmf terms formed
AMPLI_FN float ampli_nb_score(int32_t k, int32_t d, float e, double w, int32_t *terms)
{
    ampli_nb_sum s;
    float q;
    if (ampli_nb_score_begin(&s, k, d, e, w, &q)) {
        while (s.live) ampli_nb_step(&s);
        q = ampli_nb_q_from_p(s.res);
    }
    if (terms) *terms = s.total;
    return q;
}

// ---------------------------------------------------------------------------
// Paired comparison (the definition is tests/paired_model.py): the exact conditional test of two count files at one cell.
//
// File a shows k_a alternative reads among d_a on a strand, file b k_b among d_b.  N = d_a + d_b, K = k_a + k_b, n = d_a, and X is
// hypergeometric: the number of alternative reads among a's n when K alternative reads are dealt among N.  The side is decided in
// integers by c = k_a N - K n = k_a d_b - k_b d_a -- two products below 2^64 for any int32 record, compared as unsigned 64-bit words:
//   K == 0 or c == 0:  S = +0;   c > 0:  p = P[X >= k_a], S = +Q(p);   c < 0:  p = P[X <= k_a], S = -Q(p),
//   Q(p) = (float)(-10 log10(max(p, 1e-10))), +0 for p >= 1; -0 is never stored.
// Only the tail on the observation's own side of the mean is ever summed: the short sum, never a complement (no digits lost to 1 - sum).
//   * ONE term starts the sum, from three binomial terms in the saddle-point form (ampli_binom_logpmf) with v = n / N:
//       ln pmf(x) = ln b(K, x, v) + ln b(N - K, n - x, v) - ln b(N, n, v)
//     -- no lgamma difference, and the deviances are all non-negative and add (the third is 0: n is Bin(N, v)'s own mean).
//   * the later terms come from the ratio, upwards (K - x)(n - x) / ((x + 1)(N - K - n + x + 1)), downwards its mirror
//     x (N - K - n + x) / ((K - x + 1)(n - x + 1)).  Both are A B / (C D) with A and B falling and C and D rising by one per term, which
//     is how the sum keeps them.  c != 0 puts k_a strictly beyond the mean on its side, hence at or beyond the mode: the ratio is below 1
//     from the first step and falls from step to step; it is 0 at the end of the support, which ends the sum.
//   * what is left after a term t with next ratio r is below t r / (1 - r): the sum ends once that is below AMPLI_HYPER_EPS of the sum
//     (RELATIVE: p is wanted down to 1e-10, as for ampli_nb_step).  A first term with t / (1 - r) < 1e-10 decides the score without a
//     sum: +-100.
//   * terms.  The relative cut-off is reached within about 6.1 standard deviations of the mean when the sum starts there (what is left
//     is 1e-9 of a sum of about 1/2) and sooner for a start farther out; sums never cross the mean.  With the hypergeometric variance
//     var = n (K / N) (1 - K / N) (N - n) / (N - 1) a tail costs at most AMPLI_HYPER_TERMS(var) terms (asserted in
//     tests/test_paired_host.py over the grid) -- below 2^18 for every int32 record.  The loop's own bound is AMPLI_HYPER_MAX_TERMS;
//     a tail that would need more is a NaN and its score AMPLI_PAIR_NA, not a wrong number.
// One ampli_hyper_step is AMPLI_TAIL_RUN terms, so that a kernel runs all of a lane's cells in a single loop (as ampli_nb_step).
// ---------------------------------------------------------------------------
#define AMPLI_HYPER_EPS 1e-9
#define AMPLI_HYPER_MAX_TERMS (1 << 20)  // of one sum: the loop's own bound
#define AMPLI_HYPER_TERMS(var) (8.0 * sqrt(var) + 64.0)

typedef struct {
    double A, B, C, D; // the next ratio is A B / (C D)
    double t, sum;     // the latest term; the terms so far
    double res;        // the tail, once live == 0 (a NaN: not computable within the bound)
    int32_t terms;     // pmf terms formed, the first one included
    int32_t live;
} ampli_hyper_sum;

// the tail of X from k upwards (up != 0) or from k downwards, for 0 < n < N, 0 <= K <= N and k in the support of X
AMPLI_FN void ampli_hyper_init(ampli_hyper_sum *s, int64_t N, int64_t K, int64_t n, int64_t k, int up)
{
    const double dN = (double)N, dK = (double)K, dn = (double)n, x = (double)k, v = dn / dN;
    const double rest = (double)(N - K - n + k); // b's other reads, formed in integers
    double dev;
    const double lp = ampli_binom_logpmf(dK, x, v, &dev) + ampli_binom_logpmf(dN - dK, dn - x, v, &dev) - ampli_binom_logpmf(dN, dn, v, &dev);
    if (up) { s->A = dK - x; s->B = dn - x; s->C = x + 1.0; s->D = rest + 1.0; }
    else { s->A = x; s->B = rest; s->C = dK - x + 1.0; s->D = dn - x + 1.0; }
    s->t = s->sum = exp(lp);
    s->res = 0.0; s->terms = 1; s->live = 1;
    const double r = (s->A * s->B) / (s->C * s->D);
    if (!(r < 1.0)) { s->res = 1.0; s->live = 0; return; }          // not beyond the mode: no caller with c != 0 comes here
    if (s->t < 1e-10 * (1.0 - r)) { s->res = 0.0; s->live = 0; }     // the whole tail is below 1e-10: decided without a sum
}

AMPLI_FN void ampli_hyper_step(ampli_hyper_sum *s)
{
    double A = s->A, B = s->B, Cc = s->C, D = s->D, t = s->t, sum = s->sum;
    int terms = s->terms, end = 0; // 1: the sum is complete, 2: the bound
    for (int i = 0; i < AMPLI_TAIL_RUN; ++i) {
        const double r = (A * B) / (Cc * D); // 0 at the end of the support
        if (!(t * r >= AMPLI_HYPER_EPS * sum * (1.0 - r))) { end = 1; break; }
        if (terms >= AMPLI_HYPER_MAX_TERMS) { end = 2; break; }
        t *= r;
        sum += t;
        A -= 1.0; B -= 1.0; Cc += 1.0; D += 1.0;
        ++terms;
    }
    s->A = A; s->B = B; s->C = Cc; s->D = D; s->t = t; s->sum = sum; s->terms = terms;
    if (!end) return;
    s->live = 0;
    s->res = end == 2 ? (double)NAN : (sum < 1.0 ? sum : 1.0);
}

// the signed score of a tail p on side sign (+1: a's fraction is the higher): +0 for p >= 1, AMPLI_PAIR_NA for a NaN
AMPLI_FN float ampli_pair_s_from_p(double p, int sign)
{
    if (p != p) return AMPLI_PAIR_NA;
    if (p >= 1.0) return 0.0f;
    const float q = (float)(-10.0 * log10(p > 1e-10 ? p : 1e-10));
    if (q == 0.0f) return 0.0f;
    return sign > 0 ? q : -q;
}

// what a cell needs before its sum: returns the side (+1 / -1) with *s ready for ampli_hyper_step while s->live, or 0 with *q the
// score.  Counts and depths of one strand: 0 <= k_a <= d_a, 0 <= k_b <= d_b, below 2^33 (the four int32 counts of a strand).
AMPLI_FN int ampli_pair_score_begin(ampli_hyper_sum *s, int64_t k_a, int64_t d_a, int64_t k_b, int64_t d_b, float *q)
{
    s->live = 0; s->terms = 0;
    const uint64_t lhs = (uint64_t)k_a * (uint64_t)d_b, rhs = (uint64_t)k_b * (uint64_t)d_a; // c = lhs - rhs
    if (k_a + k_b == 0 || lhs == rhs) { *q = 0.0f; return 0; }
    const int sign = lhs > rhs ? 1 : -1;
    ampli_hyper_init(s, d_a + d_b, k_a + k_b, d_a, k_a, sign > 0);
    if (!s->live) { *q = ampli_pair_s_from_p(s->res, sign); return 0; }
    return sign;
}

// the whole of one cell (host, tests); *terms (optional) = pmf terms formed
AMPLI_FN float ampli_pair_score(int64_t k_a, int64_t d_a, int64_t k_b, int64_t d_b, int32_t *terms)
{
    ampli_hyper_sum s;
    float q;
    const int sign = ampli_pair_score_begin(&s, k_a, d_a, k_b, d_b, &q);
    if (sign) {
        while (s.live) ampli_hyper_step(&s);
        q = ampli_pair_s_from_p(s.res, sign);
    }
    if (terms) *terms = s.terms;
    return q;
}

// ---------------------------------------------------------------------------
// False-discovery control (the definition is tests/fdr_model.py): the Benjamini-Hochberg adjusted score of every cell of a
// score plane [rows][P][4][2], each row on its own.  A cell's p-value is the larger of its two strands' -- both strands must show the
// allele -- so its key is the SMALLER strand score a; in the two-sided mode (the paired plane) both strands must lie on one side and
// the p-value doubles, because the side was chosen by the data.
//   one-sided:  TESTED iff 0 <= s_f <= 100 and 0 <= s_b <= 100; a = min(s_f, s_b), sign +.
//   two-sided:  TESTED iff -100 <= s_f <= 100 and -100 <= s_b <= 100; both > 0: a = min, sign +; both < 0: a = min(|s_f|, |s_b|),
//               sign -; otherwise a = 0.
// Everything else -- a NaN, an infinity, any NA sentinel, anything beyond +-100 -- is UNTESTED.  A zero of either sign is a = 0.
// The key is the BIT PATTERN of a (positive floats order as their bit patterns do: no denormal mode enters), 0 for a = 0 and for an
// untested cell alike.  With m the tested cells of the row (a = 0 included) and R = #{tested j : a_j >= a} (the largest rank of a tie):
//   B = a - 10 log10(m / R) - (two_sided ? 10 log10 2 : 0),      A = max(0, max{B_j : 0 < a_j <= a})
// -- BH's step-up minimum over the larger p-values, in score space: q = 10^(-A / 10).  Stored: sign * (float)A, +0 where a = 0 or
// A = 0 (-0 never), AMPLI_FDR_NA where untested.  Rounding to float is monotone, so the running maximum may be taken over
// (float)B: max and rounding commute, and max(0, .) with them.
// ---------------------------------------------------------------------------
#define AMPLI_FDR_UNTESTED 0
#define AMPLI_FDR_ZERO 1
#define AMPLI_FDR_PLUS 2
#define AMPLI_FDR_MINUS 3

AMPLI_FN uint32_t ampli_fdr_float_bits(float a)
{
    union { float f; uint32_t u; } v;
    v.f = a;
    return v.u;
}

// the key of one cell (0 for a = 0 and for an untested cell); *cls = AMPLI_FDR_UNTESTED / _ZERO / _PLUS / _MINUS
AMPLI_FN uint32_t ampli_fdr_key(float s_f, float s_b, int two_sided, int *cls)
{
    const float lo = two_sided ? -100.0f : 0.0f;
    if (!(s_f >= lo && s_f <= 100.0f && s_b >= lo && s_b <= 100.0f)) { *cls = AMPLI_FDR_UNTESTED; return 0u; } // a NaN fails every comparison
    float a = 0.0f;
    int c = AMPLI_FDR_ZERO;
    if (s_f > 0.0f && s_b > 0.0f) { a = s_f < s_b ? s_f : s_b; c = AMPLI_FDR_PLUS; }
    else if (s_f < 0.0f && s_b < 0.0f) { a = s_f > s_b ? -s_f : -s_b; c = AMPLI_FDR_MINUS; } // only the two-sided mode tests a negative score
    *cls = c;
    return c == AMPLI_FDR_ZERO ? 0u : ampli_fdr_float_bits(a);
}

// B of a key a > 0 with rank R among the m tested cells of its row, 1 <= R <= m < 2^31
AMPLI_FN double ampli_fdr_value(uint32_t key, int32_t m, int32_t R, int two_sided)
{
    union { uint32_t u; float f; } v;
    v.u = key;
    const double b = (double)v.f - 10.0 * log10((double)m / (double)R);
    return two_sided ? b - 10.0 * log10(2.0) : b;
}

// what is stored for a cell of class cls whose running maximum of (float)B is bmax: sign * max(0, bmax), never -0
AMPLI_FN float ampli_fdr_store(int cls, float bmax)
{
    if (cls == AMPLI_FDR_UNTESTED) return AMPLI_FDR_NA;
    if (cls == AMPLI_FDR_ZERO || !(bmax > 0.0f)) return 0.0f;
    return cls == AMPLI_FDR_MINUS ? -bmax : bmax;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// In-silico dilution (the definition is tests/dilution_model.py): read-level mixing of two count files.  32-bit integer
// work only, so the device, the host library and the numpy model agree integer for integer.
//   Generator.  Philox4x32-10 (Salmon et al., 2011).  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments W0 = 0x9E3779B9,
//     W1 = 0xBB67AE85.  One round on counter (c0, c1, c2, c3) with key (k0, k1): (hi0, lo0) = M0 * c0 as a 64-bit product,
//     (hi1, lo1) = M1 * c2; the new counter is (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0).  Ten rounds; the key is bumped by (W0, W1)
//     after each round (the bump after the last round is dead).
//   Thinning.  Thin(n, keep; key, p, f, side) = #{ i < n : word_i < keep }, compared as 64-bit unsigned, keep in [0, 2^32].  word_i is
//     output word (i & 3) of Philox with counter (i >> 2, p, f | side << 3, 0) and key (low word, high word of the 64-bit key); p is the
//     position index, f in 0..7 the record field, side 0 for file a and 1 for file b.  A read is word i of its field, kept with
//     probability keep / 2^32, independently.  Exactly: keep = 2^32 keeps all, keep = 0 keeps none, Thin is non-decreasing in n and in
//     keep -- so a series with one key is nested.
//   Mixture.  {int32 row_a; int32 row_b; uint64 keep_a; uint64 keep_b; uint64 key}: out[f] = Thin(a[f], keep_a; key, p, f, 0) +
//     Thin(b[f], keep_b; key, p, f, 1) over the PRIMARY records; row_b == -1 is pure down-sampling.  The output record is ABSENT
//     (field 0 = AMPLI_ABSENT, the other seven 0) when a's record is absent, when b is named and its record is absent, or when a present
//     input record holds a count outside [0, 2^24 - 2] (AMPLI_DILUTE_BAD_COUNT).  A mixture is all ABSENT with AMPLI_DILUTE_BAD_MIXTURE
//     when a row is outside its chunk, a keep is above 2^32, row_b >= 0 without a chunk b, or row_b < -1.
//   Fractions to thresholds.  keep = (uint64) floor(ldexp(x, 32) + 0.5), x a double in [0, 1]: IEEE operations, the same everywhere.
// ------------------------------------------------------------------------------------------------------------------------------------
#define AMPLI_DILUTE_KEEP_ALL 4294967296ull // 2^32

AMPLI_FN void ampli_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the kept reads of ONE Philox block: block j of list (p, fs = f | side << 3), of whose four words the first `live` (1..4) are reads
AMPLI_FN int ampli_thin_block(uint32_t j, int live, uint64_t keep, uint64_t key, uint32_t p, uint32_t fs)
{
    const uint32_t ctr[4] = {j, p, fs, 0u}, k[2] = {(uint32_t)key, (uint32_t)(key >> 32)};
    uint32_t w[4];
    ampli_philox4x32_10(ctr, k, w);
    int c = (uint64_t)w[0] < keep ? 1 : 0;
    c += (live > 1 && (uint64_t)w[1] < keep) ? 1 : 0;
    c += (live > 2 && (uint64_t)w[2] < keep) ? 1 : 0;
    c += (live > 3 && (uint64_t)w[3] < keep) ? 1 : 0;
    return c;
}

// Thin itself, block after block (the host library and the checks; the kernel deals the blocks out to its lanes)
AMPLI_FN int64_t ampli_thin(int64_t n, uint64_t keep, uint64_t key, uint32_t p, int field, int side)
{
    if (n <= 0 || keep == 0) return 0;
    if (keep >= AMPLI_DILUTE_KEEP_ALL) return n;
    int64_t c = 0;
    for (int64_t j = 0; 4 * j < n; ++j) c += ampli_thin_block((uint32_t)j, n - 4 * j >= 4 ? 4 : (int)(n - 4 * j), keep, key, p, (uint32_t)(field | side << 3));
    return c;
}

AMPLI_FN uint64_t ampli_dilute_keep(double x) { return (uint64_t)floor(ldexp(x, 32) + 0.5); }

// a mixture's own faults, checked before any record is loaded; has_b: a chunk b was given
AMPLI_FN int ampli_dilute_mix_ok(int32_t row_a, int32_t row_b, uint64_t keep_a, uint64_t keep_b, int32_t n_a, int32_t n_b, int has_b)
{
    if (row_a < 0 || row_a >= n_a || keep_a > AMPLI_DILUTE_KEEP_ALL || keep_b > AMPLI_DILUTE_KEEP_ALL || row_b < -1) return 0;
    return row_b == -1 || (has_b && row_b < n_b);
}

// a present record's counts all lie in [0, 2^24 - 2]
AMPLI_FN int ampli_dilute_counts_ok(const int32_t r[8])
{
    int ok = 1;
    for (int f = 0; f < 8; ++f) ok &= (uint32_t)r[f] <= (uint32_t)AMPLI_DILUTE_MAX_COUNT;
    return ok;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Tumour-informed monitoring (the definition is tests/monitor_model.py): pooled evidence over the cells of a variant list.
//   Lists.  A CSR: list_off uint32 [L + 1], list_cell uint32 [W], an entry c = 4 p + y (position index p, base y).  Lists may be empty,
//     overlap and name a cell several times (it counts as often).  An entry with p >= P is none.  Offsets are cut to [0, W].
//   Evaluated entry of sample row s, from the PRIMARY record of (s, p): the record is present; D_fw >= coverage_cutoff and D_bw >=
//     coverage_cutoff (a strand's four counts); ref_code[p] in 0..3 and y != it; e_fw = thr[0][y][p] and e_bw = thr[1][y][p] both finite
//     and >= 0 (so not the -1 of VC:3844); 1000 (k_fw + k_bw) <= max_vaf_pm (D_fw + D_bw) in int64, k the strand's count of base y.
//     e == 0 is replaced by 0.0010008f (VC:3852-3856).
//   Sums per (sample, list): N_EVAL, N_SEEN (evaluated entries with k_fw + k_bw >= 1), K_FW, K_BW, D_FW, D_BW in int64, and the doubles
//     Lambda_st = sum (double)d_st * (double)e_st.  Lane j of 64 takes entries j, j + 64, ... in ascending order and adds each product to
//     an accumulator that starts at +0.0 (an entry that is not evaluated adds nothing); the 64 accumulators are combined by
//     x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1.  IEEE additions in that order, unfused: no tolerance.
//   Pooled score per strand: Q = ampli_nb_q_from_p(P[X >= K]), X Poisson of mean Lambda -- ampli_nb_init(K, Lambda, 0) and the step loop:
//     K == 0 gives 0, Lambda == 0 with K > 0 gives 100; N_EVAL == 0 gives AMPLI_MON_NA.
//   Matched random controls: entry i of list l at (p, y) with g = ref_code[p] becomes (p', y), p' = cand[(uint64(word) * m) >> 32] among
//     the m candidates of g (cand_off uint32 [5], cand_pos); word = output word 0 of Philox4x32-10 with counter (i, r, l,
//     AMPLI_MON_CONTROL_TAG) and key (low word, high word of the seed), r the replicate's global index.  No control entry where p >= P,
//     g > 3, m == 0 or p' >= P.  The multiply-high draw favours some candidates by less than m / 2^32.
// ------------------------------------------------------------------------------------------------------------------------------------
AMPLI_FN int ampli_mon_thr_ok(float e) { return e >= 0.0f && e <= 3.402823466e38f; } // a NaN, an infinity and a negative value fail

// what does not depend on the sample: the reference base, the listed base and the two thresholds
AMPLI_FN int ampli_mon_entry_ok(uint32_t ref, uint32_t y, float e_fw, float e_bw)
{
    return ref <= 3u && y != ref && ampli_mon_thr_ok(e_fw) && ampli_mon_thr_ok(e_bw);
}

// what does: the record of an entry that passed ampli_mon_entry_ok
AMPLI_FN int ampli_mon_record_ok(int present, int64_t k_fw, int64_t k_bw, int64_t D_fw, int64_t D_bw, int32_t cov, int32_t max_vaf_pm)
{
    return present && D_fw >= (int64_t)cov && D_bw >= (int64_t)cov && 1000ll * (k_fw + k_bw) <= (int64_t)max_vaf_pm * (D_fw + D_bw);
}

AMPLI_FN double ampli_mon_lambda_term(int64_t d, float e)
{
    if (e == 0.0f) e = 0.0010008f;
    return (double)d * (double)e;
}

// the index among the m candidates of its reference base that entry i of list l takes in replicate r
AMPLI_FN uint32_t ampli_mon_control_draw(uint32_t i, uint32_t r, uint32_t l, uint64_t seed, uint32_t m)
{
    const uint32_t ctr[4] = {i, r, l, AMPLI_MON_CONTROL_TAG}, k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    ampli_philox4x32_10(ctr, k, w);
    return (uint32_t)(((uint64_t)w[0] * (uint64_t)m) >> 32);
}

#ifdef __cplusplus
static_assert(AMPLI_MON_NA == AMPLI_NB_NA, "a tail beyond the term bound leaves ampli_nb_q_from_p as AMPLI_NB_NA and is stored as AMPLI_MON_NA");
#endif
// what a pooled score needs before its sum: returns 1 with *s ready for ampli_nb_step while s->live, else 0 with *q the score
AMPLI_FN int ampli_mon_score_begin(ampli_nb_sum *s, int64_t K, double lam, float *q)
{
    ampli_nb_init(s, (double)K, lam, 0.0);
    if (!s->live) { *q = ampli_nb_q_from_p(s->res); return 0; }
    return 1;
}

// the whole of one strand's pooled score (host, tests)
AMPLI_FN float ampli_mon_score(int64_t n_eval, int64_t K, double lam)
{
    if (n_eval <= 0) return AMPLI_MON_NA;
    ampli_nb_sum s;
    float q;
    if (ampli_mon_score_begin(&s, K, lam, &q)) {
        while (s.live) ampli_nb_step(&s);
        q = ampli_nb_q_from_p(s.res);
    }
    return q;
}

AMPLI_FN int ampli_mon_verdict(int64_t n_eval, int64_t n_seen, float q_fw, float q_bw, int64_t min_variants, int64_t min_seen, double q_min)
{
    if (n_eval < min_variants) return AMPLI_MON_NOT_EVALUABLE;
    return n_seen >= min_seen && (double)q_fw >= q_min && (double)q_bw >= q_min ? AMPLI_MON_DETECTED : AMPLI_MON_NOT_DETECTED;
}

// the pooled excess fraction of a strand: max(0, (K - Lambda) / D); 0 without depth
AMPLI_FN double ampli_mon_excess(int64_t K, double lam, int64_t D)
{
    if (D <= 0) return 0.0;
    const double x = ((double)K - lam) / (double)D;
    return x > 0.0 ? x : 0.0;
}

AMPLI_FN double ampli_mon_empirical_p(int64_t n_ge, int64_t R) { return (1.0 + (double)n_ge) / ((double)R + 1.0); }

// the smallest K >= floor(Lambda) + 1 whose pooled score reaches q_min, walking upwards one count at a time for at most
// AMPLI_MON_LOD_MAX_EVALS evaluations; 0 where none is found within them, q_min is above 100 (or a NaN), or Lambda is not in [0, 2^52)
AMPLI_FN int64_t ampli_mon_lod_reads(double lam, double q_min, int32_t *evals)
{
    if (evals) *evals = 0;
    if (!(q_min <= 100.0) || !(lam >= 0.0) || !(lam < 4503599627370496.0)) return 0;
    int64_t K = (int64_t)floor(lam) + 1;
    for (int i = 0; i < AMPLI_MON_LOD_MAX_EVALS; ++i, ++K) {
        if (evals) *evals = i + 1;
        if ((double)ampli_mon_score(1, K, lam) >= q_min) return K;
    }
    return 0;
}

// the pooled limit of detection of a (sample, list): the larger of the strands' (K_min - Lambda) / D; -1 where a strand has no K_min or no depth
AMPLI_FN double ampli_mon_lod(double lam_fw, double lam_bw, int64_t D_fw, int64_t D_bw, double q_min)
{
    if (D_fw <= 0 || D_bw <= 0) return -1.0;
    const int64_t kf = ampli_mon_lod_reads(lam_fw, q_min, (int32_t *)0), kb = ampli_mon_lod_reads(lam_bw, q_min, (int32_t *)0);
    if (kf <= 0 || kb <= 0) return -1.0;
    const double a = ((double)kf - lam_fw) / (double)D_fw, b = ((double)kb - lam_bw) / (double)D_bw;
    return a > b ? a : b;
}

// ---------------------------------------------------------------------------
// Allelic imbalance at germline het sites (the definition is tests/allelic_model.py).
//
// A het site of pair code c = 0..5, (lo, hi) = (A,C), (A,G), (A,T), (C,G), (C,T), (G,T), shows k_lo reads of its lower base among the
// m = k_lo + k_hi reads of its two bases; the panel of normals expects the share v of them (depth-weighted over the normals that are het
// with the same pair, or 0.5).  d = (double)k_lo - v (double)m, two operations:
//   d == 0:  q = +0;   d > 0:  p = P[X >= k_lo], X ~ Bin(m, v);   d < 0:  p = P[X <= k_lo] = P[Y >= m - k_lo], Y ~ Bin(m, 1.0 - v);
//   p2 = min(1, 2 p),  q = sign(d) (float)(-10 log10(max(p2, 1e-10))),  +0 where p2 >= 1, never -0, |q| <= 100.
// A p2 within 1e-8 of 1 counts as 1 (AMPLI_AI_P2_ONE): the sums below end 1e-9 short of their tails, and a count half a read beyond
// the mean of a symmetric law -- m odd under v = 0.5, the fallback's everyday case -- has 2 p = 1 exactly, which must give +0.
// Both sides are the UPPER tail of a binomial from a count j strictly beyond its mean n w:
//   * ONE term starts the sum, in the saddle-point form (ampli_binom_logpmf); the later ones come from the ratio
//     (n - j) / (j + 1) * w / (1 - w), which is below 1 from the first step, falls from step to step and is 0 at the end of the support;
//   * what is left after a term t with next ratio r is below t r / (1 - r): the sum ends once that is below AMPLI_AI_EPS of the sum
//     (RELATIVE, as ampli_hyper_step).  A first term with t / (1 - r) < 0.5e-10 decides the score without a sum: +-100;
//   * terms: the relative cut-off is reached within about 6.1 standard deviations of the mean when the sum starts there, and a sum that
//     starts farther out than 6.5 is decided by its first term; sums never cross the mean.  A tail costs at most
//     AMPLI_AI_TERMS(n w (1 - w)) terms (asserted in tests/test_allelic_host.py over a grid), below 2^19 for every m < 2^31.  The loop's
//     own bound is AMPLI_AI_MAX_TERMS; a tail that would need more is a NaN and its score AMPLI_AI_NA, not a wrong number.
// One ampli_ai_step is AMPLI_TAIL_RUN terms, so that a kernel runs all of a lane's cells in a single loop (as ampli_nb_step).
// ---------------------------------------------------------------------------
#define AMPLI_AI_EPS 1e-9
#define AMPLI_AI_P2_ONE (1.0 - 1e-8)     // from here on 2 p is 1
#define AMPLI_AI_MAX_TERMS (1 << 20)     // of one sum: the loop's own bound
#define AMPLI_AI_TERMS(var) (8.0 * sqrt(var) + 64.0)
#define AMPLI_AI_MAX_M 2147483647ll      // 2^31 - 1: a deeper site is AMPLI_AI_DEEP

typedef struct {
    double n, j, o;    // reads; index of the latest term; w / (1 - w)
    double t, sum;     // the latest term; the terms so far
    double res;        // the tail, once live == 0 (a NaN: not computable within the bound)
    int32_t terms;     // pmf terms formed, the first one included
    int32_t live;
} ampli_ai_sum;

// P[X >= j], X ~ Bin(n, w), for 0 < w < 1 and an integer j with n w < j <= n
AMPLI_FN void ampli_ai_init(ampli_ai_sum *s, double n, double j, double w)
{
    double dev;
    s->n = n; s->j = j; s->o = w / (1.0 - w);
    s->t = s->sum = exp(ampli_binom_logpmf(n, j, w, &dev));
    s->res = 0.0; s->terms = 1; s->live = 1;
    const double r = (n - j) / (j + 1.0) * s->o;
    if (!(r < 1.0)) { s->res = 1.0; s->live = 0; return; }            // not beyond the mode: no caller with d != 0 comes here
    if (s->t < 0.5e-10 * (1.0 - r)) { s->res = 0.0; s->live = 0; }     // twice the whole tail is below 1e-10: decided without a sum
}

AMPLI_FN void ampli_ai_step(ampli_ai_sum *s)
{
    double j = s->j, t = s->t, sum = s->sum;
    const double n = s->n, o = s->o;
    int terms = s->terms, end = 0; // 1: the sum is complete, 2: the bound
    for (int i = 0; i < AMPLI_TAIL_RUN; ++i) {
        const double r = (n - j) / (j + 1.0) * o; // 0 at the end of the support
        if (!(t * r >= AMPLI_AI_EPS * sum * (1.0 - r))) { end = 1; break; }
        if (terms >= AMPLI_AI_MAX_TERMS) { end = 2; break; }
        t *= r;
        sum += t;
        j += 1.0;
        ++terms;
    }
    s->j = j; s->t = t; s->sum = sum; s->terms = terms;
    if (!end) return;
    s->live = 0;
    s->res = end == 2 ? (double)NAN : (sum < 1.0 ? sum : 1.0);
}

// the signed score of a one-sided tail p on side sign: +0 for 2 p >= 1, AMPLI_AI_NA for a NaN
AMPLI_FN float ampli_ai_q_from_p(double p, int sign)
{
    if (p != p) return AMPLI_AI_NA;
    const double p2 = 2.0 * p;
    if (p2 >= AMPLI_AI_P2_ONE) return 0.0f;
    const float q = (float)(-10.0 * log10(p2 > 1e-10 ? p2 : 1e-10));
    if (q == 0.0f) return 0.0f;
    return sign > 0 ? q : -q;
}

// the pair code of the six plane bits of a (row, position): V and H set and exactly two of A, C, G, T; -1 for anything else
AMPLI_FN int ampli_ai_pair(unsigned g)
{
    if ((g & (AMPLI_GENO_V | AMPLI_GENO_H)) != (unsigned)(AMPLI_GENO_V | AMPLI_GENO_H)) return -1;
    const unsigned b = (g >> 1) & 15u; // A = 1, C = 2, G = 4, T = 8
    return b == 3u ? 0 : b == 5u ? 1 : b == 9u ? 2 : b == 6u ? 3 : b == 10u ? 4 : b == 12u ? 5 : -1;
}
AMPLI_FN int ampli_ai_pair_lo(int c) { return c < 3 ? 0 : (c < 5 ? 1 : 2); }
AMPLI_FN int ampli_ai_pair_hi(int c) { return c == 0 ? 1 : ((c == 1 || c == 3) ? 2 : 3); }

// the status of a cell, the first rule that applies (include/amplisolve_hip.h); *v = the expected share of a tested cell, else 0
AMPLI_FN int ampli_ai_site_status(int pair, int present, int64_t k_lo, int64_t k_hi, int64_t cnt, int64_t lo, int64_t hi, const ampli_allelic_params *prm,
                                  double *v)
{
    *v = 0.0;
    if (pair < 0) return AMPLI_AI_NOT_HET;
    if (!present) return AMPLI_AI_ABSENT;
    const int64_t m = k_lo + k_hi;
    if (m < (int64_t)prm->min_depth) return AMPLI_AI_SHALLOW;
    if (m > AMPLI_AI_MAX_M) return AMPLI_AI_DEEP;
    if (cnt >= (int64_t)prm->min_normals && lo > 0 && hi > 0) {
        *v = (double)lo / (double)(lo + hi);
        return AMPLI_AI_TESTED_REF;
    }
    if (prm->half_fallback) {
        *v = 0.5;
        return AMPLI_AI_TESTED_HALF;
    }
    return AMPLI_AI_NO_REFERENCE;
}

// what a tested cell needs before its sum: returns the side (+1 / -1) with *s ready for ampli_ai_step while s->live, or 0 with *q the score
AMPLI_FN int ampli_ai_site_begin(ampli_ai_sum *s, int64_t k_lo, int64_t m, double v, float *q)
{
    s->live = 0; s->terms = 0;
    const double dk = (double)k_lo, dm = (double)m;
    const double e = v * dm;
    const double d = dk - e;
    if (d == 0.0) { *q = 0.0f; return 0; }
    const int sign = d > 0.0 ? 1 : -1;
    if (sign > 0) ampli_ai_init(s, dm, dk, v);
    else ampli_ai_init(s, dm, (double)(m - k_lo), 1.0 - v);
    if (!s->live) { *q = ampli_ai_q_from_p(s->res, sign); return 0; }
    return sign;
}

// the whole of one tested cell (host, tests); *terms (optional) = pmf terms formed
AMPLI_FN float ampli_ai_site_score(int64_t k_lo, int64_t m, double v, int32_t *terms)
{
    ampli_ai_sum s;
    float q;
    const int sign = ampli_ai_site_begin(&s, k_lo, m, v, &q);
    if (sign) {
        while (s.live) ampli_ai_step(&s);
        q = ampli_ai_q_from_p(s.res, sign);
    }
    if (terms) *terms = s.terms;
    return q;
}

// what a tested cell adds to DEV16 and Q20 of a region
AMPLI_FN int64_t ampli_ai_dev16(int64_t k_lo, int64_t m, double v)
{
    const double e = v * (double)m;
    const double d = (double)k_lo - e;
    return (int64_t)llrint(fabs(d) * 16.0);
}
AMPLI_FN int64_t ampli_ai_q20(float q) { return (int64_t)llrint((double)fabsf(q) * 1048576.0); }

// The verdict of a region from its five sums (AMPLI_AI_SITES ..): Fisher's combination of the sites' two-sided p-values, chi-square
// with 2 SITES degrees of freedom through the project's kf_gammaq, and the pooled deviation of the share.  *Q and *imbalance are NaN
// where they do not exist (FEW; no depth).
AMPLI_FN int ampli_ai_region_verdict(const int64_t *sums, int64_t min_sites, double q_min, double min_imbalance, double *Q, double *imbalance)
{
    const int64_t sites = sums[AMPLI_AI_SITES], depth = sums[AMPLI_AI_DEPTH];
    *Q = (double)NAN;
    *imbalance = depth > 0 ? (double)sums[AMPLI_AI_DEV16] / (16.0 * (double)depth) : (double)NAN;
    if (sites < min_sites || sites < 1) return AMPLI_AI_FEW;
    const double X = (2.302585092994046 / 5.0) * ((double)sums[AMPLI_AI_Q20] / 1048576.0);
    const double p = ampli_kf_gammaq((double)sites, X / 2.0);
    *Q = p >= 1.0 ? 0.0 : (p > 1e-30 ? -10.0 * log10(p) : 300.0);
    return (*Q >= q_min && *imbalance >= min_imbalance) ? AMPLI_AI_IMBALANCED : AMPLI_AI_BALANCED;
}

// the tumour fraction an imbalance would imply: under copy-neutral LOH the share moves by f / 2, under the loss of one copy by
// f / (2 (2 - f)) -- so f = 2 i and f = 4 i / (1 + 2 i)
AMPLI_FN double ampli_ai_fraction_cnloh(double imbalance) { return 2.0 * imbalance; }
AMPLI_FN double ampli_ai_fraction_loss(double imbalance) { return 4.0 * imbalance / (1.0 + 2.0 * imbalance); }

// ------------------------------------------------------------------------------------------------------------------------------------
// Tumour fraction per (sample, list) (the definition is tests/fraction_model.py): how much of a patient's tumour is in this
// plasma sample, within what bounds.
//   Lists.  The CSR of monitoring (list_off, list_cell, an entry c = 4 p + y) and list_w float32 [W], the weight a of every entry: the
//     variant's allele fraction per unit of tumour fraction.  An entry with p >= P is none; a cell listed twice counts twice.
//   Evaluated entry of a row: monitoring's rule (ampli_mon_entry_ok, ampli_mon_record_ok; e == 0 replaced by 0.0010008f), and a weight
//     that is finite, > 0 and <= 1 (ampli_tf_weight_ok).  It gives two cells, fw then bw, each with k, d, e as doubles, a = (double)w and
//     ad = a * d.  A cell is modelled as a Poisson count of mean d (e + f a).
//   Score and information at f, per cell: r = e + f * a; g = a / r; U += g * k - ad; I += g * ad -- seven IEEE operations, unfused.  Lane
//     j of 64 takes entries j, j + 64, ... ascending, fw before bw, into two accumulators that start at +0.0 (an entry that is not
//     evaluated adds nothing); the 64 pairs are combined by x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1.  T(f) = U * |U| / I.
//   N_EVAL == 0 or I(0) <= 0 makes all four values AMPLI_TF_NA.  Otherwise, every bisection AMPLI_TF_ITERS steps of mid = 0.5 * (lo + hi)
//   and the result 0.5 * (lo + hi):
//     F_HAT: 0 if U(0) <= 0; 1 if U(1) >= 0; else on [0, 1], U(mid) > 0 ? lo = mid : hi = mid.
//     F_LO:  0 if T(0) <= z2; else on [0, F_HAT], T(mid) > z2 ? lo = mid : hi = mid.  T need not be monotone there in contrived lists:
//            the bisection's result is the definition.
//     F_HI:  0 if F_HAT == 0 and -T(0) >= z2; 1 if -T(1) < z2; else on [F_HAT, 1], -T(mid) < z2 ? lo = mid : hi = mid.
//     T0 = T(0).
//   At most 2 + 3 AMPLI_TF_ITERS = 182 evaluations of the sums.  r > 0 always (e > 0, f >= 0, a > 0), so no quotient is a NaN.
// ------------------------------------------------------------------------------------------------------------------------------------
AMPLI_FN int ampli_tf_weight_ok(float w) { return w > 0.0f && w <= 1.0f; } // a NaN, an infinity, 0 and a negative value fail

// what one cell (k reads of the listed base among a depth with a d = ad, threshold e, weight a) adds to the score U and the information I at f
AMPLI_FN void ampli_tf_cell_terms(double f, double k, double ad, double a, double e, double *U, double *I)
{
    const double fa = f * a;
    const double r = e + fa;
    const double g = a / r;
    const double gk = g * k;
    *U = *U + (gk - ad);
    *I = *I + g * ad;
}

AMPLI_FN double ampli_tf_T(double U, double I) { return U * fabs(U) / I; }

#ifdef __cplusplus
// The estimate and its interval over `sum_at(f, &U, &I)`, which gives the two combined sums at f.  The host library's twin and the
// kernel run this text; on the device every lane of a wave holds the same sums, so every branch is wave-uniform.
template <class SumAt>
AMPLI_FN void ampli_tf_solve(SumAt sum_at, int64_t n_eval, double z2, double *out /* [AMPLI_TF_VALS] */)
{
    out[AMPLI_TF_F_HAT] = out[AMPLI_TF_F_LO] = out[AMPLI_TF_F_HI] = out[AMPLI_TF_T0] = AMPLI_TF_NA;
    if (n_eval <= 0) return;
    double U0, I0, U, I;
    sum_at(0.0, &U0, &I0);
    if (!(I0 > 0.0)) return;
    const double T0 = ampli_tf_T(U0, I0);
    double U1, I1;
    sum_at(1.0, &U1, &I1);
    double fh;
    if (U0 <= 0.0) fh = 0.0;
    else if (U1 >= 0.0) fh = 1.0;
    else {
        double lo = 0.0, hi = 1.0;
        for (int i = 0; i < AMPLI_TF_ITERS; ++i) {
            const double mid = 0.5 * (lo + hi);
            sum_at(mid, &U, &I);
            if (U > 0.0) lo = mid; else hi = mid;
        }
        fh = 0.5 * (lo + hi);
    }
    double fl = 0.0;
    if (T0 > z2) {
        double lo = 0.0, hi = fh;
        for (int i = 0; i < AMPLI_TF_ITERS; ++i) {
            const double mid = 0.5 * (lo + hi);
            sum_at(mid, &U, &I);
            if (ampli_tf_T(U, I) > z2) lo = mid; else hi = mid;
        }
        fl = 0.5 * (lo + hi);
    }
    double fu;
    if (fh == 0.0 && -T0 >= z2) fu = 0.0;
    else if (-ampli_tf_T(U1, I1) < z2) fu = 1.0;
    else {
        double lo = fh, hi = 1.0;
        for (int i = 0; i < AMPLI_TF_ITERS; ++i) {
            const double mid = 0.5 * (lo + hi);
            sum_at(mid, &U, &I);
            if (-ampli_tf_T(U, I) < z2) lo = mid; else hi = mid;
        }
        fu = 0.5 * (lo + hi);
    }
    out[AMPLI_TF_F_HAT] = fh;
    out[AMPLI_TF_F_LO] = fl;
    out[AMPLI_TF_F_HI] = fu;
    out[AMPLI_TF_T0] = T0;
}
#endif

// NOT_EVALUABLE below min_variants evaluated entries (and where nothing could be estimated); QUANTIFIED if the lower end is above zero;
// else BELOW, and F_HI is the reportable upper bound
AMPLI_FN int ampli_tf_verdict(int64_t n_eval, double f_hat, double f_lo, int64_t min_variants)
{
    if (n_eval < min_variants || f_hat < 0.0) return AMPLI_TF_NOT_EVALUABLE;
    return f_lo > 0.0 ? AMPLI_TF_QUANTIFIED : AMPLI_TF_BELOW;
}

// the change from draw A to draw B of one list, from the draws' verdicts and values; *ratio = F_HAT_B / F_HAT_A, AMPLI_TF_NA where
// either draw is not evaluable or F_HAT_A is zero
AMPLI_FN int ampli_tf_change(int verdict_a, const double *a, int verdict_b, const double *b, double *ratio)
{
    *ratio = AMPLI_TF_NA;
    if (verdict_a == AMPLI_TF_NOT_EVALUABLE || verdict_b == AMPLI_TF_NOT_EVALUABLE) return AMPLI_TF_CHANGE_NOT_EVALUABLE;
    if (a[AMPLI_TF_F_HAT] > 0.0) *ratio = b[AMPLI_TF_F_HAT] / a[AMPLI_TF_F_HAT];
    if (b[AMPLI_TF_F_LO] > a[AMPLI_TF_F_HI]) return AMPLI_TF_RISING;
    if (b[AMPLI_TF_F_HI] < a[AMPLI_TF_F_LO]) return AMPLI_TF_FALLING;
    return AMPLI_TF_STABLE;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Read-level evidence (the definition is the contract comment of ampli_evidence_score, restated in tests/evidence_model.py): do
// the reads that carry the alt allele at a position rank below the reads that carry the ref allele, in base quality, MAPQ or distance to
// the read's end.  One cell per (position, metric) over two 64-bin histograms a (alt) and r (ref); a side without a usable nt is NULL and
// reads as zeros.
//   n1 = sum a, n2 = sum r, N = n1 + n2, t_b = a_b + r_b.  Medians: the smallest b with 2 cum_b >= n, -1 for n = 0.
//   U2 = sum_b a_b (2 R_<b + r_b): twice the Mann-Whitney U of alt over ref, ties counted half.  D = U2 - n1 n2.
//   Td = sum_b ascending (t t t - t), Nd = N, c = (Nd + 1) - Td / (Nd (Nd - 1)), v = n1 n2 c, z2 = 3 D D / v, negated for D < 0: every
//   operation one IEEE operation in this order (the build contracts nothing), so device, host and the numpy model agree bit for bit.
//   Untested (u2 = -1, z2 = 0; counts and medians still written): n1 = 0, n2 = 0, N >= 2^30 (keeps U2 < 2^63), !(v > 0).
// ------------------------------------------------------------------------------------------------------------------------------------
// the alt nt a position is scored with, or -1: `alt` itself when it is 0 .. 3 and not `ref`; for alt == -1 ("choose") the nt other than
// ref with the largest total over the BQ bins, ties to the lowest index; -1 for a ref outside 0 .. 3 and for any other alt
AMPLI_FN int ampli_ev_alt(const int32_t *hist /* [4][METRICS][BINS] of one position */, int ref, int alt)
{
    if (ref < 0 || ref > 3) return -1;
    if (alt != -1) return (alt < 0 || alt > 3 || alt == ref) ? -1 : alt;
    int best = -1;
    int64_t best_n = 0;
    for (int nt = 0; nt < 4; ++nt) {
        if (nt == ref) continue;
        const int32_t *h = hist + (nt * AMPLI_EVIDENCE_METRICS + AMPLI_EVIDENCE_BQ) * AMPLI_EVIDENCE_BINS;
        int64_t n = 0;
        for (int b = 0; b < AMPLI_EVIDENCE_BINS; ++b) n += h[b];
        if (best < 0 || n > best_n) { best = nt; best_n = n; }
    }
    return best;
}

// one cell: o_int = {n_ref, n_alt, u2}, o_med = {med_ref, med_alt}, *o_z2 the signed squared score
AMPLI_FN void ampli_ev_cell(const int32_t *a, const int32_t *r, int64_t *o_int, int32_t *o_med, double *o_z2)
{
    int64_t n1 = 0, n2 = 0;
    for (int b = 0; b < AMPLI_EVIDENCE_BINS; ++b) {
        n1 += a ? a[b] : 0;
        n2 += r ? r[b] : 0;
    }
    const int64_t N = n1 + n2;
    int64_t c1 = 0, c2 = 0; // alt and ref reads in the bins up to b; c2 before its update is R_<b
    int32_t m1 = -1, m2 = -1;
    uint64_t u2 = 0; // wraps only where the cell is untested (N >= 2^30)
    double Td = 0.0;
    for (int b = 0; b < AMPLI_EVIDENCE_BINS; ++b) {
        const int64_t ab = a ? a[b] : 0, rb = r ? r[b] : 0;
        u2 += (uint64_t)ab * (uint64_t)(2 * c2 + rb);
        c1 += ab;
        c2 += rb;
        if (m1 < 0 && n1 > 0 && 2 * c1 >= n1) m1 = b;
        if (m2 < 0 && n2 > 0 && 2 * c2 >= n2) m2 = b;
        const double t = (double)(ab + rb);
        const double t3 = t * t * t;
        Td = Td + (t3 - t);
    }
    o_int[0] = n2;
    o_int[1] = n1;
    o_int[2] = -1;
    o_med[0] = m2;
    o_med[1] = m1;
    *o_z2 = 0.0;
    if (n1 <= 0 || n2 <= 0 || N >= (1ll << 30)) return;
    const double Nd = (double)N;
    const double c = (Nd + 1.0) - Td / (Nd * (Nd - 1.0));
    const double v = (double)n1 * (double)n2 * c;
    if (!(v > 0.0)) return;
    const int64_t D = (int64_t)u2 - n1 * n2;
    const double z2 = 3.0 * (double)D * (double)D / v;
    o_int[2] = (int64_t)u2;
    *o_z2 = D < 0 ? -z2 : z2;
}

// ---------------------------------------------------------------------------
// Read-level phasing (the definition is the contract comment of ampli_phase_score, restated in tests/phase_model.py): do two
// listed variants share their reads?  One pair = one 5 x 5 cell of ampli_pileup_phase's joint table, rows the state at key i, columns the
// state at key j.  The four corners (ref / alt at i) x (ref / alt at j) are the 2 x 2 table of the exact test above: the score is
// ampli_pair_score(n_aa, n_aa + n_ar, n_ra, n_ra + n_rr), positive when alt at j is commoner among the reads that show alt at i.
// ---------------------------------------------------------------------------
// is the pair tested?  pair_cell = i K + k inside [0, P K) with i + 1 + k < P; four nts in 0 .. 3; ref != alt on both sides
AMPLI_FN int ampli_ph_tested(int64_t pair_cell, int64_t P, int ref_i, int alt_i, int ref_j, int alt_j)
{
    if (pair_cell < 0 || pair_cell >= P * AMPLI_PHASE_PARTNERS) return 0;
    const int64_t i = pair_cell / AMPLI_PHASE_PARTNERS, k = pair_cell - i * AMPLI_PHASE_PARTNERS;
    if (i + 1 + k >= P) return 0;
    if ((unsigned)ref_i > 3u || (unsigned)alt_i > 3u || (unsigned)ref_j > 3u || (unsigned)alt_j > 3u) return 0;
    return ref_i != alt_i && ref_j != alt_j;
}

// the six counts of a tested pair's cell [5][5]: rr, ra, ar, aa (the first letter is the state at key i), joint, other
AMPLI_FN void ampli_ph_counts(const int32_t *cell, int ref_i, int alt_i, int ref_j, int alt_j, int64_t *v)
{
    int64_t joint = 0;
    for (int c = 0; c < AMPLI_PHASE_STATES * AMPLI_PHASE_STATES; ++c) joint += cell[c];
    v[0] = cell[ref_i * AMPLI_PHASE_STATES + ref_j];
    v[1] = cell[ref_i * AMPLI_PHASE_STATES + alt_j];
    v[2] = cell[alt_i * AMPLI_PHASE_STATES + ref_j];
    v[3] = cell[alt_i * AMPLI_PHASE_STATES + alt_j];
    v[4] = joint;
    v[5] = joint - (v[0] + v[1] + v[2] + v[3]);
}

// the class: bit 0 = aa, bit 1 = ar, bit 2 = ra present.  A group x is present iff x >= min_alt and 100 x >= min_share m, m the reads
// that show an alt at either key; compared in int64
AMPLI_FN int32_t ampli_ph_class(int64_t n_ra, int64_t n_ar, int64_t n_aa, int32_t min_alt, int32_t min_share)
{
    const int64_t m = n_aa + n_ar + n_ra;
    const int aa = n_aa >= min_alt && 100 * n_aa >= (int64_t)min_share * m;
    const int ar = n_ar >= min_alt && 100 * n_ar >= (int64_t)min_share * m;
    const int ra = n_ra >= min_alt && 100 * n_ra >= (int64_t)min_share * m;
    return (int32_t)(aa | (ar << 1) | (ra << 2));
}

// the whole of one pair (host, tests): v [6], the score, the class.  An untested pair: six -1, score 0, class -1
AMPLI_FN void ampli_ph_cell(const int32_t *table, int64_t P, int64_t pair_cell, const int8_t *nt, int32_t min_alt, int32_t min_share, int64_t *v, float *score,
                            int32_t *cls)
{
    if (!ampli_ph_tested(pair_cell, P, nt[0], nt[1], nt[2], nt[3])) {
        for (int c = 0; c < 6; ++c) v[c] = -1;
        *score = 0.0f;
        *cls = -1;
        return;
    }
    ampli_ph_counts(table + pair_cell * (AMPLI_PHASE_STATES * AMPLI_PHASE_STATES), nt[0], nt[1], nt[2], nt[3], v);
    *score = ampli_pair_score(v[3], v[3] + v[2], v[1], v[1] + v[0], (int32_t *)0);
    *cls = ampli_ph_class(v[1], v[2], v[3], min_alt, min_share);
}

#endif
