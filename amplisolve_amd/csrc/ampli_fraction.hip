// amplisolve_amd/csrc/ampli_fraction.hip -- tumour fraction per (sample, list): the score estimate of how much of a
// patient's tumour a plasma sample holds, and its Rao score interval.
//
// fraction_kernel (ampli_fraction_records) gathers the primary records of every sample of a resident chunk along the cells of every
// weighted list, and finds F_HAT, F_LO and F_HI by bisection over the summed score U(f) and information I(f) (ampli_tf_solve,
// csrc/ampli_math.h: the text the host library runs).  The definition is tests/fraction_model.py; the doubles agree with the host
// library and the model bit for bit: every operation is an IEEE + - * / in a fixed order (unfused, -ffp-contract=off; a double
// division is the correctly rounded v_div_scale / v_rcp / v_fma / v_div_fmas / v_div_fixup sequence).
//
// The small helpers of the gather (the bounds of a list, the entry of a cell, the count of a lane's own base) restate those of
// ampli_monitor.hip, which stay where they are: that file's kernels are not touched by this one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

constexpr int TF_WAVES = 4;      // waves per workgroup: each owns its own work, nothing is shared between them
constexpr int TF_STRIP = 8;      // consecutive rows (samples) one wave estimates for its list
constexpr int TF_REG_ROUNDS = 4; // lists of up to 4 x 64 entries keep their entries and the row's cells in registers
// Two kernels share a launch's lists by their length, each list in exactly one: ROUNDS = 1 takes the lists of up to 64 entries -- the
// everyday case, in about half the registers of the other, so that twice as many waves hide each other's butterflies and divisions --,
// ROUNDS = TF_REG_ROUNDS the longer ones.  A wave of the kernel that does not take its list reads the list's bounds and ends.

// the count of base y, for a y that differs from lane to lane, as a chain of selects over the four counts by value (no array: one
// would be kept in scratch or LDS)
__device__ __forceinline__ int tf_pick(const int a, const int c, const int g, const int t, const unsigned y)
{
    int k = a;
    k = y == 1u ? c : k;
    k = y == 2u ? g : k;
    k = y == 3u ? t : k;
    return k;
}

// the butterfly of the definition: x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1 (an IEEE addition is commutative, so every lane ends
// with the same bits); the result is then read from the first lane into scalar registers, which tells the compiler what the butterfly
// guarantees -- every branch of the bisection on it is a scalar branch
__device__ __forceinline__ double tf_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    const long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the bounds of list l, cut to [0, W]: whatever list_off holds, no entry at or beyond W is addressed
__device__ __forceinline__ void tf_bounds(const unsigned *__restrict__ list_off, const long long l, const unsigned W, unsigned &off, unsigned &end)
{
    const unsigned off_ = list_off[l], end_ = list_off[l + 1];
    off = off_ < W ? off_ : W;
    end = end_ < off ? off : (end_ < W ? end_ : W);
}

// one entry of a list as its lane holds it: the position, the base, the weight and the two thresholds as the doubles of the definition
// (a zero threshold already replaced), and whether it can be evaluated in any sample
struct TfEnt {
    unsigned p, y;
    double a, ef, eb;
    bool on;
};

__device__ __forceinline__ TfEnt tf_none()
{
    TfEnt t;
    t.p = t.y = 0u;
    t.a = t.ef = t.eb = 0.0;
    t.on = false;
    return t;
}

// the entry of cell c with weight w; the thresholds are read only for a position below P with a reference base
__device__ __forceinline__ TfEnt tf_entry(const unsigned c, const float w, const long long P, const float *__restrict__ thr,
                                          const unsigned char *__restrict__ ref_code)
{
    TfEnt t = tf_none();
    t.p = c >> 2;
    t.y = c & 3u;
    if ((long long)t.p >= P) return t;
    const unsigned ref = ref_code[t.p];
    if (ref > 3u) return t;
    float ef = thr[(size_t)t.y * (size_t)P + (size_t)t.p];
    float eb = thr[(size_t)(4u + t.y) * (size_t)P + (size_t)t.p];
    t.on = ampli_mon_entry_ok(ref, t.y, ef, eb) != 0 && ampli_tf_weight_ok(w) != 0;
    if (ef == 0.0f) ef = 0.0010008f;
    if (eb == 0.0f) eb = 0.0010008f;
    t.a = (double)w;
    t.ef = (double)ef;
    t.eb = (double)eb;
    return t;
}

// what the record of one entry gives: whether the entry is evaluated in this row, and then k and a d of both strands
struct TfCell {
    double kf, kb, adf, adb;
    bool ok, seen;
};

template <int LAY>
__device__ __forceinline__ TfCell tf_cell(const RawRec<LAY> &raw, const TfEnt &t, const int cov, const int vaf)
{
    int4 f, r;
    rec_decode<LAY>(raw, f, r);
    // a depth is below 2^27 with the 16- and 24-bit layouts, below 2^34 with int32 records: exact as a double
    const long long FW = (long long)f.x + (long long)f.y + (long long)f.z + (long long)f.w;
    const long long BW = (long long)r.x + (long long)r.y + (long long)r.z + (long long)r.w;
    const long long kf = tf_pick(f.x, f.y, f.z, f.w, t.y), kb = tf_pick(r.x, r.y, r.z, r.w, t.y);
    TfCell c;
    c.ok = t.on && ampli_mon_record_ok(f.x != AMPLI_ABSENT, kf, kb, FW, BW, cov, vaf) != 0;
    c.seen = c.ok && kf + kb >= 1;
    c.kf = (double)kf;
    c.kb = (double)kb;
    c.adf = t.a * (double)FW;
    c.adb = t.a * (double)BW;
    return c;
}

__device__ __forceinline__ void tf_store(double *__restrict__ o, long long *__restrict__ oc, const double *v, const long long n_eval, const long long n_seen,
                                         const int lane)
{
    if (lane == 0) {
        o[AMPLI_TF_F_HAT] = v[AMPLI_TF_F_HAT];
        o[AMPLI_TF_F_LO] = v[AMPLI_TF_F_LO];
        o[AMPLI_TF_F_HI] = v[AMPLI_TF_F_HI];
        o[AMPLI_TF_T0] = v[AMPLI_TF_T0];
        oc[AMPLI_TF_N_EVAL] = n_eval;
        oc[AMPLI_TF_N_SEEN] = n_seen;
    }
}

// fraction_kernel<LAY, ROUNDS>: blockIdx.x = list l, (blockIdx.y, wave) = strip of TF_STRIP consecutive rows.  The wave reads its list's
// bounds, ends if the list is the other kernel's, then
//   * a list of up to ROUNDS * 64 entries: lane i holds entry 64 k + i of round k -- the cell, the weight and the two thresholds
//     as doubles -- in registers, loaded ONCE per wave; per row it loads the records at those positions and keeps k and a d of both
//     strands.  An evaluation of the sums at f is then arithmetic on registers: one division per cell, and the butterfly of two doubles.
//     A round in which no lane holds an evaluated entry is skipped by the wave (a list of 32 entries runs one round);
//   * a longer list (any length; ROUNDS = TF_REG_ROUNDS only): every evaluation walks the list in rounds of 64, each lane reloading its
//     entry and its record -- up to 182 gathers of the list per row.  Correct and slow: such a list is far from the use the command is
//     made for.
// Lane i takes entries i, i + 64, ... in ascending order, fw before bw, in both forms: the order of the definition.  Lane 0 stores the
// four doubles and the two counts.  No LDS, no barrier, no atomics: every cell has one owner and is stored once.
template <int LAY, int ROUNDS>
__global__ __launch_bounds__(64 * TF_WAVES) void fraction_kernel(const RecView rv, const long long P, const int n, const int L, const float *__restrict__ thr,
                                                                   const unsigned char *__restrict__ ref_code, const unsigned *__restrict__ list_off,
                                                                   const unsigned *__restrict__ list_cell, const float *__restrict__ list_w, const unsigned W,
                                                                   const int cov, const int vaf, const double z2, double *__restrict__ est,
                                                                   long long *__restrict__ count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long l = blockIdx.x;
    const long long row0 = ((long long)blockIdx.y * TF_WAVES + wave) * TF_STRIP;
    if (row0 >= n) return;
    const long long row1 = row0 + TF_STRIP < n ? row0 + TF_STRIP : n;
    unsigned off, end;
    tf_bounds(list_off, l, W, off, end);
    const unsigned len = end - off;
    if (ROUNDS == 1 ? len > 64u : len <= 64u) return; // the other kernel's list
    const size_t rb = rec_bytes(LAY);
    const size_t stride = (size_t)rv.row_stride * rb;
    double *__restrict__ o = est + ((size_t)row0 * (size_t)L + (size_t)l) * AMPLI_TF_VALS;
    long long *__restrict__ oc = count + ((size_t)row0 * (size_t)L + (size_t)l) * AMPLI_TF_COUNTS;

    if (len <= ROUNDS * 64) {
        TfEnt ent[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const unsigned e = off + 64u * k + lane;
            ent[k] = tf_none();
            if (e < end) ent[k] = tf_entry(list_cell[e], list_w[e], P, thr, ref_code);
        }
        for (long long row = row0; row < row1; ++row, o += (size_t)L * AMPLI_TF_VALS, oc += (size_t)L * AMPLI_TF_COUNTS) {
            const char *__restrict__ q = rv.base + (size_t)row * stride;
            TfCell cell[ROUNDS];
            long long n_eval = 0, n_seen = 0;
#pragma unroll
            for (int k = 0; k < ROUNDS; ++k) {
                RawRec<LAY> raw = {};
                if (ent[k].on) raw = rec_load_at<LAY>(q + (size_t)ent[k].p * rb);
                cell[k] = tf_cell<LAY>(raw, ent[k], cov, vaf);
                n_eval += __popcll(__ballot(cell[k].ok));
                n_seen += __popcll(__ballot(cell[k].seen));
            }
            auto sum_at = [&](const double f, double *U, double *I) {
                double u = 0.0, i = 0.0;
#pragma unroll
                for (int k = 0; k < ROUNDS; ++k)
                    if (cell[k].ok) {
                        ampli_tf_cell_terms(f, cell[k].kf, cell[k].adf, ent[k].a, ent[k].ef, &u, &i);
                        ampli_tf_cell_terms(f, cell[k].kb, cell[k].adb, ent[k].a, ent[k].eb, &u, &i);
                    }
                *U = tf_wave_sum(u);
                *I = tf_wave_sum(i);
            };
            double v[AMPLI_TF_VALS];
            ampli_tf_solve(sum_at, n_eval, z2, v);
            tf_store(o, oc, v, n_eval, n_seen, lane);
        }
        return;
    }
    if (ROUNDS == 1) return; // not reached: this kernel's lists fit its registers
    for (long long row = row0; row < row1; ++row, o += (size_t)L * AMPLI_TF_VALS, oc += (size_t)L * AMPLI_TF_COUNTS) {
        const char *__restrict__ q = rv.base + (size_t)row * stride;
        long long n_eval = 0, n_seen = 0;
        // one walk of the list: the counts where `counting`, the sums at f in any case
        auto walk = [&](const double f, double *U, double *I, const bool counting) {
            double u = 0.0, i = 0.0;
            for (unsigned e0 = off; e0 < end; e0 += 64u) { // e0 + lane cannot wrap: end <= W < 2^28
                const unsigned e = e0 + lane;
                TfEnt t = tf_none();
                if (e < end) t = tf_entry(list_cell[e], list_w[e], P, thr, ref_code);
                RawRec<LAY> raw = {};
                if (t.on) raw = rec_load_at<LAY>(q + (size_t)t.p * rb);
                const TfCell c = tf_cell<LAY>(raw, t, cov, vaf);
                if (counting) {
                    n_eval += __popcll(__ballot(c.ok));
                    n_seen += __popcll(__ballot(c.seen));
                }
                if (c.ok) {
                    ampli_tf_cell_terms(f, c.kf, c.adf, t.a, t.ef, &u, &i);
                    ampli_tf_cell_terms(f, c.kb, c.adb, t.a, t.eb, &u, &i);
                }
            }
            *U = tf_wave_sum(u);
            *I = tf_wave_sum(i);
        };
        double U, I;
        walk(0.0, &U, &I, true); // the counts; ampli_tf_solve asks for the sums at 0 again
        auto sum_at = [&](const double f, double *U_, double *I_) { walk(f, U_, I_, false); };
        double v[AMPLI_TF_VALS];
        ampli_tf_solve(sum_at, n_eval, z2, v);
        tf_store(o, oc, v, n_eval, n_seen, lane);
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_fraction_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                      const uint32_t *d_list_off, const uint32_t *d_list_cell, const float *d_list_w, int32_t L, int64_t W,
                                      const ampli_fraction_params *prm, double *d_est, int64_t *d_count)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || L < 0 || W < 0 || !d_thr || !d_ref_code || !d_list_off || !d_list_cell || !d_list_w || !prm || !d_est || !d_count ||
        (((uintptr_t)d_est | (uintptr_t)d_count) & 7) != 0 || (((uintptr_t)d_thr | (uintptr_t)d_list_off | (uintptr_t)d_list_cell | (uintptr_t)d_list_w) & 3) != 0 ||
        prm->coverage_cutoff < 0 || prm->max_vaf_pm < 0 || prm->max_vaf_pm > 1000 || !std::isfinite(prm->z2) || !(prm->z2 > 0.0))
        return fail(ctx, AMPLI_E_INVALID,
                    "fraction_records: bad argument (P > 0, L >= 0, W >= 0, coverage_cutoff >= 0, max_vaf_pm in 0..1000, z2 finite and > 0, 4-byte aligned "
                    "d_thr, d_list_off, d_list_cell and d_list_w, d_ref_code, 8-byte aligned d_est and d_count)");
    { int rc = check_records(ctx, co, "fraction_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "fraction_records: P must be below 2^31");
    if (W >= (1ll << 28)) return fail(ctx, AMPLI_E_RANGE, "fraction_records: W must be below 2^28");
    const long long strips = ((long long)co.n + TF_WAVES * TF_STRIP - 1) / (TF_WAVES * TF_STRIP);
    if (strips > 65535) return fail(ctx, AMPLI_E_RANGE, "fraction_records: n_samples must be at most 2097120");
    if (L == 0) return AMPLI_OK; // no list: both outputs are empty
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const dim3 grid((unsigned)L, (unsigned)strips);
    with_layout(co.layout, [&](auto LAY) {
        hipLaunchKernelGGL((fraction_kernel<LAY, 1>), grid, dim3(64 * TF_WAVES), 0, st, co.rv, (long long)P, co.n, (int)L, d_thr, (const unsigned char *)d_ref_code,
                           (const unsigned *)d_list_off, (const unsigned *)d_list_cell, d_list_w, (unsigned)W, (int)prm->coverage_cutoff, (int)prm->max_vaf_pm,
                           (double)prm->z2, d_est, (long long *)d_count);
        hipLaunchKernelGGL((fraction_kernel<LAY, TF_REG_ROUNDS>), grid, dim3(64 * TF_WAVES), 0, st, co.rv, (long long)P, co.n, (int)L, d_thr,
                           (const unsigned char *)d_ref_code, (const unsigned *)d_list_off, (const unsigned *)d_list_cell, d_list_w, (unsigned)W,
                           (int)prm->coverage_cutoff, (int)prm->max_vaf_pm, (double)prm->z2, d_est, (long long *)d_count);
    });
    return check_launch(ctx, "fraction_kernel");
}
