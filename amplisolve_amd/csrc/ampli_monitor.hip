// amplisolve_amd/csrc/ampli_monitor.hip -- tumour-informed monitoring: pooled evidence over the cells of variant lists.
//
// monitor_sums_kernel (ampli_monitor_sums_records) gathers the primary records of every sample of a resident chunk along the cells of
// every list into six int64 sums and the two expected counts Lambda per (sample, list).  monitor_control_kernel
// (ampli_monitor_control_records) does the same for matched random lists: every entry moved to a drawn position of the same reference
// base.  monitor_score_kernel (ampli_monitor_score) turns the sums into the pooled Poisson score of each strand.  The definition is
// tests/monitor_model.py; the integers, the doubles and the scores agree with the host library bit for bit (the order of every double
// addition is part of the definition; unfused, -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long mo_u64;

constexpr int MO_WAVES = 4;      // waves per workgroup: each owns its own work, nothing is shared between them
constexpr int MO_STRIP = 8;      // consecutive rows (samples) one wave sums for its list (AMPLI_MON_STRIP)
constexpr int MO_REG_ROUNDS = 4; // lists of up to 4 x 64 entries keep their cells and thresholds in registers; longer ones reload them
static_assert(MO_STRIP == AMPLI_MON_STRIP, "the header documents the strip");

// a lane's share of one (row, list): evaluated | seen << 32 in one word (both stay below 2^28, W < 2^28), the alternative reads and the
// depths of the strands (modular 64-bit additions: the int64 sums exactly), and the two expected counts
struct MoAcc {
    mo_u64 ns, kf, kb, df, db;
    double lf, lb;
};

__device__ __forceinline__ MoAcc mo_zero()
{
    MoAcc s;
    s.ns = s.kf = s.kb = s.df = s.db = 0ull;
    s.lf = s.lb = 0.0;
    return s;
}

// the count of base y, for a y that differs from lane to lane, as a chain of selects over the four counts BY VALUE: no array, and no
// reference to the decoded int4 -- with one the compiler kept the two vectors of every lane in LDS (16 KB per workgroup)
__device__ __forceinline__ int mo_pick(const int a, const int c, const int g, const int t, const unsigned y)
{
    int k = a;
    k = y == 1u ? c : k;
    k = y == 2u ? g : k;
    k = y == 3u ? t : k;
    return k;
}

// what the record of one entry adds; `on`: the entry exists and passed ampli_mon_entry_ok.  An entry that is not evaluated leaves
// every accumulator as it is (the doubles too: nothing is added, not even +0.0).
template <int LAY>
__device__ __forceinline__ void mo_add(MoAcc &s, const RawRec<LAY> &raw, const bool on, const unsigned y, const float ef, const float eb,
                                       const int cov, const int vaf)
{
    int4 f, r;
    rec_decode<LAY>(raw, f, r);
    // a depth is below 2^27 with the 16- and 24-bit layouts, below 2^34 with int32 records
    const long long FW = (long long)f.x + (long long)f.y + (long long)f.z + (long long)f.w;
    const long long BW = (long long)r.x + (long long)r.y + (long long)r.z + (long long)r.w;
    const long long kf = mo_pick(f.x, f.y, f.z, f.w, y), kb = mo_pick(r.x, r.y, r.z, r.w, y);
    const bool ok = on && ampli_mon_record_ok(f.x != AMPLI_ABSENT, kf, kb, FW, BW, cov, vaf) != 0;
    s.ns += ok ? 1ull + (kf + kb >= 1 ? 1ull << 32 : 0ull) : 0ull;
    s.kf += ok ? (mo_u64)kf : 0ull;
    s.kb += ok ? (mo_u64)kb : 0ull;
    s.df += ok ? (mo_u64)FW : 0ull;
    s.db += ok ? (mo_u64)BW : 0ull;
    const double tf = ampli_mon_lambda_term(FW, ef), tb = ampli_mon_lambda_term(BW, eb);
    s.lf = ok ? s.lf + tf : s.lf;
    s.lb = ok ? s.lb + tb : s.lb;
}

__device__ __forceinline__ mo_u64 mo_wave_sum(mo_u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (mo_u64)__shfl_xor((long long)v, d);
    return v;
}

// the butterfly of the definition: x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1 (an IEEE addition is commutative, so every lane ends
// with the same bits)
__device__ __forceinline__ double mo_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void mo_store(long long *__restrict__ o, double *__restrict__ ol, const MoAcc &s, const int lane)
{
    const mo_u64 ns = mo_wave_sum(s.ns), kf = mo_wave_sum(s.kf), kb = mo_wave_sum(s.kb), df = mo_wave_sum(s.df), db = mo_wave_sum(s.db);
    const double lf = mo_wave_sum(s.lf), lb = mo_wave_sum(s.lb);
    if (lane == 0) {
        o[AMPLI_MON_N_EVAL] = (long long)(ns & 0xFFFFFFFFull);
        o[AMPLI_MON_N_SEEN] = (long long)(ns >> 32);
        o[AMPLI_MON_K_FW] = (long long)kf;
        o[AMPLI_MON_K_BW] = (long long)kb;
        o[AMPLI_MON_D_FW] = (long long)df;
        o[AMPLI_MON_D_BW] = (long long)db;
        ol[0] = lf;
        ol[1] = lb;
    }
}

// the bounds of list l, cut to [0, W]: whatever list_off holds, no entry at or beyond W is addressed
__device__ __forceinline__ void mo_bounds(const unsigned *__restrict__ list_off, const long long l, const unsigned W, unsigned &off, unsigned &end)
{
    const unsigned off_ = list_off[l], end_ = list_off[l + 1];
    off = off_ < W ? off_ : W;
    end = end_ < off ? off : (end_ < W ? end_ : W);
}

// one entry of a list as its lane holds it: the position, the base, the two thresholds, and whether it can be evaluated in any sample
struct MoEnt {
    unsigned p, y;
    float ef, eb;
    bool on;
};

__device__ __forceinline__ MoEnt mo_none()
{
    MoEnt t;
    t.p = t.y = 0u;
    t.ef = t.eb = 0.0f;
    t.on = false;
    return t;
}

// the entry of cell c; the thresholds are read only for a position below P with a reference base
__device__ __forceinline__ MoEnt mo_entry(const unsigned c, const long long P, const float *__restrict__ thr, const unsigned char *__restrict__ ref_code)
{
    MoEnt t = mo_none();
    t.p = c >> 2;
    t.y = c & 3u;
    if ((long long)t.p >= P) return t;
    const unsigned ref = ref_code[t.p];
    if (ref > 3u) return t;
    t.ef = thr[(size_t)t.y * (size_t)P + (size_t)t.p];
    t.eb = thr[(size_t)(4u + t.y) * (size_t)P + (size_t)t.p];
    t.on = ampli_mon_entry_ok(ref, t.y, t.ef, t.eb) != 0;
    return t;
}

// monitor_sums_kernel<LAY>: blockIdx.x = list l, (blockIdx.y, wave) = strip of MO_STRIP consecutive rows.  The wave reads its list's
// bounds, then
//   * a list of up to MO_REG_ROUNDS * 64 entries: lane i holds entry 64 k + i of round k -- the cell, the two thresholds and whether it
//     can be evaluated at all -- in registers, loaded ONCE per wave; per row it loads the records at those positions with the NEXT
//     row's loads issued before this row's records are decoded;
//   * a longer list (any length; nothing is cut across waves): per row the wave walks the list in rounds of 64, each lane reloading its
//     entry (list, reference bases and thresholds stay in L2 from row to row) and loading its record.
// Lane i takes entries i, i + 64, ... in ascending order in both forms: the order of the definition.  One shuffle reduction per (row,
// list); lane 0 stores the six sums and the two doubles.  No LDS, no barrier, no atomics: every cell has one owner and is stored once.
template <int LAY>
__global__ __launch_bounds__(64 * MO_WAVES) void monitor_sums_kernel(const RecView rv, const long long P, const int n, const int L,
                                                                       const float *__restrict__ thr, const unsigned char *__restrict__ ref_code,
                                                                       const unsigned *__restrict__ list_off, const unsigned *__restrict__ list_cell,
                                                                       const unsigned W, const int cov, const int vaf, long long *__restrict__ sums,
                                                                       double *__restrict__ lambda)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long l = blockIdx.x;
    const long long row0 = ((long long)blockIdx.y * MO_WAVES + wave) * MO_STRIP;
    if (row0 >= n) return;
    const long long row1 = row0 + MO_STRIP < n ? row0 + MO_STRIP : n;
    unsigned off, end;
    mo_bounds(list_off, l, W, off, end);
    const unsigned len = end - off;
    const size_t rb = rec_bytes(LAY);
    const size_t stride = (size_t)rv.row_stride * rb;
    long long *__restrict__ o = sums + ((size_t)row0 * (size_t)L + (size_t)l) * AMPLI_MON_SUMS;
    double *__restrict__ ol = lambda + ((size_t)row0 * (size_t)L + (size_t)l) * 2;

    if (len <= MO_REG_ROUNDS * 64) {
        MoEnt ent[MO_REG_ROUNDS];
#pragma unroll
        for (int k = 0; k < MO_REG_ROUNDS; ++k) {
            const unsigned e = off + 64u * k + lane;
            ent[k] = mo_none();
            if (e < end) ent[k] = mo_entry(list_cell[e], P, thr, ref_code);
        }
        RawRec<LAY> nxt[MO_REG_ROUNDS] = {};
        auto fetch = [&](const long long row) {
            const char *__restrict__ q = rv.base + (size_t)row * stride;
#pragma unroll
            for (int k = 0; k < MO_REG_ROUNDS; ++k)
                if (ent[k].on) nxt[k] = rec_load_at<LAY>(q + (size_t)ent[k].p * rb);
        };
        fetch(row0);
        for (long long row = row0; row < row1; ++row, o += (size_t)L * AMPLI_MON_SUMS, ol += (size_t)L * 2) {
            RawRec<LAY> cur[MO_REG_ROUNDS];
#pragma unroll
            for (int k = 0; k < MO_REG_ROUNDS; ++k) cur[k] = nxt[k];
            if (row + 1 < row1) fetch(row + 1);
            MoAcc s = mo_zero();
#pragma unroll
            for (int k = 0; k < MO_REG_ROUNDS; ++k) mo_add<LAY>(s, cur[k], ent[k].on, ent[k].y, ent[k].ef, ent[k].eb, cov, vaf);
            mo_store(o, ol, s, lane);
        }
        return;
    }
    for (long long row = row0; row < row1; ++row, o += (size_t)L * AMPLI_MON_SUMS, ol += (size_t)L * 2) {
        const char *__restrict__ q = rv.base + (size_t)row * stride;
        MoAcc s = mo_zero();
        for (unsigned e0 = off; e0 < end; e0 += 64u) { // e0 + lane cannot wrap: end <= W < 2^28
            const unsigned e = e0 + lane;
            MoEnt t = mo_none();
            if (e < end) t = mo_entry(list_cell[e], P, thr, ref_code);
            RawRec<LAY> raw = {};
            if (t.on) raw = rec_load_at<LAY>(q + (size_t)t.p * rb);
            mo_add<LAY>(s, raw, t.on, t.y, t.ef, t.eb, cov, vaf);
        }
        mo_store(o, ol, s, lane);
    }
}

// monitor_control_kernel<LAY>: blockIdx.y = pair pair_base + blockIdx.y, (blockIdx.x, wave) = replicate rep of this call (global index
// first_rep + rep).  A pair whose row or list index is outside its range stores zeros and loads nothing else -- checked before any list
// or record is read.  Otherwise the wave walks the pair's list in rounds of 64: lane i of a round draws its entry's position among the
// candidates of the entry's reference base (ampli_mon_control_draw), reads that position's thresholds and the row's record there, and
// adds as monitor_sums_kernel does -- the same lanes, the same order, the same reduction.  The candidates' bounds are cut to
// [0, n_cand] and a drawn position at or beyond P is no entry: nothing outside the buffers is addressed whatever the arrays hold.
template <int LAY>
__global__ __launch_bounds__(64 * MO_WAVES) void monitor_control_kernel(const RecView rv, const long long P, const int n, const int L,
                                                                          const float *__restrict__ thr, const unsigned char *__restrict__ ref_code,
                                                                          const unsigned *__restrict__ list_off, const unsigned *__restrict__ list_cell,
                                                                          const unsigned W, const int *__restrict__ pairs, const int pair_base,
                                                                          const unsigned *__restrict__ cand_off, const unsigned *__restrict__ cand_pos,
                                                                          const unsigned n_cand, const int R, const unsigned first_rep,
                                                                          const mo_u64 seed, const int cov, const int vaf, long long *__restrict__ sums,
                                                                          double *__restrict__ lambda)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rep = (long long)blockIdx.x * MO_WAVES + wave;
    if (rep >= R) return;
    const size_t q = (size_t)pair_base + blockIdx.y; // < n_pairs by the launch
    const int row = pairs[2 * q], l = pairs[2 * q + 1];
    long long *__restrict__ o = sums + (q * (size_t)R + (size_t)rep) * AMPLI_MON_SUMS;
    double *__restrict__ ol = lambda + (q * (size_t)R + (size_t)rep) * 2;
    MoAcc s = mo_zero();
    if ((unsigned)row < (unsigned)n && (unsigned)l < (unsigned)L) { // wave-uniform
        unsigned off, end;
        mo_bounds(list_off, l, W, off, end);
        const size_t rb = rec_bytes(LAY);
        const char *__restrict__ rec = rv.base + (size_t)row * (size_t)rv.row_stride * rb;
        for (unsigned e0 = off; e0 < end; e0 += 64u) {
            const unsigned e = e0 + lane;
            MoEnt t = mo_none();
            if (e < end) {
                const unsigned c = list_cell[e];
                const unsigned p = c >> 2;
                if ((long long)p < P) {
                    const unsigned g = ref_code[p];
                    if (g <= 3u) {
                        const unsigned lo_ = cand_off[g], hi_ = cand_off[g + 1];
                        const unsigned lo = lo_ < n_cand ? lo_ : n_cand;
                        const unsigned hi = hi_ < lo ? lo : (hi_ < n_cand ? hi_ : n_cand);
                        const unsigned m = hi - lo;
                        if (m > 0u) {
                            const unsigned drawn = cand_pos[lo + ampli_mon_control_draw(e - off, first_rep + (unsigned)rep, (unsigned)l, seed, m)];
                            // (drawn << 2 | y) of mo_entry would wrap for a drawn position at or beyond 2^30: that is no entry either
                            if ((long long)drawn < P && drawn < (1u << 30)) t = mo_entry(drawn << 2 | (c & 3u), P, thr, ref_code);
                        }
                    }
                }
            }
            RawRec<LAY> raw = {};
            if (t.on) raw = rec_load_at<LAY>(rec + (size_t)t.p * rb);
            mo_add<LAY>(s, raw, t.on, t.y, t.ef, t.eb, cov, vaf);
        }
    }
    mo_store(o, ol, s, lane);
}

// monitor_score_kernel: a lane per cell; the cell's two tails run in ONE loop, a turn of which runs one ampli_nb_step of each tail that
// is live -- lanes whose tails differ in length share every turn.  No LDS, no barrier: the same inputs give the same bytes.
__global__ __launch_bounds__(256) void monitor_score_kernel(const long long *__restrict__ sums, const double *__restrict__ lambda, const long long n_cells,
                                                            float *__restrict__ q_out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    const long long *__restrict__ c = sums + (size_t)i * AMPLI_MON_SUMS;
    float qf = AMPLI_MON_NA, qb = AMPLI_MON_NA;
    if (c[AMPLI_MON_N_EVAL] > 0) {
        ampli_nb_sum a, b;
        ampli_mon_score_begin(&a, c[AMPLI_MON_K_FW], lambda[2 * (size_t)i], &qf);
        ampli_mon_score_begin(&b, c[AMPLI_MON_K_BW], lambda[2 * (size_t)i + 1], &qb);
        while (a.live | b.live) {
            if (a.live) {
                ampli_nb_step(&a);
                if (!a.live) qf = ampli_nb_q_from_p(a.res);
            }
            if (b.live) {
                ampli_nb_step(&b);
                if (!b.live) qb = ampli_nb_q_from_p(b.res);
            }
        }
    }
    ((float2 *)q_out)[i] = make_float2(qf, qb);
}

// ==== C ABI ==============================================================================================================================

// what the two gathers share; `who` names the entry point in the message
static int mo_check(ampli_ctx *ctx, const char *who, const DevCohort &co, int64_t P, const float *d_thr, const uint8_t *d_ref_code, const uint32_t *d_list_off,
                    const uint32_t *d_list_cell, int32_t L, int64_t W, const ampli_monitor_params *prm, const int64_t *d_sums, const double *d_lambda)
{
    char msg[320];
    if (P <= 0 || L < 1 || W < 0 || !d_thr || !d_ref_code || !d_list_off || !d_list_cell || !prm || !d_sums || !d_lambda ||
        (((uintptr_t)d_sums | (uintptr_t)d_lambda) & 7) != 0 || (((uintptr_t)d_thr | (uintptr_t)d_list_off | (uintptr_t)d_list_cell) & 3) != 0 ||
        prm->coverage_cutoff < 0 || prm->max_vaf_pm < 0 || prm->max_vaf_pm > 1000) {
        snprintf(msg, sizeof msg,
                 "%s: bad argument (P > 0, L >= 1, W >= 0, coverage_cutoff >= 0, max_vaf_pm in 0..1000, 4-byte aligned d_thr, d_list_off and d_list_cell, "
                 "d_ref_code, 8-byte aligned d_sums and d_lambda)", who);
        return fail(ctx, AMPLI_E_INVALID, msg);
    }
    { int rc = check_records(ctx, co, who, nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) {
        snprintf(msg, sizeof msg, "%s: P must be below 2^31", who);
        return fail(ctx, AMPLI_E_RANGE, msg);
    }
    if (W >= (1ll << 28)) {
        snprintf(msg, sizeof msg, "%s: W must be below 2^28 (a depth is below 2^34: the int64 sums are exact below that for any counts)", who);
        return fail(ctx, AMPLI_E_RANGE, msg);
    }
    return AMPLI_OK;
}

extern "C" int ampli_monitor_sums_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                          const uint32_t *d_list_off, const uint32_t *d_list_cell, int32_t L, int64_t W, const ampli_monitor_params *prm,
                                          int64_t *d_sums, double *d_lambda)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    { int rc = mo_check(ctx, "monitor_sums_records", co, P, d_thr, d_ref_code, d_list_off, d_list_cell, L, W, prm, d_sums, d_lambda); if (rc) return rc; }
    const long long strips = ((long long)co.n + MO_WAVES * MO_STRIP - 1) / (MO_WAVES * MO_STRIP);
    if (strips > 65535) return fail(ctx, AMPLI_E_RANGE, "monitor_sums_records: n_samples must be at most 2097120");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const dim3 grid((unsigned)L, (unsigned)strips);
    with_layout(co.layout, [&](auto LAY) {
        hipLaunchKernelGGL((monitor_sums_kernel<LAY>), grid, dim3(64 * MO_WAVES), 0, st, co.rv, (long long)P, co.n, (int)L, d_thr,
                           (const unsigned char *)d_ref_code, (const unsigned *)d_list_off, (const unsigned *)d_list_cell, (unsigned)W,
                           (int)prm->coverage_cutoff, (int)prm->max_vaf_pm, (long long *)d_sums, d_lambda);
    });
    return check_launch(ctx, "monitor_sums_kernel");
}

extern "C" int ampli_monitor_control_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                             const uint32_t *d_list_off, const uint32_t *d_list_cell, int32_t L, int64_t W, const int32_t *d_pairs,
                                             int32_t n_pairs, const uint32_t *d_cand_off, const uint32_t *d_cand_pos, int64_t n_cand, int32_t R,
                                             int32_t first_rep, uint64_t seed, const ampli_monitor_params *prm, int64_t *d_sums, double *d_lambda)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (n_pairs < 1 || R < 1 || first_rep < 0 || n_cand < 0 || !d_pairs || !d_cand_off || !d_cand_pos ||
        (((uintptr_t)d_pairs | (uintptr_t)d_cand_off | (uintptr_t)d_cand_pos) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "monitor_control_records: bad argument (n_pairs >= 1, R >= 1, first_rep >= 0, n_cand >= 0, 4-byte aligned d_pairs, d_cand_off and "
                    "d_cand_pos)");
    { int rc = mo_check(ctx, "monitor_control_records", co, P, d_thr, d_ref_code, d_list_off, d_list_cell, L, W, prm, d_sums, d_lambda); if (rc) return rc; }
    if (n_cand >= (1ll << 32) || (long long)first_rep + (long long)R > 0x7FFFFFFFll)
        return fail(ctx, AMPLI_E_RANGE, "monitor_control_records: n_cand must be below 2^32 and first_rep + R below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const unsigned groups = (unsigned)(((long long)R + MO_WAVES - 1) / MO_WAVES);
    constexpr int MAX_Y = 65535; // a launch takes at most this many pairs
    for (int q0 = 0; q0 < n_pairs; q0 += MAX_Y) {
        const dim3 grid(groups, (unsigned)(n_pairs - q0 < MAX_Y ? n_pairs - q0 : MAX_Y));
        with_layout(co.layout, [&](auto LAY) {
            hipLaunchKernelGGL((monitor_control_kernel<LAY>), grid, dim3(64 * MO_WAVES), 0, st, co.rv, (long long)P, co.n, (int)L, d_thr,
                               (const unsigned char *)d_ref_code, (const unsigned *)d_list_off, (const unsigned *)d_list_cell, (unsigned)W,
                               (const int *)d_pairs, q0, (const unsigned *)d_cand_off, (const unsigned *)d_cand_pos, (unsigned)n_cand, (int)R,
                               (unsigned)first_rep, (mo_u64)seed, (int)prm->coverage_cutoff, (int)prm->max_vaf_pm, (long long *)d_sums, d_lambda);
        });
    }
    return check_launch(ctx, "monitor_control_kernel");
}

extern "C" int ampli_monitor_score(ampli_ctx *ctx, const int64_t *d_sums, const double *d_lambda, int64_t n_cells, float *d_q)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (n_cells < 1 || !d_sums || !d_lambda || !d_q || (((uintptr_t)d_sums | (uintptr_t)d_lambda | (uintptr_t)d_q) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "monitor_score: bad argument (n_cells >= 1, 8-byte aligned d_sums, d_lambda and d_q)");
    const long long blocks = ((long long)n_cells + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "monitor_score: n_cells must be at most 2^39 - 256");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    hipLaunchKernelGGL(monitor_score_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const long long *)d_sums, d_lambda, (long long)n_cells, d_q);
    return check_launch(ctx, "monitor_score_kernel");
}
