// amplisolve_amd/csrc/ampli_limits.hip -- detection limits and detection power of the calling gate.
//
// limit_pairs_kernel (ampli_limit_records) and limit_power_kernel (ampli_power_records), each with the work counters its entry point
// reports (ampli_limit_stats, ampli_power_stats).  The searches and tails themselves are ampli_math.h's; records and dispatch:
// ampli_device.h.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// ==== detection limits: the smallest alternative counts the calling gate would pass, per record and base ===============================

// limit_pairs_kernel<LAY,IRR>: one lane per (record, alternative base) pair, a workgroup = 3 waves over 64 records of one
// sample.  A pair is two searches (forward, reverse; ampli_limit_init / ampli_limit_step of ampli_math.h), and a search is 1 to ~26
// scorer evaluations of ~1000 dependent fp64 instructions each, so a wave runs as long as the longest of its lanes.  The lane therefore
// runs ONE loop whose body is one evaluation, and moves from its forward to its reverse strand inside it: a wave lasts the largest SUM
// of two searches of its lanes, not the sum of the two largest.  Three lanes per record, not four: the reference base has no search
// and a fourth lane would idle through every evaluation of its wave; lane 0 of a record writes the reference base's cell as well.
// The lanes of a wave hold consecutive (record, base) cells, so their stores are one contiguous run of 8-byte and of 1-byte elements.
// Counters: one ballot per counter and wave, summed over the workgroup in LDS, one atomic per workgroup and non-zero counter.
constexpr int LIM_RECS = 64, LIM_THREADS = 3 * LIM_RECS;

template <int LAY, bool IRR>
__global__ __launch_bounds__(LIM_THREADS) void limit_pairs_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ ext_pos, const float *__restrict__ thr,
    const unsigned char *__restrict__ ref_code, const int cov, const float *__restrict__ levels, const int n_levels,
    int2 *__restrict__ min_reads, unsigned char *__restrict__ status, unsigned long long *__restrict__ counts,
    const double *__restrict__ lgtab, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned cnt[AMPLI_LIMIT_COUNTERS + AMPLI_LIMIT_MAX_LEVELS];
    __shared__ unsigned ev[3]; // strands searched, evaluations, the most of one strand
    const int tid = threadIdx.x;
    if (tid < AMPLI_LIMIT_COUNTERS + AMPLI_LIMIT_MAX_LEVELS) cnt[tid] = 0;
    if (tid < 3) ev[tid] = 0;
    __syncthreads();
    const long long R = P + E;
    const int rl = tid / 3, a = tid - 3 * rl;
    const long long r = (long long)blockIdx.x * LIM_RECS + rl;
    const int t = blockIdx.y;
    const bool in_range = r < R; // lanes past the end keep company at the barrier
    int code = AMPLI_LIMIT_ABSENT, nt = a, mf = 0, mb = 0;
    bool recheck = false, called = false, noref_line = false, second_cell = false;
    int second_code = AMPLI_LIMIT_ABSENT, second_nt = 3;
    float min_af = 0.0f;
    unsigned n_strands = 0, n_evals = 0, max_evals = 0;
    if (in_range) {
        const long long p = r < P ? r : (long long)ext_pos[r - P];
        const int ref = ref_code[p];
        const RecCounts rc = rec_counts<LAY, IRR>(rv, P, E, t, r);
        const bool present = rc.present;
        second_cell = a == 0;
        if (present && ref > 3) {
            code = second_code = AMPLI_LIMIT_NOREF; // VC:3290
            noref_line = a == 0;
        } else if (present) {
            nt = a + (a >= ref ? 1 : 0);
            second_code = AMPLI_LIMIT_REF; second_nt = ref;
            const int FW = rc.FW, BW = rc.BW, RD = rc.RD;
            const float th_fw = thr[(size_t)nt * P + p], th_bw = thr[(size_t)(4 + nt) * P + p]; // VC:887-890
            int k_fw = 0, k_bw = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { if (j == nt) { k_fw = rc.fw[j]; k_bw = rc.bw[j]; } }
            if (FW < cov || BW < cov) code = AMPLI_LIMIT_LOWDEPTH; // VC:898
            else if (th_fw == -1 || th_bw == -1) code = AMPLI_LIMIT_NOESTIMATE;
            else {
                // the two searches in one loop: a pass of the body is one scorer evaluation, whichever strand the lane is at
                ampli_limit_search s;
                ampli_limit_init(&s, RD - BW, th_fw, FW); // VC:895: forward depth is RD - RD_reverse
                int strand = 0, r_fw = AMPLI_LIMK_PENDING, r_bw = AMPLI_LIMK_PENDING;
                for (;;) {
                    if (s.res != AMPLI_LIMK_PENDING) {
                        if (s.evals) { ++n_strands; n_evals += (unsigned)s.evals; max_evals = max(max_evals, (unsigned)s.evals); }
                        if (strand == 0) {
                            r_fw = s.res;
                            if (r_fw <= 0) break; // no forward count, or not decided here: the reverse strand changes nothing
                            strand = 1;
                            ampli_limit_init(&s, BW, th_bw, BW); // VC:896
                            continue;
                        }
                        r_bw = s.res;
                        break;
                    }
                    ampli_limit_step(&s, lgtab, AMPLI_LGTAB);
                }
                if (r_fw == AMPLI_LIMK_RECHECK || r_bw == AMPLI_LIMK_RECHECK) recheck = true;
                else if (r_fw == AMPLI_LIMK_UNREACHABLE || r_bw == AMPLI_LIMK_UNREACHABLE) {
                    code = AMPLI_LIMIT_UNREACHABLE;
                    if (RD - BW <= 0 && k_fw > 0) {
                        // an own-RD line without forward depth has no limit, but the reference's gate still scores it (a mean of 0 gives
                        // p = 0, Q = 100): the called bit is whatever the literal scorer says, as in poisson_call
                        const double q_fw = ampli_poisson_score(k_fw, RD - BW, th_fw), q_bw = ampli_poisson_score(k_bw, BW, th_bw);
                        const double lo = 5.0 - AMPLI_CALL_GATE_EPS, hi = 5.0 + AMPLI_CALL_GATE_EPS;
                        called = q_fw >= 5 && q_bw >= 5;
                        if (q_fw >= lo && q_bw >= lo && (q_fw < hi || q_bw < hi)) recheck = true;
                    }
                }
                else {
                    code = AMPLI_LIMIT_OK;
                    mf = r_fw; mb = r_bw;
                    called = k_fw >= mf && k_bw >= mb; // Q rises with the count: the gate on the observed counts
                    min_af = (float)(mf + mb) / (float)RD; // as VC:814-817 forms an AF
                }
            }
        }
        const size_t o = ((size_t)t * (size_t)R + (size_t)r) * 4;
        min_reads[o + nt] = make_int2(mf, mb);
        status[o + nt] = recheck ? (unsigned char)AMPLI_LIMIT_RECHECK : (unsigned char)(code | (called ? AMPLI_LIMIT_CALLED : 0));
        if (second_cell) {
            min_reads[o + second_nt] = make_int2(0, 0);
            status[o + second_nt] = (unsigned char)second_code;
        }
    }
    const bool pair = in_range && !recheck;
    const bool lane0 = (tid & 63) == 0;
    auto tally = [&](const int slot, const bool pred) { // one LDS add per wave
        const unsigned n = (unsigned)__popcll(__ballot(pred));
        if (lane0 && n) atomicAdd(&cnt[slot], n);
    };
    tally(0, noref_line);
    tally(1, pair && code == AMPLI_LIMIT_OK);
    tally(2, pair && code == AMPLI_LIMIT_LOWDEPTH);
    tally(3, pair && code == AMPLI_LIMIT_NOESTIMATE);
    tally(4, pair && code == AMPLI_LIMIT_UNREACHABLE);
    tally(5, recheck);
    for (int l = 0; l < n_levels; ++l) tally(AMPLI_LIMIT_COUNTERS + l, pair && code == AMPLI_LIMIT_OK && min_af <= levels[l]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_strands += __shfl_xor(n_strands, d);
        n_evals += __shfl_xor(n_evals, d);
        max_evals = max(max_evals, __shfl_xor(max_evals, d));
    }
    if (lane0 && n_strands) { atomicAdd(&ev[0], n_strands); atomicAdd(&ev[1], n_evals); atomicMax(&ev[2], max_evals); }
    __syncthreads();
    const int nc = AMPLI_LIMIT_COUNTERS + n_levels;
    if (tid < nc && cnt[tid]) atomicAdd(&counts[(size_t)t * nc + tid], (unsigned long long)cnt[tid]);
    if (tid == 0 && ev[0]) { atomicAdd(&stats[0], (unsigned long long)ev[0]); atomicAdd(&stats[1], (unsigned long long)ev[1]); atomicMax(&stats[2], (unsigned long long)ev[2]); }
}

static int ensure_limit_stats(ampli_ctx *ctx)
{
    if (ctx->d_limit_stats) return AMPLI_OK;
    if (is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "the limit counters would have to be allocated while capturing: run the sequence once first");
    if (hipMalloc((void **)&ctx->d_limit_stats, 3 * sizeof(unsigned long long)) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "limit counters hipMalloc failed");
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_limit_stats, 0, 3 * sizeof(unsigned long long), main_stream(ctx)));
    return AMPLI_OK;
}

extern "C" int ampli_limit_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                   int32_t cov, const float *d_levels, int32_t n_levels, int32_t *d_min_reads, uint8_t *d_status,
                                   int64_t *d_counts)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, trecs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_thr || !d_ref_code || cov < 1 || !d_min_reads || !d_status || !d_counts)
        return fail(ctx, AMPLI_E_INVALID, "limit_records: bad argument (P > 0, thr, ref_code, coverage_cutoff >= 1 and the three outputs are required)");
    if (n_levels < 0 || n_levels > AMPLI_LIMIT_MAX_LEVELS || (n_levels > 0 && !d_levels))
        return fail(ctx, AMPLI_E_INVALID, "limit_records: n_levels must be 0 .. 8, with d_levels when it is not 0");
    { int rc = check_records(ctx, co, "limit_records", co.ext_pos, "ext_pos"); if (rc) return rc; }
    if (((uintptr_t)d_min_reads & 7) != 0 || ((uintptr_t)d_counts & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "limit_records: min_reads and counts must be 8-byte aligned");
    const long long E = co.E, R = P + E;
    if (R >= (1ll << 30)) return fail(ctx, AMPLI_E_RANGE, "limit_records: P + E must be below 2^30 records per sample");
    if (co.n > 65535) return fail(ctx, AMPLI_E_RANGE, "limit_records: more than 65535 samples in one call (grid limit); split the cohort");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
    { int rcs = ensure_limit_stats(ctx); if (rcs) return rcs; }
    const dim3 grid((unsigned)((R + LIM_RECS - 1) / LIM_RECS), (unsigned)co.n);
    with_layout(co.layout, [&](auto L) {
        with_bool(co.rv.rd || co.rv.rd_ext, [&](auto IRR) {
            hipLaunchKernelGGL((limit_pairs_kernel<L, IRR>), grid, dim3(LIM_THREADS), 0, main_stream(ctx), co.rv, (long long)P, E, co.ext_pos, d_thr,
                               d_ref_code, (int)cov, d_levels, (int)n_levels, (int2 *)d_min_reads, d_status, (unsigned long long *)d_counts,
                               (const double *)ctx->d_lgtab, ctx->d_limit_stats);
        });
    });
    return check_launch(ctx, "limit_pairs_kernel");
}

extern "C" int ampli_limit_stats(ampli_ctx *ctx, uint64_t out[3], int32_t reset)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!out) return fail(ctx, AMPLI_E_INVALID, "limit_stats: out is required");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    out[0] = out[1] = out[2] = 0;
    if (!ctx->d_limit_stats) return AMPLI_OK;
    hipStream_t st = main_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_limit_stats, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(ctx, hipMemsetAsync(ctx->d_limit_stats, 0, 3 * sizeof(unsigned long long), st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return AMPLI_OK;
}

// ==== detection power: the probability that the gate passes at given allele fractions, and the fraction at which it reaches a confidence =

// limit_power_kernel<LAY>: one lane per cell (record, base), a workgroup = 4 waves over 64 records of one sample, so the
// lanes of a wave hold 64 consecutive cells: the LoD store is one contiguous run of floats; a level's power store has a stride of
// n_levels floats between neighbouring lanes and is issued where the lane finishes that level.  A lane whose cell is OK owes two
// binomial tails per level and two per step of the root search, each a closed-form first term and a sum of a few to a few thousand
// further ones (ampli_math.h).  A wave lasts as long as its longest lane, so the lane runs ONE loop whose body is one unit of that work
// (ampli_power_advance: a tail's start if one is due, one run of AMPLI_TAIL_RUN terms, the change of strand when the run ends the tail)
// and walks through its levels and its search inside it.  Lanes whose tails all fit one run stay in step, tail by tail; a lane with a
// longer tail falls behind by a trip per further run, and from then on a trip of the wave pays the start of some lanes AND the run of
// others.  Nothing is indexed at run time but global memory: no scratch.  Counters as limit_pairs_kernel: one ballot per counter and
// wave, summed in LDS, one atomic per workgroup and non-zero counter; the work counters are summed in 64 bits from the wave on (a lane's
// own stay below 2^32: at most 208 tails of at most 2^19 terms).
constexpr int PWR_RECS = 64, PWR_THREADS = 4 * PWR_RECS;

template <int LAY>
__global__ __launch_bounds__(PWR_THREADS) void limit_power_kernel(
    const RecView rv, const long long P, const long long E, const int2 *__restrict__ min_reads, const unsigned char *__restrict__ status,
    const float *__restrict__ levels, const int n_levels, const double conf, float *__restrict__ power, float *__restrict__ lod,
    unsigned long long *__restrict__ counts, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned cnt[1 + AMPLI_POWER_MAX_LEVELS];
    __shared__ unsigned long long ev[3]; // tails, terms, the most terms of one tail
    const int tid = threadIdx.x;
    if (tid < 1 + AMPLI_POWER_MAX_LEVELS) cnt[tid] = 0;
    if (tid < 3) ev[tid] = 0;
    __syncthreads();
    const long long R = P + E;
    const int rl = tid >> 2, nt = tid & 3;
    const long long r = (long long)blockIdx.x * PWR_RECS + rl;
    const int t = blockIdx.y;
    const bool in_range = r < R; // lanes past the end keep company at the barrier
    const size_t cell = ((size_t)t * (size_t)R + (size_t)(in_range ? r : 0)) * 4 + nt;
    bool ok = false;
    unsigned pass = 0; // bit l: power(levels[l]) >= conf
    float lod_out = 0.0f;
    unsigned n_tails = 0, n_terms = 0, max_terms = 0;
    if (in_range) {
        const unsigned st = status[cell];
        int FW = 0, BW = 0;
        int2 mr = make_int2(0, 0);
        if ((st & (7u | AMPLI_LIMIT_RECHECK)) == AMPLI_LIMIT_OK) {
            mr = min_reads[cell];
            const RecCounts rc = rec_counts<LAY, false>(rv, P, E, t, r);
            if (rc.present) { FW = rc.FW; BW = rc.BW; }
            ok = mr.x >= 1 && mr.y >= 1 && mr.x <= FW && mr.y <= BW;
        }
        if (ok) {
            ampli_power_eval e;
            ampli_lod_search s;
            ampli_power_begin(&e, FW, mr.x, BW, mr.y);
            int l = 0; // the level in hand; n_levels: the root search
            bool go = true;
            if (n_levels > 0) ampli_power_at(&e, (double)levels[0]);
            else if (lod) ampli_power_at(&e, ampli_lod_begin(&s, FW, mr.x, BW, mr.y, conf));
            else go = false;
            while (go) {
                if (!ampli_power_advance(&e)) continue;
                if (l < n_levels) {
                    if (power) power[cell * (size_t)n_levels + l] = (float)e.pw;
                    pass |= (e.pw >= conf ? 1u : 0u) << l;
                    ++l;
                    if (l < n_levels) ampli_power_at(&e, (double)levels[l]);
                    else if (lod) ampli_power_at(&e, ampli_lod_begin(&s, FW, mr.x, BW, mr.y, conf));
                    else go = false;
                } else {
                    const double v = ampli_lod_update(&s, e.pw, e.dpw);
                    if (s.done) { lod_out = (float)v; go = false; }
                    else ampli_power_at(&e, v);
                }
            }
            n_tails = e.n_tails; n_terms = e.n_terms; max_terms = e.max_terms;
        } else if (power) {
            for (int l = 0; l < n_levels; ++l) power[cell * (size_t)n_levels + l] = 0.0f;
        }
        if (lod) lod[cell] = lod_out;
    }
    const bool lane0 = (tid & 63) == 0;
    auto tally = [&](const int slot, const bool pred) { // one LDS add per wave
        const unsigned n = (unsigned)__popcll(__ballot(pred));
        if (lane0 && n) atomicAdd(&cnt[slot], n);
    };
    tally(0, ok);
    for (int l = 0; l < n_levels; ++l) tally(1 + l, (pass >> l) & 1u);
    unsigned long long w_tails = n_tails, w_terms = n_terms, w_max = max_terms;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        w_tails += __shfl_xor(w_tails, d);
        w_terms += __shfl_xor(w_terms, d);
        w_max = max(w_max, __shfl_xor(w_max, d));
    }
    if (lane0 && w_tails) { atomicAdd(&ev[0], w_tails); atomicAdd(&ev[1], w_terms); atomicMax(&ev[2], w_max); }
    __syncthreads();
    const int nc = 1 + n_levels;
    if (tid < nc && cnt[tid]) atomicAdd(&counts[(size_t)t * nc + tid], (unsigned long long)cnt[tid]);
    if (tid == 0 && ev[0]) { atomicAdd(&stats[0], ev[0]); atomicAdd(&stats[1], ev[1]); atomicMax(&stats[2], ev[2]); }
}

static int ensure_power_stats(ampli_ctx *ctx)
{
    if (ctx->d_power_stats) return AMPLI_OK;
    if (is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "the power counters would have to be allocated while capturing: run the sequence once first");
    if (hipMalloc((void **)&ctx->d_power_stats, 3 * sizeof(unsigned long long)) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "power counters hipMalloc failed");
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_power_stats, 0, 3 * sizeof(unsigned long long), main_stream(ctx)));
    return AMPLI_OK;
}

extern "C" int ampli_power_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const int32_t *d_min_reads, const uint8_t *d_status,
                                   const float *d_levels, int32_t n_levels, float confidence, float *d_power, float *d_lod, int64_t *d_counts)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!trecs || P <= 0 || !d_min_reads || !d_status || !d_counts || n_levels < 0 || n_levels > AMPLI_POWER_MAX_LEVELS || (n_levels > 0 && !d_levels) ||
        !(confidence >= 0.5f && confidence <= 0.99f))
        return fail(ctx, AMPLI_E_INVALID, "power_records: bad argument (records, P > 0, min_reads, status and counts are required; n_levels 0 .. 8, with "
                                          "d_levels when it is not 0; confidence in [0.5, 0.99])");
    DevCohort co;
    { int rc = cohort_from_records(ctx, trecs, P, co); if (rc) return rc; }
    { int rc = check_records(ctx, co, "power_records", nullptr, nullptr); if (rc) return rc; } // a cell needs its record only: no index of the extras
    if (((uintptr_t)d_min_reads & 7) != 0 || ((uintptr_t)d_counts & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "power_records: min_reads and counts must be 8-byte aligned");
    const long long E = co.E, R = P + E;
    if (R >= (1ll << 30)) return fail(ctx, AMPLI_E_RANGE, "power_records: P + E must be below 2^30 records per sample");
    if (co.n > 65535) return fail(ctx, AMPLI_E_RANGE, "power_records: more than 65535 samples in one call (grid limit); split the cohort");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcs = ensure_power_stats(ctx); if (rcs) return rcs; }
    const dim3 grid((unsigned)((R + PWR_RECS - 1) / PWR_RECS), (unsigned)co.n);
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((limit_power_kernel<L>), grid, dim3(PWR_THREADS), 0, main_stream(ctx), co.rv, (long long)P, E, (const int2 *)d_min_reads, d_status,
                           d_levels, (int)n_levels, (double)confidence, d_power, d_lod, (unsigned long long *)d_counts, ctx->d_power_stats);
    });
    return check_launch(ctx, "limit_power_kernel");
}

extern "C" int ampli_power_stats(ampli_ctx *ctx, uint64_t out[3], int32_t reset)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!out) return fail(ctx, AMPLI_E_INVALID, "power_stats: out is required");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    out[0] = out[1] = out[2] = 0;
    if (!ctx->d_power_stats) return AMPLI_OK;
    hipStream_t st = main_stream(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_power_stats, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(ctx, hipMemsetAsync(ctx->d_power_stats, 0, 3 * sizeof(unsigned long long), st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return AMPLI_OK;
}
