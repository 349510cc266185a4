// amplisolve_amd/csrc/ampli_allelic.hip -- allelic imbalance at germline het sites, pooled per region.
//
// hetsite_reference_kernel (ampli_hetsite_reference_records) adds, for every position and het pair, the reads the normals that are het
// there show of the pair's two bases into the int64 reference [3][6][P].  allelic_site_kernel (ampli_allelic_site_records) scores the
// share of every sample at every het site of its germline against that reference with the exact two-sided binomial tail
// (ampli_ai_site_begin / ampli_ai_step, ampli_math.h).  allelic_region_kernel (ampli_allelic_region_sums) gathers the site planes
// along the regions' position lists into five int64 sums per (sample, region).  The verdict of a region is
// ampli_ai_region_verdict, decided on the host.  The definition is tests/allelic_model.py.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long ai_u64;

// the six masks of a (row, tile): bit i of pm[c] is set where the row is het with pair c at position 64 tile + i -- V and H set and
// exactly the pair's two bases.  Wave-uniform: w[] are the six plane words of the tile.
__device__ __forceinline__ void ai_pair_masks(const ai_u64 w[AMPLI_GENO_PLANES], ai_u64 pm[AMPLI_AI_PAIRS])
{
    const ai_u64 vh = w[0] & w[5], A = w[1], Cc = w[2], G = w[3], T = w[4];
    pm[0] = vh & A & Cc & ~G & ~T;
    pm[1] = vh & A & G & ~Cc & ~T;
    pm[2] = vh & A & T & ~Cc & ~G;
    pm[3] = vh & Cc & G & ~A & ~T;
    pm[4] = vh & Cc & T & ~A & ~G;
    pm[5] = vh & G & T & ~A & ~Cc;
}

// the six plane words of (row, tile) as wave-uniform values; `row` is wave-uniform
__device__ __forceinline__ void ai_load_words(const ai_u64 *__restrict__ planes, const long long row, const long long W, const long long tile,
                                              ai_u64 w[AMPLI_GENO_PLANES])
{
    const ai_u64 *__restrict__ q = planes + (size_t)row * AMPLI_GENO_PLANES * (size_t)W + (size_t)tile;
#pragma unroll
    for (int k = 0; k < AMPLI_GENO_PLANES; ++k) {
        const ai_u64 x = q[(size_t)k * (size_t)W];
        w[k] = ((ai_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
    }
}

// the lane's pair code from the six masks, -1 where none; and the reads of the pair's two bases (selects on the decoded record: no array
// indexed by a lane's own value, so nothing for the compiler to move to scratch)
__device__ __forceinline__ int ai_lane_pair(const ai_u64 pm[AMPLI_AI_PAIRS], const int lane)
{
    int c = -1;
#pragma unroll
    for (int k = 0; k < AMPLI_AI_PAIRS; ++k) c = ((pm[k] >> lane) & 1ull) ? k : c;
    return c;
}
__device__ __forceinline__ void ai_pair_reads(const int4 &f, const int4 &b, const int c, long long &k_lo, long long &k_hi)
{
    const long long nA = (long long)f.x + b.x, nC = (long long)f.y + b.y, nG = (long long)f.z + b.z, nT = (long long)f.w + b.w;
    k_lo = c < 3 ? nA : (c < 5 ? nC : nG);
    k_hi = c == 0 ? nC : ((c == 1 || c == 3) ? nG : nT);
}

// ==== stage R: the het-site reference ===================================================================================================

constexpr int HR_WAVES = 4; // waves of a workgroup: they share one tile and take the rows w, w + 4, ...

// hetsite_reference_kernel<LAY>: blockIdx.x = 64-position tile, a lane a position; wave w of the workgroup takes the chunk's rows
// w, w + HR_WAVES, ... with the next row's record in flight while the current one is decoded.  A lane adds into its own 18 sums
// (CNT, LO, HI of the six pairs, through selects); the four waves' sums meet in LDS and wave 0 adds them ONTO ref with plain vector
// loads and stores: one owner per cell and launch, integer additions only, the same bytes whatever the order.  A lane at or beyond P
// reads position P - 1 and stores nothing.
template <int LAY>
__global__ __launch_bounds__(64 * HR_WAVES) void hetsite_reference_kernel(const RecView rv, const long long P, const int n,
                                                                          const ai_u64 *__restrict__ planes, const long long W, const long long min_depth,
                                                                          long long *__restrict__ ref)
{
    __shared__ long long part[HR_WAVES - 1][AMPLI_AI_REF_PLANES * AMPLI_AI_PAIRS][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long tile = blockIdx.x;
    const long long p_raw = tile * 64 + lane;
    const bool on = p_raw < P;
    const long long p = on ? p_raw : P - 1;
    const char *__restrict__ q = rv.base + (size_t)p * rec_bytes(LAY);
    const size_t row_bytes = (size_t)rv.row_stride * rec_bytes(LAY);
    long long cnt[AMPLI_AI_PAIRS], lo[AMPLI_AI_PAIRS], hi[AMPLI_AI_PAIRS];
#pragma unroll
    for (int c = 0; c < AMPLI_AI_PAIRS; ++c) cnt[c] = lo[c] = hi[c] = 0;
    if (wave < n) {
        RawRec<LAY> cur = rec_load_at<LAY>(q + (size_t)wave * row_bytes);
        for (long long s = wave; s < n; s += HR_WAVES) {
            const RawRec<LAY> nxt = rec_load_at<LAY>(q + (size_t)(s + HR_WAVES < n ? s + HR_WAVES : s) * row_bytes);
            ai_u64 w[AMPLI_GENO_PLANES], pm[AMPLI_AI_PAIRS];
            ai_load_words(planes, s, W, tile, w);
            ai_pair_masks(w, pm);
            int4 f, b;
            rec_decode<LAY>(cur, f, b);
            const int c = ai_lane_pair(pm, lane);
            long long k_lo, k_hi;
            ai_pair_reads(f, b, c, k_lo, k_hi);
            const bool take = c >= 0 && f.x != AMPLI_ABSENT && k_lo + k_hi >= min_depth;
#pragma unroll
            for (int k = 0; k < AMPLI_AI_PAIRS; ++k) {
                const bool t = take && c == k;
                cnt[k] += t ? 1ll : 0ll;
                lo[k] += t ? k_lo : 0ll;
                hi[k] += t ? k_hi : 0ll;
            }
            cur = nxt;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < AMPLI_AI_PAIRS; ++c) {
            part[wave - 1][AMPLI_AI_REF_CNT * AMPLI_AI_PAIRS + c][lane] = cnt[c];
            part[wave - 1][AMPLI_AI_REF_LO * AMPLI_AI_PAIRS + c][lane] = lo[c];
            part[wave - 1][AMPLI_AI_REF_HI * AMPLI_AI_PAIRS + c][lane] = hi[c];
        }
    }
    __syncthreads();
    if (wave != 0 || !on) return;
#pragma unroll
    for (int c = 0; c < AMPLI_AI_PAIRS; ++c) {
#pragma unroll
        for (int v = 0; v < HR_WAVES - 1; ++v) {
            cnt[c] += part[v][AMPLI_AI_REF_CNT * AMPLI_AI_PAIRS + c][lane];
            lo[c] += part[v][AMPLI_AI_REF_LO * AMPLI_AI_PAIRS + c][lane];
            hi[c] += part[v][AMPLI_AI_REF_HI * AMPLI_AI_PAIRS + c][lane];
        }
        long long *__restrict__ o = ref + (size_t)c * (size_t)P + (size_t)p;
        const size_t plane = (size_t)AMPLI_AI_PAIRS * (size_t)P;
        o[AMPLI_AI_REF_CNT * plane] += cnt[c];
        o[AMPLI_AI_REF_LO * plane] += lo[c];
        o[AMPLI_AI_REF_HI * plane] += hi[c];
    }
}

// ==== stage S: the site planes ==========================================================================================================

constexpr int AS_WAVES = 4;    // waves of a workgroup, each with a run of rows of its own
constexpr int AS_MAX_RUN = 16; // rows of a run at most: the lane's pending cells are bits of one word

// allelic_site_kernel<LAY>: a wave = one 64-position tile (blockIdx.x) and the rows [r0, r1) of its run, one lane per position.
//   * first every row of the run is classified, the next row's record loaded before the current one is decoded: the row's germline
//     row g = row_g[s] is checked against [0, n_g) BEFORE anything is read through it, its six plane words are wave-uniform loads, the
//     reference's three cells of the lane's pair are loaded only where the lane is het, present and deep enough.  code, km and v of
//     every cell are stored here, and q = AMPLI_AI_NA of every cell that is not tested; a tested cell sets its bit in the lane's
//     `todo` word;
//   * then the lane runs all its tested cells in ONE loop: a turn starts the next cell's tail if that is due (k_lo, m and v are read
//     back from the lane's own stores), runs one ampli_ai_step of it if it is live, and stores q and moves on once it is not --
//     lanes in different cells and different stages share every turn, so a long tail holds up only the lanes that still have work.
// Every output cell is stored exactly once, with plain vector stores.  A lane at or beyond P reads position P - 1 and stores nothing.
template <int LAY>
__global__ __launch_bounds__(64 * AS_WAVES) void allelic_site_kernel(const RecView rv, const long long P, const int n, const int run,
                                                                     const ai_u64 *__restrict__ planes, const int n_g, const int *__restrict__ row_g,
                                                                     const long long W, const long long *__restrict__ ref, const ampli_allelic_params prm,
                                                                     float *__restrict__ q_out, int *km_out, double *v_out,
                                                                     unsigned char *__restrict__ code_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long tile = blockIdx.x;
    const long long r0 = ((long long)blockIdx.y * AS_WAVES + wave) * run;
    const long long r1 = r0 + run < n ? r0 + run : n;
    if (r0 >= r1) return; // wave-uniform; the kernel has no barrier
    const long long p_raw = tile * 64 + lane;
    const bool on = p_raw < P;
    const long long p = on ? p_raw : P - 1;
    const char *__restrict__ q = rv.base + (size_t)p * rec_bytes(LAY);
    const size_t row_bytes = (size_t)rv.row_stride * rec_bytes(LAY);
    const size_t plane = (size_t)AMPLI_AI_PAIRS * (size_t)P;
    unsigned todo = 0;
    RawRec<LAY> cur = rec_load_at<LAY>(q + (size_t)r0 * row_bytes);
    for (long long s = r0; s < r1; ++s) {
        const RawRec<LAY> nxt = rec_load_at<LAY>(q + (size_t)(s + 1 < r1 ? s + 1 : s) * row_bytes);
        const int g = __builtin_amdgcn_readfirstlane(row_g[s]);
        ai_u64 pm[AMPLI_AI_PAIRS] = {0, 0, 0, 0, 0, 0};
        if ((unsigned)g < (unsigned)n_g) { // wave-uniform, checked before any load through g
            ai_u64 w[AMPLI_GENO_PLANES];
            ai_load_words(planes, g, W, tile, w);
            ai_pair_masks(w, pm);
        }
        int4 f, b;
        rec_decode<LAY>(cur, f, b);
        const int c = ai_lane_pair(pm, lane);
        long long k_lo, k_hi;
        ai_pair_reads(f, b, c, k_lo, k_hi);
        const bool present = f.x != AMPLI_ABSENT;
        long long rc = 0, rl = 0, rh = 0;
        if (on && c >= 0 && present && k_lo + k_hi >= (long long)prm.min_depth && k_lo + k_hi <= AMPLI_AI_MAX_M) {
            const long long *__restrict__ rp = ref + (size_t)c * (size_t)P + (size_t)p;
            rc = rp[AMPLI_AI_REF_CNT * plane];
            rl = rp[AMPLI_AI_REF_LO * plane];
            rh = rp[AMPLI_AI_REF_HI * plane];
        }
        double v;
        const int status = ampli_ai_site_status(c, present, k_lo, k_hi, rc, rl, rh, &prm, &v);
        const bool tested = status >= AMPLI_AI_TESTED_REF;
        if (on) {
            const size_t cell = (size_t)s * (size_t)P + (size_t)p;
            code_out[cell] = (unsigned char)(status * 8 + (c >= 0 ? c : AMPLI_AI_NO_PAIR));
            ((int2 *)km_out)[cell] = tested ? make_int2((int)k_lo, (int)(k_lo + k_hi)) : make_int2(0, 0);
            v_out[cell] = v;
            if (tested) todo |= 1u << (unsigned)(s - r0);
            else q_out[cell] = AMPLI_AI_NA;
        }
        cur = nxt;
    }
    // the lane's tested cells, in one loop
    ampli_ai_sum sum;
    sum.live = 0;
    int sign = 0;
    bool start = true;
    float val = 0.0f;
    size_t cell = 0;
    while (todo) {
        if (start) {
            cell = (size_t)(r0 + __builtin_ctz(todo)) * (size_t)P + (size_t)p;
            const int2 km = ((const int2 *)km_out)[cell];
            sign = ampli_ai_site_begin(&sum, (long long)km.x, (long long)km.y, v_out[cell], &val);
            start = false;
        }
        if (sum.live) {
            ampli_ai_step(&sum);
            if (!sum.live) val = ampli_ai_q_from_p(sum.res, sign);
        }
        if (!sum.live) {
            q_out[cell] = val;
            todo &= todo - 1;
            start = true;
        }
    }
}

// ==== stage G: the region sums ==========================================================================================================

constexpr int AG_WAVES = 4; // waves per workgroup: each owns its own strip of rows, nothing is shared between them
static_assert(AMPLI_AI_STRIP == 8, "the header documents the strip");

__device__ __forceinline__ ai_u64 ag_wave_sum(ai_u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (ai_u64)__shfl_xor((long long)v, d);
    return v;
}

// allelic_region_kernel: blockIdx.x = region r, (blockIdx.y, wave) = strip of AMPLI_AI_STRIP consecutive rows.  Per row the wave walks
// the region's list in rounds of 64 -- one form for every list length; the list stays in L2 from row to row --, a lane loading the
// code of its entry and, where that is a tested cell, q, (k_lo, m) and v.  One shuffle reduction per (row, region); lane 0 stores the
// five sums, 40 bytes.  No LDS, no barrier, no atomics: every cell has one owner and is stored once, so the launcher clears nothing.
// An entry that is not below P loads nothing and adds nothing, and the list's bounds are cut to [0, W] before anything is read
// through them.  A tested cell whose q is AMPLI_AI_NA (a tail beyond its term bound) does not enter.
__global__ __launch_bounds__(64 * AG_WAVES) void allelic_region_kernel(const float *__restrict__ q_in, const int *__restrict__ km_in,
                                                                       const double *__restrict__ v_in, const unsigned char *__restrict__ code_in, const int S,
                                                                       const long long P, const int R, const unsigned *__restrict__ reg_off,
                                                                       const unsigned *__restrict__ reg_pos, const unsigned W, const double site_q,
                                                                       long long *__restrict__ sums)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = blockIdx.x;
    const long long row0 = ((long long)blockIdx.y * AG_WAVES + wave) * AMPLI_AI_STRIP;
    if (row0 >= S) return;
    const long long row1 = row0 + AMPLI_AI_STRIP < S ? row0 + AMPLI_AI_STRIP : S;
    const unsigned off_ = reg_off[r], end_ = reg_off[r + 1];
    const unsigned off = off_ < W ? off_ : W;
    const unsigned end = end_ < off ? off : (end_ < W ? end_ : W);
    for (long long row = row0; row < row1; ++row) {
        const size_t base = (size_t)row * (size_t)P;
        ai_u64 sites = 0, depth = 0, dev16 = 0, q20 = 0; // sites | sig << 32: both stay below 2^27
        for (unsigned e0 = off; e0 < end; e0 += 64u) { // e0 + lane cannot wrap: end <= W < 2^27
            const unsigned e = e0 + lane;
            if (e >= end) continue;
            const unsigned p = reg_pos[e];
            if ((long long)p >= P) continue;
            const size_t cell = base + (size_t)p;
            if ((code_in[cell] >> 3) < AMPLI_AI_TESTED_REF) continue;
            const float qv = q_in[cell];
            if (qv == AMPLI_AI_NA) continue;
            const int2 km = ((const int2 *)km_in)[cell];
            sites += 1ull + ((double)fabsf(qv) >= site_q ? 1ull << 32 : 0ull);
            depth += (ai_u64)(long long)km.y;
            dev16 += (ai_u64)ampli_ai_dev16((long long)km.x, (long long)km.y, v_in[cell]);
            q20 += (ai_u64)ampli_ai_q20(qv);
        }
        sites = ag_wave_sum(sites);
        depth = ag_wave_sum(depth);
        dev16 = ag_wave_sum(dev16);
        q20 = ag_wave_sum(q20);
        if (lane == 0) {
            long long *__restrict__ o = sums + ((size_t)row * (size_t)R + (size_t)r) * AMPLI_AI_SUMS;
            o[AMPLI_AI_SITES] = (long long)(sites & 0xFFFFFFFFull);
            o[AMPLI_AI_SIG] = (long long)(sites >> 32);
            o[AMPLI_AI_DEPTH] = (long long)depth;
            o[AMPLI_AI_DEV16] = (long long)dev16;
            o[AMPLI_AI_Q20] = (long long)q20;
        }
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_hetsite_reference_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes, int32_t min_depth,
                                               int64_t *d_ref)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_planes || !d_ref || min_depth < 1 || (((uintptr_t)d_planes | (uintptr_t)d_ref) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "hetsite_reference_records: bad argument (P > 0, min_depth >= 1, 8-byte aligned d_planes and d_ref)");
    { int rc = check_records(ctx, co, "hetsite_reference_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "hetsite_reference_records: P must be below 2^31");
    if (co.layout == AMPLI_RECORDS_I32 && P >= (1ll << 28))
        return fail(ctx, AMPLI_E_RANGE, "hetsite_reference_records: P must be below 2^28 with int32 records");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long W = (P + 63) / 64;
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((hetsite_reference_kernel<L>), dim3((unsigned)W), dim3(64 * HR_WAVES), 0, st, co.rv, (long long)P, co.n,
                           (const ai_u64 *)d_planes, W, (long long)min_depth, (long long *)d_ref);
    });
    return check_launch(ctx, "hetsite_reference_kernel");
}

extern "C" int ampli_allelic_site_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes_g, int32_t n_g,
                                          const int32_t *d_row_g, const int64_t *d_ref, const ampli_allelic_params *prm, float *d_q, int32_t *d_km,
                                          double *d_v, uint8_t *d_code)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_planes_g || n_g < 1 || !d_row_g || !d_ref || !prm || !d_q || !d_km || !d_v || !d_code ||
        (((uintptr_t)d_planes_g | (uintptr_t)d_ref | (uintptr_t)d_v | (uintptr_t)d_km) & 7) != 0 || (((uintptr_t)d_row_g | (uintptr_t)d_q) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "allelic_site_records: bad argument (P > 0, n_g >= 1, 8-byte aligned d_planes_g, d_ref, d_km and d_v, 4-byte aligned d_row_g and d_q)");
    if (prm->min_depth < 1 || prm->min_normals < 1 || (prm->half_fallback != 0 && prm->half_fallback != 1))
        return fail(ctx, AMPLI_E_INVALID, "allelic_site_records: prm must hold min_depth >= 1, min_normals >= 1 and half_fallback 0 or 1");
    { int rc = check_records(ctx, co, "allelic_site_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "allelic_site_records: P must be below 2^31");
    const int n = co.n;
    if (n > 65535 * AS_WAVES * AS_MAX_RUN) return fail(ctx, AMPLI_E_RANGE, "allelic_site_records: n_samples must be at most 4194240");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long W = (P + 63) / 64;
    // rows per wave: 16, fewer while the grid would not fill the device four times over; the grid's y stays below 65536
    int run = AS_MAX_RUN;
    while (run > 1 && W * ((n + AS_WAVES * run - 1) / (AS_WAVES * run)) < 4ll * ctx->n_cu) run >>= 1;
    while ((n + AS_WAVES * run - 1) / (AS_WAVES * run) > 65535) run <<= 1;
    const dim3 grid((unsigned)W, (unsigned)((n + AS_WAVES * run - 1) / (AS_WAVES * run)));
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((allelic_site_kernel<L>), grid, dim3(64 * AS_WAVES), 0, st, co.rv, (long long)P, n, run, (const ai_u64 *)d_planes_g, (int)n_g,
                           (const int *)d_row_g, W, (const long long *)d_ref, *prm, d_q, (int *)d_km, d_v, d_code);
    });
    return check_launch(ctx, "allelic_site_kernel");
}

extern "C" int ampli_allelic_region_sums(ampli_ctx *ctx, const float *d_q, const int32_t *d_km, const double *d_v, const uint8_t *d_code, int32_t S,
                                         int64_t P, int32_t R, const uint32_t *d_reg_off, const uint32_t *d_reg_pos, int64_t W, double site_q,
                                         int64_t *d_sums)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_q || !d_km || !d_v || !d_code || !d_reg_off || !d_reg_pos || !d_sums || S <= 0 || P <= 0 || R <= 0 || W < 0 || !(site_q >= 0.0) ||
        (((uintptr_t)d_km | (uintptr_t)d_v | (uintptr_t)d_sums) & 7) != 0 || (((uintptr_t)d_q | (uintptr_t)d_reg_off | (uintptr_t)d_reg_pos) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "allelic_region_sums: bad argument (S > 0, P > 0, R > 0, W >= 0, site_q >= 0, 8-byte aligned d_km, d_v and d_sums, 4-byte aligned d_q, "
                    "d_reg_off and d_reg_pos)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "allelic_region_sums: P must be below 2^31");
    if (W >= (1ll << 27))
        return fail(ctx, AMPLI_E_RANGE, "allelic_region_sums: W must be below 2^27 (a site adds less than 2^35 to DEV16: the int64 sums are exact below that)");
    const long long strips = ((long long)S + AG_WAVES * AMPLI_AI_STRIP - 1) / (AG_WAVES * AMPLI_AI_STRIP);
    if (strips > 65535) return fail(ctx, AMPLI_E_RANGE, "allelic_region_sums: S must be at most 2097120");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    hipLaunchKernelGGL(allelic_region_kernel, dim3((unsigned)R, (unsigned)strips), dim3(64 * AG_WAVES), 0, st, d_q, (const int *)d_km, d_v, d_code, (int)S,
                       (long long)P, (int)R, (const unsigned *)d_reg_off, (const unsigned *)d_reg_pos, (unsigned)W, site_q, (long long *)d_sums);
    return check_launch(ctx, "allelic_region_kernel");
}
