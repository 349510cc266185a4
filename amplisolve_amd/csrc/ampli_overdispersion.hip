// amplisolve_amd/csrc/ampli_overdispersion.hip -- overdispersion-aware calling: the dispersion omega of every cell of the
// panel of normals and the negative-binomial score of every cell of a tumour.
//
// overdispersion_stream_kernel (ampli_overdispersion_records) adds S2 = sum d_i^2 over a cell's qualifying records -- the set the
// threshold sums and dispersion count: thr_gate (ampli_device.h) on records that come through rec_counts.
// overdispersion_finalize_kernel (ampli_overdispersion_finalize) turns dispersion's X2 and status and S2 into omega
// (ampli_overdispersion_cell, ampli_math.h).  nb_score_kernel (ampli_nb_score_records) scores a chunk of tumours against the table's
// thresholds and omega (ampli_nb_score_begin / ampli_nb_step, ampli_math.h).  The host library exports the same texts.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long od_u64;

// a sum of squares as two words: d < 2^31, so one square is below 2^62 and only the sum can leave 64 bits
struct OdSum {
    od_u64 lo[8], hi[8]; // strand-major: cell c = st * 4 + nt
};

__device__ __forceinline__ void od_add(od_u64 &lo, od_u64 &hi, const od_u64 v, const od_u64 vhi)
{
    lo += v;
    hi += vhi + (lo < v ? 1ull : 0ull);
}

// the sum as a double: exact below 2^53, else one rounding of each word and of their sum
__device__ __forceinline__ double od_value(const od_u64 lo, const od_u64 hi) { return (double)hi * 18446744073709551616.0 + (double)lo; }

// one record's terms: dispersion's gate (disp_visit), without its OK mask -- S2 is defined for every cell
__device__ __forceinline__ void od_visit(const RecCounts &a, const bool on, const int cov, OdSum &s)
{
    const bool covok = on && a.present && a.FW >= cov && a.BW >= cov;
    const unsigned qual = thr_gate(a.fw, a.bw, a.FW, a.BW, covok, a.own_rd || a.RD >= AMPLI_COUNT_LIMIT);
    if (qual) { // a qualifying record has FW, BW >= cov >= 1
        const od_u64 q_fw = (od_u64)(unsigned)a.FW * (od_u64)(unsigned)a.FW, q_bw = (od_u64)(unsigned)a.BW * (od_u64)(unsigned)a.BW;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            if ((qual >> nt) & 1u) {
                od_add(s.lo[nt], s.hi[nt], q_fw, 0);
                od_add(s.lo[4 + nt], s.hi[4 + nt], q_bw, 0);
            }
        }
    }
}

// overdispersion_stream_kernel<LAY,IRR>: dispersion_stream_kernel's shape.  A workgroup = 4 waves over one 64-position tile, one lane
// per position, wave w taking rows w, w + 4, ...; the extras of a position are its lane's own.  Eight two-word integer sums per lane
// are handed over in LDS and added in wave order -- integers, so any order gives the same words -- then stored as doubles or added to
// the plane.  No atomics: the same inputs in the same chunks give the same bytes.  One barrier, reached by every wave.
template <int LAY, bool IRR>
__global__ __launch_bounds__(256) void overdispersion_stream_kernel(const RecView rv, const long long P, const long long E,
                                                                    const unsigned *__restrict__ dup_off, const int n, const int cov,
                                                                    double *__restrict__ s2_out, const int accumulate)
{
    __shared__ od_u64 lds[3][16][64]; // waves 1..3: lo[8] | hi[8] per lane
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p_raw = (long long)blockIdx.x * 64 + lane;
    const bool valid = p_raw < P;
    const long long p = valid ? p_raw : P - 1;
    const long long e0 = E > 0 ? (long long)dup_off[p] : 0;
    const int n_ext = E > 0 && valid ? (int)(dup_off[p + 1] - dup_off[p]) : 0;
    OdSum s;
#pragma unroll
    for (int c = 0; c < 8; ++c) { s.lo[c] = 0; s.hi[c] = 0; }
    RecCounts cur = rec_counts<LAY, IRR>(rv, P, E, wave < n ? wave : 0, p);
    for (int r = wave; r < n; r += 4) {
        const RecCounts nxt = rec_counts<LAY, IRR>(rv, P, E, r + 4 < n ? r + 4 : r, p); // in flight during this row's arithmetic
        od_visit(cur, valid, cov, s);
        for (int j = 0; j < n_ext; ++j) od_visit(rec_counts<LAY, IRR>(rv, P, E, r, P + e0 + j), true, cov, s);
        cur = nxt;
    }
    if (wave) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            lds[wave - 1][c][lane] = s.lo[c];
            lds[wave - 1][8 + c][lane] = s.hi[c];
        }
    }
    __syncthreads();
    if (wave == 0 && valid) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            od_u64 lo = s.lo[c], hi = s.hi[c];
#pragma unroll
            for (int w = 0; w < 3; ++w) od_add(lo, hi, lds[w][c][lane], lds[w][8 + c][lane]);
            const double v = od_value(lo, hi);
            const long long o = c * P + p;
            s2_out[o] = accumulate ? s2_out[o] + v : v;
        }
    }
}

// one lane per position, eight cells each (ampli_overdispersion_cell)
__global__ __launch_bounds__(256) void overdispersion_finalize_kernel(const long long P, const double *__restrict__ snt, const long long *__restrict__ srd,
                                                                      const int *__restrict__ cnt, const double *__restrict__ x2,
                                                                      const double *__restrict__ s2, const unsigned char *__restrict__ status,
                                                                      double *__restrict__ omega)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nq = cnt[nt * P + p];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const long long o = (st * 4 + nt) * P + p;
            omega[o] = ampli_overdispersion_cell(status[o], nq, snt[o], (double)srd[o], x2[o], s2[o]);
        }
    }
}

// nb_score_kernel<LAY>: blockIdx.x = 64-position tile, a lane a position; wave w of workgroup blockIdx.y owns tumour row row_base +
// blockIdx.y * 4 + w.  A lane at or beyond P and a row at or beyond n_t load and store nothing.  A lane whose (row, position) is not
// evaluated stores eight AMPLI_NB_NA; every other lane stores NA for the reference base and walks its six cells (c = base * 2 +
// strand, the order of d_q) in ONE loop: a turn of the loop starts the cell's tail if that is due, runs one ampli_nb_step of it if it
// is live, and stores the score and moves on once it is not -- lanes in different cells and different stages share every turn.
// There is no LDS and no barrier; the eight counts are indexed by the cell and the compiler keeps them in registers (no scratch).
template <int LAY>
__global__ __launch_bounds__(256) void nb_score_kernel(const RecView rt, const int n_t, const int row_base, const long long P,
                                                       const float *__restrict__ thr, const double *__restrict__ omega,
                                                       const unsigned char *__restrict__ ref_code, const int cutoff, float *__restrict__ q_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p = (long long)blockIdx.x * 64 + lane;
    const int t = row_base + (int)blockIdx.y * 4 + wave;
    if (p >= P || t >= n_t) return;
    const RawRec<LAY> raw = rec_load_at<LAY>(rt.base + ((size_t)t * (size_t)rt.row_stride + (size_t)p) * rec_bytes(LAY));
    int4 f, b;
    rec_decode<LAY>(raw, f, b);
    const bool present = f.x != AMPLI_ABSENT;
    const int x[8] = {f.x, b.x, f.y, b.y, f.z, b.z, f.w, b.w}; // c = base * 2 + strand
    const int D0 = f.x + f.y + f.z + f.w, D1 = b.x + b.y + b.z + b.w;
    const unsigned ref = ref_code[p];
    float *__restrict__ out = q_out + ((size_t)t * (size_t)P + (size_t)p) * 8;
    if (!(present && D0 >= cutoff && D1 >= cutoff && ref <= 3u)) {
        const float4 na = make_float4(AMPLI_NB_NA, AMPLI_NB_NA, AMPLI_NB_NA, AMPLI_NB_NA);
        ((float4 *)out)[0] = na;
        ((float4 *)out)[1] = na;
        return;
    }
    out[2 * ref] = AMPLI_NB_NA;
    out[2 * ref + 1] = AMPLI_NB_NA;
    ampli_nb_sum s;
    s.live = 0;
    int c = ref == 0u ? 2 : 0;
    bool start = true;
    float q = 0.0f;
    while (c < 8) {
        if (start) {
            const int st = c & 1, nt = c >> 1;
            const size_t o = (size_t)(st * 4 + nt) * (size_t)P + (size_t)p;
            ampli_nb_score_begin(&s, x[c], st ? D1 : D0, thr[o], omega ? omega[o] : 0.0, &q);
            start = false;
        }
        if (s.live) {
            ampli_nb_step(&s);
            if (!s.live) q = ampli_nb_q_from_p(s.res);
        }
        if (!s.live) {
            out[c] = q;
            ++c;
            if ((unsigned)(c >> 1) == ref) c += 2;
            start = true;
        }
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_overdispersion_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc0, int32_t cov,
                                            double *d_s2, int32_t accumulate)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || cov < 1 || !d_s2 || ((uintptr_t)d_s2 & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "overdispersion_records: bad argument (P > 0, coverage_cutoff >= 1, an 8-byte aligned S2 plane)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "overdispersion_records: P must be below 2^31");
    if (!acc_is_bound(d_acc0) || d_acc0->P != P)
        return fail(ctx, AMPLI_E_INVALID, "overdispersion_records: d_acc0 must be an ampli_acc_bind table of P positions");
    { int rc = check_records(ctx, co, "overdispersion_records", co.dup_off, "dup_off"); if (rc) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long tiles = (P + 63) / 64;
    with_layout(co.layout, [&](auto L) {
        with_bool(co.rv.rd || co.rv.rd_ext, [&](auto IRR) {
            hipLaunchKernelGGL((overdispersion_stream_kernel<L, IRR>), dim3((unsigned)tiles), dim3(256), 0, st, co.rv, (long long)P, co.E, co.dup_off, co.n,
                               (int)cov, d_s2, accumulate ? 1 : 0);
        });
    });
    return check_launch(ctx, "overdispersion_stream_kernel");
}

extern "C" int ampli_overdispersion_finalize(ampli_ctx *ctx, int64_t P, const ampli_acc_table *d_acc0, const double *d_x2, const double *d_s2,
                                             const uint8_t *d_status, double *d_omega)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || !d_x2 || !d_s2 || !d_status || !d_omega || (((uintptr_t)d_x2 | (uintptr_t)d_s2 | (uintptr_t)d_omega) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "overdispersion_finalize: bad argument (P > 0, every plane given, the double planes 8-byte aligned)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "overdispersion_finalize: P must be below 2^31");
    if (!acc_is_bound(d_acc0) || d_acc0->P != P)
        return fail(ctx, AMPLI_E_INVALID, "overdispersion_finalize: d_acc0 must be an ampli_acc_bind table of P positions");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const AccPtrs acc = to_ptrs(d_acc0);
    hipLaunchKernelGGL(overdispersion_finalize_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (long long)P, (const double *)acc.snt,
                       (const long long *)acc.srd, (const int *)acc.cnt, d_x2, d_s2, d_status, d_omega);
    return check_launch(ctx, "overdispersion_finalize_kernel");
}

extern "C" int ampli_nb_score_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr, const double *d_omega,
                                      const uint8_t *d_ref_code, int32_t calling_cutoff, float *d_q)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, trecs, P, co); if (rc) return rc; }
    if (P <= 0 || calling_cutoff < 0 || !d_thr || !d_ref_code || !d_q || ((uintptr_t)d_thr & 3) != 0 || ((uintptr_t)d_omega & 7) != 0 ||
        ((uintptr_t)d_q & 15) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "nb_score_records: bad argument (P > 0, calling_cutoff >= 0, d_thr 4-byte aligned, d_omega NULL or 8-byte aligned, d_ref_code, "
                    "16-byte aligned d_q)");
    { int rc = check_records(ctx, co, "nb_score_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "nb_score_records: P must be below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long tiles = (P + 63) / 64, groups = ((long long)co.n + 3) / 4;
    constexpr long long MAX_Y = 65535; // a launch takes at most this many row groups
    for (long long g0 = 0; g0 < groups; g0 += MAX_Y) {
        const dim3 grid((unsigned)tiles, (unsigned)(groups - g0 < MAX_Y ? groups - g0 : MAX_Y));
        with_layout(co.layout, [&](auto L) {
            hipLaunchKernelGGL((nb_score_kernel<L>), grid, dim3(256), 0, st, co.rv, co.n, (int)(g0 * 4), (long long)P, d_thr, d_omega, d_ref_code,
                               (int)calling_cutoff, d_q);
        });
    }
    return check_launch(ctx, "nb_score_kernel");
}
