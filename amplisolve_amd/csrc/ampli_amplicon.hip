// amplisolve_amd/csrc/ampli_amplicon.hip -- amplicon coverage and copy ratio against the panel of normals.
//
// amplicon_depth_kernel (ampli_amplicon_depth_records) gathers the primary records of every sample of a resident chunk along the
// position lists of the amplicons into four int64 sums per (sample, amplicon).  amplicon_total_kernel, amplicon_reference_kernel
// (ampli_amplicon_reference) and amplicon_ratio_kernel (ampli_amplicon_ratio) are the robust statistics along the two axes of that
// matrix: library totals, the median and MAD of every amplicon's share over the normals, and every sample's ratios centred by their
// median.  The definition is tests/amplicon_model.py; the doubles agree with it bit for bit (unfused, -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long ad_u64;

// ==== stage 1: depth sums ===============================================================================================================

constexpr int AD_WAVES = 4;      // waves per workgroup: each owns its own strip of rows, nothing is shared between them
constexpr int AD_STRIP = 8;      // consecutive rows (samples) one wave sums for its amplicon (AMPLI_AMPLICON_STRIP)
constexpr int AD_REG_ROUNDS = 4; // lists of up to 4 x 64 entries keep their position indices in registers; longer ones reload them
static_assert(AD_STRIP == AMPLI_AMPLICON_STRIP, "the header documents the strip");

constexpr unsigned AD_NONE = 0xFFFFFFFFu; // the index of a lane whose entry is past the list's end, or not a position: loads nothing

// what one record adds to its lane's sums: present | callable << 32 in one word (both stay below 2^28, W < 2^28), and the strands' depths
struct AdAcc {
    ad_u64 pc, fw, bw;
};

template <int LAY> __device__ __forceinline__ void ad_add(AdAcc &s, const RawRec<LAY> &raw, const bool on, const int cov)
{
    int4 f, r;
    rec_decode<LAY>(raw, f, r);
    const bool present = on && f.x != AMPLI_ABSENT;
    // a depth is below 2^27 with the 16- and 24-bit layouts, below 2^34 with int32 records
    const long long FW = (long long)f.x + (long long)f.y + (long long)f.z + (long long)f.w;
    const long long BW = (long long)r.x + (long long)r.y + (long long)r.z + (long long)r.w;
    const bool callable = present && FW >= (long long)cov && BW >= (long long)cov;
    s.pc += (present ? 1ull : 0ull) + (callable ? 1ull << 32 : 0ull);
    s.fw += present ? (ad_u64)FW : 0ull;
    s.bw += present ? (ad_u64)BW : 0ull;
}

__device__ __forceinline__ ad_u64 ad_wave_sum(ad_u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (ad_u64)__shfl_xor((long long)v, d);
    return v;
}

__device__ __forceinline__ void ad_store(long long *__restrict__ o, const AdAcc &s, const int lane)
{
    const ad_u64 pc = ad_wave_sum(s.pc), fw = ad_wave_sum(s.fw), bw = ad_wave_sum(s.bw);
    if (lane == 0) {
        o[AMPLI_AMP_PRESENT] = (long long)(pc & 0xFFFFFFFFull);
        o[AMPLI_AMP_DEPTH_FW] = (long long)fw;
        o[AMPLI_AMP_DEPTH_BW] = (long long)bw;
        o[AMPLI_AMP_CALLABLE] = (long long)(pc >> 32);
    }
}

// amplicon_depth_kernel<LAY>: blockIdx.x = amplicon a, (blockIdx.y, wave) = strip of AD_STRIP consecutive rows.  The wave reads its
// list's bounds, then
//   * a list of up to AD_REG_ROUNDS * 64 entries: lane i holds entry 64 k + i of round k in a register (AD_NONE past the end); per
//     row it loads the records at those positions -- contiguous wherever the walk is -- with the NEXT row's loads issued before this
//     row's records are summed;
//   * a longer list (any length: there is no other form, and nothing is cut across waves): per row the wave walks the list in rounds
//     of 64, each lane reloading its index (the list stays in L2 from row to row) and loading its record.
// One shuffle reduction per (row, amplicon); lane 0 stores the four sums.  No LDS, no barrier, no atomics: every cell has one owner
// and is stored once, so the launcher clears nothing.  An entry that is not below P loads nothing and adds nothing, and the
// list's bounds are cut to [0, W] before anything is read through them.
template <int LAY>
__global__ __launch_bounds__(64 * AD_WAVES) void amplicon_depth_kernel(const RecView rv, const long long P, const int n, const int A,
                                                                         const unsigned *__restrict__ amp_off, const unsigned *__restrict__ amp_pos,
                                                                         const unsigned W, const int cov, long long *__restrict__ sums)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long a = blockIdx.x;
    const long long row0 = ((long long)blockIdx.y * AD_WAVES + wave) * AD_STRIP;
    if (row0 >= n) return;
    const long long row1 = row0 + AD_STRIP < n ? row0 + AD_STRIP : n;
    // the list's bounds, cut to [0, W]: whatever amp_off holds, no entry at or beyond W is addressed
    const unsigned off_ = amp_off[a], end_ = amp_off[a + 1];
    const unsigned off = off_ < W ? off_ : W;
    const unsigned end = end_ < off ? off : (end_ < W ? end_ : W);
    const unsigned len = end - off;
    const size_t rb = rec_bytes(LAY);
    const size_t stride = (size_t)rv.row_stride * rb;
    long long *__restrict__ o = sums + ((size_t)row0 * (size_t)A + (size_t)a) * AMPLI_AMP_SUMS;

    if (len <= AD_REG_ROUNDS * 64) {
        unsigned idx[AD_REG_ROUNDS];
#pragma unroll
        for (int k = 0; k < AD_REG_ROUNDS; ++k) {
            const unsigned e = off + 64u * k + lane;
            idx[k] = AD_NONE;
            if (e < end) {
                const unsigned p = amp_pos[e];
                if ((long long)p < P) idx[k] = p;
            }
        }
        RawRec<LAY> nxt[AD_REG_ROUNDS] = {};
        auto fetch = [&](const long long row) {
            const char *__restrict__ q = rv.base + (size_t)row * stride;
#pragma unroll
            for (int k = 0; k < AD_REG_ROUNDS; ++k)
                if (idx[k] != AD_NONE) nxt[k] = rec_load_at<LAY>(q + (size_t)idx[k] * rb);
        };
        fetch(row0);
        for (long long row = row0; row < row1; ++row, o += (size_t)A * AMPLI_AMP_SUMS) {
            RawRec<LAY> cur[AD_REG_ROUNDS];
#pragma unroll
            for (int k = 0; k < AD_REG_ROUNDS; ++k) cur[k] = nxt[k];
            if (row + 1 < row1) fetch(row + 1);
            AdAcc s = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < AD_REG_ROUNDS; ++k) ad_add<LAY>(s, cur[k], idx[k] != AD_NONE, cov);
            ad_store(o, s, lane);
        }
        return;
    }
    for (long long row = row0; row < row1; ++row, o += (size_t)A * AMPLI_AMP_SUMS) {
        const char *__restrict__ q = rv.base + (size_t)row * stride;
        AdAcc s = {0, 0, 0};
        for (unsigned e0 = off; e0 < end; e0 += 64u) { // e0 + lane cannot wrap: end <= W < 2^28
            const unsigned e = e0 + lane;
            unsigned p = AD_NONE;
            if (e < end) p = amp_pos[e];
            const bool on = p != AD_NONE && (long long)p < P;
            RawRec<LAY> raw = {};
            if (on) raw = rec_load_at<LAY>(q + (size_t)p * rb);
            ad_add<LAY>(s, raw, on, cov);
        }
        ad_store(o, s, lane);
    }
}

// ==== stage 2: totals, reference, ratios ================================================================================================

constexpr int AS_THREADS = 256;
constexpr ad_u64 AS_SENTINEL = ~0ull;                 // above every non-negative double's bit pattern: a value that is not in the set
constexpr ad_u64 AS_QNAN = 0x7FF8000000000000ull;     // the model's NaN
static_assert(AMPLI_AMPLICON_MAX * sizeof(ad_u64) <= 48 * 1024, "the selection buffer is static LDS");

__device__ __forceinline__ double as_nan() { return __longlong_as_double((long long)AS_QNAN); }
__device__ __forceinline__ double as_canon(const double v) { return v != v ? as_nan() : v; }

// the sum of one int per thread over the workgroup, for every thread; `slot` alternates between calls so that one barrier per call is enough
__device__ __forceinline__ int as_block_sum(int v, int (*part)[AS_THREADS / 64], int &slot)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) part[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < AS_THREADS / 64; ++w) t += part[slot][w];
    slot = (slot + 1) % 3;
    return t;
}

// The k-th smallest (k from 0) of the m values that are not AS_SENTINEL among buf[0 .. count), as bit patterns: non-negative doubles
// order as their bit patterns, so this is a bitwise search from the top bit down with one workgroup count per step -- no sort, no
// floating-point comparison.  Requires k < m.  buf is left as it is.
__device__ __forceinline__ ad_u64 as_select(const ad_u64 *buf, const int count, int k, int (*part)[AS_THREADS / 64], int &slot)
{
    ad_u64 prefix = 0;
    for (int b = 63; b >= 0; --b) {
        // the values that agree with the prefix above bit b and have bit b clear
        int c = 0;
        for (int i = threadIdx.x; i < count; i += AS_THREADS) c += (buf[i] >> b) == (prefix >> b) ? 1 : 0;
        c = as_block_sum(c, part, slot);
        if (k >= c) {
            k -= c;
            prefix |= 1ull << b;
        }
    }
    return prefix;
}

// the median of those m values (ampli_amplicon_median_pick: the one definition)
__device__ __forceinline__ double as_median(const ad_u64 *buf, const int count, const int m, int (*part)[AS_THREADS / 64], int &slot)
{
    if (m == 0) return as_nan();
    const ad_u64 hi = as_select(buf, count, m / 2, part, slot);
    const ad_u64 lo = (m & 1) ? hi : as_select(buf, count, m / 2 - 1, part, slot);
    return ampli_amplicon_median_pick(__longlong_as_double((long long)lo), __longlong_as_double((long long)hi), m);
}

// amplicon_total_kernel: one workgroup per sample: T[s] = the sum of DEPTH_FW + DEPTH_BW over the amplicons with use[a], in int64
__global__ __launch_bounds__(AS_THREADS) void amplicon_total_kernel(const long long *__restrict__ sums, const int A, const unsigned char *__restrict__ use,
                                                                    long long *__restrict__ total)
{
    __shared__ long long part[AS_THREADS / 64];
    const long long *__restrict__ row = sums + (size_t)blockIdx.x * (size_t)A * AMPLI_AMP_SUMS;
    long long t = 0;
    for (int a = threadIdx.x; a < A; a += AS_THREADS)
        if (use[a]) t += row[(size_t)a * AMPLI_AMP_SUMS + AMPLI_AMP_DEPTH_FW] + row[(size_t)a * AMPLI_AMP_SUMS + AMPLI_AMP_DEPTH_BW];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < AS_THREADS / 64; ++w) s += part[w];
        total[blockIdx.x] = s;
    }
}

// amplicon_reference_kernel: one workgroup per amplicon.  The shares x[n] = d[n][a] / T[n] of the included normals (T[n] > 0) go into
// LDS as bit patterns, the others as AS_SENTINEL; med by selection, then the absolute deviations in place and mad by selection.
__global__ __launch_bounds__(AS_THREADS) void amplicon_reference_kernel(const long long *__restrict__ sums, const int N, const int A,
                                                                        const long long *__restrict__ total, const int min_normals,
                                                                        double *__restrict__ ref, unsigned char *__restrict__ status)
{
    __shared__ ad_u64 buf[AMPLI_AMPLICON_MAX];
    __shared__ int part[3][AS_THREADS / 64];
    int slot = 0;
    const int a = blockIdx.x;
    int inc = 0;
    for (int n = threadIdx.x; n < N; n += AS_THREADS) {
        const long long T = total[n];
        ad_u64 bits = AS_SENTINEL;
        if (T > 0) {
            const long long *__restrict__ c = sums + ((size_t)n * (size_t)A + (size_t)a) * AMPLI_AMP_SUMS;
            const double x = ampli_amplicon_share(c[AMPLI_AMP_DEPTH_FW] + c[AMPLI_AMP_DEPTH_BW], T);
            bits = (ad_u64)__double_as_longlong(x);
            ++inc;
        }
        buf[n] = bits;
    }
    const int n_eff = as_block_sum(inc, part, slot); // its barrier also publishes buf
    const double med = as_median(buf, N, n_eff, part, slot);
    __syncthreads(); // every thread is done reading the shares
    for (int n = threadIdx.x; n < N; n += AS_THREADS) {
        const ad_u64 bits = buf[n];
        if (bits != AS_SENTINEL) buf[n] = (ad_u64)__double_as_longlong(fabs(__longlong_as_double((long long)bits) - med));
    }
    __syncthreads();
    const double mad = as_median(buf, N, n_eff, part, slot);
    if (threadIdx.x == 0) {
        ref[2 * (size_t)a + 0] = as_canon(med);
        ref[2 * (size_t)a + 1] = as_canon(mad);
        status[a] = (unsigned char)(n_eff < min_normals ? AMPLI_AMPLICON_FEW : (med == 0.0 ? AMPLI_AMPLICON_DARK : AMPLI_AMPLICON_OK));
    }
}

// amplicon_ratio_kernel: one workgroup per sample.  r[a] = (d[a] / T) / med[a] of the OK amplicons; the ones with use[a] go into LDS
// (the others as AS_SENTINEL), the centre is their median, and ratio and z of every amplicon follow from it.
__global__ __launch_bounds__(AS_THREADS) void amplicon_ratio_kernel(const long long *__restrict__ sums, const int A, const unsigned char *__restrict__ use,
                                                                    const double *__restrict__ ref, const unsigned char *__restrict__ status,
                                                                    const long long *__restrict__ total, double *__restrict__ centre,
                                                                    int *__restrict__ kk, double *__restrict__ ratio, double *__restrict__ z)
{
    __shared__ ad_u64 buf[AMPLI_AMPLICON_MAX];
    __shared__ int part[3][AS_THREADS / 64];
    int slot = 0;
    const size_t s = blockIdx.x;
    const long long T = total[s];
    const long long *__restrict__ row = sums + s * (size_t)A * AMPLI_AMP_SUMS;
    auto r_of = [&](const int a) {
        if (status[a] != AMPLI_AMPLICON_OK || T <= 0) return as_nan();
        const double x = ampli_amplicon_share(row[(size_t)a * AMPLI_AMP_SUMS + AMPLI_AMP_DEPTH_FW] + row[(size_t)a * AMPLI_AMP_SUMS + AMPLI_AMP_DEPTH_BW], T);
        return x / ref[2 * (size_t)a];
    };
    int cnt = 0;
    for (int a = threadIdx.x; a < A; a += AS_THREADS) {
        ad_u64 bits = AS_SENTINEL;
        if (use[a] && status[a] == AMPLI_AMPLICON_OK && T > 0) {
            bits = (ad_u64)__double_as_longlong(r_of(a));
            ++cnt;
        }
        buf[a] = bits;
    }
    const int K = as_block_sum(cnt, part, slot);
    const double c = as_median(buf, A, K, part, slot);
    if (threadIdx.x == 0) {
        centre[s] = as_canon(c);
        kk[s] = K;
    }
    for (int a = threadIdx.x; a < A; a += AS_THREADS) {
        const double q = r_of(a) / c;
        ratio[s * (size_t)A + a] = as_canon(q);
        z[s * (size_t)A + a] = as_canon(ampli_amplicon_z(q, ref[2 * (size_t)a], ref[2 * (size_t)a + 1]));
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_amplicon_depth_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t A, const uint32_t *d_amp_off,
                                            const uint32_t *d_amp_pos, int64_t W, int32_t coverage_cutoff, int64_t *d_sums)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || A <= 0 || W < 0 || coverage_cutoff < 0 || !d_amp_off || !d_amp_pos || !d_sums || ((uintptr_t)d_sums & 7) != 0 ||
        (((uintptr_t)d_amp_off | (uintptr_t)d_amp_pos) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "amplicon_depth_records: bad argument (P > 0, A > 0, W >= 0, coverage_cutoff >= 0, 4-byte aligned d_amp_off and d_amp_pos, 8-byte "
                    "aligned d_sums)");
    { int rc = check_records(ctx, co, "amplicon_depth_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "amplicon_depth_records: P must be below 2^31");
    if (W >= (1ll << 28))
        return fail(ctx, AMPLI_E_RANGE, "amplicon_depth_records: W must be below 2^28 (a depth is below 2^34: the int64 sums are exact below that for any counts)");
    const long long strips = ((long long)co.n + AD_WAVES * AD_STRIP - 1) / (AD_WAVES * AD_STRIP);
    if (strips > 65535) return fail(ctx, AMPLI_E_RANGE, "amplicon_depth_records: n_samples must be at most 2097120");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const dim3 grid((unsigned)A, (unsigned)strips);
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((amplicon_depth_kernel<L>), grid, dim3(64 * AD_WAVES), 0, st, co.rv, (long long)P, co.n, (int)A, (const unsigned *)d_amp_off,
                           (const unsigned *)d_amp_pos, (unsigned)W, (int)coverage_cutoff, (long long *)d_sums);
    });
    return check_launch(ctx, "amplicon_depth_kernel");
}

extern "C" int ampli_amplicon_reference(ampli_ctx *ctx, const int64_t *d_sums, int32_t N, int32_t A, const uint8_t *d_use, int32_t min_normals,
                                        int64_t *d_total, double *d_ref, uint8_t *d_status)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_sums || !d_use || !d_total || !d_ref || !d_status || N <= 0 || A <= 0 || min_normals < 1 ||
        (((uintptr_t)d_sums | (uintptr_t)d_total | (uintptr_t)d_ref) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "amplicon_reference: bad argument (N > 0, A > 0, min_normals >= 1, 8-byte aligned d_sums, d_total and d_ref)");
    if (N > AMPLI_AMPLICON_MAX) return fail(ctx, AMPLI_E_RANGE, "amplicon_reference: N must be at most AMPLI_AMPLICON_MAX (4096)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    hipLaunchKernelGGL(amplicon_total_kernel, dim3((unsigned)N), dim3(AS_THREADS), 0, st, (const long long *)d_sums, (int)A, d_use, (long long *)d_total);
    hipLaunchKernelGGL(amplicon_reference_kernel, dim3((unsigned)A), dim3(AS_THREADS), 0, st, (const long long *)d_sums, (int)N, (int)A,
                       (const long long *)d_total, (int)min_normals, d_ref, d_status);
    return check_launch(ctx, "amplicon_reference_kernel");
}

extern "C" int ampli_amplicon_ratio(ampli_ctx *ctx, const int64_t *d_sums, int32_t S, int32_t A, const uint8_t *d_use, const double *d_ref,
                                    const uint8_t *d_status, int64_t *d_total, double *d_centre, int32_t *d_k, double *d_ratio, double *d_z)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_sums || !d_use || !d_ref || !d_status || !d_total || !d_centre || !d_k || !d_ratio || !d_z || S <= 0 || A <= 0 ||
        (((uintptr_t)d_sums | (uintptr_t)d_ref | (uintptr_t)d_total | (uintptr_t)d_centre | (uintptr_t)d_ratio | (uintptr_t)d_z) & 7) != 0 ||
        ((uintptr_t)d_k & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "amplicon_ratio: bad argument (S > 0, A > 0, 8-byte aligned d_sums, d_ref, d_total, d_centre, d_ratio and d_z, 4-byte aligned d_k)");
    if (A > AMPLI_AMPLICON_MAX) return fail(ctx, AMPLI_E_RANGE, "amplicon_ratio: A must be at most AMPLI_AMPLICON_MAX (4096)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    hipLaunchKernelGGL(amplicon_total_kernel, dim3((unsigned)S), dim3(AS_THREADS), 0, st, (const long long *)d_sums, (int)A, d_use, (long long *)d_total);
    hipLaunchKernelGGL(amplicon_ratio_kernel, dim3((unsigned)S), dim3(AS_THREADS), 0, st, (const long long *)d_sums, (int)A, d_use, d_ref, d_status,
                       (const long long *)d_total, d_centre, d_k, d_ratio, d_z);
    return check_launch(ctx, "amplicon_ratio_kernel");
}
