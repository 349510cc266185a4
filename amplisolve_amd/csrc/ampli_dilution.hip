// amplisolve_amd/csrc/ampli_dilution.hip -- in-silico dilution: read-level mixing of two count files on the device.
//
// dilute_kernel (ampli_dilute_records) thins row a of chunk A and, where one is named, row b of chunk B read by read for every listed
// mixture and writes the sum as a dense int32 record.  A read is one 32-bit word of Philox4x32-10, kept when it lies below the
// mixture's threshold (ampli_philox4x32_10 / ampli_thin_block, ampli_math.h).  Integer work only: the host library and the numpy model
// (tests/dilution_model.py) run the same text and agree integer for integer.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

constexpr int DI_WAVES = 4;     // waves of a workgroup
constexpr int DI_POS_WAVE = 4;  // positions a wave owns, one after the other
constexpr int DI_POS_WG = DI_WAVES * DI_POS_WAVE;

// the primary record of (row, p), decoded whatever the chunk's layout (a wave-uniform branch: a few instructions beside thousands of
// draws, and the two chunks of a mixture may be packed differently); every lane of the wave loads the same address
__device__ __forceinline__ void di_load(const RecView &rv, const int layout, const int row, const long long p, int4 &fw, int4 &bw)
{
    const char *__restrict__ q = rv.base + ((size_t)row * (size_t)rv.row_stride + (size_t)p) * (size_t)rec_bytes(layout);
    if (layout == AMPLI_RECORDS_U24) rec_decode<AMPLI_RECORDS_U24>(rec_load_at<AMPLI_RECORDS_U24>(q), fw, bw);
    else if (layout == AMPLI_RECORDS_U16) rec_decode<AMPLI_RECORDS_U16>(rec_load_at<AMPLI_RECORDS_U16>(q), fw, bw);
    else rec_decode<AMPLI_RECORDS_I32>(rec_load_at<AMPLI_RECORDS_I32>(q), fw, bw);
}

__device__ __forceinline__ int di_uniform(const int v) { return __builtin_amdgcn_readfirstlane(v); }

// dilute_kernel: blockIdx.y = mixture mix_base + blockIdx.y, blockIdx.x = a tile of DI_POS_WG positions; wave w owns positions
// tile * DI_POS_WG + w, + DI_WAVES, ... one record at a time.  The record's counts are wave-uniform.  Its 64 lanes deal out the
// record's Philox blocks, block j of a list to lane j mod 64; the per-field counts are added across the wave and lane 0 stores the
// 32-byte record.
// The 16 (side, field) lists are walked one after the other -- 12 of them nearly empty rounds (the alternative bases).  The form that
// lays them end to end by a wave-uniform prefix sum measured 1.8 times slower on config 3's shape (DESIGN 22;
// tools/experiments/dilution_flat_form.patch).
// A list whose threshold keeps all or none draws nothing.  A count is at most 2^24 - 2, so a list has at most 2^22 blocks and the 16
// of a record at most 2^26: 2^20 trips of a lane's loop.  A bad mixture (ampli_dilute_mix_ok) is found before any record is loaded.
// Flags: every wave ORs its bits into LDS, one integer atomic per workgroup ORs them onto the word the call cleared -- OR is
// order-free, so the bytes are reproducible.  No kernel reads another mixture's data.
__global__ __launch_bounds__(DI_WAVES * 64) void dilute_kernel(const RecView ra, const int lay_a, const int n_a, const RecView rb, const int lay_b,
                                                               const int n_b, const int has_b, const long long P,
                                                               const ampli_dilute_mix *__restrict__ mix, const int n_mix, const int mix_base,
                                                               int *__restrict__ out, int *__restrict__ flags)
{
    __shared__ int wg_flags[DI_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = di_uniform(threadIdx.x >> 6);
    const int m = mix_base + (int)blockIdx.y; // < n_mix by the launch
    const ampli_dilute_mix mx = mix[m];
    const int row_a = di_uniform(mx.row_a), row_b = di_uniform(mx.row_b);
    const unsigned long long keep_a = ((unsigned long long)(unsigned)di_uniform((int)(mx.keep_a >> 32)) << 32) | (unsigned)di_uniform((int)mx.keep_a);
    const unsigned long long keep_b = ((unsigned long long)(unsigned)di_uniform((int)(mx.keep_b >> 32)) << 32) | (unsigned)di_uniform((int)mx.keep_b);
    const unsigned long long key = ((unsigned long long)(unsigned)di_uniform((int)(mx.key >> 32)) << 32) | (unsigned)di_uniform((int)mx.key);
    const bool mix_ok = ampli_dilute_mix_ok(row_a, row_b, keep_a, keep_b, n_a, n_b, has_b) != 0;
    int wflag = mix_ok ? 0 : AMPLI_DILUTE_BAD_MIXTURE;
    const bool named_b = row_b >= 0;

    for (int i = 0; i < DI_POS_WAVE; ++i) {
        const long long p = (long long)blockIdx.x * DI_POS_WG + (long long)i * DI_WAVES + wave;
        if (p >= P) break; // wave-uniform
        int4 *__restrict__ dst = (int4 *)(out + ((size_t)m * (size_t)P + (size_t)p) * 8);
        bool present = mix_ok;
        int n[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) n[c] = 0;
        if (mix_ok) {
            int4 f, b;
            di_load(ra, lay_a, row_a, p, f, b);
            n[0] = di_uniform(f.x); n[1] = di_uniform(f.y); n[2] = di_uniform(f.z); n[3] = di_uniform(f.w);
            n[4] = di_uniform(b.x); n[5] = di_uniform(b.y); n[6] = di_uniform(b.z); n[7] = di_uniform(b.w);
            bool bad = false;
            if (n[0] == AMPLI_ABSENT) present = false;
            else bad = !ampli_dilute_counts_ok(n);
            if (named_b) {
                di_load(rb, lay_b, row_b, p, f, b);
                n[8] = di_uniform(f.x); n[9] = di_uniform(f.y); n[10] = di_uniform(f.z); n[11] = di_uniform(f.w);
                n[12] = di_uniform(b.x); n[13] = di_uniform(b.y); n[14] = di_uniform(b.z); n[15] = di_uniform(b.w);
                if (n[8] == AMPLI_ABSENT) present = false;
                else bad = bad || !ampli_dilute_counts_ok(n + 8);
            }
            if (bad) { wflag |= AMPLI_DILUTE_BAD_COUNT; present = false; }
        }
        if (!present) { // wave-uniform
            if (lane == 0) {
                dst[0] = make_int4(AMPLI_ABSENT, 0, 0, 0);
                dst[1] = make_int4(0, 0, 0, 0);
            }
            continue;
        }
        // what needs no draw: a threshold that keeps all or none (a side that is not named has counts 0)
        int fixed[8], acc[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) { fixed[f] = 0; acc[f] = 0; }
        int nb[16]; // blocks of each list
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const unsigned long long keep = c < 8 ? keep_a : keep_b;
            const bool all = keep >= AMPLI_DILUTE_KEEP_ALL, none = keep == 0ull;
            if (all) fixed[c & 7] += n[c];
            nb[c] = (all || none) ? 0 : (n[c] + 3) >> 2;
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const unsigned long long keep = c < 8 ? keep_a : keep_b;
            for (int jb = lane; jb < nb[c]; jb += 64) {
                const int left = n[c] - 4 * jb;
                acc[c & 7] += ampli_thin_block((uint32_t)jb, left >= 4 ? 4 : left, keep, key, (uint32_t)p, (uint32_t)c);
            }
        }
        // the per-field counts across the wave: every sum is below 2^25
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            int v = acc[f];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
            acc[f] = v + fixed[f];
        }
        if (lane == 0) {
            dst[0] = make_int4(acc[0], acc[1], acc[2], acc[3]);
            dst[1] = make_int4(acc[4], acc[5], acc[6], acc[7]);
        }
    }
    if (lane == 0) wg_flags[wave] = wflag;
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = 0;
#pragma unroll
        for (int w = 0; w < DI_WAVES; ++w) all |= wg_flags[w];
        if (all) atomicOr(flags + m, all);
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_dilute_records(ampli_ctx *ctx, const ampli_records *recs_a, const ampli_records *recs_b, int64_t P, const ampli_dilute_mix *d_mix,
                                    int32_t n_mix, int32_t *d_out, int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort ca, cb;
    { int rc = cohort_from_records(ctx, recs_a, P, ca); if (rc) return rc; }
    if (recs_b) { int rc = cohort_from_records(ctx, recs_b, P, cb); if (rc) return rc; }
    if (P <= 0 || n_mix < 1 || !d_mix || !d_out || !d_flags || ((uintptr_t)d_mix & 7) != 0 || ((uintptr_t)d_out & 15) != 0 || ((uintptr_t)d_flags & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "dilute_records: bad argument (P > 0, n_mix >= 1, 8-byte aligned d_mix, 16-byte aligned d_out, 4-byte aligned d_flags)");
    { int rc = check_records(ctx, ca, "dilute_records (a)", nullptr, nullptr); if (rc) return rc; }
    if (recs_b) { int rc = check_records(ctx, cb, "dilute_records (b)", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "dilute_records: P must be below 2^31");
    if (!recs_b) { cb = ca; cb.n = 0; } // never read: a mixture that names a row of b is a bad mixture
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, (size_t)n_mix * sizeof(int32_t), st));
    const long long tiles = (P + DI_POS_WG - 1) / DI_POS_WG;
    constexpr int MAX_Y = 65535; // a launch takes at most this many mixtures
    for (int m0 = 0; m0 < n_mix; m0 += MAX_Y) {
        const dim3 grid((unsigned)tiles, (unsigned)(n_mix - m0 < MAX_Y ? n_mix - m0 : MAX_Y));
        hipLaunchKernelGGL(dilute_kernel, grid, dim3(DI_WAVES * 64), 0, st, ca.rv, ca.layout, ca.n, cb.rv, cb.layout, cb.n, recs_b ? 1 : 0, (long long)P, d_mix,
                           (int)n_mix, m0, (int *)d_out, (int *)d_flags);
    }
    return check_launch(ctx, "dilute_kernel");
}
