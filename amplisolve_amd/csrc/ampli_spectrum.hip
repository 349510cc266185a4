// amplisolve_amd/csrc/ampli_spectrum.hip -- substitution spectrum: the primary records of every sample of a resident chunk binned by a
// per-position class.
//
// spectrum_kernel (ampli_spectrum_records) is the one reduction of the tree that runs along the positions into bins the data chooses:
// a streaming histogram of nine-field vectors.  Which record enters is ampli_spectrum_enters (ampli_math.h), which the host library
// exports too; the folds and the score of the sums are host work (ampli_spectrum_fold, ampli_spectrum_score).  Integers only.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long sp_u64;

constexpr int SP_WAVES = 4;                     // waves per workgroup: they share the strip's bins and take the segment's tiles in turn
constexpr int SP_STRIP = AMPLI_SPECTRUM_STRIP;  // consecutive rows (samples) of a workgroup
// the bins of a workgroup are [row of strip][class][9] uint64 in LDS, exactly the layout of its rows of d_sums: the flush is one
// contiguous copy.  Nine is odd, so the same field of 32 consecutive classes falls on 32 different 8-byte bank pairs without padding.
static_assert(AMPLI_SPEC_SUMS % 2 == 1, "an odd class stride spreads consecutive classes over the LDS banks");
static_assert((size_t)SP_STRIP * AMPLI_SPECTRUM_MAX_CLASSES * AMPLI_SPEC_SUMS * sizeof(sp_u64) <= 64 * 1024, "the bins are dynamic LDS below 64 KB");

// spectrum_kernel<LAY>: blockIdx.x = strip of SP_STRIP consecutive rows, blockIdx.y = position segment: the 64-position tiles
// [y * tps, min(tiles, (y + 1) * tps)).
//   * the workgroup clears its bins; one barrier;
//   * a wave takes the segment's tiles wave, wave + SP_WAVES, ...: a lane reads its position's reference code and class once (a lane at
//     or beyond P, or whose position is skipped, loads nothing and adds nothing), then walks the strip's rows with the NEXT row's
//     record in flight while this row's is gated;
//   * an entering lane adds 1 and its non-zero counts into bins[row][class][0..8] with 64-bit LDS atomics: lanes of one class
//     serialise on its nine words, lanes of different classes do not meet (see the stride above);
//   * one barrier; the bins go to the rows' cells of d_sums in one coalesced sweep: with one segment every cell is stored, zeros
//     included (nothing was cleared); with several (`add`) the non-zero ones are added with 64-bit integer atomics onto the
//     matrix the launcher cleared -- integer addition commutes, so the bytes do not depend on the order the segments arrive in.
// Every wave reaches both barriers: nothing returns early.
template <int LAY>
__global__ __launch_bounds__(64 * SP_WAVES) void spectrum_kernel(const RecView rv, const long long P, const int n, const unsigned char *__restrict__ ref_code,
                                                                 const unsigned char *__restrict__ cls_of, const int C, const int cov, const int max_alt_pm,
                                                                 const long long tiles, const long long tps, const int add, long long *__restrict__ sums)
{
    extern __shared__ sp_u64 bins[]; // [rows of the strip][C][9]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row0 = (long long)blockIdx.x * SP_STRIP;
    const int rows = (int)(row0 + SP_STRIP < n ? SP_STRIP : n - row0);
    const int cells = rows * C * AMPLI_SPEC_SUMS;
    for (int i = threadIdx.x; i < cells; i += 64 * SP_WAVES) bins[i] = 0ull;
    __syncthreads();

    const long long t0 = (long long)blockIdx.y * tps, t1 = t0 + tps < tiles ? t0 + tps : tiles;
    const size_t rb = rec_bytes(LAY);
    const size_t stride = (size_t)rv.row_stride * rb;
    for (long long tile = t0 + wave; tile < t1; tile += SP_WAVES) {
        const long long p = tile * 64 + lane;
        unsigned ref = 255u, cls = AMPLI_SPECTRUM_SKIP;
        if (p < P) {
            ref = ref_code[p];
            cls = cls_of[p];
        }
        const bool on = ref <= 3u && cls < (unsigned)C; // false at and beyond P
        const char *__restrict__ q = rv.base + (size_t)row0 * stride + (size_t)(on ? p : 0) * rb;
        RawRec<LAY> nxt = {};
        if (on) nxt = rec_load_at<LAY>(q);
        sp_u64 *__restrict__ b = bins + (size_t)(on ? cls : 0u) * AMPLI_SPEC_SUMS;
        for (int r = 0; r < rows; ++r, b += (size_t)C * AMPLI_SPEC_SUMS) {
            const RawRec<LAY> cur = nxt;
            if (on && r + 1 < rows) nxt = rec_load_at<LAY>(q + (size_t)(r + 1) * stride);
            int4 f, w;
            rec_decode<LAY>(cur, f, w);
            const int fw[4] = {f.x, f.y, f.z, f.w}, bw[4] = {w.x, w.y, w.z, w.w};
            if (on && ampli_spectrum_enters(fw, bw, f.x != AMPLI_ABSENT, ref, cls, C, cov, max_alt_pm)) {
                atomicAdd(b + AMPLI_SPEC_SITES, 1ull);
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    if (fw[y]) atomicAdd(b + AMPLI_SPEC_FW_A + y, (sp_u64)(long long)fw[y]);
                    if (bw[y]) atomicAdd(b + AMPLI_SPEC_BW_A + y, (sp_u64)(long long)bw[y]);
                }
            }
        }
    }
    __syncthreads();

    sp_u64 *__restrict__ o = (sp_u64 *)sums + (size_t)row0 * (size_t)C * AMPLI_SPEC_SUMS;
    for (int i = threadIdx.x; i < cells; i += 64 * SP_WAVES) {
        const sp_u64 v = bins[i];
        if (!add) o[i] = v;
        else if (v) atomicAdd(o + i, v);
    }
}

// ==== C ABI ==============================================================================================================================

// The launcher's position segments (the rule of ct_slices, ampli_contamination.hip).  A launch without segments is
// ceil(n / SP_STRIP) workgroups; while that is fewer than SP_GROUPS_PER_CU per compute unit -- a CU holds eight of these workgroups
// at 68 classes -- the T = ceil(P / 64) tiles are cut into up to SP_MAX_SEGMENTS segments of at least SP_MIN_TILES tiles (four per
// wave), all equal but the last:
//   want = min(SP_MAX_SEGMENTS, ceil(SP_GROUPS_PER_CU n_cu / strips)), tps = max(SP_MIN_TILES, ceil(T / want)), segments = ceil(T / tps).
// More segments than that buy no occupancy and cost up to rows x C x 9 atomics each; fewer tiles than that are not worth the bins'
// clearing and flush.  Every panel of up to 1024 positions is one segment, whatever n is.
constexpr int SP_MAX_SEGMENTS = 64, SP_MIN_TILES = 16, SP_GROUPS_PER_CU = 8;
static void sp_segments(const long long strips, const int n_cu, const long long tiles, long long &tps, int &segments)
{
    long long want = ((long long)SP_GROUPS_PER_CU * n_cu + strips - 1) / strips;
    if (want > SP_MAX_SEGMENTS) want = SP_MAX_SEGMENTS;
    if (want < 1) want = 1;
    tps = (tiles + want - 1) / want;
    if (tps < SP_MIN_TILES) tps = SP_MIN_TILES;
    segments = (int)((tiles + tps - 1) / tps);
}

extern "C" int ampli_spectrum_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint8_t *d_ref_code, const uint8_t *d_class, int32_t C,
                                      int32_t coverage_cutoff, int32_t max_alt_pm, int64_t *d_sums)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || C <= 0 || coverage_cutoff < 0 || max_alt_pm < 0 || max_alt_pm > 1000 || !d_ref_code || !d_class || !d_sums ||
        ((uintptr_t)d_sums & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "spectrum_records: bad argument (P > 0, C > 0, coverage_cutoff >= 0, max_alt_pm in [0, 1000], d_ref_code, d_class, 8-byte aligned "
                    "d_sums)");
    { int rc = check_records(ctx, co, "spectrum_records", nullptr, nullptr); if (rc) return rc; }
    if (C > AMPLI_SPECTRUM_MAX_CLASSES) return fail(ctx, AMPLI_E_RANGE, "spectrum_records: C must be at most AMPLI_SPECTRUM_MAX_CLASSES (128)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "spectrum_records: P must be below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long strips = ((long long)co.n + SP_STRIP - 1) / SP_STRIP, tiles = (P + 63) / 64;
    long long tps;
    int segments;
    sp_segments(strips, ctx->n_cu, tiles, tps, segments);
    if (segments > 1) HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, (size_t)co.n * (size_t)C * AMPLI_SPEC_SUMS * sizeof(int64_t), st));
    ctx->last_spectrum_segments = segments;
    const dim3 grid((unsigned)strips, (unsigned)segments);
    const size_t lds = (size_t)SP_STRIP * (size_t)C * AMPLI_SPEC_SUMS * sizeof(sp_u64);
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((spectrum_kernel<L>), grid, dim3(64 * SP_WAVES), lds, st, co.rv, (long long)P, co.n, d_ref_code, d_class, (int)C,
                           (int)coverage_cutoff, (int)max_alt_pm, tiles, tps, segments > 1 ? 1 : 0, (long long *)d_sums);
    });
    return check_launch(ctx, "spectrum_kernel");
}

extern "C" int ampli_last_spectrum_segments(const ampli_ctx *ctx)
{
    return ctx && ctx->last_spectrum_segments > 0 ? ctx->last_spectrum_segments : AMPLI_E_INVALID;
}
