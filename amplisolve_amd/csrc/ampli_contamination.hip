// amplisolve_amd/csrc/ampli_contamination.hip -- cross-sample contamination: the counts of every recipient weighed against the genotypes
// of every source.
//
// contamination_kernel (ampli_contamination_records) forms, for every ordered pair (recipient a of a resident chunk, source b), nine
// int64 sums over the positions from a's primary records and the genotype bit planes of a and b (ampli_concordance.hip encodes
// them).  The estimate of a pair is ampli_contamination_estimate (ampli_math.h), decided on the host.  Integers only.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long ct_u64;

// the value lane `src` holds, for every lane: src is wave-uniform (it comes out of a scalar bit walk), so this is one v_readlane
// per dword into an SGPR -- no LDS, no cross-lane network
__device__ __forceinline__ unsigned ct_bcast(const unsigned x, const int src) { return (unsigned)__builtin_amdgcn_readlane((int)x, src); }
__device__ __forceinline__ ct_u64 ct_bcast(const ct_u64 x, const int src)
{
    return ((ct_u64)ct_bcast((unsigned)(x >> 32), src) << 32) | ct_bcast((unsigned)x, src);
}
__device__ __forceinline__ ct_u64 ct_uniform(const ct_u64 x)
{
    return ((ct_u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
}

// all ones where bit i of x is set, else 0: one v_bfe_i32 (the sign-extended one-bit field), so that a selected value is that and one
// v_and with the broadcast operand -- not a compare, a move and a conditional move
template <class T> __device__ __forceinline__ T ct_sel(const unsigned x, const int i) { return (T)(long long)(int)__builtin_amdgcn_sbfe(x, (unsigned)i, 1u); }

// The per-lane masks of one 32-position half of a plane word, for the lane's source b against the wave's recipient a.
struct CtMasks {
    unsigned vb[4]; // Vb & B_Y: with the recipient's n[Y] zeroed where A_Y is set, (vb[Y] bit) * nz[Y] is o[Y]'s addend
    unsigned hb;    // Hb
    unsigned mh;    // any o[Y] & ~Hb
    unsigned mt1;   // any o[Y] & Hb
    unsigned mt2;   // two o[Y] & Hb: the second slot of such a position
    unsigned bg;
};

// The seven running sums a position adds to (the three site counts are popcounts, one per word): alt_hom is ALT_ALL - ALT_HET and
// depth_het is D_HET + D_HET2 at the end.
enum { CT_ALT_ALL, CT_ALT_HET, CT_D_HOM, CT_D_HET, CT_D_HET2, CT_A_BG, CT_D_BG, CT_RUN };

// One half word: the positions at which a is validly homozygous (the bits of `hom`, wave-uniform: a scalar walk, ~80 % of a
// panel's positions) each add bit * value into the lane's own accumulators.  T is the width the per-position values need:
// 32 bits with the 16- and 24-bit layouts (d <= 8 (2^24 - 2) < 2^27, an alt sum <= d), 64 with int32 records (d < 2^34).  The
// half's 32 positions are summed in 32 bits first with the narrow layouts -- 32 values below 2^27 stay below 2^32 -- and widened
// into the 64-bit running sums once per half; with int32 records a position adds to the 64-bit sums directly.  nz, d and u are
// the recipient's values of the word's 64 positions, one position per lane.
template <class T, class A>
__device__ __forceinline__ void ct_walk(const unsigned hom, const int lane0, const CtMasks &k, const unsigned nz[4], const T d, const T u, A acc[CT_RUN])
{
    for (unsigned m = hom; m; m &= m - 1) {
        const int i = __builtin_ctz(m), src = lane0 + i;
        const unsigned z0 = ct_bcast(nz[0], src), z1 = ct_bcast(nz[1], src), z2 = ct_bcast(nz[2], src), z3 = ct_bcast(nz[3], src);
        const T dd = ct_bcast(d, src), uu = ct_bcast(u, src);
        const T alt = (T)(ct_sel<unsigned>(k.vb[0], i) & z0) + (T)(ct_sel<unsigned>(k.vb[1], i) & z1) + (T)(ct_sel<unsigned>(k.vb[2], i) & z2) +
                      (T)(ct_sel<unsigned>(k.vb[3], i) & z3);
        const T g = ct_sel<T>(k.bg, i);
        acc[CT_ALT_ALL] += alt;
        acc[CT_ALT_HET] += ct_sel<T>(k.hb, i) & alt;
        acc[CT_D_HOM] += ct_sel<T>(k.mh, i) & dd;
        acc[CT_D_HET] += ct_sel<T>(k.mt1, i) & dd;
        acc[CT_D_HET2] += ct_sel<T>(k.mt2, i) & dd;
        acc[CT_A_BG] += g & uu;
        acc[CT_D_BG] += g & dd;
    }
}
template <class T>
__device__ __forceinline__ void ct_half(const unsigned hom, const int lane0, const CtMasks &k, const unsigned nz[4], const T d, const T u,
                                        ct_u64 run[CT_RUN])
{
    if constexpr (sizeof(T) == 8) {
        ct_walk<T, ct_u64>(hom, lane0, k, nz, d, u, run);
    } else {
        unsigned part[CT_RUN] = {0, 0, 0, 0, 0, 0, 0};
        ct_walk<T, unsigned>(hom, lane0, k, nz, d, u, part);
#pragma unroll
        for (int c = 0; c < CT_RUN; ++c) run[c] += part[c];
    }
}

// contamination_kernel<LAY>: one wave per workgroup.  blockIdx.x = recipient row a of the chunk, blockIdx.y = tile of 64 sources
// (lane = source), blockIdx.z = position slice: the words [z * wps, min(W, (z + 1) * wps)).
//   * per word the lane loads the six plane words of ITS source (a lane past n_b loads nothing and holds zeros) -- the next word's
//     are in flight during this word's walk -- and forms the masks above with a's six words, which are wave-uniform;
//   * the word's 64 records of a are loaded one per lane (coalesced; a lane at or beyond P loads nothing and counts zero, an absent
//     record counts zero), reduced to nz[Y] = A_Y ? 0 : n[Y], d and u = sum nz, and broadcast position by position;
//   * every lane adds into its own accumulators: no cross-lane reduction, no LDS, the same registers whatever n_b is.
// With one slice the nine sums are stored; with several (`add`) they are added with 64-bit integer atomics onto the matrix the
// launcher cleared -- integer addition commutes, so the bytes do not depend on the order the slices arrive in.
template <int LAY>
__global__ __launch_bounds__(64) void contamination_kernel(const RecView rv, const long long P, const ct_u64 *__restrict__ pa,
                                                           const ct_u64 *__restrict__ pb, const int n_b, const long long W, const long long wps,
                                                           const int add, long long *__restrict__ sums)
{
    using T = std::conditional_t<LAY == AMPLI_RECORDS_I32, ct_u64, unsigned>;
    const int lane = threadIdx.x;
    const long long a = blockIdx.x;
    const long long b = (long long)blockIdx.y * 64 + lane;
    const bool live = b < n_b;
    const long long w0 = (long long)blockIdx.z * wps, w1 = w0 + wps < W ? w0 + wps : W;
    const ct_u64 *__restrict__ qa = pa + (size_t)a * AMPLI_GENO_PLANES * (size_t)W;
    const ct_u64 *__restrict__ qb = pb + (size_t)(live ? b : 0) * AMPLI_GENO_PLANES * (size_t)W;
    const char *__restrict__ qr = rv.base + (size_t)a * (size_t)rv.row_stride * rec_bytes(LAY);

    ct_u64 run[CT_RUN] = {0, 0, 0, 0, 0, 0, 0};
    ct_u64 sites_hom = 0, sites_het = 0, sites_bg = 0;

    ct_u64 Bn[AMPLI_GENO_PLANES] = {0, 0, 0, 0, 0, 0};
    RawRec<LAY> rn = {};
    auto fetch = [&](const long long w) {
        if (live) {
#pragma unroll
            for (int pl = 0; pl < AMPLI_GENO_PLANES; ++pl) Bn[pl] = qb[(size_t)pl * (size_t)W + (size_t)w];
        }
        const long long p = w * 64 + lane;
        if (p < P) rn = rec_load_at<LAY>(qr + (size_t)p * rec_bytes(LAY));
    };
    if (w0 < w1) fetch(w0);
    for (long long w = w0; w < w1; ++w) {
        ct_u64 B[AMPLI_GENO_PLANES];
#pragma unroll
        for (int pl = 0; pl < AMPLI_GENO_PLANES; ++pl) B[pl] = Bn[pl];
        const RawRec<LAY> raw = rn;
        if (w + 1 < w1) fetch(w + 1);
        ct_u64 A[AMPLI_GENO_PLANES];
#pragma unroll
        for (int pl = 0; pl < AMPLI_GENO_PLANES; ++pl) A[pl] = ct_uniform(qa[(size_t)pl * (size_t)W + (size_t)w]);
        // the recipient's values of this lane's position
        int4 f, r;
        rec_decode<LAY>(raw, f, r);
        const bool counted = w * 64 + lane < P && f.x != AMPLI_ABSENT;
        const unsigned n4[4] = {(unsigned)f.x + (unsigned)r.x, (unsigned)f.y + (unsigned)r.y, (unsigned)f.z + (unsigned)r.z, (unsigned)f.w + (unsigned)r.w};
        unsigned nz[4];
        T d = 0, u = 0;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const unsigned n = counted ? n4[y] : 0u;
            nz[y] = ((A[1 + y] >> lane) & 1ull) ? 0u : n;
            d += (T)n;
            u += (T)nz[y];
        }
        // the masks of the lane's source
        const ct_u64 homA = A[0] & ~A[5];
        const ct_u64 base = homA & B[0];
        const ct_u64 oA = base & B[1] & ~A[1], oC = base & B[2] & ~A[2], oG = base & B[3] & ~A[3], oT = base & B[4] & ~A[4];
        const ct_u64 any = oA | oC | oG | oT;
        const ct_u64 two = (oA & (oC | oG | oT)) | (oC & (oG | oT)) | (oG & oT);
        const ct_u64 mh = any & ~B[5], mt1 = any & B[5], mt2 = two & B[5], bg = base & ~any;
        sites_hom += (ct_u64)__popcll(mh);
        sites_het += (ct_u64)__popcll(mt1);
        sites_bg += (ct_u64)__popcll(bg);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int sh = 32 * h;
            CtMasks k;
#pragma unroll
            for (int y = 0; y < 4; ++y) k.vb[y] = (unsigned)((B[0] & B[1 + y]) >> sh);
            k.hb = (unsigned)(B[5] >> sh);
            k.mh = (unsigned)(mh >> sh);
            k.mt1 = (unsigned)(mt1 >> sh);
            k.mt2 = (unsigned)(mt2 >> sh);
            k.bg = (unsigned)(bg >> sh);
            ct_half<T>((unsigned)(homA >> sh), sh, k, nz, d, u, run);
        }
    }
    if (!live) return;
    long long out[AMPLI_CONTAM_SUMS];
    out[AMPLI_CONTAM_SITES_HOM] = (long long)sites_hom;
    out[AMPLI_CONTAM_ALT_HOM] = (long long)(run[CT_ALT_ALL] - run[CT_ALT_HET]);
    out[AMPLI_CONTAM_DEPTH_HOM] = (long long)run[CT_D_HOM];
    out[AMPLI_CONTAM_SITES_HET] = (long long)sites_het;
    out[AMPLI_CONTAM_ALT_HET] = (long long)run[CT_ALT_HET];
    out[AMPLI_CONTAM_DEPTH_HET] = (long long)(run[CT_D_HET] + run[CT_D_HET2]);
    out[AMPLI_CONTAM_SITES_BG] = (long long)sites_bg;
    out[AMPLI_CONTAM_ALT_BG] = (long long)run[CT_A_BG];
    out[AMPLI_CONTAM_DEPTH_BG] = (long long)run[CT_D_BG];
    long long *__restrict__ o = sums + ((size_t)a * (size_t)n_b + (size_t)b) * AMPLI_CONTAM_SUMS;
    if (add) {
#pragma unroll
        for (int c = 0; c < AMPLI_CONTAM_SUMS; ++c) atomicAdd((ct_u64 *)(o + c), (ct_u64)out[c]);
    } else {
#pragma unroll
        for (int c = 0; c < AMPLI_CONTAM_SUMS; ++c) o[c] = out[c];
    }
}

// ==== C ABI ==============================================================================================================================

// The launcher's position slices.  A launch without slices is n * ceil(n_b / 64) waves; while that is fewer than CT_WAVES_PER_CU
// per compute unit -- a CU holds 20 of these waves at a time, and a second round evens out their ends -- the W plane words are cut
// into up to CT_MAX_SLICES slices of at least CT_MIN_WORDS words, all equal but the last:
//   want = min(CT_MAX_SLICES, ceil(32 n_cu / waves)), wps = max(CT_MIN_WORDS, ceil(W / want)), slices = ceil(W / wps).
// More slices than that buy no occupancy and cost nine atomics per pair each; fewer words than that are not worth a wave.
constexpr int CT_MAX_SLICES = 16, CT_MIN_WORDS = 4, CT_WAVES_PER_CU = 32;
static void ct_slices(const long long waves, const int n_cu, const long long W, long long &wps, int &slices)
{
    long long want = ((long long)CT_WAVES_PER_CU * n_cu + waves - 1) / waves;
    if (want > CT_MAX_SLICES) want = CT_MAX_SLICES;
    if (want < 1) want = 1;
    wps = (W + want - 1) / want;
    if (wps < CT_MIN_WORDS) wps = CT_MIN_WORDS;
    slices = (int)((W + wps - 1) / wps);
}

extern "C" int ampli_contamination_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const uint64_t *d_planes_a, const uint64_t *d_planes_b,
                                           int32_t n_b, int64_t *d_sums)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_planes_a || !d_planes_b || !d_sums || n_b <= 0 || (((uintptr_t)d_planes_a | (uintptr_t)d_planes_b | (uintptr_t)d_sums) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "contamination_records: bad argument (P > 0, n_b > 0, 8-byte aligned d_planes_a, d_planes_b and d_sums)");
    { int rc = check_records(ctx, co, "contamination_records", nullptr, nullptr); if (rc) return rc; }
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "contamination_records: P must be below 2^31");
    if (co.layout == AMPLI_RECORDS_I32 && P >= (1ll << 28))
        return fail(ctx, AMPLI_E_RANGE,
                    "contamination_records: P must be below 2^28 with int32 records (a position adds up to 2^35 to a sum: the int64 sums are exact "
                    "below that for any counts)");
    const long long tb = ((long long)n_b + 63) / 64;
    if (tb > 65535) return fail(ctx, AMPLI_E_RANGE, "contamination_records: n_b must be at most 4194240");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long W = (P + 63) / 64;
    long long wps;
    int slices;
    ct_slices((long long)co.n * tb, ctx->n_cu, W, wps, slices);
    if (slices > 1) HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, (size_t)co.n * (size_t)n_b * AMPLI_CONTAM_SUMS * sizeof(int64_t), st));
    const dim3 grid((unsigned)co.n, (unsigned)tb, (unsigned)slices);
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((contamination_kernel<L>), grid, dim3(64), 0, st, co.rv, (long long)P, (const ct_u64 *)d_planes_a,
                           (const ct_u64 *)d_planes_b, (int)n_b, W, wps, slices > 1 ? 1 : 0, (long long *)d_sums);
    });
    return check_launch(ctx, "contamination_kernel");
}
