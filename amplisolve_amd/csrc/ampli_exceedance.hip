// amplisolve_amd/csrc/ampli_exceedance.hip -- panel-of-normals exceedance: for every (tumour row, position, base, strand), how many of
// the normals show the allele at the tumour's fraction or above.
//
// exceedance_kernel (ampli_exceedance_records) is the one dense (row x row) comparison of COUNTS in the tree: every tumour row of a
// chunk against every normal row of a chunk, per position, exactly, in unsigned 64-bit integers.  The candidate rule on top of the
// counts is host work (ampli_exceedance_candidate, ampli_math.h).  Integers only, no atomics: every (t, p) cell has one owning lane.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

typedef unsigned long long ex_u64;

constexpr int EX_WAVES = 4;                            // waves per workgroup: they share the decoded strip of normals
constexpr int EX_RPW = 2;                              // tumour rows a lane keeps in registers: one LDS read of a normal serves both
constexpr int EX_ROWS = AMPLI_EXCEEDANCE_ROWS;         // tumour rows per workgroup
constexpr int EX_STRIP = AMPLI_EXCEEDANCE_STRIP;       // normal rows decoded into LDS at a time
constexpr int EX_PF = EX_STRIP / EX_WAVES;             // raw records of the next strip a lane keeps in flight
constexpr int EX_WORDS = 11;                           // a decoded record: 8 counts, the low words of the two depths, flags
static_assert(EX_ROWS == EX_WAVES * EX_RPW, "a workgroup's rows are its waves' rows");
static_assert(EX_STRIP % EX_WAVES == 0, "every wave decodes the same number of rows of a strip");
static_assert((size_t)EX_STRIP * EX_WORDS * 64 * 4 <= 64 * 1024, "the strip is static LDS below 64 KB");

// The decoded record of a normal in LDS is word-major, strip[(row * EX_WORDS + word) * 64 + lane]: a wave's read of one word is 64
// consecutive dwords, free of bank conflicts.  Words 0..7: fw[0..3], bw[0..3]; 8, 9: the low 32 bits of D[0], D[1]; 10: bit 0 =
// present and covered on both strands (eligible but for skip_same_index), bits 1.. and 3..: bits 32.. of D[0] and D[1] (a depth is
// below 2^33: four fields below 2^31).  An absent record, a row at or beyond n_n and a lane at or beyond P are all zeros.
struct ExRec {
    unsigned x[8];
    ex_u64 D[2];
    bool ok; // present (for a normal: and covered on both strands)
};

template <int LAY> __device__ __forceinline__ ExRec ex_decode(const RawRec<LAY> &raw, const bool loaded, const int cutoff)
{
    int4 f, w;
    rec_decode<LAY>(raw, f, w);
    const bool present = loaded && f.x != AMPLI_ABSENT;
    ExRec r;
    const int v[8] = {f.x, f.y, f.z, f.w, w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) r.x[i] = present ? (unsigned)v[i] : 0u;
    r.D[0] = (ex_u64)r.x[0] + r.x[1] + r.x[2] + r.x[3];
    r.D[1] = (ex_u64)r.x[4] + r.x[5] + r.x[6] + r.x[7];
    r.ok = present && r.D[0] >= (ex_u64)cutoff && r.D[1] >= (ex_u64)cutoff;
    return r;
}

// exceedance_kernel<LT, LN>: blockIdx.x = 64-position tile, blockIdx.y = group of EX_ROWS tumour rows starting at row_base; a lane is
// a position, wave w owns the rows row_base + blockIdx.y * EX_ROWS + w * EX_RPW + {0, 1} of it.
//   * a lane loads and decodes its tumour records once (a lane at or beyond P and a row at or beyond n_t load nothing);
//   * the normals pass through LDS in strips of EX_STRIP rows: wave w decodes rows w, w + 4, ... of the strip for the tile's 64
//     positions, one barrier, then every wave walks the strip -- one record read serves its EX_RPW rows -- while the raw records
//     of the NEXT strip are in flight, one barrier;
//   * a cell counts normal s iff s is eligible and x_s D_t >= x_t D_s, both products unsigned 64-bit: WIDE (an int32 layout on
//     either side) multiplies a 32-bit count by a 33-bit depth, otherwise every operand is below 2^26 and a product is one
//     32 x 32 -> 64 multiply;
//   * the owning lane stores d_elig and the 16 bytes of d_ge[t][p] -- or, with `accumulate`, reads them, adds and stores: nothing
//     else ever touches the cell in this launch, so there are no atomics and the bytes do not depend on any order.
// Every wave reaches every barrier: the strip loop's bounds are uniform and nothing returns early.
template <int LT, int LN>
__global__ __launch_bounds__(64 * EX_WAVES) void exceedance_kernel(const RecView rt, const int n_t, const int row_base, const RecView rn, const int n_n,
                                                                   const long long P, const unsigned char *__restrict__ ref_code, const int normal_cutoff,
                                                                   const int calling_cutoff, const long long skip_delta, const int skip,
                                                                   const int accumulate, unsigned short *__restrict__ elig_out,
                                                                   unsigned short *__restrict__ ge_out)
{
    constexpr bool WIDE = LT == AMPLI_RECORDS_I32 || LN == AMPLI_RECORDS_I32;
    __shared__ unsigned strip[EX_STRIP * EX_WORDS * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p = (long long)blockIdx.x * 64 + lane;
    const bool in = p < P;
    const size_t pp = in ? (size_t)p : 0;

    // this lane's tumour rows
    const int t0 = row_base + (int)blockIdx.y * EX_ROWS + wave * EX_RPW;
    ExRec tum[EX_RPW];
    long long skip_s[EX_RPW]; // the normal row of this chunk that is the same file as the tumour row, or -1
    unsigned ge[EX_RPW][8], el[EX_RPW];
#pragma unroll
    for (int j = 0; j < EX_RPW; ++j) {
        const int t = t0 + j;
        const bool on = in && t < n_t;
        RawRec<LT> raw = {};
        if (on) raw = rec_load_at<LT>(rt.base + ((size_t)t * (size_t)rt.row_stride + pp) * rec_bytes(LT));
        tum[j] = ex_decode<LT>(raw, on, calling_cutoff);
        skip_s[j] = skip ? (long long)t + skip_delta : -1;
        el[j] = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) ge[j][i] = 0;
    }

    const size_t nb = rec_bytes(LN);
    const char *__restrict__ qn = rn.base + pp * nb;
    const size_t nstride = (size_t)rn.row_stride * nb;
    RawRec<LN> nxt[EX_PF];
#pragma unroll
    for (int i = 0; i < EX_PF; ++i) {
        const int s = wave + EX_WAVES * i;
        nxt[i] = RawRec<LN>{};
        if (in && s < n_n) nxt[i] = rec_load_at<LN>(qn + (size_t)s * nstride);
    }
    for (int s0 = 0; s0 < n_n; s0 += EX_STRIP) {
#pragma unroll
        for (int i = 0; i < EX_PF; ++i) {
            const int r = wave + EX_WAVES * i;
            const ExRec d = ex_decode<LN>(nxt[i], in && s0 + r < n_n, normal_cutoff);
            unsigned *__restrict__ o = strip + (size_t)r * EX_WORDS * 64 + lane;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k * 64] = d.x[k];
            o[8 * 64] = (unsigned)d.D[0];
            o[9 * 64] = (unsigned)d.D[1];
            o[10 * 64] = (d.ok ? 1u : 0u) | (unsigned)(d.D[0] >> 32) << 1 | (unsigned)(d.D[1] >> 32) << 3;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EX_PF; ++i) {
            const int s = s0 + EX_STRIP + wave + EX_WAVES * i;
            if (in && s < n_n) nxt[i] = rec_load_at<LN>(qn + (size_t)s * nstride);
        }
        const int rows = n_n - s0 < EX_STRIP ? n_n - s0 : EX_STRIP;
        for (int r = 0; r < rows; ++r) {
            const unsigned *__restrict__ q = strip + (size_t)r * EX_WORDS * 64 + lane;
            unsigned xs[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) xs[k] = q[k * 64];
            const unsigned fl = q[10 * 64];
            ex_u64 Ds[2] = {q[8 * 64], q[9 * 64]};
            if (WIDE) {
                Ds[0] |= (ex_u64)((fl >> 1) & 3u) << 32;
                Ds[1] |= (ex_u64)((fl >> 3) & 3u) << 32;
            }
#pragma unroll
            for (int j = 0; j < EX_RPW; ++j) {
                const unsigned e = (fl & 1u) & (skip_s[j] != (long long)(s0 + r) ? 1u : 0u);
                el[j] += e;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int st = k >> 2;
                    bool reach;
                    if (WIDE) reach = (ex_u64)xs[k] * tum[j].D[st] >= (ex_u64)tum[j].x[k] * Ds[st];
                    else reach = (ex_u64)xs[k] * (unsigned)tum[j].D[st] >= (ex_u64)tum[j].x[k] * (unsigned)Ds[st];
                    ge[j][k] += reach ? e : 0u;
                }
            }
        }
        __syncthreads();
    }

    const unsigned ref = in ? ref_code[p] : 255u;
#pragma unroll
    for (int j = 0; j < EX_RPW; ++j) {
        const int t = t0 + j;
        if (!in || t >= n_t) continue;
        const size_t cell = (size_t)t * (size_t)P + (size_t)p;
        const bool evaluated = tum[j].ok && ref <= 3u;
        unsigned short *__restrict__ eo = elig_out + cell;
        uint4 *__restrict__ go = (uint4 *)(ge_out + cell * 8);
        unsigned short v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // [base][strand]
        if (accumulate) {
            const uint4 old = *go;
            const unsigned w[4] = {old.x, old.y, old.z, old.w};
#pragma unroll
            for (int b = 0; b < 4; ++b) { v[2 * b] = (unsigned short)w[b]; v[2 * b + 1] = (unsigned short)(w[b] >> 16); }
            *eo = (unsigned short)(*eo + el[j]);
        } else {
            *eo = (unsigned short)el[j];
        }
        unsigned w[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool cellok = evaluated && (unsigned)b != ref;
            const unsigned lo = cellok ? (unsigned short)(v[2 * b] + ge[j][b]) : AMPLI_EXCEEDANCE_NA;
            const unsigned hi = cellok ? (unsigned short)(v[2 * b + 1] + ge[j][4 + b]) : AMPLI_EXCEEDANCE_NA;
            w[b] = lo | hi << 16;
        }
        *go = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_exceedance_records(ampli_ctx *ctx, const ampli_records *recs_t, const ampli_records *recs_n, int64_t P, const uint8_t *d_ref_code,
                                        int32_t normal_cutoff, int32_t calling_cutoff, int64_t first_t, int64_t first_n, int32_t skip_same_index,
                                        int32_t accumulate, uint16_t *d_elig, uint16_t *d_ge)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort ct, cn;
    { int rc = cohort_from_records(ctx, recs_t, P, ct); if (rc) return rc; }
    { int rc = cohort_from_records(ctx, recs_n, P, cn); if (rc) return rc; }
    if (P <= 0 || normal_cutoff < 0 || calling_cutoff < 0 || first_t < 0 || first_n < 0 || !d_ref_code || !d_elig || !d_ge || ((uintptr_t)d_elig & 1) != 0 ||
        ((uintptr_t)d_ge & 15) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "exceedance_records: bad argument (P > 0, normal_cutoff >= 0, calling_cutoff >= 0, first_t >= 0, first_n >= 0, d_ref_code, 2-byte "
                    "aligned d_elig, 16-byte aligned d_ge)");
    { int rc = check_records(ctx, ct, "exceedance_records (tumours)", nullptr, nullptr); if (rc) return rc; }
    { int rc = check_records(ctx, cn, "exceedance_records (normals)", nullptr, nullptr); if (rc) return rc; }
    if (first_n + (int64_t)cn.n > AMPLI_EXCEEDANCE_MAX_NORMALS)
        return fail(ctx, AMPLI_E_RANGE, "exceedance_records: first_n + n_n must be at most AMPLI_EXCEEDANCE_MAX_NORMALS (65534)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "exceedance_records: P must be below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long tiles = (P + 63) / 64, groups = ((long long)ct.n + EX_ROWS - 1) / EX_ROWS;
    constexpr long long MAX_Y = 65535; // a launch takes at most this many row groups
    for (long long g0 = 0; g0 < groups; g0 += MAX_Y) {
        const dim3 grid((unsigned)tiles, (unsigned)(groups - g0 < MAX_Y ? groups - g0 : MAX_Y));
        with_layout(ct.layout, [&](auto LT) {
            with_layout(cn.layout, [&](auto LN) {
                hipLaunchKernelGGL((exceedance_kernel<LT, LN>), grid, dim3(64 * EX_WAVES), 0, st, ct.rv, ct.n, (int)(g0 * EX_ROWS), cn.rv, cn.n, (long long)P,
                                   d_ref_code, (int)normal_cutoff, (int)calling_cutoff, (long long)(first_t - first_n), skip_same_index ? 1 : 0,
                                   accumulate ? 1 : 0, (unsigned short *)d_elig, (unsigned short *)d_ge);
            });
        });
    }
    return check_launch(ctx, "exceedance_kernel");
}
