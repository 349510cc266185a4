// amplisolve_amd/csrc/ampli_concordance.hip -- sample identity: genotype bit planes and all-pairs concordance.
//
// genotype_planes_kernel (ampli_genotype_planes_records) encodes the primary records of a resident chunk into six uint64 bit planes
// per sample; concordance_pairs_kernel (ampli_concordance_pairs) counts, for every pair of samples, five popcounts over the planes.
// The genotype of one record is ampli_genotype_classify (ampli_math.h), which the host library exports too.  Integers only.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// ==== encode: records -> planes ==========================================================================================================

constexpr int GP_WAVES = 4; // waves of a workgroup, each with a run of rows of its own

// genotype_planes_kernel<LAY>: a wave = one 64-position tile (blockIdx.x) and the rows [r0, r1) of its run, one lane per position.
// The next row's record is loaded before the current row is classified.  Each of the six predicates goes through one __ballot, which
// IS the plane's word of the tile; lanes 0..5 then store the six words of (row, tile) with one vector store.  A lane at or beyond P
// reads position P - 1 and votes 0: the partial last tile gets zero bits, never a skipped store.  Only rv.base / rv.row_stride are
// read: extra occurrences and the RD planes do not enter (ampli_math.h).  16 / 24 / 32 B read, 48 B written per record.
template <int LAY>
__global__ __launch_bounds__(64 * GP_WAVES) void genotype_planes_kernel(const RecView rv, const long long P, const int n, const int run,
                                                                        const ampli_genotype_params prm, unsigned long long *__restrict__ planes,
                                                                        const long long W)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long tile = blockIdx.x;
    const long long r0 = ((long long)blockIdx.y * GP_WAVES + wave) * run;
    const long long r1 = r0 + run < n ? r0 + run : n;
    if (r0 >= r1) return; // wave-uniform; the kernel has no barrier
    const long long p_raw = tile * 64 + lane;
    const bool on = p_raw < P;
    const long long p = on ? p_raw : P - 1;
    const char *__restrict__ q = rv.base + (size_t)p * rec_bytes(LAY);
    const size_t row_bytes = (size_t)rv.row_stride * rec_bytes(LAY);
    RawRec<LAY> cur = rec_load_at<LAY>(q + (size_t)r0 * row_bytes);
    for (long long s = r0; s < r1; ++s) {
        const RawRec<LAY> nxt = rec_load_at<LAY>(q + (size_t)(s + 1 < r1 ? s + 1 : s) * row_bytes); // in flight during this row's arithmetic
        int4 f, b;
        rec_decode<LAY>(cur, f, b);
        const int fw[4] = {f.x, f.y, f.z, f.w}, bw[4] = {b.x, b.y, b.z, b.w};
        const unsigned g = on ? ampli_genotype_classify(fw, bw, f.x != AMPLI_ABSENT, &prm) : 0u;
        unsigned long long word = 0;
#pragma unroll
        for (int k = 0; k < AMPLI_GENO_PLANES; ++k) {
            const unsigned long long w = __ballot((g >> k) & 1u);
            word = lane == k ? w : word;
        }
        if (lane < AMPLI_GENO_PLANES) planes[((size_t)s * AMPLI_GENO_PLANES + lane) * (size_t)W + (size_t)tile] = word;
        cur = nxt;
    }
}

// ==== pairs: planes x planes -> five counts per pair =====================================================================================

// The tile of a workgroup: CP_TA rows of a times CP_TB rows of b, walked over the W words in slabs of CP_SLAB words staged in LDS.
// A thread keeps CP_RA x CP_RB pairs x 5 counters: its a rows are ty * CP_RA + i (ty = thread / 32: the same for a half-wave, so an a
// operand is one broadcast ds_read_b64), its b rows tx + 32 j (tx = thread % 32: a half-wave reads 32 consecutive rows of one
// (plane, word), 256 contiguous bytes, conflict-free).
constexpr int CP_TA = 32, CP_TB = 64, CP_SLAB = 8, CP_RA = 4, CP_RB = 2, CP_THREADS = 256;
// the LDS image is [plane][word][row] with the row dimension padded by 4: the staging stores of a half-wave -- 8 consecutive words of
// 4 consecutive rows -- then fall on 32 different 8-byte bank pairs (word * 4 + row mod 32); the reads above never see the padding
constexpr int CP_PA = CP_TA + 4, CP_PB = CP_TB + 4;
static_assert(CP_TA == (CP_THREADS / 32) * CP_RA && CP_TB == 32 * CP_RB && CP_PA % 32 == 4 && CP_PB % 32 == 4, "tile shape");

// `rows` rows from row0 of one plane set, words [w0, w0 + CP_SLAB): rows at or beyond n and words at or beyond W are staged as zeros,
// so that the inner loop has no edge of any kind.  Thread t takes element t, t + 256, ...: the word runs fastest (8 consecutive
// uint64 of one (row, plane) from memory), then the row, then the plane.
template <int ROWS, int PAD>
__device__ __forceinline__ void cp_stage(unsigned long long (*__restrict__ dst)[CP_SLAB][PAD], const unsigned long long *__restrict__ planes,
                                         const long long row0, const int n, const long long w0, const long long W)
{
    for (int e = threadIdx.x; e < AMPLI_GENO_PLANES * ROWS * CP_SLAB; e += CP_THREADS) {
        const int word = e % CP_SLAB, row = (e / CP_SLAB) % ROWS, plane = e / (CP_SLAB * ROWS);
        const long long r = row0 + row, w = w0 + word;
        const bool in = r < n && w < W;
        dst[plane][word][row] = in ? planes[((size_t)r * AMPLI_GENO_PLANES + plane) * (size_t)W + (size_t)w] : 0ull;
    }
}

// concordance_pairs_kernel: blockIdx.y = a tile, blockIdx.x = b tile.  symmetric (the two plane sets are one): a tile that lies
// wholly below the diagonal leaves at once, and a thread stores a pair (i, j) with j >= i together with its mirror (j, i) -- the five
// counts are symmetric (on a matching position the presence sets are equal, so Ha == Hb) -- and no pair with j < i: every cell of
// the matrix is written exactly once, with plain vector stores.
__global__ __launch_bounds__(CP_THREADS) void concordance_pairs_kernel(const unsigned long long *__restrict__ pa, const int n_a,
                                                                       const unsigned long long *__restrict__ pb, const int n_b, const long long W,
                                                                       const int symmetric, int *__restrict__ counts)
{
    __shared__ unsigned long long sa[AMPLI_GENO_PLANES][CP_SLAB][CP_PA];
    __shared__ unsigned long long sb[AMPLI_GENO_PLANES][CP_SLAB][CP_PB];
    const long long a0 = (long long)blockIdx.y * CP_TA, b0 = (long long)blockIdx.x * CP_TB;
    if (symmetric && b0 + CP_TB - 1 < a0) return; // block-uniform, in front of every barrier
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int acc[CP_RA][CP_RB][5];
#pragma unroll
    for (int i = 0; i < CP_RA; ++i)
#pragma unroll
        for (int j = 0; j < CP_RB; ++j)
#pragma unroll
            for (int c = 0; c < 5; ++c) acc[i][j][c] = 0;
    for (long long w0 = 0; w0 < W; w0 += CP_SLAB) {
        cp_stage<CP_TA, CP_PA>(sa, pa, a0, n_a, w0, W);
        cp_stage<CP_TB, CP_PB>(sb, pb, b0, n_b, w0, W);
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < CP_SLAB; ++k) {
            unsigned long long B[CP_RB][AMPLI_GENO_PLANES];
#pragma unroll
            for (int j = 0; j < CP_RB; ++j)
#pragma unroll
                for (int pl = 0; pl < AMPLI_GENO_PLANES; ++pl) B[j][pl] = sb[pl][k][tx + 32 * j];
#pragma unroll
            for (int i = 0; i < CP_RA; ++i) {
                unsigned long long A[AMPLI_GENO_PLANES];
#pragma unroll
                for (int pl = 0; pl < AMPLI_GENO_PLANES; ++pl) A[pl] = sa[pl][k][ty * CP_RA + i];
#pragma unroll
                for (int j = 0; j < CP_RB; ++j) {
                    const unsigned long long both = A[0] & B[j][0];
                    const unsigned long long diff = (A[1] ^ B[j][1]) | (A[2] ^ B[j][2]) | (A[3] ^ B[j][3]) | (A[4] ^ B[j][4]);
                    const unsigned long long share = (A[1] & B[j][1]) | (A[2] & B[j][2]) | (A[3] & B[j][3]) | (A[4] & B[j][4]);
                    const unsigned long long match = both & ~diff;
                    acc[i][j][0] += __popcll(both);
                    acc[i][j][1] += __popcll(match);
                    acc[i][j][2] += __popcll(both & ~share);
                    acc[i][j][3] += __popcll(both & (A[5] | B[j][5]));
                    acc[i][j][4] += __popcll(match & A[5]);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < CP_RA; ++i) {
        const long long a = a0 + ty * CP_RA + i;
#pragma unroll
        for (int j = 0; j < CP_RB; ++j) {
            const long long b = b0 + tx + 32 * j;
            if (a >= n_a || b >= n_b || (symmetric && b < a)) continue;
            int *__restrict__ o = counts + ((size_t)a * (size_t)n_b + (size_t)b) * 5;
#pragma unroll
            for (int c = 0; c < 5; ++c) o[c] = acc[i][j][c];
            if (symmetric && b > a) {
                int *__restrict__ m = counts + ((size_t)b * (size_t)n_b + (size_t)a) * 5;
#pragma unroll
                for (int c = 0; c < 5; ++c) m[c] = acc[i][j][c];
            }
        }
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int64_t ampli_concordance_words(int64_t P) { return P > 0 ? (P + 63) / 64 : 0; }

extern "C" int ampli_genotype_planes_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_genotype_params *prm,
                                             uint64_t *d_planes)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_planes || ((uintptr_t)d_planes & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "genotype_planes_records: bad argument (P > 0, 8-byte aligned d_planes)");
    if (!prm || !ampli_genotype_params_ok(prm))
        return fail(ctx, AMPLI_E_INVALID,
                    "genotype_planes_records: prm must hold min_depth >= 1 and 0 <= absent_max_pm < het_min_pm <= het_max_pm < hom_min_pm <= 1000");
    { int rc = check_records(ctx, co, "genotype_planes_records", nullptr, nullptr); if (rc) return rc; }
    const long long W = (P + 63) / 64;
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "genotype_planes_records: P must be below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    // rows per wave: 16, fewer while the grid would not fill the device four times over; the grid's y stays below 65536
    const int n = co.n;
    int run = 16;
    while (run > 1 && W * ((n + GP_WAVES * run - 1) / (GP_WAVES * run)) < 4ll * ctx->n_cu) run >>= 1;
    while ((n + GP_WAVES * run - 1) / (GP_WAVES * run) > 65535) run <<= 1;
    const dim3 grid((unsigned)W, (unsigned)((n + GP_WAVES * run - 1) / (GP_WAVES * run)));
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((genotype_planes_kernel<L>), grid, dim3(64 * GP_WAVES), 0, st, co.rv, (long long)P, n, run, *prm,
                           (unsigned long long *)d_planes, W);
    });
    return check_launch(ctx, "genotype_planes_kernel");
}

extern "C" int ampli_concordance_pairs(ampli_ctx *ctx, int64_t P, const uint64_t *d_planes_a, int32_t n_a, const uint64_t *d_planes_b, int32_t n_b,
                                       int32_t *d_counts)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || !d_planes_a || !d_planes_b || !d_counts || n_a <= 0 || n_b <= 0 || (((uintptr_t)d_planes_a | (uintptr_t)d_planes_b) & 7) != 0 ||
        ((uintptr_t)d_counts & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "concordance_pairs: bad argument (P > 0, n_a > 0, n_b > 0, 8-byte aligned planes, 4-byte aligned d_counts)");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "concordance_pairs: P must be below 2^31 (the counts are int32)");
    const long long ta = ((long long)n_a + CP_TA - 1) / CP_TA, tb = ((long long)n_b + CP_TB - 1) / CP_TB;
    if (ta > 65535) return fail(ctx, AMPLI_E_RANGE, "concordance_pairs: n_a must be at most 2097120");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const int symmetric = d_planes_a == d_planes_b && n_a == n_b;
    hipLaunchKernelGGL(concordance_pairs_kernel, dim3((unsigned)tb, (unsigned)ta), dim3(CP_THREADS), 0, st, (const unsigned long long *)d_planes_a, (int)n_a,
                       (const unsigned long long *)d_planes_b, (int)n_b, (long long)((P + 63) / 64), symmetric, d_counts);
    return check_launch(ctx, "concordance_pairs_kernel");
}
