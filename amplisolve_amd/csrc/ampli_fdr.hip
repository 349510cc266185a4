// amplisolve_amd/csrc/ampli_fdr.hip -- false-discovery control: the Benjamini-Hochberg adjusted score of every cell of a
// score plane [rows][P][4][2], each row (a file, a pair) on its own, and with it the project's device sort and scan.
//
// ampli_fdr_adjust runs, per row of n = 4 P keys, on the context's stream and without a host synchronisation:
//   fdr_key_kernel      the cell keys (ampli_fdr_key, ampli_math.h: the bit pattern of the smaller strand score, 0 for a zero and
//                       for an untested cell) and m, the tested cells of the row, by integer atomics (order-free)
//   4 x { fdr_hist_kernel, fdr_hist_scan_kernel, fdr_totals_kernel, fdr_scatter_kernel }
//                       an LSD radix sort of the keys, 8 bits per pass, ascending, ping-pong between two key arrays: per-tile digit
//                       histograms [256][tiles], their exclusive scan in digit-major order (two levels: blocks of
//                       AMPLI_FDR_SCAN_BLOCK, then the block totals by ONE workgroup per row that walks them with a carry), and a
//                       STABLE scatter
//   fdr_adjust_kernel   (float)B at the first slot of every tie group of positive keys -- its rank is n - slot, known without a scan
//                       -- and -inf elsewhere, and the inclusive running maximum of that inside each scan block
//   fdr_totals_kernel   the running maximum over the blocks' totals
//   fdr_lookup_kernel   every cell finds the first slot of its key by binary search in the sorted row: R = n - slot, A = the running
//                       maximum there
// No kernel waits for another workgroup: the levels of a scan are separate launches.  A row touches its own slice of the workspace
// and nothing else, so a row's bytes do not depend on which other rows are in the batch.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_internal.h"
#include "ampli_math.h"

constexpr int FDR_THREADS = 256;
constexpr int FDR_WAVES = FDR_THREADS / 64;
constexpr int FDR_TILE = AMPLI_FDR_TILE_KEYS;
constexpr int FDR_ITEMS = FDR_TILE / FDR_THREADS; // keys of a lane in the sort kernels
constexpr int FDR_SB = AMPLI_FDR_SCAN_BLOCK;      // elements of one scan block: two per thread
constexpr int FDR_BINS = 256;
static_assert(FDR_SB == 2 * FDR_THREADS, "a scan block is two elements per thread");
static_assert(FDR_TILE % FDR_THREADS == 0 && FDR_BINS == FDR_THREADS, "one thread per digit bin");

// where a row's arrays live: base + row * stride + off*.  keys_a holds the keys before pass 0 and the sorted row after pass 3; keys_b
// is the other side of the ping-pong and, after the sort, the running maxima (float) per sorted slot.
struct FdrWs {
    char *base;
    size_t stride, off_a, off_b, off_hist, off_tot;
    int n, tiles, hist_len, nb_hist, nb_adj;
};

static bool fdr_layout(int32_t rows, int64_t P, FdrWs &w)
{
    if (rows < 1 || P <= 0 || P >= (1ll << 29)) return false;
    const long long n = 4 * P;
    w.n = (int)n;
    w.tiles = (int)((n + FDR_TILE - 1) / FDR_TILE);
    w.hist_len = w.tiles * FDR_BINS;
    w.nb_hist = (w.hist_len + FDR_SB - 1) / FDR_SB;
    w.nb_adj = (int)((n + FDR_SB - 1) / FDR_SB);
    const auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    w.off_a = 0;
    w.off_b = w.off_a + up((size_t)n * 4);
    w.off_hist = w.off_b + up((size_t)n * 4);
    w.off_tot = w.off_hist + up((size_t)w.hist_len * 4);
    w.stride = w.off_tot + up((size_t)(w.nb_hist > w.nb_adj ? w.nb_hist : w.nb_adj) * 4);
    w.base = nullptr;
    return true;
}

template <typename T>
__device__ __forceinline__ T *fdr_row(const FdrWs &w, const size_t off)
{
    return (T *)(w.base + (size_t)blockIdx.y * w.stride + off);
}

struct FdrSum {
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a + b; }
};
struct FdrMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return a > b ? a : b; }
};

// the scan of one block of FDR_SB elements, two per thread in order: returns what lies before the thread's pair (exclusive), *total
// = the whole block.  Hillis-Steele over the threads' pair totals in LDS; every thread of the workgroup calls it.
template <typename T, typename Op>
__device__ __forceinline__ T fdr_block_scan(const T x0, const T x1, const T identity, const Op op, T *total)
{
    __shared__ T buf[2][FDR_THREADS];
    const int t = threadIdx.x;
    __syncthreads(); // the buffer may still be read by the previous call
    buf[0][t] = op(x0, x1);
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < FDR_THREADS; d <<= 1) {
        const T v = buf[cur][t];
        buf[cur ^ 1][t] = t >= d ? op(buf[cur][t - d], v) : v;
        cur ^= 1;
        __syncthreads();
    }
    *total = buf[cur][FDR_THREADS - 1];
    return t ? buf[cur][t - 1] : identity;
}

// fdr_key_kernel: blockIdx.x = FDR_KEY_POS positions, taken in rounds of 256, a lane a position, blockIdx.y = row.  Two 16-byte loads
// and one 16-byte store of four keys per position; the workgroup's tested cells are added up across lanes and waves and go to
// d_m[row] in ONE integer atomic (integer addition is order-free: the same bytes every run).  With an atomic per wave the 1563 waves of
// a row of 100 000 positions queued on one address, and the kernel took 0.78 ms where the traffic asks for 0.1.  A lane at
// or beyond P loads and stores nothing.
constexpr int FDR_KEY_POS = 8 * FDR_THREADS;
__global__ __launch_bounds__(FDR_THREADS) void fdr_key_kernel(const float *__restrict__ d_s, const long long P, const int two_sided, const FdrWs w,
                                                              int *__restrict__ d_m)
{
    __shared__ int wave_sum[FDR_WAVES];
    int tested = 0;
    for (int j = 0; j < FDR_KEY_POS / FDR_THREADS; ++j) {
        const long long p = (long long)blockIdx.x * FDR_KEY_POS + j * FDR_THREADS + threadIdx.x;
        if (p >= P) break;
        const float4 *src = (const float4 *)(d_s + ((size_t)blockIdx.y * (size_t)P + (size_t)p) * 8);
        const float4 v0 = src[0], v1 = src[1];
        int c0, c1, c2, c3;
        uint4 k;
        k.x = ampli_fdr_key(v0.x, v0.y, two_sided, &c0);
        k.y = ampli_fdr_key(v0.z, v0.w, two_sided, &c1);
        k.z = ampli_fdr_key(v1.x, v1.y, two_sided, &c2);
        k.w = ampli_fdr_key(v1.z, v1.w, two_sided, &c3);
        tested += (c0 != AMPLI_FDR_UNTESTED) + (c1 != AMPLI_FDR_UNTESTED) + (c2 != AMPLI_FDR_UNTESTED) + (c3 != AMPLI_FDR_UNTESTED);
        ((uint4 *)fdr_row<unsigned>(w, w.off_a))[p] = k;
    }
    for (int d = 32; d > 0; d >>= 1) tested += __shfl_xor(tested, d); // every lane is back here: the loop only ends early
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = tested;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int v = 0; v < FDR_WAVES; ++v) total += wave_sum[v];
        if (total) atomicAdd(&d_m[blockIdx.y], total);
    }
}

// fdr_hist_kernel: blockIdx.x = tile of FDR_TILE keys; the tile's digit histogram to hist[digit][tile] (digit-major: the order in
// which the scan turns counts into offsets).  Keys at or beyond n are not loaded.
__global__ __launch_bounds__(FDR_THREADS) void fdr_hist_kernel(const FdrWs w, const size_t off_in, const int shift)
{
    __shared__ unsigned h[FDR_BINS];
    const unsigned *__restrict__ in = fdr_row<unsigned>(w, off_in);
    unsigned *__restrict__ hist = fdr_row<unsigned>(w, w.off_hist);
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * FDR_TILE;
    for (int j = 0; j < FDR_ITEMS; ++j) {
        const long long i = base + j * FDR_THREADS + threadIdx.x;
        if (i < w.n) atomicAdd(&h[(in[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * w.tiles + blockIdx.x] = h[threadIdx.x];
}

// fdr_hist_scan_kernel: blockIdx.x = scan block of the row's hist[digit][tile] array: the exclusive sum inside the block, in place,
// and the block's total to tot[block]
__global__ __launch_bounds__(FDR_THREADS) void fdr_hist_scan_kernel(const FdrWs w)
{
    unsigned *__restrict__ hist = fdr_row<unsigned>(w, w.off_hist);
    unsigned *__restrict__ tot = fdr_row<unsigned>(w, w.off_tot);
    const int e = (int)blockIdx.x * FDR_SB + 2 * (int)threadIdx.x;
    const unsigned x0 = e < w.hist_len ? hist[e] : 0u, x1 = e + 1 < w.hist_len ? hist[e + 1] : 0u;
    unsigned total;
    const unsigned before = fdr_block_scan(x0, x1, 0u, FdrSum(), &total);
    if (e < w.hist_len) hist[e] = before;
    if (e + 1 < w.hist_len) hist[e + 1] = before + x0;
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// fdr_totals_kernel: ONE workgroup per row turns the nb block totals into what lies before each block (exclusive), in place, FDR_SB
// totals at a time with a carry -- the second level of both scans
template <typename T, typename Op>
__global__ __launch_bounds__(FDR_THREADS) void fdr_totals_kernel(const FdrWs w, const int nb, const T identity)
{
    T *__restrict__ tot = fdr_row<T>(w, w.off_tot);
    const Op op;
    T carry = identity;
    for (int c0 = 0; c0 < nb; c0 += FDR_SB) {
        const int e = c0 + 2 * (int)threadIdx.x;
        const T x0 = e < nb ? tot[e] : identity, x1 = e + 1 < nb ? tot[e + 1] : identity;
        T total;
        const T before = op(carry, fdr_block_scan(x0, x1, identity, op, &total));
        if (e < nb) tot[e] = before;
        if (e + 1 < nb) tot[e + 1] = op(before, x0);
        carry = op(carry, total);
    }
}

// fdr_scatter_kernel: blockIdx.x = tile.  Wave v owns the tile's keys [v * 64 * FDR_ITEMS, (v + 1) * 64 * FDR_ITEMS) and takes them
// in FDR_ITEMS rounds of 64 consecutive keys, a lane a key, so the order of the tile is (wave, round, lane).  In a round the lanes
// that hold the same digit find each other with eight ballots; a key's place among the wave's keys of its digit is the wave's count
// so far (cnt[wave][digit], LDS) plus the matching lanes below it, and the lowest matching lane adds the group to the count: stable
// inside the wave.  Thread d then turns cnt[.][d] into the waves' first output slots -- the tile's offset of digit d (the scanned
// histogram plus its block's carry) plus the counts of the waves before -- which makes it stable across waves and tiles.  Keys at
// or beyond n are neither loaded nor stored.
__global__ __launch_bounds__(FDR_THREADS) void fdr_scatter_kernel(const FdrWs w, const size_t off_in, const size_t off_out, const int shift)
{
    __shared__ unsigned cnt[FDR_WAVES][FDR_BINS];
    const unsigned *__restrict__ in = fdr_row<unsigned>(w, off_in);
    unsigned *__restrict__ out = fdr_row<unsigned>(w, off_out);
    const unsigned *__restrict__ hist = fdr_row<unsigned>(w, w.off_hist);
    const unsigned *__restrict__ tot = fdr_row<unsigned>(w, w.off_tot);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int v = 0; v < FDR_WAVES; ++v) cnt[v][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * FDR_TILE + (long long)wave * (64 * FDR_ITEMS) + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned key[FDR_ITEMS], place[FDR_ITEMS];
#pragma unroll
    for (int j = 0; j < FDR_ITEMS; ++j) {
        const long long i = base + j * 64;
        const bool valid = i < w.n;
        key[j] = valid ? in[i] : 0u;
        const unsigned d = (key[j] >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long has = __ballot(bit);
            same &= bit ? has : ~has;
        }
        const unsigned mine = (unsigned)__popcll(same & below);
        unsigned so_far = 0;
        if (valid) so_far = cnt[wave][d];
        __builtin_amdgcn_wave_barrier(); // every lane of the group has read the count before its lowest lane replaces it
        if (valid && mine == 0) cnt[wave][d] = so_far + (unsigned)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        place[j] = so_far + mine;
    }
    __syncthreads();
    {
        const int e = (int)threadIdx.x * w.tiles + (int)blockIdx.x;
        unsigned run = hist[e] + tot[e / FDR_SB];
        for (int v = 0; v < FDR_WAVES; ++v) {
            const unsigned c = cnt[v][threadIdx.x];
            cnt[v][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FDR_ITEMS; ++j) {
        const long long i = base + j * 64;
        if (i < w.n) {
            const unsigned slot = cnt[wave][(key[j] >> shift) & 255u] + place[j];
            if (slot < (unsigned)w.n) out[slot] = key[j]; // a slot is below n by construction; the test costs nothing
        }
    }
}

// fdr_adjust_kernel: blockIdx.x = scan block of the sorted row.  The first slot i of a tie group of positive keys carries
// (float)ampli_fdr_value(key, m, n - i) -- every key from slot i on is at least this one, and all of them are tested -- every other
// slot -inf; the inclusive running maximum inside the block goes to amax[slot], the block's to tot[block].  m comes from device memory.
__global__ __launch_bounds__(FDR_THREADS) void fdr_adjust_kernel(const FdrWs w, const int two_sided, const int *__restrict__ d_m)
{
    const unsigned *__restrict__ sorted = fdr_row<unsigned>(w, w.off_a);
    float *__restrict__ amax = fdr_row<float>(w, w.off_b);
    float *__restrict__ tot = fdr_row<float>(w, w.off_tot);
    const int m = d_m[blockIdx.y];
    const long long i0 = (long long)blockIdx.x * FDR_SB + 2 * (long long)threadIdx.x;
    float x[2];
    unsigned prev = i0 > 0 && i0 - 1 < w.n ? sorted[i0 - 1] : 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long i = i0 + j;
        x[j] = -INFINITY;
        if (i < w.n) {
            const unsigned k = sorted[i];
            if (k != 0u && (i == 0 || k != prev)) x[j] = (float)ampli_fdr_value(k, m, (int32_t)(w.n - i), two_sided);
            prev = k;
        }
    }
    float total;
    const float before = fdr_block_scan(x[0], x[1], -INFINITY, FdrMax(), &total);
    const FdrMax mx;
    if (i0 < w.n) amax[i0] = mx(before, x[0]);
    if (i0 + 1 < w.n) amax[i0 + 1] = mx(mx(before, x[0]), x[1]);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// fdr_lookup_kernel: blockIdx.x = 256 positions, a lane a position.  The cell's class and key again from d_s (32 bytes a position,
// cheaper than a class array written and read); a positive key finds the first slot of its tie group by binary search in the sorted
// row (about log2(4 P) steps on a row that lies in L2): R = n - slot, A = the running maximum there.  A lane at or beyond P loads
// and stores nothing.
__global__ __launch_bounds__(FDR_THREADS) void fdr_lookup_kernel(const float *__restrict__ d_s, const long long P, const int two_sided, const FdrWs w,
                                                                 float *__restrict__ d_a, int *__restrict__ d_rank)
{
    const long long p = (long long)blockIdx.x * FDR_THREADS + threadIdx.x;
    if (p >= P) return;
    const unsigned *__restrict__ sorted = fdr_row<unsigned>(w, w.off_a);
    const float *__restrict__ amax = fdr_row<float>(w, w.off_b);
    const float *__restrict__ tot = fdr_row<float>(w, w.off_tot);
    const size_t cell = ((size_t)blockIdx.y * (size_t)P + (size_t)p);
    const float4 *src = (const float4 *)(d_s + cell * 8);
    const float4 v0 = src[0], v1 = src[1];
    const float sf[4] = {v0.x, v0.z, v1.x, v1.z}, sb[4] = {v0.y, v0.w, v1.y, v1.w};
    float a[4];
    int r[4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        int cls;
        const unsigned k = ampli_fdr_key(sf[y], sb[y], two_sided, &cls);
        float bmax = 0.0f;
        r[y] = 0;
        if (k != 0u) {
            int lo = 0, hi = w.n; // the first slot whose key is not below k: it exists, the cell's own key is in the row
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (sorted[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            if (lo < w.n) {
                const float in_block = amax[lo], carried = tot[lo / FDR_SB];
                bmax = in_block > carried ? in_block : carried;
                r[y] = w.n - lo;
            }
        }
        a[y] = ampli_fdr_store(cls, bmax);
    }
    ((float4 *)d_a)[cell] = make_float4(a[0], a[1], a[2], a[3]);
    if (d_rank) ((int4 *)d_rank)[cell] = make_int4(r[0], r[1], r[2], r[3]);
}

// ==== C ABI ==============================================================================================================================

extern "C" size_t ampli_fdr_workspace_bytes(int32_t rows, int64_t P)
{
    FdrWs w;
    return fdr_layout(rows, P, w) ? (size_t)rows * w.stride : 0;
}

extern "C" int ampli_fdr_adjust(ampli_ctx *ctx, const float *d_s, int32_t rows, int64_t P, int32_t two_sided, void *d_work, size_t work_bytes, float *d_a,
                                int32_t *d_m, int32_t *d_rank)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_s || !d_a || !d_m || !d_work || rows < 1 || P <= 0 || (two_sided != 0 && two_sided != 1) || ((uintptr_t)d_s & 15) != 0 ||
        ((uintptr_t)d_a & 15) != 0 || ((uintptr_t)d_work & 15) != 0 || ((uintptr_t)d_m & 3) != 0 || ((uintptr_t)d_rank & 15) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "fdr_adjust: bad argument (rows >= 1, P > 0, two_sided 0 or 1, 16-byte aligned d_s, d_a, d_work and d_rank, 4-byte aligned d_m)");
    if (P >= (1ll << 29)) return fail(ctx, AMPLI_E_RANGE, "fdr_adjust: 4 P must be below 2^31");
    FdrWs w;
    fdr_layout(rows, P, w);
    if (work_bytes < (size_t)rows * w.stride) return fail(ctx, AMPLI_E_INVALID, "fdr_adjust: the workspace is smaller than ampli_fdr_workspace_bytes(rows, P)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    HIP_TRY(ctx, hipMemsetAsync(d_m, 0, (size_t)rows * sizeof(int32_t), st));
    const dim3 tb(FDR_THREADS);
    const unsigned pos_blocks = (unsigned)((P + FDR_THREADS - 1) / FDR_THREADS), key_blocks = (unsigned)((P + FDR_KEY_POS - 1) / FDR_KEY_POS);
    constexpr int MAX_Y = 65535; // a launch takes at most this many rows
    for (int r0 = 0; r0 < rows; r0 += MAX_Y) {
        const unsigned ny = (unsigned)(rows - r0 < MAX_Y ? rows - r0 : MAX_Y);
        w.base = (char *)d_work + (size_t)r0 * w.stride;
        const float *s = d_s + (size_t)r0 * (size_t)P * 8;
        int *m = d_m + r0;
        hipLaunchKernelGGL(fdr_key_kernel, dim3(key_blocks, ny), tb, 0, st, s, (long long)P, (int)two_sided, w, m);
        size_t in = w.off_a, out = w.off_b;
        for (int shift = 0; shift < 32; shift += 8) {
            hipLaunchKernelGGL(fdr_hist_kernel, dim3((unsigned)w.tiles, ny), tb, 0, st, w, in, shift);
            hipLaunchKernelGGL(fdr_hist_scan_kernel, dim3((unsigned)w.nb_hist, ny), tb, 0, st, w);
            hipLaunchKernelGGL((fdr_totals_kernel<unsigned, FdrSum>), dim3(1, ny), tb, 0, st, w, w.nb_hist, 0u);
            hipLaunchKernelGGL(fdr_scatter_kernel, dim3((unsigned)w.tiles, ny), tb, 0, st, w, in, out, shift);
            const size_t t = in; in = out; out = t;
        }
        // four passes: the sorted row is back in keys_a, keys_b is free for the running maxima
        hipLaunchKernelGGL(fdr_adjust_kernel, dim3((unsigned)w.nb_adj, ny), tb, 0, st, w, (int)two_sided, (const int *)m);
        hipLaunchKernelGGL((fdr_totals_kernel<float, FdrMax>), dim3(1, ny), tb, 0, st, w, w.nb_adj, -INFINITY);
        hipLaunchKernelGGL(fdr_lookup_kernel, dim3(pos_blocks, ny), tb, 0, st, s, (long long)P, (int)two_sided, w, d_a + (size_t)r0 * (size_t)P * 4,
                           d_rank ? d_rank + (size_t)r0 * (size_t)P * 4 : (int *)nullptr);
    }
    return check_launch(ctx, "fdr_adjust");
}
