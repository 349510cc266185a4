// amplisolve_amd/csrc/ampli_amplicon_count.hip -- amplicon_count_kernel + ampli_pileup_amplicon_count and amplicon_layers_kernel +
// ampli_amplicon_layers (include/amplisolve_hip.h): the third walk over the alignment records of a BAM file, the counting half of
// computeAmpliconCounts; the container half is csrc/host/bam.cpp, the command csrc/host/run_ca.cpp.  ampli_pileup.hip pools
// every read over a position; this unit first decides which amplicon a read came from and counts it there only.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ampli_bam.h"    // the record layout, the keys and their searches
#include "ampli_device.h" // with_bool, the launch dispatch
#include "ampli_internal.h"

// ---------------------------------------------------------------------------
// amplicon_count: per walk entry w = amp_off[a] + (x - first[a]) -- "position x as seen by amplicon a" -- the bases of the reads ASSIGNED
// to amplicon a (the definition: include/amplisolve_hip.h, ampli_pileup_amplicon_count).
// Shape of indel_count_kernel (ampli_indel.hip): a workgroup takes AMPCOUNT_READS consecutive reads, one wave per read at a time, the
// records read straight from global memory.  The assignment is wave-uniform: every lane walks the same CIGAR for the span, the two
// binary searches give the candidate range, the candidates are dealt to the lanes in rounds of 64 and one (overlap, anchor distance,
// index) key is reduced across the wave.  Then the columns of every match run are dealt to the lanes; the cell is arithmetic, there is no
// key search per column.
// Counters: an LDS window of AMPCOUNT_WINDOW consecutive walk entries x 8 that starts at the walk entry the workgroup's first assigned
// read begins in, flushed with one global atomic per non-zero counter; whatever falls outside it (unsorted files, a read assigned far
// from the first one, amplicons longer than the window) goes to the global counters directly.  The reads of a wave that follow each
// other on one amplicon and strand share one atomic on amp_reads.
// ---------------------------------------------------------------------------
constexpr int AMPCOUNT_READS = 256;
constexpr int AMPCOUNT_WINDOW = 512;

struct ampcount_hit { // the amplicon a read is assigned to: its sorted index, its interval and its first walk entry
    long long a, first, last, off;
};

// The amplicon of a kept read; false: none (R = 0, no overlap, or an overlap under the threshold).  Wave-uniform, every lane returns the
// same.  c0, c1: the candidate range of the wave's previous read, tried first -- the reads of an amplicon follow each other, and four
// independent loads say whether the range still holds, where the two searches are eighteen dependent ones.  Start with c0 = -1.
__device__ __forceinline__ bool ampcount_assign(const BamRead &h, const int lane, const unsigned long long *__restrict__ lo,
                                                const unsigned long long *__restrict__ hi, const unsigned long long *__restrict__ reach,
                                                const long long *__restrict__ amp_off, const long long A, const int min_overlap, long long &c0,
                                                long long &c1, ampcount_hit &hit)
{
    long long R = 0; // reference positions the alignment spans: M = X D N
    for (int c = 0; c < h.n_cigar; ++c) {
        // bam_cigar and bam_op_match || bam_op_ref of ampli_bam.h, written out: with the helpers this loop -- a chain of dependent loads in
        // front of every read's assignment -- made the kernel 1.3 % slower (profiles/bam_walks)
        const unsigned op_len = bam_u32()(h.cig + 4 * (size_t)c);
        const unsigned op = op_len & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) R += (long long)(op_len >> 4);
    }
    if (R == 0) return false;
    const long long sf = h.pos + 1, sl = h.pos + R; // 1-based, inclusive
    const unsigned long long ref_hi = bam_key(h.ref_id, 0);
    // (a span that runs past 2^32 - 1 is searched with its end at 2^32 - 1: no amplicon starts behind that)
    const unsigned long long kf = ref_hi | (unsigned long long)sf, kl = ref_hi | (unsigned long long)(sl < 0xffffffffll ? sl : 0xffffffffll);
    // c0: the first a with reach[a] >= span_first (A if none); c1: the last a with lo[a] <= span_last (-1 if none)
    bool ok0 = false, ok1 = false;
    if (c0 >= 0) { // (then 0 <= c0 <= A and -1 <= c1 < A: they are an earlier read's answers)
        const unsigned long long r0 = reach[c0 < A ? c0 : A - 1], r0m = reach[c0 > 0 ? c0 - 1 : 0];
        const unsigned long long l1 = lo[c1 >= 0 ? c1 : 0], l1p = lo[c1 + 1 < A ? c1 + 1 : A - 1];
        ok0 = (c0 == A || r0 >= kf) && (c0 == 0 || r0m < kf);
        ok1 = (c1 < 0 || l1 <= kl) && (c1 + 1 == A || l1p > kl);
    }
    if (!ok0) c0 = bam_lower<long long>(reach, 0, A, kf);
    if (!ok1) c1 = bam_upper<long long>(lo, 0, A, kl) - 1;
    // the key: largest overlap, then smallest anchor distance, then lowest index
    long long b_ov = -1, b_an = 0, b_a = -1, b_first = 0, b_last = 0, b_off = 0;
    for (long long a0 = c0; a0 <= c1; a0 += 64) {
        const long long a = a0 + lane;
        if (a > c1) continue;
        const unsigned long long l = lo[a], u = hi[a];
        const long long off = amp_off[a];
        const long long first = (long long)(l & 0xffffffffull), last = (long long)(u & 0xffffffffull);
        long long ov = 0, an = 0;
        if ((l >> 32) == (unsigned long long)(unsigned)h.ref_id) {
            ov = (sl < last ? sl : last) - (sf > first ? sf : first) + 1;
            if (ov < 0) ov = 0;
            an = h.rev ? sl - last : sf - first;
            if (an < 0) an = -an;
        }
        if (ov > b_ov || (ov == b_ov && an < b_an)) { // (a grows within a lane: an equal key keeps the lower index)
            b_ov = ov;
            b_an = an;
            b_a = a;
            b_first = first;
            b_last = last;
            b_off = off;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const long long o_ov = __shfl_xor(b_ov, d, 64), o_an = __shfl_xor(b_an, d, 64), o_a = __shfl_xor(b_a, d, 64);
        if (o_ov > b_ov || (o_ov == b_ov && (o_an < b_an || (o_an == b_an && o_a < b_a)))) {
            b_ov = o_ov;
            b_an = o_an;
            b_a = o_a;
        }
    }
    if (b_ov < 1 || b_ov * 100 < (long long)min_overlap * R) return false;
    const int owner = (int)((b_a - c0) & 63); // the lane that met the winner holds it as its own best: its interval and offset come from there
    hit.a = b_a;
    hit.first = __shfl(b_first, owner, 64);
    hit.last = __shfl(b_last, owner, 64);
    hit.off = __shfl(b_off, owner, 64);
    return true;
}

__device__ __forceinline__ unsigned long long ampcount_wave_sum(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool STATS>
__global__ __launch_bounds__(256) void amplicon_count_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                             const long long n_reads, const unsigned long long *__restrict__ lo,
                                                             const unsigned long long *__restrict__ hi, const unsigned long long *__restrict__ reach,
                                                             const long long *__restrict__ amp_off, const long long A, const long long W, const int mbq,
                                                             const int mrq, const int min_overlap, int *__restrict__ counts,
                                                             unsigned long long *__restrict__ amp_reads, unsigned long long *__restrict__ stats)
{
    __shared__ int win[AMPCOUNT_WINDOW * 8]; // [window entry][slot]
    __shared__ long long win_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first = (long long)blockIdx.x * AMPCOUNT_READS;
    const long long end = first + AMPCOUNT_READS < n_reads ? first + AMPCOUNT_READS : n_reads;
    for (int i = threadIdx.x; i < AMPCOUNT_WINDOW * 8; i += 256) win[i] = 0;
    long long c0 = -1, c1 = -1; // the candidate range of the wave's previous read
    if (wave == 0) { // the window starts at the walk entry the workgroup's first assigned read begins in
        long long wb = 0;
        for (long long rd = first; rd < end; ++rd) {
            BamRead h;
            if (!bam_read_header<bam_u32>(bam + rec_off[rd] + 4, mrq, h)) continue;
            ampcount_hit hit;
            if (!ampcount_assign(h, lane, lo, hi, reach, amp_off, A, min_overlap, c0, c1, hit)) continue;
            wb = hit.off + (h.pos + 1 > hit.first ? h.pos + 1 - hit.first : 0);
            break;
        }
        if (lane == 0) win_base = wb;
    }
    __syncthreads();
    const long long wb = win_base;
    unsigned long long kept = 0, assigned = 0, added = 0, clipped = 0; // kept, assigned, clipped: wave-uniform; added: per lane
    long long run_a = -1; // the amplicon and strand of the wave's latest assigned reads, and how many of them are not yet in amp_reads
    int run_rev = 0;
    unsigned long long run_n = 0;
    for (long long read = first + wave; read < end; read += 4) {
        BamRead h;
        if (!bam_read_header<bam_u32>(bam + rec_off[read] + 4, mrq, h)) continue;
        ++kept;
        ampcount_hit hit;
        if (!ampcount_assign(h, lane, lo, hi, reach, amp_off, A, min_overlap, c0, c1, hit)) continue; // off-target: in the statistics and nowhere else
        ++assigned;
        const long long a = hit.a;
        if (a != run_a || h.rev != run_rev) {
            if (run_n && lane == 0) atomicAdd(&amp_reads[run_a * 2 + run_rev], run_n);
            run_a = a;
            run_rev = h.rev;
            run_n = 0;
        }
        ++run_n;
        const long long af = hit.first, al = hit.last;
        const long long cell0 = hit.off - af; // walk entry of position x: cell0 + x
        long long refpos = h.pos + 1;            // 1-based position of the next column
        long long qpos = 0;
        for (int c = 0; c < h.n_cigar; ++c) {
            const BamOp o = bam_cigar<bam_u32>(h.cig, c);
            const long long len = o.len;
            if (bam_op_match(o.op)) { // a match run: M, =, X; its columns refpos .. refpos + len - 1, those inside [af, al] are counted
                const long long j0 = af > refpos ? af - refpos : 0;
                const long long j1 = al - refpos + 1 < len ? al - refpos + 1 : len; // exclusive
                const long long inside = j1 > j0 ? j1 - j0 : 0;
                clipped += (unsigned long long)(len - inside);
                for (long long j = j0 + lane; j < j1; j += 64) {
                    const long long q = qpos + j;
                    const int nt = bam_nt(h.seq, q);
                    if (nt < 0 || (int)h.qual[q] < mbq) continue;
                    const long long w = cell0 + refpos + j; // in [amp_off[a], amp_off[a + 1]): j0 <= j < j1
                    const long long rel = w - wb;
                    if (rel >= 0 && rel < AMPCOUNT_WINDOW) {
                        atomicAdd(&win[rel * 8 + nt], 1);
                        if (h.rev) atomicAdd(&win[rel * 8 + 4 + nt], 1);
                    } else {
                        atomicAdd(&counts[w * 8 + nt], 1);
                        if (h.rev) atomicAdd(&counts[w * 8 + 4 + nt], 1);
                    }
                    ++added;
                }
                refpos += len;
                qpos += len;
            } else if (bam_op_query(o.op)) { // I, S
                qpos += len;
            } else if (bam_op_ref(o.op)) { // D, N
                refpos += len;
            } // H, P: neither
        }
    }
    if (run_n && lane == 0) atomicAdd(&amp_reads[run_a * 2 + run_rev], run_n);
    __syncthreads();
    for (int i = threadIdx.x; i < AMPCOUNT_WINDOW * 8; i += 256) {
        const int v = win[i];
        if (v != 0 && wb + (i >> 3) < W) atomicAdd(&counts[(wb + (i >> 3)) * 8 + (i & 7)], v);
    }
    if (STATS) {
        added = ampcount_wave_sum(added);
        if (lane == 0) {
            if (kept) atomicAdd(&stats[0], kept);         // reads kept
            if (assigned) atomicAdd(&stats[1], assigned); // reads assigned
            if (added) atomicAdd(&stats[2], added);       // bases counted
            if (clipped) atomicAdd(&stats[3], clipped);   // bases clipped
        }
    }
}

// ---------------------------------------------------------------------------
// amplicon_layers: the gather behind the walk.  One lane per listed position: the same candidate search, then a scan of the candidates in
// sorted order.  The l-th covering amplicon's record goes to layer l < L, the sum of all of them to total; every output cell has one
// owner and is overwritten.  No atomics, no LDS.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void amplicon_layers_kernel(const int *__restrict__ counts, const unsigned long long *__restrict__ lo,
                                                              const unsigned long long *__restrict__ hi, const unsigned long long *__restrict__ reach,
                                                              const long long *__restrict__ amp_off, const long long A,
                                                              const unsigned long long *__restrict__ keys, const long long P, const int L,
                                                              int *__restrict__ layers, int *__restrict__ layer_amp, int *__restrict__ total)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const unsigned long long key = keys[p];
    const long long c0 = bam_lower<long long>(reach, 0, A, key), c1 = bam_upper<long long>(lo, 0, A, key) - 1;
    int4 t0 = make_int4(0, 0, 0, 0), t1 = make_int4(0, 0, 0, 0);
    int l = 0;
    for (long long a = c0; a <= c1; ++a) {
        if (hi[a] < key) continue; // (lo[a] <= key: a <= c1)
        const long long w = amp_off[a] + (long long)(key - lo[a]);
        const int4 r0 = *(const int4 *)(counts + w * 8), r1 = *(const int4 *)(counts + w * 8 + 4);
        t0.x += r0.x; t0.y += r0.y; t0.z += r0.z; t0.w += r0.w;
        t1.x += r1.x; t1.y += r1.y; t1.z += r1.z; t1.w += r1.w;
        if (l < L) {
            int *o = layers + ((long long)l * P + p) * 8;
            *(int4 *)o = r0;
            *(int4 *)(o + 4) = r1;
            layer_amp[(long long)l * P + p] = (int)a;
        }
        ++l;
    }
    for (; l < L; ++l) { // no such amplicon: the absent-record marker
        int *o = layers + ((long long)l * P + p) * 8;
        *(int4 *)o = make_int4(INT_MIN, 0, 0, 0);
        *(int4 *)(o + 4) = make_int4(0, 0, 0, 0);
        layer_amp[(long long)l * P + p] = -1;
    }
    *(int4 *)(total + p * 8) = t0;
    *(int4 *)(total + p * 8 + 4) = t1;
}

extern "C" int ampli_pileup_amplicon_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_lo,
                                           const uint64_t *d_hi, const uint64_t *d_reach, const int64_t *d_amp_off, int64_t A, int64_t W, int32_t mbq,
                                           int32_t mrq, int32_t min_overlap, int32_t *d_counts, int64_t *d_amp_reads, uint64_t *d_stats)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_bam || !d_rec_off || n_reads < 0 || !d_lo || !d_hi || !d_reach || !d_amp_off || A < 0 || W < 0 || !d_counts || !d_amp_reads)
        return fail(ctx, AMPLI_E_INVALID, "pileup_amplicon_count: bad argument");
    if ((((uintptr_t)d_rec_off | (uintptr_t)d_lo | (uintptr_t)d_hi | (uintptr_t)d_reach | (uintptr_t)d_amp_off | (uintptr_t)d_amp_reads | (uintptr_t)d_stats) & 7) != 0 ||
        ((uintptr_t)d_counts & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "pileup_amplicon_count: bad argument (8-byte aligned d_rec_off, d_lo, d_hi, d_reach, d_amp_off, d_amp_reads and d_stats, 4-byte aligned "
                    "d_counts)");
    if (min_overlap < 1 || min_overlap > 100) return fail(ctx, AMPLI_E_INVALID, "pileup_amplicon_count: min_overlap must lie in 1 .. 100");
    if (W > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "pileup_amplicon_count: 2^31 walk entries or more");
    if ((n_reads + AMPCOUNT_READS - 1) / AMPCOUNT_READS > 0x7fffffffll)
        return fail(ctx, AMPLI_E_RANGE, "pileup_amplicon_count: too many reads in one call; split the batch");
    if (A == 0 || n_reads == 0) return AMPLI_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((n_reads + AMPCOUNT_READS - 1) / AMPCOUNT_READS)); // 1-D over groups of reads
    with_bool(d_stats != nullptr, [&](auto with_stats) {
        hipLaunchKernelGGL(amplicon_count_kernel<decltype(with_stats)::value>, grid, dim3(256), 0, main_stream(ctx), (const unsigned char *)d_bam,
                           (const unsigned long long *)d_rec_off, (long long)n_reads, (const unsigned long long *)d_lo, (const unsigned long long *)d_hi,
                           (const unsigned long long *)d_reach, (const long long *)d_amp_off, (long long)A, (long long)W, (int)mbq, (int)mrq,
                           (int)min_overlap, d_counts, (unsigned long long *)d_amp_reads, (unsigned long long *)d_stats);
    });
    return check_launch(ctx, "amplicon_count_kernel");
}

extern "C" int ampli_amplicon_layers(ampli_ctx *ctx, const int32_t *d_counts, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_reach,
                                     const int64_t *d_amp_off, int64_t A, int64_t W, const uint64_t *d_keys, int64_t P, int32_t L, int32_t *d_layers,
                                     int32_t *d_layer_amp, int32_t *d_total)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_counts || !d_lo || !d_hi || !d_reach || !d_amp_off || A < 0 || W < 0 || !d_keys || P < 0 || L < 0 || (L > 0 && (!d_layers || !d_layer_amp)) ||
        !d_total)
        return fail(ctx, AMPLI_E_INVALID, "amplicon_layers: bad argument");
    // the gather loads and stores int4: d_counts, d_layers and d_total are 16-byte aligned by the contract; the other pointers are typed
    if ((((uintptr_t)d_counts | (uintptr_t)d_layers | (uintptr_t)d_total) & 15) != 0 ||
        (((uintptr_t)d_lo | (uintptr_t)d_hi | (uintptr_t)d_reach | (uintptr_t)d_amp_off | (uintptr_t)d_keys) & 7) != 0 || ((uintptr_t)d_layer_amp & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "amplicon_layers: bad argument (16-byte aligned d_counts, d_layers and d_total, 8-byte aligned d_lo, d_hi, d_reach, d_amp_off and d_keys, "
                    "4-byte aligned d_layer_amp)");
    if (W > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "amplicon_layers: 2^31 walk entries or more");
    if ((P + 255) / 256 > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "amplicon_layers: too many positions in one call");
    if (A == 0 || P == 0) return AMPLI_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(amplicon_layers_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), d_counts, (const unsigned long long *)d_lo,
                       (const unsigned long long *)d_hi, (const unsigned long long *)d_reach, (const long long *)d_amp_off, (long long)A,
                       (const unsigned long long *)d_keys, (long long)P, (int)L, d_layers, d_layer_amp, d_total);
    return check_launch(ctx, "amplicon_layers_kernel");
}
