// amplisolve_amd/csrc/ampli_pileup.hip -- pileup_count_kernel + ampli_pileup_count (include/amplisolve_hip.h): the counting
// half of computeCounts (BAM -> .PILEUP.ASEQ); the container half is amplisolve_amd/csrc/host/bam.cpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ampli_bam.h" // the record layout, the keys and their searches
#include "ampli_internal.h"

// ---------------------------------------------------------------------------
// pileup_count: the upstream step of the path, BAM alignments -> per-position base x strand counts (what ASEQ's PILEUP mode
// / the reference's binary-only computeCounts write as .PILEUP.ASEQ; /root/reference/Execution_examples.md:16-46).
// The host inflates the BGZF blocks and lists the byte offsets of the alignment records; this kernel decodes the records
// themselves.  One wave per read at a time, lanes over the bases of a CIGAR match run: the reads of an amplicon start at the
// same place, so a lane-per-read mapping would have all 64 lanes of a wave add to the SAME counter at every step.
//   kept reads: mapped, not secondary / QC-fail / duplicate (the pileup engine's default mask), MAPQ >= mrq;
//   counted bases: inside M / = / X runs (deletions and reference skips contribute nothing), A/C/G/T only, quality >= mbq;
//   counts[p][0..3] = A,C,G,T over both strands, counts[p][4..7] = the same on the reverse strand (flag 0x10).
// keys: the panel's unique positions as (BAM reference id << 32 | 1-based position), sorted ascending.
// ---------------------------------------------------------------------------

// A workgroup takes PILEUP_READS consecutive reads (one wave per read at a time, lanes over the bases of a match run) and counts
// into a private LDS window of PILEUP_WINDOW panel positions that starts where its first read starts: a coordinate-sorted BAM keeps
// the reads of an amplicon together, so nearly every update is an LDS atomic and the window is flushed with one global atomic per
// non-zero counter (global atomics straight from the lanes ran at 4 G updates/s -- every read of an amplicon hits the same
// counters).  Updates outside the window (unsorted files, very long reads) go to the global counters directly.
constexpr int PILEUP_READS = 256;
constexpr int PILEUP_WINDOW = 1024;

// One column of a match run that lies on panel position a: base q of the read into ctr[a][b4], and ctr[a][4 + b4] on the reverse strand.
// ctr: the LDS window (a: window index) or the global counters (a: panel index).  true: the base was counted.
template <typename I>
__device__ __forceinline__ bool pileup_column(int *ctr, const I a, const unsigned char *seq, const unsigned char *qual, const int q, const int rev,
                                              const int mbq)
{
    const int b4 = bam_nt(seq, q);
    if (b4 < 0 || (int)qual[q] < mbq) return false;
    atomicAdd(&ctr[a * 8 + b4], 1);
    if (rev) atomicAdd(&ctr[a * 8 + 4 + b4], 1);
    return true;
}

// The wave-per-read walk over reads first + wave, first + wave + 4, .. < end, the records read straight from global memory.  WINDOW: runs
// inside the key range of the LDS window (win, its nw keys in wkeys) are searched and counted there; without it, and for every other
// run, global search and global counters.  kept counts on lane 0 only, added on every lane.
template <bool WINDOW>
__device__ __forceinline__ void pileup_wave_walk(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off, const long long first,
                                                 const long long end, const unsigned long long *__restrict__ keys, const long long P, const int mbq,
                                                 const int mrq, int *__restrict__ counts, int *win, const unsigned long long *wkeys, const int nw,
                                                 unsigned long long &kept, unsigned long long &added)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long prev_k0 = ~0ull; // the reads of an amplicon start at the same place: the last run's search is usually this run's
    int prev_lo = 0;
    for (long long read = first + wave; read < end; read += 4) {
        BamRead h;
        if (!bam_read_header<bam_u32>(bam + rec_off[read] + 4, mrq, h)) continue; // + 4: past block_size
        if (lane == 0) ++kept;
        long long refpos = h.pos; // 0-based
        int qpos = 0;
        for (int c = 0; c < h.n_cigar; ++c) {
            const BamOp o = bam_cigar<bam_u32>(h.cig, c);
            const int len = o.len;
            if (bam_op_match(o.op)) {
                const unsigned long long k0 = bam_key(h.ref_id, refpos + 1);
                // the run lies inside the window's key range: everything below happens in LDS.  (No len > 0 as in the staged walk: a
                // zero-length run executes no column on either side.)
                const bool inwin = WINDOW && nw > 0 && k0 >= wkeys[0] && k0 + (unsigned long long)len - 1 <= wkeys[nw - 1];
                if (inwin) {
                    if (k0 != prev_k0) { // first window key >= k0 (wave-uniform)
                        prev_lo = bam_lower<int>(wkeys, 0, nw, k0);
                        prev_k0 = k0;
                    }
                    const int lo = prev_lo;
                    const int wend = lo + len < nw ? lo + len : nw; // the keys of this run are among the next `len`
                    for (int j = lane; j < len; j += 64) {
                        const int a = bam_window_find(wkeys, lo, wend, j, k0 + (unsigned long long)j);
                        if (a >= 0 && pileup_column(win, a, h.seq, h.qual, qpos + j, h.rev, mbq)) ++added;
                    }
                } else {
                    // outside the window (unsorted file, a run that leaves the window, a position before it): global search and counters
                    const long long lo = bam_lower<long long>(keys, 0, P, k0);
                    const long long wend = lo + len < P ? lo + len : P;
                    if (lo < wend && keys[lo] < k0 + (unsigned long long)len) {
                        for (int j = lane; j < len; j += 64) {
                            const unsigned long long key = k0 + (unsigned long long)j;
                            const long long a = bam_lower<long long>(keys, lo, wend, key);
                            if (a < wend && keys[a] == key && pileup_column(counts, a, h.seq, h.qual, qpos + j, h.rev, mbq)) ++added;
                        }
                    }
                }
                refpos += len;
                qpos += len;
            } else if (bam_op_query(o.op)) {
                qpos += len;
            } else if (bam_op_ref(o.op)) {
                refpos += len;
            }
        }
    }
}

__global__ __launch_bounds__(256) void pileup_count_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                           const long long n_reads, const unsigned long long *__restrict__ keys, const long long P,
                                                           const int mbq, const int mrq, int *__restrict__ counts, unsigned long long *__restrict__ stats)
{
    __shared__ int win[PILEUP_WINDOW * 8];
    __shared__ unsigned long long wkeys[PILEUP_WINDOW]; // the window's panel keys: every search of an in-window run stays in LDS
    __shared__ long long win_base;
    const long long first = (long long)blockIdx.x * PILEUP_READS;
    const long long end = first + PILEUP_READS < n_reads ? first + PILEUP_READS : n_reads;
    for (int i = threadIdx.x; i < PILEUP_WINDOW * 8; i += 256) win[i] = 0;
    if (threadIdx.x == 0) {
        unsigned long long k0;
        win_base = bam_window_base(bam, rec_off, first, end, keys, P, k0);
    }
    __syncthreads();
    const long long wb = win_base;
    const int nw = (int)(P - wb < PILEUP_WINDOW ? P - wb : PILEUP_WINDOW);
    for (int i = threadIdx.x; i < nw; i += 256) wkeys[i] = keys[wb + i];
    __syncthreads();
    unsigned long long kept = 0, added = 0;
    pileup_wave_walk<true>(bam, rec_off, first, end, keys, P, mbq, mrq, counts, win, wkeys, nw, kept, added);
    __syncthreads();
    for (int i = threadIdx.x; i < PILEUP_WINDOW * 8; i += 256) {
        const int v = win[i];
        if (v != 0 && wb + (i >> 3) < P) atomicAdd(&counts[(wb + (i >> 3)) * 8 + (i & 7)], v);
    }
    if (stats) {
        if (kept) atomicAdd(&stats[0], kept);   // reads kept
        if (added) atomicAdd(&stats[1], added); // bases counted
    }
}

// ---------------------------------------------------------------------------
// The staged form (default): the wave-per-read kernel above spends its time on the dependent loads of ONE record at a time
// per wave (header -> CIGAR -> bases: 2.5 ms for 2 M reads, 185 GB/s).  Here a workgroup first copies the bytes of its
// PILEUP_READS consecutive records -- they are contiguous in the stream -- into LDS with coalesced 16-byte loads, and then every
// THREAD walks one read out of LDS: 64 records in flight per wave instead of one, no global load in the walk at all.  The
// reads of an amplicon start at the same place, so lane l starts its walk of a match run l * PILEUP_ROT bases in (wrapping
// around): at any step the lanes of a wave then add to different counters of the LDS window instead of all to the same one.
// A group whose records do not fit the stage (very long reads) falls back to the wave-per-read walk from global memory.
// ---------------------------------------------------------------------------
constexpr int PILEUP_STAGE = 56 * 1024; // bytes of records a workgroup stages
constexpr int PILEUP_SWINDOW = 384;     // panel positions of the staged kernel's LDS window
constexpr int PILEUP_ROT = 3;

__global__ __launch_bounds__(256) void pileup_count_staged_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                                  const long long n_reads, const unsigned long long *__restrict__ keys, const long long P,
                                                                  const int mbq, const int mrq, int *__restrict__ counts,
                                                                  unsigned long long *__restrict__ stats)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[PILEUP_STAGE + 32];
    __shared__ int win[PILEUP_SWINDOW * 8];
    __shared__ unsigned long long wkeys[PILEUP_SWINDOW];
    __shared__ long long s_wb;
    __shared__ unsigned long long s_span[2]; // first byte (16-byte aligned down) and end of the group's records in the stream
    const long long first = (long long)blockIdx.x * PILEUP_READS;
    const int n_here = (int)(n_reads - first < PILEUP_READS ? n_reads - first : PILEUP_READS);
    for (int i = threadIdx.x; i < PILEUP_SWINDOW * 8; i += 256) win[i] = 0;
    if (threadIdx.x == 0) {
        const unsigned long long b0 = rec_off[first], last = rec_off[first + n_here - 1];
        s_span[0] = b0 & ~15ull;
        s_span[1] = last + 4ull + (unsigned long long)bam_u32()(bam + last);
        unsigned long long k0;
        s_wb = bam_window_base(bam, rec_off, first, first + n_here, keys, P, k0);
    }
    __syncthreads();
    const long long wb = s_wb;
    const unsigned long long g0 = s_span[0], g1 = s_span[1];
    const bool staged = g1 - g0 <= (unsigned long long)PILEUP_STAGE; // workgroup-uniform
    const int nw = (int)(P - wb < PILEUP_SWINDOW ? P - wb : PILEUP_SWINDOW);
    for (int i = threadIdx.x; i < nw; i += 256) wkeys[i] = keys[wb + i];
    if (staged) { // coalesced copy of the group's bytes (the host pads the buffer so that whole 16-byte pieces can be read)
        const uint4 *src = (const uint4 *)(bam + g0);
        uint4 *dst = (uint4 *)stage;
        const int n16 = (int)((g1 - g0 + 15) >> 4);
        for (int i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    unsigned long long kept = 0, added = 0;
    if (staged) {
        const int t = threadIdx.x;
        BamRead h;
        if (t < n_here && bam_read_header<lds_u32>(stage + (rec_off[first + t] - g0) + 4, mrq, h)) { // + 4: past block_size
            kept = 1;
            const int lane = t & 63;
            long long refpos = h.pos;
            int qpos = 0;
            for (int c = 0; c < h.n_cigar; ++c) {
                const BamOp o = bam_cigar<lds_u32>(h.cig, c);
                const int len = o.len;
                if (bam_op_match(o.op)) {
                    const unsigned long long k0 = bam_key(h.ref_id, refpos + 1);
                    const bool inwin = len > 0 && nw > 0 && k0 >= wkeys[0] && k0 + (unsigned long long)len - 1 <= wkeys[nw - 1];
                    int lo = 0;
                    long long glo = 0, gend = 0;
                    if (inwin) { // first window key >= k0
                        lo = bam_lower<int>(wkeys, 0, nw, k0);
                    } else if (len > 0) { // outside the window: global keys, global counters
                        glo = bam_lower<long long>(keys, 0, P, k0);
                        gend = glo + len < P ? glo + len : P;
                    }
                    const int wend = lo + len < nw ? lo + len : nw;
                    int j = len > 0 ? (lane * PILEUP_ROT) % len : 0; // rotated start: the lanes of a wave hit different counters
                    for (int step = 0; step < len; ++step, j = j + 1 == len ? 0 : j + 1) {
                        const unsigned long long key = k0 + (unsigned long long)j;
                        if (inwin) {
                            const int a = bam_window_find(wkeys, lo, wend, j, key);
                            if (a >= 0 && pileup_column(win, a, h.seq, h.qual, qpos + j, h.rev, mbq)) ++added;
                        } else if (glo < gend) {
                            const long long a = bam_lower<long long>(keys, glo, gend, key);
                            if (a < gend && keys[a] == key && pileup_column(counts, a, h.seq, h.qual, qpos + j, h.rev, mbq)) ++added;
                        }
                    }
                    refpos += len;
                    qpos += len;
                } else if (bam_op_query(o.op)) {
                    qpos += len;
                } else if (bam_op_ref(o.op)) {
                    refpos += len;
                }
            }
        }
    } else {
        // records too long for the stage: one wave per read at a time, straight from global memory, global counters
        pileup_wave_walk<false>(bam, rec_off, first, first + n_here, keys, P, mbq, mrq, counts, nullptr, nullptr, 0, kept, added);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PILEUP_SWINDOW * 8; i += 256) {
        const int v = win[i];
        if (v != 0 && wb + (i >> 3) < P) atomicAdd(&counts[(wb + (i >> 3)) * 8 + (i & 7)], v);
    }
    if (stats) {
        if (kept) atomicAdd(&stats[0], kept);
        if (added) atomicAdd(&stats[1], added);
    }
}

extern "C" int ampli_pileup_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P,
                                  int32_t mbq, int32_t mrq, int32_t *d_counts, uint64_t *d_stats)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_bam || !d_rec_off || n_reads < 0 || !d_keys || P <= 0 || !d_counts) return fail(ctx, AMPLI_E_INVALID, "pileup_count: bad argument");
    // the staged kernel copies uint4 pieces from d_bam + (offset & ~15); the other pointers are typed
    if (((uintptr_t)d_bam & 15) != 0 || (((uintptr_t)d_rec_off | (uintptr_t)d_keys | (uintptr_t)d_stats) & 7) != 0 || ((uintptr_t)d_counts & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "pileup_count: bad argument (16-byte aligned d_bam, 8-byte aligned d_rec_off, d_keys and d_stats, 4-byte aligned d_counts)");
    if (n_reads == 0) return AMPLI_OK;
    if ((n_reads + PILEUP_READS - 1) / PILEUP_READS > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "pileup_count: too many reads in one call; split the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // AMPLI_PILEUP_WAVE_PER_READ (build-time) keeps the first form for comparison (tools/pileup_bench.py)
#ifdef AMPLI_PILEUP_WAVE_PER_READ
    const auto kernel = pileup_count_kernel;
#else
    const auto kernel = pileup_count_staged_kernel;
#endif
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_reads + PILEUP_READS - 1) / PILEUP_READS)), dim3(256), 0, main_stream(ctx), (const unsigned char *)d_bam,
                       (const unsigned long long *)d_rec_off, (long long)n_reads, (const unsigned long long *)d_keys, (long long)P, (int)mbq, (int)mrq,
                       d_counts, (unsigned long long *)d_stats);
    return check_launch(ctx, "pileup_count_kernel");
}
