// amplisolve_amd/csrc/ampli_evidence.hip -- evidence_count_kernel + ampli_pileup_evidence, evidence_score_kernel + ampli_evidence_score
// (include/amplisolve_hip.h): the third walk over the alignment records of a BAM file, the counting half of computeReadEvidence (DESIGN
// 29); the container half is csrc/host/bam.cpp, the command csrc/host/run_re.cpp.  ampli_pileup.hip counts the base of every column; this
// unit keeps, for every counted column, what the read behind it looked like: its base quality, its MAPQ and where in the read it sat.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ampli_bam.h" // the record layout, the keys and their searches
#include "ampli_internal.h"
#include "ampli_math.h" // ampli_ev_*: the score's arithmetic, shared with the host library

// ---------------------------------------------------------------------------
// evidence_count: per panel position p and nt, three 64-bin histograms over the counted columns (the definition: include/amplisolve_hip.h,
// ampli_pileup_evidence): hist[p][nt][metric][bin].
// Geometry of indel_count_kernel (ampli_indel.hip): a workgroup of 256 threads takes EVIDENCE_READS consecutive reads.  The intended
// input is a CALL LIST -- tens to hundreds of listed positions, every read of an amplicon over the same one or two of them -- so the work
// of a read is a handful of columns, not its whole length, and a wave has nothing to share out: every THREAD walks one read, the records
// read straight from global memory.  The walk is a merge: the read's CIGAR and the sorted keys advance together, so a read costs its
// operations plus the listed keys inside its span, whatever the list.
// Counters: the reads of an amplicon hit the same positions and a sequencer emits 4-8 distinct qualities, so nearly every column of a
// workgroup lands in the same few bins.  They go into an LDS window of EVIDENCE_WINDOW listed keys (3 KB of bins each) that starts at the
// first key not below the start of the workgroup's first placed read; it is flushed with one global atomic per non-zero bin of the keys
// that were touched.  Whatever falls outside the window (a dense list, an unsorted file) goes to the global counters directly.
// ---------------------------------------------------------------------------
constexpr int EVIDENCE_READS = 256;
constexpr int EVIDENCE_WINDOW = 8;
constexpr int EVIDENCE_CELLS = 4 * AMPLI_EVIDENCE_METRICS * AMPLI_EVIDENCE_BINS; // counters of one key

__global__ __launch_bounds__(256) void evidence_count_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                             const long long n_reads, const unsigned long long *__restrict__ keys, const long long P,
                                                             const int mbq, const int mrq, int *__restrict__ hist, unsigned long long *__restrict__ stats)
{
    __shared__ __attribute__((aligned(16))) int win[EVIDENCE_WINDOW * EVIDENCE_CELLS];
    __shared__ unsigned long long wkeys[EVIDENCE_WINDOW]; // the window's keys
    __shared__ int touched[EVIDENCE_WINDOW];
    __shared__ long long win_base;
    __shared__ unsigned long long win_k0; // the key of the start of the workgroup's first placed read: win_base is its lower bound
    __shared__ unsigned long long s_stats[2];
    const long long first = (long long)blockIdx.x * EVIDENCE_READS;
    const long long end = first + EVIDENCE_READS < n_reads ? first + EVIDENCE_READS : n_reads;
    {
        int4 *w4 = (int4 *)win;
        for (int i = threadIdx.x; i < EVIDENCE_WINDOW * EVIDENCE_CELLS / 4; i += 256) w4[i] = make_int4(0, 0, 0, 0);
    }
    if (threadIdx.x < EVIDENCE_WINDOW) touched[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        s_stats[0] = s_stats[1] = 0;
        unsigned long long wk0;
        win_base = bam_window_base(bam, rec_off, first, end, keys, P, wk0);
        win_k0 = wk0;
    }
    __syncthreads();
    const long long wb = win_base;
    const unsigned long long wk0 = win_k0;
    const int nw = (int)(P - wb < EVIDENCE_WINDOW ? P - wb : EVIDENCE_WINDOW);
    if ((int)threadIdx.x < nw) wkeys[threadIdx.x] = keys[wb + threadIdx.x];
    __syncthreads();
    const auto key_at = [&](long long k) { return k >= wb && k < wb + nw ? wkeys[k - wb] : keys[k]; };
    const long long read = first + threadIdx.x;
    unsigned kept = 0, added = 0;
    BamRead h;
    if (read < n_reads && bam_read_header<bam_u32>(bam + rec_off[read] + 4, mrq, h)) { // + 4: past block_size
        kept = 1;
        const unsigned rid = (unsigned)h.ref_id;
        const unsigned long long ref_hi = bam_key(h.ref_id, 0);
        const int mq_bin = (h.mapq >> 2) < AMPLI_EVIDENCE_BINS - 1 ? (h.mapq >> 2) : AMPLI_EVIDENCE_BINS - 1;
        // k: the first key not below the read's start; from here on "the first key not below the next column"
        const unsigned long long k0 = bam_key(h.ref_id, h.pos + 1);
        long long k;
        if (nw > 0 && k0 >= wk0 && k0 <= wkeys[nw - 1]) k = wb + bam_lower<int>(wkeys, 0, nw, k0); // its lower bound lies inside the window: LDS
        else k = bam_lower<long long>(keys, 0, P, k0);
        long long refpos = h.pos; // 0-based
        int qpos = 0;
        for (int c = 0; c < h.n_cigar && k < P; ++c) {
            const BamOp o = bam_cigar<bam_u32>(h.cig, c);
            const int len = o.len;
            if (bam_op_match(o.op)) { // M, =, X: the listed keys on columns refpos + 1 .. refpos + len (1-based)
                for (; k < P; ++k) {
                    const unsigned long long kk = key_at(k);
                    const long long x = (long long)(kk & 0xffffffffull);
                    if ((unsigned)(kk >> 32) != rid || x > refpos + len) break;
                    const int q = qpos + (int)(x - 1 - refpos);
                    const int b4 = bam_nt(h.seq, q);
                    const int bq = (int)h.qual[q];
                    if (b4 < 0 || bq < mbq) continue;
                    int d = q < h.l_seq - 1 - q ? q : h.l_seq - 1 - q;
                    d = d < 0 ? 0 : d; // (a record whose CIGAR overruns its l_seq: the host scanner drops those)
                    const int bins[AMPLI_EVIDENCE_METRICS] = {bq < AMPLI_EVIDENCE_BINS - 1 ? bq : AMPLI_EVIDENCE_BINS - 1, mq_bin,
                                                              d < AMPLI_EVIDENCE_BINS - 1 ? d : AMPLI_EVIDENCE_BINS - 1};
                    if (k >= wb && k < wb + nw) {
                        const int w = (int)(k - wb);
                        int *cell = win + (w * 4 + b4) * (AMPLI_EVIDENCE_METRICS * AMPLI_EVIDENCE_BINS);
#pragma unroll
                        for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) atomicAdd(&cell[m * AMPLI_EVIDENCE_BINS + bins[m]], 1);
                        touched[w] = 1;
                    } else {
                        int *cell = hist + (k * 4 + b4) * (long long)(AMPLI_EVIDENCE_METRICS * AMPLI_EVIDENCE_BINS);
#pragma unroll
                        for (int m = 0; m < AMPLI_EVIDENCE_METRICS; ++m) atomicAdd(&cell[m * AMPLI_EVIDENCE_BINS + bins[m]], 1);
                    }
                    ++added;
                }
                refpos += len;
                qpos += len;
            } else if (bam_op_query(o.op)) { // I, S
                qpos += len;
            } else if (bam_op_ref(o.op)) { // D, N: the keys on the positions it spans are no column of this read
                refpos += len;
                const unsigned long long kk = key_at(k);
                if ((unsigned)(kk >> 32) == rid && (long long)(kk & 0xffffffffull) <= refpos) {
                    // first key behind the gap: (rid, refpos + 1), or the next reference's first where that leaves 32 bits
                    const unsigned long long t = refpos + 1 <= 0xffffffffll ? bam_key(h.ref_id, refpos + 1) : ref_hi + (1ull << 32);
                    k = bam_lower<long long>(keys, k + 1, P, t);
                }
            } // H, P: neither
        }
    }
    if (stats && (kept | added)) { // one pair of LDS atomics per thread, one pair of global atomics per workgroup
        if (kept) atomicAdd(&s_stats[0], 1ull);
        if (added) atomicAdd(&s_stats[1], (unsigned long long)added);
    }
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
        if (!touched[w]) continue; // (workgroup-uniform)
        int *cell = hist + (wb + w) * (long long)EVIDENCE_CELLS;
        for (int i = threadIdx.x; i < EVIDENCE_CELLS; i += 256) {
            const int v = win[w * EVIDENCE_CELLS + i];
            if (v != 0) atomicAdd(&cell[i], v);
        }
    }
    if (stats && threadIdx.x == 0) {
        if (s_stats[0]) atomicAdd(&stats[0], s_stats[0]); // reads kept
        if (s_stats[1]) atomicAdd(&stats[1], s_stats[1]); // columns counted
    }
}

extern "C" int ampli_pileup_evidence(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P,
                                     int32_t mbq, int32_t mrq, int32_t *d_hist, uint64_t *d_stats)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_bam || !d_rec_off || n_reads < 0 || !d_keys || P < 0 || !d_hist) return fail(ctx, AMPLI_E_INVALID, "pileup_evidence: bad argument");
    if ((((uintptr_t)d_rec_off | (uintptr_t)d_keys | (uintptr_t)d_stats) & 7) != 0 || ((uintptr_t)d_hist & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "pileup_evidence: bad argument (8-byte aligned d_rec_off, d_keys and d_stats, 4-byte aligned d_hist)");
    if (n_reads == 0 || P == 0) return AMPLI_OK;
    if ((n_reads + EVIDENCE_READS - 1) / EVIDENCE_READS > 0x7fffffffll)
        return fail(ctx, AMPLI_E_RANGE, "pileup_evidence: too many reads in one call; split the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((n_reads + EVIDENCE_READS - 1) / EVIDENCE_READS)); // 1-D over groups of reads
    hipLaunchKernelGGL(evidence_count_kernel, grid, dim3(256), 0, main_stream(ctx), (const unsigned char *)d_bam, (const unsigned long long *)d_rec_off,
                       (long long)n_reads, (const unsigned long long *)d_keys, (long long)P, (int)mbq, (int)mrq, d_hist, (unsigned long long *)d_stats);
    return check_launch(ctx, "evidence_count_kernel");
}

// ---------------------------------------------------------------------------
// evidence_score: one lane per (position, metric), the 64-bin loops of ampli_ev_cell over d_hist; no LDS, no barrier, no atomics.  The three
// lanes of a position each find the alt nt for themselves (ampli_ev_alt reads the same 4 x 64 words); the lane of metric 0 stores it.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void evidence_score_kernel(const int *__restrict__ hist, const long long P, const signed char *__restrict__ ref_nt,
                                                             const signed char *__restrict__ alt_nt, long long *__restrict__ o_int, int *__restrict__ o_med,
                                                             double *__restrict__ o_z2, signed char *__restrict__ alt_used)
{
    const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= P * AMPLI_EVIDENCE_METRICS) return;
    const long long p = cell / AMPLI_EVIDENCE_METRICS;
    const int m = (int)(cell - p * AMPLI_EVIDENCE_METRICS);
    const int *h = hist + p * EVIDENCE_CELLS;
    const int ref = (int)ref_nt[p];
    const int alt = ampli_ev_alt(h, ref, (int)alt_nt[p]);
    const int *a = alt >= 0 ? h + (alt * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS : nullptr;
    const int *r = ref >= 0 && ref <= 3 ? h + (ref * AMPLI_EVIDENCE_METRICS + m) * AMPLI_EVIDENCE_BINS : nullptr;
    int64_t vi[3];
    int32_t vm[2];
    double z2;
    ampli_ev_cell(a, r, vi, vm, &z2);
    o_int[cell * 3] = vi[0];
    o_int[cell * 3 + 1] = vi[1];
    o_int[cell * 3 + 2] = vi[2];
    o_med[cell * 2] = vm[0];
    o_med[cell * 2 + 1] = vm[1];
    o_z2[cell] = z2;
    if (m == 0) alt_used[p] = (signed char)alt;
}

extern "C" int ampli_evidence_score(ampli_ctx *ctx, const int32_t *d_hist, int64_t P, const int8_t *d_ref_nt, const int8_t *d_alt_nt, int64_t *d_int,
                                    int32_t *d_med, double *d_z2, int8_t *d_alt_used)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_hist || P < 0 || !d_ref_nt || !d_alt_nt || !d_int || !d_med || !d_z2 || !d_alt_used) return fail(ctx, AMPLI_E_INVALID, "evidence_score: bad argument");
    if ((((uintptr_t)d_int | (uintptr_t)d_z2) & 7) != 0 || (((uintptr_t)d_hist | (uintptr_t)d_med) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "evidence_score: bad argument (8-byte aligned d_int and d_z2, 4-byte aligned d_hist and d_med)");
    if (P == 0) return AMPLI_OK;
    const int64_t groups = (P * AMPLI_EVIDENCE_METRICS + 255) / 256;
    if (groups > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "evidence_score: too many positions in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(evidence_score_kernel, dim3((unsigned)groups), dim3(256), 0, main_stream(ctx), (const int *)d_hist, (long long)P, (const signed char *)d_ref_nt,
                       (const signed char *)d_alt_nt, (long long *)d_int, (int *)d_med, (double *)d_z2, (signed char *)d_alt_used);
    return check_launch(ctx, "evidence_score_kernel");
}
