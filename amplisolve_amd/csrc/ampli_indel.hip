// amplisolve_amd/csrc/ampli_indel.hip -- indel_count_kernel + ampli_pileup_indel_count (include/amplisolve_hip.h): the second walk over
// the alignment records of a BAM file, the counting half of computeIndelCounts; the container half is csrc/host/bam.cpp,
// the command csrc/host/run_ci.cpp.  ampli_pileup.hip counts the base of every column; this unit counts what lies BEHIND every column.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ampli_bam.h"    // the record layout, the keys and their searches
#include "ampli_device.h" // with_bool, the launch dispatch
#include "ampli_internal.h"

// ---------------------------------------------------------------------------
// indel_count: per panel position p and read strand, how many kept reads show an insertion, a deletion or neither at junction p, the
// boundary between reference positions p and p + 1 (the definition: include/amplisolve_hip.h, ampli_pileup_indel_count).
//   counts[p][0] reference junctions, counts[p][1] insertions, counts[p][2] deletions, counts[p][4..6] the same on the reverse strand;
//   slots 3 and 7 are never written; lengths[p][kind][min(L, 32) - 1], kind 0 insertion, 1 deletion, both strands pooled.
// Shape of pileup_count_kernel (ampli_pileup.hip): a workgroup takes INDEL_READS consecutive reads, one wave per read at a time, lanes
// over the columns of a match run, the records read straight from global memory.  The CIGAR state machine is wave-uniform: every lane
// of a wave walks the same operations and holds the same state; only the columns of a run are dealt to the lanes.
// Counters: reference junctions -- one per column, every read of an amplicon on the same ones -- go into an LDS window of INDEL_WINDOW
// panel positions x 2 planes (both strands, reverse strand) that starts where the workgroup's first read starts and is flushed with one
// global atomic per non-zero counter.  Events are rare: they and their length bins go to the global counters directly (32 bins x 2 x
// 1024 positions do not belong in LDS), and so does whatever falls outside the window (unsorted files, very long reads).
// ---------------------------------------------------------------------------
constexpr int INDEL_READS = 256;
constexpr int INDEL_WINDOW = 1024;

template <bool LENGTHS>
__global__ __launch_bounds__(256) void indel_count_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                          const long long n_reads, const unsigned long long *__restrict__ keys, const long long P,
                                                          const int mbq, const int mrq, int *__restrict__ counts, int *__restrict__ lengths,
                                                          unsigned long long *__restrict__ stats)
{
    __shared__ int win[INDEL_WINDOW * 2];               // [window position][0: slot 0, 1: slot 4]
    __shared__ unsigned long long wkeys[INDEL_WINDOW]; // the window's panel keys: every search of an in-window run stays in LDS
    __shared__ long long win_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long first = (long long)blockIdx.x * INDEL_READS;
    const long long end = first + INDEL_READS < n_reads ? first + INDEL_READS : n_reads;
    for (int i = threadIdx.x; i < INDEL_WINDOW * 2; i += 256) win[i] = 0;
    if (threadIdx.x == 0) {
        unsigned long long k0;
        win_base = bam_window_base(bam, rec_off, first, end, keys, P, k0);
    }
    __syncthreads();
    const long long wb = win_base;
    const int nw = (int)(P - wb < INDEL_WINDOW ? P - wb : INDEL_WINDOW);
    for (int i = threadIdx.x; i < nw; i += 256) wkeys[i] = keys[wb + i];
    __syncthreads();
    unsigned long long kept = 0, added = 0;
    unsigned long long prev_k0 = ~0ull; // the reads of an amplicon start at the same place: the last run's search is usually this run's
    int prev_lo = 0;
    for (long long read = first + wave; read < end; read += 4) {
        // bam_read_header<bam_u32> of ampli_bam.h, written out: through the helper both instantiations take 54 VGPRs instead of 52
        // (profiles/bam_walks).  A change to the record layout there is a change here.
        const unsigned char *r = bam + rec_off[read] + 4; // past block_size
        const int ref_id = (int)bam_u32()(r), pos = (int)bam_u32()(r + 4);
        const unsigned bin_mq_nl = bam_u32()(r + 8), flag_nc = bam_u32()(r + 12);
        const int l_read_name = (int)(bin_mq_nl & 0xffu), mapq = (int)((bin_mq_nl >> 8) & 0xffu);
        const int n_cigar = (int)(flag_nc & 0xffffu);
        const unsigned flag = flag_nc >> 16;
        if (ref_id < 0 || pos < 0 || (flag & BAM_FILTERED) != 0 || mapq < mrq) continue;
        ++kept;
        const int l_seq = (int)bam_u32()(r + 16);
        const unsigned char *cig = r + 32 + l_read_name;
        const unsigned char *qual = cig + 4 * (size_t)n_cigar + (l_seq + 1) / 2;
        const int rev = (int)((flag >> 4) & 1u);
        const unsigned long long ref_hi = bam_key(ref_id, 0);
        long long refpos = pos; // 0-based
        int qpos = 0;
        // the state: "the previous effective operation was a match run, ending at column run_end (1-based) with query index run_q", and
        // at most one pending indel behind it (pend: 0 none, 1 I, 2 D -- the slot it will be counted in -- of length pend_len)
        bool run = false;
        long long run_end = 0;
        int run_q = 0, pend = 0, pend_len = 0;
        for (int c = 0; c < n_cigar; ++c) {
            const BamOp o = bam_cigar<bam_u32>(cig, c);
            const unsigned op = o.op;
            const int len = o.len;
            if (len == 0 || op == 6) continue; // not an effective operation: zero length, or P
            if (bam_op_match(op)) { // a match run: M, =, X
                // it first settles what is pending: the pending event at its anchor, or a reference junction between two adjacent runs
                if (run && lane == 0 && (int)qual[run_q] >= mbq) {
                    const unsigned long long key = ref_hi | (unsigned long long)run_end;
                    const bool inwin = pend == 0 && nw > 0 && key >= wkeys[0] && key <= wkeys[nw - 1];
                    if (inwin) {
                        const int a = bam_lower<int>(wkeys, 0, nw, key);
                        if (wkeys[a] == key) { // (a < nw: key <= wkeys[nw - 1])
                            atomicAdd(&win[a * 2], 1);
                            if (rev) atomicAdd(&win[a * 2 + 1], 1);
                            ++added;
                        }
                    } else {
                        const long long a = bam_lower<long long>(keys, 0, P, key);
                        if (a < P && keys[a] == key) {
                            atomicAdd(&counts[a * 8 + pend], 1);
                            if (rev) atomicAdd(&counts[a * 8 + 4 + pend], 1);
                            ++added;
                            if (LENGTHS && pend != 0) {
                                const int bin = (pend_len < AMPLI_INDEL_LEN_BINS ? pend_len : AMPLI_INDEL_LEN_BINS) - 1;
                                atomicAdd(&lengths[(a * 2 + (pend - 1)) * AMPLI_INDEL_LEN_BINS + bin], 1);
                            }
                        }
                    }
                }
                // it then counts its own len - 1 inner junctions as reference junctions: anchors are its columns 0 .. len - 2
                const int n = len - 1;
                const unsigned long long k0 = ref_hi | (unsigned long long)(refpos + 1);
                // the anchors lie inside the window's key range: everything below happens in LDS
                const bool inwin = n > 0 && nw > 0 && k0 >= wkeys[0] && k0 + (unsigned long long)n - 1 <= wkeys[nw - 1];
                if (inwin) {
                    if (k0 != prev_k0) { // first window key >= k0 (wave-uniform)
                        prev_lo = bam_lower<int>(wkeys, 0, nw, k0);
                        prev_k0 = k0;
                    }
                    const int lo = prev_lo;
                    const int wend = lo + n < nw ? lo + n : nw; // the keys of these anchors are among the next `n`
                    for (int j = lane; j < n; j += 64) {
                        const int a = bam_window_find(wkeys, lo, wend, j, k0 + (unsigned long long)j);
                        if (a >= 0 && (int)qual[qpos + j] >= mbq) {
                            atomicAdd(&win[a * 2], 1);
                            if (rev) atomicAdd(&win[a * 2 + 1], 1);
                            ++added;
                        }
                    }
                } else if (n > 0) {
                    // outside the window (unsorted file, a run that leaves the window, a position before it): global search and counters
                    const long long lo = bam_lower<long long>(keys, 0, P, k0);
                    const long long wend = lo + n < P ? lo + n : P;
                    if (lo < wend && keys[lo] < k0 + (unsigned long long)n) {
                        for (int j = lane; j < n; j += 64) {
                            const unsigned long long key = k0 + (unsigned long long)j;
                            const long long a = bam_lower<long long>(keys, lo, wend, key);
                            if (a < wend && keys[a] == key && (int)qual[qpos + j] >= mbq) {
                                atomicAdd(&counts[a * 8], 1);
                                if (rev) atomicAdd(&counts[a * 8 + 4], 1);
                                ++added;
                            }
                        }
                    }
                }
                refpos += len;
                qpos += len;
                run = true;
                run_end = refpos; // 1-based position of the run's last column
                run_q = qpos - 1;
                pend = 0;
            } else if ((op == 1 || op == 2) && run && pend == 0) { // I or D behind a match run with nothing pending becomes pending
                pend = (int)op;
                pend_len = len;
                if (op == 1) qpos += len;
                else refpos += len;
            } else { // every other case clears both states
                run = false;
                pend = 0;
                if (bam_op_query(op)) qpos += len;      // I, S
                else if (bam_op_ref(op)) refpos += len; // D, N
                // H: neither
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < INDEL_WINDOW * 2; i += 256) {
        const int v = win[i];
        if (v != 0 && wb + (i >> 1) < P) atomicAdd(&counts[(wb + (i >> 1)) * 8 + (i & 1) * 4], v);
    }
    if (stats) {
        if (lane == 0 && kept) atomicAdd(&stats[0], kept); // reads kept
        if (added) atomicAdd(&stats[1], added);            // junctions counted, all three slots
    }
}

extern "C" int ampli_pileup_indel_count(ampli_ctx *ctx, const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys,
                                        int64_t P, int32_t mbq, int32_t mrq, int32_t *d_counts, int32_t *d_lengths, uint64_t *d_stats)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_bam || !d_rec_off || n_reads < 0 || !d_keys || P < 0 || !d_counts) return fail(ctx, AMPLI_E_INVALID, "pileup_indel_count: bad argument");
    if ((((uintptr_t)d_rec_off | (uintptr_t)d_keys | (uintptr_t)d_stats) & 7) != 0 || (((uintptr_t)d_counts | (uintptr_t)d_lengths) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "pileup_indel_count: bad argument (8-byte aligned d_rec_off, d_keys and d_stats, 4-byte aligned d_counts and d_lengths)");
    if (n_reads == 0 || P == 0) return AMPLI_OK;
    if ((n_reads + INDEL_READS - 1) / INDEL_READS > 0x7fffffffll)
        return fail(ctx, AMPLI_E_RANGE, "pileup_indel_count: too many reads in one call; split the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((n_reads + INDEL_READS - 1) / INDEL_READS)); // 1-D over groups of reads
    with_bool(d_lengths != nullptr, [&](auto with_lengths) {
        hipLaunchKernelGGL(indel_count_kernel<decltype(with_lengths)::value>, grid, dim3(256), 0, main_stream(ctx), (const unsigned char *)d_bam,
                           (const unsigned long long *)d_rec_off, (long long)n_reads, (const unsigned long long *)d_keys, (long long)P, (int)mbq, (int)mrq,
                           d_counts, d_lengths, (unsigned long long *)d_stats);
    });
    return check_launch(ctx, "indel_count_kernel");
}
