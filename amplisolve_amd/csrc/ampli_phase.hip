// amplisolve_amd/csrc/ampli_phase.hip -- phase_count_kernel + ampli_pileup_phase, phase_score_kernel + ampli_phase_score
// (include/amplisolve_hip.h): the fifth walk over the alignment records of a BAM file.  The other walks count columns one at a
// time; this unit keeps the one fact that only a read carries: which alleles it shows at two listed positions at once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ampli_bam.h" // the record layout, the keys and their searches
#include "ampli_internal.h"
#include "ampli_math.h" // ampli_ph_*: the pair's arithmetic, shared with the host library

// ---------------------------------------------------------------------------
// phase_count: per listed key i and partner k < K the 5 x 5 table of (state at key i, state at key i + 1 + k) over the kept reads that
// cover both (the definition: include/amplisolve_hip.h, ampli_pileup_phase): table[i][k][s_i][s_j].
// Geometry and merge of evidence_count_kernel (ampli_evidence.hip): a workgroup of 256 threads takes PHASE_READS consecutive reads, every
// THREAD walks one read, the read's CIGAR and the sorted keys advance together.  Unlike there a D or an N is walked too: the keys inside it
// are covered, in state OTHER.  The keys a read covers are a contiguous index range, so the states of the last K covered keys are all a
// thread has to remember: 3 bits a key in one register (`reg`, the latest key in the lowest bits) and how many of them are valid.  Visiting
// covered key j adds 1 to the cells (j - t, t - 1) for t = 1 .. valid: no per-thread array, no scratch.
// Counters: the reads of an amplicon cover the same keys and show the same few states, so nearly every increment of a workgroup lands in
// the same few cells.  They go into an LDS window of PHASE_WINDOW keys (K x 25 words = 800 bytes each; a cell belongs to its LOWER key i)
// that starts at the first key not below the start of the workgroup's first placed read; it is flushed with one global atomic per
// non-zero cell of the keys that were touched.  Whatever falls outside the window (a dense list, an unsorted file) goes to the global
// counters directly.
// ---------------------------------------------------------------------------
constexpr int PHASE_READS = 256;
constexpr int PHASE_WINDOW = 32;
constexpr int PHASE_K = AMPLI_PHASE_PARTNERS;
constexpr int PHASE_PAIR = AMPLI_PHASE_STATES * AMPLI_PHASE_STATES; // counters of one (key, partner)
constexpr int PHASE_CELLS = PHASE_K * PHASE_PAIR;                    // counters of one key
static_assert(3 * PHASE_K <= 32 && AMPLI_PHASE_OTHER < 8 && AMPLI_PHASE_OTHER == AMPLI_PHASE_STATES - 1, "K states of 3 bits in one register");
static_assert(PHASE_READS == 256 && (PHASE_WINDOW * PHASE_CELLS) % 4 == 0 && PHASE_WINDOW <= 256, "one thread a read; the window is cleared as int4");

__global__ __launch_bounds__(256) void phase_count_kernel(const unsigned char *__restrict__ bam, const unsigned long long *__restrict__ rec_off,
                                                          const long long n_reads, const unsigned long long *__restrict__ keys, const long long P,
                                                          const int mbq, const int mrq, int *__restrict__ table, unsigned long long *__restrict__ stats)
{
    __shared__ __attribute__((aligned(16))) int win[PHASE_WINDOW * PHASE_CELLS];
    __shared__ unsigned long long wkeys[PHASE_WINDOW]; // the window's keys
    __shared__ int touched[PHASE_WINDOW];
    __shared__ long long win_base;
    __shared__ unsigned long long win_k0; // the key of the start of the workgroup's first placed read: win_base is its lower bound
    __shared__ unsigned long long s_stats[3];
    const long long first = (long long)blockIdx.x * PHASE_READS;
    const long long end = first + PHASE_READS < n_reads ? first + PHASE_READS : n_reads;
    {
        int4 *w4 = (int4 *)win;
        for (int i = threadIdx.x; i < PHASE_WINDOW * PHASE_CELLS / 4; i += 256) w4[i] = make_int4(0, 0, 0, 0);
    }
    if (threadIdx.x < PHASE_WINDOW) touched[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        s_stats[0] = s_stats[1] = s_stats[2] = 0;
        unsigned long long wk0;
        win_base = bam_window_base(bam, rec_off, first, end, keys, P, wk0);
        win_k0 = wk0;
    }
    __syncthreads();
    const long long wb = win_base;
    const unsigned long long wk0 = win_k0;
    const int nw = (int)(P - wb < PHASE_WINDOW ? P - wb : PHASE_WINDOW);
    if ((int)threadIdx.x < nw) wkeys[threadIdx.x] = keys[wb + threadIdx.x];
    __syncthreads();
    const auto key_at = [&](long long k) { return k >= wb && k < wb + nw ? wkeys[k - wb] : keys[k]; };
    const long long read = first + threadIdx.x;
    unsigned kept = 0, covered = 0, added = 0;
    BamRead h;
    if (read < n_reads && bam_read_header<bam_u32>(bam + rec_off[read] + 4, mrq, h)) { // + 4: past block_size
        kept = 1;
        const unsigned rid = (unsigned)h.ref_id;
        // k: the first key not below the read's start; from here on "the first key not below the next reference position"
        const unsigned long long k0 = bam_key(h.ref_id, h.pos + 1);
        long long k;
        if (nw > 0 && k0 >= wk0 && k0 <= wkeys[nw - 1]) k = wb + bam_lower<int>(wkeys, 0, nw, k0); // its lower bound lies inside the window: LDS
        else k = bam_lower<long long>(keys, 0, P, k0);
        long long refpos = h.pos; // 0-based
        int qpos = 0;
        unsigned reg = 0; // the states of the latest covered keys, 3 bits each, key k - 1 in bits 0 .. 2
        int valid = 0;    // how many of them there are, at most K
        for (int c = 0; c < h.n_cigar && k < P; ++c) {
            const BamOp o = bam_cigar<bam_u32>(h.cig, c);
            const int len = o.len;
            const bool match = bam_op_match(o.op);
            if (match || bam_op_ref(o.op)) { // M, =, X, D, N: the listed keys on positions refpos + 1 .. refpos + len (1-based) are covered
                for (; k < P; ++k) {
                    const unsigned long long kk = key_at(k);
                    const long long x = (long long)(kk & 0xffffffffull);
                    if ((unsigned)(kk >> 32) != rid || x > refpos + len) break;
                    int s = AMPLI_PHASE_OTHER;
                    if (match) { // a counted column: A/C/G/T at or above mbq
                        const int q = qpos + (int)(x - 1 - refpos);
                        if (q < h.l_seq) { // (a record whose CIGAR overruns its l_seq: the host scanner drops those)
                            const int b4 = bam_nt(h.seq, q);
                            const int bq = (int)h.qual[q]; // (loaded beside the base, not behind it: one latency per key)
                            if (b4 >= 0 && bq >= mbq) s = b4;
                        }
                    }
                    for (int t = 1; t <= valid; ++t) { // the pair (k - t, k): partner t - 1 of key k - t
                        const int sp = (int)((reg >> (3 * (t - 1))) & 7u);
                        const int cell = (t - 1) * PHASE_PAIR + sp * AMPLI_PHASE_STATES + s;
                        const long long i = k - t;
                        if (i >= wb && i < wb + nw) {
                            const int w = (int)(i - wb);
                            atomicAdd(&win[w * PHASE_CELLS + cell], 1);
                            touched[w] = 1;
                        } else {
                            atomicAdd(&table[i * (long long)PHASE_CELLS + cell], 1);
                        }
                    }
                    added += (unsigned)valid;
                    reg = (reg << 3) | (unsigned)s;
                    valid = valid < PHASE_K ? valid + 1 : PHASE_K;
                    ++covered;
                }
                refpos += len;
                if (match) qpos += len;
            } else if (bam_op_query(o.op)) { // I, S
                qpos += len;
            } // H, P: neither
        }
    }
    if (stats && kept) { // three LDS atomics per thread at most, one set of global atomics per workgroup
        atomicAdd(&s_stats[0], 1ull);
        if (covered >= 2) atomicAdd(&s_stats[1], 1ull);
        if (added) atomicAdd(&s_stats[2], (unsigned long long)added);
    }
    __syncthreads();
    for (int w = 0; w < nw; ++w) {
        if (!touched[w]) continue; // (workgroup-uniform)
        int *cell = table + (wb + w) * (long long)PHASE_CELLS;
        for (int i = threadIdx.x; i < PHASE_CELLS; i += 256) {
            const int v = win[w * PHASE_CELLS + i];
            if (v != 0) atomicAdd(&cell[i], v);
        }
    }
    if (stats && threadIdx.x == 0) {
        if (s_stats[0]) atomicAdd(&stats[0], s_stats[0]); // reads kept
        if (s_stats[1]) atomicAdd(&stats[1], s_stats[1]); // reads covering at least two keys
        if (s_stats[2]) atomicAdd(&stats[2], s_stats[2]); // cells incremented
    }
}

extern "C" int ampli_pileup_phase(const uint8_t *d_bam, const uint64_t *d_rec_off, int64_t n_reads, const uint64_t *d_keys, int64_t P, int32_t mbq, int32_t mrq,
                                  int32_t *d_table, uint64_t *d_stats, ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_bam || !d_rec_off || n_reads < 0 || !d_keys || P < 0 || !d_table) return fail(ctx, AMPLI_E_INVALID, "pileup_phase: bad argument");
    if ((((uintptr_t)d_rec_off | (uintptr_t)d_keys | (uintptr_t)d_stats) & 7) != 0 || ((uintptr_t)d_table & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "pileup_phase: bad argument (8-byte aligned d_rec_off, d_keys and d_stats, 4-byte aligned d_table)");
    if (n_reads == 0 || P == 0) return AMPLI_OK;
    if ((n_reads + PHASE_READS - 1) / PHASE_READS > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "pileup_phase: too many reads in one call; split the batch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 grid((unsigned)((n_reads + PHASE_READS - 1) / PHASE_READS)); // 1-D over groups of reads
    hipLaunchKernelGGL(phase_count_kernel, grid, dim3(256), 0, main_stream(ctx), (const unsigned char *)d_bam, (const unsigned long long *)d_rec_off,
                       (long long)n_reads, (const unsigned long long *)d_keys, (long long)P, (int)mbq, (int)mrq, d_table, (unsigned long long *)d_stats);
    return check_launch(ctx, "phase_count_kernel");
}

// ---------------------------------------------------------------------------
// phase_score: one lane per pair; the exact test in the loop shape of paired_score_kernel (ampli_hyper_step while live); no LDS, no barrier,
// no atomics.  Every output cell has one owner and is stored exactly once.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phase_score_kernel(const int *__restrict__ table, const long long P, const long long *__restrict__ pair_cell,
                                                          const signed char *__restrict__ pair_nt, const long long Q, const int min_alt, const int min_share,
                                                          long long *__restrict__ o_int, float *__restrict__ o_score, int *__restrict__ o_class)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const long long cell = pair_cell[q];
    const int ref_i = pair_nt[q * 4], alt_i = pair_nt[q * 4 + 1], ref_j = pair_nt[q * 4 + 2], alt_j = pair_nt[q * 4 + 3];
    int64_t v[6] = {-1, -1, -1, -1, -1, -1};
    float score = 0.0f;
    int cls = -1;
    if (ampli_ph_tested(cell, P, ref_i, alt_i, ref_j, alt_j)) { // checked before any load of the table
        ampli_ph_counts(table + cell * PHASE_PAIR, ref_i, alt_i, ref_j, alt_j, v);
        cls = ampli_ph_class(v[1], v[2], v[3], min_alt, min_share);
        ampli_hyper_sum s;
        const int sign = ampli_pair_score_begin(&s, v[3], v[3] + v[2], v[1], v[1] + v[0], &score);
        if (sign) {
            while (s.live) ampli_hyper_step(&s);
            score = ampli_pair_s_from_p(s.res, sign);
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) o_int[q * 6 + c] = v[c];
    o_score[q] = score;
    o_class[q] = cls;
}

extern "C" int ampli_phase_score(const int32_t *d_table, int64_t P, const int64_t *d_pair_cell, const int8_t *d_pair_nt, int64_t Q, int32_t min_alt, int32_t min_share,
                                 int64_t *d_int, float *d_score, int32_t *d_class, ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_table || P < 0 || !d_pair_cell || !d_pair_nt || Q < 0 || min_alt < 1 || min_share < 0 || min_share > 100 || !d_int || !d_score || !d_class)
        return fail(ctx, AMPLI_E_INVALID, "phase_score: bad argument (min_alt >= 1, min_share in 0 .. 100)");
    if ((((uintptr_t)d_pair_cell | (uintptr_t)d_int) & 7) != 0 || (((uintptr_t)d_table | (uintptr_t)d_score | (uintptr_t)d_class) & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "phase_score: bad argument (8-byte aligned d_pair_cell and d_int, 4-byte aligned d_table, d_score and d_class)");
    if (Q == 0) return AMPLI_OK;
    const int64_t groups = (Q + 255) / 256;
    if (groups > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "phase_score: too many pairs in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(phase_score_kernel, dim3((unsigned)groups), dim3(256), 0, main_stream(ctx), (const int *)d_table, (long long)P, (const long long *)d_pair_cell,
                       (const signed char *)d_pair_nt, (long long)Q, (int)min_alt, (int)min_share, (long long *)d_int, d_score, (int *)d_class);
    return check_launch(ctx, "phase_score_kernel");
}
