// amplisolve_amd/csrc/ampli_loo.hip -- leave-one-out: what the panel of normals calls in itself.
//
// loo_stream_kernel + loo_drain_kernel and their entry point ampli_loo_call_records.  The threshold gate, the rates, the queue's item,
// its hand-over and the drain's body are the ones error_reduce and poisson_call use (ampli_device.h); the queue itself and the lgamma
// table are poisson_call's (queue_prepare, ensure_lgtab: ampli_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// loo_stream_kernel<LAY,IRR>: for every normal s of a resident chunk and every position p, the calling gate of VC on
// s's records at p against the thresholds the OTHER S-1 normals give.  One lane owns one position: it loads the whole
// cohort's sums once (snt, srd, cnt, nrec: 148 B) and, for every row, subtracts the held-out sample's own contribution -- its
// records at p that pass the threshold gate error_reduce used (thr_gate) -- and finalises that row's S-1 table in registers
// (fin_rates, the text round trip).  Inside the exactness envelope every addend of snt is >= 0, so every partial sum of any subset
// is bounded by the total and exact: the difference IS the S-1 sum, in whatever order the reference would have added it.  Outside
// the envelope that fails: flag bit 0 (the caller refuses).
// A workgroup = 4 waves over one 64-position tile, wave w taking rows w, w + 4, ...; the per-position callable count is summed over
// the waves in LDS (no atomics), the per-sample one takes one reduction and one atomic per (wave, row).  Survivors of the prefilter
// go onto poisson_call's queue as PcItems carrying the raw S-1 thresholds, and loo_drain_kernel scores them.
template <int LAY, bool IRR>
__global__ __launch_bounds__(256) void loo_stream_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ dup_off, const int n, const AccPtrs acc,
    const float C, const int cov, const int call_cov, const unsigned char *__restrict__ ref_code, const int prefilter,
    PcItem *__restrict__ queue, const long long queue_per_shard, unsigned long long *__restrict__ queue_n,
    unsigned long long *__restrict__ n_calls, int *__restrict__ callable_pos, int *__restrict__ callable_sample,
    float *__restrict__ thr_loo, int *__restrict__ env_flags, int *__restrict__ ctx_flags)
{
    __shared__ PcItem stage[4][PC_STAGE];
    __shared__ int lds_callable[4][64];
    int staged = 0; // wave-uniform
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the call-list counters are reset here: only the drain, which starts after this kernel has finished, appends to the list
    if (n_calls && blockIdx.x == 0 && threadIdx.x < AMPLI_CALL_SHARDS) n_calls[threadIdx.x * AMPLI_CALL_COUNTER_STRIDE] = 0ull;
    const long long p_raw = (long long)blockIdx.x * 64 + lane;
    const bool valid = p_raw < P;
    const long long p = valid ? p_raw : P - 1;
    double tsnt[2][4];
    long long tsrd[2][4];
    int tcnt[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            tsnt[st][nt] = acc.snt[(st * 4 + nt) * P + p];
            tsrd[st][nt] = acc.srd[(st * 4 + nt) * P + p];
        }
        tcnt[nt] = acc.cnt[nt * P + p];
    }
    const int tnrec = acc.nrec[p];
    const int ref = valid ? (int)ref_code[p] : 255;
    const long long e0 = E > 0 ? (long long)dup_off[p] : 0;
    const int n_ext = E > 0 && valid ? (int)(dup_off[p + 1] - dup_off[p]) : 0;
    // the record loops below run n_ext_max + 1 times in EVERY lane: the queue staging inside them is wave-wide (ballots, the
    // wave-uniform fill count of the stage), so no lane may leave them early; a lane past its own records visits nothing
    int n_ext_max = n_ext;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n_ext_max = max(n_ext_max, __shfl_xor(n_ext_max, off));
    if (env_flags && wave == 0) { // the totals' exactness envelope (finalize_one's test): outside it the differences below are not the S-1 sums
        const double limit = envelope_limit(C, cov);
        bool bad = false;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bad |= !(tsnt[0][nt] < limit) || !(tsnt[1][nt] < limit);
        if (valid && bad) atomicOr(env_flags, 1);
    }
    const unsigned shard = blockIdx.x % AMPLI_CALL_SHARDS;
    int callable = 0; // this lane's callable records over this wave's rows
    for (int s = wave; s < n; s += 4) {
        // 1. the S-1 sums of (s, p): the totals minus s's records at p that pass the threshold gate
        double snt[2][4];
        long long srd[2][4];
        int cnt[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            snt[0][nt] = tsnt[0][nt]; snt[1][nt] = tsnt[1][nt];
            srd[0][nt] = tsrd[0][nt]; srd[1][nt] = tsrd[1][nt];
            cnt[nt] = tcnt[nt];
        }
        int m = 0;       // s's present records at p: nrec' = nrec - m
        bool any_live = false;
        for (int j = 0; j <= n_ext_max; ++j) { // the primary record, then the extras of p (record P + e0 + j - 1)
            const bool has = j <= n_ext;
            RecCounts a = rec_counts<LAY, IRR>(rv, P, E, s, j == 0 || !has ? p : P + e0 + j - 1);
            a.present &= has;
            m += a.present ? 1 : 0;
            const bool covok = a.present && a.FW >= cov && a.BW >= cov;
            any_live |= valid && a.present && ref <= 3 && a.FW >= call_cov && a.BW >= call_cov;
            const unsigned qual = thr_gate(a.fw, a.bw, a.FW, a.BW, covok, a.own_rd || a.RD >= AMPLI_COUNT_LIMIT); // big: as visit_record
            if (qual) {
                const double prod_fw = (double)((float)a.FW * C), prod_bw = (double)((float)a.BW * C); // EE:1597,1599
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if ((qual >> nt) & 1u) { // the addends of EE:1597-1606, taken out in the order they went in
                        snt[0][nt] = snt[0][nt] - (double)a.fw[nt] - prod_fw;
                        snt[1][nt] = snt[1][nt] - (double)a.bw[nt] - prod_bw;
                        srd[0][nt] -= a.FW;
                        srd[1][nt] -= a.BW;
                        cnt[nt] -= 1;
                    }
                }
            }
        }
        // 2. the S-1 table's thresholds: quorum, fp32 rate, NaN -> NONE, text round trip, 0.01 for NONE (finalize_one)
        float thr[2][4] = {{0.01f, 0.01f, 0.01f, 0.01f}, {0.01f, 0.01f, 0.01f, 0.01f}}; // read only where a record is live
        int tcode[4] = {1, 1, 1, 1};
        if (any_live || thr_loo) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                float r_fw, r_bw;
                const unsigned char c = tcode[nt] = fin_rates(snt[0][nt], snt[1][nt], srd[0][nt], srd[1][nt], cnt[nt], tnrec - m, r_fw, r_bw);
                thr[0][nt] = c ? 0.01f : ampli_text_roundtrip(r_fw); // EE:2680-2684 / EE:1704 -> VC:889-890
                thr[1][nt] = c ? 0.01f : ampli_text_roundtrip(r_bw);
                if (thr_loo && valid) {
                    thr_loo[((size_t)s * 8 + nt) * P + p] = thr[0][nt];
                    thr_loo[((size_t)s * 8 + 4 + nt) * P + p] = thr[1][nt];
                }
            }
        }
        // 3. VC's gate on each of s's records at p against those thresholds (poisson_stream_kernel's, per record)
        int row_callable = 0;
        for (int j = 0; j <= n_ext_max; ++j) {
            const bool has = j <= n_ext;
            const long long r = j == 0 || !has ? p : P + e0 + j - 1;
            RecCounts a = rec_counts<LAY, IRR>(rv, P, E, s, r);
            a.present &= has;
            const bool live = valid && a.present && ref <= 3 && a.FW >= call_cov && a.BW >= call_cov; // VC:898, VC:3290
            row_callable += live ? 1 : 0;
            const int d_fw = a.RD - a.BW, d_bw = a.BW; // VC:895-896
            const bool exact = prefilter && (unsigned)a.RD < (unsigned)AMPLI_COUNT_LIMIT && a.FW >= 0 && a.BW >= 0 && d_fw >= 0;
            const float c_fw = (float)d_fw * 0.999999f, c_bw = (float)d_bw * 0.999999f;
            unsigned pushmask = 0;
            if (live) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) { // ampli_prefilter_skip_f32: settles most pairs; what it does not skip is scored exactly
                    const bool skip_fw = exact && (unsigned)a.fw[nt] < (unsigned)AMPLI_COUNT_LIMIT && (float)a.fw[nt] <= c_fw * ampli_effective_err(thr[0][nt]);
                    const bool skip_bw = exact && (unsigned)a.bw[nt] < (unsigned)AMPLI_COUNT_LIMIT && (float)a.bw[nt] <= c_bw * ampli_effective_err(thr[1][nt]);
                    if (nt != ref && !skip_fw && !skip_bw) pushmask |= 1u << nt;
                }
            }
            // the staging of poisson_stream_kernel (ampli_kernels.hip), with another fill of the item
            if (__any(pushmask != 0)) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const bool push = (pushmask >> nt) & 1;
                    const unsigned long long bal = __ballot(push);
                    if (bal) {
                        const int k = __popcll(bal);
                        if (staged + k > PC_STAGE) {
                            pc_flush(stage[wave], staged, lane, queue, queue_per_shard, queue_n, shard, ctx_flags);
                            staged = 0;
                        }
                        if (push) {
                            PcItem it;
                            it.sample = s; it.record_alt = (int)r | (nt << 30);
                            it.k_fw = a.fw[nt]; it.k_bw = a.bw[nt]; it.FW = a.FW; it.BW = a.BW; it.rd = a.RD;
                            it.e_fw = thr[0][nt]; it.e_bw = thr[1][nt]; it.pad = tcode[nt];
                            stage[wave][staged + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0))] = it;
                        }
                        staged += k;
                    }
                }
            }
        }
        callable += row_callable;
        if (callable_sample) { // one reduction and one atomic per (wave, row)
            int w = row_callable;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) w += __shfl_xor(w, off);
            if (lane == 0 && w) atomicAdd(&callable_sample[s], w);
        }
    }
    if (staged) pc_flush(stage[wave], staged, lane, queue, queue_per_shard, queue_n, shard, ctx_flags);
    if (callable_pos) {
        lds_callable[wave][lane] = callable;
        __syncthreads();
        if (wave == 0 && valid) callable_pos[p] += lds_callable[0][lane] + lds_callable[1][lane] + lds_callable[2][lane] + lds_callable[3][lane];
    }
}

__global__ __launch_bounds__(256) void loo_drain_kernel(
    const PcItem *__restrict__ queue, const long long queue_per_shard, const unsigned long long *__restrict__ queue_n,
    const long long R, unsigned *__restrict__ mask_words, ampli_loo_call *__restrict__ calls, const long long capacity,
    unsigned long long *__restrict__ n_calls, unsigned long long *__restrict__ next_queue_n, const double *__restrict__ lgtab)
{
    drain_body<true>(queue, queue_per_shard, queue_n, R, mask_words, calls, capacity, n_calls, next_queue_n, 0, AMPLI_CALL_SHARDS, lgtab);
}

extern "C" int ampli_loo_call_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc, float C,
                                      int32_t cov, int32_t call_cov, const uint8_t *d_ref_code, int32_t mode, uint8_t *d_call_mask,
                                      ampli_loo_call *d_calls, int64_t capacity, unsigned long long *d_n_calls, int32_t *d_callable_pos,
                                      int32_t *d_callable_sample, float *d_thr_loo, int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || !d_ref_code || !d_call_mask || cov < 1 || call_cov < 1) return fail(ctx, AMPLI_E_INVALID, "loo_call: bad argument");
    if (!acc_is_bound(d_acc) || d_acc->P != P) return fail(ctx, AMPLI_E_INVALID, "loo_call: d_acc must be an ampli_acc_bind table of P positions");
    { int rc = check_records(ctx, co, "loo_call", co.dup_off, "dup_off"); if (rc) return rc; }
    if (mode != AMPLI_POISSON_FULL && mode != AMPLI_POISSON_PREFILTER) return fail(ctx, AMPLI_E_INVALID, "loo_call: bad mode");
    if (d_calls && (!d_n_calls || capacity < AMPLI_CALL_SHARDS)) return fail(ctx, AMPLI_E_INVALID, "loo_call: call list needs n_calls and capacity >= AMPLI_CALL_SHARDS");
    if (d_n_calls && !d_calls) capacity = 0;
    if (((uintptr_t)d_call_mask & 3) != 0) return fail(ctx, AMPLI_E_INVALID, "loo_call: call_mask must be 4-byte aligned");
    const long long E = co.E, R = P + E;
    const int n = co.n;
    if (R >= (1ll << 30)) return fail(ctx, AMPLI_E_RANGE, "loo_call: P + E must be below 2^30 records per sample");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcj = join_drain(ctx); if (rcj) return rcj; } // the queue and its counters are about to be reused
    { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
    hipStream_t st = main_stream(ctx);
    // all-scores mode queues every live (record, alt) pair: the drain's exact bound decides them all
    // items go to shard blockIdx.x % AMPLI_CALL_SHARDS, one workgroup = one tile of 64 positions: a shard takes at most
    // ceil(tiles / SHARDS) tiles' worth of pairs (3 alternatives of every record of the tile's positions, extras included), which is
    // what the all-scores mode sizes for; ampli_set_queue_items raises either mode's size
    const unsigned tiles = (unsigned)((P + 63) / 64);
    const size_t shard_tiles = (tiles + AMPLI_CALL_SHARDS - 1) / AMPLI_CALL_SHARDS;
    size_t want = mode == AMPLI_POISSON_FULL ? (size_t)AMPLI_CALL_SHARDS * shard_tiles * 3 * ((size_t)n * 64 + (size_t)n * (size_t)E)
                                             : (size_t)std::max<long long>(1 << 16, (long long)n * R / 4);
    if (ctx->queue_min_items) want = std::max(want, ctx->queue_min_items + (size_t)AMPLI_CALL_SHARDS * shard_tiles * 3 * 64 * (size_t)n);
    long long per;
    unsigned long long *qn, *qn_next;
    { int rcq = queue_prepare(ctx, ctx->lanes[0].q, want, st, per, qn, qn_next); if (rcq) return rcq; }
    HIP_TRY(ctx, hipMemsetAsync(d_call_mask, 0, ((size_t)n * (size_t)R + 3) / 4 * 4, st));
    with_layout(co.layout, [&](auto L) {
        with_bool(co.rv.rd || co.rv.rd_ext, [&](auto IRR) {
            hipLaunchKernelGGL((loo_stream_kernel<L, IRR>), dim3(tiles), dim3(256), 0, st, co.rv, (long long)P, E, co.dup_off, n, to_ptrs(d_acc), C,
                               (int)cov, (int)call_cov, d_ref_code, mode == AMPLI_POISSON_PREFILTER ? 1 : 0, (PcItem *)ctx->lanes[0].q.items, per, qn,
                               d_n_calls, d_callable_pos, d_callable_sample, d_thr_loo, d_flags, ctx->d_flags);
        });
    });
    { int rc = check_launch(ctx, "loo_stream_kernel"); if (rc) return rc; }
    const unsigned dgy = (unsigned)(ctx->pc_drain_blocks > 0 ? ctx->pc_drain_blocks
                                                             : std::min<long long>(1024, std::max<long long>(16, (long long)n * R / 300000)));
    hipLaunchKernelGGL(loo_drain_kernel, dim3(AMPLI_CALL_SHARDS, dgy), dim3(256), 0, st, (const PcItem *)ctx->lanes[0].q.items, per, qn, (long long)R,
                       (unsigned *)d_call_mask, d_calls, (long long)capacity, d_n_calls, qn_next, (const double *)ctx->d_lgtab);
    return check_launch(ctx, "loo_drain_kernel");
}
