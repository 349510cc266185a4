// amplisolve_amd/csrc/ampli_kernels.hip -- the kernels of the step bench.py times, their launchers and C ABI (gfx950, wave64); and the
// map of the kernel translation units of libamplisolve_hip.so.
//
// HBM-bound integer / scalar-FP work, no MFMA.  LAY = record layout (AMPLI_RECORDS_I32 / _U16 / _U24: 32 / 16 / 24 bytes per record).
// The units follow the path; every stage holds its kernels, then their launchers and entry points.  A kernel is defined and launched
// in one unit only; where another unit needs it, it calls a host launcher declared in ampli_device.h.
// This file (bench.py's kernel_source_sha() covers it and ampli_math.h):
//   records            records_pack16_kernel / records_pack24_kernel   int32 records -> the packed layouts
//   error reduce       error_reduce_kernel<FAST,G,LAY>   EE:1149-1296 (+clones), EE:1565-1631 (+clones)   one record read per
//                        (position, sample); epilogue: fused finalize_lane (one GPU), packed sums (all-reduce merge) or slice-major
//                        sums + germ-max pairs (position-sliced merge)
//                      error_reduce_u16_kernel / error_reduce_u24_kernel<DUP,TAB>   the same with a compact per-position state, the
//                        shipped shape for packed records; dup_tiles_kernel lists the tiles they leave to error_reduce_kernel
//                      acc_merge_kernel / acc_pack_sliced_kernel   after a cut along the samples: the partial tables folded in order,
//                        the merged table -> slice-major exchange buffers
//                      error_sums_inorder_kernel<LAY>   the eight threshold sums in the reference's own order (outside the envelope)
//   finalize           error_finalize_kernel   EE:1659-1714 (+clones), sentinel rule EE:1260/1318/1374/1431, text round trip
//                        EE:1704 -> VC:889
//   Poisson            poisson_stream_kernel<LAY,IRR> + poisson_drain_kernel   VC:752-898 (+clones), VC:3721-3884   prefilter mode:
//                        one record read per (position, tumour), the few scores past the gate queued and drained
//                      poisson_full_kernel<LAY>   all-scores mode: light scores in place, heavy ones compacted per workgroup
//                      poisson_call_kernel<MODE,LAY>   one lane per record, every score in place: the dense VAF output (either mode)
//                      lgamma_table_kernel   kf_lgamma at the integers, for the drain and the all-scores mode
//                      queue_counters_reset_kernel   the prefilter queue's counters inside a captured graph
// ampli_exchange.hip   merges and slices of the multi-GPU paths:
//                      acc_merge_ptr_kernel / gm_merge_kernel   ordered combines of partial accumulator tables
//                      acc_pack_kernel / acc_unpack_kernel   additive planes <-> exchange buffers
//                      error_finalize_slice_kernel -> error_table_unslice_kernel   one slice's error-table block -> plane-major table
//                      error_finalize_merged_kernel   finalize from the all-reduced sums and the gathered germ-max regions
// ampli_loo.hip        leave-one-out: loo_stream_kernel<LAY,IRR> + loo_drain_kernel   the panel of normals against its S-1 tables
// ampli_limits.hip     detection limits and power: limit_pairs_kernel<LAY,IRR>   the smallest counts the gate of VC:898 would pass, per
//                        record and base; limit_power_kernel<LAY>   the gate's power at given allele fractions, LoD
// ampli_aux.hip        score_batch_kernel / score_dense_batch_kernel / roundtrip_batch_kernel   scorer and text round trip on lists
//                      synth_fill_kernel / synth_ref_kernel   synthetic panels (ampli_synth.h)
// ampli_device.h       what more than one of these units needs: record types and decode, accumulator state, finalize, the queue's item,
//                        hand-over and drain body, launch dispatch, the host helpers one unit defines for the others
// See include/amplisolve_hip.h for the data layout and DESIGN.md for the rooflines.  The library's other translation units:
// ampli_runtime.hip (context, streams, memory, settings), ampli_pileup.hip (pileup_count_kernel, the step upstream of the path),
// ampli_indel.hip, ampli_amplicon_count.hip, ampli_evidence.hip (the other walks over a BAM stream's records), ampli_bam.h (the record
// layout, the position keys and their searches, the base decode and the CIGAR classes those four walks share),
// ampli_comm.hip (RCCL binding of the multi-GPU merge), ampli_internal.h (the context and the stream helpers they all share).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// ==== records: layouts, the cohort a kernel reads, int32 -> packed records =============================================================

// the record types, rec_load_at / rec_decode, RecView and DevCohort: ampli_device.h

// 8 x int32 records -> 8 x uint16 records (AMPLI_ABSENT -> 0xFFFF); *overflow is raised for a count above 65534
__global__ __launch_bounds__(256) void records_pack16_kernel(const int4 *__restrict__ in, const long long n, uint4 *__restrict__ out,
                                                             int *__restrict__ overflow)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 a = in[i * 2], b = in[i * 2 + 1];
    const bool absent = a.x == AMPLI_ABSENT;
    const unsigned v[8] = {absent ? 0xFFFFu : (unsigned)a.x, (unsigned)a.y, (unsigned)a.z, (unsigned)a.w,
                           (unsigned)b.x, (unsigned)b.y, (unsigned)b.z, (unsigned)b.w};
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) bad |= (j == 0 && absent) ? false : v[j] > 65534u;
    if (bad) atomicOr(overflow, 1);
    out[i] = make_uint4((v[0] & 0xFFFFu) | (v[1] << 16), (v[2] & 0xFFFFu) | (v[3] << 16), (v[4] & 0xFFFFu) | (v[5] << 16),
                        (v[6] & 0xFFFFu) | (v[7] << 16));
}

// 8 x int32 records -> 8 x 24-bit records (AMPLI_ABSENT -> 0xFFFFFF); *overflow is raised for a count above 2^24 - 2
__global__ __launch_bounds__(256) void records_pack24_kernel(const int4 *__restrict__ in, const long long n, uint2 *__restrict__ out,
                                                             int *__restrict__ overflow)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 a = in[i * 2], b = in[i * 2 + 1];
    const bool absent = a.x == AMPLI_ABSENT;
    const unsigned v[8] = {absent ? 0xFFFFFFu : (unsigned)a.x, (unsigned)a.y, (unsigned)a.z, (unsigned)a.w,
                           (unsigned)b.x, (unsigned)b.y, (unsigned)b.z, (unsigned)b.w};
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) bad |= (j == 0 && absent) ? false : v[j] > 0xFFFFFEu;
    if (bad) atomicOr(overflow, 1);
    unsigned w[6];
#pragma unroll
    for (int h = 0; h < 2; ++h) { // four 24-bit fields -> three dwords
        const unsigned f0 = v[4 * h] & 0xFFFFFFu, f1 = v[4 * h + 1] & 0xFFFFFFu, f2 = v[4 * h + 2] & 0xFFFFFFu, f3 = v[4 * h + 3] & 0xFFFFFFu;
        w[3 * h] = f0 | (f1 << 24);
        w[3 * h + 1] = (f1 >> 8) | (f2 << 16);
        w[3 * h + 2] = (f2 >> 16) | (f3 << 8);
    }
    out[i * 3] = make_uint2(w[0], w[1]);
    out[i * 3 + 1] = make_uint2(w[2], w[3]);
    out[i * 3 + 2] = make_uint2(w[4], w[5]);
}

// the dense interchange layout [n][P+E] in the context's record layout (the classic entry points)
static DevCohort dense_cohort(const ampli_ctx *ctx, const void *d_recs, int64_t P, int64_t E, int n, const uint32_t *dup_off,
                              const uint32_t *ext_pos)
{
    DevCohort c;
    c.layout = ctx->rec_layout;
    c.rv.base = (const char *)d_recs;
    c.rv.row_stride = P + E;
    c.rv.ext = (const char *)d_recs + (size_t)P * rec_bytes(c.layout);
    c.rv.ext_stride = P + E;
    c.rv.rd = nullptr; c.rv.rd_ext = nullptr;
    c.n = n; c.E = E; c.dup_off = dup_off; c.ext_pos = ext_pos;
    return c;
}

int cohort_from_records(ampli_ctx *ctx, const ampli_records *r, int64_t P, DevCohort &c)
{
    if (!r || !r->recs || r->n_samples <= 0 || r->E < 0) return fail(ctx, AMPLI_E_INVALID, "records: recs, n_samples > 0 and E >= 0 are required");
    if (r->layout != AMPLI_RECORDS_I32 && r->layout != AMPLI_RECORDS_U16 && r->layout != AMPLI_RECORDS_U24)
        return fail(ctx, AMPLI_E_INVALID, "records: unknown layout");
    c.layout = r->layout;
    c.n = r->n_samples;
    c.E = r->E;
    c.dup_off = r->dup_off; c.ext_pos = r->ext_pos;
    c.rv.rd = r->rd;
    c.rv.rd_ext = r->rd_ext;
    c.rv.base = (const char *)r->recs;
    c.rv.row_stride = r->row_stride > 0 ? r->row_stride : (r->ext ? P : P + r->E);
    if (r->ext) {
        c.rv.ext = (const char *)r->ext;
        c.rv.ext_stride = r->ext_stride > 0 ? r->ext_stride : r->E;
        if (c.rv.row_stride < P || c.rv.ext_stride < r->E) return fail(ctx, AMPLI_E_INVALID, "records: row_stride < P or ext_stride < E");
    } else {
        c.rv.ext = c.rv.base + (size_t)P * rec_bytes(c.layout);
        c.rv.ext_stride = c.rv.row_stride;
        if (c.rv.row_stride < P + r->E) return fail(ctx, AMPLI_E_INVALID, "records: row_stride < P + E");
    }
    return AMPLI_OK;
}

// what every kernel reading a cohort needs of it: extras come with their index (`index`, called `index_name` in the message;
// index_name == nullptr: the kernel needs no index of the extras and none is asked for),
// records 16-byte aligned (8-byte in the 24-byte layout)
int check_records(ampli_ctx *ctx, const DevCohort &co, const char *what, const uint32_t *index, const char *index_name)
{
    if (co.E > 0 && !index && index_name) return fail(ctx, AMPLI_E_INVALID, (std::string(what) + ": E > 0 needs " + index_name).c_str());
    const uintptr_t am = co.layout == AMPLI_RECORDS_U24 ? 7 : 15;
    if (((uintptr_t)co.rv.base & am) != 0 || (co.E > 0 && ((uintptr_t)co.rv.ext & am) != 0))
        return fail(ctx, AMPLI_E_INVALID, (std::string(what) + ": recs must be 16-byte aligned (8-byte for the 24-byte layout)").c_str());
    return AMPLI_OK;
}

extern "C" int ampli_records_pack16(ampli_ctx *ctx, const int32_t *d_recs32, int64_t n_records, void *d_recs16, int32_t *d_overflow)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_recs32 || !d_recs16 || !d_overflow || n_records <= 0 || ((uintptr_t)d_recs32 & 15) || ((uintptr_t)d_recs16 & 15))
        return fail(ctx, AMPLI_E_INVALID, "records_pack16: bad argument (16-byte aligned buffers, n_records > 0, overflow word)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(records_pack16_kernel, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, main_stream(ctx), (const int4 *)d_recs32,
                       (long long)n_records, (uint4 *)d_recs16, d_overflow);
    return check_launch(ctx, "records_pack16_kernel");
}

extern "C" int ampli_records_pack24(ampli_ctx *ctx, const int32_t *d_recs32, int64_t n_records, void *d_recs24, int32_t *d_overflow)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_recs32 || !d_recs24 || !d_overflow || n_records <= 0 || ((uintptr_t)d_recs32 & 15) || ((uintptr_t)d_recs24 & 7))
        return fail(ctx, AMPLI_E_INVALID, "records_pack24: bad argument (aligned buffers, n_records > 0, overflow word)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(records_pack24_kernel, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, main_stream(ctx), (const int4 *)d_recs32,
                       (long long)n_records, (uint2 *)d_recs24, d_overflow);
    return check_launch(ctx, "records_pack24_kernel");
}

// ==== error reduce: records -> accumulator table (or straight to an error table / exchange buffers) ====================================

// ---------------------------------------------------------------------------
// accumulator table layout
// ---------------------------------------------------------------------------
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// every plane starts 256-byte aligned
void acc_offsets(int64_t P, size_t off[9])
{
    size_t o = 0;
    off[0] = o; o = align_up(o + (size_t)P * 8 * sizeof(double), 256);   // snt
    off[1] = o; o = align_up(o + (size_t)P * 8 * sizeof(int64_t), 256);  // srd
    off[2] = o; o = align_up(o + (size_t)P * 4 * sizeof(int32_t), 256);  // cnt
    off[3] = o; o = align_up(o + (size_t)P * 1 * sizeof(int32_t), 256);  // nrec
    // memory order: gm_n | gm_first_af | gm_rest | gm_first -- the first three are what shards exchange (the "gm
    // region"); gm_first is bookkeeping and stays local
    off[4] = o; o = align_up(o + (size_t)P * 4 * sizeof(int32_t), 256);  // gm_n
    off[6] = o; o = align_up(o + (size_t)P * 4 * sizeof(float), 256);    // gm_first_af
    off[7] = o; o = align_up(o + (size_t)P * 4 * sizeof(float), 256);    // gm_rest
    off[5] = o; o = align_up(o + (size_t)P * 4 * sizeof(int32_t), 256);  // gm_first
    off[8] = o;
}

extern "C" size_t ampli_acc_bytes(int64_t P)
{
    if (P <= 0) return 0;
    size_t off[9];
    acc_offsets(P, off);
    return off[8];
}

extern "C" int ampli_acc_bind(void *base, int64_t P, ampli_acc_table *out)
{
    if (!base || !out || P <= 0) return AMPLI_E_INVALID;
    size_t off[9];
    acc_offsets(P, off);
    char *b = (char *)base;
    out->P = P;
    out->snt = (double *)(b + off[0]);
    out->srd = (int64_t *)(b + off[1]);
    out->cnt = (int32_t *)(b + off[2]);
    out->nrec = (int32_t *)(b + off[3]);
    out->gm_n = (int32_t *)(b + off[4]);
    out->gm_first = (int32_t *)(b + off[5]);
    out->gm_first_af = (float *)(b + off[6]);
    out->gm_rest = (float *)(b + off[7]);
    return AMPLI_OK;
}

__device__ __forceinline__ void lane_acc_init(LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        a.snt[0][nt] = 0.0; a.snt[1][nt] = 0.0;
        a.srd[0][nt] = 0; a.srd[1][nt] = 0;
        a.cnt[nt] = 0;
        a.gm_n[nt] = 0;
        a.gm_first[nt] = 0x7fffffff;
        a.gm_first_af[nt] = 0.0f;
        a.gm_rest[nt] = -INFINITY;
    }
    a.nrec = 0;
}

// One record of one sample at this lane's position.  r0 = {Afw,Cfw,Gfw,Tfw}, r1 = {Ars,Crs,Grs,Trs}.
// rd_col: the RD column of an irregular line (RD != A+C+G+T), AMPLI_ABSENT otherwise.
__device__ __forceinline__ void visit_record(LaneAcc &a, const int4 r0, const int4 r1, const int sample,
                                             const float C, const int cov, const int rd_col = AMPLI_ABSENT)
{
    const bool present = r0.x != AMPLI_ABSENT;
    const int fw[4] = {r0.x, r0.y, r0.z, r0.w};
    const int bw[4] = {r1.x, r1.y, r1.z, r1.w};
    const int FW = fw[0] + fw[1] + fw[2] + fw[3];  // EE:1175
    const int BW = bw[0] + bw[1] + bw[2] + bw[3];  // EE:1176
    const bool irregular = rd_col != AMPLI_ABSENT; // EE:1178-1181: such a line is used with its own RD (EE:1229-1232)
    const int RD = irregular ? rd_col : FW + BW;   // the ASEQ RD column
    const bool covok = present && FW >= cov && BW >= cov; // EE:1595, EE:1251 (cov >= 1)
    a.nrec += present ? 1 : 0;                     // Value_Hash.count(key), EE:1659
    if (!__any(covok)) return;                     // wave-uniform: nothing below can change state

    // AF <= 0.05 as an integer bound (ampli_math.h); fp form for counts beyond exact floats
    const bool big = irregular || RD >= AMPLI_COUNT_LIMIT; // the literal fp gates: any RD, also a negative or zero one
    const unsigned qual = thr_gate(fw, bw, FW, BW, covok, big);
    const int lim_rd = ampli_af_limit(RD);
    // EE:1597,1599: float(RD_s)*float(C), an fp32 product widened to double
    const double prod_fw = (double)((float)FW * C);
    const double prod_bw = (double)((float)BW * C);
    const float rdf = (float)RD;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        bool g_tot = (fw[nt] + bw[nt]) <= lim_rd;
        if (big) g_tot = ampli_af_gate_fp(fw[nt] + bw[nt], RD); // never taken for real panels
        if ((qual >> nt) & 1u) { // EE:1595
            a.snt[0][nt] = a.snt[0][nt] + (double)fw[nt] + prod_fw; // EE:1597
            a.srd[0][nt] += FW;                                     // EE:1598
            a.snt[1][nt] = a.snt[1][nt] + (double)bw[nt] + prod_bw; // EE:1599
            a.srd[1][nt] += BW;                                     // EE:1600
            a.cnt[nt] += 1;                                         // EE:1606
        }
        if (covok && g_tot) { // EE:1251 (+ clones at 1309, 1365, 1422)
            const float af = (float)(fw[nt] + bw[nt]) / rdf; // EE:1229-1232
            if (a.gm_n[nt] == 0) {
                a.gm_first[nt] = sample;
                a.gm_first_af[nt] = af;
            } else if (a.gm_rest[nt] <= af) { // EE:1266
                a.gm_rest[nt] = af;
            }
            a.gm_n[nt] += 1;
        }
    }
}

__device__ __forceinline__ AccPtrs acc_at(char *base, long long /*P*/, size_t o0, size_t o1, size_t o2, size_t o3,
                                          size_t o4, size_t o5, size_t o6, size_t o7)
{
    AccPtrs a;
    a.snt = (double *)(base + o0); a.srd = (long long *)(base + o1); a.cnt = (int *)(base + o2);
    a.nrec = (int *)(base + o3); a.gm_n = (int *)(base + o4); a.gm_first = (int *)(base + o5);
    a.gm_first_af = (float *)(base + o6); a.gm_rest = (float *)(base + o7);
    return a;
}

__device__ __forceinline__ void lane_acc_store_packed(double *__restrict__ pk, const long long P, const long long p, const LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        pk[(0 * 4 + nt) * P + p] = a.snt[0][nt];
        pk[(1 * 4 + nt) * P + p] = a.snt[1][nt];
        pk[8 * P + (0 * 4 + nt) * P + p] = (double)a.srd[0][nt];
        pk[8 * P + (1 * 4 + nt) * P + p] = (double)a.srd[1][nt];
        pk[16 * P + nt * P + p] = (double)a.cnt[nt];
    }
    pk[20 * P + p] = (double)a.nrec;
}

// slice-major stores for the reduce-scatter merge: each destination rank's slice is one contiguous chunk
// (Acc: LaneAcc, or the compact kernel's Part16 -- the same fields under the same names)
template <class Acc> __device__ __forceinline__ void lane_acc_store_sliced(const FinOut &o, const long long p, const Acc &a)
{
    const long long L = o.slice_len, k = p / L, q = p - k * L;
    double *__restrict__ pk = o.sl_sums + (size_t)k * o.sl_group * slice_planes(o.sl_fmt) * L + q;
    float *__restrict__ gm = o.sl_gm + (size_t)k * o.sl_group * 8 * L + q;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        pk[(0 * 4 + nt) * L] = a.snt[0][nt];
        pk[(1 * 4 + nt) * L] = a.snt[1][nt];
        // what the ordered fold needs of a shard: whether it has a qualifying record, its first AF, the max of the rest
        gm[nt * L] = a.gm_n[nt] > 0 ? a.gm_first_af[nt] : -1.0f;
        gm[(4 + nt) * L] = a.gm_n[nt] > 1 ? a.gm_rest[nt] : -INFINITY;
    }
    if (o.sl_fmt == AMPLI_SLICE_SLIM) {
        const long long lim_d = (1ll << 26) / o.sl_n, lim_c = (1ll << 17) / o.sl_n; // this shard's share of a field
        bool fits = (long long)a.nrec < lim_c;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            fits = fits && a.srd[0][nt] >= 0 && a.srd[0][nt] < lim_d && a.srd[1][nt] >= 0 && a.srd[1][nt] < lim_d && (long long)a.cnt[nt] < lim_c;
            pk[(8 + nt) * L] = (double)a.srd[0][nt] + (double)a.srd[1][nt] * SLIM_D;
        }
        pk[12 * L] = (double)a.cnt[0] + (double)a.cnt[1] * SLIM_C + (double)a.cnt[2] * SLIM_C2;
        pk[13 * L] = (double)a.cnt[3] + (double)a.nrec * SLIM_C;
        if (!fits && o.sl_flags) atomicOr(o.sl_flags, AMPLI_FLAG_SLICE_RANGE);
        return;
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        pk[(8 + 0 * 4 + nt) * L] = (double)a.srd[0][nt];
        pk[(8 + 1 * 4 + nt) * L] = (double)a.srd[1][nt];
        pk[(16 + nt) * L] = (double)a.cnt[nt];
    }
    pk[20 * L] = (double)a.nrec;
}

// germ-max planes only (the additive planes travel in the packed buffer)
__device__ __forceinline__ void lane_acc_store_gm(const AccPtrs &t, const long long P, const long long p, const LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        t.gm_n[nt * P + p] = a.gm_n[nt];
        t.gm_first[nt * P + p] = a.gm_first[nt];
        t.gm_first_af[nt * P + p] = a.gm_first_af[nt];
        t.gm_rest[nt * P + p] = a.gm_rest[nt];
    }
}

// ---------------------------------------------------------------------------
// Fast per-lane state (the shipped inner loop).  Same results as LaneAcc /
// visit_record, fewer instructions per record:
//   * the qualifying sums are kept as an integer part (sum of X, sum of depth,
//     int32 / int64) and a double part (sum of
//     the fp32 products); snt = (double)sumX + sumP is exact inside the
//     envelope of DESIGN.md section 4, like every other association;
//   * Germ_Max needs max over records of RN(x/d); RN is monotone, so the
//     argmax of the exact fraction is tracked by cross-multiplication (two
//     24-bit multiplies per side) and ONE division per lane is done at the end
//     instead of one IEEE fp32 division per record and nucleotide.
// Valid while every depth is < 2^22 (FAST_COUNT_LIMIT): beyond that a lane
// raises AMPLI_FLAG_RERUN_GENERAL and the caller reruns the literal kernel.
// ---------------------------------------------------------------------------
constexpr int FAST_COUNT_LIMIT = 1 << 22;
constexpr int FAST_MAX_CHUNK = 1024;      // samples per lane: sum of X (<= 0.05 x 2^22 each) stays below 2^31 for 8191 records
constexpr int FAST_MAX_RECORDS = 8191;    // records per lane (samples x (1 + extras)) before the int32 sum of X could wrap

struct FastAcc {
    int sx[2][4];     // sum of X over qualifying records
    long long sd[2][4]; // sum of strand depth over qualifying records
    double sp[2][4];  // sum of float(depth)*float(C) over qualifying records
    int cnt[4];
    int nrec;
    int gn[4], gfx[4], gfd[4], gfi[4]; // germ-max: qualifying count; first record as a fraction + its sample index
    int gbx[4], gbd[4];                // best later record as a fraction (0/1 until one exists)
    int bad;                           // a depth beyond FAST_COUNT_LIMIT was seen
    // wave-uniform: lanes whose gn[nt] is still 0.  Lets the steady state of the Germ_Max tracking skip the
    // "first qualifying record" bookkeeping (LEAN visits only; kept in scalar registers)
    unsigned long long zmask[4];
};

__device__ __forceinline__ void fast_init(FastAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        a.sx[0][nt] = a.sx[1][nt] = 0;
        a.sd[0][nt] = a.sd[1][nt] = 0;
        a.sp[0][nt] = a.sp[1][nt] = 0.0;
        a.cnt[nt] = 0;
        a.gn[nt] = 0; a.gfx[nt] = 0; a.gfd[nt] = 1; a.gfi[nt] = 0x7fffffff;
        a.gbx[nt] = 0; a.gbd[nt] = 1;
        a.zmask[nt] = ~0ull;
    }
    a.nrec = 0;
    a.bad = 0;
}

// 48-bit product of two values known to be < 2^24 (v_mul_u32_u24 + v_mul_hi_u32_u24, both full rate)
__device__ __forceinline__ unsigned long long mul24x24(int a, int b)
{
    return (unsigned long long)((unsigned)a & 0xFFFFFFu) * (unsigned long long)((unsigned)b & 0xFFFFFFu);
}

// the same as two named instructions (both full rate, both read only the low 24 bits of their operands): left to itself
// hipcc turns some of these products into v_mad_u64_u32, which takes four passes
__device__ __forceinline__ unsigned long long mul24x24_pair(int a, int b)
{
    unsigned lo, hi;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    return ((unsigned long long)hi << 32) | lo;
}
// LEAN: the caller guarantees a full, converged wave (no lane group / extras divergence) and keeps a.zmask current.
template <bool LEAN>
__device__ __forceinline__ void visit_fast(FastAcc &a, const int4 r0, const int4 r1, const int sample, const float C,
                                           const int cov)
{
    const bool present = r0.x != AMPLI_ABSENT;
    const int fw[4] = {r0.x, r0.y, r0.z, r0.w};
    const int bw[4] = {r1.x, r1.y, r1.z, r1.w};
    const int FW = fw[0] + fw[1] + fw[2] + fw[3];  // EE:1175
    const int BW = bw[0] + bw[1] + bw[2] + bw[3];  // EE:1176
    const int RD = FW + BW;
    const bool covok = present && FW >= cov && BW >= cov; // EE:1595, EE:1251
    a.nrec += present ? 1 : 0;                     // EE:1659
    if (!__any(covok)) return;
    a.bad |= (covok && (unsigned)RD >= (unsigned)FAST_COUNT_LIMIT) ? 1 : 0;
    const int lim_fw = ampli_af_limit(FW), lim_bw = ampli_af_limit(BW), lim_rd = ampli_af_limit(RD);
    const double prod_fw = (double)((float)FW * C); // EE:1597
    const double prod_bw = (double)((float)BW * C); // EE:1599
    const unsigned long long covmask = LEAN ? __builtin_amdgcn_ballot_w64(covok) : 0ull;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (covok && fw[nt] <= lim_fw && bw[nt] <= lim_bw) { // EE:1595
            a.sx[0][nt] += fw[nt]; a.sd[0][nt] += FW; a.sp[0][nt] += prod_fw; // EE:1597-1598
            a.sx[1][nt] += bw[nt]; a.sd[1][nt] += BW; a.sp[1][nt] += prod_bw; // EE:1599-1600
            a.cnt[nt] += 1;                                                   // EE:1606
        }
        const int x = fw[nt] + bw[nt];
        const bool pass = covok && x <= lim_rd; // EE:1251: float(X)/float(RD) <= 0.05
        if (LEAN) {
            // straight-line steady state: every passing lane already holds its first record, so only "x/RD > best" is
            // left (EE:1266).  A lane meeting its FIRST qualifying record (its AF is dropped by the reference,
            // EE:1258-1261) is dealt with in the rare wave-uniform block and taken out of this row's comparison.
            bool cand = pass;
            // the wave mask straight from the compare (a ballot of the bool costs a v_cndmask + v_cmp pair per nucleotide)
            if ((__builtin_amdgcn_uicmp((unsigned)x, (unsigned)lim_rd, 37 /*ule*/) & covmask) & a.zmask[nt]) {
                const bool is_first = pass && a.gn[nt] == 0;
                if (is_first) { a.gfx[nt] = x; a.gfd[nt] = RD; a.gfi[nt] = sample; a.gn[nt] = 1; }
                a.zmask[nt] = __builtin_amdgcn_ballot_w64(a.gn[nt] == 0);
                cand = pass && !is_first;
            }
            const bool better = cand && mul24x24(x, a.gbd[nt]) > mul24x24(a.gbx[nt], RD); // ties keep the value
            a.gbx[nt] = better ? x : a.gbx[nt];
            a.gbd[nt] = better ? RD : a.gbd[nt];
            a.gn[nt] += cand ? 1 : 0;
        } else if (pass) {
            if (a.gn[nt] == 0) {    // first qualifying record: its AF is dropped by the reference (EE:1258-1261)
                a.gfx[nt] = x; a.gfd[nt] = RD; a.gfi[nt] = sample;
            } else if (mul24x24(x, a.gbd[nt]) > mul24x24(a.gbx[nt], RD)) { // x/RD > best: EE:1266 (ties keep the value)
                a.gbx[nt] = x; a.gbd[nt] = RD;
            }
            a.gn[nt] += 1;
        }
    }
}

// ---------------------------------------------------------------------------
// error_reduce: workgroup = 4 waves x 64 positions.  Wave w of workgroup
// (tile, split) owns the contiguous sample chunk c = split*4 + w and streams
// its 64 positions' 32-byte records (2 KiB contiguous per sample row, two
// dwordx4 per lane), UNROLL rows in flight.  The 4 per-wave partials are
// combined in sample order through LDS; split > 1 leaves one partial table per
// split for acc_merge_kernel.
// ---------------------------------------------------------------------------
constexpr int RED_WAVES = 4;

__device__ __forceinline__ void fast_to_lane(const FastAcc &f, LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            a.snt[st][nt] = (double)f.sx[st][nt] + f.sp[st][nt];
            a.srd[st][nt] = (long long)f.sd[st][nt];
        }
        a.cnt[nt] = f.cnt[nt];
        a.gm_n[nt] = f.gn[nt];
        a.gm_first[nt] = f.gfi[nt];
        a.gm_first_af[nt] = f.gn[nt] > 0 ? (float)f.gfx[nt] / (float)f.gfd[nt] : 0.0f; // EE:1229-1232
        a.gm_rest[nt] = f.gn[nt] > 1 ? (float)f.gbx[nt] / (float)f.gbd[nt] : -INFINITY;
    }
    a.nrec = f.nrec;
}

// LDS staging for the ordered combine of the 4 wave partials: a two-level tree (waves 1,3 -> 0,2; then 2 -> 0)
// needs room for two partials only (27 KB instead of 40 KB: four workgroups per CU instead of three).
struct RedShared {
    double snt[2][8][64];
    long long srd[2][8][64];
    int ints[2][13][64];
    float flts[2][8][64];
};

__device__ __forceinline__ void lds_put(RedShared &sh, const int slot, const int lane, const LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        sh.snt[slot][nt][lane] = a.snt[0][nt]; sh.snt[slot][4 + nt][lane] = a.snt[1][nt];
        sh.srd[slot][nt][lane] = a.srd[0][nt]; sh.srd[slot][4 + nt][lane] = a.srd[1][nt];
        sh.ints[slot][nt][lane] = a.cnt[nt];
        sh.ints[slot][4 + nt][lane] = a.gm_n[nt];
        sh.ints[slot][8 + nt][lane] = a.gm_first[nt];
        sh.flts[slot][nt][lane] = a.gm_first_af[nt];
        sh.flts[slot][4 + nt][lane] = a.gm_rest[nt];
    }
    sh.ints[slot][12][lane] = a.nrec;
}

__device__ __forceinline__ void lds_get(const RedShared &sh, const int slot, const int lane, LaneAcc &b)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        b.snt[0][nt] = sh.snt[slot][nt][lane]; b.snt[1][nt] = sh.snt[slot][4 + nt][lane];
        b.srd[0][nt] = sh.srd[slot][nt][lane]; b.srd[1][nt] = sh.srd[slot][4 + nt][lane];
        b.cnt[nt] = sh.ints[slot][nt][lane];
        b.gm_n[nt] = sh.ints[slot][4 + nt][lane];
        b.gm_first[nt] = sh.ints[slot][8 + nt][lane];
        b.gm_first_af[nt] = sh.flts[slot][nt][lane];
        b.gm_rest[nt] = sh.flts[slot][4 + nt][lane];
    }
    b.nrec = sh.ints[slot][12][lane];
}

__device__ __forceinline__ void lane_acc_shfl_down(const LaneAcc &a, LaneAcc &b, const int off)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        b.snt[0][nt] = __shfl_down(a.snt[0][nt], off); b.snt[1][nt] = __shfl_down(a.snt[1][nt], off);
        b.srd[0][nt] = __shfl_down(a.srd[0][nt], off); b.srd[1][nt] = __shfl_down(a.srd[1][nt], off);
        b.cnt[nt] = __shfl_down(a.cnt[nt], off);
        b.gm_n[nt] = __shfl_down(a.gm_n[nt], off);
        b.gm_first[nt] = __shfl_down(a.gm_first[nt], off);
        b.gm_first_af[nt] = __shfl_down(a.gm_first_af[nt], off);
        b.gm_rest[nt] = __shfl_down(a.gm_rest[nt], off);
    }
    b.nrec = __shfl_down(a.nrec, off);
}

// G lane groups per wave: a wave covers 64/G positions and G consecutive sample chunks (group g of wave w of
// workgroup (tile, split) owns chunk ((split*4 + w)*G + g)).  More, shorter waves for the same panel: the launch
// then runs several balanced rounds instead of one and a half long ones (the fixed ~24 us of ramp + tail measured
// at G = 1 shrinks with the wave lifetime).  A lane group still reads >= 512 contiguous bytes per sample row.
template <bool FAST, int G, int LAY>
__global__ __launch_bounds__(256) void error_reduce_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ dup_off,
    const int S, const int first_sample, const int chunk_len, const float C, const int cov, char *out_base,
    const size_t part_stride, const size_t o0, const size_t o1, const size_t o2, const size_t o3, const size_t o4,
    const size_t o5, const size_t o6, const size_t o7, int *__restrict__ flags, const FinOut fin, const unsigned *__restrict__ tile_list)
{
    constexpr int W = 64 / G; // positions per wave
    __shared__ RedShared sh;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform, and the compiler may know it
    const int group = lane / W;
    // tile_list (G == 1 only): the tiles this launch serves -- those the compact kernel left because they hold a position listed
    // more than once (dup_tiles_kernel); the grid is an upper bound of their number
    unsigned tile = blockIdx.x;
    if (tile_list) {
        if (blockIdx.x >= tile_list[0]) return;
        tile = tile_list[1 + blockIdx.x];
    }
    const long long p_raw = (long long)tile * W + (lane % W);
    const bool valid = p_raw < P;
    const long long p = valid ? p_raw : P - 1; // clamp: out-of-range lanes re-read the last position, never store
    const int chunk = (blockIdx.y * RED_WAVES + wave) * G + group;
    const int s0 = min(S, chunk * chunk_len);
    const int s1 = min(S, s0 + chunk_len);

    LaneAcc a;
    FastAcc f;
    if (FAST) fast_init(f);
    else lane_acc_init(a);

    unsigned e0 = 0, e1 = 0;
    if (E > 0) { e0 = dup_off[p]; e1 = dup_off[p + 1]; }
    const bool any_dup = E > 0 && __any(e1 > e0);

    // one sample row in registers + the next one in flight; every lane group walks its own chunk, the trip count
    // (chunk_len) is wave-uniform and rows past a group's chunk are loaded clamped and not visited
    constexpr int RB = rec_bytes(LAY);
    const size_t row_step = (size_t)rv.row_stride * RB; // bytes between the same position of consecutive samples
    const char *__restrict__ q = rv.base + ((size_t)min(s0, S - 1) * (size_t)rv.row_stride + (size_t)p) * RB;
    RawRec<LAY> nx = rec_load_at<LAY>(q);
    for (int i = 0; i < chunk_len; ++i) {
        const int s = s0 + i;
        int4 c0, c1;
        rec_decode<LAY>(nx, c0, c1);
        if (i + 1 < chunk_len) { // prefetch while this row is consumed
            if (s + 1 < S) q += row_step;
            nx = rec_load_at<LAY>(q);
        }
        if (s < s1) {
            // G == 1: s0 / s1 are wave-uniform, the whole wave is here -> the lean Germ_Max path.  Only the 16-byte
            // and 24-byte layouts are VALU-bound enough to profit; with 32-byte records the extra registers cost a wave of occupancy
            if (FAST) visit_fast<G == 1 && LAY != AMPLI_RECORDS_I32>(f, c0, c1, first_sample + s, C, cov);
            else visit_record(a, c0, c1, first_sample + s, C, cov, rv.rd ? rv.rd[(size_t)s * P + p] : AMPLI_ABSENT);
            if (any_dup) { // extras of this position in the same sample, in file order
                for (unsigned e = e0; e < e1; ++e) {
                    int4 x0, x1;
                    rec_decode<LAY>(rec_load_at<LAY>(rv.ext + ((size_t)s * (size_t)rv.ext_stride + e) * RB), x0, x1);
                    if (FAST) visit_fast<false>(f, x0, x1, first_sample + s, C, cov); // per-lane trip counts: no wave-level shortcuts
                    else visit_record(a, x0, x1, first_sample + s, C, cov, rv.rd_ext ? rv.rd_ext[(size_t)s * E + e] : AMPLI_ABSENT);
                }
                if (FAST && G == 1 && LAY != AMPLI_RECORDS_I32) { // the extras may have given lanes their first record
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) f.zmask[nt] = __builtin_amdgcn_ballot_w64(f.gn[nt] == 0);
                }
            }
        }
    }
    if (FAST) {
        if (f.bad || f.nrec > FAST_MAX_RECORDS) atomicOr(flags, AMPLI_FLAG_RERUN_GENERAL);
        fast_to_lane(f, a);
    }

    // ordered combine, stage 1: the G lane groups of this wave (group order = sample order), in registers
#pragma unroll
    for (int off = W; off < 64; off <<= 1) {
        LaneAcc b;
        lane_acc_shfl_down(a, b, off);
        if ((group % (2 * off / W)) == 0) lane_acc_merge(a, b);
    }
    // stage 2: the 4 waves through LDS, a tree over adjacent chunks (wave order = sample order):
    // waves 1,3 hand over to 0,2; then wave 2 hands over to wave 0
    if (wave & 1) lds_put(sh, wave >> 1, lane, a);
    __syncthreads();
    if (!(wave & 1)) {
        LaneAcc b;
        lds_get(sh, wave >> 1, lane, b);
        lane_acc_merge(a, b);
    }
    __syncthreads();
    if (wave == 2) lds_put(sh, 0, lane, a);
    __syncthreads();
    if (wave == 0) {
        LaneAcc b;
        lds_get(sh, 0, lane, b);
        lane_acc_merge(a, b);
        if (valid && group == 0) {
            if (fin.accumulate) { // earlier chunks of the cohort (+) this one; never with sample splits (host folds those)
                LaneAcc prior;
                lane_acc_load(acc_at(out_base, P, o0, o1, o2, o3, o4, o5, o6, o7), P, p_raw, prior);
                lane_acc_merge(prior, a);
                a = prior;
            }
            if (out_base) {
                const AccPtrs t = acc_at(out_base + (size_t)blockIdx.y * part_stride, P, o0, o1, o2, o3, o4, o5, o6, o7);
                if (fin.packed) { // multi-GPU shard: sums straight into the all-reduce buffer, table keeps the gm planes
                    lane_acc_store_packed(fin.packed, P, p_raw, a);
                    lane_acc_store_gm(t, P, p_raw, a);
                } else {
                    lane_acc_store(t, P, p_raw, a);
                }
            }
            // multi-GPU shard, sliced exchange: no table at all, or (last chunk of a streamed shard) the table's state (+) this chunk
            if (fin.slice_len) lane_acc_store_sliced(fin, p_raw, a);
            // fused epilogue (single split only): the merged state is in registers, finalize it here and spare the
            // table round trip through HBM plus a launch
            if (fin.rate) finalize_lane(a, P, p_raw, C, cov, fin);
        }
    }
}

// ---------------------------------------------------------------------------
// error_reduce for uint16 records with a COMPACT per-position state (round 4): the same one-wave-per-position loop as
// error_reduce_kernel<true, 1, AMPLI_RECORDS_U16>, in fewer registers, so that FIVE waves fit a SIMD instead of four.
// What the shipped kernel's 120 VGPRs are (code objects, round 4): the loop needs 110, the LaneAcc-by-LaneAcc merge of the
// epilogue the rest.  Here:
//   * strand-depth sums in 32 bits (a uint16 record's strand depth is < 2^18, a lane takes at most 8191 records);
//   * the four qualifying counts as two registers of 16-bit halves (a lane takes at most 8191 records);
//   * the first qualifying record of the Germ_Max state machine kept as its AF (one float, formed in the rare block where a
//     lane meets it) instead of the fraction x / RD (two registers); its sample index is not kept at all (bookkeeping of the
//     accumulator table, which this kernel does not write);
//   * nrec and the "depth beyond the fast envelope" bit share a register;
//   * the epilogue combines the four chunks field by field through LDS and finalises nucleotide by nucleotide.
// Only the headline's shape, like every specialisation here: fast arithmetic, one lane group, one sample split, no position
// listed twice, no accumulator table -- the table finalised in the epilogue (one GPU) or the shard's sums stored slice-major for
// the multi-GPU exchange; everything else takes error_reduce_kernel.  Same results, bit for bit.
// ---------------------------------------------------------------------------
struct Fast16 {
    int sx[2][4];
    unsigned sd[2][4]; // unsigned: 1023 records of 24-bit strand depths below 2^22 reach 2^32 - 2^22, beyond INT_MAX (a signed sum would be undefined there)
    double sp[2][4];
    unsigned cnt01, cnt23; // cnt[0] | cnt[1] << 16, cnt[2] | cnt[3] << 16
    float gfa[4];          // AF of the first qualifying record (EE:1229-1232); its value is dropped by the reference (EE:1258-1261)
    int gbx[4], gbd[4];    // best later record as a fraction (0/1 until one exists)
    unsigned nrec_bad;     // nrec | bad << 31
    unsigned long long zmask[4], lmask[4]; // wave masks (scalar registers): no first record yet | a later one met
};

// DEPTH_CHECK (24-bit records): a covered record with RD >= FAST_COUNT_LIMIT raises the lane's "beyond the fast envelope" bit (the 24-bit
// cross products and the 32-bit depth sums stop being exact there); a uint16 record's RD is below 2^19 by construction.
template <bool DEPTH_CHECK>
__device__ __forceinline__ void visit16(Fast16 &a, const int4 r0, const int4 r1, const float C, const int cov)
{
    const bool present = r0.x != AMPLI_ABSENT;
    const int fw[4] = {r0.x, r0.y, r0.z, r0.w};
    const int bw[4] = {r1.x, r1.y, r1.z, r1.w};
    const int FW = fw[0] + fw[1] + fw[2] + fw[3];  // EE:1175
    const int BW = bw[0] + bw[1] + bw[2] + bw[3];  // EE:1176
    const int RD = FW + BW;
    // EE:1595, EE:1251; an absent record has fw[0] = INT32_MIN, so its FW is negative and fails by itself (one compare feeds the
    // wave mask below directly; with "present &&" in front the mask takes a v_cndmask / v_cmp round trip per row)
    const unsigned long long covmask = __builtin_amdgcn_sicmp(min(FW, BW), cov, 39 /*sge*/);
    a.nrec_bad += present ? 1u : 0u;               // EE:1659
    if (covmask == 0) return;
    if (DEPTH_CHECK) a.nrec_bad |= (min(FW, BW) >= cov && (unsigned)RD >= (unsigned)FAST_COUNT_LIMIT) ? 0x80000000u : 0u;
    // RD < 2^19 for uint16 records: never beyond FAST_COUNT_LIMIT; the bit stays for the records-per-lane check
    // ampli_af_limit(d) as one float multiply (ampli_math.h): the same integer for every d < 2^24, and the floats are needed anyway
    const float fFW = (float)FW, fBW = (float)BW, fRD = (float)RD;
    const int lim_fw = ampli_af_limit_f32(fFW), lim_bw = ampli_af_limit_f32(fBW), lim_rd = ampli_af_limit_f32(fRD);
    const double prod_fw = (double)(fFW * C); // EE:1597
    const double prod_bw = (double)(fBW * C); // EE:1599
    // All wave masks of the row first, then ONE test for the rare first-record block, then the updates as straight-line code:
    // four separate "rare?" branches per row cut the row into pieces the scheduler cannot move work across, and a wave that has
    // its SIMD to itself (the partly filled last round of a launch) is bound by exactly that chain.
    int x[4];
    unsigned long long thrmask[4], candmask[4], anyfirst = 0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        x[nt] = fw[nt] + bw[nt];
        thrmask[nt] = __builtin_amdgcn_sicmp(fw[nt], lim_fw, 41 /*sle*/) & __builtin_amdgcn_sicmp(bw[nt], lim_bw, 41 /*sle*/) & covmask; // EE:1595
        // EE:1251: float(X)/float(RD) <= 0.05.  The Germ_Max state machine of EE:1229-1271 in wave masks: zmask = lanes that have not
        // met their first qualifying record, lmask = lanes that have met a later one (all a reader ever asks of the count)
        candmask[nt] = __builtin_amdgcn_uicmp((unsigned)x[nt], (unsigned)lim_rd, 37 /*ule*/) & covmask;
        anyfirst |= candmask[nt] & a.zmask[nt];
    }
    if (__builtin_expect(anyfirst != 0, 0)) { // rare: in steady state every passing lane already holds its first record
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const unsigned long long firstmask = candmask[nt] & a.zmask[nt];
            if (__builtin_amdgcn_inverse_ballot_w64(firstmask)) a.gfa[nt] = (float)x[nt] / fRD; // EE:1229-1232
            a.zmask[nt] &= ~firstmask;
            candmask[nt] &= ~firstmask;
        }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (__builtin_amdgcn_inverse_ballot_w64(thrmask[nt])) {
            a.sx[0][nt] += fw[nt]; a.sd[0][nt] += (unsigned)FW; a.sp[0][nt] += prod_fw; // EE:1597-1598
            a.sx[1][nt] += bw[nt]; a.sd[1][nt] += (unsigned)BW; a.sp[1][nt] += prod_bw; // EE:1599-1600
            if (nt < 2) a.cnt01 += nt == 0 ? 1u : 65536u;                     // EE:1606
            else a.cnt23 += nt == 2 ? 1u : 65536u;
        }
        a.lmask[nt] |= candmask[nt];
        // EE:1266 by cross-multiplication, ties keep the value
        const unsigned long long gtmask = __builtin_amdgcn_uicmpl(mul24x24_pair(x[nt], a.gbd[nt]), mul24x24_pair(a.gbx[nt], RD), 34 /*ugt*/);
        const bool better = __builtin_amdgcn_inverse_ballot_w64(candmask[nt] & gtmask);
        a.gbx[nt] = better ? x[nt] : a.gbx[nt];
        a.gbd[nt] = better ? RD : a.gbd[nt];
    }
}

// tiles (64 positions) that hold a position listed more than once: list[0] = their number, list[1..] = their indices, any order.
// dup_off is a prefix sum, so a tile holds extras iff dup_off differs at its two ends.
__global__ __launch_bounds__(256) void dup_tiles_kernel(const unsigned *__restrict__ dup_off, const long long P, unsigned *__restrict__ list)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long lo = t * 64, hi = lo + 64 < P ? lo + 64 : P;
    if (lo >= P) return;
    if (dup_off[hi] != dup_off[lo]) list[1 + atomicAdd(&list[0], 1u)] = (unsigned)t;
}

struct Red16Shared {
    double snt[2][8][64];
    long long srd[2][8][64];
    int ints[2][9][64];   // cnt[4] | nrec | gm_n[4]
    float flts[2][8][64]; // first_af[4] | rest[4]
};

// one chunk's summary, in the units the chunks are combined in
struct Part16 {
    double snt[2][4];
    long long srd[2][4];
    int cnt[4], nrec, gm_n[4];
    float gm_first_af[4], gm_rest[4];
};

__device__ __forceinline__ void part16_put(Red16Shared &sh, const int slot, const int lane, const Part16 &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        sh.snt[slot][nt][lane] = a.snt[0][nt]; sh.snt[slot][4 + nt][lane] = a.snt[1][nt];
        sh.srd[slot][nt][lane] = a.srd[0][nt]; sh.srd[slot][4 + nt][lane] = a.srd[1][nt];
        sh.ints[slot][nt][lane] = a.cnt[nt];
        sh.ints[slot][5 + nt][lane] = a.gm_n[nt];
        sh.flts[slot][nt][lane] = a.gm_first_af[nt];
        sh.flts[slot][4 + nt][lane] = a.gm_rest[nt];
    }
    sh.ints[slot][4][lane] = a.nrec;
}

// L = L (+) slot, L covering the earlier samples (lane_acc_merge, field by field out of LDS)
__device__ __forceinline__ void part16_merge(Part16 &L, const Red16Shared &sh, const int slot, const int lane)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        L.snt[0][nt] += sh.snt[slot][nt][lane]; L.snt[1][nt] += sh.snt[slot][4 + nt][lane];
        L.srd[0][nt] += sh.srd[slot][nt][lane]; L.srd[1][nt] += sh.srd[slot][4 + nt][lane];
        L.cnt[nt] += sh.ints[slot][nt][lane];
        const int rn = sh.ints[slot][5 + nt][lane];
        if (rn != 0) {
            const float rf = sh.flts[slot][nt][lane], rr = sh.flts[slot][4 + nt][lane];
            if (L.gm_n[nt] == 0) {
                L.gm_first_af[nt] = rf; L.gm_rest[nt] = rr;
            } else {
                float m = L.gm_rest[nt];
                if (m <= rf) m = rf;
                if (m <= rr) m = rr;
                L.gm_rest[nt] = m;
            }
            L.gm_n[nt] += rn;
        }
    }
    L.nrec += sh.ints[slot][4][lane];
}

// the state of the EARLIER samples out of the accumulator table (a streamed cohort: one launch per uploaded chunk, in visit order):
// a = table (+) a, lane_acc_merge with the table on the left, field by field out of HBM.  Returns a bit per nucleotide whose
// first qualifying record already lies in the table (its gm_first entry then stays what it is).
__device__ __forceinline__ unsigned part16_carry_in(Part16 &a, const AccPtrs &t, const long long P, const long long p)
{
    unsigned had = 0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        a.snt[0][nt] += t.snt[(0 * 4 + nt) * P + p]; a.snt[1][nt] += t.snt[(1 * 4 + nt) * P + p];
        a.srd[0][nt] += t.srd[(0 * 4 + nt) * P + p]; a.srd[1][nt] += t.srd[(1 * 4 + nt) * P + p];
        a.cnt[nt] += t.cnt[nt * P + p];
        const int ln = t.gm_n[nt * P + p];
        if (ln != 0) {
            const float lf = t.gm_first_af[nt * P + p], lr = t.gm_rest[nt * P + p];
            float m = lr;
            if (a.gm_n[nt] != 0) { // EE:1266 over the later records: the table's rest, this chunk's first, this chunk's rest
                if (m <= a.gm_first_af[nt]) m = a.gm_first_af[nt];
                if (m <= a.gm_rest[nt]) m = a.gm_rest[nt];
            }
            a.gm_rest[nt] = m;
            a.gm_first_af[nt] = lf;
            a.gm_n[nt] += ln;
            had |= 1u << nt;
        }
        // one nucleotide's loads at a time: hoisted together they need more registers than the row loop does (the kernel sits at
        // exactly 96 VGPRs = five waves per SIMD; the first build of this epilogue spilled 12 bytes per lane for them)
        asm volatile("" ::: "memory");
    }
    a.nrec += t.nrec[p];
    return had;
}

// The table as this kernel leaves it is a SUMMARY of the Germ_Max bookkeeping (AMPLI_REDUCE_SUMMARY): gm_n counts a chunk's
// qualifying records as none / one / two-or-more -- all any merge, the sliced store or finalize ever ask of it -- and the sample
// index of a first record met here reads -1 (unknown), as after a gathered merge.  Every other plane is exact.
__device__ __forceinline__ void part16_store(const AccPtrs &t, const long long P, const long long p, const Part16 &a, const unsigned had)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        t.snt[(0 * 4 + nt) * P + p] = a.snt[0][nt]; t.snt[(1 * 4 + nt) * P + p] = a.snt[1][nt];
        t.srd[(0 * 4 + nt) * P + p] = a.srd[0][nt]; t.srd[(1 * 4 + nt) * P + p] = a.srd[1][nt];
        t.cnt[nt * P + p] = a.cnt[nt];
        t.gm_n[nt * P + p] = a.gm_n[nt];
        t.gm_first_af[nt * P + p] = a.gm_first_af[nt];
        t.gm_rest[nt * P + p] = a.gm_rest[nt];
        if (!((had >> nt) & 1)) t.gm_first[nt * P + p] = a.gm_n[nt] ? -1 : 0x7fffffff;
    }
    t.nrec[p] = a.nrec;
}

// positions [p_lo, p_hi) of a panel of P (P = the stride of every per-position plane); tile b = positions p_lo + 64 b ...
// DUP: the cohort lists positions more than once (E > 0, overlapping amplicons: every line is a record, EE:1555 equal_range over
// all lines of a key, and EE:1251-1271 is order-dependent: primary record, then the extras in file order, sample after sample).
// A tile that holds such a position is not this kernel's: its workgroup leaves at once and error_reduce_kernel takes the tile
// from dup_tiles_kernel's list (same epilogue forms, same outputs).  Measured alternative, round 5: the sample-by-sample walk of
// such tiles inside this kernel -- correct, but the second loop costs the first one two registers it does not have (spill
// stores inside the row loop of EVERY tile of the cohort).
// TAB: the launch reads and / or writes the accumulator table (a streamed cohort's chunks); without it the epilogue is the headline's.
// LAY: AMPLI_RECORDS_U16, or (round 5) AMPLI_RECORDS_U24 -- the same state fits 24-bit records as long as a covered record's RD stays
// below FAST_COUNT_LIMIT = 2^22 (checked per record) and a lane takes at most COMPACT_MAX_REC_U24 = 1023 records: a strand depth sum
// is then < 2^22 x 1023 < 2^32 (kept and widened as unsigned), a sum of X < 0.05 x 2^22 x 1023 < 2^28, a count < 2^16.
constexpr int COMPACT_MAX_REC_U24 = 1023;
template <int LAY, bool DUP, bool TAB>
__device__ __forceinline__ void compact_reduce_body(Red16Shared &sh, const RecView &rv, const long long P, const long long p_lo, const long long p_hi,
                                                    const unsigned *__restrict__ dup_off, const int S, const int chunk_len,
                                                    const float C, const int cov, int *__restrict__ flags, const AccPtrs &tab,
                                                    const FinOut &fin)
{
    constexpr int RB = rec_bytes(LAY);
    constexpr bool DC = LAY != AMPLI_RECORDS_U16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p_raw = p_lo + (long long)blockIdx.x * 64 + lane;
    const bool valid = p_raw < p_hi;
    const long long p = valid ? p_raw : p_hi - 1; // clamp: out-of-range lanes re-read the last position, never store
    const int s0 = min(S, wave * chunk_len);
    const int s1 = min(S, s0 + chunk_len);
    Fast16 f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        f.sx[0][nt] = f.sx[1][nt] = 0; f.sd[0][nt] = f.sd[1][nt] = 0u; f.sp[0][nt] = f.sp[1][nt] = 0.0;
        f.gfa[nt] = 0.0f; f.gbx[nt] = 0; f.gbd[nt] = 1; f.zmask[nt] = ~0ull; f.lmask[nt] = 0ull;
    }
    f.cnt01 = f.cnt23 = 0u;
    f.nrec_bad = 0u;
    const size_t row_step = (size_t)rv.row_stride * RB;
    const char *__restrict__ q = rv.base + ((size_t)min(s0, S - 1) * (size_t)rv.row_stride + (size_t)p) * RB;
    if (DUP) { // a tile with a position listed more than once is left to error_reduce_kernel (launched over the list of such tiles)
        if (__any(dup_off[p + 1] != dup_off[p])) return; // the four waves of a workgroup see the same tile: all leave, before any barrier
    }
    // Three named register sets in rotation: rows s + 1 and s + 2 are in flight while row s is consumed (s_waitcnt vmcnt(2)).
    // (Written as one row per trip with a "next" record, hipcc copies the freshly loaded record into the loop-carried registers
    // at the latch and waits for it there -- s_waitcnt vmcnt(0) right behind the load -- so the prefetch is none; that form ran
    // at 166 us on config 3 against the general kernel's 124; two sets, one row in flight: 107; three: 102.)  Past the end of
    // the chunk the loads stay on its last row (cache hits) and the rows are not visited.
    RawRec<LAY> ra = rec_load_at<LAY>(q), rb, rc;
    if (s0 + 1 < s1) q += row_step;
    rb = rec_load_at<LAY>(q);
    for (int s = s0; s < s1; s += 3) {
        if (s + 2 < s1) q += row_step;
        rc = rec_load_at<LAY>(q);
        {
            int4 c0, c1;
            rec_decode<LAY>(ra, c0, c1);
            if (s < s1) visit16<DC>(f, c0, c1, C, cov);
        }
        if (s + 3 < s1) q += row_step;
        ra = rec_load_at<LAY>(q);
        {
            int4 c0, c1;
            rec_decode<LAY>(rb, c0, c1);
            if (s + 1 < s1) visit16<DC>(f, c0, c1, C, cov);
        }
        if (s + 4 < s1) q += row_step;
        rb = rec_load_at<LAY>(q);
        {
            int4 c0, c1;
            rec_decode<LAY>(rc, c0, c1);
            if (s + 2 < s1) visit16<DC>(f, c0, c1, C, cov);
        }
    }
    if ((f.nrec_bad & 0x7FFFFFFFu) > (unsigned)(DC ? COMPACT_MAX_REC_U24 : FAST_MAX_RECORDS) || (DC && (f.nrec_bad >> 31))) atomicOr(flags, AMPLI_FLAG_RERUN_GENERAL);
    Part16 a;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            a.snt[st][nt] = (double)f.sx[st][nt] + f.sp[st][nt];
            a.srd[st][nt] = (long long)f.sd[st][nt];
        }
        // qualifying records of the chunk, saturated at two: every reader asks "none, one, or more" (lane_acc_merge's sums keep that)
        const bool none = (f.zmask[nt] >> lane) & 1, later = (f.lmask[nt] >> lane) & 1;
        a.gm_n[nt] = none ? 0 : later ? 2 : 1;
        a.gm_first_af[nt] = f.gfa[nt];
        a.gm_rest[nt] = later ? (float)f.gbx[nt] / (float)f.gbd[nt] : -INFINITY;
    }
    a.cnt[0] = (int)(f.cnt01 & 0xFFFFu); a.cnt[1] = (int)(f.cnt01 >> 16);
    a.cnt[2] = (int)(f.cnt23 & 0xFFFFu); a.cnt[3] = (int)(f.cnt23 >> 16);
    a.nrec = (int)(f.nrec_bad & 0x7FFFFFFFu);
    // the four chunks in sample order, a tree over adjacent chunks: waves 1, 3 hand over to 0, 2; then 2 to 0
    if (wave & 1) part16_put(sh, wave >> 1, lane, a);
    __syncthreads();
    if (!(wave & 1)) part16_merge(a, sh, wave >> 1, lane);
    __syncthreads();
    if (wave == 2) part16_put(sh, 0, lane, a);
    __syncthreads();
    if (wave == 0) {
        part16_merge(a, sh, 0, lane);
        if (valid) {
            unsigned had = 0;
            if (TAB && fin.accumulate) had = part16_carry_in(a, tab, P, p_raw); // earlier chunks of the cohort (+) this one
            if (TAB && tab.snt) part16_store(tab, P, p_raw, a, had);
            if (fin.slice_len) lane_acc_store_sliced(fin, p_raw, a); // multi-GPU shard, sliced exchange: straight into the exchange buffers
            if (fin.rate) {
                const double limit = envelope_limit(C, cov);
                bool bad = false;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    bad |= finalize_one(nt, a.snt[0][nt], a.snt[1][nt], a.srd[0][nt], a.srd[1][nt], a.cnt[nt], a.nrec, a.gm_n[nt], a.gm_rest[nt], P, p_raw, limit, fin);
                if (bad && fin.flags) atomicOr(fin.flags, 1);
            }
        }
    }
}

template <bool DUP, bool TAB>
__global__ __launch_bounds__(256, 5) void error_reduce_u16_kernel(const RecView rv, const long long P, const long long p_lo, const long long p_hi,
                                                                  const unsigned *__restrict__ dup_off, const int S, const int chunk_len,
                                                                  const float C, const int cov, int *__restrict__ flags, const AccPtrs tab,
                                                                  const FinOut fin)
{
    __shared__ Red16Shared sh;
    compact_reduce_body<AMPLI_RECORDS_U16, DUP, TAB>(sh, rv, P, p_lo, p_hi, dup_off, S, chunk_len, C, cov, flags, tab, fin);
}

template <bool DUP, bool TAB>
__global__ __launch_bounds__(256, 5) void error_reduce_u24_kernel(const RecView rv, const long long P, const long long p_lo, const long long p_hi,
                                                                  const unsigned *__restrict__ dup_off, const int S, const int chunk_len,
                                                                  const float C, const int cov, int *__restrict__ flags, const AccPtrs tab,
                                                                  const FinOut fin)
{
    __shared__ Red16Shared sh;
    compact_reduce_body<AMPLI_RECORDS_U24, DUP, TAB>(sh, rv, P, p_lo, p_hi, dup_off, S, chunk_len, C, cov, flags, tab, fin);
}

int ensure_ws(ampli_ctx *ctx, size_t bytes)
{
    if (ctx->ws_bytes >= bytes) return AMPLI_OK;
    if (is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "workspace would have to grow while capturing: run the sequence once first");
    if (ctx->ws) { HIP_TRY(ctx, hipStreamSynchronize(main_stream(ctx))); (void)hipFree(ctx->ws); ctx->ws = nullptr; ctx->ws_bytes = 0; }
    if (hipMalloc(&ctx->ws, bytes) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "workspace hipMalloc failed");
    ctx->ws_bytes = bytes;
    return AMPLI_OK;
}

AccPtrs to_ptrs(const ampli_acc_table *t)
{
    AccPtrs a;
    a.snt = t->snt; a.srd = (long long *)t->srd; a.cnt = t->cnt; a.nrec = t->nrec; a.gm_n = t->gm_n;
    a.gm_first = t->gm_first; a.gm_first_af = t->gm_first_af; a.gm_rest = t->gm_rest;
    return a;
}

// the planes of a table carved from `base` at the offsets of acc_offsets (a partial or merged table of the workspace)
static AccPtrs acc_ptrs(char *base, const size_t off[9])
{
    AccPtrs a;
    a.snt = (double *)(base + off[0]); a.srd = (long long *)(base + off[1]); a.cnt = (int *)(base + off[2]);
    a.nrec = (int *)(base + off[3]); a.gm_n = (int *)(base + off[4]); a.gm_first = (int *)(base + off[5]);
    a.gm_first_af = (float *)(base + off[6]); a.gm_rest = (float *)(base + off[7]);
    return a;
}

// the error table a finalize writes (rate and code required; thr, germ_val, germ_present and flags optional)
FinOut table_out(float *rate, uint8_t *code, float *thr, float *germ_val, uint8_t *germ_present, int32_t *flags)
{
    FinOut o = {};
    o.rate = rate; o.code = code; o.thr = thr; o.germ_val = germ_val; o.germ_present = germ_present; o.flags = flags;
    return o;
}

// the slice-major exchange buffers of a position-sliced merge: [n_slices][group][planes][L] sums and [n_slices][group][8][L]
// germ-max pairs, of which this call fills batch grp_index (ampli_set_slice_group) in the context's format (ampli_set_slice_format)
FinOut slice_out(const ampli_ctx *ctx, const long long P, const int n_slices, double *d_sums, float *d_gm)
{
    FinOut o = {};
    o.slice_len = ampli_slice_len(P, n_slices);
    o.sl_group = ctx->grp_size;
    o.sl_fmt = ctx->slice_fmt; o.sl_n = n_slices; o.sl_flags = ctx->d_flags;
    o.sl_sums = d_sums + (size_t)ctx->grp_index * slice_planes(o.sl_fmt) * (size_t)o.slice_len;
    o.sl_gm = d_gm + (size_t)ctx->grp_index * 8 * (size_t)o.slice_len;
    return o;
}

// a bound table must be one buffer carved by ampli_acc_bind
bool acc_is_bound(const ampli_acc_table *t)
{
    if (!t || !t->snt || t->P <= 0) return false;
    size_t off[9];
    acc_offsets(t->P, off);
    const AccPtrs carved = acc_ptrs((char *)t->snt, off), given = to_ptrs(t);
    return memcmp(&carved, &given, sizeof(AccPtrs)) == 0;
}

// after a cut along the samples error_reduce_impl folds the partial tables and, for a multi-GPU shard, fills the exchange buffers
// from the merged table (acc_pack_kernel: ampli_exchange.hip, through launch_acc_pack)

// dst = parts[0] (+) parts[1] (+) ... in order; parts are tables at base + i*stride
__global__ __launch_bounds__(256) void acc_merge_kernel(char *dst_base, const char *parts_base, const size_t part_stride,
                                                        const int nparts, const long long P, const size_t o0,
                                                        const size_t o1, const size_t o2, const size_t o3,
                                                        const size_t o4, const size_t o5, const size_t o6,
                                                        const size_t o7, const char *prior_base)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
    // prior_base: a table holding the state of earlier samples (streamed cohorts); the parts follow it in order
    lane_acc_load(acc_at(const_cast<char *>(prior_base ? prior_base : parts_base), P, o0, o1, o2, o3, o4, o5, o6, o7), P, p, a);
    for (int i = prior_base ? 0 : 1; i < nparts; ++i) {
        LaneAcc b;
        lane_acc_load(acc_at(const_cast<char *>(parts_base) + (size_t)i * part_stride, P, o0, o1, o2, o3, o4, o5, o6, o7), P, p, b);
        lane_acc_merge(a, b);
    }
    lane_acc_store(acc_at(dst_base, P, o0, o1, o2, o3, o4, o5, o6, o7), P, p, a);
}

// table -> slice-major exchange buffers (only when the sample axis had to be split across workgroups)
__global__ __launch_bounds__(256) void acc_pack_sliced_kernel(AccPtrs t, const long long P, const FinOut o)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
    lane_acc_load(t, P, p, a);
    lane_acc_store_sliced(o, p, a);
}

int launch_acc_pack_sliced(ampli_ctx *ctx, const AccPtrs &t, long long P, const FinOut &fo)
{
    hipLaunchKernelGGL(acc_pack_sliced_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), t, P, fo);
    return check_launch(ctx, "acc_pack_sliced_kernel");
}

static int launch_finalize(ampli_ctx *ctx, const AccPtrs &t, long long P, float C, int cov, const FinOut &fo);

// reduce (+ optional fused finalize).  d_acc may be NULL when fin.rate is set (the table is then not materialised
// unless the sample axis has to be split across workgroups).
static int error_reduce_impl(ampli_ctx *ctx, const DevCohort &co, int64_t P, int32_t first_sample, float C, int32_t cov,
                             const ampli_acc_table *d_acc, const FinOut &fin)
{
    if (!ctx) return AMPLI_E_INVALID;
    const int64_t E = co.E;
    const int32_t S = co.n;
    const uint32_t *d_dup_off = co.dup_off;
    if (!co.rv.base || P <= 0 || E < 0 || S <= 0 || cov < 1 || (d_acc && (!acc_is_bound(d_acc) || d_acc->P != P)) || (!d_acc && !fin.rate && !fin.slice_len) || (fin.packed && !d_acc))
        return fail(ctx, AMPLI_E_INVALID, "error_reduce: bad argument (P,S>0, cov>=1, table bound with ampli_acc_bind for the same P)");
    if (fin.accumulate && !d_acc) return fail(ctx, AMPLI_E_INVALID, "error_reduce: accumulate needs the table");
    { int rc = check_records(ctx, co, "error_reduce", d_dup_off, "dup_off"); if (rc) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // lane groups per wave: only for panels too small to fill the chip with 64-position waves (measured on c3:
    // G = 2 / 4 cost 6 % / 11 % -- the narrower per-row segments outweigh the shorter tail)
    const long long resident_waves = (long long)ctx->n_cu * 16;
    const bool fast = !ctx->reduce_general && !co.rv.rd && !co.rv.rd_ext; // lines with their own RD column: the literal kernel
    // the shape error_reduce_u16_kernel takes (below).  From one tile per CU on it beats every cut of the general kernel along
    // lanes or samples (tools/sweep_tiles.py: 48 us against 62 at 768 tiles, 69 against 102 at 1280), so such a launch is not cut
    const bool compact_shape = ctx->reduce_compact && fast && (!d_acc || fin.summary) && !fin.packed &&
                               ((co.layout == AMPLI_RECORDS_U16 && S <= RED_WAVES * FAST_MAX_CHUNK) ||
                                (co.layout == AMPLI_RECORDS_U24 && S <= RED_WAVES * COMPACT_MAX_REC_U24 && !ctx->reduce_compact_u16_only));
    const bool compact_uncut = compact_shape && (P + 63) / 64 >= ctx->n_cu;
    int G = ctx->reduce_groups;
    if (G != 1 && G != 2 && G != 4) {
        G = 1;
        while (!compact_uncut && G < 4 && ((P + 64 / G - 1) / (64 / G)) * RED_WAVES < resident_waves && S / (RED_WAVES * 2 * G) >= 8) G *= 2;
    }
    const long long tiles = (P + 64 / G - 1) / (64 / G);
    // sample splits: enough waves to fill the chip (>= ~24 waves per CU), each lane group with >= 8 samples
    int splits = ctx->reduce_splits;
    if (splits <= 0 && compact_uncut && G == 1) {
        splits = 1;
    } else if (splits <= 0) {
        const long long want_waves = (long long)ctx->n_cu * 24;
        splits = (int)((want_waves + tiles * RED_WAVES - 1) / (tiles * RED_WAVES));
        const int max_splits = (S + RED_WAVES * G * 8 - 1) / (RED_WAVES * G * 8);
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
    }
    if (splits > S) splits = S;
    if (fast) { // int32 partial sums: a lane takes at most FAST_MAX_CHUNK samples
        const int need = (S + RED_WAVES * G * FAST_MAX_CHUNK - 1) / (RED_WAVES * G * FAST_MAX_CHUNK);
        if (splits < need) splits = need;
    }
    const int chunks = splits * RED_WAVES * G;
    const int chunk_len = (S + chunks - 1) / chunks;

    size_t off[9];
    acc_offsets(P, off);
    char *out_base = d_acc ? (char *)d_acc->snt : nullptr;
    size_t stride = 0;
    FinOut kfin = fin; // what the reduce kernel itself finalises
    if (splits > 1) {
        // partial tables, one per split, plus one slot for the merged table when the caller did not ask for it
        int rc = ensure_ws(ctx, off[8] * (size_t)(splits + 1));
        if (rc) return rc;
        out_base = (char *)ctx->ws;
        stride = off[8];
        kfin.rate = nullptr;
        kfin.packed = nullptr; // packed after the merge, below
        kfin.slice_len = 0;
        kfin.accumulate = 0;   // folded in by the merge kernel, below
    }
    if (splits > 65535 || tiles > 0x7fffffffll) return fail(ctx, AMPLI_E_RANGE, "error_reduce: panel or sample count beyond the grid limits");
    ctx->last_reduce_kernel = (compact_shape && G == 1 && splits == 1) ? (co.layout == AMPLI_RECORDS_U24 ? 2 : 1) : 0;
    if (ctx->last_reduce_kernel) {
        const AccPtrs tab = d_acc ? to_ptrs(d_acc) : AccPtrs{};
        const int clen = (S + RED_WAVES - 1) / RED_WAVES;
        const bool u24 = co.layout == AMPLI_RECORDS_U24; // the compact shape exists for the two packed layouts only
        // the compact kernel over positions [lo, hi) on st: DUP skips the tiles dup_tiles_kernel listed, TAB writes the table
        auto launch_compact = [&](const bool dup, hipStream_t st, const long long lo, const long long hi) {
            with_bool(dup, [&](auto DUP) {
                with_bool(d_acc != nullptr, [&](auto TAB) {
                    const auto kernel = u24 ? error_reduce_u24_kernel<DUP, TAB> : error_reduce_u16_kernel<DUP, TAB>;
                    hipLaunchKernelGGL(kernel, dim3((unsigned)((hi - lo + 63) / 64)), dim3(256), 0, st, co.rv, (long long)P, lo, hi, d_dup_off,
                                       (int)S, clen, C, (int)cov, ctx->d_flags, tab, fin);
                });
            });
        };
        if (E > 0) {
            // the tiles with a position listed more than once go to the general kernel (at most one such tile per extra slot)
            hipStream_t st = main_stream(ctx);
            const long long ntiles = (P + 63) / 64;
            { int rc = ensure_ws(ctx, (size_t)(ntiles + 1) * sizeof(unsigned)); if (rc) return rc; }
            unsigned *list = (unsigned *)ctx->ws;
            HIP_TRY(ctx, hipMemsetAsync(list, 0, sizeof(unsigned), st));
            hipLaunchKernelGGL(dup_tiles_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, st, d_dup_off, (long long)P, list);
            launch_compact(true, st, 0, P);
            { int rc = check_launch(ctx, "error_reduce_u16_kernel"); if (rc) return rc; }
            const auto dup_kernel = u24 ? error_reduce_kernel<true, 1, AMPLI_RECORDS_U24> : error_reduce_kernel<true, 1, AMPLI_RECORDS_U16>;
            hipLaunchKernelGGL(dup_kernel, dim3((unsigned)std::min<long long>(E, ntiles)), dim3(256), 0, st, co.rv, (long long)P, (long long)E,
                               d_dup_off, (int)S, (int)first_sample, clen, C, (int)cov, d_acc ? (char *)d_acc->snt : (char *)nullptr, (size_t)0,
                               off[0], off[1], off[2], off[3], off[4], off[5], off[6], off[7], ctx->d_flags, fin, (const unsigned *)list);
            return check_launch(ctx, "error_reduce_kernel (tiles with positions listed more than once)");
        }
        if (ranges_apply(ctx, P)) { // position ranges on concurrent streams (ampli_set_ranges)
            { int rc = ranges_fork(ctx, P); if (rc) return rc; }
            long long cut[AMPLI_MAX_RANGES + 1];
            range_cuts(P, ctx->n_ranges, cut);
            for (int k = 0; k < ctx->n_ranges; ++k) launch_compact(false, lane_stream(ctx, k), cut[k], cut[k + 1]);
            return check_launch(ctx, "error_reduce_u16_kernel");
        }
        launch_compact(false, main_stream(ctx), 0, P);
        return check_launch(ctx, "error_reduce_u16_kernel");
    }
    const dim3 grid((unsigned)tiles, (unsigned)splits);
    auto launch_general = [&](auto FAST, auto GV) {
        with_layout(co.layout, [&](auto L) {
            hipLaunchKernelGGL((error_reduce_kernel<FAST, GV, L>), grid, dim3(256), 0, main_stream(ctx), co.rv, (long long)P, (long long)E,
                               d_dup_off, (int)S, (int)first_sample, chunk_len, C, (int)cov, out_base, stride, off[0], off[1], off[2], off[3],
                               off[4], off[5], off[6], off[7], ctx->d_flags, kfin, (const unsigned *)nullptr);
        });
    };
    with_bool(fast, [&](auto FAST) {
        if (G == 4) launch_general(FAST, Const<4>{});
        else if (G == 2) launch_general(FAST, Const<2>{});
        else launch_general(FAST, Const<1>{});
    });
    int rc = check_launch(ctx, "error_reduce_kernel");
    if (rc) return rc;
    if (splits > 1) {
        char *merged = d_acc ? (char *)d_acc->snt : (char *)ctx->ws + off[8] * (size_t)splits;
        const AccPtrs t = acc_ptrs(merged, off);
        hipLaunchKernelGGL(acc_merge_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), merged,
                           (const char *)ctx->ws, stride, splits, (long long)P, off[0], off[1], off[2], off[3], off[4], off[5],
                           off[6], off[7], fin.accumulate ? (const char *)d_acc->snt : (const char *)nullptr);
        rc = check_launch(ctx, "acc_merge_kernel");
        if (rc) return rc;
        if (fin.packed) {
            rc = launch_acc_pack(ctx, t, P, fin.packed);
            if (rc) return rc;
        }
        if (fin.slice_len) {
            rc = launch_acc_pack_sliced(ctx, t, P, fin);
            if (rc) return rc;
        }
        if (fin.rate) rc = launch_finalize(ctx, t, P, C, cov, fin);
    }
    return rc;
}

extern "C" int ampli_error_reduce(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                                  int32_t S, int32_t first_sample, float C, int32_t cov, const ampli_acc_table *d_acc)
{
    if (!d_acc) return ctx ? fail(ctx, AMPLI_E_INVALID, "error_reduce: d_acc is required") : AMPLI_E_INVALID;
    if (!ctx) return AMPLI_E_INVALID;
    return error_reduce_impl(ctx, dense_cohort(ctx, d_recs, P, E, S, d_dup_off, nullptr), P, first_sample, C, cov, d_acc, FinOut{});
}

extern "C" int ampli_error_estimate(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                                    int32_t S, float C, int32_t cov, const ampli_acc_table *d_acc, float *d_rate,
                                    uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present,
                                    int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_rate || !d_code) return fail(ctx, AMPLI_E_INVALID, "error_estimate: rate and code outputs are required");
    return error_reduce_impl(ctx, dense_cohort(ctx, d_recs, P, E, S, d_dup_off, nullptr), P, 0, C, cov, d_acc,
                             table_out(d_rate, d_code, d_thr, d_germ_val, d_germ_present, d_flags));
}

extern "C" int ampli_error_reduce_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t first_sample, float C, int32_t cov,
                                          const ampli_acc_table *d_acc, int32_t accumulate, float *d_rate, uint8_t *d_code, float *d_thr,
                                          float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if ((d_rate != nullptr) != (d_code != nullptr)) return fail(ctx, AMPLI_E_INVALID, "error_reduce_records: rate and code come together");
    FinOut fo = table_out(d_rate, d_code, d_thr, d_germ_val, d_germ_present, d_flags);
    fo.accumulate = (accumulate & AMPLI_REDUCE_ACCUMULATE) ? 1 : 0;
    fo.summary = (accumulate & AMPLI_REDUCE_SUMMARY) ? 1 : 0;
    return error_reduce_impl(ctx, co, P, first_sample, C, cov, d_acc, fo);
}

// the LAST chunk of a shard's streamed cohort: table (+) chunk straight into the slice-major exchange buffers (no table -> slices pass;
// a shard whose cohort is one chunk needs no table at all)
extern "C" int ampli_error_reduce_records_sliced(ampli_ctx *ctx, const ampli_records *recs, int64_t P, int32_t first_sample, float C, int32_t cov,
                                                 const ampli_acc_table *d_acc, int32_t accumulate, int32_t n_slices, double *d_sums, float *d_gm)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_sums || !d_gm || n_slices < 1) return fail(ctx, AMPLI_E_INVALID, "error_reduce_records_sliced: exchange buffers and n_slices >= 1 are required");
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    FinOut fo = slice_out(ctx, P, n_slices, d_sums, d_gm);
    fo.accumulate = (accumulate & AMPLI_REDUCE_ACCUMULATE) ? 1 : 0;
    fo.summary = (accumulate & AMPLI_REDUCE_SUMMARY) ? 1 : 0;
    return error_reduce_impl(ctx, co, P, first_sample, C, cov, d_acc, fo);
}

extern "C" int ampli_error_reduce_packed(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                                         int32_t S, int32_t first_sample, float C, int32_t cov, const ampli_acc_table *d_acc,
                                         double *d_packed)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_acc || !d_packed) return fail(ctx, AMPLI_E_INVALID, "error_reduce_packed: table and packed buffer are required");
    FinOut fo = {};
    fo.packed = d_packed;
    return error_reduce_impl(ctx, dense_cohort(ctx, d_recs, P, E, S, d_dup_off, nullptr), P, first_sample, C, cov, d_acc, fo);
}

extern "C" int ampli_error_reduce_sliced(ampli_ctx *ctx, const int32_t *d_recs, int64_t P, int64_t E, const uint32_t *d_dup_off,
                                         int32_t S, int32_t first_sample, float C, int32_t cov, int32_t n_slices,
                                         double *d_sums, float *d_gm)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_sums || !d_gm || n_slices < 1) return fail(ctx, AMPLI_E_INVALID, "error_reduce_sliced: exchange buffers and n_slices >= 1 are required");
    return error_reduce_impl(ctx, dense_cohort(ctx, d_recs, P, E, S, d_dup_off, nullptr), P, first_sample, C, cov, nullptr,
                             slice_out(ctx, P, n_slices, d_sums, d_gm));
}

// ---------------------------------------------------------------------------
// The threshold sums in the REFERENCE's own order (round 6), for cohorts outside the exactness envelope of DESIGN 4.2.
// Inside it every partial sum of `sum = sum + X + float(RD)*float(C)` (EE:1597, 1599) is exact, so any order and association --
// ours: sample shards, waves, chunks -- gives the reference's double.  Outside it (a coverage cut-off of a few reads with depths
// in the millions) the double depends on the order the reference adds in: estimateThresholds walks `equal_range` of an
// unordered_multimap (EE:1555, 1565), which libstdc++ fills so that equal keys come out in REVERSE insertion order -- the last
// file of the visit order first, and within a file a position's later lines before its first one.  One lane per position walks
// exactly that: samples of the chunk from last to first, extras from last to first, then the primary record; the double is
// updated as the reference's expression associates, (sum + X) + (double)(float(RD) * float(C)).  A cohort in several chunks is
// walked chunk by chunk from the LAST chunk to the first with the sums carried in the table (accumulate).  Only the eight sums
// are produced: counts, depth sums (integers in a double: exact to 2^53) and the Germ_Max state do not depend on this order.
// Speed is irrelevant (a rerun of a cohort the fast path flagged); positions are independent, so it is still one launch.
// ---------------------------------------------------------------------------
template <int LAY>
__global__ __launch_bounds__(256) void error_sums_inorder_kernel(const RecView rv, const long long P, const long long E, const int n,
                                                                 const unsigned *__restrict__ dup_off, const float C, const int cov,
                                                                 double *__restrict__ snt, const int accumulate)
{
    constexpr int RB = rec_bytes(LAY);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
    lane_acc_init(a);
    if (accumulate) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            a.snt[0][nt] = snt[(0 * 4 + nt) * P + p];
            a.snt[1][nt] = snt[(1 * 4 + nt) * P + p];
        }
    }
    const unsigned e0 = dup_off ? dup_off[p] : 0u, e1 = dup_off ? dup_off[p + 1] : 0u;
    for (int t = n - 1; t >= 0; --t) {
        for (unsigned e = e1; e > e0; --e) { // the position's later lines of this file first
            int4 r0, r1;
            rec_decode<LAY>(rec_load_at<LAY>(rv.ext + ((size_t)t * (size_t)rv.ext_stride + (size_t)(e - 1)) * RB), r0, r1);
            visit_record(a, r0, r1, t, C, cov, rv.rd_ext ? rv.rd_ext[(size_t)t * (size_t)E + (e - 1)] : AMPLI_ABSENT);
        }
        int4 r0, r1;
        rec_decode<LAY>(rec_load_at<LAY>(rv.base + ((size_t)t * (size_t)rv.row_stride + (size_t)p) * RB), r0, r1);
        visit_record(a, r0, r1, t, C, cov, rv.rd ? rv.rd[(size_t)t * (size_t)P + p] : AMPLI_ABSENT);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        snt[(0 * 4 + nt) * P + p] = a.snt[0][nt];
        snt[(1 * 4 + nt) * P + p] = a.snt[1][nt];
    }
}

extern "C" int ampli_error_sums_inorder(ampli_ctx *ctx, const ampli_records *recs, int64_t P, float C, int32_t cov,
                                        const ampli_acc_table *d_acc, int32_t accumulate)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!recs || P <= 0 || cov < 1 || !d_acc || !acc_is_bound(d_acc) || d_acc->P != P) return fail(ctx, AMPLI_E_INVALID, "error_sums_inorder: bad argument");
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (co.n <= 0 || !co.rv.base) return fail(ctx, AMPLI_E_INVALID, "error_sums_inorder: empty cohort");
    { int rc = check_records(ctx, co, "error_sums_inorder", co.dup_off, "dup_off"); if (rc) return rc; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    with_layout(co.layout, [&](auto L) {
        hipLaunchKernelGGL((error_sums_inorder_kernel<L>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), co.rv, (long long)P,
                           (long long)co.E, (int)co.n, co.E > 0 ? co.dup_off : nullptr, C, (int)cov, d_acc->snt, accumulate ? 1 : 0);
    });
    return check_launch(ctx, "error_sums_inorder_kernel");
}

// ==== finalize: accumulator table -> error table =======================================================================================

__global__ __launch_bounds__(256) void error_finalize_kernel(AccPtrs t, const long long P, const float C, const int cov, FinOut o)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
    lane_acc_load(t, P, p, a);
    finalize_lane(a, P, p, C, cov, o);
}

static int launch_finalize(ampli_ctx *ctx, const AccPtrs &t, long long P, float C, int cov, const FinOut &fo)
{
    hipLaunchKernelGGL(error_finalize_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), t, P, C, cov, fo);
    return check_launch(ctx, "error_finalize_kernel");
}

extern "C" int ampli_error_finalize(ampli_ctx *ctx, const ampli_acc_table *d_acc, float C, int32_t cov, float *d_rate,
                                    uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present,
                                    int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_acc || d_acc->P <= 0 || !d_rate || !d_code || cov < 1) return fail(ctx, AMPLI_E_INVALID, "error_finalize: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_finalize(ctx, to_ptrs(d_acc), d_acc->P, C, (int)cov, table_out(d_rate, d_code, d_thr, d_germ_val, d_germ_present, d_flags));
}

// ==== Poisson: tumour records + thresholds -> calls ====================================================================================

// ---------------------------------------------------------------------------
// poisson_call: one lane per record, SAMPLES_PER_BLOCK tumour samples per
// workgroup so the position's 8 thresholds + reference code are loaded once
// and reused from registers.
// ---------------------------------------------------------------------------

// Compact call list, sharded: a returning atomic on ONE word serialises at ~11 ns per add (about 90 per us chip-wide,
// MI355X_MICROARCH.md "dequeue"), which at a few thousand calls per launch would bound the whole kernel.  The list is
// therefore AMPLI_CALL_SHARDS independent segments, each with its own counter on its own 128-byte line; a workgroup
// appends to the shard blockIdx.x % AMPLI_CALL_SHARDS.  Segment k holds entries [k*cap_per_shard, ...).
__device__ __forceinline__ long long call_slot(unsigned long long *__restrict__ n_calls, const long long capacity)
{
    const unsigned shard = blockIdx.x % AMPLI_CALL_SHARDS;
    const long long per = capacity / AMPLI_CALL_SHARDS;
    const unsigned long long i = atomicAdd(&n_calls[shard * AMPLI_CALL_COUNTER_STRIDE], 1ull);
    return ((long long)i < per) ? (long long)shard * per + (long long)i : -1;
}

constexpr int PC_SAMPLES = 4;

// threshold plane j (= strand*4 + nucleotide) of position p: plane-major [8][P] (slice_len == 0), or straight from the
// all-gathered blocks of a position-sliced merge (block k = positions [k*slice_len, ...): rate 32L | thr 32L | ...)
__device__ __forceinline__ float thr_at(const float *__restrict__ thr, const long long P, const long long slice_len,
                                        const size_t block_bytes, const int j, const long long p)
{
    if (slice_len == 0) return thr[j * P + p];
    const long long k = p / slice_len, q = p - k * slice_len;
    return ((const float *)((const char *)thr + (size_t)k * block_bytes + (size_t)slice_len * 32))[j * slice_len + q];
}

template <int MODE, int LAY>
__global__ __launch_bounds__(256) void poisson_call_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ ext_pos,
    const int T, const float *__restrict__ thr, const long long thr_L, const size_t thr_bb,
    const unsigned char *__restrict__ ref_code, const int cov,
    unsigned char *__restrict__ call_mask, ampli_call *__restrict__ calls, const long long capacity,
    unsigned long long *__restrict__ n_calls, double *__restrict__ qd, float *__restrict__ afd, const double *__restrict__ lgtab)
{
    constexpr int RB = rec_bytes(LAY);
    const long long R = P + E;
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const long long p = r < P ? r : (long long)ext_pos[r - P];
    float th[2][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        th[0][nt] = thr_at(thr, P, thr_L, thr_bb, 0 * 4 + nt, p); // VC:887-890
        th[1][nt] = thr_at(thr, P, thr_L, thr_bb, 1 * 4 + nt, p);
    }
    const int ref = ref_code[p];
    const int t0 = blockIdx.y * PC_SAMPLES;
    for (int dt = 0; dt < PC_SAMPLES; ++dt) {
        const int t = t0 + dt;
        if (t >= T) break;
        const size_t o = (size_t)t * R + r;
        const char *q = r < P ? rv.base + ((size_t)t * (size_t)rv.row_stride + (size_t)r) * RB
                              : rv.ext + ((size_t)t * (size_t)rv.ext_stride + (size_t)(r - P)) * RB;
        int4 r0, r1;
        rec_decode<LAY>(rec_load_at<LAY>(q), r0, r1);
        const bool present = r0.x != AMPLI_ABSENT;
        const int fw[4] = {r0.x, r0.y, r0.z, r0.w};
        const int bw[4] = {r1.x, r1.y, r1.z, r1.w};
        const int FW = fw[0] + fw[1] + fw[2] + fw[3]; // VC:760
        const int BW = bw[0] + bw[1] + bw[2] + bw[3]; // VC:761
        const int *rdp = r < P ? rv.rd : rv.rd_ext;   // the RD column of lines where it is not A+C+G+T (VC:762-765)
        const int rdc = rdp ? rdp[r < P ? (size_t)t * P + r : (size_t)t * E + (r - P)] : AMPLI_ABSENT;
        const int RD = rdc != AMPLI_ABSENT ? rdc : FW + BW;
        const bool covok = FW >= cov && BW >= cov;    // VC:898
        unsigned mask = 0;
        if (qd) {
#pragma unroll
            for (int j = 0; j < 8; ++j) qd[o * 8 + j] = -1.0;
        }
        if (afd) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) { // VC:772-817
                afd[o * 12 + nt * 3 + 0] = present ? (float)(fw[nt] + bw[nt]) / (float)RD : 0.0f;
                afd[o * 12 + nt * 3 + 1] = (present && FW != 0) ? (float)fw[nt] / (float)FW : 0.0f;
                afd[o * 12 + nt * 3 + 2] = (present && BW != 0) ? (float)bw[nt] / (float)BW : 0.0f;
            }
        }
        if (present && ref <= 3) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                if (nt == ref) continue;
                // VC:895-896: forward depth is RD - RD_reverse
                const int k_fw = fw[nt], d_fw = RD - BW, k_bw = bw[nt], d_bw = BW;
                double q_fw, q_bw;
                if (MODE == AMPLI_POISSON_PREFILTER) {
                    if (!covok) continue;
                    if (ampli_prefilter_nocall(k_fw, d_fw, th[0][nt]) || ampli_prefilter_nocall(k_bw, d_bw, th[1][nt])) continue;
                    q_fw = ampli_poisson_score(k_fw, d_fw, th[0][nt]);
                    if (!(q_fw >= 5.0 - AMPLI_CALL_GATE_EPS)) continue;
                    q_bw = ampli_poisson_score(k_bw, d_bw, th[1][nt]);
                } else {
                    // every score of every record, as the reference evaluates them (VC:895-896) -- through the integer-count
                    // form of the same scorer (csrc/ampli_math.h, ampli_poisson_score_dense)
                    q_fw = ampli_poisson_score_dense(k_fw, d_fw, th[0][nt], lgtab, AMPLI_LGTAB);
                    q_bw = ampli_poisson_score_dense(k_bw, d_bw, th[1][nt], lgtab, AMPLI_LGTAB);
                    if (qd) { qd[o * 8 + nt * 2 + 0] = q_fw; qd[o * 8 + nt * 2 + 1] = q_bw; }
                }
                const bool is_call = covok && q_fw >= 5 && q_bw >= 5; // VC:898
                const double lo = 5.0 - AMPLI_CALL_GATE_EPS, hi = 5.0 + AMPLI_CALL_GATE_EPS;
                const bool near_gate = covok && q_fw >= lo && q_bw >= lo && (q_fw < hi || q_bw < hi); // AMPLI_CALL_BORDERLINE
                if (is_call) mask |= 1u << nt;
                if ((is_call || near_gate) && n_calls) {
                    const long long idx = call_slot(n_calls, capacity);
                    if (calls && idx >= 0) {
                        ampli_call c;
                        call_fill(c, t, (int)r, nt, RD, q_fw, q_bw, k_fw, k_bw, FW, BW, near_gate ? AMPLI_CALL_BORDERLINE : 0);
                        calls[idx] = c;
                    }
                }
            }
        }
        call_mask[o] = (unsigned char)mask;
    }
}

// ---------------------------------------------------------------------------
// poisson_call, all-scores mode (AMPLI_POISSON_FULL), round 5: every score of every record, as the reference evaluates them
// (VC:895-896), scheduled by how much work a score is.  On a ctDNA-like panel (config 3) 45 % of the (record, alternative,
// strand) scores have k = 0 (p = 1, VC:3858-3861), 53 % lie on the continued fraction's side (z = RD err > k >= 1), nearly all
// of them with k <= 4 (0.7 % with k > 20), and 2.5 % take the series (16+ terms).  Evaluated lane by lane (round 4's kernel,
// kept for the dense-VAF validation output) a wave pays the series AND the longest continued fraction of its 64 lanes in every
// one of its six score slots: 80 % of the wave-slots hold a series lane, a third a lane with k > 20.
// Here a lane evaluates its LIGHT scores in place -- k = 0, the special error codes, and the continued fraction's side up to
// k = AMPLI_HORNER_K in its closed form (ampli_gammaq_horner_int: one exp, k - 1 FMAs) -- and hands the HEAVY ones -- series;
// longer continued fractions -- to two lists in LDS, which the whole workgroup then evaluates densely, a list at a time: a wave
// runs ONE of the two loops, over lanes that all need it.  The scorer is ampli_poisson_p_dense, item for item, wherever it runs.
// Config 3, uint16 records: 1.49 ms (round 4) -> 1.03-1.11 (lists; generic fraction loop in place) -> 0.55 ms (closed form).
// p is kept, not Q: -10 log10 p is only taken where somebody reads it -- the dense output, and pairs that can pass the gate
// (p <= PF_GATE_P on both strands, a superset of Q >= 5 - 1e-6; the decisions themselves are then made on Q, as ever).
// ---------------------------------------------------------------------------
constexpr int PF_LIST = 384; // heavy items per list and sample row of a workgroup (config 3: ~40 series + ~10 long fractions of 1536 scores)
constexpr double PF_GATE_P = 0.3162279; // > 10^-(5 - 1e-6)/10 = 0.31622783...: Q >= 5 - AMPLI_CALL_GATE_EPS implies p <= PF_GATE_P
constexpr double PF_P_CODE = 2.0, PF_P_NONE = 3.0; // in place of a p: err == -1 (Q = -888, VC:3844-3849) | not scored
struct PfItem { int k, d; float err; int slot; }; // slot = owning thread * 6 + alternative * 2 + strand

__device__ __forceinline__ double pf_q(const double p) { return p == PF_P_CODE ? -888.0 : p == PF_P_NONE ? -1.0 : ampli_q_from_p(p); }

template <int LAY>
__global__ __launch_bounds__(256, 4) void poisson_full_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ ext_pos,
    const int T, const float *__restrict__ thr, const long long thr_L, const size_t thr_bb,
    const unsigned char *__restrict__ ref_code, const int cov,
    unsigned char *__restrict__ call_mask, ampli_call *__restrict__ calls, const long long capacity,
    unsigned long long *__restrict__ n_calls, double *__restrict__ qd, const double *__restrict__ lgtab)
{
    constexpr int RB = rec_bytes(LAY);
    __shared__ PfItem items[2][PF_LIST]; // [0] series, [1] long continued fractions; a full list sends its item back to be scored in place
    __shared__ double res[256 * 6];      // by owning thread and score slot (the three alternatives x two strands)
    __shared__ int n_list[2];
    const long long R = P + E;
    const long long r_raw = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = r_raw < R; // lanes past the end keep company at the barriers
    const long long r = in_range ? r_raw : R - 1;
    const long long p = r < P ? r : (long long)ext_pos[r - P];
    float th[2][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        th[0][nt] = thr_at(thr, P, thr_L, thr_bb, 0 * 4 + nt, p); // VC:887-890
        th[1][nt] = thr_at(thr, P, thr_L, thr_bb, 1 * 4 + nt, p);
    }
    const int ref = ref_code[p];
    const int t0 = blockIdx.y * PC_SAMPLES;
    for (int dt = 0; dt < PC_SAMPLES; ++dt) {
        const int t = t0 + dt;
        if (t >= T) break; // block-uniform
        if (threadIdx.x < 2) n_list[threadIdx.x] = 0;
        __syncthreads(); // also: every lane has collected its results of the previous sample
        const size_t o = (size_t)t * R + r;
        const char *q = r < P ? rv.base + ((size_t)t * (size_t)rv.row_stride + (size_t)r) * RB
                              : rv.ext + ((size_t)t * (size_t)rv.ext_stride + (size_t)(r - P)) * RB;
        int4 r0, r1;
        rec_decode<LAY>(rec_load_at<LAY>(q), r0, r1);
        const bool present = r0.x != AMPLI_ABSENT;
        const int fw[4] = {r0.x, r0.y, r0.z, r0.w};
        const int bw[4] = {r1.x, r1.y, r1.z, r1.w};
        const int FW = fw[0] + fw[1] + fw[2] + fw[3]; // VC:760
        const int BW = bw[0] + bw[1] + bw[2] + bw[3]; // VC:761
        const int *rdp = r < P ? rv.rd : rv.rd_ext;   // the RD column of lines where it is not A+C+G+T (VC:762-765)
        const int rdc = rdp ? rdp[r < P ? (size_t)t * P + r : (size_t)t * E + (r - P)] : AMPLI_ABSENT;
        const int RD = rdc != AMPLI_ABSENT ? rdc : FW + BW;
        const bool covok = FW >= cov && BW >= cov;    // VC:898
        const bool scored = in_range && present && ref <= 3;
        double pv[4][2];
        unsigned pending = 0; // bit nt * 2 + strand: the p comes back through res[]
        int alt = 0;          // running index of the alternative nucleotide (0 .. 2)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            pv[nt][0] = pv[nt][1] = PF_P_NONE;
            if (!scored || nt == ref) continue;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const int k = st ? bw[nt] : fw[nt], d = st ? BW : RD - BW; // VC:895-896: forward depth is RD - RD_reverse
                float err = th[st][nt];
                if (err == -1) { pv[nt][st] = PF_P_CODE; continue; } // VC:3844-3849
                if (err == 0) err = 0.0010008f;                       // VC:3852-3856
                if (k == 0) { pv[nt][st] = 1.0; continue; }           // VC:3858-3861
                const double z = (double)d * err;                     // VC:3864
                const bool series = z <= 1. || z < (double)k;         // VC:3728
                // light: the closed form of the fraction's side; and, in place because it never happens on real panels, whatever
                // is not a count or has z <= 0 / NaN (the literal arithmetic)
                const bool light = k < 0 || !(z > 0) || (!series && k <= AMPLI_HORNER_K && z < 838860.8);
                int at = PF_LIST;
                if (!light) at = atomicAdd(&n_list[series ? 0 : 1], 1);
                if (at < PF_LIST) {
                    PfItem it;
                    it.k = k; it.d = d; it.err = err; it.slot = (int)threadIdx.x * 6 + alt * 2 + st;
                    items[series ? 0 : 1][at] = it;
                    pending |= 1u << (nt * 2 + st);
                } else {
                    pv[nt][st] = ampli_poisson_p_dense(k, d, err, lgtab, AMPLI_LGTAB);
                }
            }
            ++alt;
        }
        __syncthreads();
        // the heavy items, densely: all lanes of a pass run the same loop (series: 16+ terms; continued fraction: 4 .. 99 steps)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const int n = min(n_list[l], PF_LIST);
            for (int i = threadIdx.x; i < n; i += 256) {
                const PfItem it = items[l][i];
                res[it.slot] = ampli_poisson_p_dense(it.k, it.d, it.err, lgtab, AMPLI_LGTAB);
            }
        }
        __syncthreads();
        if (!in_range) continue;
        unsigned mask = 0;
        alt = 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
            for (int st = 0; st < 2; ++st)
                if ((pending >> (nt * 2 + st)) & 1) pv[nt][st] = res[threadIdx.x * 6 + alt * 2 + st];
            if (scored && nt != ref) ++alt;
            if (qd) { qd[o * 8 + nt * 2 + 0] = pf_q(pv[nt][0]); qd[o * 8 + nt * 2 + 1] = pf_q(pv[nt][1]); } // -1: not scored (reference nucleotide, absent record)
            // VC:898 needs Q >= 5 on both strands: nothing with p > PF_GATE_P on a strand can pass it or lie within 1e-6 of it
            if (!(covok && pv[nt][0] <= PF_GATE_P && pv[nt][1] <= PF_GATE_P)) continue;
            const double q_fw = ampli_q_from_p(pv[nt][0]), q_bw = ampli_q_from_p(pv[nt][1]);
            const bool is_call = q_fw >= 5 && q_bw >= 5; // VC:898 (coverage checked above)
            const double lo = 5.0 - AMPLI_CALL_GATE_EPS, hi = 5.0 + AMPLI_CALL_GATE_EPS;
            const bool near_gate = q_fw >= lo && q_bw >= lo && (q_fw < hi || q_bw < hi); // AMPLI_CALL_BORDERLINE
            if (is_call) mask |= 1u << nt;
            if ((is_call || near_gate) && n_calls) {
                const long long idx = call_slot(n_calls, capacity);
                if (calls && idx >= 0) {
                    ampli_call c;
                    call_fill(c, t, (int)r, nt, RD, q_fw, q_bw, fw[nt], bw[nt], FW, BW, near_gate ? AMPLI_CALL_BORDERLINE : 0);
                    calls[idx] = c;
                }
            }
        }
        call_mask[o] = (unsigned char)mask;
    }
}

// ---------------------------------------------------------------------------
// poisson_call, prefilter mode = two kernels.
//
// poisson_stream_kernel: one lane per record, one WAVE per (64-record tile, group of tumour rows); the four waves of a
//   workgroup take four consecutive row groups of the same tile, so the tile's thresholds / reference codes (33 B per
//   position) are fetched once per workgroup and hit L1/L2 for the other three waves, and the workgroups of one tile
//   are dealt to ONE XCD (blockIdx -> (tile, row group) mapping below) so that they share that XCD's L2 copy: the
//   thresholds cross the fabric about once per launch instead of once per four rows.
//   Most (record, alt) pairs are settled by a conservative fp32 form of the exact bound "k <= m = RD*err => Q < 5"
//   (ampli_prefilter_nocall):       skip  <=>  float(k) <= (float(RD) * 0.999999f) * err_eff
//   which implies k < m (both operands are exact floats below 2^24 and the product is rounded below RD*err), with
//   err_eff = +inf for err == -1 (Q = -888) and 0.0010008f for err == 0.  Anything not provably skippable -- real
//   variants, noisy cells, the rounding fringe: ~0.2 % of the records -- is appended to a queue in HBM.
// poisson_drain_kernel<LPS>: evaluates the queue DENSELY with the kf scorer, LPS lanes per (item, strand); ORs the
//   call bits into the mask and appends the compact call records.
//
// Evaluating survivors in place would stall 63 lanes behind one ~100-iteration fp64 loop; draining per wave from
// LDS (an earlier version) still paid one such loop per wave for a couple of items.
// ---------------------------------------------------------------------------

// blockIdx.x -> (tile, row group): workgroups are dealt round-robin to the 8 XCDs (b and b + 8 share one), so the
// row groups of a tile are given consecutive slots of ONE XCD.  tiles8 = tiles rounded up to a multiple of 8.
__device__ __forceinline__ void pc_block_map(const unsigned b, const unsigned gy, unsigned &tile, unsigned &y)
{
    const unsigned xcd = b & 7u, slot = b >> 3;
    tile = (slot / gy) * 8u + xcd;
    y = slot % gy;
}

// Seven waves per SIMD (72 VGPRs), not eight: at 64 VGPRs the compiler spilled 7-23 registers to scratch, and every wave's
// spill stores are HBM writes -- r03's PMC showed them as WRITE_SIZE 17.1 MB against a 9.6 MB mask ("the mask touched twice"
// of VERDICT r03; the mask is written once).  Round 4, tools/ps_spill_ab.sh: 8 waves with spills 47.2-47.8 us per call, 7 waves
// without 45.4-45.7 us (uint16 records; 24-byte records 61 -> 59.7 us); six waves (80 VGPRs) gain nothing more and lose 10 %
// with 24-byte records.
template <int LAY, bool IRR>
__global__ __launch_bounds__(256, 7) void poisson_stream_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ ext_pos,
    const int T, const int rows_per_wave, const unsigned gy, const float *__restrict__ thr, const long long thr_L, const size_t thr_bb,
    const unsigned char *__restrict__ ref_code,
    const int cov, PcItem *__restrict__ queue, const long long queue_per_shard, unsigned long long *__restrict__ queue_n,
    unsigned char *__restrict__ call_mask, int *__restrict__ flags, unsigned long long *__restrict__ n_calls,
    const long long r_lo, const long long r_hi, const unsigned shard_lo, const unsigned shard_n)
{
    // records [r_lo, r_hi) of every sample's R = P + E (the whole row, or one range of a context with position ranges: r_lo a
    // multiple of 64, the call list's shards [shard_lo, shard_lo + shard_n) are this launch's)
    constexpr int RB = rec_bytes(LAY);
    __shared__ PcItem stage[4][PC_STAGE];
    int staged = 0; // wave-uniform
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long R = P + E;
    // the call-list counters are reset here: only the drain kernel, which starts after this one has finished,
    // appends to the list
    if (n_calls && blockIdx.x == 0 && threadIdx.x < shard_n) n_calls[(shard_lo + threadIdx.x) * AMPLI_CALL_COUNTER_STRIDE] = 0ull;
    unsigned tile, y;
    pc_block_map(blockIdx.x, gy, tile, y);
    const long long r_raw = r_lo + (long long)tile * 64 + lane;
    const int t0 = ((int)y * 4 + wave) * rows_per_wave; // this wave's run of rows
    const int nt_rows = min(rows_per_wave, T - t0);
    // padding workgroups of the XCD mapping and waves beyond the last row only clear their share of the mask (below)
    const bool has_rows = r_lo + (long long)tile * 64 < r_hi && nt_rows > 0;
    const bool valid = r_raw < r_hi;
    const long long r = valid ? r_raw : r_hi - 1;
    // Everything the row loop needs from memory is REQUESTED first -- the position's reference code, its eight thresholds, the
    // first record -- and only then is the wave's share of the call mask cleared: written the other way round, the loads queue
    // behind the mask stores (vmcnt counts both, in order) and behind one another (two dependent round trips before row 0).
    long long p = 0;
    int ref = 255;
    float traw[2][4];
    RawRec<LAY> nx;
    size_t step = 0;
    const char *__restrict__ q = nullptr;
    if (has_rows) {
        p = r < P ? r : (long long)ext_pos[r - P];
        // where this position's eight thresholds live: the plane-major table, or the block of the position's slice (one
        // integer division per lane, done once)
        const float *__restrict__ tbase = thr;
        long long tstride = P, tp = p;
        if (thr_L != 0) {
            const long long k = p / thr_L;
            tbase = (const float *)((const char *)thr + (size_t)k * thr_bb + (size_t)thr_L * 32);
            tstride = thr_L;
            tp = p - k * thr_L;
        }
        step = (size_t)(r < P ? rv.row_stride : rv.ext_stride) * RB; // bytes between consecutive samples
        q = r < P ? rv.base + ((size_t)t0 * (size_t)rv.row_stride + (size_t)r) * RB
                  : rv.ext + ((size_t)t0 * (size_t)rv.ext_stride + (size_t)(r - P)) * RB;
        nx = rec_load_at<LAY>(q);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
            for (int st = 0; st < 2; ++st) traw[st][nt] = tbase[(st * 4 + nt) * tstride + tp];
        }
        ref = valid ? (int)ref_code[p] : 255;
    }
    // The call mask starts as "no call" (the drain ORs bits in).  Every wave of the grid clears an equal, CONTIGUOUS share
    // of the mask's bytes -- whole 128-byte lines, one store instruction per 256 bytes -- rather than the 64 scattered
    // bytes per row that belong to its own records (partial-line writes cost the streaming kernel ~10 % in the loop).
    // (Clearing when a wave leaves instead of when it starts was measured twice: no faster.)
    if (r_lo == 0 && r_hi == R) {
        const size_t m4 = ((size_t)T * (size_t)R + 3) / 4;       // the mask as dwords (the buffer is padded to a multiple of 4)
        const size_t share = (size_t)rows_per_wave * 16;         // dwords per wave: grid waves x share >= m4
        const size_t w0 = ((size_t)blockIdx.x * 4 + wave) * share;
        const size_t w1 = w0 + share < m4 ? w0 + share : m4;
        for (size_t o = w0 + lane; o < w1; o += 64) ((unsigned *)call_mask)[o] = 0u;
    } else {
        // a range owns bytes [t R + r_lo, t R + r_hi) of every row t: T segments of seg dwords (the host only cuts ranges when R,
        // r_lo and r_hi are multiples of 4), cleared in the same contiguous shares, a share wrapping from one row's segment to the next's
        const size_t seg = (size_t)(r_hi - r_lo) >> 2, m4 = (size_t)T * seg;
        const size_t share = (size_t)rows_per_wave * 16;
        const size_t w0 = ((size_t)blockIdx.x * 4 + wave) * share;
        const size_t w1 = w0 + share < m4 ? w0 + share : m4;
        if (w0 < w1) {
            const size_t row0 = w0 / seg, off0 = w0 - row0 * seg; // wave-uniform
            for (size_t i = lane; w0 + i < w1; i += 64) {
                size_t o = off0 + i, row = row0;
                while (o >= seg) { o -= seg; ++row; }
                ((unsigned *)call_mask)[((row * (size_t)R + (size_t)r_lo) >> 2) + o] = 0u;
            }
        }
    }
    if (!has_rows) return;
    float te[2][4]; // effective error per strand / nucleotide
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int st = 0; st < 2; ++st) te[st][nt] = ampli_effective_err(traw[st][nt]); // VC:887-890
    }
    const unsigned shard = blockIdx.x % AMPLI_CALL_SHARDS;

    for (int dt = 0; dt < nt_rows; ++dt) {
        int4 r0v, r1v;
        rec_decode<LAY>(nx, r0v, r1v);
        if (dt + 1 < nt_rows) { // prefetch the next sample row
            q += step;
            nx = rec_load_at<LAY>(q);
        }
        const int fw[4] = {r0v.x, r0v.y, r0v.z, r0v.w};
        const int bw[4] = {r1v.x, r1v.y, r1v.z, r1v.w};
        const int FW = fw[0] + fw[1] + fw[2] + fw[3]; // VC:760
        const int BW = bw[0] + bw[1] + bw[2] + bw[3]; // VC:761
        int RD = FW + BW;
        if (IRR) { // cohorts with lines whose RD column is not A+C+G+T (VC:762-765): the column decides (VC:895, VC:814)
            const int *rdp = r < P ? rv.rd : rv.rd_ext;
            const int rdc = rdp ? rdp[r < P ? (size_t)(t0 + dt) * P + r : (size_t)(t0 + dt) * E + (r - P)] : AMPLI_ABSENT;
            if (rdc != AMPLI_ABSENT) RD = rdc;
        }
        const int d_fw = RD - BW, d_bw = BW;          // VC:895-896
        const bool live = valid && r0v.x != AMPLI_ABSENT && ref <= 3 && FW >= cov && BW >= cov; // VC:898, VC:3290
        // conservative fp32 bound (ampli_prefilter_skip_f32, hoisted); depths or counts >= 2^24 are not exact
        // floats: never skip those
        const bool exact = (unsigned)RD < (unsigned)AMPLI_COUNT_LIMIT && FW >= 0 && BW >= 0 && d_fw >= 0;
        const float c_fw = (float)d_fw * 0.999999f, c_bw = (float)d_bw * 0.999999f;
        unsigned pushmask = 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const bool skip_fw = exact && (unsigned)fw[nt] < (unsigned)AMPLI_COUNT_LIMIT && (float)fw[nt] <= c_fw * te[0][nt];
            const bool skip_bw = exact && (unsigned)bw[nt] < (unsigned)AMPLI_COUNT_LIMIT && (float)bw[nt] <= c_bw * te[1][nt];
            if (live && nt != ref && !skip_fw && !skip_bw) pushmask |= 1u << nt;
        }
        // (the same staging, with another fill of the item: loo_stream_kernel, ampli_loo.hip; a shared helper changes this kernel's code)
        if (__any(pushmask != 0)) { // rare: stage the items in LDS, one slot range per wave
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const bool push = (pushmask >> nt) & 1;
                const unsigned long long bal = __ballot(push);
                if (bal) {
                    const int n = __popcll(bal);
                    if (staged + n > PC_STAGE) { // wave-uniform: no room for this batch -> hand the staged items over first
                        pc_flush(stage[wave], staged, lane, queue, queue_per_shard, queue_n, shard, flags);
                        staged = 0;
                    }
                    if (push) {
                        PcItem it;
                        it.sample = t0 + dt; it.record_alt = (int)r | (nt << 30);
                        it.k_fw = fw[nt]; it.k_bw = bw[nt]; it.FW = FW; it.BW = BW; it.rd = RD;
                        it.e_fw = te[0][nt]; it.e_bw = te[1][nt]; it.pad = 0;
                        stage[wave][staged + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0))] = it;
                    }
                    staged += n;
                }
            }
        }
    }
    if (staged) pc_flush(stage[wave], staged, lane, queue, queue_per_shard, queue_n, shard, flags);
}

__global__ __launch_bounds__(256) void poisson_drain_kernel(
    const PcItem *__restrict__ queue, const long long queue_per_shard, const unsigned long long *__restrict__ queue_n,
    const long long R, unsigned *__restrict__ mask_words, ampli_call *__restrict__ calls, const long long capacity,
    unsigned long long *__restrict__ n_calls, unsigned long long *__restrict__ next_queue_n, const unsigned shard_lo, const unsigned shard_n,
    const double *__restrict__ lgtab)
{
    drain_body<false>(queue, queue_per_shard, queue_n, R, mask_words, calls, capacity, n_calls, next_queue_n, shard_lo, shard_n, lgtab);
}

__global__ void lgamma_table_kernel(double *t, const int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = ampli_kf_lgamma((double)i);
}

int ensure_lgtab(ampli_ctx *ctx)
{
    if (ctx->d_lgtab) return AMPLI_OK;
    if (is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "the lgamma table would have to be built while capturing: run the sequence once first");
    if (hipMalloc((void **)&ctx->d_lgtab, sizeof(double) * AMPLI_LGTAB) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "lgamma table hipMalloc failed");
    hipLaunchKernelGGL(lgamma_table_kernel, dim3((AMPLI_LGTAB + 255) / 256), dim3(256), 0, main_stream(ctx), ctx->d_lgtab, AMPLI_LGTAB);
    return check_launch(ctx, "lgamma_table_kernel");
}

// the shard counters of one half of the queue's double buffer back to zero (captured passes only, below)
__global__ void queue_counters_reset_kernel(unsigned long long *__restrict__ qn)
{
    qn[threadIdx.x * AMPLI_CALL_COUNTER_STRIDE] = 0ull;
}

// The prefilter queue of a launch on `st`: at least `want` items (rounded up to whole shards), and the half of the double-buffered shard
// counters this launch appends to (qn; the stream kernel finds it zeroed) and the half its drain resets for the next launch (qn_next)
int queue_prepare(ampli_ctx *ctx, AmpliQueue &Q, size_t want, hipStream_t st, long long &per, unsigned long long *&qn,
                         unsigned long long *&qn_next)
{
    want = (want + AMPLI_CALL_SHARDS - 1) / AMPLI_CALL_SHARDS * AMPLI_CALL_SHARDS;
    const bool capturing = is_capturing(ctx);
    if ((Q.n_items < want || !Q.n) && capturing)
        return fail(ctx, AMPLI_E_INVALID, "queue would have to be allocated while capturing: run the sequence once first");
    if (Q.n_items < want) {
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (Q.items) (void)hipFree(Q.items);
        Q.items = nullptr; Q.n_items = 0;
        if (hipMalloc(&Q.items, want * sizeof(PcItem)) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "queue hipMalloc failed");
        Q.n_items = want;
    }
    if (!Q.n) {
        if (hipMalloc((void **)&Q.n, 2 * sizeof(unsigned long long) * AMPLI_CALL_COUNTER_WORDS) != hipSuccess)
            return fail(ctx, AMPLI_E_NOMEM, "queue counter hipMalloc failed");
        HIP_TRY(ctx, hipMemsetAsync(Q.n, 0, 2 * sizeof(unsigned long long) * AMPLI_CALL_COUNTER_WORDS, st));
    }
    per = (long long)(Q.n_items / AMPLI_CALL_SHARDS);
    qn = Q.n + (size_t)(Q.parity & 1) * AMPLI_CALL_COUNTER_WORDS;
    qn_next = Q.n + (size_t)((Q.parity + 1) & 1) * AMPLI_CALL_COUNTER_WORDS;
    if (capturing) { // a replayed graph cannot alternate halves: reset the half it uses with a node of its own instead.  A KERNEL node: behind a
        // memset node the stream kernel of a replay found counters that were not zero -- AMPLI_FLAG_QUEUE_OVERFLOW from the second or third
        // replay on with a handful of items queued, and once a call listed twice (tests/test_gpu_output_contracts.py, the hipGraph case)
        hipLaunchKernelGGL(queue_counters_reset_kernel, dim3(1), dim3(AMPLI_CALL_SHARDS), 0, st, qn);
        int rcz = check_launch(ctx, "queue_counters_reset_kernel");
        if (rcz) return rcz;
    }
    else
        Q.parity ^= 1;
    return AMPLI_OK;
}

// poisson_call, prefilter mode: poisson_stream_kernel + poisson_drain_kernel over the records [r_lo, r_hi) of every sample, on
// `st`, with lane `lane_k`'s queue and the call list's shards [shard_lo, shard_lo + shard_n) (the whole row, lane 0 and every shard
// unless the context runs position ranges)
static int poisson_prefilter_launch(ampli_ctx *ctx, const int lane_k, hipStream_t st, const DevCohort &co, const int64_t P, const float *d_thr,
                                    const long long thr_L, const size_t thr_bb, const uint8_t *d_ref_code, const int32_t cov, uint8_t *d_call_mask,
                                    ampli_call *d_calls, const int64_t capacity, unsigned long long *d_n_calls, const long long r_lo,
                                    const long long r_hi, const unsigned shard_lo, const unsigned shard_n)
{
    const int64_t E = co.E;
    const int32_t T = co.n;
    const uint32_t *d_ext_pos = co.ext_pos;
    const long long R = P + E, Rk = r_hi - r_lo;
    AmpliQueue &Q = ctx->lanes[lane_k].q;
    // one wave per (64-record tile, rows_per_wave tumour rows), four row groups per workgroup.  Few rows per wave =
    // many short waves that keep every CU fed through the tail; the thresholds of a tile are shared through the
    // XCD's L2 by the mapping of poisson_stream_kernel, so short waves no longer cost re-reads over the fabric.
    const long long tiles = (Rk + 63) / 64, tiles8 = (tiles + 7) / 8 * 8;
    // rows per wave: long-lived waves stream best from cold HBM (config 3 in bench.py's loop: 24 rows 0.062 ms, 8 rows
    // 0.065 ms, 4 rows 0.068 ms), as long as the launch still fills the chip: halve them while it would leave more than
    // half of the wave slots empty (a range counts for the launch of the whole row it is a part of)
    const long long tiles_all = (R + 63) / 64;
    int rpw = ctx->pc_rows_per_wave > 0 ? ctx->pc_rows_per_wave : 24;
    if (rpw > (T + 3) / 4) rpw = (T + 3) / 4;
    if (ctx->pc_rows_per_wave <= 0)
        while (rpw > 2 && tiles_all * 4 * ((T + 4 * rpw - 1) / (4 * rpw)) < (long long)ctx->n_cu * 16) rpw = (rpw + 1) / 2;
    if (rpw < 1) rpw = 1;
    long long gy = (T + 4 * rpw - 1) / (4 * rpw);
    // the same number of row groups with the rows dealt evenly: 128 tumours are 2 x 4 x 16 rows, not 4 x 24 + 4 x 8 -- a thin tumour
    // shard (config 4 cut eight ways) otherwise ends on workgroups with a third of the others' rows: 64.0 -> 55.4 us for its call
    // (round 6, tools/experiments/r06_poisson_fused_per_workgroup.log, run 3)
    if (ctx->pc_rows_per_wave <= 0) rpw = (int)((T + 4 * gy - 1) / (4 * gy));
    while (tiles8 * gy > 0x7fffffffll) { rpw *= 2; gy = (T + 4 * rpw - 1) / (4 * rpw); } // gridDim.x limit
    // queue workspace: T*R/4 items by default (the synthetic and Toy_data panels queue ~0.2 % of the records),
    // or what ampli_set_queue_items asked for plus one workgroup's worth of slack per shard (workgroups are dealt
    // to the shards round-robin, so a shard holds at most ceil(blocks/SHARDS) workgroups' items)
    size_t want = (size_t)std::max<long long>(1 << 16, (long long)T * Rk / 4);
    const size_t slack = (size_t)AMPLI_CALL_SHARDS * 256 * 3 * (size_t)rpw;
    if (ctx->queue_min_items) want = std::max(want, ctx->queue_min_items + slack);
    long long per;
    unsigned long long *qn, *qn_next;
    { int rcq = queue_prepare(ctx, Q, want, st, per, qn, qn_next); if (rcq) return rcq; }
    dim3 qgrid((unsigned)(tiles8 * gy));
    with_layout(co.layout, [&](auto L) {
        with_bool(co.rv.rd || co.rv.rd_ext, [&](auto IRR) {
            hipLaunchKernelGGL((poisson_stream_kernel<L, IRR>), qgrid, dim3(256), 0, st, co.rv, (long long)P, (long long)E, d_ext_pos, (int)T,
                               rpw, (unsigned)gy, d_thr, thr_L, thr_bb, d_ref_code, (int)cov, (PcItem *)Q.items, per, qn, d_call_mask,
                               ctx->d_flags, d_n_calls, r_lo, r_hi, shard_lo, shard_n);
        });
    });
    { int rc = check_launch(ctx, "poisson_stream_kernel"); if (rc) return rc; }
    hipStream_t dstream = st;
    if (ctx->async_drain) { // let the drain run beside whatever the caller enqueues next (never with ranges)
        HIP_TRY(ctx, hipEventRecord(ctx->ev_stream_done, st));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_stream_done, 0));
        dstream = ctx->side;
    }
    // AMPLI_CALL_SHARDS x dgy workgroups, 128 items per workgroup pass: one pass while up to ~1.4 % of the records are
    // queued (0.2 % on the synthetic and Toy_data panels); a workgroup without items leaves after one load
    const unsigned dgy = (unsigned)(ctx->pc_drain_blocks > 0 ? ctx->pc_drain_blocks
                                                             : std::min<long long>(1024, std::max<long long>(16, (long long)T * Rk / 300000)));
    hipLaunchKernelGGL(poisson_drain_kernel, dim3(AMPLI_CALL_SHARDS, dgy), dim3(256), 0, dstream, (const PcItem *)Q.items, per, qn,
                       (long long)R, (unsigned *)d_call_mask, d_calls, (long long)capacity, d_n_calls, qn_next, shard_lo, shard_n,
                       (const double *)ctx->d_lgtab);
    if (ctx->async_drain) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_drain_done, ctx->side));
        ctx->drain_pending = true;
    }
    return check_launch(ctx, "poisson_drain_kernel");
}

static int poisson_call_impl(ampli_ctx *ctx, const DevCohort &co, int64_t P, const float *d_thr, const long long thr_L, const size_t thr_bb,
                             const uint8_t *d_ref_code, int32_t cov, int32_t mode, uint8_t *d_call_mask, ampli_call *d_calls, int64_t capacity,
                             unsigned long long *d_n_calls, double *d_q, float *d_af)
{
    if (!ctx) return AMPLI_E_INVALID;
    const int64_t E = co.E;
    const int32_t T = co.n;
    const uint32_t *d_ext_pos = co.ext_pos;
    if (!co.rv.base || P <= 0 || E < 0 || T <= 0 || !d_thr || !d_ref_code || !d_call_mask || cov < 1)
        return fail(ctx, AMPLI_E_INVALID, "poisson_call: bad argument");
    { int rc = check_records(ctx, co, "poisson_call", d_ext_pos, "ext_pos"); if (rc) return rc; }
    if (mode != AMPLI_POISSON_FULL && mode != AMPLI_POISSON_PREFILTER) return fail(ctx, AMPLI_E_INVALID, "poisson_call: bad mode");
    if (d_q && mode != AMPLI_POISSON_FULL) return fail(ctx, AMPLI_E_INVALID, "poisson_call: dense q needs AMPLI_POISSON_FULL");
    if (d_calls && (!d_n_calls || capacity < AMPLI_CALL_SHARDS)) return fail(ctx, AMPLI_E_INVALID, "poisson_call: call list needs n_calls and capacity >= AMPLI_CALL_SHARDS");
    if (d_n_calls && !d_calls) capacity = 0;
    if (P + E >= (1ll << 30)) return fail(ctx, AMPLI_E_RANGE, "poisson_call: P + E must be below 2^30 records per sample");
    if ((T + PC_SAMPLES - 1) / PC_SAMPLES > 65535) return fail(ctx, AMPLI_E_RANGE, "poisson_call: more than 262140 tumour samples in one call (grid limit); split the cohort");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcj = join_drain(ctx); if (rcj) return rcj; } // the queue, its counters and the call list are about to be reused
    const long long R = P + E;
    dim3 grid((unsigned)((R + 255) / 256), (unsigned)((T + PC_SAMPLES - 1) / PC_SAMPLES));
    if (d_n_calls && (mode == AMPLI_POISSON_FULL || d_af)) // the two-kernel path resets the counters in-kernel
        HIP_TRY(ctx, hipMemsetAsync(d_n_calls, 0, sizeof(unsigned long long) * AMPLI_CALL_COUNTER_WORDS, main_stream(ctx)));
    auto launch_in_place = [&](auto MODE) { // poisson_call_kernel: every record evaluated by its own lane
        with_layout(co.layout, [&](auto L) {
            hipLaunchKernelGGL((poisson_call_kernel<MODE, L>), grid, dim3(256), 0, main_stream(ctx), co.rv, (long long)P, (long long)E, d_ext_pos,
                               (int)T, d_thr, thr_L, thr_bb, d_ref_code, (int)cov, d_call_mask, d_calls, (long long)capacity, d_n_calls, d_q,
                               d_af, (const double *)ctx->d_lgtab);
        });
    };
    if (mode == AMPLI_POISSON_FULL && !d_af) { // all six scores of every record: light ones in place, heavy ones compacted per workgroup
        { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
        with_layout(co.layout, [&](auto L) {
            hipLaunchKernelGGL((poisson_full_kernel<L>), grid, dim3(256), 0, main_stream(ctx), co.rv, (long long)P, (long long)E, d_ext_pos,
                               (int)T, d_thr, thr_L, thr_bb, d_ref_code, (int)cov, d_call_mask, d_calls, (long long)capacity, d_n_calls, d_q,
                               (const double *)ctx->d_lgtab);
        });
        return check_launch(ctx, "poisson_full_kernel");
    }
    if (mode == AMPLI_POISSON_FULL) {
        { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
        launch_in_place(Const<AMPLI_POISSON_FULL>{});
    } else if (d_af) { // dense VAFs are a validation output: literal per-lane kernel
        launch_in_place(Const<AMPLI_POISSON_PREFILTER>{});
    } else {
        if (((uintptr_t)d_call_mask & 3) != 0) return fail(ctx, AMPLI_E_INVALID, "poisson_call: call_mask must be 4-byte aligned");
        if (ctx->async_drain && is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "asynchronous drain cannot be captured");
        // the drain's scorer reads kf_lgamma at the integers from the table: built once, on the context's stream, BEFORE any range forks
        { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
        // position ranges on concurrent streams (ampli_set_ranges): every range behind its own error_estimate.  Only the listed-once
        // shape: an extra occurrence reads the thresholds of a position that may belong to another range
        const bool ranged = ranges_apply(ctx, R) && E == 0 && (R & 3) == 0 && !ctx->async_drain;
        if (!ranged) return poisson_prefilter_launch(ctx, 0, main_stream(ctx), co, P, d_thr, thr_L, thr_bb, d_ref_code, cov, d_call_mask, d_calls, capacity, d_n_calls,
                                                     0, R, 0, AMPLI_CALL_SHARDS);
        { int rcf = ranges_fork(ctx, P); if (rcf) return rcf; }
        long long cut[AMPLI_MAX_RANGES + 1];
        range_cuts(R, ctx->n_ranges, cut);
        for (int k = 0; k < ctx->n_ranges; ++k) {
            const unsigned s_lo = (unsigned)(AMPLI_CALL_SHARDS * k / ctx->n_ranges), s_hi = (unsigned)(AMPLI_CALL_SHARDS * (k + 1) / ctx->n_ranges);
            hipStream_t st = lane_stream(ctx, k);
            int rck = poisson_prefilter_launch(ctx, k, st, co, P, d_thr, thr_L, thr_bb, d_ref_code, cov, d_call_mask, d_calls, capacity, d_n_calls,
                                               cut[k], cut[k + 1], s_lo, s_hi - s_lo);
            if (rck) return rck;
        }
        return AMPLI_OK;
    }
    return check_launch(ctx, "poisson_call_kernel");
}

extern "C" int ampli_poisson_call(ampli_ctx *ctx, const int32_t *d_trecs, int64_t P, int64_t E, const uint32_t *d_ext_pos,
                                  int32_t T, const float *d_thr, const uint8_t *d_ref_code, int32_t cov, int32_t mode,
                                  uint8_t *d_call_mask, ampli_call *d_calls, int64_t capacity,
                                  unsigned long long *d_n_calls, double *d_q, float *d_af)
{
    if (!ctx) return AMPLI_E_INVALID;
    return poisson_call_impl(ctx, dense_cohort(ctx, d_trecs, P, E, T, nullptr, d_ext_pos), P, d_thr, 0, 0, d_ref_code, cov, mode, d_call_mask,
                             d_calls, capacity, d_n_calls, d_q, d_af);
}

extern "C" int ampli_poisson_call_records(ampli_ctx *ctx, const ampli_records *trecs, int64_t P, const float *d_thr, const uint8_t *d_ref_code,
                                          int32_t cov, int32_t mode, uint8_t *d_call_mask, ampli_call *d_calls, int64_t capacity,
                                          unsigned long long *d_n_calls, double *d_q, float *d_af)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, trecs, P, co); if (rc) return rc; }
    return poisson_call_impl(ctx, co, P, d_thr, 0, 0, d_ref_code, cov, mode, d_call_mask, d_calls, capacity, d_n_calls, d_q, d_af);
}

extern "C" int ampli_poisson_call_blocks(ampli_ctx *ctx, const int32_t *d_trecs, int64_t P, int64_t E, const uint32_t *d_ext_pos,
                                         int32_t T, const void *d_blocks, int32_t n_slices, const uint8_t *d_ref_code, int32_t cov,
                                         int32_t mode, uint8_t *d_call_mask, ampli_call *d_calls, int64_t capacity,
                                         unsigned long long *d_n_calls, double *d_q, float *d_af)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (n_slices < 1 || P <= 0) return fail(ctx, AMPLI_E_INVALID, "poisson_call_blocks: bad argument");
    const long long L = ampli_slice_len(P, n_slices);
    d_blocks = (const char *)d_blocks + (size_t)ctx->grp_index * slice_block_bytes(L); // [n_slices][group][block]: this batch's blocks
    return poisson_call_impl(ctx, dense_cohort(ctx, d_trecs, P, E, T, nullptr, d_ext_pos), P, (const float *)d_blocks, L,
                             (size_t)ctx->grp_size * slice_block_bytes(L), d_ref_code, cov, mode, d_call_mask, d_calls, capacity, d_n_calls, d_q, d_af);
}
