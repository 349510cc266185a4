// amplisolve_amd/csrc/ampli_exchange.hip -- merges and slices: partial accumulator tables of several launches or GPUs -> one error table.
//
// The kernels and entry points of the multi-GPU merges (amplisolve_amd/dist.py, ampli_comm.hip): the gathered merge (ampli_acc_merge,
// ampli_gm_merge), the all-reduce merge's packed planes (ampli_acc_pack / _unpack, ampli_error_finalize_merged) and the position-sliced
// merge (ampli_acc_to_slices, ampli_error_finalize_slice, ampli_error_table_unslice) with its buffer sizes.  error_reduce_impl
// (ampli_kernels.hip) fills the same exchange buffers straight from its epilogue; after a cut along the samples it calls
// launch_acc_pack here, and ampli_acc_to_slices calls its launch_acc_pack_sliced.  The accumulator state is ampli_device.h's.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// merge of arbitrary (non-strided) part tables: pointers passed through a small device array
__global__ __launch_bounds__(256) void acc_merge_ptr_kernel(AccPtrs dst, const AccPtrs *parts, const int nparts,
                                                            const long long P)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
    lane_acc_load(parts[0], P, p, a);
    for (int i = 1; i < nparts; ++i) {
        LaneAcc b;
        lane_acc_load(parts[i], P, p, b);
        lane_acc_merge(a, b);
    }
    lane_acc_store(dst, P, p, a);
}

// ---------------------------------------------------------------------------
// pack / unpack of the additive planes for the multi-GPU merge: ONE float64 buffer
// [snt 8P | srd 8P | cnt 4P | nrec P] so that the shards merge with a single RCCL all-reduce (SUM).
// srd / cnt / nrec are integers far below 2^53: exact in a double, exact under any summation order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void acc_pack_kernel(AccPtrs t, const long long P, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 21 * P) return;
    double v;
    if (i < 8 * P) v = t.snt[i];
    else if (i < 16 * P) v = (double)t.srd[i - 8 * P];
    else if (i < 20 * P) v = (double)t.cnt[i - 16 * P];
    else v = (double)t.nrec[i - 20 * P];
    out[i] = v;
}

__global__ __launch_bounds__(256) void acc_unpack_kernel(AccPtrs t, const long long P, const double *__restrict__ in)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 21 * P) return;
    const double v = in[i];
    if (i < 8 * P) t.snt[i] = v;
    else if (i < 16 * P) t.srd[i - 8 * P] = (long long)v;
    else if (i < 20 * P) t.cnt[i - 16 * P] = (int)v;
    else t.nrec[i - 20 * P] = (int)v;
}

// germ-max triples only.  regions: nparts copies of the gm region of a table (gm_n .. end of gm_rest),
// region k at regions + k*stride; plane offsets inside a region as in the table.
__global__ __launch_bounds__(256) void gm_merge_kernel(int *gm_n, int *gm_first, float *gm_first_af, float *gm_rest,
                                                       const char *regions, const size_t stride, const size_t ofa,
                                                       const size_t orr, const int nparts, const long long P)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; // over 4*P
    if (i >= 4 * P) return;
    int n = 0, first = 0x7fffffff;
    float first_af = 0.0f, rest = -INFINITY;
    for (int k = 0; k < nparts; ++k) {
        const char *b = regions + (size_t)k * stride;
        const int rn = ((const int *)b)[i];
        if (rn == 0) continue;
        const float fa = ((const float *)(b + ofa))[i], rr = ((const float *)(b + orr))[i];
        if (n == 0) {
            first = -1; first_af = fa; rest = rr; // the sample index is not exchanged: unknown after a gathered merge
        } else {
            if (rest <= fa) rest = fa;
            if (rest <= rr) rest = rr;
        }
        n += rn;
    }
    gm_n[i] = n; gm_first[i] = first; gm_first_af[i] = first_af; gm_rest[i] = rest;
}

// ---------------------------------------------------------------------------
// Position-sliced merge (reduce-scatter / all-to-all / all-gather): rank k owns positions [k*L, (k+1)*L).
//   error_finalize_slice_kernel: the reduce-scattered sums of one slice + every rank's germ-max pair for that slice
//                                (folded in rank order = sample order) -> one error-table block
//   error_table_unslice_kernel : the all-gathered blocks -> the plane-major error table poisson_call reads
// Block of a slice (all-gather unit): rate f32[8][L] | thr f32[8][L] | germ_val f32[4][L] | code u8[4][L] |
// germ_present u8[4][L] | 64-byte tail (int32 flags).
// ---------------------------------------------------------------------------
__device__ __forceinline__ FinOut slice_block_view(char *blk, const long long L)
{
    FinOut o = {};
    o.rate = (float *)blk;
    o.thr = (float *)(blk + (size_t)L * 32);
    o.germ_val = (float *)(blk + (size_t)L * 64);
    o.code = (unsigned char *)(blk + (size_t)L * 80);
    o.germ_present = (unsigned char *)(blk + (size_t)L * 84);
    o.flags = (int *)(blk + (size_t)L * 88);
    return o;
}

__global__ __launch_bounds__(256) void error_finalize_slice_kernel(const double *__restrict__ sums, const float *__restrict__ gm,
                                                                   const size_t gm_stride /* elements between the shards' pairs */,
                                                                   const int nparts, const long long L, const long long p0,
                                                                   const long long P, const float C, const int cov, char *blk, const int fmt)
{
    // one thread per (nucleotide, position of the slice): the slice is short (P / n positions), so the launch is a
    // latency chain -- four times the threads, a quarter of the chain
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nt = (int)(t / L);
    const long long q = t - (long long)nt * L;
    if (nt >= 4 || p0 + q >= P) return;
    int n = 0;
    float rest = -INFINITY;
    for (int k = 0; k < nparts; ++k) { // L (+) R = (L.first, max(L.rest, R.first_af, R.rest)), shards in sample order
        const float fa = gm[(size_t)k * gm_stride + (size_t)nt * L + q];
        if (fa < 0.0f) continue; // shard without a qualifying record
        const float rr = gm[(size_t)k * gm_stride + (size_t)(4 + nt) * L + q];
        if (n == 0) { rest = rr; n = (rr > -INFINITY) ? 2 : 1; } // n: 0, 1 or "more than one"
        else { if (rest <= fa) rest = fa; if (rest <= rr) rest = rr; n = 2; }
    }
    const FinOut o = slice_block_view(blk, L);
    long long d_fw, d_bw;
    int cnt, nrec;
    if (fmt == AMPLI_SLICE_SLIM) { // the summed fields come apart again: every one stayed below its width (checked where the shards packed them)
        const double d = sums[(8 + nt) * L + q], hi = floor(d / SLIM_D);
        d_fw = (long long)(d - hi * SLIM_D);
        d_bw = (long long)hi;
        const double c0 = sums[12 * L + q], c1 = sums[13 * L + q];
        const double c0_2 = floor(c0 / SLIM_C2), c0_r = c0 - c0_2 * SLIM_C2, c0_1 = floor(c0_r / SLIM_C), c0_0 = c0_r - c0_1 * SLIM_C;
        const double c1_1 = floor(c1 / SLIM_C), c1_0 = c1 - c1_1 * SLIM_C;
        cnt = (int)(nt == 0 ? c0_0 : nt == 1 ? c0_1 : nt == 2 ? c0_2 : c1_0);
        nrec = (int)c1_1;
    } else {
        d_fw = (long long)sums[(8 + 0 * 4 + nt) * L + q];
        d_bw = (long long)sums[(8 + 1 * 4 + nt) * L + q];
        cnt = (int)sums[(16 + nt) * L + q];
        nrec = (int)sums[20 * L + q];
    }
    const bool bad = finalize_one(nt, sums[(0 * 4 + nt) * L + q], sums[(1 * 4 + nt) * L + q], d_fw, d_bw, cnt, nrec, n, rest, L, q,
                                  envelope_limit(C, cov), o);
    if (bad) atomicOr(o.flags, 1);
}

__global__ __launch_bounds__(256) void error_table_unslice_kernel(const char *__restrict__ blocks, const size_t block_stride,
                                                                  const int nparts, const long long L, const long long P, const FinOut o)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 && o.flags) {
        int f = 0;
        for (int k = 0; k < nparts; ++k) f |= *(const int *)(blocks + (size_t)k * block_stride + (size_t)L * 88);
        if (f) atomicOr(o.flags, f);
    }
    if (p >= P) return;
    const long long k = p / L, q = p - k * L;
    const FinOut b = slice_block_view(const_cast<char *>(blocks) + (size_t)k * block_stride, L);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        o.rate[j * P + p] = b.rate[j * L + q];
        if (o.thr) o.thr[j * P + p] = b.thr[j * L + q];
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        o.code[nt * P + p] = b.code[nt * L + q];
        if (o.germ_val) o.germ_val[nt * P + p] = b.germ_val[nt * L + q];
        if (o.germ_present) o.germ_present[nt * P + p] = b.germ_present[nt * L + q];
    }
}

int launch_acc_pack(ampli_ctx *ctx, const AccPtrs &t, long long P, double *d_packed)
{
    hipLaunchKernelGGL(acc_pack_kernel, dim3((unsigned)((21 * P + 255) / 256)), dim3(256), 0, main_stream(ctx), t, P, d_packed);
    return check_launch(ctx, "acc_pack_kernel");
}

extern "C" int ampli_acc_merge(ampli_ctx *ctx, const ampli_acc_table *d_dst, const ampli_acc_table *d_parts, int32_t nparts)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_dst || !d_parts || nparts < 1 || nparts > 64) return fail(ctx, AMPLI_E_INVALID, "acc_merge: 1 <= nparts <= 64");
    const int64_t P = d_dst->P;
    for (int i = 0; i < nparts; ++i)
        if (d_parts[i].P != P) return fail(ctx, AMPLI_E_INVALID, "acc_merge: part table P mismatch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (is_capturing(ctx)) return fail(ctx, AMPLI_E_INVALID, "acc_merge cannot be captured (it uploads a pointer list)");
    { int rc = ensure_ws(ctx, sizeof(AccPtrs) * 64); if (rc) return rc; }
    AccPtrs hp[64];
    for (int i = 0; i < nparts; ++i) hp[i] = to_ptrs(&d_parts[i]);
    // small synchronous upload of the pointer list (not on a captured path)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws, hp, sizeof(AccPtrs) * nparts, hipMemcpyHostToDevice, main_stream(ctx)));
    HIP_TRY(ctx, hipStreamSynchronize(main_stream(ctx)));
    hipLaunchKernelGGL(acc_merge_ptr_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), to_ptrs(d_dst),
                       (const AccPtrs *)ctx->ws, (int)nparts, (long long)P);
    return check_launch(ctx, "acc_merge_ptr_kernel");
}

extern "C" int64_t ampli_acc_packed_len(int64_t P) { return P > 0 ? 21 * P : 0; }

extern "C" int ampli_acc_pack(ampli_ctx *ctx, const ampli_acc_table *d_acc, double *d_packed)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_acc || d_acc->P <= 0 || !d_packed) return fail(ctx, AMPLI_E_INVALID, "acc_pack: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_acc_pack(ctx, to_ptrs(d_acc), d_acc->P, d_packed);
}

extern "C" int ampli_acc_unpack(ampli_ctx *ctx, const double *d_packed, const ampli_acc_table *d_acc)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_acc || d_acc->P <= 0 || !d_packed) return fail(ctx, AMPLI_E_INVALID, "acc_unpack: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long P = d_acc->P;
    hipLaunchKernelGGL(acc_unpack_kernel, dim3((unsigned)((21 * P + 255) / 256)), dim3(256), 0, main_stream(ctx), to_ptrs(d_acc), P, d_packed);
    return check_launch(ctx, "acc_unpack_kernel");
}

extern "C" int ampli_acc_regions(int64_t P, size_t *sum_bytes, size_t *gm_offset, size_t *gm_bytes)
{
    if (P <= 0) return AMPLI_E_INVALID;
    size_t off[9];
    acc_offsets(P, off);
    if (sum_bytes) *sum_bytes = off[6]; // snt|srd|cnt|nrec|gm_n
    if (gm_offset) *gm_offset = off[4];
    if (gm_bytes) *gm_bytes = off[5] - off[4]; // gm_n|gm_first_af|gm_rest
    return AMPLI_OK;
}

extern "C" int ampli_gm_merge(ampli_ctx *ctx, const ampli_acc_table *d_dst, const void *d_regions, int32_t nparts)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_dst || !d_regions || nparts < 1) return fail(ctx, AMPLI_E_INVALID, "gm_merge: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long P = d_dst->P;
    size_t off[9];
    acc_offsets(P, off);
    hipLaunchKernelGGL(gm_merge_kernel, dim3((unsigned)((4 * P + 255) / 256)), dim3(256), 0, main_stream(ctx), d_dst->gm_n,
                       d_dst->gm_first, d_dst->gm_first_af, d_dst->gm_rest, (const char *)d_regions, off[5] - off[4],
                       off[6] - off[4], off[7] - off[4], (int)nparts, P);
    return check_launch(ctx, "gm_merge_kernel");
}

extern "C" int64_t ampli_slice_len(int64_t P, int32_t n_slices)
{
    if (P <= 0 || n_slices < 1) return 0;
    const int64_t per = (P + n_slices - 1) / n_slices;
    return (per + 63) / 64 * 64;
}

extern "C" int32_t ampli_slice_planes(int32_t format) { return slice_planes(format); }

extern "C" int ampli_set_slice_format(ampli_ctx *ctx, int32_t format)
{
    if (!ctx || (format != AMPLI_SLICE_WIDE && format != AMPLI_SLICE_SLIM)) return AMPLI_E_INVALID;
    ctx->slice_fmt = format;
    return AMPLI_OK;
}

extern "C" int ampli_slice_bytes_fmt(int64_t P, int32_t n_slices, int32_t format, size_t *sums_bytes, size_t *gm_bytes, size_t *block_bytes)
{
    const int64_t L = ampli_slice_len(P, n_slices);
    if (L <= 0 || (format != AMPLI_SLICE_WIDE && format != AMPLI_SLICE_SLIM)) return AMPLI_E_INVALID;
    if (sums_bytes) *sums_bytes = (size_t)n_slices * (size_t)slice_planes(format) * (size_t)L * sizeof(double);
    if (gm_bytes) *gm_bytes = (size_t)n_slices * 8 * (size_t)L * sizeof(float);
    if (block_bytes) *block_bytes = slice_block_bytes(L);
    return AMPLI_OK;
}

extern "C" int ampli_slice_bytes(int64_t P, int32_t n_slices, size_t *sums_bytes, size_t *gm_bytes, size_t *block_bytes)
{
    return ampli_slice_bytes_fmt(P, n_slices, AMPLI_SLICE_WIDE, sums_bytes, gm_bytes, block_bytes);
}

extern "C" int ampli_acc_to_slices(ampli_ctx *ctx, const ampli_acc_table *d_acc, int32_t n_slices, double *d_sums, float *d_gm)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!d_acc || !acc_is_bound(d_acc) || n_slices < 1 || !d_sums || !d_gm) return fail(ctx, AMPLI_E_INVALID, "acc_to_slices: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return launch_acc_pack_sliced(ctx, to_ptrs(d_acc), d_acc->P, slice_out(ctx, d_acc->P, n_slices, d_sums, d_gm));
}

extern "C" int ampli_error_finalize_slice(ampli_ctx *ctx, int64_t P, int32_t n_slices, int32_t slice_index,
                                          const double *d_sum_slice, const float *d_gm_recv, float C, int32_t cov, void *d_block)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || n_slices < 1 || slice_index < 0 || slice_index >= n_slices || !d_sum_slice || !d_gm_recv || !d_block || cov < 1)
        return fail(ctx, AMPLI_E_INVALID, "error_finalize_slice: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long L = ampli_slice_len(P, n_slices);
    const size_t G = (size_t)ctx->grp_size, g = (size_t)ctx->grp_index; // [group][planes][L] sums, [n][group][8][L] pairs, [group][block] out
    hipLaunchKernelGGL(error_finalize_slice_kernel, dim3((unsigned)((4 * L + 255) / 256)), dim3(256), 0, main_stream(ctx),
                       d_sum_slice + g * (size_t)slice_planes(ctx->slice_fmt) * (size_t)L, d_gm_recv + g * 8 * (size_t)L, G * 8 * (size_t)L, (int)n_slices, L,
                       (long long)slice_index * L, (long long)P, C, (int)cov, (char *)d_block + g * slice_block_bytes(L), ctx->slice_fmt);
    return check_launch(ctx, "error_finalize_slice_kernel");
}

extern "C" int ampli_error_table_unslice(ampli_ctx *ctx, int64_t P, int32_t n_slices, const void *d_blocks, float *d_rate,
                                         uint8_t *d_code, float *d_thr, float *d_germ_val, uint8_t *d_germ_present,
                                         int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || n_slices < 1 || !d_blocks || !d_rate || !d_code) return fail(ctx, AMPLI_E_INVALID, "error_table_unslice: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long L = ampli_slice_len(P, n_slices);
    hipLaunchKernelGGL(error_table_unslice_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx),
                       (const char *)d_blocks + (size_t)ctx->grp_index * slice_block_bytes(L), (size_t)ctx->grp_size * slice_block_bytes(L),
                       (int)n_slices, L, (long long)P, table_out(d_rate, d_code, d_thr, d_germ_val, d_germ_present, d_flags));
    return check_launch(ctx, "error_table_unslice_kernel");
}

// finalize straight from the merged pieces of a multi-GPU reduction: the all-reduced packed sums and the gathered
// germ-max regions (folded here in rank order); no accumulator table is read or written.
__global__ __launch_bounds__(256) void error_finalize_merged_kernel(const double *__restrict__ pk, const char *__restrict__ regions,
                                                                    const size_t stride, const size_t ofa, const size_t orr,
                                                                    const int nparts, const long long P, const float C,
                                                                    const int cov, FinOut o)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    LaneAcc a;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        a.snt[0][nt] = pk[(0 * 4 + nt) * P + p];
        a.snt[1][nt] = pk[(1 * 4 + nt) * P + p];
        a.srd[0][nt] = (long long)pk[8 * P + (0 * 4 + nt) * P + p];
        a.srd[1][nt] = (long long)pk[8 * P + (1 * 4 + nt) * P + p];
        a.cnt[nt] = (int)pk[16 * P + nt * P + p];
        int n = 0;
        float rest = -INFINITY;
        for (int k = 0; k < nparts; ++k) { // ordered fold of the shards' germ-max triples (as gm_merge_kernel)
            const char *b = regions + (size_t)k * stride;
            const long long i = nt * P + p;
            const int rn = ((const int *)b)[i];
            if (rn == 0) continue;
            const float fa = ((const float *)(b + ofa))[i], rr = ((const float *)(b + orr))[i];
            if (n == 0) rest = rr;
            else { if (rest <= fa) rest = fa; if (rest <= rr) rest = rr; }
            n += rn;
        }
        a.gm_n[nt] = n; a.gm_rest[nt] = rest; a.gm_first[nt] = 0; a.gm_first_af[nt] = 0.0f;
    }
    a.nrec = (int)pk[20 * P + p];
    finalize_lane(a, P, p, C, cov, o);
}

extern "C" int ampli_error_finalize_merged(ampli_ctx *ctx, int64_t P, const double *d_packed, const void *d_gm_regions,
                                           int32_t nparts, float C, int32_t cov, float *d_rate, uint8_t *d_code, float *d_thr,
                                           float *d_germ_val, uint8_t *d_germ_present, int32_t *d_flags)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || !d_packed || !d_gm_regions || nparts < 1 || !d_rate || !d_code || cov < 1)
        return fail(ctx, AMPLI_E_INVALID, "error_finalize_merged: bad argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t off[9];
    acc_offsets(P, off);
    hipLaunchKernelGGL(error_finalize_merged_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), d_packed,
                       (const char *)d_gm_regions, off[5] - off[4], off[6] - off[4], off[7] - off[4], (int)nparts, (long long)P, C,
                       (int)cov, table_out(d_rate, d_code, d_thr, d_germ_val, d_germ_present, d_flags));
    return check_launch(ctx, "error_finalize_merged_kernel");
}
