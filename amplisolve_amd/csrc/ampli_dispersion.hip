// amplisolve_amd/csrc/ampli_dispersion.hip -- dispersion of the panel of normals and per-normal outlier scores.
//
// dispersion_stream_kernel + dispersion_sample_reduce_kernel (ampli_dispersion_records) and dispersion_finalize_kernel
// (ampli_dispersion_finalize).  The qualifying set of a cell is the one the threshold sums count: the gate is error_reduce's and
// leave-one-out's (thr_gate, ampli_device.h), the records come through rec_counts.  The arithmetic of one finalized cell is
// ampli_dispersion_cell (ampli_math.h), which the host library exports too.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// what a lane keeps of its position's eight cells (strand-major: cell c = st * 4 + nt)
struct DispCells {
    double r[8];    // pooled rate K / D of an OK cell, else 0
    double rinv[8]; // 1 / r = D / K
    double dinv[8]; // 1 / D
    unsigned ok;    // bit c: the cell is OK (n >= 2 and K >= 2)
};

// one record's terms: X2 and sum 1/d of the lane's cells, and the record's share of its sample's sums.  Two divisions per record,
// 1 / FW and 1 / BW, shared by the four bases.
__device__ __forceinline__ void disp_visit(const RecCounts &a, const bool on, const int cov, const DispCells &t, double x2[8], double ri[8],
                                           double &row_x2, double &row_ex, int &row_terms)
{
    const bool covok = on && a.present && a.FW >= cov && a.BW >= cov;
    const unsigned qual = thr_gate(a.fw, a.bw, a.FW, a.BW, covok, a.own_rd || a.RD >= AMPLI_COUNT_LIMIT); // big: as visit_record
    const unsigned m = (qual | (qual << 4)) & t.ok;
    if (m) { // a qualifying record has FW, BW >= cov >= 1
        const double d_fw = (double)a.FW, d_bw = (double)a.BW;
        const double i_fw = 1.0 / d_fw, i_bw = 1.0 / d_bw;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const int c = st * 4 + nt;
                if ((m >> c) & 1u) {
                    const double k = (double)(st ? a.bw[nt] : a.fw[nt]), d = st ? d_bw : d_fw, id = st ? i_bw : i_fw;
                    const double df = k - t.r[c] * d;
                    const double term = df * df * t.rinv[c] * id; // (k - r d)^2 / (r d)
                    x2[c] += term;
                    ri[c] += id;
                    row_x2 += term;
                    row_ex += 1.0 - d * t.dinv[c];
                    row_terms += 1;
                }
            }
        }
    }
}

// dispersion_stream_kernel<LAY,IRR>: one pass over a resident chunk.  A workgroup = 4 waves over one 64-position tile, one lane per
// position, wave w taking rows w, w + 4, ... (loo_stream_kernel's shape).  A lane loads its position's K, D and n once and forms
// r, 1 / r and 1 / D once per cell; every record then costs two divisions.  16 fp64 accumulators per lane (X2 and sum 1/d per cell)
// are combined over the waves in LDS in wave order and stored or added to the planes: no floating-point atomic anywhere, the result
// depends on the inputs and the chunking alone.  The per-sample sums: every (wave, row) reduces its lanes with a fixed butterfly and
// stores ONE partial per (row, tile) into the workspace (every slot is written: nothing to clear); dispersion_sample_reduce_kernel
// adds them in a fixed order.  The next row's primary record is loaded before the current row's arithmetic.
template <int LAY, bool IRR>
__global__ __launch_bounds__(256) void dispersion_stream_kernel(
    const RecView rv, const long long P, const long long E, const unsigned *__restrict__ dup_off, const int n,
    const double *__restrict__ snt, const long long *__restrict__ srd, const int *__restrict__ cnt, const int cov,
    double *__restrict__ x2_out, double *__restrict__ rinv_out, const int accumulate, const long long tiles,
    double *__restrict__ part_x2, double *__restrict__ part_ex, long long *__restrict__ part_terms)
{
    __shared__ double lds[3][16][64]; // waves 1..3: X2[8] | sum 1/d [8] per lane
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p_raw = (long long)blockIdx.x * 64 + lane;
    const bool valid = p_raw < P;
    const long long p = valid ? p_raw : P - 1;
    DispCells t;
    t.ok = 0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nq = cnt[nt * P + p];
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int c = st * 4 + nt;
            const double K = snt[c * P + p];         // C = 0: the exact integer sum of the alternative counts
            const double D = (double)srd[c * P + p]; // < 2^53: exact
            const bool ok = nq >= 2 && K >= 2.0;     // then D >= K >= 2
            t.ok |= ok ? 1u << c : 0u;
            t.r[c] = ok ? K / D : 0.0;
            t.rinv[c] = ok ? D / K : 0.0;
            t.dinv[c] = ok ? 1.0 / D : 0.0;
        }
    }
    const long long e0 = E > 0 ? (long long)dup_off[p] : 0;
    const int n_ext = E > 0 && valid ? (int)(dup_off[p + 1] - dup_off[p]) : 0;
    double x2[8], ri[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { x2[c] = 0.0; ri[c] = 0.0; }
    RecCounts cur = rec_counts<LAY, IRR>(rv, P, E, wave < n ? wave : 0, p);
    for (int s = wave; s < n; s += 4) {
        const RecCounts nxt = rec_counts<LAY, IRR>(rv, P, E, s + 4 < n ? s + 4 : s, p); // in flight during this row's arithmetic
        double row_x2 = 0.0, row_ex = 0.0;
        int row_terms = 0;
        disp_visit(cur, valid, cov, t, x2, ri, row_x2, row_ex, row_terms);
        for (int j = 0; j < n_ext; ++j) // the extras of p (record P + e0 + j): a lane's own count, nothing in here is wave-wide
            disp_visit(rec_counts<LAY, IRR>(rv, P, E, s, P + e0 + j), true, cov, t, x2, ri, row_x2, row_ex, row_terms);
        if (part_x2) { // wave-uniform
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                row_x2 += __shfl_xor(row_x2, off);
                row_ex += __shfl_xor(row_ex, off);
                row_terms += __shfl_xor(row_terms, off);
            }
            if (lane == 0) {
                const size_t o = (size_t)s * (size_t)tiles + blockIdx.x;
                part_x2[o] = row_x2;
                part_ex[o] = row_ex;
                part_terms[o] = row_terms;
            }
        }
        cur = nxt;
    }
    if (wave) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            lds[wave - 1][c][lane] = x2[c];
            lds[wave - 1][8 + c][lane] = ri[c];
        }
    }
    __syncthreads();
    if (wave == 0 && valid) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double sx = ((x2[c] + lds[0][c][lane]) + lds[1][c][lane]) + lds[2][c][lane];
            const double sr = ((ri[c] + lds[0][8 + c][lane]) + lds[1][8 + c][lane]) + lds[2][8 + c][lane];
            const long long o = c * P + p;
            x2_out[o] = accumulate ? x2_out[o] + sx : sx;
            rinv_out[o] = accumulate ? rinv_out[o] + sr : sr;
        }
    }
}

// one wave per sample: lane l adds the partials of tiles l, l + 64, ... in that order, then the fixed butterfly
__global__ __launch_bounds__(64) void dispersion_sample_reduce_kernel(
    const double *__restrict__ part_x2, const double *__restrict__ part_ex, const long long *__restrict__ part_terms, const long long tiles,
    double *__restrict__ sample_x2, double *__restrict__ sample_expect, long long *__restrict__ sample_terms)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    double a = 0.0, b = 0.0;
    long long m = 0;
    for (long long tile = lane; tile < tiles; tile += 64) {
        const size_t o = (size_t)s * (size_t)tiles + (size_t)tile;
        a += part_x2[o];
        b += part_ex[o];
        m += part_terms[o];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        m += __shfl_xor(m, off);
    }
    if (lane == 0) {
        sample_x2[s] = a;
        sample_expect[s] = b;
        sample_terms[s] = m;
    }
}

// one lane per position, eight cells each (ampli_dispersion_cell); the four counters take one integer atomic per wave and counter
__global__ __launch_bounds__(256) void dispersion_finalize_kernel(
    const long long P, const double *__restrict__ snt, const long long *__restrict__ srd, const int *__restrict__ cnt,
    const double *__restrict__ x2, const double *__restrict__ rinv, const double z_cutoff, double *__restrict__ z_out, float *__restrict__ phi_out,
    unsigned char *__restrict__ status_out, unsigned long long *__restrict__ counts)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    int n_ok = 0, n_few = 0, n_high = 0;
    if (p < P) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int nq = cnt[nt * P + p];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const long long o = (st * 4 + nt) * P + p;
                double z;
                float phi;
                const unsigned char c = ampli_dispersion_cell(nq, snt[o], (double)srd[o], x2[o], rinv[o], z_cutoff, &z, &phi);
                z_out[o] = z;
                phi_out[o] = phi;
                status_out[o] = c;
                n_few += c == AMPLI_DISPERSION_FEW ? 1 : 0;
                n_ok += c != AMPLI_DISPERSION_FEW ? 1 : 0;
                n_high += c & AMPLI_DISPERSION_HIGH ? 1 : 0;
            }
        }
    }
    int n_pos = n_high ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_ok += __shfl_xor(n_ok, off);
        n_few += __shfl_xor(n_few, off);
        n_high += __shfl_xor(n_high, off);
        n_pos += __shfl_xor(n_pos, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_ok) atomicAdd(&counts[0], (unsigned long long)n_ok);
        if (n_few) atomicAdd(&counts[1], (unsigned long long)n_few);
        if (n_high) atomicAdd(&counts[2], (unsigned long long)n_high);
        if (n_pos) atomicAdd(&counts[3], (unsigned long long)n_pos);
    }
}

extern "C" int ampli_dispersion_records(ampli_ctx *ctx, const ampli_records *recs, int64_t P, const ampli_acc_table *d_acc0, int32_t cov,
                                        double *d_x2, double *d_rinv, int32_t accumulate, double *d_sample_x2, double *d_sample_expect,
                                        int64_t *d_sample_terms)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort co;
    { int rc = cohort_from_records(ctx, recs, P, co); if (rc) return rc; }
    if (P <= 0 || cov < 1 || !d_x2 || !d_rinv || (((uintptr_t)d_x2 | (uintptr_t)d_rinv) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "dispersion_records: bad argument (P > 0, coverage_cutoff >= 1, 8-byte aligned x2 and rinv planes)");
    if (!acc_is_bound(d_acc0) || d_acc0->P != P) return fail(ctx, AMPLI_E_INVALID, "dispersion_records: d_acc0 must be an ampli_acc_bind table of P positions");
    const int n_null = (d_sample_x2 ? 0 : 1) + (d_sample_expect ? 0 : 1) + (d_sample_terms ? 0 : 1);
    if ((n_null != 0 && n_null != 3) || (((uintptr_t)d_sample_x2 | (uintptr_t)d_sample_expect | (uintptr_t)d_sample_terms) & 7) != 0)
        return fail(ctx, AMPLI_E_INVALID, "dispersion_records: the three sample arrays are given together or not at all, 8-byte aligned");
    { int rc = check_records(ctx, co, "dispersion_records", co.dup_off, "dup_off"); if (rc) return rc; }
    const long long E = co.E;
    const int n = co.n;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long tiles = (P + 63) / 64;
    if (tiles > 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "dispersion_records: P must be below 2^37");
    double *part_x2 = nullptr, *part_ex = nullptr;
    long long *part_terms = nullptr;
    if (d_sample_x2) { // [n][tiles] partials of the three sums: the context's workspace, like the partial tables of error_reduce
        const size_t cells = (size_t)n * (size_t)tiles;
        { int rc = ensure_ws(ctx, cells * 24); if (rc) return rc; }
        part_x2 = (double *)ctx->ws;
        part_ex = part_x2 + cells;
        part_terms = (long long *)(part_ex + cells);
    }
    const AccPtrs acc = to_ptrs(d_acc0);
    with_layout(co.layout, [&](auto L) {
        with_bool(co.rv.rd || co.rv.rd_ext, [&](auto IRR) {
            hipLaunchKernelGGL((dispersion_stream_kernel<L, IRR>), dim3((unsigned)tiles), dim3(256), 0, st, co.rv, (long long)P, E, co.dup_off, n,
                               (const double *)acc.snt, (const long long *)acc.srd, (const int *)acc.cnt, (int)cov, d_x2, d_rinv, accumulate ? 1 : 0,
                               tiles, part_x2, part_ex, part_terms);
        });
    });
    { int rc = check_launch(ctx, "dispersion_stream_kernel"); if (rc) return rc; }
    if (!d_sample_x2) return AMPLI_OK;
    hipLaunchKernelGGL(dispersion_sample_reduce_kernel, dim3((unsigned)n), dim3(64), 0, st, (const double *)part_x2, (const double *)part_ex,
                       (const long long *)part_terms, tiles, d_sample_x2, d_sample_expect, (long long *)d_sample_terms);
    return check_launch(ctx, "dispersion_sample_reduce_kernel");
}

extern "C" int ampli_dispersion_finalize(ampli_ctx *ctx, int64_t P, const ampli_acc_table *d_acc0, const double *d_x2, const double *d_rinv,
                                         double z_cutoff, double *d_z, float *d_phi, uint8_t *d_status, int64_t *d_counts)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (P <= 0 || !d_x2 || !d_rinv || !d_z || !d_phi || !d_status || !d_counts || z_cutoff != z_cutoff ||
        (((uintptr_t)d_x2 | (uintptr_t)d_rinv | (uintptr_t)d_z | (uintptr_t)d_counts) & 7) != 0 || ((uintptr_t)d_phi & 3) != 0)
        return fail(ctx, AMPLI_E_INVALID, "dispersion_finalize: bad argument (P > 0, every plane and the counters given and aligned, z_cutoff a number)");
    if (!acc_is_bound(d_acc0) || d_acc0->P != P) return fail(ctx, AMPLI_E_INVALID, "dispersion_finalize: d_acc0 must be an ampli_acc_bind table of P positions");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const AccPtrs acc = to_ptrs(d_acc0);
    hipLaunchKernelGGL(dispersion_finalize_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (long long)P, (const double *)acc.snt,
                       (const long long *)acc.srd, (const int *)acc.cnt, d_x2, d_rinv, z_cutoff, d_z, d_phi, d_status, (unsigned long long *)d_counts);
    return check_launch(ctx, "dispersion_finalize_kernel");
}
