// amplisolve_amd/csrc/ampli_aux.hip -- auxiliary and synthetic: the scorer and the text round trip on lists (what the tests check
// ampli_math.h through), synthetic panels (ampli_synth.h).  Nothing here is on the path.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"
#include "ampli_synth.h"

__global__ void score_dense_batch_kernel(const int *k, const int *rd, const float *err, const long long n, double *q, const double *lgtab)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = ampli_poisson_score_dense(k[i], rd[i], err[i], lgtab, AMPLI_LGTAB);
}

// the drain's scorer on a list, one lane per item: what drain_body evaluates for one strand of a queued item with 0 < m < k
// (ampli_host_drain_score_batch's semantics: no test of that condition here either)
__global__ void drain_score_batch_kernel(const int *k, const int *rd, const float *err, const long long n, double *q, double *pv, const double *lgtab)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double m = (double)rd[i] * err[i]; // VC:3864: double * float
    const double p = ampli_drain_p(k[i], m, lgtab, AMPLI_LGTAB);
    if (pv) pv[i] = p;
    if (q) q[i] = ampli_q_from_p(p);
}

__global__ void score_batch_kernel(const int *k, const int *rd, const float *err, const long long n, double *q, double *pv)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (q) q[i] = ampli_poisson_score(k[i], rd[i], err[i]);
    if (pv) pv[i] = err[i] == -1 ? -1.0 : ampli_poisson_p(k[i], rd[i], err[i]);
}

__global__ void roundtrip_batch_kernel(const float *in, const long long n, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = ampli_text_roundtrip(in[i]);
}

__global__ void synth_fill_kernel(int4 *recs, const long long P, const int n_samples, const int first_sample,
                                  const unsigned long long seed, const int depth, const int tumour)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= P || s >= n_samples) return;
    int rec[8];
    ampli_synth_record(seed, (uint64_t)p, (uint64_t)(first_sample + s), depth, tumour, rec);
    const size_t o = ((size_t)s * P + p) * 2;
    recs[o] = make_int4(rec[0], rec[1], rec[2], rec[3]);
    recs[o + 1] = make_int4(rec[4], rec[5], rec[6], rec[7]);
}

__global__ void synth_ref_kernel(unsigned char *ref, const long long P, const unsigned long long seed)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) ref[p] = (unsigned char)ampli_synth_ref_base(seed, (uint64_t)p);
}

extern "C" int ampli_score_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err, int64_t n,
                                 double *d_q, double *d_p)
{
    if (!ctx || !d_k || !d_rd || !d_err || n <= 0) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(score_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, main_stream(ctx), d_k, d_rd, d_err,
                       (long long)n, d_q, d_p);
    return check_launch(ctx, "score_batch_kernel");
}

extern "C" int ampli_score_dense_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err, int64_t n, double *d_q)
{
    if (!ctx || !d_k || !d_rd || !d_err || !d_q || n <= 0) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
    hipLaunchKernelGGL(score_dense_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, main_stream(ctx), d_k, d_rd, d_err,
                       (long long)n, d_q, (const double *)ctx->d_lgtab);
    return check_launch(ctx, "score_dense_batch_kernel");
}

extern "C" int ampli_drain_score_batch(ampli_ctx *ctx, const int32_t *d_k, const int32_t *d_rd, const float *d_err, int64_t n, double *d_q,
                                       double *d_p)
{
    if (!ctx || !d_k || !d_rd || !d_err || n <= 0) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rcl = ensure_lgtab(ctx); if (rcl) return rcl; }
    hipLaunchKernelGGL(drain_score_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, main_stream(ctx), d_k, d_rd, d_err,
                       (long long)n, d_q, d_p, (const double *)ctx->d_lgtab);
    return check_launch(ctx, "drain_score_batch_kernel");
}

extern "C" int ampli_roundtrip_batch(ampli_ctx *ctx, const float *d_in, int64_t n, float *d_out)
{
    if (!ctx || !d_in || !d_out || n <= 0) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(roundtrip_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, main_stream(ctx), d_in, (long long)n, d_out);
    return check_launch(ctx, "roundtrip_batch_kernel");
}

extern "C" int ampli_synth_fill(ampli_ctx *ctx, int32_t *d_recs, int64_t P, int32_t n_samples, int32_t first_sample,
                                uint64_t seed, int32_t depth, int32_t tumour)
{
    if (!ctx || !d_recs || P <= 0 || n_samples <= 0 || depth <= 0) return AMPLI_E_INVALID;
    if (n_samples > 65535) return fail(ctx, AMPLI_E_RANGE, "synth_fill: more than 65535 samples in one call (grid limit); fill the panel in parts"); // n_samples = gridDim.y
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(synth_fill_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)n_samples), dim3(256), 0, main_stream(ctx),
                       (int4 *)d_recs, (long long)P, (int)n_samples, (int)first_sample, (unsigned long long)seed, (int)depth, (int)tumour);
    return check_launch(ctx, "synth_fill_kernel");
}

extern "C" int ampli_synth_ref(ampli_ctx *ctx, uint8_t *d_ref_code, int64_t P, uint64_t seed)
{
    if (!ctx || !d_ref_code || P <= 0) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(synth_ref_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, main_stream(ctx), d_ref_code, (long long)P,
                       (unsigned long long)seed);
    return check_launch(ctx, "synth_ref_kernel");
}
