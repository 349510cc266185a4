// amplisolve_amd/csrc/ampli_paired.hip -- paired comparison: the exact conditional test of two count files of one patient
// at every (pair, position, alternative base), per read strand.
//
// paired_score_kernel (ampli_pair_score_records) takes row a of chunk A and row b of chunk B for every listed pair and scores the
// 2 x 2 table (alternative reads, other reads) x (file a, file b) of every strand cell under the hypergeometric law
// (ampli_pair_score_begin / ampli_hyper_step, ampli_math.h).  The host library exports the same text.
#include <hip/hip_runtime.h>

#include "../../include/amplisolve_hip.h"
#include "ampli_device.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// the count of cell c = base * 2 + strand, for a c that differs from lane to lane, as a chain of selects on the decoded record: the
// counts stay in the registers they were decoded into (no array, so nothing for the compiler to move to scratch or LDS)
__device__ __forceinline__ int pc_pick(const int4 &f, const int4 &b, const int c)
{
    int v = f.x;
    v = c == 1 ? b.x : v;
    v = c == 2 ? f.y : v;
    v = c == 3 ? b.y : v;
    v = c == 4 ? f.z : v;
    v = c == 5 ? b.z : v;
    v = c == 6 ? f.w : v;
    v = c == 7 ? b.w : v;
    return v;
}

// paired_score_kernel<LAY>: blockIdx.x = 64-position tile, a lane a position; wave w of workgroup blockIdx.y owns pair pair_base +
// blockIdx.y * 4 + w.  A lane at or beyond P and a pair at or beyond n_pairs load and store nothing.  A pair with a row index outside
// its chunk stores eight AMPLI_PAIR_NA per lane and loads no record.  A lane whose (pair, position) is not evaluated stores eight NA;
// every other lane stores NA for the reference base and walks its six cells (c = base * 2 + strand, the order of d_s) in ONE loop: a
// turn of the loop starts the cell's tail if that is due, runs one ampli_hyper_step of it if it is live, and stores the score and
// moves on once it is not -- lanes in different cells and different stages share every turn.  No LDS, no barrier, no atomics: the
// same inputs give the same bytes.
template <int LAY>
__global__ __launch_bounds__(256) void paired_score_kernel(const RecView ra, const int n_a, const RecView rb, const int n_b, const long long P,
                                                           const int *__restrict__ pairs, const int n_pairs, const int pair_base,
                                                           const unsigned char *__restrict__ ref_code, const int cutoff, float *__restrict__ s_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long p = (long long)blockIdx.x * 64 + lane;
    const int q = pair_base + (int)blockIdx.y * 4 + wave;
    if (p >= P || q >= n_pairs) return;
    const int row_a = pairs[2 * (size_t)q], row_b = pairs[2 * (size_t)q + 1];
    float *__restrict__ out = s_out + ((size_t)q * (size_t)P + (size_t)p) * 8;
    const float4 na = make_float4(AMPLI_PAIR_NA, AMPLI_PAIR_NA, AMPLI_PAIR_NA, AMPLI_PAIR_NA);
    if ((unsigned)row_a >= (unsigned)n_a || (unsigned)row_b >= (unsigned)n_b) { // checked before any load of a record
        ((float4 *)out)[0] = na;
        ((float4 *)out)[1] = na;
        return;
    }
    const RawRec<LAY> raw_a = rec_load_at<LAY>(ra.base + ((size_t)row_a * (size_t)ra.row_stride + (size_t)p) * rec_bytes(LAY));
    const RawRec<LAY> raw_b = rec_load_at<LAY>(rb.base + ((size_t)row_b * (size_t)rb.row_stride + (size_t)p) * rec_bytes(LAY));
    int4 fa, ba, fb, bb;
    rec_decode<LAY>(raw_a, fa, ba);
    rec_decode<LAY>(raw_b, fb, bb);
    const bool present = fa.x != AMPLI_ABSENT && fb.x != AMPLI_ABSENT;
    // a strand's depth of an int32 record may pass 2^31: 64-bit sums
    const long long Da0 = (long long)fa.x + fa.y + fa.z + fa.w, Da1 = (long long)ba.x + ba.y + ba.z + ba.w;
    const long long Db0 = (long long)fb.x + fb.y + fb.z + fb.w, Db1 = (long long)bb.x + bb.y + bb.z + bb.w;
    const unsigned ref = ref_code[p];
    if (!(present && Da0 >= cutoff && Da1 >= cutoff && Db0 >= cutoff && Db1 >= cutoff && ref <= 3u)) {
        ((float4 *)out)[0] = na;
        ((float4 *)out)[1] = na;
        return;
    }
    out[2 * ref] = AMPLI_PAIR_NA;
    out[2 * ref + 1] = AMPLI_PAIR_NA;
    ampli_hyper_sum s;
    s.live = 0;
    int c = ref == 0u ? 2 : 0;
    int sign = 0;
    bool start = true;
    float v = 0.0f;
    while (c < 8) {
        if (start) {
            const int st = c & 1;
            sign = ampli_pair_score_begin(&s, pc_pick(fa, ba, c), st ? Da1 : Da0, pc_pick(fb, bb, c), st ? Db1 : Db0, &v);
            start = false;
        }
        if (s.live) {
            ampli_hyper_step(&s);
            if (!s.live) v = ampli_pair_s_from_p(s.res, sign);
        }
        if (!s.live) {
            out[c] = v;
            ++c;
            if ((unsigned)(c >> 1) == ref) c += 2;
            start = true;
        }
    }
}

// ==== C ABI ==============================================================================================================================

extern "C" int ampli_pair_score_records(ampli_ctx *ctx, const ampli_records *recs_a, const ampli_records *recs_b, int64_t P, const int32_t *d_pairs,
                                        int32_t n_pairs, const uint8_t *d_ref_code, int32_t depth_cutoff, float *d_s)
{
    if (!ctx) return AMPLI_E_INVALID;
    DevCohort ca, cb;
    { int rc = cohort_from_records(ctx, recs_a, P, ca); if (rc) return rc; }
    { int rc = cohort_from_records(ctx, recs_b, P, cb); if (rc) return rc; }
    if (P <= 0 || n_pairs < 1 || depth_cutoff < 0 || !d_pairs || !d_ref_code || !d_s || ((uintptr_t)d_pairs & 3) != 0 || ((uintptr_t)d_s & 15) != 0)
        return fail(ctx, AMPLI_E_INVALID,
                    "pair_score_records: bad argument (P > 0, n_pairs >= 1, depth_cutoff >= 0, 4-byte aligned d_pairs, d_ref_code, 16-byte aligned d_s)");
    { int rc = check_records(ctx, ca, "pair_score_records (a)", nullptr, nullptr); if (rc) return rc; }
    { int rc = check_records(ctx, cb, "pair_score_records (b)", nullptr, nullptr); if (rc) return rc; }
    if (ca.layout != cb.layout) return fail(ctx, AMPLI_E_INVALID, "pair_score_records: the two chunks must have the same record layout");
    if (P >= 0x7FFFFFFFll) return fail(ctx, AMPLI_E_RANGE, "pair_score_records: P must be below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = main_stream(ctx);
    const long long tiles = (P + 63) / 64, groups = ((long long)n_pairs + 3) / 4;
    constexpr long long MAX_Y = 65535; // a launch takes at most this many pair groups
    for (long long g0 = 0; g0 < groups; g0 += MAX_Y) {
        const dim3 grid((unsigned)tiles, (unsigned)(groups - g0 < MAX_Y ? groups - g0 : MAX_Y));
        with_layout(ca.layout, [&](auto L) {
            hipLaunchKernelGGL((paired_score_kernel<L>), grid, dim3(256), 0, st, ca.rv, ca.n, cb.rv, cb.n, (long long)P, (const int *)d_pairs, (int)n_pairs,
                               (int)(g0 * 4), d_ref_code, (int)depth_cutoff, d_s);
        });
    }
    return check_launch(ctx, "paired_score_kernel");
}
