// amplisolve_amd/csrc/ampli_device.h -- what more than one of the kernel translation units of libamplisolve_hip.so needs, and nothing
// else: the record types and their decode, the accumulator state of one position with its merge, load, store and finalize, the item
// and hand-over of poisson_call's queue with the drain both drains run, the launch dispatch, and the host helpers one unit defines
// for the others (declared at the end).  Everything on the device side is __forceinline__: a kernel is compiled whole in the unit
// that defines and launches it (ampli_kernels.hip heads the map of the units).  bench.py's kernel_source_sha() covers
// ampli_kernels.hip and ampli_math.h, not this header.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/amplisolve_hip.h"
#include "ampli_internal.h"
#include "ampli_math.h"

// ==== records: layouts, decode, the cohort a kernel reads ===============================================================================

// streaming 16-byte load of record data (default cache policy: non-temporal loads measured 4-10 % slower)
__device__ __forceinline__ int4 ld_stream(const int4 *p) { return *p; }

// Record layouts (include/amplisolve_hip.h), template parameter LAY:
//   AMPLI_RECORDS_I32  8 x int32, two int4 per record                      (absent: INT32_MIN in field 0)
//   AMPLI_RECORDS_U16  8 x uint16, one int4 per record                     (absent: 0xFFFF)
//   AMPLI_RECORDS_U24  8 x 24-bit little-endian, 24 bytes = three 8-byte loads per record (absent: 0xFFFFFF)
// A raw record is what a lane keeps in flight; rec_decode widens it to the {forward int4, reverse int4} pair every
// visit function takes.
template <int LAY> struct RawRec { int4 a, b; };
template <> struct RawRec<AMPLI_RECORDS_U24> { uint2 a, b, c; };

// A cohort (or one chunk of a streamed cohort) on the device.  Record r < P of sample s lives at
// base + (s*row_stride + r) * record_bytes; extra occurrence e (record P + e) at ext + (s*ext_stride + e) * record_bytes.
// The dense interchange layout [n][P+E] is row_stride = ext_stride = P + E, ext = base + P records; a padded row stride
// (power-of-two panels) or a separately uploaded extras array are the same kernels with other numbers.
struct RecView {
    const char *base;
    long long row_stride; // records
    const char *ext;
    long long ext_stride; // records
    // optional RD column of the lines whose RD differs from A+C+G+T (EE:1178-1181, VC:762-765): rd [n][P], rd_ext [n][E],
    // AMPLI_ABSENT where the line is regular; NULL when every line of the cohort is
    const int *rd;
    const int *rd_ext;
};

__host__ __device__ constexpr int rec_bytes(const int layout)
{
    return layout == AMPLI_RECORDS_U24 ? 24 : (layout == AMPLI_RECORDS_U16 ? 16 : 32);
}

template <int LAY> __device__ __forceinline__ RawRec<LAY> rec_load_at(const char *__restrict__ q)
{
    RawRec<LAY> r;
    if constexpr (LAY == AMPLI_RECORDS_U24) {
        const uint2 *__restrict__ u = (const uint2 *)q;
        r.a = u[0]; r.b = u[1]; r.c = u[2];
    } else if constexpr (LAY == AMPLI_RECORDS_U16) {
        r.a = ld_stream((const int4 *)q); r.b = r.a;
    } else {
        r.a = ld_stream((const int4 *)q); r.b = ld_stream((const int4 *)q + 1);
    }
    return r;
}

// four 24-bit fields out of three dwords
__device__ __forceinline__ int4 unpack24(const unsigned w0, const unsigned w1, const unsigned w2)
{
    return make_int4((int)(w0 & 0xFFFFFFu), (int)(__builtin_amdgcn_alignbit(w1, w0, 24) & 0xFFFFFFu),
                     (int)(__builtin_amdgcn_alignbit(w2, w1, 16) & 0xFFFFFFu), (int)(w2 >> 8));
}

template <int LAY> __device__ __forceinline__ void rec_decode(const RawRec<LAY> &r, int4 &fw, int4 &bw)
{
    if constexpr (LAY == AMPLI_RECORDS_U24) {
        fw = unpack24(r.a.x, r.a.y, r.b.x);
        bw = unpack24(r.b.y, r.c.x, r.c.y);
        if (fw.x == 0xFFFFFF) fw.x = AMPLI_ABSENT;
    } else if constexpr (LAY == AMPLI_RECORDS_U16) {
        fw = make_int4(r.a.x & 0xFFFF, (int)((unsigned)r.a.x >> 16), r.a.y & 0xFFFF, (int)((unsigned)r.a.y >> 16));
        bw = make_int4(r.a.z & 0xFFFF, (int)((unsigned)r.a.z >> 16), r.a.w & 0xFFFF, (int)((unsigned)r.a.w >> 16));
        if (fw.x == 0xFFFF) fw.x = AMPLI_ABSENT;
    } else {
        fw = r.a; bw = r.b;
    }
}

// One record of sample s as a visit reads it -- record r < P, or extra occurrence r - P: the strands' counts, their sums FW and BW
// (EE:1175-1176, VC:760-761) and RD, which is FW + BW unless the line carries an RD column of its own (EE:1178-1181, VC:762-765:
// own_rd; IRR = the cohort may hold such lines).  The kernels bench.py times (error reduce, poisson_stream_kernel) keep their own text.
struct RecCounts {
    int fw[4], bw[4];
    int FW, BW, RD;
    bool present, own_rd;
};

template <int LAY, bool IRR>
__device__ __forceinline__ RecCounts rec_counts(const RecView &rv, const long long P, const long long E, const int s, const long long r)
{
    const RawRec<LAY> raw = r < P ? rec_load_at<LAY>(rv.base + ((size_t)s * (size_t)rv.row_stride + (size_t)r) * rec_bytes(LAY))
                                  : rec_load_at<LAY>(rv.ext + ((size_t)s * (size_t)rv.ext_stride + (size_t)(r - P)) * rec_bytes(LAY));
    int4 r0, r1;
    rec_decode<LAY>(raw, r0, r1);
    RecCounts o;
    o.fw[0] = r0.x; o.fw[1] = r0.y; o.fw[2] = r0.z; o.fw[3] = r0.w;
    o.bw[0] = r1.x; o.bw[1] = r1.y; o.bw[2] = r1.z; o.bw[3] = r1.w;
    o.FW = r0.x + r0.y + r0.z + r0.w;
    o.BW = r1.x + r1.y + r1.z + r1.w;
    o.RD = o.FW + o.BW;
    o.own_rd = false;
    if (IRR) {
        const int *rdp = r < P ? rv.rd : rv.rd_ext;
        const int rdc = rdp ? rdp[r < P ? (size_t)s * P + r : (size_t)s * E + (r - P)] : AMPLI_ABSENT;
        if (rdc != AMPLI_ABSENT) { o.RD = rdc; o.own_rd = true; }
    }
    o.present = r0.x != AMPLI_ABSENT;
    return o;
}

// what the kernels read: a cohort (or one chunk of a streamed one) resident on the device
struct DevCohort {
    RecView rv;
    int layout;   // AMPLI_RECORDS_*
    int n;        // samples
    long long E;  // extra-occurrence slots per sample
    const unsigned *dup_off; // [P+1]: extras of position p are e in [dup_off[p], dup_off[p+1])   (error_reduce)
    const unsigned *ext_pos; // [E]: position of extra e                                          (poisson_call)
};

// Launch dispatch: f(constant) for the run-time value, inside a generic lambda the template argument of a kernel.
template <int V> using Const = std::integral_constant<int, V>;
template <class F> static void with_layout(const int layout, F &&f) // every record layout
{
    if (layout == AMPLI_RECORDS_U24) f(Const<AMPLI_RECORDS_U24>{});
    else if (layout == AMPLI_RECORDS_U16) f(Const<AMPLI_RECORDS_U16>{});
    else f(Const<AMPLI_RECORDS_I32>{});
}
template <class F> static void with_bool(const bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// ==== accumulator state: one position's sums and Germ_Max state, the table's planes, what a finalize writes ============================

// ---------------------------------------------------------------------------
// per-lane accumulator for one position (all 4 nucleotides)
// ---------------------------------------------------------------------------
struct LaneAcc {
    double snt[2][4];
    long long srd[2][4];
    int cnt[4];
    int nrec;
    int gm_n[4];
    int gm_first[4];
    float gm_first_af[4];
    float gm_rest[4];
};

// The threshold half of the record gate (EE:1595 + clones): bit nt set when the record's counts of nucleotide nt go into the
// threshold sums -- covered on both strands and AF <= 0.05 on each strand, as an integer bound (ampli_math.h), or the literal fp
// gates when `big` (an irregular line or RD >= 2^24: never for real panels).  visit_record and the leave-one-out kernel both
// gate through here, so the table of the whole cohort and the S-1 tables subtracted from it cannot drift apart.
__device__ __forceinline__ unsigned thr_gate(const int fw[4], const int bw[4], const int FW, const int BW, const bool covok, const bool big)
{
    const int lim_fw = ampli_af_limit(FW), lim_bw = ampli_af_limit(BW);
    unsigned q = 0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        bool g_fw = fw[nt] <= lim_fw, g_bw = bw[nt] <= lim_bw;
        if (big) {
            g_fw = ampli_af_gate_fp(fw[nt], FW);
            g_bw = ampli_af_gate_fp(bw[nt], BW);
        }
        q |= (covok && g_fw && g_bw) ? 1u << nt : 0u;
    }
    return q;
}

// L = L (+) R, L covering the earlier samples
__device__ __forceinline__ void lane_acc_merge(LaneAcc &L, const LaneAcc &R)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        L.snt[0][nt] += R.snt[0][nt]; L.snt[1][nt] += R.snt[1][nt];
        L.srd[0][nt] += R.srd[0][nt]; L.srd[1][nt] += R.srd[1][nt];
        L.cnt[nt] += R.cnt[nt];
        if (R.gm_n[nt] != 0) {
            if (L.gm_n[nt] == 0) {
                L.gm_first[nt] = R.gm_first[nt];
                L.gm_first_af[nt] = R.gm_first_af[nt];
                L.gm_rest[nt] = R.gm_rest[nt];
            } else {
                float m = L.gm_rest[nt];
                if (m <= R.gm_first_af[nt]) m = R.gm_first_af[nt];
                if (m <= R.gm_rest[nt]) m = R.gm_rest[nt];
                L.gm_rest[nt] = m;
            }
            L.gm_n[nt] += R.gm_n[nt];
        }
    }
    L.nrec += R.nrec;
}

struct AccPtrs {
    double *snt; long long *srd; int *cnt; int *nrec; int *gm_n; int *gm_first; float *gm_first_af; float *gm_rest;
};

__device__ __forceinline__ void lane_acc_store(const AccPtrs &t, long long P, long long p, const LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        t.snt[(0 * 4 + nt) * P + p] = a.snt[0][nt];
        t.snt[(1 * 4 + nt) * P + p] = a.snt[1][nt];
        t.srd[(0 * 4 + nt) * P + p] = a.srd[0][nt];
        t.srd[(1 * 4 + nt) * P + p] = a.srd[1][nt];
        t.cnt[nt * P + p] = a.cnt[nt];
        t.gm_n[nt * P + p] = a.gm_n[nt];
        t.gm_first[nt * P + p] = a.gm_first[nt];
        t.gm_first_af[nt * P + p] = a.gm_first_af[nt];
        t.gm_rest[nt * P + p] = a.gm_rest[nt];
    }
    t.nrec[p] = a.nrec;
}

__device__ __forceinline__ void lane_acc_load(const AccPtrs &t, long long P, long long p, LaneAcc &a)
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        a.snt[0][nt] = t.snt[(0 * 4 + nt) * P + p];
        a.snt[1][nt] = t.snt[(1 * 4 + nt) * P + p];
        a.srd[0][nt] = t.srd[(0 * 4 + nt) * P + p];
        a.srd[1][nt] = t.srd[(1 * 4 + nt) * P + p];
        a.cnt[nt] = t.cnt[nt * P + p];
        a.gm_n[nt] = t.gm_n[nt * P + p];
        a.gm_first[nt] = t.gm_first[nt * P + p];
        a.gm_first_af[nt] = t.gm_first_af[nt * P + p];
        a.gm_rest[nt] = t.gm_rest[nt * P + p];
    }
    a.nrec = t.nrec[p];
}

// ---------------------------------------------------------------------------
// finalize of one position from its merged LaneAcc: quorum, rates, NaN code, the table text round trip and the
// Germ_Max sentinel rule (EE:1659-1714 + clones, EE:1260/1318/1374/1431, EE:1704 -> VC:889-890, EE:2680-2684).
// Shared by error_finalize_kernel and by the fused epilogue of error_reduce_kernel.
// ---------------------------------------------------------------------------
struct FinOut {
    float *rate; unsigned char *code; float *thr; float *germ_val; unsigned char *germ_present; int *flags;
    double *packed; // optional: the additive planes as [snt 8P | srd 8P | cnt 4P | nrec P] doubles (multi-GPU merge)
    // position-sliced exchange buffers (reduce-scatter / all-to-all merge): slice k = positions [k*slice_len, (k+1)*slice_len)
    long long slice_len; // 0: `packed` is plane-major over the whole panel (above)
    double *sl_sums;     // [n_slices][21][slice_len]: the same 21 additive planes, slice-major
    float *sl_gm;        // [n_slices][8][slice_len]: germ-max first_af[4] (-1 = no qualifying record) | rest[4]
    long long sl_group;  // batches per slice chunk (ampli_set_slice_group): chunk k of this batch starts k*sl_group*{planes,8}*slice_len
                         //  elements behind sl_sums / sl_gm (which already point at this batch's part of chunk 0)
    int sl_fmt;          // AMPLI_SLICE_WIDE: 21 planes, one value each; AMPLI_SLICE_SLIM: 14 planes, the integer planes packed
    int sl_n;            //  (slim) number of slices = ranks whose contributions are summed: the range a shard may use of a packed field
    int *sl_flags;       //  (slim) the context's flag word: AMPLI_FLAG_SLICE_RANGE when a value does not fit its share of a field
    int accumulate;      // the table already holds the state of the EARLIER samples: result = table (+) this launch
                         //  (streamed cohorts: one launch per uploaded chunk of samples, in visit order)
    int summary;         // host side only: the caller takes the table as streaming state (AMPLI_REDUCE_SUMMARY), so the compact kernel may write it
};

// The sums of the sliced exchange travel as doubles (ONE reduce-scatter, SUM, f64).  AMPLI_SLICE_WIDE: 21 planes, one value
// each (snt 8 | srd 8 | cnt 4 | nrec 1) = 168 B per position.  AMPLI_SLICE_SLIM: 14 planes = 112 B: the integer planes share
// doubles -- the two strands' depth sums of a nucleotide as lo + hi * 2^26, the counts as a + b * 2^17 (+ c * 2^34).  A sum of
// doubles adds the fields independently and exactly as long as every field's TOTAL stays below its width (and the whole below
// 2^53): each of the n shards may therefore use 1/n of a field's range, checked here where the shard's values are packed
// (AMPLI_FLAG_SLICE_RANGE: the caller repeats the exchange in the wide format; config 4 on 8 GPUs uses < 3 % of the range).
constexpr double SLIM_D = 67108864.0;        // 2^26: strand-depth sums
constexpr double SLIM_C = 131072.0;          // 2^17: record counts
constexpr double SLIM_C2 = 17179869184.0;    // 2^34
__host__ __device__ constexpr int slice_planes(const int fmt) { return fmt == AMPLI_SLICE_SLIM ? 14 : 21; }

__host__ __device__ __forceinline__ size_t slice_block_bytes(const long long L) { return (size_t)L * 88 + 64; }

// quorum, rates and NaN code of one (position, nucleotide) from its sums (EE:1659-1682): the code, 0 estimate, 1 below quorum,
// 2 NaN; the rates are 0 unless the code is 0.  Shared by finalize_one and the leave-one-out kernel's S-1 tables.
__device__ __forceinline__ unsigned char fin_rates(const double sfw, const double sbw, const long long dfw, const long long dbw, const int cnt,
                                                   const int nrec, float &r_fw, float &r_bw)
{
    r_fw = 0.0f; r_bw = 0.0f;
    if ((double)cnt < 0.338 * (double)nrec) return 1; // EE:1659
    r_fw = (float)sfw / (float)(double)dfw; // EE:1679
    r_bw = (float)sbw / (float)(double)dbw; // EE:1680
    if (isnan(r_fw) || isnan(r_bw)) { r_fw = 0.0f; r_bw = 0.0f; return 2; } // EE:1682
    return 0;
}

// one (position, nucleotide): returns true when a double sum left the exactness envelope
__device__ __forceinline__ bool finalize_one(const int nt, const double sfw, const double sbw, const long long dfw, const long long dbw,
                                             const int cnt, const int nrec, const int gm_n, const float gm_rest, const long long P,
                                             const long long p, const double limit, const FinOut &o)
{
    const long long i = nt * P + p, ifw = (0 * 4 + nt) * P + p, ibw = (1 * 4 + nt) * P + p;
    float r_fw, r_bw;
    const unsigned char c = fin_rates(sfw, sbw, dfw, dbw, cnt, nrec, r_fw, r_bw);
    o.code[i] = c;
    o.rate[ifw] = r_fw;
    o.rate[ibw] = r_bw;
    if (o.thr) {
        o.thr[ifw] = c ? 0.01f : ampli_text_roundtrip(r_fw); // EE:2680-2684 / EE:1704 -> VC:889-890
        o.thr[ibw] = c ? 0.01f : ampli_text_roundtrip(r_bw);
    }
    if (o.germ_val) {
        float v = (nt == 0) ? -888.0f : 0.0f; // EE:1260 / EE:1318,1374,1431
        if (gm_n > 1) { if (v <= gm_rest) v = gm_rest; }
        o.germ_val[i] = gm_n ? v : 0.0f;
        if (o.germ_present) o.germ_present[i] = gm_n ? 1 : 0;
    }
    return !(sfw < limit) || !(sbw < limit);
}

// exactness envelope of the double sums: every addend is a multiple of ulp(float(cov)*C) and the
// running sum must stay below 2^52 such ulps
__device__ __forceinline__ double envelope_limit(const float C, const int cov)
{
    const float pmin = (float)cov * C;
    int ex;
    (void)frexpf(pmin > 0 ? pmin : 1.0f, &ex);
    return ldexp(1.0, ex - 24) * 9007199254740992.0 * 0.5;
}

__device__ __forceinline__ void finalize_lane(const LaneAcc &a, const long long P, const long long p, const float C,
                                              const int cov, const FinOut &o)
{
    const double limit = envelope_limit(C, cov);
    bool bad = false;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
        bad |= finalize_one(nt, a.snt[0][nt], a.snt[1][nt], a.srd[0][nt], a.srd[1][nt], a.cnt[nt], a.nrec, a.gm_n[nt], a.gm_rest[nt], P, p,
                            limit, o);
    if (bad && o.flags) atomicOr(o.flags, 1);
}

// ==== poisson_call's hand-over: the queued item, the staged flush, the drain ===========================================================

// the reported VAFs and the evidence of one emitted call (VC:772-817)
__device__ __forceinline__ void call_fill(ampli_call &c, const int sample, const int record, const int alt, const int rd, const double q_fw,
                                          const double q_bw, const int k_fw, const int k_bw, const int FW, const int BW, const int flags = 0)
{
    c.sample = sample; c.record = record; c.alt = alt; c.rd = rd;
    c.q_fw = q_fw; c.q_bw = q_bw;
    c.af = (float)(k_fw + k_bw) / (float)rd;               // VC:814-817
    c.af_fw = FW == 0 ? 0.0f : (float)k_fw / (float)FW;    // VC:785-790
    c.af_bw = BW == 0 ? 0.0f : (float)k_bw / (float)BW;    // VC:805-810
    c.k_fw = k_fw; c.k_bw = k_bw; c.fw = FW; c.bw = BW; c.flags = flags;
}

struct PcItem { // 40 bytes, self-contained: the drain kernel needs no second look at the records or the thresholds
    int sample;
    int record_alt;   // record | alt << 30
    int k_fw, k_bw;   // alt reads per strand
    int FW, BW;       // strand depths
    int rd;           // RD column: d_fw = rd - BW (VC:895), AF = X / rd (VC:814)
    float e_fw, e_bw; // effective errors (ampli_effective_err); the leave-one-out kernel queues the raw thresholds of its S-1 table here
    int pad;
};

// Queue hand-over of a wave's staged items: ONE returning atomic on the shard's counter for up to PC_STAGE items (a
// returning atomic costs a wave 1-3 us under load; one per (row, alternative) with a survivor, as a first version did,
// kept ~40 % of the waves waiting at some point of their short lives), then a coalesced copy LDS -> HBM.
constexpr int PC_STAGE = 64; // items a wave stages before it must hand over (64 lanes x at most one item per (row, alt))

__device__ __forceinline__ void pc_flush(const PcItem *__restrict__ st, const int count, const int lane, PcItem *__restrict__ queue,
                                         const long long queue_per_shard, unsigned long long *__restrict__ queue_n, const unsigned shard,
                                         int *__restrict__ flags)
{
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&queue_n[shard * AMPLI_CALL_COUNTER_STRIDE], (unsigned long long)count);
    base = __shfl(base, 0);
    // 40-byte items as 10 dwords each: lane l copies dwords l, l + 64, ...
    const unsigned *__restrict__ src = (const unsigned *)st;
    const long long room = queue_per_shard - (long long)base; // items that still fit (<= 0: none)
    const int fit = room >= count ? count : (room > 0 ? (int)room : 0);
    unsigned *__restrict__ dst = (unsigned *)(queue + (size_t)shard * queue_per_shard + base);
    for (int i = lane; i < fit * 10; i += 64) dst[i] = src[i];
    if (fit < count && lane == 0) atomicOr(flags, AMPLI_FLAG_QUEUE_OVERFLOW);
}

// Two adjacent lanes per queued item, one per strand.  The scorer here is kf_gammaq's series branch in its
// division-free form (ampli_kf_gammap_series_nodiv): a queued item has k > m on both strands or is no call.
// LOO (the leave-one-out drain): the item carries the raw thresholds of its S-1 table instead of the effective errors, and
// the list entries are ampli_loo_call, which keep those thresholds for the host.
template <bool LOO>
__device__ __forceinline__ void drain_body(
    const PcItem *__restrict__ queue, const long long queue_per_shard, const unsigned long long *__restrict__ queue_n,
    const long long R, unsigned *__restrict__ mask_words, std::conditional_t<LOO, ampli_loo_call, ampli_call> *__restrict__ calls,
    const long long capacity, unsigned long long *__restrict__ n_calls, unsigned long long *__restrict__ next_queue_n, const unsigned shard_lo,
    const unsigned shard_n, const double *__restrict__ lgtab)
{
    constexpr int IPB = 128; // items per workgroup pass
    // the counter array of the NEXT poisson_call (the other half of a double buffer; its last reader, the previous
    // drain, finished before this kernel started) is reset here, which saves a memset launch per call
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < AMPLI_CALL_SHARDS) next_queue_n[threadIdx.x * AMPLI_CALL_COUNTER_STRIDE] = 0ull;
    // blockIdx.x = queue shard, blockIdx.y = workgroup within the shard: one load tells a workgroup what is its to do
    const unsigned shard = blockIdx.x;
    const int slot = threadIdx.x >> 1, strand = threadIdx.x & 1;
    // the first pass's item is fetched BEFORE the shard's count is known (the slot exists whatever the count is): the kernel is one
    // chain of dependent latencies -- count, item, scorer, returning atomic -- and this takes one link out of it
    const long long i0 = (long long)blockIdx.y * IPB + slot;
    PcItem first = queue[(size_t)shard * queue_per_shard + (i0 < queue_per_shard ? i0 : 0)];
    long long cnt = (long long)queue_n[shard * AMPLI_CALL_COUNTER_STRIDE];
    if (cnt > queue_per_shard) cnt = queue_per_shard;
    for (long long ib = (long long)blockIdx.y * IPB; ib < cnt; ib += (long long)gridDim.y * IPB) {
        const long long i = ib + slot;
        const bool on = i < cnt;
        PcItem it = ib == (long long)blockIdx.y * IPB ? first : queue[(size_t)shard * queue_per_shard + (on ? i : ib)];
        const int k = strand ? it.k_bw : it.k_fw;
        const int d = strand ? it.BW : it.rd - it.BW; // VC:895-896
        const float err = LOO ? ampli_effective_err(strand ? it.e_bw : it.e_fw) : (strand ? it.e_bw : it.e_fw);
        // err_eff = +inf stands for err == -1 (Q = -888, VC:3844-3849); 0 was already replaced by 0.0010008f.
        // k <= m: the exact form of the prefilter bound (ampli_prefilter_nocall), Q < 5 -- no call whatever the value.
        const double m = (double)d * err; // VC:3864: double * float
        const bool eval = on && !isinf(err) && (double)k > m; // then z = m < s = k: the series branch of kf_gammaq (VC:3728)
        double qv = -1.0; // "no call" (any value below 5)
        if (eval) {
            if (m > 0) qv = ampli_q_from_p(ampli_drain_p(k, m, lgtab, AMPLI_LGTAB)); // VC:3865 on top of VC:3728: p = 1 - (1 - P(s, z))
            else if (m == 0) qv = 100.0; // z = 0: the reference's series gives P = exp(-inf) = 0, p = 0 < 1e-10
            // m < 0 (a negative error cell, or an irregular line with RD < RD_reverse): log(z) is NaN in the reference,
            // Q is NaN and VC:898 is false
        }
        const double q_other = __shfl_xor(qv, 1);
        const bool is_call = on && strand == 0 && qv >= 5 && q_other >= 5; // VC:898 (coverage was checked before queueing)
        // a Q within 1e-6 of the gate cannot be decided here (include/amplisolve_hip.h, AMPLI_CALL_BORDERLINE): the pair goes
        // on the list either way, flagged, for the host to re-evaluate with the reference's own operation sequence
        const double lo = 5.0 - AMPLI_CALL_GATE_EPS, hi = 5.0 + AMPLI_CALL_GATE_EPS;
        const bool near_gate = on && strand == 0 && qv >= lo && q_other >= lo && (qv < hi || q_other < hi);
        const bool emit = is_call || near_gate;
        if (is_call) {
            const int record = it.record_alt & 0x3FFFFFFF, alt = (it.record_alt >> 30) & 3;
            const size_t o = (size_t)it.sample * R + record;
            atomicOr(&mask_words[o >> 2], (1u << alt) << ((o & 3) * 8));
        }
        if (n_calls) { // one counter add per wave, not per call
            const unsigned long long bal = __ballot(emit);
            if (bal) {
                const int lane = threadIdx.x & 63, leader = (int)__ffsll((long long)bal) - 1;
                const unsigned cs = shard_lo + (unsigned)((blockIdx.y * gridDim.x + blockIdx.x) % shard_n); // this launch's shards of the call list
                const long long per = capacity / AMPLI_CALL_SHARDS;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(&n_calls[cs * AMPLI_CALL_COUNTER_STRIDE], (unsigned long long)__popcll(bal));
                base = __shfl(base, leader);
                if (emit && calls) {
                    const long long idx = (long long)base + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
                    if (idx < per) {
                        ampli_call c;
                        call_fill(c, it.sample, it.record_alt & 0x3FFFFFFF, (it.record_alt >> 30) & 3, it.rd, qv, q_other, it.k_fw, it.k_bw, it.FW, it.BW,
                                  near_gate ? AMPLI_CALL_BORDERLINE : 0);
                        if constexpr (LOO) {
                            ampli_loo_call lc;
                            lc.call = c; lc.thr_fw = it.e_fw; lc.thr_bw = it.e_bw; lc.code = it.pad; lc.pad = 0;
                            calls[(size_t)cs * per + idx] = lc;
                        } else {
                            calls[(size_t)cs * per + idx] = c;
                        }
                    }
                }
            }
        }
    }
}

// ==== host helpers more than one unit calls: each is defined once, in the unit that owns its stage =====================================

// ampli_kernels.hip
int cohort_from_records(ampli_ctx *ctx, const ampli_records *r, int64_t P, DevCohort &c); // an ampli_records argument as a cohort
int check_records(ampli_ctx *ctx, const DevCohort &co, const char *what, const uint32_t *index, const char *index_name);
void acc_offsets(int64_t P, size_t off[9]);    // byte offsets of the accumulator table's planes; off[8] = its size
AccPtrs to_ptrs(const ampli_acc_table *t);
bool acc_is_bound(const ampli_acc_table *t);   // one buffer carved by ampli_acc_bind
FinOut table_out(float *rate, uint8_t *code, float *thr, float *germ_val, uint8_t *germ_present, int32_t *flags);
FinOut slice_out(const ampli_ctx *ctx, long long P, int n_slices, double *d_sums, float *d_gm);
int ensure_ws(ampli_ctx *ctx, size_t bytes);   // the context's workspace, at least `bytes`
int ensure_lgtab(ampli_ctx *ctx);              // ctx->d_lgtab, built on first use
int queue_prepare(ampli_ctx *ctx, AmpliQueue &Q, size_t want, hipStream_t st, long long &per, unsigned long long *&qn,
                  unsigned long long *&qn_next);
int launch_acc_pack_sliced(ampli_ctx *ctx, const AccPtrs &t, long long P, const FinOut &fo); // acc_pack_sliced_kernel on the context's stream
// ampli_exchange.hip
int launch_acc_pack(ampli_ctx *ctx, const AccPtrs &t, long long P, double *d_packed);        // acc_pack_kernel on the context's stream
