// amplisolve_amd/csrc/ampli_bam.h -- the BAM vocabulary of the four kernels that walk alignment records (ampli_pileup.hip, ampli_indel.hip,
// ampli_amplicon_count.hip, ampli_evidence.hip): the record layout, the kept-read filter, the position keys and their searches, the base
// decode and the CIGAR classes.  Device-only, not part of the ABI.  Each walk keeps its own control flow; only the format lives here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// ---------------------------------------------------------------------------
// loads: a record starts wherever the one before it ended, so none of its dwords is aligned.  Loader types, so the header decode and
// the CIGAR read say where the record lives.
// ---------------------------------------------------------------------------
struct bam_u32 { // unaligned little-endian dword from global memory
    __device__ __forceinline__ unsigned operator()(const unsigned char *p) const
    {
        unsigned v;
        __builtin_memcpy(&v, p, 4);
        return v;
    }
};

struct lds_u32 { // the same out of LDS: two aligned dwords and a byte shift (the bytes behind p must be readable up to the next dword)
    __device__ __forceinline__ unsigned operator()(const unsigned char *p) const
    {
        const unsigned *q = (const unsigned *)((uintptr_t)p & ~(uintptr_t)3);
        const unsigned sh = (unsigned)((uintptr_t)p & 3u);
        const unsigned lo = q[0], hi = q[1];
        return sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
    }
};

// ---------------------------------------------------------------------------
// the record header.  r points past block_size: ref_id, pos, (bin << 16 | mapq << 8 | l_read_name), (flag << 16 | n_cigar), l_seq,
// three dwords of the mate, then the read name, the CIGAR, the 4-bit bases and the qualities.
// ---------------------------------------------------------------------------
constexpr unsigned BAM_FILTERED = 0x4u | 0x100u | 0x200u | 0x400u; // unmapped, secondary, QC-fail, duplicate: the pileup engine's default mask

struct BamRead { // the header fields of a kept read
    const unsigned char *cig, *seq, *qual;
    long long pos; // 0-based
    int ref_id, n_cigar, l_seq, mapq, rev;
};

// false: the read is not kept (unplaced, a filtered flag, MAPQ < mrq) and h is not written
template <typename Load>
__device__ __forceinline__ bool bam_read_header(const unsigned char *r, const int mrq, BamRead &h)
{
    const Load ld;
    const int ref_id = (int)ld(r), pos = (int)ld(r + 4);
    const unsigned bin_mq_nl = ld(r + 8), flag_nc = ld(r + 12);
    const int l_read_name = (int)(bin_mq_nl & 0xffu), mapq = (int)((bin_mq_nl >> 8) & 0xffu);
    const unsigned flag = flag_nc >> 16;
    if (ref_id < 0 || pos < 0 || (flag & BAM_FILTERED) != 0 || mapq < mrq) return false;
    h.ref_id = ref_id;
    h.pos = pos;
    h.mapq = mapq;
    h.n_cigar = (int)(flag_nc & 0xffffu);
    h.l_seq = (int)ld(r + 16);
    h.rev = (int)((flag >> 4) & 1u);
    h.cig = r + 32 + l_read_name;
    h.seq = h.cig + 4 * (size_t)h.n_cigar;
    h.qual = h.seq + (h.l_seq + 1) / 2;
    return true;
}

// ---------------------------------------------------------------------------
// keys: (BAM reference id << 32 | 1-based position), sorted ascending, and their searches.  I is the index type: int over an LDS
// window, long long over the global list.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long bam_key(const int ref_id, const long long pos1)
{
    return ((unsigned long long)(unsigned)ref_id << 32) | (unsigned long long)pos1;
}

// first index in [a, b) with v[i] >= key (b if none)
template <typename I>
__device__ __forceinline__ I bam_lower(const unsigned long long *v, I a, I b, const unsigned long long key)
{
    while (a < b) {
        const I mid = (a + b) >> 1;
        if (v[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// first index in [a, b) with v[i] > key (b if none)
template <typename I>
__device__ __forceinline__ I bam_upper(const unsigned long long *v, I a, I b, const unsigned long long key)
{
    while (a < b) {
        const I mid = (a + b) >> 1;
        if (v[mid] <= key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// Where a workgroup's LDS window starts: the first key at or behind the start of the first PLACED read among reads [first, end) -- 0
// if there is none.  Only unplaced reads are skipped, not filtered ones: a filtered read lies where its neighbours lie.  k0: that
// read's key, ~0 if there is none.  One thread's work.
__device__ __forceinline__ long long bam_window_base(const unsigned char *bam, const unsigned long long *rec_off, const long long first, const long long end,
                                                     const unsigned long long *keys, const long long P, unsigned long long &k0)
{
    k0 = ~0ull;
    for (long long rd = first; rd < end; ++rd) {
        const unsigned char *r = bam + rec_off[rd] + 4;
        const int ref_id = (int)bam_u32()(r), pos = (int)bam_u32()(r + 4);
        if (ref_id < 0 || pos < 0) continue;
        k0 = bam_key(ref_id, (long long)pos + 1);
        return bam_lower<long long>(keys, 0, P, k0);
    }
    return 0;
}

// Column j of a run whose first key has the lower bound lo in the window; wend = min(lo + run length, window keys).  Where the panel
// has no gap along the run the key sits at lo + j; otherwise it is searched in [lo, wend).  The window index of key, -1: not a panel position.
__device__ __forceinline__ int bam_window_find(const unsigned long long *wkeys, const int lo, const int wend, const int j, const unsigned long long key)
{
    int a = lo + j < wend ? lo + j : wend - 1;
    if (wkeys[a] != key) a = bam_lower<int>(wkeys, lo, wend, key);
    return a < wend && wkeys[a] == key ? a : -1;
}

// ---------------------------------------------------------------------------
// bases and CIGAR
// ---------------------------------------------------------------------------
// base q of the 4-bit sequence (high nibble first): A, C, G, T -> 0..3, everything else (N and the ambiguity codes) -> -1
template <typename I>
__device__ __forceinline__ int bam_nt(const unsigned char *seq, const I q)
{
    const unsigned nib = (seq[q >> 1] >> ((~q & 1) * 4)) & 15u;
    return nib == 1u ? 0 : (nib == 2u ? 1 : (nib == 4u ? 2 : (nib == 8u ? 3 : -1)));
}

struct BamOp {
    unsigned op; // 0 M, 1 I, 2 D, 3 N, 4 S, 5 H, 6 P, 7 =, 8 X
    int len;
};

template <typename Load>
__device__ __forceinline__ BamOp bam_cigar(const unsigned char *cig, const int c)
{
    const unsigned op_len = Load()(cig + 4 * (size_t)c);
    return {op_len & 15u, (int)(op_len >> 4)};
}

// The three classes a walk tells apart; H and P are in none: they consume neither.
__device__ __forceinline__ bool bam_op_match(const unsigned op) { return op == 0 || op == 7 || op == 8; } // M, =, X: a run of columns
__device__ __forceinline__ bool bam_op_query(const unsigned op) { return op == 1 || op == 4; }            // I, S: the query only
__device__ __forceinline__ bool bam_op_ref(const unsigned op) { return op == 2 || op == 3; }              // D, N: the reference only
