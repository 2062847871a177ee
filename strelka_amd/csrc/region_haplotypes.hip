// region_haplotypes.hip -- from the list of active regions to each region's selected haplotypes: what the reference's detector keeps
// per read for haplotype generation (ActiveRegionReadBuffer::insertMatch / insertMismatch / insertSoftClipSegment / insertIndel,
// L/starling_common/ActiveRegionReadBuffer.cpp:26-141, as addAlignmentIndelsToPosProcessor calls them,
// L/starling_common/starling_pos_processor_indel_util.cpp:428-481), getHaplotypeBase (:143-171), getReadSegments with
// includePartialReads = false (:191-256), and ActiveRegionProcessor's counting path (L/starling_common/ActiveRegionProcessor.cpp:
// processHaplotypes' check :45-56, generateHaplotypesWithCounting :79-114, the phasing-noise filter :296-414, selectHaplotypes and
// selectOrDropHaplotypesWithSameCount :416-516).
//
// The store is never built.  What a read registered at a position is a closed form of its path and its observations (hp_resolve), so a
// read's string over a region is rebuilt wherever it is needed:
//
//   H0  hap_extent_kernel   a thread per read: first and last registered position
//   H1  hap_region_kernel   one WAVE per region slot (one-wave workgroups striding over region_cap slots, leaving at *n_regions).
//       a) the reads registered anywhere in the region, by ballot in index order, into an LDS list (their extents first, then the exact
//          walk: a hole -- a swap, a breakpoint -- may cover the whole region); the decline rules
//       b) per listed read its string, lanes across the region's positions 64 at a time, a wave prefix sum placing the bytes in an LDS
//          row; covering or not (getReadSegments' five conditions), a 64-bit polynomial hash and the length
//       c) classes: a read's representative is the first earlier read with the same (hash, length) whose BYTES are equal -- both
//          strings are rebuilt and compared, so a hash collision costs time and nothing else ($SK_HAP_TEST_HASH_BITS narrows the hash
//          for the tests)
//       d) counts and forward-strand counts per class; the classes of 3 reads and more (at most 16, else declined) get their strings
//          into LDS; one lane orders them (std::map order, then libstdc++'s insertion sort on the count), applies the filter and runs
//          the select-or-drop rule as the reference writes it
//       e) the selected strings and their supporting reads go to scratch pools at atomically taken offsets
//   H2  hap_offsets_kernel  one workgroup: region order offsets (a scan), query_off, totals
//   H3  hap_copy_kernel     scratch pools -> the output pools at those offsets, so the layout does not depend on workgroup timing
//
// Out of scope (see the header): routing, the assembly fallback, doNotUseHaplotyping's marks, _haplotypesToExclude, the multi-sample
// synchroniser, external and forced candidates.
#include "sk_common.h"

#include <climits>
#include <cstdlib>

namespace
{

typedef unsigned long long u64;

enum {
    HP_MAX_LEN = SK_PILEUP_MAX_READ_LEN,
    HP_LIST = 1024,       // room of the list of registered reads: a region with more than 1 000 is declined (the index spread)
    HP_RING = 1000,       // ActiveRegionReadBuffer::MaxDepth, MaxBufferSize (.hh:61-65)
    HP_MAX_GROUPS = SK_HAP_MAX_GROUPS,
    HP_MIN_COUNT = 3,     // MinHaplotypeCount
    HP_MIN_HPOL = 10,     // minPhaseErrorHpolSize (ActiveRegionProcessor.cpp:338)
    HP_GRID = 2048,
    HP_SCAN_T = 1024
};
enum { EK_NONE = 0, EK_MATCH, EK_MISMATCH, EK_DELETE, EK_INSERT, EK_MISMATCH_INSERT, EK_SOFT_CLIP };
enum { HC_SEQ = 0, HC_SUPPORT = 1 };

struct HapArgs
{
    const char* ref;
    int32_t ref_offset, ref_len;
    int32_t n_reads;
    const int64_t* read_off;
    const uint8_t* read_code;
    const int64_t* path_off;
    const int32_t* n_seg;
    const sk_path_seg* path;
    const int32_t* pos;
    const uint8_t* low_mapq;
    const uint8_t* is_fwd;
    const int64_t* obs_off;
    const sk_intake_obs* obs;
    uint32_t max_indel_size;
    int32_t buf_begin, buf_end, ploidy;
    const sk_region_params* params; // per region instead of the three above; nullptr: the same for all
    const sk_active_region* regions;
    const int32_t* n_regions;
    int64_t region_cap;
    sk_region_haplotypes_rec* recs;
    int32_t* ext;     // scratch: first and last registered position per read (first > last: none)
    u64* counters;    // scratch: bytes and entries taken from the scratch pools
    int64_t* tmp_off; // scratch: per (slot, selected haplotype) its offsets in the scratch pools
    uint8_t* tmp_seq;
    int32_t* tmp_support;
    int64_t seq_cap, support_cap;
    u64 hash_mask;
    unsigned* err;
};

__device__ __forceinline__ bool hp_is_match(const uint32_t t) { return t == SK_SEG_MATCH || t == SK_SEG_SEQ_MATCH || t == SK_SEG_SEQ_MISMATCH; }
// bam_seq::get_char of a BAM 4-bit code
__device__ __forceinline__ uint32_t hp_code_char(const uint32_t c)
{
    return c == 0u ? uint32_t('=') : c == 1u ? uint32_t('A') : c == 2u ? uint32_t('C') : c == 4u ? uint32_t('G') : c == 8u ? uint32_t('T') : uint32_t('N');
}
// reference_contig_segment::get_base
__device__ __forceinline__ uint32_t hp_ref_char(const HapArgs& a, const int64_t p)
{
    const int64_t k = p - a.ref_offset;
    return (k < 0 || k >= a.ref_len) ? uint32_t('N') : uint32_t(uint8_t(a.ref[k]));
}

struct ReadView
{
    bool ok; // registers anything at all: not low-MAPQ, sizes in range
    int L, ns;
    int32_t pos;
    const uint8_t* code;
    const sk_path_seg* p;
    int64_t ob, oe;
};
__device__ __forceinline__ ReadView hp_view(const HapArgs& a, const int r, bool* bad_input)
{
    ReadView v;
    const int64_t rb = a.read_off[r];
    const int64_t L64 = a.read_off[r + 1] - rb;
    v.ns = a.n_seg[r];
    v.ob = a.obs_off[r];
    v.oe = a.obs_off[r + 1];
    const bool bad = L64 < 0 || L64 > HP_MAX_LEN || v.ns < 0 || v.ob < 0 || v.oe < v.ob; // (the host entry refuses these)
    if (bad_input) *bad_input = bad;
    v.ok = !bad && a.low_mapq[r] == 0; // a low-MAPQ read registers nothing (:430, :463, .cpp:70)
    v.L = bad ? 0 : int(L64);
    v.pos = a.pos[r];
    v.code = a.read_code + rb;
    v.p = a.path + a.path_off[r];
    return v;
}
__device__ __forceinline__ int hp_last_match(const ReadView& v)
{
    int last = -1;
    for (int i = 0; i < v.ns; ++i)
        if (hp_is_match(v.p[i].type)) last = i;
    return last;
}
__device__ __forceinline__ bool hp_primitive_insertion(const sk_intake_obs& o) { return o.type == SK_INDEL_INDEL && !o.is_low_mapq && o.ins_len > 0u && o.deletion_length == 0u; }
__device__ __forceinline__ bool hp_primitive_deletion(const sk_intake_obs& o) { return o.type == SK_INDEL_INDEL && !o.is_low_mapq && o.deletion_length > 0u && o.ins_len == 0u; }

// The registered positions of a read as intervals [lo, hi]: f(lo, hi) for every match segment, edge soft clip, primitive deletion and
// primitive insertion (its key.pos - 1); f returns true to stop.
template <typename F> __device__ __forceinline__ void hp_intervals(const HapArgs& a, const ReadView& v, F f)
{
    if (!v.ok) return;
    const int last = hp_last_match(v);
    bool seen = false;
    int64_t fs = v.pos;
    for (int i = 0; i < v.ns; ++i) {
        const sk_path_seg s = v.p[i];
        if (hp_is_match(s.type)) {
            if (s.length && f(fs, fs + int64_t(s.length) - 1)) return;
            seen = true;
            fs += s.length;
        } else if (s.type == SK_SEG_SOFT_CLIP) {
            if (!seen || i > last) { // an edge soft clip: at al.pos - 1, or at the reference head after the last aligned base (:428-441)
                const int64_t at = seen ? fs : fs - 1;
                if (f(at, at)) return;
            }
        } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
            fs += s.length;
        }
    }
    for (int64_t k = v.ob; k < v.oe; ++k) {
        const sk_intake_obs o = a.obs[k];
        if (hp_primitive_deletion(o)) {
            if (f(int64_t(o.pos), int64_t(o.pos) + int64_t(o.deletion_length) - 1)) return;
        } else if (hp_primitive_insertion(o)) {
            if (f(int64_t(o.pos) - 1, int64_t(o.pos) - 1)) return;
        }
    }
}

// H0
__global__ __launch_bounds__(256) void hap_extent_kernel(const HapArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    bool bad = false;
    const ReadView v = hp_view(a, r, &bad);
    if (bad) atomicOr(a.err, unsigned(SK_DEVERR_HAPLOTYPES));
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    hp_intervals(a, v, [&](const int64_t x, const int64_t y) {
        lo = x < lo ? x : lo;
        hi = y > hi ? y : hi;
        return false;
    });
    if (lo > hi) {
        a.ext[2 * r] = 1;
        a.ext[2 * r + 1] = 0;
    } else { // (clamped: only compared against regions, which are int32)
        a.ext[2 * r] = int32_t(lo < INT32_MIN ? INT32_MIN : lo > INT32_MAX ? INT32_MAX : lo);
        a.ext[2 * r + 1] = int32_t(hi < INT32_MIN ? INT32_MIN : hi > INT32_MAX ? INT32_MAX : hi);
    }
}

__device__ __forceinline__ bool hp_any_registered(const HapArgs& a, const ReadView& v, const int32_t begin, const int32_t end)
{
    bool hit = false;
    hp_intervals(a, v, [&](const int64_t x, const int64_t y) {
        hit = x < int64_t(end) && y >= int64_t(begin);
        return hit;
    });
    return hit;
}

// What the read registered at position p (setMatch / setMismatch / setSoftClipSegment / setDelete / setInsert, .cpp:109-141)
struct Emit
{
    int kind;
    uint32_t base;              // MISMATCH, MISMATCH_INSERT: the read's character
    uint32_t ins_begin, ins_len; // INSERT, MISMATCH_INSERT: the insert as a range of the read's bases
};
__device__ __forceinline__ Emit hp_resolve(const HapArgs& a, const ReadView& v, const int last, const int64_t p)
{
    Emit e;
    e.kind = EK_NONE;
    e.base = 0;
    e.ins_begin = e.ins_len = 0;
    if (!v.ok) return e;
    bool seen = false;
    int64_t rs = 0, fs = v.pos;
    for (int i = 0; i < v.ns; ++i) {
        const sk_path_seg s = v.p[i];
        if (hp_is_match(s.type)) {
            if (p >= fs && p < fs + int64_t(s.length)) {
                const int64_t rp = rs + (p - fs);
                if (rp < v.L) { // (a path longer than the read: refused by the host entry)
                    const uint32_t rc = hp_code_char(v.code[rp]);
                    e.kind = rc != hp_ref_char(a, p) ? EK_MISMATCH : EK_MATCH; // the raw characters (:471-480)
                    e.base = rc;
                }
            }
            seen = true;
            rs += s.length;
            fs += s.length;
        } else if (s.type == SK_SEG_SOFT_CLIP) {
            if ((!seen || i > last) && p == (seen ? fs : fs - 1)) e.kind = EK_SOFT_CLIP;
            rs += s.length;
        } else if (s.type == SK_SEG_INSERT) {
            rs += s.length;
        } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
            fs += s.length;
        }
    }
    for (int64_t k = v.ob; k < v.oe; ++k) {
        const sk_intake_obs o = a.obs[k];
        if (hp_primitive_insertion(o)) {
            if (p == int64_t(o.pos) - 1) {
                e.kind = e.kind == EK_MISMATCH ? EK_MISMATCH_INSERT : EK_INSERT; // setInsert :139
                e.ins_begin = o.ins_begin;
                e.ins_len = o.ins_len;
            }
        } else if (hp_primitive_deletion(o)) {
            if (p >= int64_t(o.pos) && p < int64_t(o.pos) + int64_t(o.deletion_length)) e.kind = EK_DELETE;
        }
    }
    return e;
}

__device__ __forceinline__ int hp_incl_scan(int v, const int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ u64 hp_wave_sum64(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += u64(__shfl_xor((long long)v, d, 64));
    return v;
}
__device__ __forceinline__ u64 hp_pow(u64 b, unsigned e)
{
    u64 r = 1;
    while (e) {
        if (e & 1u) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// One read's string over [begin, end) (getReadSegments :202-237 for one align id), written to `row` (HP_MAX_LEN bytes of LDS) by the
// whole wave.  Every lane gets the same result.
struct Built
{
    bool registered;  // at any position of the region (allAlignIds)
    bool covering;    // at begin and at end - 1, never soft-clipped, no N, not empty (:215, :221, :234, :245-250)
    int len;
    u64 hash;
};
__device__ __forceinline__ Built hp_build(const HapArgs& a, const int r, const int32_t begin, const int32_t end, uint8_t* row, const int lane)
{
    const u64 HB = 0x9E3779B97F4A7C15ull; // the hash: sum of (byte + 1) * HB^index, so every lane adds its own bytes' terms
    const ReadView v = hp_view(a, r, nullptr);
    const int last = hp_last_match(v);
    bool any = false, at_begin = false, at_end = false, invalid = false;
    int total = 0;
    u64 h = 0;
    for (int64_t c0 = begin; c0 < end; c0 += 64) {
        const int64_t p = c0 + lane;
        Emit e;
        e.kind = EK_NONE;
        if (p < end) e = hp_resolve(a, v, last, p);
        const bool reg = e.kind != EK_NONE;
        bool bad = e.kind == EK_SOFT_CLIP;
        int n = 0;
        uint32_t first = 0;
        const bool with_insert = e.kind == EK_INSERT || e.kind == EK_MISMATCH_INSERT;
        if (reg && !bad && e.kind != EK_DELETE) { // getHaplotypeBase :148-167
            first = (e.kind == EK_MATCH || e.kind == EK_INSERT) ? hp_ref_char(a, p) : e.base;
            n = 1 + (with_insert ? int(e.ins_len) : 0);
            bad = first == uint32_t('N');
        }
        const int incl = hp_incl_scan(n, lane);
        const int off = total + incl - n;
        if (n > 0) {
            u64 pw = hp_pow(HB, unsigned(off));
            if (off < HP_MAX_LEN) row[off] = uint8_t(first);
            h += u64(first + 1u) * pw;
            for (int k = 1; k < n; ++k) {
                const int64_t rp = int64_t(e.ins_begin) + (k - 1);
                const uint32_t c = rp < v.L ? hp_code_char(v.code[rp]) : uint32_t('N');
                if (c == uint32_t('N')) bad = true; // haplotypeBase.find('N') :220
                pw *= HB;
                if (off + k < HP_MAX_LEN) row[off + k] = uint8_t(c);
                h += u64(c + 1u) * pw;
            }
        }
        any = any || __ballot(reg) != 0ull;
        at_begin = at_begin || __ballot(reg && p == begin) != 0ull;
        at_end = at_end || __ballot(reg && p == int64_t(end) - 1) != 0ull;
        invalid = invalid || __ballot(bad) != 0ull;
        total += __shfl(incl, 63, 64);
    }
    Built b;
    b.registered = any;
    // (longer than a read's bases: only from input the host entry refuses; the extent kernel has raised the flag)
    b.covering = at_begin && at_end && !invalid && total > 0 && total <= HP_MAX_LEN;
    b.len = total;
    b.hash = hp_wave_sum64(h) & a.hash_mask;
    return b;
}

// std::string's operator< on two LDS rows (char_traits<char>::compare is memcmp, then the shorter first): <0, 0, >0
__device__ int hp_compare(const uint8_t* x, const int nx, const uint8_t* y, const int ny)
{
    const int n = nx < ny ? nx : ny;
    for (int k = 0; k < n; ++k)
        if (x[k] != y[k]) return int(x[k]) - int(y[k]);
    return nx - ny;
}

// isFilterSecondHaplotypeAsSequencerPhasingNoise :330-414 with an empty duplicate set (on the counting path a read is in one group)
__device__ bool hp_is_phasing_noise(const uint8_t* hap1, const int n1, const uint8_t* hap2, const int n2, const int hap2_count, const int hap2_fwd_count)
{
    // doHaplotypesMeetPhasingErrorCondition1 :297-314
    if (n1 != n2) return false;
    int at = -1;
    for (int k = 0; k < n1; ++k) {
        if (hap1[k] != hap2[k]) {
            if (at >= 0) return false;
            at = k;
        }
    }
    if (at < 0) return false;
    if (hap2_fwd_count > 0 && hap2_fwd_count < hap2_count) return false; // :385
    const uint8_t base = hap2[at];
    if (hap2_fwd_count == 0) { // :392-401
        int it = at;
        for (; it != n2; ++it)
            if (hap2[it] != base) break;
        return (it - at) > HP_MIN_HPOL;
    }
    int it = at; // :402-413
    while (true) {
        if (hap2[it] != base) break;
        if (it == 0) break;
        --it;
    }
    return (at - it) > HP_MIN_HPOL;
}

__device__ __forceinline__ void hp_write_rec(sk_region_haplotypes_rec* dst, const int status, const int reason, const uint32_t aligned, const uint32_t covering)
{
    sk_region_haplotypes_rec r;
    r.status = status;
    r.reason = reason;
    r.n_reads_aligned = aligned;
    r.n_reads_covering = covering;
    r.n_selected = 0;
    r.pad = 0;
    for (int k = 0; k < SK_HAP_MAX_SELECTED; ++k) {
        r.hap[k].seq_off = r.hap[k].support_off = 0;
        r.hap[k].seq_len = r.hap[k].count = r.hap[k].is_reference = r.hap[k].pad = 0;
    }
    *dst = r;
}

// H1
__global__ __launch_bounds__(64) void hap_region_kernel(const HapArgs a)
{
    __shared__ int s_list[HP_LIST];       // the registered reads, ascending
    __shared__ u64 s_hash[HP_LIST];
    __shared__ int s_len[HP_LIST];        // the string's length, -1: not covering
    __shared__ int s_rep[HP_LIST];        // list index of the first read with the same string
    __shared__ unsigned s_cnt[HP_LIST];   // per representative: reads in the low half, forward-strand reads in the high half
    __shared__ uint8_t s_row_a[HP_MAX_LEN], s_row_b[HP_MAX_LEN];
    __shared__ uint8_t s_gstr[HP_MAX_GROUPS][HP_MAX_LEN];
    __shared__ int s_gidx[HP_MAX_GROUPS], s_glen[HP_MAX_GROUPS], s_gcnt[HP_MAX_GROUPS], s_gfwd[HP_MAX_GROUPS];
    __shared__ int s_order[HP_MAX_GROUPS], s_same[HP_MAX_GROUPS], s_sel[SK_HAP_MAX_SELECTED + 1], s_nsel;
    const int lane = threadIdx.x;
    const u64 lanes_below = (1ull << lane) - 1ull;
    int32_t n_regions = *a.n_regions;
    if (int64_t(n_regions) > a.region_cap) n_regions = int32_t(a.region_cap);
    for (int64_t slot = blockIdx.x; slot < n_regions; slot += gridDim.x) {
        __syncthreads(); // (the LDS of the slot before is done with)
        const int32_t begin = a.regions[slot].begin, end = a.regions[slot].end;
        sk_region_haplotypes_rec* rec = a.recs + slot;
        if (end <= begin) { // (the host entry refuses this)
            if (lane == 0) {
                atomicOr(a.err, unsigned(SK_DEVERR_HAPLOTYPES));
                hp_write_rec(rec, SK_HAP_BYPASSED, 0, 0, 0);
            }
            continue;
        }
        int32_t buf_begin = a.buf_begin, buf_end = a.buf_end, ploidy = a.ploidy;
        if (a.params) {
            const sk_region_params p = a.params[slot];
            buf_begin = p.buf_begin;
            buf_end = p.buf_end;
            ploidy = p.ploidy;
            if (ploidy != 1 && ploidy != 2) { // (the host entry refuses this)
                if (lane == 0) {
                    atomicOr(a.err, unsigned(SK_DEVERR_HAPLOTYPES));
                    hp_write_rec(rec, SK_HAP_BYPASSED, 0, 0, 0);
                }
                continue;
            }
        }
        // processHaplotypes :45-56
        if (begin < buf_begin || end > buf_end || int64_t(end) - begin > SK_HAP_MAX_REF_SPAN) {
            if (lane == 0) hp_write_rec(rec, SK_HAP_BYPASSED, 0, 0, 0);
            continue;
        }

        // a) the registered reads
        int n = 0, min_index = INT_MAX, max_index = -1;
        bool long_read = false;
        for (int r0 = 0; r0 < a.n_reads; r0 += 64) {
            const int r = r0 + lane;
            bool reg = false, is_long = false;
            if (r < a.n_reads) {
                const int32_t lo = a.ext[2 * r], hi = a.ext[2 * r + 1];
                if (lo <= hi && lo < end && hi >= begin) {
                    reg = hp_any_registered(a, hp_view(a, r, nullptr), begin, end);
                    is_long = reg && int64_t(hi) - lo >= HP_RING;
                }
            }
            const u64 m = __ballot(reg);
            if (m) {
                const int at = n + __popcll(m & lanes_below);
                if (reg && at < HP_LIST) s_list[at] = r;
                n += __popcll(m);
                if (min_index == INT_MAX) min_index = r0 + __builtin_ctzll(m);
                max_index = r0 + 63 - __builtin_clzll(m);
                long_read = long_read || __ballot(is_long) != 0ull;
            }
        }
        if (n == 0) { // generateHaplotypesWithCounting :86
            if (lane == 0) hp_write_rec(rec, SK_HAP_NO_READS, 0, 0, 0);
            continue;
        }
        // _variantInfo[id % 1000][pos % 1000] must name one (read, position) pair for everything the region reads
        if (max_index - min_index >= HP_RING || long_read) {
            if (lane == 0) hp_write_rec(rec, SK_HAP_DECLINED, max_index - min_index >= HP_RING ? SK_HAP_DECLINE_READ_INDEX_SPREAD : SK_HAP_DECLINE_READ_SPAN, uint32_t(n), 0);
            continue;
        }
        __syncthreads();

        // b) strings, hashes, covering
        int n_cov = 0;
        for (int i = 0; i < n; ++i) {
            const Built b = hp_build(a, s_list[i], begin, end, s_row_a, lane);
            if (lane == 0) {
                s_len[i] = b.covering ? b.len : -1;
                s_hash[i] = b.hash;
                s_cnt[i] = 0;
            }
            n_cov += b.covering ? 1 : 0;
        }
        // :91, unsigned against float * unsigned, in float as written
        if (float(n_cov) < __fmul_rn(0.65f, float(n))) {
            if (lane == 0) hp_write_rec(rec, SK_HAP_TOO_FEW_COVERING, 0, uint32_t(n), uint32_t(n_cov));
            continue;
        }
        __syncthreads();

        // c) classes (the std::map<std::string, ...> of :95-105): equal keys are confirmed byte by byte
        for (int i = 0; i < n; ++i) {
            const int len_i = s_len[i];
            if (len_i < 0) continue;
            const u64 hash_i = s_hash[i];
            int rep = i;
            bool built_i = false;
            for (int j0 = 0; j0 < i && rep == i; j0 += 64) {
                const int j = j0 + lane;
                // only a class's first read is tried: were read i equal to a later member, it would equal that first read too
                u64 m = __ballot(j < i && s_len[j] == len_i && s_hash[j] == hash_i && s_rep[j] == j);
                while (m && rep == i) {
                    const int jj = j0 + __builtin_ctzll(m);
                    m &= m - 1ull;
                    if (!built_i) {
                        (void)hp_build(a, s_list[i], begin, end, s_row_a, lane);
                        built_i = true;
                    }
                    (void)hp_build(a, s_list[jj], begin, end, s_row_b, lane);
                    __syncthreads();
                    bool differ = false;
                    for (int k = lane; k < len_i; k += 64) differ = differ || s_row_a[k] != s_row_b[k];
                    if (__ballot(differ) == 0ull) rep = jj;
                    __syncthreads();
                }
            }
            if (lane == 0) s_rep[i] = rep;
            __syncthreads();
        }
        for (int i = lane; i < n; i += 64)
            if (s_len[i] >= 0) atomicAdd(&s_cnt[s_rep[i]], 1u | (a.is_fwd[s_list[i]] ? 0x10000u : 0u));
        __syncthreads();

        // d) the haplotypes of MinHaplotypeCount reads and more (:425)
        int n_groups = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const bool q = i < n && s_len[i] >= 0 && s_rep[i] == i && (s_cnt[i] & 0xffffu) >= unsigned(HP_MIN_COUNT);
            const u64 m = __ballot(q);
            const int at = n_groups + __popcll(m & lanes_below);
            if (q && at < HP_MAX_GROUPS) s_gidx[at] = i;
            n_groups += __popcll(m);
        }
        if (n_groups > HP_MAX_GROUPS) { // std::sort's introsort would decide the order among equal counts
            if (lane == 0) hp_write_rec(rec, SK_HAP_DECLINED, SK_HAP_DECLINE_GROUPS, uint32_t(n), uint32_t(n_cov));
            continue;
        }
        __syncthreads();
        for (int g = 0; g < n_groups; ++g) {
            const int i = s_gidx[g];
            const Built b = hp_build(a, s_list[i], begin, end, s_gstr[g], lane);
            if (lane == 0) {
                s_glen[g] = b.len;
                s_gcnt[g] = int(s_cnt[i] & 0xffffu);
                s_gfwd[g] = int(s_cnt[i] >> 16);
            }
        }
        __syncthreads();
        // is each group the reference segment (_refSegment: get_substring of the region)?
        u64 ref_mask = 0;
        for (int g = 0; g < n_groups; ++g) {
            bool differ = s_glen[g] != end - begin;
            if (!differ)
                for (int k = lane; k < end - begin; k += 64) differ = differ || uint32_t(s_gstr[g][k]) != hp_ref_char(a, int64_t(begin) + k);
            if (__ballot(differ) == 0ull) ref_mask |= 1ull << g;
        }
        if (lane == 0) {
            // std::map order, then std::sort on the count alone: libstdc++'s __insertion_sort, which keeps equal counts in place (:433-437)
            for (int g = 0; g < n_groups; ++g) {
                int j = g;
                while (j > 0 && hp_compare(s_gstr[g], s_glen[g], s_gstr[s_order[j - 1]], s_glen[s_order[j - 1]]) < 0) {
                    s_order[j] = s_order[j - 1];
                    --j;
                }
                s_order[j] = g;
            }
            for (int i = 1; i < n_groups; ++i) {
                const int val = s_order[i];
                int j = i;
                while (j > 0 && s_gcnt[val] > s_gcnt[s_order[j - 1]]) {
                    s_order[j] = s_order[j - 1];
                    --j;
                }
                s_order[j] = val;
            }
            // selectHaplotypes :439-483 with selectOrDropHaplotypesWithSameCount :486-516
            int n_sel = 0, n_same = 0;
            bool is_reference_selected = false;
            auto select_or_drop = [&]() {
                if (n_same > 0) {
                    const int after = n_sel + n_same;
                    if (after <= ploidy || (after == ploidy + 1 && is_reference_selected)) {
                        for (int k = 0; k < n_same; ++k) s_sel[n_sel++] = s_same[k];
                        n_same = 0;
                    }
                }
            };
            if (n_groups > 0) {
                const int top = s_order[0];
                unsigned prev_count = 0xffffffffu;
                for (int i = 0; i < n_groups; ++i) {
                    const int g = s_order[i];
                    const unsigned count = unsigned(s_gcnt[g]);
                    if (count < prev_count) select_or_drop();
                    if (n_sel >= ploidy) break;
                    if (!hp_is_phasing_noise(s_gstr[top], s_glen[top], s_gstr[g], s_glen[g], s_gcnt[g], s_gfwd[g])) {
                        s_same[n_same++] = g;
                        if ((ref_mask >> g) & 1ull) is_reference_selected = true;
                    }
                    prev_count = count;
                }
                if (n_same > 0) select_or_drop();
            }
            s_nsel = n_sel;
        }
        __syncthreads();

        // e) the record, and the selected haplotypes into the scratch pools
        const int n_sel = s_nsel;
        if (lane == 0) hp_write_rec(rec, SK_HAP_COUNTED, 0, uint32_t(n), uint32_t(n_cov));
        bool overflow = false;
        for (int k = 0; k < n_sel; ++k) {
            const int g = s_sel[k];
            const int len = s_glen[g], cnt = s_gcnt[g];
            u64 seq_at = 0, sup_at = 0;
            if (lane == 0) {
                seq_at = atomicAdd(&a.counters[HC_SEQ], u64(len));
                sup_at = atomicAdd(&a.counters[HC_SUPPORT], u64(cnt));
            }
            seq_at = u64(__shfl((long long)seq_at, 0, 64));
            sup_at = u64(__shfl((long long)sup_at, 0, 64));
            if (seq_at + u64(len) > u64(a.seq_cap) || sup_at + u64(cnt) > u64(a.support_cap)) { // (the entry refuses caps below the bounds)
                overflow = true;
                break;
            }
            for (int b = lane; b < len; b += 64) a.tmp_seq[seq_at + b] = s_gstr[g][b];
            int written = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                const bool q = i < n && s_len[i] >= 0 && s_rep[i] == s_gidx[g];
                const u64 m = __ballot(q);
                if (q) a.tmp_support[sup_at + written + __popcll(m & lanes_below)] = s_list[i];
                written += __popcll(m);
            }
            if (lane == 0) {
                a.tmp_off[(slot * SK_HAP_MAX_SELECTED + k) * 2] = int64_t(seq_at);
                a.tmp_off[(slot * SK_HAP_MAX_SELECTED + k) * 2 + 1] = int64_t(sup_at);
                rec->hap[k].seq_len = uint32_t(len);
                rec->hap[k].count = uint32_t(cnt);
                rec->hap[k].is_reference = uint32_t((ref_mask >> g) & 1ull);
            }
        }
        if (lane == 0) {
            if (overflow) {
                atomicOr(a.err, unsigned(SK_DEVERR_HAPLOTYPES));
                hp_write_rec(rec, SK_HAP_BYPASSED, 0, 0, 0);
            } else {
                rec->n_selected = uint32_t(n_sel);
            }
        }
    }
}

// H2: region order offsets of the selected haplotypes, query_off, totals
__global__ __launch_bounds__(HP_SCAN_T) void hap_offsets_kernel(const HapArgs a, int64_t* query_off, int64_t* totals)
{
    __shared__ int64_t s[3][HP_SCAN_T];
    const int tid = threadIdx.x;
    int32_t n_regions = *a.n_regions;
    if (n_regions < 0) n_regions = 0;
    if (int64_t(n_regions) > a.region_cap) n_regions = int32_t(a.region_cap);
    int64_t carry[3] = { 0, 0, 0 }; // haplotypes, bytes, supporting reads before this chunk
    for (int64_t c0 = 0; c0 < n_regions; c0 += HP_SCAN_T) {
        const int64_t slot = c0 + tid;
        int64_t v[3] = { 0, 0, 0 };
        uint32_t n_sel = 0;
        if (slot < n_regions) {
            n_sel = a.recs[slot].n_selected;
            if (n_sel > uint32_t(SK_HAP_MAX_SELECTED)) n_sel = 0;
            v[0] = n_sel;
            for (uint32_t k = 0; k < n_sel; ++k) {
                v[1] += a.recs[slot].hap[k].seq_len;
                v[2] += a.recs[slot].hap[k].count;
            }
        }
        for (int q = 0; q < 3; ++q) s[q][tid] = v[q];
        __syncthreads();
        for (int d = 1; d < HP_SCAN_T; d <<= 1) {
            int64_t t[3];
            for (int q = 0; q < 3; ++q) t[q] = tid >= d ? s[q][tid - d] : 0;
            __syncthreads();
            for (int q = 0; q < 3; ++q) s[q][tid] += t[q];
            __syncthreads();
        }
        int64_t at[3];
        for (int q = 0; q < 3; ++q) at[q] = carry[q] + s[q][tid] - v[q];
        for (uint32_t k = 0; k < n_sel; ++k) {
            sk_selected_haplotype* h = &a.recs[slot].hap[k];
            h->seq_off = at[1];
            h->support_off = at[2];
            query_off[at[0] + k] = at[1];
            at[1] += h->seq_len;
            at[2] += h->count;
        }
        for (int q = 0; q < 3; ++q) carry[q] += s[q][HP_SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) {
        query_off[carry[0]] = carry[1];
        for (int q = 0; q < 3; ++q) totals[q] = carry[q];
    }
}

// H3
__global__ __launch_bounds__(256) void hap_copy_kernel(const HapArgs a, uint8_t* seq_pool, int32_t* support_pool)
{
    int32_t n_regions = *a.n_regions;
    if (int64_t(n_regions) > a.region_cap) n_regions = int32_t(a.region_cap);
    for (int64_t slot = blockIdx.x; slot < n_regions; slot += gridDim.x) {
        const sk_region_haplotypes_rec* rec = a.recs + slot;
        uint32_t n_sel = rec->n_selected;
        if (n_sel > uint32_t(SK_HAP_MAX_SELECTED)) n_sel = 0;
        for (uint32_t k = 0; k < n_sel; ++k) {
            const sk_selected_haplotype h = rec->hap[k];
            const int64_t seq_from = a.tmp_off[(slot * SK_HAP_MAX_SELECTED + k) * 2], sup_from = a.tmp_off[(slot * SK_HAP_MAX_SELECTED + k) * 2 + 1];
            if (h.seq_off + int64_t(h.seq_len) > a.seq_cap || h.support_off + int64_t(h.count) > a.support_cap) continue; // (cannot be: the totals are the scratch pools')
            for (uint32_t b = threadIdx.x; b < h.seq_len; b += blockDim.x) seq_pool[h.seq_off + b] = a.tmp_seq[seq_from + b];
            for (uint32_t b = threadIdx.x; b < h.count; b += blockDim.x) support_pool[h.support_off + b] = a.tmp_support[sup_from + b];
        }
    }
}

struct ScratchLayout
{
    size_t ext, counters, tmp_off, tmp_seq, tmp_support, total;
};
ScratchLayout hap_scratch_layout(const int32_t n_reads, const int64_t region_cap, const int64_t seq_cap, const int64_t support_cap)
{
    ScratchLayout s;
    size_t at = 0;
    s.ext = at;
    at += sk_align256(8 * size_t(n_reads) + 8);
    s.counters = at;
    at += 256;
    s.tmp_off = at;
    at += sk_align256(16 * size_t(SK_HAP_MAX_SELECTED) * size_t(region_cap) + 16);
    s.tmp_seq = at;
    at += sk_align256(size_t(seq_cap) + 16);
    s.tmp_support = at;
    at += sk_align256(4 * size_t(support_cap) + 16);
    s.total = at;
    return s;
}

u64 hap_hash_mask()
{
    if (const char* e = std::getenv("SK_HAP_TEST_HASH_BITS")) { // tests: a narrow hash, so that the byte comparison decides
        const int bits = std::atoi(e);
        if (bits >= 1 && bits < 64) return (1ull << bits) - 1ull;
    }
    return ~0ull;
}

} // namespace

extern "C" {

int64_t sk_region_haplotypes_seq_bound(int64_t n_regions)
{
    if (n_regions < 0) return -1;
    return n_regions * int64_t(SK_HAP_MAX_SELECTED) * int64_t(SK_PILEUP_MAX_READ_LEN);
}

int64_t sk_region_haplotypes_support_bound(int32_t n_reads, int64_t n_regions)
{
    if (n_reads < 0 || n_regions < 0) return -1;
    return n_regions * int64_t(n_reads < HP_RING ? n_reads : int32_t(HP_RING)); // a region of reads further apart is declined
}

size_t sk_region_haplotypes_scratch_bytes(int32_t n_reads, int64_t region_cap, int64_t seq_cap, int64_t support_cap)
{
    if (n_reads < 0 || region_cap < 0 || seq_cap < 0 || support_cap < 0) return 0;
    return hap_scratch_layout(n_reads, region_cap, seq_cap, support_cap).total;
}

// sk_region_haplotypes_dev and sk_region_haplotypes_params_dev: dev_params == nullptr takes (buf_begin, buf_end, ploidy) for every region
static int hap_enqueue(const std::string& who, const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* dev_read_off,
                             const uint8_t* dev_read_code, const int64_t* dev_path_off, const int32_t* dev_n_seg, const sk_path_seg* dev_path,
                             const int32_t* dev_pos, const uint8_t* dev_low_mapq, const uint8_t* dev_is_fwd_strand, const int64_t* dev_obs_off,
                             const sk_intake_obs* dev_obs, uint32_t max_indel_size, int32_t buf_begin, int32_t buf_end, int32_t ploidy, const sk_region_params* dev_params,
                             const sk_active_region* dev_regions, const int32_t* dev_n_regions, int64_t region_cap, sk_region_haplotypes_rec* dev_recs,
                             uint8_t* dev_seq_pool, int64_t seq_cap, int32_t* dev_support_pool, int64_t support_cap, int64_t* dev_query_off,
                             int64_t* dev_totals, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (n_reads < 0 || ref_len < 0 || region_cap < 0 || seq_cap < 0 || support_cap < 0) return sk_fail(who + ": negative size");
    if (region_cap > INT32_MAX) return sk_fail(who + ": region_cap beyond int32");
    if (!dev_params && ploidy != 1 && ploidy != 2) return sk_fail(who + ": ploidy must be 1 or 2");
    if (seq_cap < sk_region_haplotypes_seq_bound(region_cap)) return sk_fail(who + ": seq_cap is below sk_region_haplotypes_seq_bound");
    if (support_cap < sk_region_haplotypes_support_bound(n_reads, region_cap))
        return sk_fail(who + ": support_cap is below sk_region_haplotypes_support_bound");
    if (!dev_n_regions || !dev_query_off || !dev_totals || (ref_len > 0 && !dev_ref_seq)) return sk_fail(who + ": null argument");
    if (region_cap > 0 && (!dev_regions || !dev_recs)) return sk_fail(who + ": null argument");
    if ((seq_cap > 0 && !dev_seq_pool) || (support_cap > 0 && !dev_support_pool)) return sk_fail(who + ": null argument");
    if (n_reads > 0 && (!dev_read_off || !dev_read_code || !dev_path_off || !dev_n_seg || !dev_path || !dev_pos || !dev_low_mapq || !dev_is_fwd_strand || !dev_obs_off))
        return sk_fail(who + ": null argument");
    if (!dev_scratch || scratch_bytes < sk_region_haplotypes_scratch_bytes(n_reads, region_cap, seq_cap, support_cap))
        return sk_fail(who + ": scratch is below sk_region_haplotypes_scratch_bytes");
    if (reinterpret_cast<uintptr_t>(dev_scratch) & 15u) return sk_fail(who + ": scratch must be 16-byte aligned");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    (void)max_indel_size; // (the observations already carry it: an indel above it arrived as a breakpoint pair)
    const ScratchLayout lay = hap_scratch_layout(n_reads, region_cap, seq_cap, support_cap);
    char* scratch = static_cast<char*>(dev_scratch);
    HapArgs a;
    a.ref = dev_ref_seq;
    a.ref_offset = ref_offset;
    a.ref_len = ref_len;
    a.n_reads = n_reads;
    a.read_off = dev_read_off;
    a.read_code = dev_read_code;
    a.path_off = dev_path_off;
    a.n_seg = dev_n_seg;
    a.path = dev_path;
    a.pos = dev_pos;
    a.low_mapq = dev_low_mapq;
    a.is_fwd = dev_is_fwd_strand;
    a.obs_off = dev_obs_off;
    a.obs = dev_obs;
    a.max_indel_size = max_indel_size;
    a.buf_begin = buf_begin;
    a.buf_end = buf_end;
    a.ploidy = ploidy;
    a.params = dev_params;
    a.regions = dev_regions;
    a.n_regions = dev_n_regions;
    a.region_cap = region_cap;
    a.recs = dev_recs;
    a.ext = reinterpret_cast<int32_t*>(scratch + lay.ext);
    a.counters = reinterpret_cast<u64*>(scratch + lay.counters);
    a.tmp_off = reinterpret_cast<int64_t*>(scratch + lay.tmp_off);
    a.tmp_seq = reinterpret_cast<uint8_t*>(scratch + lay.tmp_seq);
    a.tmp_support = reinterpret_cast<int32_t*>(scratch + lay.tmp_support);
    a.seq_cap = seq_cap;
    a.support_cap = support_cap;
    a.hash_mask = hap_hash_mask();
    a.err = sk_ctx().dev_error_flags;
    SK_HIP(skrt::memsetAsync(a.counters, 0, 256, st));
    if (n_reads > 0) SK_LAUNCH(hap_extent_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, st, a);
    if (region_cap > 0) {
        const unsigned grid = unsigned(region_cap < HP_GRID ? region_cap : int64_t(HP_GRID));
        SK_LAUNCH(hap_region_kernel, dim3(grid), dim3(64), 0, st, a);
    }
    SK_LAUNCH(hap_offsets_kernel, dim3(1), dim3(HP_SCAN_T), 0, st, a, dev_query_off, dev_totals);
    if (region_cap > 0) {
        const unsigned grid = unsigned(region_cap < HP_GRID ? region_cap : int64_t(HP_GRID));
        SK_LAUNCH(hap_copy_kernel, dim3(grid), dim3(256), 0, st, a, dev_seq_pool, dev_support_pool);
    }
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_region_haplotypes_dev(const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* dev_read_off,
                             const uint8_t* dev_read_code, const int64_t* dev_path_off, const int32_t* dev_n_seg, const sk_path_seg* dev_path,
                             const int32_t* dev_pos, const uint8_t* dev_low_mapq, const uint8_t* dev_is_fwd_strand, const int64_t* dev_obs_off,
                             const sk_intake_obs* dev_obs, uint32_t max_indel_size, int32_t buf_begin, int32_t buf_end, int32_t ploidy,
                             const sk_active_region* dev_regions, const int32_t* dev_n_regions, int64_t region_cap, sk_region_haplotypes_rec* dev_recs,
                             uint8_t* dev_seq_pool, int64_t seq_cap, int32_t* dev_support_pool, int64_t support_cap, int64_t* dev_query_off,
                             int64_t* dev_totals, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    return hap_enqueue("sk_region_haplotypes_dev", dev_ref_seq, ref_offset, ref_len, n_reads, dev_read_off, dev_read_code, dev_path_off, dev_n_seg, dev_path, dev_pos, dev_low_mapq, dev_is_fwd_strand,
                       dev_obs_off, dev_obs, max_indel_size, buf_begin, buf_end, ploidy, nullptr, dev_regions, dev_n_regions, region_cap, dev_recs, dev_seq_pool, seq_cap, dev_support_pool,
                       support_cap, dev_query_off, dev_totals, dev_scratch, scratch_bytes, hip_stream);
}

int sk_region_haplotypes_params_dev(const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* dev_read_off,
                                    const uint8_t* dev_read_code, const int64_t* dev_path_off, const int32_t* dev_n_seg, const sk_path_seg* dev_path,
                                    const int32_t* dev_pos, const uint8_t* dev_low_mapq, const uint8_t* dev_is_fwd_strand, const int64_t* dev_obs_off,
                                    const sk_intake_obs* dev_obs, uint32_t max_indel_size, const sk_region_params* dev_params,
                                    const sk_active_region* dev_regions, const int32_t* dev_n_regions, int64_t region_cap, sk_region_haplotypes_rec* dev_recs,
                                    uint8_t* dev_seq_pool, int64_t seq_cap, int32_t* dev_support_pool, int64_t support_cap, int64_t* dev_query_off,
                                    int64_t* dev_totals, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (!dev_params) return sk_fail("sk_region_haplotypes_params_dev: null argument");
    return hap_enqueue("sk_region_haplotypes_params_dev", dev_ref_seq, ref_offset, ref_len, n_reads, dev_read_off, dev_read_code, dev_path_off, dev_n_seg, dev_path, dev_pos, dev_low_mapq, dev_is_fwd_strand,
                       dev_obs_off, dev_obs, max_indel_size, 0, 0, 0, dev_params, dev_regions, dev_n_regions, region_cap, dev_recs, dev_seq_pool, seq_cap, dev_support_pool,
                       support_cap, dev_query_off, dev_totals, dev_scratch, scratch_bytes, hip_stream);
}

// sk_region_haplotypes and sk_region_haplotypes_params: params == nullptr takes (buf_begin, buf_end, ploidy) for every region
static int hap_host(const std::string& who, const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* read_off, const uint8_t* read_code,
                         const int64_t* path_off, const int32_t* n_seg, const sk_path_seg* path, const int32_t* pos, const uint8_t* low_mapq,
                         const uint8_t* is_fwd_strand, const int64_t* obs_off, const sk_intake_obs* obs, uint32_t max_indel_size, int32_t buf_begin,
                         int32_t buf_end, int32_t ploidy, const sk_region_params* params, const sk_active_region* regions, int32_t n_regions, sk_region_haplotypes_rec* recs,
                         uint8_t* seq_pool, int64_t seq_cap, int32_t* support_pool, int64_t support_cap, int64_t* query_off, int64_t* totals)
{
    if (n_reads < 0 || ref_len < 0 || n_regions < 0 || seq_cap < 0 || support_cap < 0) return sk_fail(who + ": negative size");
    if (!params && ploidy != 1 && ploidy != 2) return sk_fail(who + ": ploidy must be 1 or 2");
    for (int32_t i = 0; params && i < n_regions; ++i)
        if (params[i].ploidy != 1 && params[i].ploidy != 2) return sk_fail(who + ": region " + std::to_string(i) + ": ploidy must be 1 or 2");
    if (!query_off || !totals || (ref_len > 0 && !ref_seq) || (n_regions > 0 && (!regions || !recs))) return sk_fail(who + ": null argument");
    if (n_reads > 0 && (!read_off || !read_code || !path_off || !n_seg || !path || !pos || !low_mapq || !is_fwd_strand || !obs_off))
        return sk_fail(who + ": null argument");
    int64_t n_bases = 0, n_segs = 0, n_obs = 0;
    if (n_reads > 0) {
        if (read_off[0] < 0 || path_off[0] < 0 || obs_off[0] < 0) return sk_fail(who + ": negative size (an offset below zero)");
        for (int32_t r = 0; r < n_reads; ++r) {
            const int64_t len = read_off[r + 1] - read_off[r], slots = path_off[r + 1] - path_off[r];
            const std::string where = who + ": read " + std::to_string(r) + ": ";
            if (len < 0 || slots < 0 || obs_off[r + 1] < obs_off[r]) return sk_fail(where + "negative size (offsets are not ascending)");
            if (len > SK_PILEUP_MAX_READ_LEN) return sk_fail(where + "longer than SK_PILEUP_MAX_READ_LEN");
            if (n_seg[r] < 0 || int64_t(n_seg[r]) > slots) return sk_fail(where + "n_seg beyond the read's path slots");
            if (const char* why = sk_intake_path_issue(path + path_off[r], n_seg[r], len)) return sk_fail(where + why);
        }
        n_bases = read_off[n_reads];
        n_segs = path_off[n_reads];
        n_obs = obs_off[n_reads];
    }
    if (n_obs > 0 && !obs) return sk_fail(who + ": null argument");
    for (int32_t i = 0; i < n_regions; ++i)
        if (regions[i].end <= regions[i].begin) return sk_fail(who + ": region " + std::to_string(i) + " is empty (end <= begin)");
    const int64_t seq_bound = sk_region_haplotypes_seq_bound(n_regions), support_bound = sk_region_haplotypes_support_bound(n_reads, n_regions);
    if (seq_cap < seq_bound) return sk_fail(who + ": seq_cap is below sk_region_haplotypes_seq_bound");
    if (support_cap < support_bound) return sk_fail(who + ": support_cap is below sk_region_haplotypes_support_bound");
    if ((seq_bound > 0 && !seq_pool) || (support_bound > 0 && !support_pool)) return sk_fail(who + ": null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nr = size_t(n_reads), ng = size_t(n_regions), no = n_reads > 0 ? nr + 1 : 0; // (nothing of the reads' arrays goes up without reads)
    const size_t scratch_bytes = sk_region_haplotypes_scratch_bytes(n_reads, n_regions, seq_bound, support_bound);
    struct
    {
        char* ref; int64_t* read_off; uint8_t* code; int64_t* path_off; int32_t* n_seg; sk_path_seg* path; int32_t* pos; uint8_t* low; uint8_t* fwd;
        int64_t* obs_off; sk_intake_obs* obs; sk_active_region* regions; int32_t* n_regions; sk_region_haplotypes_rec* recs; uint8_t* seq; int32_t* support;
        int64_t* query_off; char* scratch; int64_t* totals; sk_region_params* params;
    } d;
    int rc = 0;
    // (+ 16 bytes and the like: kernels read whole words past an array's end; every piece starts at a multiple of 256 bytes, which the
    // scratch's 16-byte alignment needs; sk_region_haplotypes_dev and sk_check_device_errors reserve nothing of the arena)
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(ref_seq, size_t(ref_len), 16, st, rc), ar.up(read_off, no, 1, st, rc), ar.up(read_code, size_t(n_bases), 16, st, rc),
                                ar.up(path_off, no, 1, st, rc), ar.up(n_seg, nr, 4, st, rc), ar.up(path, size_t(n_segs), 2, st, rc), ar.up(pos, nr, 4, st, rc),
                                ar.up(low_mapq, nr, 16, st, rc), ar.up(is_fwd_strand, nr, 16, st, rc), ar.up(obs_off, no, 1, st, rc),
                                ar.up(obs, size_t(n_obs), 1, st, rc), ar.up(regions, ng, 2, st, rc), ar.up(&n_regions, 1, 0, st, rc),
                                ar.take<sk_region_haplotypes_rec>(ng + 1), ar.take<uint8_t>(size_t(seq_bound) + 16), ar.take<int32_t>(size_t(support_bound) + 4),
                                ar.take<int64_t>(size_t(SK_HAP_MAX_SELECTED) * ng + 1), ar.take<char>(scratch_bytes + 16), ar.take<int64_t>(3),
                                ar.up(params, params ? ng : 0, 1, st, rc) };
        }) || rc)
        return 1;
    if (hap_enqueue(who + "_dev", d.ref, ref_offset, ref_len, n_reads, d.read_off, d.code, d.path_off, d.n_seg, d.path, d.pos, d.low, d.fwd, d.obs_off, d.obs,
                    max_indel_size, buf_begin, buf_end, ploidy, params ? d.params : nullptr, d.regions, d.n_regions, n_regions, d.recs, d.seq, seq_bound, d.support, support_bound,
                                 d.query_off, d.totals, d.scratch, scratch_bytes, st))
        return 1;
    int64_t t[3] = { 0, 0, 0 };
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    if (n_regions > 0) SK_HIP(skrt::memcpyAsync(recs, d.recs, sizeof(sk_region_haplotypes_rec) * ng, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    if (t[0] < 0 || t[0] > int64_t(SK_HAP_MAX_SELECTED) * n_regions || t[1] < 0 || t[1] > seq_bound || t[2] < 0 || t[2] > support_bound)
        return sk_fail(who + ": totals out of range");
    SK_HIP(skrt::memcpyAsync(query_off, d.query_off, 8 * size_t(t[0] + 1), hipMemcpyDeviceToHost, st));
    if (t[1] > 0) SK_HIP(skrt::memcpyAsync(seq_pool, d.seq, size_t(t[1]), hipMemcpyDeviceToHost, st));
    if (t[2] > 0) SK_HIP(skrt::memcpyAsync(support_pool, d.support, 4 * size_t(t[2]), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    for (int q = 0; q < 3; ++q) totals[q] = t[q];
    return 0;
}

int sk_region_haplotypes(const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* read_off, const uint8_t* read_code,
                         const int64_t* path_off, const int32_t* n_seg, const sk_path_seg* path, const int32_t* pos, const uint8_t* low_mapq,
                         const uint8_t* is_fwd_strand, const int64_t* obs_off, const sk_intake_obs* obs, uint32_t max_indel_size, int32_t buf_begin,
                         int32_t buf_end, int32_t ploidy, const sk_active_region* regions, int32_t n_regions, sk_region_haplotypes_rec* recs,
                         uint8_t* seq_pool, int64_t seq_cap, int32_t* support_pool, int64_t support_cap, int64_t* query_off, int64_t* totals)
{
    return hap_host("sk_region_haplotypes", ref_seq, ref_offset, ref_len, n_reads, read_off, read_code, path_off, n_seg, path, pos, low_mapq, is_fwd_strand, obs_off, obs, max_indel_size,
                    buf_begin, buf_end, ploidy, nullptr, regions, n_regions, recs, seq_pool, seq_cap, support_pool, support_cap, query_off, totals);
}

int sk_region_haplotypes_params(const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* read_off, const uint8_t* read_code,
                                const int64_t* path_off, const int32_t* n_seg, const sk_path_seg* path, const int32_t* pos, const uint8_t* low_mapq,
                                const uint8_t* is_fwd_strand, const int64_t* obs_off, const sk_intake_obs* obs, uint32_t max_indel_size,
                                const sk_region_params* params, const sk_active_region* regions, int32_t n_regions, sk_region_haplotypes_rec* recs,
                                uint8_t* seq_pool, int64_t seq_cap, int32_t* support_pool, int64_t support_cap, int64_t* query_off, int64_t* totals)
{
    if (!params) return sk_fail("sk_region_haplotypes_params: null argument");
    return hap_host("sk_region_haplotypes_params", ref_seq, ref_offset, ref_len, n_reads, read_off, read_code, path_off, n_seg, path, pos, low_mapq, is_fwd_strand, obs_off, obs, max_indel_size,
                    0, 0, 0, params, regions, n_regions, recs, seq_pool, seq_cap, support_pool, support_cap, query_off, totals);
}

} // extern "C"
