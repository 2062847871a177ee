// read_intake.hip -- the arithmetic of taking a read in: what addAlignmentIndelsToPosProcessor
// (L/starling_common/starling_pos_processor_indel_util.cpp:300-491) derives from one read that does not depend on buffer state.
//
// Input: the arrays sk_bam_decode_dev -> sk_normalize_alignments_dev leave on the device (bam_feed.hip), so the three chain on one
// stream.  Per read: the valid range (get_valid_alignment_range, L/starling_common/starling_read_util.cpp:218-329), the indel
// observations (process_simple_indel :231-296, process_swap :163-224; edge indels of genomic reads give nothing) and the returned
// total_indel_ref_span_per_read; per position of a caller-given window: the active-region detector's counters
// (ActiveRegionReadBuffer.hh:263-292, .cpp:26-107) and isCandidateVariant (.cpp:258-269).
//
//   R1  intake_read_kernel       one WAVE per read (one-wave workgroups; a workgroup takes 1 to 16 consecutive reads,
//       intake_reads_per_group).  Segment heads: a wave scan over the path, 64 segments at a time.  Per-base scores land in an LDS row of the read (forward score in the low
//       half of a word, reverse in the high half); "the reckoning" (:304-328) is then two running sums over the row in turns of 64
//       bases -- wave prefix sums with a carried offset, a min / last-arg-min for the forward sum and a max / first-arg-max of the
//       exclusive reverse sum (the reverse sum ending at k is total - P[k]).  The same pass counts the observations, sums the
//       reference span, and -- a base's match or mismatch being in a register right there -- adds the detector's counters: the reads
//       arrive sorted by position, a workgroup's reads touch a short span, which is kept in LDS (count and depth of a position as the
//       two halves of one 64-bit word) and flushed once per workgroup with 64-bit global atomics.  What falls outside the LDS span
//       goes to the global counters directly, what falls outside the window is dropped.  Integer adds only: the order does not matter.
//   R2  intake_scan_kernel<0/1>  exclusive scan of n_obs -> obs_off (per 4 096 reads, then the carry of the chunks before)
//   R3  intake_obs_kernel        a wave per read again, for the reads that have observations: walks the path as R1 does and
//       writes the records, is_noise from R1's valid range.  The bases are not read again.
//   R4  intake_candidate_kernel  a thread per position: the flag from the counters and the reference byte
//
// Out of scope (see the header): pinned edges (RNA), externally supplied candidate or forced indels, the per-read haplotype store
// (setMatch, _positionToAlignIds, getReadSegments), the repeat finder, IndelBuffer bookkeeping.
#include "sk_common.h"

#include <climits>
#include <cstdlib>
#include <vector>

namespace
{

enum {
    RI_MAX_LEN = SK_PILEUP_MAX_READ_LEN,
    RI_READS_MAX = 16, // consecutive reads per one-wave workgroup: at most this many, fewer while that keeps RI_GROUPS_WANTED workgroups
    RI_GROUPS_WANTED = 4096,
    RI_SPAN = 1024,   // positions of the counters kept in LDS per workgroup, from the first read's pos - 1
    RI_SCAN_T = 1024, // threads of a scan workgroup
    RI_SCAN_E = 4     // reads per thread
};
enum { RI_MATCH_SCORE = 2, RI_MISMATCH_SCORE = -5, RI_MIN_SEGMENT_SCORE = -11 }; // starling_read_util.cpp:224-226
enum { RI_MISMATCH_WEIGHT = 1, RI_INDEL_WEIGHT = 4, RI_MIN_NUM_VARIANTS = 9 };   // ActiveRegionReadBuffer.hh:67-80
enum { RI_MAX_CAND_FILTER_INSERT = 10 };                                         // starling_pos_processor_indel_util.cpp:70

typedef unsigned long long u64;

struct IntakeArgs
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
    uint32_t max_indel_size;
    int32_t win_begin, n_pos;
    int32_t reads_per_group;
    sk_intake_read* reads;
    int64_t* obs_off;
    sk_intake_obs* obs;
    int64_t obs_cap;
    u64* sites; // sk_intake_site as one word: variant_count in the low half, depth in the high half
    unsigned* err;
};

__host__ __device__ __forceinline__ bool ri_is_match(const uint32_t t) { return t == SK_SEG_MATCH || t == SK_SEG_SEQ_MATCH || t == SK_SEG_SEQ_MISMATCH; }
__host__ __device__ __forceinline__ bool ri_is_read_len(const uint32_t t) { return ri_is_match(t) || t == SK_SEG_INSERT || t == SK_SEG_SOFT_CLIP; }
__host__ __device__ __forceinline__ bool ri_is_ref_len(const uint32_t t) { return ri_is_match(t) || t == SK_SEG_DELETE || t == SK_SEG_SKIP; }
__host__ __device__ __forceinline__ bool ri_is_indel(const uint32_t t) { return t == SK_SEG_INSERT || t == SK_SEG_DELETE; }

// one byte through the aligned word that holds it (as the feed's kernels fetch byte-addressed data)
__device__ __forceinline__ uint32_t ri_byte(const uint8_t* p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    return (w >> (8u * unsigned(a & 3u))) & 0xffu;
}
// bam_seq::get_char of a BAM 4-bit code
__device__ __forceinline__ uint32_t ri_code_char(const uint32_t c)
{
    return c == 0u ? uint32_t('=') : c == 1u ? uint32_t('A') : c == 2u ? uint32_t('C') : c == 4u ? uint32_t('G') : c == 8u ? uint32_t('T') : uint32_t('N');
}
// reference_contig_segment::get_base
__device__ __forceinline__ uint32_t ri_ref_char(const IntakeArgs& a, const int32_t p)
{
    const int64_t k = int64_t(p) - a.ref_offset;
    return (k < 0 || k >= a.ref_len) ? uint32_t('N') : ri_byte(reinterpret_cast<const uint8_t*>(a.ref) + k);
}

__device__ __forceinline__ int ri_incl_scan(int v, const int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int ri_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int ri_wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int ri_wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// ends of get_match_edge_segments (L/blt_util/align_path.cpp:735-752): first and last match segment, n_seg for both when there is none
__device__ __forceinline__ void ri_match_edges(const sk_path_seg* p, const int ns, const int lane, int* first, int* last)
{
    int f = ns, l = ns;
    for (int c0 = 0; c0 < ns; c0 += 64) {
        const int i = c0 + lane;
        const u64 m = __ballot(i < ns && ri_is_match(p[i].type));
        if (m) {
            if (f == ns) f = c0 + __builtin_ctzll(m);
            l = c0 + 63 - __builtin_clzll(m);
        }
    }
    *first = f;
    *last = l;
}

// What the walk of addAlignmentIndelsToPosProcessor :351-488 does at segment i, which is not a match segment.
struct SegEmit
{
    int kind;          // 0 nothing, 1 one INDEL observation, 2 a BP_LEFT + BP_RIGHT pair
    uint32_t ins, del; // the indel's (a swap's: summed) insert and delete length
    uint32_t rlen;     // read length of the indel's read range (:376-401)
    uint32_t span_add; // what the segment adds to total_indel_ref_span_per_read
    bool clear_noise;  // inserts longer than max_cand_filter_insert_size are not filtered as noise
    bool soft_clip;    // an edge soft clip (:428-441)
    bool begin_edge;
};
__device__ __forceinline__ SegEmit ri_segment(const sk_path_seg* p, const int ns, const int i, const uint32_t t, const uint32_t len, const int first,
                                              const int last, const uint32_t max_indel)
{
    SegEmit e;
    e.kind = 0;
    e.ins = e.del = e.rlen = e.span_add = 0;
    e.clear_noise = e.soft_clip = false;
    e.begin_edge = i < first;
    const bool edge = i < first || i > last;
    const bool indel = ri_is_indel(t);
    // is_segment_swap_start (align_path.cpp:867-895) and swap_info (align_path_util.hh:75-103): the run of indel segments from i on
    uint32_t ins = 0, del = 0;
    bool has_ins = false, has_del = false;
    if (indel) {
        for (int j = i; j < ns; ++j) {
            const sk_path_seg s = p[j];
            if (s.type == SK_SEG_INSERT) {
                ins += s.length;
                has_ins = true;
            } else if (s.type == SK_SEG_DELETE) {
                del += s.length;
                has_del = true;
            } else {
                break;
            }
        }
    }
    const bool swap_start = has_ins && has_del;
    // a swap that is not on an edge consumes its whole run (n_seg, :446): the segments after its first are never visited
    if (indel && !edge) {
        bool bi = has_ins, bd = has_del;
        int k = i;
        while (k > 0) {
            const uint32_t tt = p[k - 1].type;
            if (tt == SK_SEG_INSERT) bi = true;
            else if (tt == SK_SEG_DELETE) bd = true;
            else break;
            --k;
        }
        if (k < i && bi && bd) return e;
    }
    if (swap_start) {
        e.rlen = ins;
        if (del <= max_indel) e.span_add = del;
    } else if (ri_is_read_len(t)) {
        e.rlen = len;
    } else if (t == SK_SEG_DELETE && len <= max_indel) {
        e.span_add = len;
    }
    if (edge) {
        e.soft_clip = t == SK_SEG_SOFT_CLIP;
        return e;
    }
    if (swap_start) {
        e.ins = ins;
        e.del = del;
        e.kind = max(ins, del) <= max_indel ? 1 : 2;
        e.clear_noise = ins > uint32_t(RI_MAX_CAND_FILTER_INSERT);
    } else if (indel) {
        e.ins = t == SK_SEG_INSERT ? len : 0u;
        e.del = t == SK_SEG_DELETE ? len : 0u;
        e.kind = len <= max_indel ? 1 : 2;
        e.clear_noise = t == SK_SEG_INSERT && len > uint32_t(RI_MAX_CAND_FILTER_INSERT);
    }
    return e;
}

// addVariantCount (count and depth) / addSoftClipCount (count alone) at `pos`
__device__ __forceinline__ void ri_add(const IntakeArgs& a, u64* s_span, const int32_t span_begin, const int32_t pos, const u64 v)
{
    const int64_t w = int64_t(pos) - a.win_begin;
    if (w < 0 || w >= a.n_pos) return;
    const int64_t k = int64_t(pos) - span_begin;
    if (k >= 0 && k < RI_SPAN) atomicAdd(&s_span[k], v);
    else atomicAdd(&a.sites[w], v);
}

__global__ __launch_bounds__(64) void intake_read_kernel(const IntakeArgs a)
{
    __shared__ u64 s_span[RI_SPAN];
    __shared__ int s_score[RI_MAX_LEN]; // forward score in the low 16 bits, reverse score in the high 16 (both small: a few adds of 2 and -5)
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * a.reads_per_group;
    const int r1 = min(a.n_reads, r0 + a.reads_per_group);
    for (int k = lane; k < RI_SPAN; k += 64) s_span[k] = 0;
    const int32_t span_begin = a.pos[r0] - 1;
    const u64 one_depth = u64(1) << 32;
    __syncthreads();
    for (int r = r0; r < r1; ++r) {
        const int64_t rb = a.read_off[r];
        const int64_t L64 = a.read_off[r + 1] - rb;
        const int ns = a.n_seg[r];
        if (L64 < 0 || L64 > RI_MAX_LEN || ns < 0) { // (the host entry refuses these; a *_dev caller hears of them from sk_check_device_errors)
            if (lane == 0) {
                atomicOr(a.err, unsigned(SK_DEVERR_INTAKE));
                sk_intake_read z;
                z.valid_begin = z.valid_end = 0;
                z.total_indel_ref_span = z.n_obs = 0;
                a.reads[r] = z;
            }
            continue;
        }
        const int L = int(L64);
        const uint8_t* code = a.read_code + rb;
        const sk_path_seg* p = a.path + a.path_off[r];
        const bool counted = a.low_mapq[r] == 0; // the detector's counters take reads that are not low-MAPQ only (:430, :463, .cpp:70)
        for (int b = lane; b < L; b += 64) s_score[b] = 0;
        int first, last;
        ri_match_edges(p, ns, lane, &first, &last);
        __syncthreads();

        int carry_read = 0;
        int32_t carry_ref = a.pos[r];
        int n_obs = 0;
        uint32_t span = 0;
        for (int c0 = 0; c0 < ns; c0 += 64) {
            const int i = c0 + lane;
            const bool act = i < ns;
            const sk_path_seg sg = act ? p[i] : sk_path_seg{ 0u, 0u };
            const uint32_t t = sg.type, len = sg.length;
            const int rl = (act && ri_is_read_len(t)) ? int(len) : 0;
            const int fl = (act && ri_is_ref_len(t)) ? int(len) : 0;
            const int rs_incl = ri_incl_scan(rl, lane), fs_incl = ri_incl_scan(fl, lane);
            const int rs = carry_read + rs_incl - rl;     // read_offset at the segment
            const int32_t fs = carry_ref + fs_incl - fl;  // ref_head_pos at the segment
            if (act && !ri_is_match(t)) {
                // get_valid_alignment_range :240-264: an insert is charged at its first base forward and its last base in reverse, a
                // deletion on the neighbouring bases (with the leading and trailing guards)
                if (t == SK_SEG_INSERT && len > 0) {
                    if (rs >= 0 && rs < L) atomicAdd(&s_score[rs], int(RI_MISMATCH_SCORE));
                    const int64_t e = int64_t(rs) + len - 1;
                    if (e >= 0 && e < L) atomicAdd(&s_score[e], int(RI_MISMATCH_SCORE) * 65536);
                } else if (t == SK_SEG_DELETE) {
                    if (rs > 0 && rs <= L) atomicAdd(&s_score[rs - 1], int(RI_MISMATCH_SCORE));
                    if (rs >= 0 && rs < L) atomicAdd(&s_score[rs], int(RI_MISMATCH_SCORE) * 65536);
                }
                const SegEmit e = ri_segment(p, ns, i, t, len, first, last, a.max_indel_size);
                n_obs += e.kind;
                span += e.span_add;
                if (counted) {
                    const u64 indel = u64(RI_INDEL_WEIGHT) | one_depth;
                    if (e.soft_clip) { // insertSoftClipSegment .cpp:33-49: at al.pos - 1 / the reference head, the bare count one position inside
                        const int32_t at = e.begin_edge ? fs - 1 : fs;
                        ri_add(a, s_span, span_begin, at, indel);
                        ri_add(a, s_span, span_begin, e.begin_edge ? at + 1 : at - 1, u64(RI_INDEL_WEIGHT));
                    } else if (e.kind == 1 && e.del == 0 && e.ins > 0) { // isPrimitiveInsertionAllele .cpp:82-88
                        ri_add(a, s_span, span_begin, fs - 1, indel);
                        ri_add(a, s_span, span_begin, fs, indel);
                    } else if (e.kind == 1 && e.ins == 0 && e.del > 0) { // isPrimitiveDeletionAllele .cpp:89-99 (inside the window only)
                        ri_add(a, s_span, span_begin, fs - 1, indel);
                        const int64_t lo = max(int64_t(fs), int64_t(a.win_begin));
                        const int64_t hi = min(int64_t(fs) + e.del, int64_t(a.win_begin) + a.n_pos);
                        for (int64_t q = lo; q < hi; ++q) ri_add(a, s_span, span_begin, int32_t(q), indel);
                    }
                }
            }
            // the match segments of this turn, one after the other, their bases across the lanes
            u64 mm = __ballot(act && ri_is_match(t));
            while (mm) {
                const int s = __builtin_ctzll(mm);
                mm &= mm - 1;
                const int srs = __shfl(rs, s, 64);
                const int32_t sfs = __shfl(fs, s, 64);
                const uint32_t slen = __shfl(len, s, 64);
                for (uint32_t j = lane; j < slen; j += 64) {
                    const int64_t rp = int64_t(srs) + j;
                    if (rp < 0 || rp >= L) break; // (a path longer than the read: refused by the host entry, flagged below)
                    const int32_t fp = sfs + int32_t(j);
                    const uint32_t rc = ri_code_char(ri_byte(code + rp));
                    const uint32_t fc = ri_ref_char(a, fp);
                    const bool differ = rc != fc; // the raw characters: '=' differs from a base, N against N is a match (:471-480)
                    if (rc != 'N' && fc != 'N') { // :274-286
                        const int sc = differ ? int(RI_MISMATCH_SCORE) : int(RI_MATCH_SCORE);
                        atomicAdd(&s_score[rp], sc + sc * 65536);
                    }
                    if (counted) ri_add(a, s_span, span_begin, fp, (differ ? u64(RI_MISMATCH_WEIGHT) : u64(0)) | one_depth);
                }
            }
            carry_read += __shfl(rs_incl, 63, 64);
            carry_ref += __shfl(fs_incl, 63, 64);
        }
        if (carry_read != L && lane == 0) atomicOr(a.err, unsigned(SK_DEVERR_INTAKE));
        n_obs = ri_wave_sum(n_obs);
        span = uint32_t(ri_wave_sum(int(span)));
        __syncthreads();

        // the reckoning :304-328 in closed form.  Forward: S = running sum; begin = 1 + the LAST index attaining min S when min S <= -11.
        // Reverse: the sum of the bases from k on is total - P[k], P the exclusive running sum; end = the FIRST index attaining max P when
        // total - max P <= -11.
        int f_carry = 0, f_min = RI_MIN_SEGMENT_SCORE, f_arg = -1;
        int r_carry = 0, r_max = INT_MIN, r_arg = 0;
        for (int t0 = 0; t0 < L; t0 += 64) {
            const int b = t0 + lane;
            const bool valid = b < L;
            const int v = valid ? s_score[b] : 0;
            const int f = int(short(v & 0xffff));
            const int rv = (v - f) >> 16;
            const int f_incl = ri_incl_scan(f, lane) + f_carry;
            const int r_incl = ri_incl_scan(rv, lane) + r_carry;
            const int r_excl = r_incl - rv;
            const int turn_min = ri_wave_min(valid ? f_incl : INT_MAX);
            if (turn_min <= f_min) {
                f_min = turn_min;
                f_arg = t0 + 63 - __builtin_clzll(__ballot(valid && f_incl == turn_min));
            }
            const int turn_max = ri_wave_max(valid ? r_excl : INT_MIN);
            if (turn_max > r_max) {
                r_max = turn_max;
                r_arg = t0 + __builtin_ctzll(__ballot(valid && r_excl == turn_max));
            }
            f_carry = __shfl(f_incl, 63, 64);
            r_carry = __shfl(r_incl, 63, 64);
        }
        int begin = f_arg + 1;
        int end = (L > 0 && r_carry - r_max <= RI_MIN_SEGMENT_SCORE) ? r_arg : L;
        if (end <= begin) begin = end = 0;
        if (lane == 0) {
            sk_intake_read o;
            o.valid_begin = begin;
            o.valid_end = end;
            o.total_indel_ref_span = span;
            o.n_obs = uint32_t(n_obs);
            a.reads[r] = o;
        }
        __syncthreads();
    }
    // one flush of the workgroup's span (what was added is inside the window: ri_add)
    for (int k = lane; k < RI_SPAN; k += 64) {
        const u64 v = s_span[k];
        if (v) atomicAdd(&a.sites[int64_t(span_begin) + k - a.win_begin], v);
    }
}

__device__ __forceinline__ int64_t ri_block_scan(const int64_t v, int64_t* s_wave, int64_t* total)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int k = 0; k < RI_SCAN_T / 64; ++k) {
        const int64_t s = s_wave[k];
        if (k < w) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + x; // inclusive
}

// R2.  PASS 0: obs_off[i] = the observations of the reads of i's chunk before i, chunk_sum[c] = the chunk's total.
//      PASS 1: + the totals of the chunks before; the last chunk writes obs_off[n_reads].
template <int PASS> __global__ __launch_bounds__(RI_SCAN_T) void intake_scan_kernel(const sk_intake_read* reads, const int32_t n_reads, int64_t* obs_off, int64_t* chunk_sum)
{
    __shared__ int64_t s_wave[RI_SCAN_T / 64];
    const int tid = threadIdx.x;
    const int64_t base = int64_t(blockIdx.x) * (RI_SCAN_T * RI_SCAN_E) + int64_t(tid) * RI_SCAN_E;
    if (PASS == 0) {
        int64_t v[RI_SCAN_E], sum = 0;
#pragma unroll
        for (int e = 0; e < RI_SCAN_E; ++e) {
            v[e] = (base + e < n_reads) ? int64_t(reads[base + e].n_obs) : 0;
            sum += v[e];
        }
        int64_t total;
        int64_t at = ri_block_scan(sum, s_wave, &total) - sum;
#pragma unroll
        for (int e = 0; e < RI_SCAN_E; ++e) {
            if (base + e < n_reads) obs_off[base + e] = at;
            at += v[e];
        }
        if (tid == 0) chunk_sum[blockIdx.x] = total;
    } else {
        int64_t mine = 0;
        for (int c = tid; c < int(blockIdx.x); c += RI_SCAN_T) mine += chunk_sum[c];
        int64_t carry;
        (void)ri_block_scan(mine, s_wave, &carry);
#pragma unroll
        for (int e = 0; e < RI_SCAN_E; ++e)
            if (base + e < n_reads) obs_off[base + e] += carry;
        if (blockIdx.x + 1 == gridDim.x && tid == 0) obs_off[n_reads] = carry + chunk_sum[blockIdx.x];
    }
}

__global__ __launch_bounds__(64) void intake_obs_kernel(const IntakeArgs a)
{
    const int lane = threadIdx.x;
    const int r0 = blockIdx.x * a.reads_per_group;
    const int r1 = min(a.n_reads, r0 + a.reads_per_group);
    for (int r = r0; r < r1; ++r) {
        const sk_intake_read rd = a.reads[r];
        if (rd.n_obs == 0) continue;
        const int L = int(a.read_off[r + 1] - a.read_off[r]);
        const int ns = a.n_seg[r];
        const sk_path_seg* p = a.path + a.path_off[r];
        const uint8_t low = a.low_mapq[r] ? 1 : 0;
        int first, last;
        ri_match_edges(p, ns, lane, &first, &last);
        int carry_read = 0;
        int32_t carry_ref = a.pos[r];
        int64_t at = a.obs_off[r];
        for (int c0 = 0; c0 < ns; c0 += 64) {
            const int i = c0 + lane;
            const bool act = i < ns;
            const sk_path_seg sg = act ? p[i] : sk_path_seg{ 0u, 0u };
            const uint32_t t = sg.type, len = sg.length;
            const int rl = (act && ri_is_read_len(t)) ? int(len) : 0;
            const int fl = (act && ri_is_ref_len(t)) ? int(len) : 0;
            const int rs_incl = ri_incl_scan(rl, lane), fs_incl = ri_incl_scan(fl, lane);
            const int rs = carry_read + rs_incl - rl;
            const int32_t fs = carry_ref + fs_incl - fl;
            SegEmit e;
            e.kind = 0;
            if (act && !ri_is_match(t)) e = ri_segment(p, ns, i, t, len, first, last, a.max_indel_size);
            const int k_incl = ri_incl_scan(e.kind, lane);
            if (e.kind) {
                // the indel's read range against the valid range (:373-402), pos_range::is_superset_of
                const int64_t range_begin = rs == 0 ? 0 : rs - 1;
                const int64_t range_end = min(int64_t(L), int64_t(rs) + 1 + e.rlen);
                bool noise = !(range_end <= rd.valid_end && range_begin >= rd.valid_begin);
                if (e.clear_noise) noise = false;
                sk_intake_obs o;
                o.read = r;
                o.pos = fs;
                o.deletion_length = 0;
                o.ins_begin = o.ins_len = o.bp_begin = o.bp_len = 0;
                o.is_noise = noise ? 1 : 0;
                o.is_low_mapq = low;
                o.pad = 0;
                const int64_t k = at + k_incl - e.kind;
                if (k + e.kind > a.obs_cap) {
                    atomicOr(a.err, unsigned(SK_DEVERR_INTAKE));
                } else if (e.kind == 1) { // :190-197, :258-271
                    o.type = SK_INDEL_INDEL;
                    o.deletion_length = e.del;
                    if (e.ins) {
                        o.ins_begin = uint32_t(rs);
                        o.ins_len = e.ins;
                    }
                    a.obs[k] = o;
                } else { // the breakpoint pair :200-220, :273-294; the windows are clipped at the read's end and start
                    const uint32_t m = a.max_indel_size;
                    const uint32_t left = min(uint32_t(L - rs), m);
                    o.type = SK_INDEL_BP_LEFT;
                    if (left) {
                        o.bp_begin = uint32_t(rs);
                        o.bp_len = left;
                    }
                    a.obs[k] = o;
                    const uint32_t next = uint32_t(rs) + e.ins;
                    const uint32_t right = min(next, m);
                    o.type = SK_INDEL_BP_RIGHT;
                    o.pos = fs + int32_t(e.del);
                    o.bp_begin = right ? next - right : 0u;
                    o.bp_len = right;
                    a.obs[k + 1] = o;
                }
            }
            at += __shfl(k_incl, 63, 64);
            carry_read += __shfl(rs_incl, 63, 64);
            carry_ref += __shfl(fs_incl, 63, 64);
        }
    }
}

// R4: isCandidateVariant .cpp:258-269, in float as written: unsigned count against float * unsigned.  The product is __fmul_rn -- a plain
// float multiply that is never contracted into the compare's operand or anything else -- and the library is built with -ffp-contract=off.
__global__ __launch_bounds__(256) void intake_candidate_kernel(const IntakeArgs a, const float min_alt_allele_fraction, uint8_t* is_candidate)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= a.n_pos) return;
    const u64 v = a.sites[i];
    const uint32_t count = uint32_t(v), depth = uint32_t(v >> 32);
    const float c = float(count), d = float(depth);
    const float by_fraction = __fmul_rn(min_alt_allele_fraction, d);
    const float by_low_depth = __fmul_rn(0.35f, d); // MinAlternativeAlleleFractionLowDepth, ActiveRegionReadBuffer.hh:84
    const bool ref_n = ri_ref_char(a, int32_t(int64_t(a.win_begin) + i)) == uint32_t('N');
    is_candidate[i] = (!ref_n && ((count >= uint32_t(RI_MIN_NUM_VARIANTS) && c >= by_fraction) || c >= by_low_depth)) ? 1 : 0;
}

// A wave takes its workgroup's reads one after the other, so a window of a few thousand reads wants a read per workgroup; a large batch
// wants many, so that the LDS span is zeroed and flushed once for all of them.  $SK_INTAKE_READS_PER_GROUP pins it (experiments).
int intake_reads_per_group(const int32_t n_reads)
{
    if (const char* e = std::getenv("SK_INTAKE_READS_PER_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64) return v;
    }
    const int v = (n_reads + RI_GROUPS_WANTED - 1) / RI_GROUPS_WANTED;
    return v < 1 ? 1 : v > RI_READS_MAX ? int(RI_READS_MAX) : v;
}

int64_t intake_chunks(const int32_t n_reads) { return (int64_t(n_reads) + RI_SCAN_T * RI_SCAN_E - 1) / (RI_SCAN_T * RI_SCAN_E); }

// get_apath_invalid_type (L/blt_util/align_path.cpp:928-997) + is_apath_starling_invalid (:1005-1013) + what the function asserts against
// or indexes outside its arrays on: nullptr when addAlignmentIndelsToPosProcessor takes the path
const char* intake_path_issue(const sk_path_seg* p, const int n, const int64_t read_len)
{
    bool is_match = false;
    uint32_t last_type = SK_SEG_NONE;
    int64_t path_read_len = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t t = p[i].type;
        if (t == SK_SEG_NONE || t > SK_SEG_SEQ_MISMATCH) return "unknown segment type in the path";
        if (i != 0 && t == last_type) return "repeated segment type in the path";
        if (t == SK_SEG_SKIP) return "a SKIP segment (spliced reads are out of scope)";
        if (t == SK_SEG_PAD) return "a PAD segment (is_apath_starling_invalid)";
        if (p[i].length == 0) return "a zero-length segment";
        if (t == SK_SEG_HARD_CLIP && !(i == 0 || i + 1 == n)) return "clipping inside the path";
        if (t == SK_SEG_SOFT_CLIP && !(i == 0 || i + 1 == n)) {
            if (i == 1) {
                if (n == 3) {
                    if (p[0].type != SK_SEG_HARD_CLIP && p[i + 1].type != SK_SEG_HARD_CLIP) return "clipping inside the path";
                } else if (p[0].type != SK_SEG_HARD_CLIP) {
                    return "clipping inside the path";
                }
            } else if (i + 2 == n) {
                if (p[i + 1].type != SK_SEG_HARD_CLIP) return "clipping inside the path";
            } else {
                return "clipping inside the path";
            }
        }
        if (ri_is_match(t)) is_match = true;
        if (ri_is_read_len(t)) path_read_len += p[i].length;
        last_type = t;
    }
    if (!is_match) return "no match segment in the path (floating)";
    if (path_read_len != read_len) return "the path's read length differs from the read_off span";
    return nullptr;
}

} // namespace

const char* sk_intake_path_issue(const sk_path_seg* path, const int n_seg, const int64_t read_len) { return intake_path_issue(path, n_seg, read_len); }

extern "C" {

void sk_intake_options_default(sk_intake_options* o)
{
    o->max_indel_size = 49;             // starling_base_shared.hh:124
    o->min_alt_allele_fraction = 0.2f;  // ActiveRegionDetector.hh:68
}

int64_t sk_read_intake_obs_bound(int64_t n_path_segments)
{
    if (n_path_segments < 0) return -1;
    return 2 * n_path_segments; // a segment gives at most a breakpoint pair
}

size_t sk_read_intake_scratch_bytes(int32_t n_reads, int64_t n_path_segments, int32_t n_pos)
{
    (void)n_path_segments;
    (void)n_pos;
    if (n_reads < 0) return 0;
    return sk_align256(8 * size_t(intake_chunks(n_reads) + 1));
}

int sk_read_intake_dev(const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* dev_read_off,
                       const uint8_t* dev_read_code, const int64_t* dev_path_off, const int32_t* dev_n_seg, const sk_path_seg* dev_path,
                       const int32_t* dev_pos, const uint8_t* dev_low_mapq, const sk_intake_options* opt, int32_t win_begin, int32_t n_pos,
                       sk_intake_read* dev_reads, int64_t* dev_obs_off, sk_intake_obs* dev_obs, int64_t obs_cap, sk_intake_site* dev_sites,
                       uint8_t* dev_is_candidate, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (n_reads < 0 || ref_len < 0 || n_pos < 0 || obs_cap < 0) return sk_fail("sk_read_intake_dev: negative size");
    if (!opt || !dev_obs_off || (ref_len > 0 && !dev_ref_seq) || (n_pos > 0 && (!dev_sites || !dev_is_candidate)))
        return sk_fail("sk_read_intake_dev: null argument");
    if (n_reads > 0 && (!dev_read_off || !dev_read_code || !dev_path_off || !dev_n_seg || !dev_path || !dev_pos || !dev_low_mapq || !dev_reads))
        return sk_fail("sk_read_intake_dev: null argument");
    if (n_reads > 0 && obs_cap > 0 && !dev_obs) return sk_fail("sk_read_intake_dev: null argument");
    if (reinterpret_cast<uintptr_t>(dev_sites) & 7u) return sk_fail("sk_read_intake_dev: sites must be 8-byte aligned");
    if (n_reads > 0 && (!dev_scratch || scratch_bytes < sk_read_intake_scratch_bytes(n_reads, 0, n_pos)))
        return sk_fail("sk_read_intake_dev: scratch is below sk_read_intake_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    IntakeArgs a;
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
    a.max_indel_size = opt->max_indel_size;
    a.win_begin = win_begin;
    a.n_pos = n_pos;
    a.reads = dev_reads;
    a.obs_off = dev_obs_off;
    a.obs = dev_obs;
    a.obs_cap = obs_cap;
    a.sites = reinterpret_cast<u64*>(dev_sites);
    a.err = sk_ctx().dev_error_flags;
    a.reads_per_group = 1;
    if (n_pos > 0) SK_HIP(skrt::memsetAsync(dev_sites, 0, sizeof(sk_intake_site) * size_t(n_pos), st));
    if (n_reads == 0) {
        SK_HIP(skrt::memsetAsync(dev_obs_off, 0, sizeof(int64_t), st));
    } else {
        a.reads_per_group = intake_reads_per_group(n_reads);
        const int groups = (n_reads + a.reads_per_group - 1) / a.reads_per_group;
        const int chunks = int(intake_chunks(n_reads));
        int64_t* chunk_sum = static_cast<int64_t*>(dev_scratch);
        SK_LAUNCH(intake_read_kernel, dim3(groups), dim3(64), 0, st, a);
        SK_LAUNCH(intake_scan_kernel<0>, dim3(chunks), dim3(RI_SCAN_T), 0, st, static_cast<const sk_intake_read*>(dev_reads), n_reads, dev_obs_off, chunk_sum);
        SK_LAUNCH(intake_scan_kernel<1>, dim3(chunks), dim3(RI_SCAN_T), 0, st, static_cast<const sk_intake_read*>(dev_reads), n_reads, dev_obs_off, chunk_sum);
        SK_LAUNCH(intake_obs_kernel, dim3(groups), dim3(64), 0, st, a);
    }
    if (n_pos > 0) SK_LAUNCH(intake_candidate_kernel, dim3((n_pos + 255) / 256), dim3(256), 0, st, a, opt->min_alt_allele_fraction, dev_is_candidate);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_read_intake(const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t n_reads, const int64_t* read_off, const uint8_t* read_code,
                   const int64_t* path_off, const int32_t* n_seg, const sk_path_seg* path, const int32_t* pos, const uint8_t* low_mapq,
                   const sk_intake_options* opt, int32_t win_begin, int32_t n_pos, sk_intake_read* reads, int64_t* obs_off, sk_intake_obs* obs,
                   int64_t obs_cap, sk_intake_site* sites, uint8_t* is_candidate)
{
    if (n_reads < 0 || ref_len < 0 || n_pos < 0 || obs_cap < 0) return sk_fail("sk_read_intake: negative size");
    if (!opt || !obs_off || (ref_len > 0 && !ref_seq) || (n_pos > 0 && (!sites || !is_candidate))) return sk_fail("sk_read_intake: null argument");
    if (n_reads > 0 && (!read_off || !read_code || !path_off || !n_seg || !path || !pos || !low_mapq || !reads)) return sk_fail("sk_read_intake: null argument");
    int64_t n_bases = 0, n_segs = 0;
    if (n_reads > 0) {
        if (read_off[0] < 0 || path_off[0] < 0) return sk_fail("sk_read_intake: negative size (an offset below zero)");
        for (int32_t r = 0; r < n_reads; ++r) {
            const int64_t len = read_off[r + 1] - read_off[r], slots = path_off[r + 1] - path_off[r];
            const std::string where = "sk_read_intake: read " + std::to_string(r) + ": ";
            if (len < 0 || slots < 0) return sk_fail(where + "negative size (offsets are not ascending)");
            if (len > SK_PILEUP_MAX_READ_LEN) return sk_fail(where + "longer than SK_PILEUP_MAX_READ_LEN");
            if (n_seg[r] < 0 || int64_t(n_seg[r]) > slots) return sk_fail(where + "n_seg beyond the read's path slots");
            if (const char* why = intake_path_issue(path + path_off[r], n_seg[r], len)) return sk_fail(where + why);
        }
        n_bases = read_off[n_reads];
        n_segs = path_off[n_reads];
    }
    const int64_t bound = sk_read_intake_obs_bound(n_segs);
    if (obs_cap < bound) return sk_fail("sk_read_intake: obs_cap is below sk_read_intake_obs_bound");
    if (bound > 0 && !obs) return sk_fail("sk_read_intake: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nr = size_t(n_reads), no = n_reads > 0 ? nr + 1 : 0; // (nothing of the reads' arrays goes up without reads)
    const size_t scratch_bytes = sk_read_intake_scratch_bytes(n_reads, n_segs, n_pos);
    struct
    {
        char* ref; int64_t* read_off; uint8_t* code; int64_t* path_off; int32_t* n_seg; sk_path_seg* path; int32_t* pos; uint8_t* low;
        sk_intake_read* reads; int64_t* obs_off; sk_intake_obs* obs; sk_intake_site* sites; uint8_t* cand; char* scratch;
    } d;
    int rc = 0;
    // (+ 16 bytes and the like: kernels read whole words past an array's end; sk_read_intake_dev reserves nothing of the arena)
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(ref_seq, size_t(ref_len), 16, st, rc), ar.up(read_off, no, 1, st, rc), ar.up(read_code, size_t(n_bases), 16, st, rc),
                                ar.up(path_off, no, 1, st, rc), ar.up(n_seg, nr, 4, st, rc), ar.up(path, size_t(n_segs), 2, st, rc), ar.up(pos, nr, 4, st, rc),
                                ar.up(low_mapq, nr, 16, st, rc), ar.take<sk_intake_read>(nr + 1), ar.take<int64_t>(nr + 1), ar.take<sk_intake_obs>(size_t(bound) + 1),
                                ar.take<sk_intake_site>(size_t(n_pos) + 2), ar.take<uint8_t>(size_t(n_pos) + 16), ar.take<char>(scratch_bytes + 16) };
        }) || rc)
        return 1;
    if (sk_read_intake_dev(d.ref, ref_offset, ref_len, n_reads, d.read_off, d.code, d.path_off, d.n_seg, d.path, d.pos, d.low, opt, win_begin, n_pos, d.reads,
                           d.obs_off, d.obs, bound, d.sites, d.cand, d.scratch, scratch_bytes, st))
        return 1;
    if (n_reads > 0) SK_HIP(skrt::memcpyAsync(reads, d.reads, sizeof(sk_intake_read) * nr, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::memcpyAsync(obs_off, d.obs_off, 8 * (nr + 1), hipMemcpyDeviceToHost, st));
    if (n_pos > 0) {
        SK_HIP(skrt::memcpyAsync(sites, d.sites, sizeof(sk_intake_site) * size_t(n_pos), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(is_candidate, d.cand, size_t(n_pos), hipMemcpyDeviceToHost, st));
    }
    SK_HIP(skrt::streamSynchronize(st));
    const int64_t total = obs_off[n_reads];
    if (total < 0 || total > bound) return sk_fail("sk_read_intake: observation count out of range");
    if (total > 0) {
        SK_HIP(skrt::memcpyAsync(obs, d.obs, sizeof(sk_intake_obs) * size_t(total), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::streamSynchronize(st));
    }
    return 0;
}

} // extern "C"
