// pileup_read.h -- a section of pileup.hip: the pileup's constants and kernel arguments (PileupArgs), the segment predicates, and P1,
// `pileup_read_kernel`: one wave per read, a 16-bit record per read base.  Part of that one translation unit (its first device
// section), not a reusable interface.
#pragma once

#include "sk_common.h"

#include <climits>

namespace
{

constexpr int WAVE = 64;
constexpr int P1_WAVES = 4;
constexpr int MAX_READ_LEN = SK_PILEUP_MAX_READ_LEN;  // LDS: 4 B delta + 1 B flag per read base
constexpr unsigned REC_TIER2 = 1u << 14, REC_EMIT = 1u << 15;
constexpr unsigned REC_SUBLIVE = 1u; // (REC_EMIT clear) a live position of a submapped read: no basecall, but it counts for the MAPQ tracker
constexpr int COL_STAGE = 3072;     // calls of one wave's 64 columns staged in LDS (6 KiB); deeper spans store directly

struct PileupArgs
{
    sk_read_batch b;
    sk_pileup_options o;
    const SkTables* tab;
    uint16_t* rec;        // [n_bases]
    int2* span;           // [n_reads] {begin, end} of reads that pile up, {INT_MAX, INT_MIN} otherwise
    const int* maxend;    // [n_reads] prefix max of span.y
    const int* minbegin;  // [n_reads] suffix min of span.x
    uint32_t* count;      // [n_loci + 1]
    const int64_t* call_off;
    uint16_t* calls;
    uint32_t* spandel;
    uint32_t* submapped;
    int n_loci;
    int mode;
    int store; // 0: count, 1: store
    int r0;    // P1 handles reads [r0, n_reads): the reads before r0 kept their records from an earlier launch (pileup stream)
    // the three-column form of P2 (pileup_column3_kernel): raw tier1, raw tier2 and CleanPileupFilter'ed tier1 columns of the
    // same loci in one pass over the records, plus the MAPQ tracker (insert_mapq_count: every live match position of every read)
    uint32_t* count3[3];
    const int64_t* call_off3[3];
    uint16_t* calls3[3];
    uint32_t* mapq_count;
    uint32_t* mapq_zero;
    unsigned long long* mapq_sumsq;
    // the somatic extension of the three-column form (template flag SOM): a fourth column, CleanPileupFilter(pi, true)
    // (PileupCleaner.cpp:43-64: the tier1 calls that pass or fail only the tier1-specific filter, then the passing tier2 calls),
    // and, parallel to the raw tier1 column, each call's position in its read and the read's length
    // (updateSomaticScoringMetrics' readPos / readLength, starling_pos_processor_base.cpp:1360)
    uint32_t* count4;       // [n_loci + 1] size of the fourth column
    uint32_t* count4a;      // [n_loci + 1] ... of its tier1 part
    const int64_t* call_off4;
    uint16_t* calls4;
    uint32_t* read_pos;     // [tier1 calls] read_pos | read_size << 16, or nullptr
    // the germline EVS extension (template flag EVS): one word per live match position of every read -- submapped reads included --
    // with what updateGermlineScoringMetrics accumulates (starling_pos_processor_base.cpp:1346-1357): base id | mapq << 3 |
    // qscore << 11 | cycle << 18 | min(20, distance from the read edge) << 29 | is_submapped << 34; a locus has mapq_count of them
    const int64_t* evs_off;
    unsigned long long* evs_words;
};

__host__ __device__ __forceinline__ bool seg_match(const uint32_t t) { return t == SK_SEG_MATCH || t == SK_SEG_SEQ_MATCH || t == SK_SEG_SEQ_MISMATCH; }
__host__ __device__ __forceinline__ bool seg_read_len(const uint32_t t) { return seg_match(t) || t == SK_SEG_INSERT || t == SK_SEG_SOFT_CLIP; }
__host__ __device__ __forceinline__ bool seg_ref_len(const uint32_t t) { return seg_match(t) || t == SK_SEG_DELETE || t == SK_SEG_SKIP; }

__device__ __forceinline__ unsigned ref_code_at(const sk_read_batch& b, const int p)
{
    if (p < b.ref_offset || p >= b.ref_offset + b.ref_len) return SK_BAM_ANY; // reference_contig_segment::get_base -> 'N'
    switch (b.ref_seq[p - b.ref_offset]) {
    case 'A': return SK_BAM_A;
    case 'C': return SK_BAM_C;
    case 'G': return SK_BAM_G;
    case 'T': return SK_BAM_T;
    default: return SK_BAM_ANY;
    }
}

// the same with an unconditional load (clamped index) and selects: straight-line code for the per-position loops
__device__ __forceinline__ unsigned ref_code_at_nobranch(const sk_read_batch& b, const int p)
{
    const int i = p - b.ref_offset;
    const bool inside = (i >= 0) && (i < b.ref_len);
    const int ci = min(max(i, 0), max(b.ref_len - 1, 0));
    const unsigned c = (b.ref_len > 0) ? unsigned(b.ref_seq[ci]) : unsigned('N');
    unsigned code = SK_BAM_ANY;
    code = (c == 'A') ? unsigned(SK_BAM_A) : code;
    code = (c == 'C') ? unsigned(SK_BAM_C) : code;
    code = (c == 'G') ? unsigned(SK_BAM_G) : code;
    code = (c == 'T') ? unsigned(SK_BAM_T) : code;
    return inside ? code : unsigned(SK_BAM_ANY);
}

constexpr int FAST_K = 4; // positions per lane on the short-read path (reads up to 256 bases)

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, WAVE));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, WAVE));
    return v;
}

// P1, reads of up to 256 bases: every lane keeps its (at most four) read positions in registers -- base code, quality,
// reference position -- so the read is loaded once, the alignment path is walked once, and every record is written once.
// Same arithmetic as the general path below.
__device__ void pileup_read_short(const PileupArgs& a, const int r, const int lane, int* delta)
{
    const int64_t ro = a.b.read_off[r];
    const int L = int(a.b.read_off[r + 1] - ro);
    const int64_t so = a.b.path_off[r];
    const int nseg = int(a.b.path_off[r + 1] - so);
    const sk_path_seg* __restrict__ path = a.b.path + so;
    const int pos = a.b.pos[r];
    const bool fwd = a.b.is_fwd[r] != 0;
    const unsigned mapq = a.b.mapq[r];
    const unsigned level = a.b.map_level[r];
    const sk_pileup_options& o = a.o;

    unsigned code[FAST_K], qual[FAST_K];
#pragma unroll
    for (int k = 0; k < FAST_K; ++k) {
        const int p = lane + WAVE * k;
        code[k] = (p < L) ? a.b.read_code[ro + p] : unsigned(SK_BAM_ANY);
        qual[k] = (p < L) ? a.b.read_qual[ro + p] : 0u;
    }
    if (lane == 0) a.span[r] = make_int2(INT_MAX, INT_MIN);
    auto store_none = [&]() {
#pragma unroll
        for (int k = 0; k < FAST_K; ++k) {
            const int p = lane + WAVE * k;
            if (p < L) a.rec[ro + p] = 0;
        }
    };

    // one walk over the path: totals, edge segments, and for each of the lane's positions its segment
    int ref_len = 0, read_len_path = 0, first_match = nseg, last_match = nseg;
    bool indel_since_match = false, has_internal_indel = false; // an insertion / deletion with match segments on both sides
    int refpos[FAST_K];
    bool in_match[FAST_K];
#pragma unroll
    for (int k = 0; k < FAST_K; ++k) {
        refpos[k] = 0;
        in_match[k] = false;
    }
    for (int i = 0; i < nseg; ++i) {
        const uint32_t t = path[i].type;
        const int len = int(path[i].length);
        if (seg_match(t)) {
            if (first_match == nseg) first_match = i;
            last_match = i;
            has_internal_indel = has_internal_indel || indel_since_match;
#pragma unroll
            for (int k = 0; k < FAST_K; ++k) {
                const int p = lane + WAVE * k;
                if (p >= read_len_path && p < read_len_path + len) {
                    in_match[k] = true;
                    refpos[k] = pos + ref_len + (p - read_len_path);
                }
            }
        } else if ((t == SK_SEG_INSERT || t == SK_SEG_DELETE) && first_match != nseg) {
            indel_since_match = true;
        }
        if (seg_ref_len(t)) ref_len += len;
        if (seg_read_len(t)) read_len_path += len;
    }
    if (nseg == 0 || read_len_path != L || ref_len > L + o.largest_total_indel_ref_span_per_read || pos >= o.report_end ||
        pos + ref_len <= o.report_begin) {
        store_none();
        return;
    }
    // ambiguous read end: trailing Ns of a forward read, leading Ns of a reverse read
    int amb;
    {
        int hi_non_n = -1, lo_non_n = L;
#pragma unroll
        for (int k = 0; k < FAST_K; ++k) {
            const int p = lane + WAVE * k;
            if (p < L && code[k] != SK_BAM_ANY) {
                hi_non_n = max(hi_non_n, p);
                lo_non_n = min(lo_non_n, p);
            }
        }
        amb = fwd ? (L - 1 - wave_max(hi_non_n)) : wave_min(lo_non_n);
    }
    int read_begin = 0, read_end = L;
    if (amb > 0) {
        if (fwd) read_end -= amb;
        else read_begin += amb;
    }
    if (o.min_distance_from_read_edge > 0) {
        read_begin += o.min_distance_from_read_edge;
        if (o.min_distance_from_read_edge <= read_end) read_end -= o.min_distance_from_read_edge;
        else read_end = 0;
        if (read_end <= read_begin) {
            store_none();
            return;
        }
    }
    const bool is_submapped = !(level == SK_MAPLEVEL_TIER1 || level == SK_MAPLEVEL_TIER2);
    const bool is_tier1 = (level == SK_MAPLEVEL_TIER1);
    const bool mdf = (o.mismatch_density_flank_size > 0);
    const int fs = o.mismatch_density_flank_size, fs2 = 2 * fs;
    const int delta_size = max(1 + fs2, L) - fs2;

    bool mmk[FAST_K];
#pragma unroll
    for (int k = 0; k < FAST_K; ++k) mmk[k] = false;
    // The mismatch-density counts: +1 / -1 marks per mismatch and internal indel in the difference array, then its running sum.  Most
    // reads have neither -- every count is 0 then, and the array, its atomics and the scan (three LDS round trips and 18 shuffles) are
    // skipped for the wave.  (No measurable change on the bench's reads, 2.35 ms per 2^20 either way: P1 spends its time in the ~500
    // vector and ~470 scalar instructions per read around this, profiles/r04_v46_pileup_sq_counters.txt.)
    bool have_delta = false;
    if (!is_submapped && mdf) {
        bool any_mm = false;
#pragma unroll
        for (int k = 0; k < FAST_K; ++k) {
            const int p = lane + WAVE * k;
            const unsigned fc = ref_code_at_nobranch(a.b, refpos[k]);
            if (in_match[k] && p >= read_begin && p < read_end) {
                if (code[k] != fc) {
                    bool cand = false;
                    if (a.b.cand_snv_mask && refpos[k] >= a.b.ref_offset && refpos[k] < a.b.ref_offset + a.b.ref_len) {
                        const unsigned id = code[k] == SK_BAM_A ? 0u : code[k] == SK_BAM_C ? 1u : code[k] == SK_BAM_G ? 2u : code[k] == SK_BAM_T ? 3u : 4u;
                        cand = (id < 4u) && ((a.b.cand_snv_mask[refpos[k] - a.b.ref_offset] >> id) & 1u);
                    }
                    mmk[k] = !cand;
                    any_mm = any_mm || !cand;
                }
            }
        }
        have_delta = has_internal_indel || (__ballot(any_mm) != 0ull); // (wave-uniform)
    }
    if (have_delta) {
        for (int i = lane; i < delta_size; i += WAVE) delta[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        auto inc = [&](const int start, const int length) {
            atomicAdd(&delta[max(fs2, start) - fs2], 1);
            if (start + length < delta_size) atomicAdd(&delta[start + length], -1);
        };
        if (lane == 0 && has_internal_indel) { // internal indels
            int read_head = 0;
            for (int i = 0; i < nseg; ++i) {
                const uint32_t t = path[i].type;
                const int len = int(path[i].length);
                const bool edge = (i < first_match) || (i > last_match);
                if (t == SK_SEG_INSERT && !edge) inc(read_head, len);
                if (t == SK_SEG_DELETE && !edge) inc(read_head, 0);
                if (seg_read_len(t)) read_head += len;
            }
        }
#pragma unroll
        for (int k = 0; k < FAST_K; ++k)
            if (mmk[k]) inc(lane + WAVE * k, 1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int carry = 0;
        for (int base = 0; base < delta_size; base += WAVE) {
            const int i = base + lane;
            int v = (i < delta_size) ? delta[i] : 0;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int up = __shfl_up(v, d, WAVE);
                if (lane >= d) v += up;
            }
            v += carry;
            if (i < delta_size) delta[i] = v;
            carry = __shfl(v, WAVE - 1, WAVE);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0) a.span[r] = make_int2(pos, pos + ref_len);

    const unsigned adj_mapq = mapq < 5u ? 5u : mapq;
    const bool mapq_adjust = o.is_mapq_adjust && (adj_mapq <= 80u);
    if (is_submapped) { // (per read, hence wave-uniform) no basecalls, only the counter
#pragma unroll
        for (int k = 0; k < FAST_K; ++k) {
            const int p = lane + WAVE * k;
            const bool live = in_match[k] && p >= read_begin && p < read_end && refpos[k] >= o.report_begin && refpos[k] < o.report_end;
            if (live && a.submapped) atomicAdd(&a.submapped[refpos[k] - o.report_begin], 1u);
            if (p < L) a.rec[ro + p] = uint16_t(live ? REC_SUBLIVE : 0u);
        }
    } else {
        // straight-line per position: table and LDS reads use clamped indices, every flag is a select, and the record of a
        // position that does not emit a call is 0
        const uint8_t* __restrict__ mq = a.tab->mappedq[mapq_adjust ? adj_mapq : 0u];
#pragma unroll
        for (int k = 0; k < FAST_K; ++k) {
            const int p = lane + WAVE * k;
            const bool live = in_match[k] && p >= read_begin && p < read_end && refpos[k] >= o.report_begin && refpos[k] < o.report_end;
            const unsigned c = code[k];
            const unsigned id = c == SK_BAM_A ? 0u : c == SK_BAM_C ? 1u : c == SK_BAM_G ? 2u : c == SK_BAM_T ? 3u : 4u;
            const unsigned q0 = qual[k];
            const unsigned qm = mq[q0 > 70u ? 70u : q0];
            const unsigned q = mapq_adjust ? qm : q0;
            const bool base_filter = (c == SK_BAM_ANY) || (int(q) < o.min_basecall_qscore);
            const int del = have_delta ? delta[min(delta_size - 1, max(fs, p) - fs)] : 0; // (delta_size >= 1; no marks: every count is 0)
            const bool is_call_filter = base_filter || (mdf && o.mismatch_density_max_count < del);
            const bool is_tier2_call_filter =
                base_filter || (mdf && (o.use_tier2_evidence ? (o.tier2_mismatch_density_max_count < del) : (o.mismatch_density_max_count < del)));
            const bool nmm = mdf && (del - int(mmk[k])) > 0;
            const bool current = is_tier1 ? is_call_filter : is_tier2_call_filter;
            const bool tscf = is_tier1 && is_call_filter && !is_tier2_call_filter;
            const unsigned qb = q > 63u ? 63u : q;
            const unsigned rec = qb | (id << 6) | (fwd ? 1u << 10 : 0u) | (nmm ? 1u << 11 : 0u) | (current ? 1u << 12 : 0u) |
                                 (tscf ? 1u << 13 : 0u) | (is_tier1 ? 0u : REC_TIER2) | REC_EMIT;
            if (p < L) a.rec[ro + p] = uint16_t(live ? rec : 0u);
        }
    }
    // spanning deletions (order-free counters)
    {
        int ref_head = pos;
        for (int i = 0; i < nseg; ++i) {
            const uint32_t t = path[i].type;
            const int len = int(path[i].length);
            if (t == SK_SEG_DELETE && !((i < first_match) || (i > last_match))) {
                for (int j = lane; j < len; j += WAVE) {
                    const int refp = ref_head + j;
                    if (refp < o.report_begin || refp >= o.report_end) continue;
                    uint32_t* ctr = is_submapped ? a.submapped : a.spandel;
                    if (ctr) atomicAdd(&ctr[refp - o.report_begin], 1u);
                }
            }
            if (seg_ref_len(t)) ref_head += len;
        }
    }
}

// P1: one wave per read
__global__ __launch_bounds__(P1_WAVES* WAVE) void pileup_read_kernel(const PileupArgs a)
{
    __shared__ int s_delta[P1_WAVES][MAX_READ_LEN + 1];
    __shared__ unsigned char s_mm[P1_WAVES][MAX_READ_LEN];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / WAVE);
    const int r = a.r0 + blockIdx.x * P1_WAVES + wave;
    if (r >= a.b.n_reads) return;
    int* delta = s_delta[wave];
    unsigned char* mm = s_mm[wave];

    const int64_t ro = a.b.read_off[r];
    const int L = int(a.b.read_off[r + 1] - ro);
    if (L <= FAST_K * WAVE) {
        pileup_read_short(a, r, lane, delta);
        return;
    }
    const int64_t so = a.b.path_off[r];
    const int nseg = int(a.b.path_off[r + 1] - so);
    const sk_path_seg* __restrict__ path = a.b.path + so;
    const int pos = a.b.pos[r];
    const bool fwd = a.b.is_fwd[r] != 0;
    const unsigned mapq = a.b.mapq[r];
    const unsigned level = a.b.map_level[r];
    const sk_pileup_options& o = a.o;

    // every base starts as "not emitted"
    for (int p = lane; p < L; p += WAVE) a.rec[ro + p] = 0;
    if (lane == 0) a.span[r] = make_int2(INT_MAX, INT_MIN);

    // ---- read-level gates (:1144-1196)
    int ref_len = 0, read_len_path = 0;
    int first_match = nseg, last_match = nseg; // get_match_edge_segments
    for (int i = 0; i < nseg; ++i) {
        const uint32_t t = path[i].type;
        if (seg_ref_len(t)) ref_len += int(path[i].length);
        if (seg_read_len(t)) read_len_path += int(path[i].length);
        if (seg_match(t)) {
            if (first_match == nseg) first_match = i;
            last_match = i;
        }
    }
    if (nseg == 0 || read_len_path != L || L > MAX_READ_LEN) return; // empty alignment / malformed (host validates)
    if (ref_len > L + o.largest_total_indel_ref_span_per_read) return;
    if (pos >= o.report_end) return;
    if (pos + ref_len <= o.report_begin) return;

    // ambiguous read end (getReadAmbiguousEndLength): trailing Ns of a forward read, leading Ns of a reverse read
    int amb = 0;
    {
        const uint8_t* __restrict__ code = a.b.read_code + ro;
        if (fwd) {
            int e = L;
            while (e > 0 && code[e - 1] == SK_BAM_ANY) --e;
            amb = L - e;
        } else {
            int s = 0;
            while (s < L && code[s] == SK_BAM_ANY) ++s;
            amb = s;
        }
    }
    int read_begin = 0, read_end = L;
    if (amb > 0) {
        if (fwd) read_end -= amb;
        else read_begin += amb;
    }
    if (o.min_distance_from_read_edge > 0) {
        read_begin += o.min_distance_from_read_edge;
        if (o.min_distance_from_read_edge <= read_end) read_end -= o.min_distance_from_read_edge;
        else read_end = 0;
        if (read_end <= read_begin) return;
    }

    const bool is_submapped = !(level == SK_MAPLEVEL_TIER1 || level == SK_MAPLEVEL_TIER2);
    const bool is_tier1 = (level == SK_MAPLEVEL_TIER1);
    const bool mdf = (o.mismatch_density_flank_size > 0);
    const bool do_mdf = (!is_submapped) && mdf;
    const int fs = o.mismatch_density_flank_size, fs2 = 2 * fs;
    const int delta_size = max(1 + fs2, L) - fs2; // ddata, starling_read_util.cpp:43-56

    // ---- mismatch-density difference array (create_mismatch_filter_map :121-213)
    if (do_mdf) {
        for (int i = lane; i < delta_size; i += WAVE) delta[i] = 0;
        for (int i = lane; i < L; i += WAVE) mm[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        auto inc = [&](const int start, const int length) { // ddata::inc :58-68
            atomicAdd(&delta[max(fs2, start) - fs2], 1);
            if (start + length < delta_size) atomicAdd(&delta[start + length], -1);
        };
        int read_head = 0, ref_head = pos;
        for (int i = 0; i < nseg; ++i) {
            const uint32_t t = path[i].type;
            const int len = int(path[i].length);
            const bool edge = (i < first_match) || (i > last_match);
            if (t == SK_SEG_INSERT) {
                if (!edge && lane == 0) inc(read_head, len);
                read_head += len;
            } else if (t == SK_SEG_DELETE) {
                if (!edge && lane == 0) inc(read_head, 0);
                ref_head += len;
            } else if (seg_match(t)) {
                for (int j = lane; j < len; j += WAVE) {
                    const int rp = read_head + j;
                    if (rp < read_begin || rp >= read_end) continue;
                    const int refp = ref_head + j;
                    const unsigned rc = a.b.read_code[ro + rp];
                    const unsigned fc = ref_code_at(a.b, refp);
                    if (rc != fc) {
                        bool cand = false; // a candidate SNV of an active region does not count (:180-185)
                        if (a.b.cand_snv_mask && refp >= a.b.ref_offset && refp < a.b.ref_offset + a.b.ref_len) {
                            const unsigned id = rc == SK_BAM_A ? 0u : rc == SK_BAM_C ? 1u : rc == SK_BAM_G ? 2u : rc == SK_BAM_T ? 3u : 4u;
                            cand = (id < 4u) && ((a.b.cand_snv_mask[refp - a.b.ref_offset] >> id) & 1u);
                        }
                        if (!cand) {
                            mm[rp] = 1;
                            inc(rp, 1);
                        }
                    }
                }
                read_head += len;
                ref_head += len;
            } else if (t == SK_SEG_SOFT_CLIP) {
                read_head += len;
            } else if (t == SK_SEG_SKIP) {
                ref_head += len; // (the reference throws on N in this function; spliced reads are outside the DNA path)
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ddata::total: inclusive prefix sum, 64 entries per step
        int carry = 0;
        for (int base = 0; base < delta_size; base += WAVE) {
            const int i = base + lane;
            int v = (i < delta_size) ? delta[i] : 0;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int up = __shfl_up(v, d, WAVE);
                if (lane >= d) v += up;
            }
            v += carry;
            if (i < delta_size) delta[i] = v;
            carry = __shfl(v, WAVE - 1, WAVE);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    if (lane == 0) a.span[r] = make_int2(pos, pos + ref_len);

    // ---- records and order-free counters
    const unsigned adj_mapq = mapq < 5u ? 5u : mapq;
    const bool mapq_adjust = o.is_mapq_adjust && (adj_mapq <= 80u);
    int read_head = 0, ref_head = pos;
    for (int i = 0; i < nseg; ++i) {
        const uint32_t t = path[i].type;
        const int len = int(path[i].length);
        if (seg_match(t)) {
            for (int j = lane; j < len; j += WAVE) {
                const int rp = read_head + j;
                if (rp < read_begin || rp >= read_end) continue;
                const int refp = ref_head + j;
                if (refp < o.report_begin || refp >= o.report_end) continue;
                if (is_submapped) {
                    if (a.submapped) atomicAdd(&a.submapped[refp - o.report_begin], 1u);
                    a.rec[ro + rp] = uint16_t(REC_SUBLIVE);
                    continue;
                }
                const unsigned code = a.b.read_code[ro + rp];
                const unsigned id = code == SK_BAM_A ? 0u : code == SK_BAM_C ? 1u : code == SK_BAM_G ? 2u : code == SK_BAM_T ? 3u : 4u;
                unsigned q = a.b.read_qual[ro + rp];
                if (mapq_adjust) q = a.tab->mappedq[adj_mapq][q > 70u ? 70u : q];
                bool is_call_filter = (code == SK_BAM_ANY) || (int(q) < o.min_basecall_qscore);
                bool is_tier2_call_filter = is_call_filter;
                bool nmm = false;
                if (mdf) {
                    const int del = delta[min(delta_size - 1, max(fs, rp) - fs)]; // ddata::get :70-79
                    if (!is_call_filter) {
                        is_call_filter = (o.mismatch_density_max_count < del);
                        is_tier2_call_filter = o.use_tier2_evidence ? (o.tier2_mismatch_density_max_count < del) : is_call_filter;
                    }
                    nmm = (del - int(mm[rp])) > 0;
                }
                const bool current = is_tier1 ? is_call_filter : is_tier2_call_filter;
                const bool tscf = is_tier1 && is_call_filter && !is_tier2_call_filter;
                const unsigned qb = q > 63u ? 63u : q;
                const unsigned bc = qb | (id << 6) | (fwd ? 1u << 10 : 0u) | (nmm ? 1u << 11 : 0u) | (current ? 1u << 12 : 0u) |
                                    (tscf ? 1u << 13 : 0u);
                a.rec[ro + rp] = uint16_t(bc | (is_tier1 ? 0u : REC_TIER2) | REC_EMIT);
            }
        } else if (t == SK_SEG_DELETE) {
            const bool edge = (i < first_match) || (i > last_match); // DNA reads carry no exon pins: edge deletions are dropped
            if (!edge) {
                for (int j = lane; j < len; j += WAVE) {
                    const int refp = ref_head + j;
                    if (refp < o.report_begin || refp >= o.report_end) continue;
                    uint32_t* ctr = is_submapped ? a.submapped : a.spandel;
                    if (ctr) atomicAdd(&ctr[refp - o.report_begin], 1u);
                }
            }
        }
        if (seg_read_len(t)) read_head += len;
        if (seg_ref_len(t)) ref_head += len;
    }
}

} // namespace
