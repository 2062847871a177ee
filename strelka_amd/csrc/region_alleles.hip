// region_alleles.hip -- from each region's selected haplotypes to its candidate alleles: ActiveRegionProcessor::processSelectedHaplotypes
// (L/starling_common/ActiveRegionProcessor.cpp:518-571), discoverIndelsAndMismatches (:573-707) and
// processDiscoveredIndelsAndMismatches (:709-757), for every region of the list, from what region_haplotypes.hip leaves.
//
//   A0  alleles_plan_kernel     one workgroup: per region its alternates (the selected haplotypes that are not the reference segment,
//       at most two), a scan placing their alignment problems -- query_off / ref_off of the aligner's CSR, the problem count -- in
//       region order; _prevActiveRegionEnd after the last region
//   A1  alleles_gather_kernel   a workgroup per problem (the grid sized by 2 * region_cap, leaving at the count): the haplotype's bytes
//       and the region's reference segment (N outside the reference) into the CSR
//   D1  global_align_kernel     (global_align.hip) over the same grid, its problem count read from device memory
//   A2  alleles_region_kernel   one WAVE per region slot (one-wave workgroups striding over region_cap slots, leaving at *n_regions).
//       a) per alternate the walk of :593-706: a lane per path segment, the reference position and haplotype offset of each by a wave
//          prefix sum; a segment's keys (csrc/alleles_core.h, the statement the host's sk_discover_indels_and_mismatches walks too)
//          are placed in path order by a second prefix sum, at the region's own room in scratch
//       b) the distinct MISMATCH keys (:525-554) and each record's first equal earlier record: an LDS table over (position, base)
//          of the region's at most 250 positions holding the lowest record index, filled by atomicMin during the walk; indel keys, and
//          mismatches the table does not hold (a base other than ACGT, a position outside the region), by a wave-wide search of the
//          earlier records
//       c) doNotAddMismatchesToIndelBuffer (:553-560); haplotypeId and altAlleleHaplotypeCountRatio as the additions of :750-755
//          leave them, by one lane in record order (float additions are ordered); the decline rules
//   A3  alleles_offsets_kernel  one workgroup: region order offsets of the records and insert bytes (a scan), totals
//   A4  alleles_copy_kernel     scratch -> the outputs at those offsets, so the layout does not depend on workgroup timing
//
// Out of scope (see the header): routing, addIndelObservation / addCandidateSnv themselves, the assembly fallback,
// doNotUseHaplotyping's marks, _haplotypesToExclude and the somatic branch, the multi-sample synchroniser,
// filterOutConflictingForcedIndels.
#include "sk_common.h"

#include "alleles_core.h"

#include <climits>

namespace
{

typedef unsigned long long u64;

enum {
    RA_MAX_LEN = 1024,                  // the aligner's limit on a query
    RA_MAX_SPAN = SK_HAP_MAX_REF_SPAN,
    RA_TABLE_POS = RA_MAX_SPAN, // the aligner emits no SOFT_CLIP, so a MISMATCH key lies inside the region; one that did not would go to the search
    RA_GRID = 2048,
    RA_SCAN_T = 1024
};
constexpr unsigned RA_NONE = 0xffffffffu;

struct RaArgs
{
    const char* ref;
    int32_t ref_offset, ref_len;
    const sk_active_region* regions;
    const int32_t* n_regions;
    int64_t region_cap;
    const sk_region_haplotypes_rec* hap;
    const uint8_t* seq;
    int64_t seq_cap;
    uint32_t max_indel_size;
    int32_t max_hap_len, prev_end_in;
    sk_region_alleles_rec* recs;
    int64_t allele_cap, insert_cap;
    // scratch
    int32_t* n_prob;       // the alignment problems
    int32_t* prob0;        // per region slot: its first problem
    int32_t* prob_src;     // per problem: slot * 4 + the haplotype's k
    int64_t* q_off;        // the aligner's CSR
    int64_t* r_off;
    char* query;
    char* ref_copy;
    int32_t* score;        // the aligner's outputs
    int32_t* begin;
    int32_t* nseg;
    sk_path_seg* path;
    sk_region_allele* tmp_alleles; // per region slot room for 2 * (RA_MAX_SPAN + max_hap_len) records ...
    uint8_t* tmp_ins;              // ... and 2 * max_hap_len insert bytes
    unsigned* err;
    int32_t ids_twice; // sk_debug_region_alleles: tests only
};

__device__ __forceinline__ int32_t ra_n_regions(const RaArgs& a)
{
    int32_t n = *a.n_regions;
    if (n < 0) n = 0;
    if (int64_t(n) > a.region_cap) n = int32_t(a.region_cap);
    return n;
}
__device__ __forceinline__ int64_t ra_region_alleles(const RaArgs& a) { return 2 * (int64_t(RA_MAX_SPAN) + a.max_hap_len); }
__device__ __forceinline__ int64_t ra_region_ins(const RaArgs& a) { return 2 * int64_t(a.max_hap_len); }

// What becomes of a region before any alignment
enum { PL_PASS = 0, PL_ALIGN, PL_TOO_LONG, PL_BAD };
struct Plan
{
    int kind;
    int n_alt;
    int k0, k1; // the alternates' slots in the haplotype record
};
__device__ __forceinline__ Plan ra_plan(const RaArgs& a, const int64_t slot)
{
    const sk_region_haplotypes_rec* h = a.hap + slot;
    Plan p;
    p.kind = PL_PASS;
    p.n_alt = 0;
    p.k0 = p.k1 = 0;
    if (h->status != SK_HAP_COUNTED || h->n_selected == 0u) return p; // the status passes through
    p.kind = PL_BAD;                                                  // (what the host entry refuses)
    if (h->n_selected > uint32_t(SK_HAP_MAX_SELECTED)) return p;
    const int64_t span = int64_t(a.regions[slot].end) - a.regions[slot].begin;
    if (span < 1 || span > RA_MAX_SPAN) return p;
    bool too_long = false;
    for (uint32_t k = 0; k < h->n_selected; ++k) {
        const sk_selected_haplotype* s = &h->hap[k];
        if (s->seq_off < 0 || s->seq_len == 0u || s->seq_off + int64_t(s->seq_len) > a.seq_cap) return p;
        if (s->is_reference) continue; // haplotype != _refSegment (:529)
        if (p.n_alt == SK_ALLELE_MAX_ALT) return p;
        if (p.n_alt == 0) p.k0 = int(k);
        else p.k1 = int(k);
        ++p.n_alt;
        too_long = too_long || s->seq_len > uint32_t(a.max_hap_len);
    }
    p.kind = too_long ? PL_TOO_LONG : PL_ALIGN;
    return p;
}

// A0
__global__ __launch_bounds__(RA_SCAN_T) void alleles_plan_kernel(const RaArgs a, int32_t* prev_end_out)
{
    __shared__ int64_t s[3][RA_SCAN_T];
    const int tid = threadIdx.x;
    const int32_t n_regions = ra_n_regions(a);
    int64_t carry[3] = { 0, 0, 0 }; // problems, query bytes, reference bytes before this chunk
    for (int64_t c0 = 0; c0 < n_regions; c0 += RA_SCAN_T) {
        const int64_t slot = c0 + tid;
        int64_t v[3] = { 0, 0, 0 };
        Plan pl;
        pl.kind = PL_PASS;
        pl.n_alt = 0;
        pl.k0 = pl.k1 = 0;
        int64_t span = 0;
        if (slot < n_regions) {
            pl = ra_plan(a, slot);
            if (pl.kind == PL_BAD) atomicOr(a.err, unsigned(SK_DEVERR_ALLELES));
            if (pl.kind != PL_ALIGN) pl.n_alt = 0;
            span = int64_t(a.regions[slot].end) - a.regions[slot].begin;
            v[0] = pl.n_alt;
            for (int j = 0; j < pl.n_alt; ++j) v[1] += a.hap[slot].hap[j ? pl.k1 : pl.k0].seq_len;
            v[2] = pl.n_alt * span;
        }
        for (int q = 0; q < 3; ++q) s[q][tid] = v[q];
        __syncthreads();
        for (int d = 1; d < RA_SCAN_T; d <<= 1) {
            int64_t t[3];
            for (int q = 0; q < 3; ++q) t[q] = tid >= d ? s[q][tid - d] : 0;
            __syncthreads();
            for (int q = 0; q < 3; ++q) s[q][tid] += t[q];
            __syncthreads();
        }
        int64_t at[3];
        for (int q = 0; q < 3; ++q) at[q] = carry[q] + s[q][tid] - v[q];
        if (slot < n_regions) a.prob0[slot] = int32_t(at[0]);
        for (int j = 0; j < pl.n_alt; ++j) {
            const int64_t p = at[0] + j;
            const int k = j ? pl.k1 : pl.k0;
            a.q_off[p] = at[1];
            a.r_off[p] = at[2];
            a.prob_src[p] = int32_t(slot * 4 + k);
            at[1] += a.hap[slot].hap[k].seq_len;
            at[2] += span;
        }
        for (int q = 0; q < 3; ++q) carry[q] += s[q][RA_SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) {
        a.q_off[carry[0]] = carry[1];
        a.r_off[carry[0]] = carry[2];
        *a.n_prob = int32_t(carry[0]);
        *prev_end_out = n_regions > 0 ? a.regions[n_regions - 1].end : a.prev_end_in; // ActiveRegionDetector.cpp:248
    }
}

// A1
__global__ __launch_bounds__(256) void alleles_gather_kernel(const RaArgs a)
{
    const int32_t n_prob = *a.n_prob;
    for (int64_t p = blockIdx.x; p < n_prob; p += gridDim.x) {
        const int32_t src = a.prob_src[p];
        const int64_t slot = src >> 2;
        const sk_selected_haplotype h = a.hap[slot].hap[src & 3];
        char* q = a.query + a.q_off[p];
        for (uint32_t i = threadIdx.x; i < h.seq_len; i += blockDim.x) q[i] = char(a.seq[h.seq_off + i]);
        const int32_t begin = a.regions[slot].begin;
        const int32_t span = int32_t(a.r_off[p + 1] - a.r_off[p]);
        char* r = a.ref_copy + a.r_off[p];
        for (int32_t i = threadIdx.x; i < span; i += blockDim.x) { // _refSegment: get_substring of the region, N outside the segment
            const int64_t k = int64_t(begin) + i - a.ref_offset;
            r[i] = (k < 0 || k >= a.ref_len) ? 'N' : a.ref[k];
        }
    }
}

__device__ __forceinline__ int ra_incl_scan(int v, const int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int ra_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int ra_base_code(const uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
// what one wave wrote to global memory, read by its other lanes
__device__ __forceinline__ void ra_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__device__ __forceinline__ void ra_write_rec(sk_region_alleles_rec* dst, const int status, const int reason, const int32_t prev_end)
{
    sk_region_alleles_rec r;
    r.status = status;
    r.reason = reason;
    r.prev_end = prev_end;
    r.n_alt = r.n_alleles = r.n_indels = r.n_distinct_mismatches = r.do_not_add_mismatches = 0;
    r.allele_off = r.insert_off = 0;
    r.n_insert_bytes = r.pad = 0;
    r.score[0] = r.score[1] = 0;
    r.hap_slot[0] = r.hap_slot[1] = 0;
    *dst = r;
}

// A2
__global__ __launch_bounds__(64) void alleles_region_kernel(const RaArgs a)
{
    __shared__ unsigned s_first[RA_TABLE_POS * 4]; // (position - begin, base) -> the region's first MISMATCH record with that key
    const int lane = threadIdx.x;
    const int32_t n_regions = ra_n_regions(a);
    const int64_t per_region = ra_region_alleles(a), per_ins = ra_region_ins(a);
    // nothing is truncated: room below the bound of the regions there are is refused as a whole
    const bool cap_ok = a.allele_cap >= n_regions * per_region && a.insert_cap >= n_regions * per_ins;
    for (int64_t slot = blockIdx.x; slot < n_regions; slot += gridDim.x) {
        __syncthreads(); // (the LDS of the slot before is done with)
        const int32_t begin = a.regions[slot].begin, end = a.regions[slot].end;
        const int32_t prev_end = slot == 0 ? a.prev_end_in : a.regions[slot - 1].end; // ActiveRegionDetector.cpp:248
        const sk_region_haplotypes_rec* h = a.hap + slot;
        sk_region_alleles_rec* rec = a.recs + slot;
        const Plan pl = ra_plan(a, slot);
        if (!cap_ok || pl.kind == PL_BAD) {
            if (lane == 0) {
                atomicOr(a.err, unsigned(SK_DEVERR_ALLELES));
                ra_write_rec(rec, SK_HAP_BYPASSED, 0, prev_end);
            }
            continue;
        }
        if (pl.kind == PL_PASS) {
            if (lane == 0) ra_write_rec(rec, h->status, h->reason, prev_end);
            continue;
        }
        if (pl.kind == PL_TOO_LONG) {
            if (lane == 0) ra_write_rec(rec, SK_HAP_DECLINED, SK_ALLELE_DECLINE_HAP_LEN, prev_end);
            continue;
        }
        const int span = end - begin;
        const int table_n = span * 4;
        for (int i = lane; i < table_n; i += 64) s_first[i] = RA_NONE;
        __syncthreads();

        // a) the walk, alternate by alternate
        sk_region_allele* out = a.tmp_alleles + slot * per_region;
        uint8_t* out_ins = a.tmp_ins + slot * per_ins;
        int n = 0, nb = 0, ni = 0, decline = 0;
        bool bad = false;
        int32_t score0 = 0, score1 = 0;
        const int32_t p0 = a.prob0[slot];
        for (int j = 0; j < pl.n_alt && !decline && !bad; ++j) {
            const int64_t p = int64_t(p0) + j;
            const int kj = j ? pl.k1 : pl.k0;
            const sk_selected_haplotype hp = h->hap[kj];
            if (j) score1 = a.score[p];
            else score0 = a.score[p];
            if (a.begin[p] > 0) { // the reference asserts (:596-599)
                decline = SK_ALLELE_DECLINE_BEGIN_POS;
                break;
            }
            const int64_t qo = a.q_off[p], ro = a.r_off[p];
            const skalleles::Walk w = { a.ref, a.ref_offset, a.ref_len, end, prev_end, a.max_indel_size, a.query + qo, int32_t(hp.seq_len) };
            const sk_path_seg* path = a.path + qo + ro + 4 * p;
            const int ns = a.nseg[p];
            const float ratio = __fdiv_rn(float(hp.count), float(h->n_reads_aligned)); // (:719)
            int ref_pos = begin, hap_off = 0;
            for (int c0 = 0; c0 < ns; c0 += 64) {
                const int i = c0 + lane;
                const bool valid = i < ns;
                uint32_t type = SK_SEG_NONE, len = 0;
                int32_t dr = 0, dh = 0;
                if (valid) {
                    type = path[i].type;
                    len = path[i].length;
                    (void)skalleles::advance(type, len, &dr, &dh);
                }
                const int incl_r = ra_incl_scan(dr, lane), incl_h = ra_incl_scan(dh, lane);
                const int my_ref = ref_pos + incl_r - dr, my_hap = hap_off + incl_h - dh;
                skalleles::Seg s;
                s.d_ref = s.d_hap = s.n_keys = s.n_ins = s.n_indels = s.pos = s.shift = 0;
                s.err = skalleles::ERR_NONE;
                if (valid) s = skalleles::segment(w, type, len, my_ref, my_hap);
                if (__ballot(s.err == skalleles::ERR_PATH || s.err == skalleles::ERR_SEGMENT) != 0ull) { // (not from the aligner's paths)
                    bad = true;
                    break;
                }
                if (__ballot(s.err == skalleles::ERR_LEFT_SHIFT) != 0ull) {
                    decline = SK_ALLELE_DECLINE_LEFT_SHIFT;
                    break;
                }
                const int incl_k = ra_incl_scan(s.n_keys, lane), incl_b = ra_incl_scan(s.n_ins, lane);
                const int tot_k = __shfl(incl_k, 63, 64), tot_b = __shfl(incl_b, 63, 64);
                if (n + tot_k > per_region || nb + tot_b > per_ins) { // (cannot be: the bounds' derivation)
                    bad = true;
                    break;
                }
                const int at = n + incl_k - s.n_keys;
                int bat = nb + incl_b - s.n_ins;
                for (int q = 0; q < s.n_keys; ++q) {
                    int32_t key_pos, key_type;
                    uint32_t del_len, ins_len;
                    skalleles::key(w, type, len, my_ref, my_hap, s, q, &key_pos, &key_type, &del_len, &ins_len, reinterpret_cast<char*>(out_ins) + bat);
                    sk_region_allele* r = out + at + q;
                    r->pos = key_pos;
                    r->type = key_type;
                    r->del_len = del_len;
                    r->ins_len = ins_len;
                    r->ins_off = bat;
                    r->hap_slot = kj;
                    r->haplotype_id = j + 1; // (:562-570)
                    r->ratio = ratio;
                    r->to_indel_buffer = 1;
                    r->same_as = -1;
                    r->id_sum = 0;
                    r->ratio_sum = 0.0f;
                    r->pad = 0;
                    if (key_type == SK_INDEL_MISMATCH) {
                        const int code = ra_base_code(uint8_t(w.hap[my_hap + s.shift + q]));
                        const int64_t rel = int64_t(key_pos) - begin;
                        if (code >= 0 && rel >= 0 && rel * 4 < table_n) atomicMin(&s_first[rel * 4 + code], unsigned(at + q));
                    }
                    bat += int(ins_len);
                }
                n += tot_k;
                nb += tot_b;
                ni += ra_wave_sum(s.n_indels);
                ref_pos += __shfl(incl_r, 63, 64);
                hap_off += __shfl(incl_h, 63, 64);
            }
        }
        if (bad) {
            if (lane == 0) {
                atomicOr(a.err, unsigned(SK_DEVERR_ALLELES));
                ra_write_rec(rec, SK_HAP_BYPASSED, 0, prev_end);
            }
            continue;
        }
        if (decline) {
            if (lane == 0) ra_write_rec(rec, SK_HAP_DECLINED, decline, prev_end);
            continue;
        }
        ra_wave_fence();
        __syncthreads();

        // b) the distinct MISMATCH keys over the alternates (mismatchSet, :525-554), and each record's first equal earlier record
        int nd = 0;
        for (int i = lane; i < table_n; i += 64) nd += s_first[i] != RA_NONE ? 1 : 0;
        nd = ra_wave_sum(nd);
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int i = c0 + lane;
            int same = -1;
            bool searched = false; // an indel key, or a mismatch the table does not hold
            if (i < n) {
                const sk_region_allele* r = out + i;
                searched = true;
                if (r->type == SK_INDEL_MISMATCH) {
                    const int code = ra_base_code(out_ins[r->ins_off]);
                    const int64_t rel = int64_t(r->pos) - begin;
                    if (code >= 0 && rel >= 0 && rel * 4 < table_n) {
                        const unsigned f = s_first[rel * 4 + code];
                        same = f < unsigned(i) ? int(f) : -1;
                        searched = false;
                    }
                }
            }
            u64 todo = __ballot(searched);
            while (todo) {
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int ii = c0 + src;
                const sk_region_allele* t = out + ii;
                const int32_t t_pos = t->pos, t_type = t->type;
                const uint32_t t_del = t->del_len, t_ins = t->ins_len;
                const int64_t t_off = t->ins_off;
                int found = -1;
                for (int j0 = 0; j0 < ii && found < 0; j0 += 64) {
                    const int jx = j0 + lane;
                    bool eq = false;
                    if (jx < ii) { // IndelKey::operator== (L/starling_common/IndelKey.hh:79-85)
                        const sk_region_allele* o = out + jx;
                        eq = o->pos == t_pos && o->type == t_type && o->del_len == t_del && o->ins_len == t_ins;
                        const int64_t o_off = o->ins_off;
                        for (uint32_t b = 0; eq && b < t_ins; ++b) eq = out_ins[o_off + b] == out_ins[t_off + b];
                    }
                    const u64 m = __ballot(eq);
                    if (m) found = j0 + __builtin_ctzll(m);
                }
                if (lane == src) same = found;
                if (found < 0 && t_type == SK_INDEL_MISMATCH) ++nd;
            }
            if (i < n) out[i].same_as = same;
        }

        // c) :553-560, then what :731 and :750-755 leave per key
        const bool do_not_add = ni == 0 || nd > SK_ALLELE_MAX_MISMATCHES;
        for (int i = lane; i < n; i += 64) {
            sk_region_allele* r = out + i;
            const int to = (do_not_add && r->type == SK_INDEL_MISMATCH) ? 0 : 1;
            r->to_indel_buffer = to;
            if (to && r->same_as < 0) {
                r->id_sum = r->haplotype_id;
                r->ratio_sum = r->ratio; // 0.0f + ratio
            }
        }
        ra_wave_fence();
        int over = 0; // lane 0's: a sum above 3 (the assertion at :752)
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int i = c0 + lane;
            int same = -1, hid = 0;
            float ratio = 0.0f;
            if (i < n) {
                const sk_region_allele* r = out + i;
                if (r->to_indel_buffer) same = r->same_as;
                hid = r->haplotype_id;
                ratio = r->ratio;
            }
            u64 todo = __ballot(same >= 0);
            while (todo) { // in record order
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int first = __shfl(same, src, 64), id = __shfl(hid, src, 64);
                const float rt = __shfl(ratio, src, 64);
                if (lane == 0) {
                    const int sum = out[first].id_sum + (a.ids_twice ? 2 * id : id);
                    out[first].id_sum = sum;
                    out[first].ratio_sum = __fadd_rn(out[first].ratio_sum, rt);
                    over |= sum > 3 ? 1 : 0;
                }
            }
        }
        over = __shfl(over, 0, 64);
        if (lane == 0) {
            if (over) {
                ra_write_rec(rec, SK_HAP_DECLINED, SK_ALLELE_DECLINE_ID_SUM, prev_end);
            } else {
                sk_region_alleles_rec r;
                r.status = SK_HAP_COUNTED;
                r.reason = 0;
                r.prev_end = prev_end;
                r.n_alt = uint32_t(pl.n_alt);
                r.n_alleles = uint32_t(n);
                r.n_indels = uint32_t(ni);
                r.n_distinct_mismatches = uint32_t(nd);
                r.do_not_add_mismatches = do_not_add ? 1u : 0u;
                r.allele_off = r.insert_off = 0;
                r.n_insert_bytes = uint32_t(nb);
                r.pad = 0;
                r.score[0] = pl.n_alt > 0 ? score0 : 0;
                r.score[1] = pl.n_alt > 1 ? score1 : 0;
                r.hap_slot[0] = pl.n_alt > 0 ? pl.k0 : 0;
                r.hap_slot[1] = pl.n_alt > 1 ? pl.k1 : 0;
                *rec = r;
            }
        }
    }
}

// A3: region order offsets of the records and the insert bytes, totals
__global__ __launch_bounds__(RA_SCAN_T) void alleles_offsets_kernel(const RaArgs a, int64_t* totals)
{
    __shared__ int64_t s[2][RA_SCAN_T];
    const int tid = threadIdx.x;
    const int32_t n_regions = ra_n_regions(a);
    int64_t carry[2] = { 0, 0 };
    for (int64_t c0 = 0; c0 < n_regions; c0 += RA_SCAN_T) {
        const int64_t slot = c0 + tid;
        int64_t v[2] = { 0, 0 };
        if (slot < n_regions) {
            v[0] = a.recs[slot].n_alleles;
            v[1] = a.recs[slot].n_insert_bytes;
        }
        for (int q = 0; q < 2; ++q) s[q][tid] = v[q];
        __syncthreads();
        for (int d = 1; d < RA_SCAN_T; d <<= 1) {
            int64_t t[2];
            for (int q = 0; q < 2; ++q) t[q] = tid >= d ? s[q][tid - d] : 0;
            __syncthreads();
            for (int q = 0; q < 2; ++q) s[q][tid] += t[q];
            __syncthreads();
        }
        if (slot < n_regions) {
            a.recs[slot].allele_off = carry[0] + s[0][tid] - v[0];
            a.recs[slot].insert_off = carry[1] + s[1][tid] - v[1];
        }
        for (int q = 0; q < 2; ++q) carry[q] += s[q][RA_SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) {
        totals[0] = carry[0];
        totals[1] = carry[1];
    }
}

// A4
__global__ __launch_bounds__(256) void alleles_copy_kernel(const RaArgs a, sk_region_allele* alleles, uint8_t* insert_pool)
{
    const int32_t n_regions = ra_n_regions(a);
    const int64_t per_region = ra_region_alleles(a), per_ins = ra_region_ins(a);
    for (int64_t slot = blockIdx.x; slot < n_regions; slot += gridDim.x) {
        const sk_region_alleles_rec* rec = a.recs + slot;
        const uint32_t n_alleles = rec->n_alleles, n_insert_bytes = rec->n_insert_bytes;
        const int64_t allele_off = rec->allele_off, insert_off = rec->insert_off;
        if (int64_t(n_alleles) > per_region || int64_t(n_insert_bytes) > per_ins) continue; // (cannot be)
        if (allele_off + int64_t(n_alleles) > a.allele_cap || insert_off + int64_t(n_insert_bytes) > a.insert_cap) continue; // (cannot be: cap_ok)
        const sk_region_allele* from = a.tmp_alleles + slot * per_region;
        for (uint32_t i = threadIdx.x; i < n_alleles; i += blockDim.x) {
            const u64* w8 = reinterpret_cast<const u64*>(from + i);
            u64* d8 = reinterpret_cast<u64*>(alleles + allele_off + i); // (a record is seven 8-byte words)
#pragma unroll
            for (int k = 0; k < int(sizeof(sk_region_allele) / 8); ++k) d8[k] = w8[k];
            alleles[allele_off + i].ins_off = from[i].ins_off + insert_off;
        }
        const uint8_t* bytes = a.tmp_ins + slot * per_ins;
        for (uint32_t i = threadIdx.x; i < n_insert_bytes; i += blockDim.x) insert_pool[insert_off + i] = bytes[i];
    }
}

struct ScratchLayout
{
    size_t n_prob, prob0, prob_src, q_off, r_off, query, ref_copy, score, begin, nseg, path, tmp_path, ptr, tmp_alleles, tmp_ins, total;
};
ScratchLayout alleles_scratch_layout(const int64_t region_cap, const int32_t max_hap_len)
{
    ScratchLayout s;
    const size_t rc = size_t(region_cap), np = size_t(SK_ALLELE_MAX_ALT) * rc, mh = size_t(max_hap_len);
    const size_t n_path = np * (mh + RA_MAX_SPAN + 4); // the aligner's: query + reference + 4 segments per problem
    size_t at = 0;
    auto take = [&](const size_t bytes) {
        const size_t off = at;
        at += sk_align256(bytes + 16);
        return off;
    };
    s.n_prob = take(4);
    s.prob0 = take(4 * rc);
    s.prob_src = take(4 * np);
    s.q_off = take(8 * (np + 1));
    s.r_off = take(8 * (np + 1));
    s.query = take(np * mh);
    s.ref_copy = take(np * RA_MAX_SPAN);
    s.score = take(4 * np);
    s.begin = take(4 * np);
    s.nseg = take(4 * np);
    s.path = take(sizeof(sk_path_seg) * n_path);
    s.tmp_path = take(sizeof(sk_path_seg) * n_path);
    s.ptr = take(sk_ga_ptr_bytes(int64_t(np), max_hap_len, RA_MAX_SPAN));
    s.tmp_alleles = take(sizeof(sk_region_allele) * rc * 2 * (mh + RA_MAX_SPAN));
    s.tmp_ins = take(rc * 2 * mh);
    s.total = at + 256; // (the base is rounded up to 256 bytes)
    return s;
}

// sk_debug_region_alleles: the two decline rules that no input reaches with the detector's scores
int g_debug_no_edge_deletion = 0, g_debug_ids_twice = 0;

} // namespace

extern "C" {

void sk_debug_region_alleles(int no_edge_deletion, int ids_twice)
{
    g_debug_no_edge_deletion = no_edge_deletion;
    g_debug_ids_twice = ids_twice;
}

int64_t sk_region_alleles_allele_bound(int64_t n_regions, int32_t max_hap_len)
{
    if (n_regions < 0 || max_hap_len < 1 || max_hap_len > RA_MAX_LEN) return -1;
    return n_regions * 2 * (int64_t(RA_MAX_SPAN) + max_hap_len);
}

int64_t sk_region_alleles_insert_bound(int64_t n_regions, int32_t max_hap_len)
{
    if (n_regions < 0 || max_hap_len < 1 || max_hap_len > RA_MAX_LEN) return -1;
    return n_regions * 2 * int64_t(max_hap_len);
}

size_t sk_region_alleles_scratch_bytes(int64_t region_cap, int32_t max_hap_len)
{
    if (region_cap < 0 || region_cap > INT32_MAX / 4 || max_hap_len < 1 || max_hap_len > RA_MAX_LEN) return 0;
    return alleles_scratch_layout(region_cap, max_hap_len).total;
}

int sk_region_alleles_dev(const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, const sk_active_region* dev_regions, const int32_t* dev_n_regions,
                          int64_t region_cap, const sk_region_haplotypes_rec* dev_hap_recs, const uint8_t* dev_seq_pool, int64_t seq_cap,
                          uint32_t max_indel_size, int32_t max_hap_len, int32_t prev_end_in, sk_region_alleles_rec* dev_recs, sk_region_allele* dev_alleles,
                          int64_t allele_cap, uint8_t* dev_insert_pool, int64_t insert_cap, int64_t* dev_totals, int32_t* dev_prev_end_out,
                          void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (ref_len < 0 || region_cap < 0 || seq_cap < 0 || allele_cap < 0 || insert_cap < 0) return sk_fail("sk_region_alleles_dev: negative size");
    if (region_cap > INT32_MAX / 4) return sk_fail("sk_region_alleles_dev: region_cap beyond a quarter of int32");
    if (max_hap_len < 1 || max_hap_len > RA_MAX_LEN) return sk_fail("sk_region_alleles_dev: max_hap_len must be in 1..1024");
    if (!dev_n_regions || !dev_totals || !dev_prev_end_out || (ref_len > 0 && !dev_ref_seq)) return sk_fail("sk_region_alleles_dev: null argument");
    if (region_cap > 0 && (!dev_regions || !dev_hap_recs || !dev_recs)) return sk_fail("sk_region_alleles_dev: null argument");
    if ((seq_cap > 0 && !dev_seq_pool) || (allele_cap > 0 && !dev_alleles) || (insert_cap > 0 && !dev_insert_pool)) return sk_fail("sk_region_alleles_dev: null argument");
    if (!dev_scratch || scratch_bytes < sk_region_alleles_scratch_bytes(region_cap, max_hap_len))
        return sk_fail("sk_region_alleles_dev: scratch is below sk_region_alleles_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const ScratchLayout lay = alleles_scratch_layout(region_cap, max_hap_len);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    RaArgs a;
    a.ref = dev_ref_seq;
    a.ref_offset = ref_offset;
    a.ref_len = ref_len;
    a.regions = dev_regions;
    a.n_regions = dev_n_regions;
    a.region_cap = region_cap;
    a.hap = dev_hap_recs;
    a.seq = dev_seq_pool;
    a.seq_cap = seq_cap;
    a.max_indel_size = max_indel_size;
    a.max_hap_len = max_hap_len;
    a.prev_end_in = prev_end_in;
    a.recs = dev_recs;
    a.allele_cap = allele_cap;
    a.insert_cap = insert_cap;
    a.n_prob = reinterpret_cast<int32_t*>(scratch + lay.n_prob);
    a.prob0 = reinterpret_cast<int32_t*>(scratch + lay.prob0);
    a.prob_src = reinterpret_cast<int32_t*>(scratch + lay.prob_src);
    a.q_off = reinterpret_cast<int64_t*>(scratch + lay.q_off);
    a.r_off = reinterpret_cast<int64_t*>(scratch + lay.r_off);
    a.query = scratch + lay.query;
    a.ref_copy = scratch + lay.ref_copy;
    a.score = reinterpret_cast<int32_t*>(scratch + lay.score);
    a.begin = reinterpret_cast<int32_t*>(scratch + lay.begin);
    a.nseg = reinterpret_cast<int32_t*>(scratch + lay.nseg);
    a.path = reinterpret_cast<sk_path_seg*>(scratch + lay.path);
    a.tmp_alleles = reinterpret_cast<sk_region_allele*>(scratch + lay.tmp_alleles);
    a.tmp_ins = reinterpret_cast<uint8_t*>(scratch + lay.tmp_ins);
    a.err = sk_ctx().dev_error_flags;
    a.ids_twice = g_debug_ids_twice;
    SK_LAUNCH(alleles_plan_kernel, dim3(1), dim3(RA_SCAN_T), 0, st, a, dev_prev_end_out);
    if (region_cap > 0) {
        const int64_t n_prob_cap = int64_t(SK_ALLELE_MAX_ALT) * region_cap;
        SK_LAUNCH(alleles_gather_kernel, dim3(unsigned(n_prob_cap < RA_GRID ? n_prob_cap : int64_t(RA_GRID))), dim3(256), 0, st, a);
        sk_global_align_batch b;
        b.n = 0; // (the count is *a.n_prob)
        b.query_off = a.q_off;
        b.query = a.query;
        b.ref_off = a.r_off;
        b.ref = a.ref_copy;
        sk_align_scores sc;
        sk_align_scores_default(&sc); // the detector's (L/starling_common/ActiveRegionDetector.hh:59-63, .cpp:41)
        if (g_debug_no_edge_deletion) sc.is_require_edge_deletion = 0; // sk_debug_region_alleles: tests only
        if (sk_ga_launch_counted(b, a.n_prob, n_prob_cap, max_hap_len, RA_MAX_SPAN, sc, a.score, a.begin, a.path, a.nseg,
                                 reinterpret_cast<sk_path_seg*>(scratch + lay.tmp_path), reinterpret_cast<uint8_t*>(scratch + lay.ptr), st))
            return 1;
        const unsigned grid = unsigned(region_cap < RA_GRID ? region_cap : int64_t(RA_GRID));
        SK_LAUNCH(alleles_region_kernel, dim3(grid), dim3(64), 0, st, a);
    }
    SK_LAUNCH(alleles_offsets_kernel, dim3(1), dim3(RA_SCAN_T), 0, st, a, dev_totals);
    if (region_cap > 0) {
        const unsigned grid = unsigned(region_cap < RA_GRID ? region_cap : int64_t(RA_GRID));
        SK_LAUNCH(alleles_copy_kernel, dim3(grid), dim3(256), 0, st, a, dev_alleles, dev_insert_pool);
    }
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_region_alleles(const char* ref_seq, int32_t ref_offset, int32_t ref_len, const sk_active_region* regions, int32_t n_regions,
                      const sk_region_haplotypes_rec* hap_recs, const uint8_t* seq_pool, int64_t seq_len, uint32_t max_indel_size, int32_t max_hap_len,
                      int32_t prev_end_in, sk_region_alleles_rec* recs, sk_region_allele* alleles, int64_t allele_cap, uint8_t* insert_pool,
                      int64_t insert_cap, int64_t* totals, int32_t* prev_end_out)
{
    if (ref_len < 0 || n_regions < 0 || seq_len < 0 || allele_cap < 0 || insert_cap < 0) return sk_fail("sk_region_alleles: negative size");
    if (max_hap_len < 1 || max_hap_len > RA_MAX_LEN) return sk_fail("sk_region_alleles: max_hap_len must be in 1..1024");
    if (!totals || !prev_end_out || (ref_len > 0 && !ref_seq) || (n_regions > 0 && (!regions || !hap_recs || !recs)) || (seq_len > 0 && !seq_pool))
        return sk_fail("sk_region_alleles: null argument");
    for (int32_t i = 0; i < n_regions; ++i) {
        const sk_region_haplotypes_rec& h = hap_recs[i];
        if (h.status != SK_HAP_COUNTED || h.n_selected == 0u) continue;
        const std::string where = "sk_region_alleles: region " + std::to_string(i) + ": ";
        const int64_t span = int64_t(regions[i].end) - regions[i].begin;
        if (span < 1 || span > RA_MAX_SPAN) return sk_fail(where + "counted with no or more than SK_HAP_MAX_REF_SPAN positions");
        if (h.n_selected > uint32_t(SK_HAP_MAX_SELECTED)) return sk_fail(where + "more than SK_HAP_MAX_SELECTED haplotypes selected");
        int n_alt = 0;
        for (uint32_t k = 0; k < h.n_selected; ++k) {
            if (h.hap[k].seq_off < 0 || h.hap[k].seq_len == 0u || h.hap[k].seq_off + int64_t(h.hap[k].seq_len) > seq_len)
                return sk_fail(where + "a selected haplotype is empty or lies outside seq_pool");
            n_alt += h.hap[k].is_reference ? 0 : 1;
        }
        if (n_alt > SK_ALLELE_MAX_ALT) return sk_fail(where + "more than two alternate haplotypes");
    }
    const int64_t allele_bound = sk_region_alleles_allele_bound(n_regions, max_hap_len), insert_bound = sk_region_alleles_insert_bound(n_regions, max_hap_len);
    if (allele_cap < allele_bound) return sk_fail("sk_region_alleles: allele_cap is below sk_region_alleles_allele_bound");
    if (insert_cap < insert_bound) return sk_fail("sk_region_alleles: insert_cap is below sk_region_alleles_insert_bound");
    if ((allele_bound > 0 && !alleles) || (insert_bound > 0 && !insert_pool)) return sk_fail("sk_region_alleles: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t ng = size_t(n_regions);
    const size_t scratch_bytes = sk_region_alleles_scratch_bytes(n_regions, max_hap_len);
    struct
    {
        char* ref; sk_active_region* regions; sk_region_haplotypes_rec* hap; uint8_t* seq; int32_t* n_regions; sk_region_alleles_rec* recs;
        sk_region_allele* alleles; uint8_t* ins; char* scratch; int64_t* totals; int32_t* prev_end;
    } d;
    int rc = 0;
    // (+ 16 bytes and the like: kernels read whole words past an array's end; a piece starts at a multiple of 256 bytes, as the scratch's
    // layout wants its base; sk_region_alleles_dev, sk_ga_launch_counted under it and sk_check_device_errors reserve nothing of the arena)
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(ref_seq, size_t(ref_len), 16, st, rc), ar.up(regions, ng, 2, st, rc), ar.up(hap_recs, ng, 1, st, rc),
                                ar.up(seq_pool, size_t(seq_len), 16, st, rc), ar.up(&n_regions, 1, 0, st, rc), ar.take<sk_region_alleles_rec>(ng + 1),
                                ar.take<sk_region_allele>(size_t(allele_bound) + 1), ar.take<uint8_t>(size_t(insert_bound) + 16), ar.take<char>(scratch_bytes + 16),
                                ar.take<int64_t>(2), ar.take<int32_t>(1) };
        }) || rc)
        return 1;
    if (sk_region_alleles_dev(d.ref, ref_offset, ref_len, d.regions, d.n_regions, n_regions, d.hap, d.seq, seq_len, max_indel_size, max_hap_len, prev_end_in, d.recs,
                              d.alleles, allele_bound, d.ins, insert_bound, d.totals, d.prev_end, d.scratch, scratch_bytes + 16, st))
        return 1;
    int64_t t[2] = { 0, 0 };
    int32_t prev = 0;
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::memcpyAsync(&prev, d.prev_end, sizeof(prev), hipMemcpyDeviceToHost, st));
    if (n_regions > 0) SK_HIP(skrt::memcpyAsync(recs, d.recs, sizeof(sk_region_alleles_rec) * ng, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    if (t[0] < 0 || t[0] > allele_bound || t[1] < 0 || t[1] > insert_bound) return sk_fail("sk_region_alleles: totals out of range");
    if (t[0] > 0) SK_HIP(skrt::memcpyAsync(alleles, d.alleles, sizeof(sk_region_allele) * size_t(t[0]), hipMemcpyDeviceToHost, st));
    if (t[1] > 0) SK_HIP(skrt::memcpyAsync(insert_pool, d.ins, size_t(t[1]), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    totals[0] = t[0];
    totals[1] = t[1];
    *prev_end_out = prev;
    return 0;
}

} // extern "C"
