// indel_table.hip -- a window's indel observations merged by key: what the reference's IndelBuffer (std::map<IndelKey, IndelData>,
// L/starling_common/IndelBuffer.cpp) holds after every read observation of the call has been added and the call's regions have then
// been closed in order.  The rules are numbered in the header's block and restated one function each in tests/indel_table_model.py.
//
//   T0  itab_plan_kernel     one workgroup: what the host entry refuses (iat, offsets, records outside their pools); per (region, sample)
//       pair in step order the number of expanded records (a record with to_indel_buffer gives one CONTRIBUTION record and one per
//       supporting read), their offsets by a scan (block_scan.h); the pending pairs; the capacity test
//   T1  itab_expand_kernel   one record per observation and per (allele record, supporting read): key words, where the insert bytes lie,
//       sample, class, id
//   T2  itab_sort_tile_kernel  a bitonic sort of 1 024 record indices per workgroup in LDS, then itab_merge_kernel passes that double the
//       run width: every index finds its place by a binary search in the sibling run.  The order is (key, sample, class, id, record
//       index): total, so the result does not depend on scheduling.  The comparator reads insert bytes only when (pos, type, ins_len,
//       del_len) tie.  The number of passes is fixed by expand_cap.
//   T3  itab_heads_kernel    one workgroup: key heads, (key, sample, class) heads and duplicate ids by neighbour compare; the offsets of
//       keys, ids and insert bytes by three scans; the capacity test; totals
//   T4  itab_key_kernel      one wave per key: the key record and its insert bytes, the id lists, rules 4 and 5 (lane 0 walks the
//       reference: data dependent and short), rule 6 by lane s in record order (float additions are ordered), rules 7 and 8 by the lanes
//       striding over the regions -- a key exists at a step if it has a read observation or a contribution of an earlier step, the last
//       writer of active_region_id is the highest step: both are max / min reductions, no order-dependent atomics
//
// Input the host entry refuses, or a capacity below what the arrays hold, raises SK_DEVERR_INDEL_TABLE and leaves totals of zero.
#include "sk_common.h"

#include "block_scan.h"

#include <algorithm>
#include <climits>

namespace
{

typedef unsigned long long u64;

enum {
    IT_TILE = 1024,   // records a workgroup sorts in LDS
    IT_SCAN_T = 1024,
    IT_GRID = 1024,
    IT_CLASS_CONTRIB = SK_ITAB_N_SETS // an allele record's own entry: rule 6 walks them in (region, record) order
};
constexpr uint32_t IT_NONE = 0xffffffffu;

struct ItPlus
{
    __host__ __device__ int64_t operator()(const int64_t a, const int64_t b) const { return a + b; }
};

struct ItRec // one expanded record
{
    int32_t pos;
    uint32_t type, ins_len, del_len; // (a breakpoint's lengths are 0: rule 1 compares no further)
    int64_t ins_off;                 // its insert bytes: read codes at read_code[ins_off ..), or ASCII at insert_pool[ins_off ..)
    uint32_t sample, cls;            // SK_ITAB_* or IT_CLASS_CONTRIB
    uint32_t id;                     // the align id; CONTRIB: the record's index in the sample's alleles
    uint32_t aux;                    // bit 0: a read observation; bit 1: its bytes are ASCII; CONTRIB: region index << 2
};

enum { CTL_N = 0, CTL_OK, CTL_BAD, CTL_PENDING, CTL_KEYS, CTL_OK2, CTL_WORDS = 8 };

struct ItArgs
{
    int32_t n_samples;
    sk_indel_table_sample s[SK_MAX_SAMPLES];
    const char* ref;
    int32_t ref_offset, ref_len;
    const sk_active_region* regions;
    const int32_t* n_regions;
    int64_t region_cap;
    int32_t prev_end_in;
    int64_t expand_cap, key_cap, id_cap, insert_cap;
    sk_indel_table_key* keys;
    sk_indel_table_sample_data* data;
    uint32_t* id_pool;
    uint8_t* insert_pool;
    int64_t* totals;
    // scratch
    int64_t* ctl;       // [CTL_WORDS]
    int64_t* obs_base;  // [SK_MAX_SAMPLES + 1]
    int64_t* pair_off;  // [region_cap * n_samples + 1] (step order)
    ItRec* rec;         // [expand_cap]
    uint32_t* idx[2];   // [expand_cap] the sorted order, ping and pong
    int64_t* id_at;     // [expand_cap + 1] per sorted position: the ids kept before it
    int64_t* key_start; // [expand_cap + 1] per key: its first sorted position
    int64_t* key_ins;   // [expand_cap + 1] per key: its insert bytes' offset
    unsigned* err;
};

__device__ __forceinline__ int32_t it_n_regions(const ItArgs& a)
{
    int32_t n = *a.n_regions;
    if (n < 0) n = 0;
    if (int64_t(n) > a.region_cap) n = int32_t(a.region_cap);
    return n;
}
__device__ __forceinline__ uint8_t it_code_char(const uint8_t c) // bam_seq::get_char
{
    return c == 0 ? '=' : c == 1 ? 'A' : c == 2 ? 'C' : c == 4 ? 'G' : c == 8 ? 'T' : 'N';
}
__device__ __forceinline__ uint8_t it_ins_char(const ItArgs& a, const ItRec& r, const uint32_t k)
{
    const sk_indel_table_sample& s = a.s[r.sample];
    return (r.aux & 2u) ? s.insert_pool[r.ins_off + k] : it_code_char(s.read_code[r.ins_off + k]);
}
// rule 1: -1, 0, 1 as IndelKey::operator< orders the keys (IndelKey.hh:56-76); the bytes in ASCII order
__device__ __forceinline__ int it_key_cmp(const ItArgs& a, const ItRec& x, const ItRec& y)
{
    if (x.pos != y.pos) return x.pos < y.pos ? -1 : 1;
    if (x.type != y.type) return x.type < y.type ? -1 : 1;
    if (x.ins_len != y.ins_len) return x.ins_len < y.ins_len ? -1 : 1;
    if (x.del_len != y.del_len) return x.del_len < y.del_len ? -1 : 1;
    for (uint32_t k = 0; k < x.ins_len; ++k) {
        const uint8_t cx = it_ins_char(a, x, k), cy = it_ins_char(a, y, k);
        if (cx != cy) return cx < cy ? -1 : 1;
    }
    return 0;
}
__device__ __forceinline__ bool it_less(const ItArgs& a, const uint32_t i, const uint32_t j)
{
    if (i == IT_NONE || j == IT_NONE) return j == IT_NONE && i != IT_NONE; // (the tile's padding sorts last)
    const ItRec x = a.rec[i], y = a.rec[j];
    const int c = it_key_cmp(a, x, y);
    if (c) return c < 0;
    if (x.sample != y.sample) return x.sample < y.sample;
    if (x.cls != y.cls) return x.cls < y.cls;
    if (x.cls == uint32_t(IT_CLASS_CONTRIB) && (x.aux >> 2) != (y.aux >> 2)) return (x.aux >> 2) < (y.aux >> 2); // (region, record) order whatever the offsets
    if (x.id != y.id) return x.id < y.id;
    return i < j;
}

enum { PAIR_NONE = 0, PAIR_RECORDS, PAIR_BYPASSED, PAIR_PENDING };
__device__ __forceinline__ int it_pair_kind(const ItArgs& a, const int s, const int64_t region)
{
    const int hs = a.s[s].hap_recs[region].status;
    if (hs == SK_HAP_NO_READS || hs == SK_HAP_TOO_FEW_COVERING || hs == SK_HAP_DECLINED || a.s[s].recs[region].status == SK_HAP_DECLINED) return PAIR_PENDING; // rule 8
    return hs == SK_HAP_BYPASSED ? PAIR_BYPASSED : PAIR_RECORDS;
}
// the expanded records allele record k of (sample, region) gives, -1 for one the host entry refuses
__device__ __forceinline__ int64_t it_record_count(const ItArgs& a, const int s, const int64_t region, const int64_t k)
{
    const sk_indel_table_sample& sm = a.s[s];
    const sk_region_allele al = sm.alleles[k];
    if (al.type != SK_INDEL_INDEL && al.type != SK_INDEL_MISMATCH) return -1;
    if (al.ins_off < 0 || al.ins_off + int64_t(al.ins_len) > sm.insert_cap) return -1;
    if (!al.to_indel_buffer) return 0;
    const sk_region_haplotypes_rec* h = sm.hap_recs + region;
    if (al.hap_slot < 0 || al.hap_slot >= SK_HAP_MAX_SELECTED || uint32_t(al.hap_slot) >= h->n_selected) return -1;
    const sk_selected_haplotype hp = h->hap[al.hap_slot];
    if (hp.support_off < 0 || hp.support_off + int64_t(hp.count) > sm.support_cap) return -1;
    return 1 + int64_t(hp.count);
}

// T0
__global__ __launch_bounds__(IT_SCAN_T) void itab_plan_kernel(const ItArgs a)
{
    __shared__ int64_t s_wave[16];
    __shared__ int s_bad;
    __shared__ int64_t s_obs[SK_MAX_SAMPLES + 1];
    const int tid = threadIdx.x;
    const int S = a.n_samples;
    const int32_t n_regions = it_n_regions(a);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    if (tid < S) {
        const sk_indel_table_sample& sm = a.s[tid];
        const int64_t n_obs = sm.n_reads > 0 ? sm.obs_off[sm.n_reads] : 0;
        if (n_obs < 0 || n_obs > sm.obs_cap) bad = 1;
        if (sm.n_reads > 0 && (sm.obs_off[0] != 0 || sm.read_off[0] != 0)) bad = 1; // (every slot of rec below n_obs is then some read's)
        s_obs[tid] = bad ? 0 : n_obs;
    }
    for (int s = 0; s < S; ++s) { // rule 9: an iat above 2
        const sk_indel_table_sample& sm = a.s[s];
        for (int32_t r = tid; r < sm.n_reads; r += IT_SCAN_T) bad |= sm.iat[r] > SK_IAT_SUBMAP ? 1 : 0;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (tid == 0) {
        int64_t at = 0;
        for (int s = 0; s < S; ++s) {
            a.obs_base[s] = at;
            at += s_obs[s];
        }
        a.obs_base[S] = at;
        s_obs[SK_MAX_SAMPLES] = at;
    }
    __syncthreads();
    const int64_t n_obs_total = s_obs[SK_MAX_SAMPLES];
    const int64_t n_pairs = int64_t(n_regions) * S;
    int64_t carry = n_obs_total, pending = 0;
    for (int64_t c0 = 0; c0 < n_pairs; c0 += IT_SCAN_T) {
        const int64_t p = c0 + tid;
        int64_t v = 0;
        if (p < n_pairs) {
            const int64_t region = p / S;
            const int s = int(p % S);
            const int kind = it_pair_kind(a, s, region);
            pending += kind == PAIR_PENDING ? 1 : 0;
            if (kind == PAIR_RECORDS) {
                const sk_region_alleles_rec rc = a.s[s].recs[region];
                if (rc.allele_off < 0 || rc.allele_off + int64_t(rc.n_alleles) > a.s[s].allele_cap) {
                    bad = 1;
                } else {
                    for (uint32_t k = 0; k < rc.n_alleles; ++k) {
                        const int64_t c = it_record_count(a, s, region, rc.allele_off + k);
                        if (c < 0) bad = 1;
                        else v += c;
                    }
                }
            }
        }
        const int64_t incl = block_scan_1024(v, ItPlus(), s_wave) + carry;
        if (p < n_pairs) a.pair_off[p] = incl - v;
        __syncthreads();
        if (tid == IT_SCAN_T - 1) s_wave[0] = incl;
        __syncthreads();
        carry = s_wave[0];
        __syncthreads();
    }
    pending = block_scan_1024(pending, ItPlus(), s_wave);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (tid == IT_SCAN_T - 1) {
        const bool ok = !s_bad && carry <= a.expand_cap;
        a.pair_off[n_pairs] = carry;
        a.ctl[CTL_N] = ok ? carry : 0;
        a.ctl[CTL_OK] = ok ? 1 : 0;
        a.ctl[CTL_BAD] = 0;
        a.ctl[CTL_PENDING] = pending;
        a.ctl[CTL_KEYS] = 0;
        a.ctl[CTL_OK2] = 0;
        if (!ok) atomicOr(a.err, unsigned(SK_DEVERR_INDEL_TABLE));
    }
}

__device__ __forceinline__ void it_expand_bad(const ItArgs& a)
{
    a.ctl[CTL_BAD] = 1; // (every writer writes 1)
    atomicOr(a.err, unsigned(SK_DEVERR_INDEL_TABLE));
}

// T1: blocks 0 .. gridDim.x / 2 - 1 take the reads, the others the (region, sample) pairs
__global__ __launch_bounds__(IT_SCAN_T) void itab_expand_kernel(const ItArgs a)
{
    __shared__ int64_t s_wave[16];
    if (!a.ctl[CTL_OK]) return;
    const int tid = threadIdx.x;
    const int S = a.n_samples;
    const int half = int(gridDim.x) / 2;
    if (int(blockIdx.x) < half) { // rule 2
        for (int s = 0; s < S; ++s) {
            const sk_indel_table_sample& sm = a.s[s];
            const int64_t base = a.obs_base[s], n_obs = a.obs_base[s + 1] - base;
            for (int64_t r = int64_t(blockIdx.x) * IT_SCAN_T + tid; r < sm.n_reads; r += int64_t(half) * IT_SCAN_T) {
                const int64_t o0 = sm.obs_off[r], o1 = sm.obs_off[r + 1];
                const int64_t b0 = sm.read_off[r], b1 = sm.read_off[r + 1];
                if (o0 < 0 || o1 < o0 || o1 > n_obs || b0 < 0 || b1 < b0) {
                    it_expand_bad(a); // (its slots keep whatever they held: nothing reads them once CTL_BAD is up)
                    continue;
                }
                const uint32_t id = sm.align_id ? sm.align_id[r] : uint32_t(r);
                const uint32_t iat = sm.iat[r];
                for (int64_t j = o0; j < o1; ++j) {
                    const sk_intake_obs o = sm.obs[j];
                    ItRec x;
                    x.pos = o.pos;
                    x.type = o.type;
                    const bool bp = o.type == SK_INDEL_BP_LEFT || o.type == SK_INDEL_BP_RIGHT;
                    bool good = (bp || o.type == SK_INDEL_INDEL) && int64_t(o.ins_begin) + o.ins_len <= b1 - b0;
                    x.ins_len = (bp || !good) ? 0u : o.ins_len;
                    x.del_len = bp ? 0u : o.deletion_length;
                    x.ins_off = b0 + o.ins_begin;
                    x.sample = uint32_t(s);
                    x.cls = o.is_noise ? uint32_t(SK_ITAB_NOISE) : iat;
                    x.id = id;
                    x.aux = 1u;
                    a.rec[base + j] = x;
                    if (!good) it_expand_bad(a);
                }
            }
        }
        return;
    }
    // rule 3, and one CONTRIBUTION record per allele record for rule 6
    const int32_t n_regions = it_n_regions(a);
    const int64_t n_pairs = int64_t(n_regions) * S;
    for (int64_t p = int64_t(blockIdx.x) - half; p < n_pairs; p += int64_t(gridDim.x) - half) {
        const int64_t region = p / S;
        const int s = int(p % S);
        if (a.pair_off[p + 1] == a.pair_off[p]) continue; // (uniform over the workgroup)
        const sk_indel_table_sample& sm = a.s[s];
        const sk_region_alleles_rec rc = sm.recs[region];
        int64_t carry = a.pair_off[p];
        for (uint32_t c0 = 0; c0 < rc.n_alleles; c0 += IT_SCAN_T) {
            const uint32_t k = c0 + tid;
            const int64_t v = k < rc.n_alleles ? it_record_count(a, s, region, rc.allele_off + k) : 0;
            const int64_t incl = block_scan_1024(v, ItPlus(), s_wave) + carry;
            if (v > 0) {
                const int64_t ak = rc.allele_off + k;
                const sk_region_allele al = sm.alleles[ak];
                ItRec x;
                x.pos = al.pos;
                x.type = uint32_t(al.type);
                x.ins_len = al.ins_len;
                x.del_len = al.del_len;
                x.ins_off = al.ins_off;
                x.sample = uint32_t(s);
                x.cls = uint32_t(IT_CLASS_CONTRIB);
                x.id = uint32_t(ak);
                x.aux = 2u | (uint32_t(region) << 2);
                int64_t at = incl - v;
                a.rec[at++] = x;
                const sk_selected_haplotype hp = sm.hap_recs[region].hap[al.hap_slot];
                x.aux = 2u;
                for (uint32_t q = 0; q < hp.count; ++q) {
                    const int32_t r = sm.support_pool[hp.support_off + q];
                    const bool good = r >= 0 && r < sm.n_reads;
                    x.cls = good ? uint32_t(sm.iat[r]) : 0u; // never noise (:736-739)
                    x.id = good ? (sm.align_id ? sm.align_id[r] : uint32_t(r)) : 0u;
                    a.rec[at++] = x;
                    if (!good) it_expand_bad(a);
                }
            }
            __syncthreads();
            if (tid == IT_SCAN_T - 1) s_wave[0] = incl;
            __syncthreads();
            carry = s_wave[0];
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int64_t it_live_n(const ItArgs& a) { return (a.ctl[CTL_OK] && !a.ctl[CTL_BAD]) ? a.ctl[CTL_N] : 0; }

// T2, the tiles
__global__ __launch_bounds__(IT_TILE) void itab_sort_tile_kernel(const ItArgs a)
{
    __shared__ uint32_t s_idx[IT_TILE];
    const int64_t n = it_live_n(a);
    const int64_t t0 = int64_t(blockIdx.x) * IT_TILE;
    if (t0 >= n) return;
    const int tid = threadIdx.x;
    s_idx[tid] = t0 + tid < n ? uint32_t(t0 + tid) : IT_NONE;
    __syncthreads();
    for (int k = 2; k <= IT_TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (other > tid) {
                const uint32_t x = s_idx[tid], y = s_idx[other];
                const bool up = (tid & k) == 0;
                if (it_less(a, y, x) == up) {
                    s_idx[tid] = y;
                    s_idx[other] = x;
                }
            }
            __syncthreads();
        }
    }
    if (t0 + tid < n) a.idx[0][t0 + tid] = s_idx[tid];
}

// T2, one merge pass: runs of `width` sorted positions in src become runs of 2 * width in dst
__global__ __launch_bounds__(256) void itab_merge_kernel(const ItArgs a, const int from, const int64_t width)
{
    const int64_t n = it_live_n(a);
    const uint32_t* src = a.idx[from];
    uint32_t* dst = a.idx[from ^ 1];
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        const int64_t l0 = i / (2 * width) * (2 * width);
        const int64_t r0 = l0 + width < n ? l0 + width : n, r1 = l0 + 2 * width < n ? l0 + 2 * width : n;
        const bool left = i < r0;
        const uint32_t x = src[i];
        int64_t lo = left ? r0 : l0, hi = left ? r1 : r0; // the elements of the sibling run below x (the order is total: none equals x)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (it_less(a, src[mid], x)) lo = mid + 1;
            else hi = mid;
        }
        const int64_t below = lo - (left ? r0 : l0);
        dst[l0 + (i - (left ? l0 : r0)) + below] = x;
    }
}

// T3
__global__ __launch_bounds__(IT_SCAN_T) void itab_heads_kernel(const ItArgs a, const int from)
{
    __shared__ int64_t s_wave[16];
    const int64_t n = it_live_n(a);
    const uint32_t* idx = a.idx[from];
    const int tid = threadIdx.x;
    int64_t carry[3] = { 0, 0, 0 }; // keys, ids, insert bytes
    for (int64_t c0 = 0; c0 < n; c0 += IT_SCAN_T) {
        const int64_t j = c0 + tid;
        int64_t v[3] = { 0, 0, 0 };
        if (j < n) {
            const ItRec x = a.rec[idx[j]];
            bool key_head = true, id_head = x.cls != uint32_t(IT_CLASS_CONTRIB);
            if (j > 0) {
                const ItRec y = a.rec[idx[j - 1]];
                key_head = it_key_cmp(a, y, x) != 0;
                if (!key_head && y.sample == x.sample && y.cls == x.cls && y.id == x.id) id_head = false; // the same id twice is one member
            }
            v[0] = key_head ? 1 : 0;
            v[1] = id_head ? 1 : 0;
            v[2] = key_head ? x.ins_len : 0;
        }
        int64_t incl[3];
        for (int q = 0; q < 3; ++q) {
            incl[q] = block_scan_1024(v[q], ItPlus(), s_wave) + carry[q];
            __syncthreads();
            if (tid == IT_SCAN_T - 1) s_wave[0] = incl[q];
            __syncthreads();
            carry[q] = s_wave[0];
            __syncthreads();
        }
        if (j < n) {
            a.id_at[j] = incl[1] - v[1];
            if (v[0]) {
                a.key_start[incl[0] - 1] = j;
                a.key_ins[incl[0] - 1] = incl[2] - v[2];
            }
        }
    }
    if (tid == 0) {
        const bool live = a.ctl[CTL_OK] && !a.ctl[CTL_BAD];
        const bool ok = live && carry[0] <= a.key_cap && carry[1] <= a.id_cap && carry[2] <= a.insert_cap;
        if (live && !ok) atomicOr(a.err, unsigned(SK_DEVERR_INDEL_TABLE));
        a.id_at[n] = carry[1];
        a.key_start[carry[0]] = n;
        a.key_ins[carry[0]] = carry[2];
        a.ctl[CTL_KEYS] = ok ? carry[0] : 0;
        a.ctl[CTL_OK2] = ok ? 1 : 0;
        a.totals[0] = ok ? carry[0] : 0;
        a.totals[1] = ok ? carry[1] : 0;
        a.totals[2] = ok ? carry[2] : 0;
        a.totals[3] = ok ? a.ctl[CTL_PENDING] : 0;
    }
}

// ---- rule 5: getAlleleReportInfo and set_repeat_info (L/starling_common/AlleleReportInfoUtil.cpp:96-216)
struct ItKeySeq // a key's bytes and the reference
{
    const ItArgs* a;
    ItRec head;
    __device__ __forceinline__ uint8_t base(const int64_t p) const // reference_contig_segment::get_base: 'N' outside the segment
    {
        const int64_t k = p - a->ref_offset;
        return (k < 0 || k >= a->ref_len) ? uint8_t('N') : uint8_t(a->ref[k]);
    }
    __device__ __forceinline__ uint8_t ins(const uint32_t k) const { return it_ins_char(*a, head, k); }
    __device__ __forceinline__ uint8_t del(const uint32_t k) const { return base(int64_t(head.pos) + k); }
};
// get_seq_repeat_unit (L/blt_util/seq_util.cpp:125-164): the smallest perfect repeat -> the unit's length (the unit is the first bytes)
template <bool INS> __device__ __forceinline__ uint32_t it_repeat_unit(const ItKeySeq& q, const uint32_t n)
{
    for (uint32_t i = 1; i < n; ++i) {
        if (n % i) continue;
        bool rep = true;
        for (uint32_t j = i; j < n && rep; ++j) rep = (INS ? q.ins(j) : q.del(j)) == (INS ? q.ins(j % i) : q.del(j % i));
        if (rep) return i;
    }
    return n;
}
// getInterruptedHomopolymerLength (L/blt_common/ref_context.cpp:237-272) with ihpol_data (:183-232)
struct ItIhpol
{
    uint8_t r1 = 'N', r2 = 'N';
    uint32_t nr1 = 0, nr2 = 0;
    __device__ __forceinline__ bool add(const uint8_t b)
    {
        if (nr1 == 0) {
            r1 = b;
            nr1 = 1;
        } else if (r1 == b) {
            if (nr2 > 1 || r1 == 'N') return false;
            ++nr1;
        } else if (nr2 == 0) {
            r2 = b;
            nr2 = 1;
        } else if (r2 == b) {
            if (nr1 > 1 || r2 == 'N') return false;
            ++nr2;
        } else {
            return false;
        }
        return true;
    }
    __device__ __forceinline__ uint32_t size() const { return nr1 > nr2 ? nr1 : nr2; }
};
__device__ __forceinline__ uint32_t it_ihpol(const ItKeySeq& q, const int64_t pos)
{
    const int64_t rs = int64_t(q.a->ref_offset) + q.a->ref_len;
    ItIhpol up, dn;
    for (int64_t i = pos; i >= 0; --i)
        if (!up.add(q.base(i))) break;
    for (int64_t i = pos + 1; i < rs; ++i)
        if (!up.add(q.base(i))) break;
    for (int64_t i = pos; i < rs; ++i)
        if (!dn.add(q.base(i))) break;
    for (int64_t i = pos - 1; i >= 0; --i)
        if (!dn.add(q.base(i))) break;
    return up.size() > dn.size() ? up.size() : dn.size();
}
__device__ __forceinline__ void it_report_info(const ItKeySeq& q, sk_indel_table_key* out)
{
    const ItRec& h = q.head;
    const bool bp = h.type == SK_INDEL_BP_LEFT || h.type == SK_INDEL_BP_RIGHT;
    int it = SK_ITAB_OTHER; // SimplifiedIndelReportType::getRateType (AlleleReportInfo.hh:47-72)
    if (h.type == SK_INDEL_INDEL) it = (h.ins_len == 0 && h.del_len > 0) ? SK_ITAB_DELETE : (h.ins_len > 0 && h.del_len == 0) ? SK_ITAB_INSERT : SK_ITAB_SWAP;
    else if (bp) it = SK_ITAB_BREAKPOINT;
    const int64_t pos = h.pos, right = pos + int64_t(h.del_len);
    uint32_t unit = 0, ins_count = 0, del_count = 0;
    bool unit_of_insert = true;
    if (it == SK_ITAB_INSERT) {
        unit = it_repeat_unit<true>(q, h.ins_len);
        ins_count = h.ins_len / unit;
    } else if (it == SK_ITAB_DELETE) {
        unit = it_repeat_unit<false>(q, h.del_len);
        del_count = h.del_len / unit;
        unit_of_insert = false;
    } else if (it == SK_ITAB_SWAP) {
        const uint32_t iu = h.ins_len ? it_repeat_unit<true>(q, h.ins_len) : 0u, du = h.del_len ? it_repeat_unit<false>(q, h.del_len) : 0u;
        bool same = iu == du && iu > 0; // (:134)
        for (uint32_t k = 0; same && k < iu; ++k) same = q.ins(k) == q.del(k);
        if (same) {
            unit = iu;
            ins_count = h.ins_len / iu;
            del_count = h.del_len / du;
        }
    }
    uint32_t context = 0;
    if (unit > 0) {
        const int64_t n = unit;
        for (int64_t i = pos - n; i >= 0; i -= n) { // upstream (:152-165)
            if (i + n <= int64_t(q.a->ref_offset)) {
                // wholly before the segment, where get_base gives 'N' down to position 0: a unit that is not all N ends the walk here,
                // one that is matches every step the reference's loop would still take
                bool all_n = true;
                for (int64_t j = 0; j < n && all_n; ++j) all_n = (unit_of_insert ? q.ins(uint32_t(j)) : q.del(uint32_t(j))) == 'N';
                if (all_n) context += uint32_t(i / n + 1);
                break;
            }
            bool rep = true;
            for (int64_t j = 0; j < n && rep; ++j) rep = q.base(i + j) == (unit_of_insert ? q.ins(uint32_t(j)) : q.del(uint32_t(j)));
            if (!rep) break;
            ++context;
        }
        const int64_t rs = int64_t(q.a->ref_offset) + q.a->ref_len;
        for (int64_t i = right; i + n - 1 < rs; i += n) { // downstream, stopping at ref.end() (:168-182)
            bool rep = true;
            for (int64_t j = 0; j < n && rep; ++j) rep = q.base(i + j) == (unit_of_insert ? q.ins(uint32_t(j)) : q.del(uint32_t(j)));
            if (!rep) break;
            ++context;
        }
    }
    uint32_t ih = it_ihpol(q, pos - 1); // (:205-215)
    uint32_t t = it_ihpol(q, pos);
    ih = t > ih ? t : ih;
    if (right != pos) {
        t = it_ihpol(q, right - 1);
        ih = t > ih ? t : ih;
        t = it_ihpol(q, right);
        ih = t > ih ? t : ih;
    }
    out->it = it;
    out->repeat_unit_len = unit;
    out->ref_repeat_count = unit ? context + del_count : 0u;
    out->indel_repeat_count = unit ? context + ins_count : 0u;
    out->interrupted_hpol_len = ih;
}

__device__ __forceinline__ int64_t it_wave_max(int64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t t = __shfl_xor(v, d, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ unsigned it_wave_or(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= unsigned(__shfl_xor(int(v), d, 64));
    return v;
}

// T4
__global__ __launch_bounds__(64) void itab_key_kernel(const ItArgs a, const int from)
{
    __shared__ unsigned s_count[SK_MAX_SAMPLES][SK_ITAB_N_SETS + 1];
    __shared__ unsigned s_first[SK_MAX_SAMPLES][SK_ITAB_N_SETS + 1]; // a group's first sorted position, relative to the key's
    if (!a.ctl[CTL_OK2]) return;
    const int lane = threadIdx.x;
    const int S = a.n_samples;
    const int64_t n_keys = a.ctl[CTL_KEYS];
    const int32_t n_regions = it_n_regions(a);
    const uint32_t* idx = a.idx[from];
    for (int64_t key = blockIdx.x; key < n_keys; key += gridDim.x) {
        __syncthreads();
        for (int i = lane; i < SK_MAX_SAMPLES * (SK_ITAB_N_SETS + 1); i += 64) {
            (&s_count[0][0])[i] = 0u;
            (&s_first[0][0])[i] = IT_NONE;
        }
        __syncthreads();
        const int64_t j0 = a.key_start[key], j1 = a.key_start[key + 1];
        const ItRec head = a.rec[idx[j0]];
        const bool bp = head.type == SK_INDEL_BP_LEFT || head.type == SK_INDEL_BP_RIGHT;
        // the id lists; what the key's records say about it
        unsigned n_read_obs = 0;
        int64_t last_contrib = -1, neg_first_contrib = LLONG_MIN; // steps: region * S + sample
        for (int64_t j = j0 + lane; j < j1; j += 64) {
            const ItRec x = a.rec[idx[j]];
            n_read_obs += x.aux & 1u;
            if (x.cls == uint32_t(IT_CLASS_CONTRIB)) {
                const int64_t step = int64_t(x.aux >> 2) * S + x.sample;
                last_contrib = step > last_contrib ? step : last_contrib;
                neg_first_contrib = -step > neg_first_contrib ? -step : neg_first_contrib;
                atomicAdd(&s_count[x.sample][x.cls], 1u);
                atomicMin(&s_first[x.sample][x.cls], unsigned(j - j0));
            } else if (a.id_at[j + 1] != a.id_at[j]) {
                a.id_pool[a.id_at[j]] = x.id;
                atomicAdd(&s_count[x.sample][x.cls], 1u);
                atomicMin(&s_first[x.sample][x.cls], unsigned(j - j0));
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n_read_obs += unsigned(__shfl_xor(int(n_read_obs), d, 64));
        last_contrib = it_wave_max(last_contrib);
        const int64_t m = it_wave_max(neg_first_contrib);
        const int64_t first_contrib = m == LLONG_MIN ? LLONG_MAX : -m;
        __syncthreads();
        // the insert bytes, once per key
        const int64_t ins_at = a.key_ins[key];
        for (uint32_t k = lane; k < head.ins_len; k += 64) a.insert_pool[ins_at + k] = it_ins_char(a, head, k);
        // rules 7 and 8: the lanes stride over the regions, the samples inside
        unsigned bypassed = 0, pending = 0;
        int64_t last_writer = last_contrib;
        for (int64_t region = lane; region < n_regions; region += 64) {
            const sk_active_region g = a.regions[region];
            const int32_t prev_end = region == 0 ? a.prev_end_in : a.regions[region - 1].end;
            const int32_t lo = g.begin < (prev_end > 0 ? prev_end : 0) ? g.begin : (prev_end > 0 ? prev_end : 0);
            const bool inside = g.begin <= head.pos && head.pos < g.end;
            const bool inside_pending = lo <= head.pos && head.pos < g.end;
            if (!inside && !inside_pending) continue;
            for (int s = 0; s < S; ++s) {
                const int kind = it_pair_kind(a, s, region);
                const int64_t step = region * S + s;
                if (kind == PAIR_PENDING && inside_pending) pending = 1u;
                if (kind == PAIR_BYPASSED && inside && !bp && head.type != SK_INDEL_MISMATCH && (n_read_obs > 0 || first_contrib < step)) {
                    bypassed |= 1u << s;
                    last_writer = step > last_writer ? step : last_writer;
                }
            }
        }
        bypassed = it_wave_or(bypassed);
        pending = it_wave_or(pending);
        last_writer = it_wave_max(last_writer);
        if (lane == 0) {
            sk_indel_table_key out;
            out.pos = head.pos;
            out.type = int32_t(head.type);
            out.del_len = head.del_len;
            out.ins_len = head.ins_len;
            out.ins_off = ins_at;
            out.active_region_id = last_writer >= 0 ? a.regions[last_writer / S].begin : -1;
            const bool primitive = head.type == SK_INDEL_MISMATCH ||
                                   (head.type == SK_INDEL_INDEL && ((head.ins_len > 0 && head.del_len == 0) || (head.ins_len == 0 && head.del_len > 0)));
            out.flags = (primitive ? 0u : unsigned(SK_ITAB_DO_NOT_GENOTYPE)) | (pending ? unsigned(SK_ITAB_AR_PENDING) : 0u); // rule 4
            out.n_bp_obs = bp ? n_read_obs : 0u;
            ItKeySeq q;
            q.a = &a;
            q.head = head;
            it_report_info(q, &out);
            a.keys[key] = out;
        }
        if (lane < S) { // rule 6: in (region, record) order, which is the sorted order of the sample's CONTRIBUTION records
            sk_indel_table_sample_data d;
            int64_t at = a.id_at[j0];
            for (int s = 0; s < lane; ++s)
                for (int c = 0; c < SK_ITAB_N_SETS; ++c) at += s_count[s][c];
            for (int c = 0; c < SK_ITAB_N_SETS; ++c) {
                d.off[c] = at;
                d.count[c] = s_count[lane][c];
                at += s_count[lane][c];
            }
            int32_t hid = 0;
            float ratio = 0.0f;
            const unsigned nc = s_count[lane][IT_CLASS_CONTRIB];
            for (unsigned q = 0; q < nc; ++q) {
                const ItRec x = a.rec[idx[j0 + s_first[lane][IT_CLASS_CONTRIB] + q]];
                const sk_region_allele al = a.s[lane].alleles[x.id];
                hid += al.haplotype_id;              // (:750)
                ratio = __fadd_rn(ratio, al.ratio);  // (:755)
            }
            d.haplotype_id = hid;
            d.is_haplotyping_bypassed = (bypassed >> lane) & 1u;
            d.ratio = ratio;
            d.pad = 0;
            a.data[key * S + lane] = d;
        }
    }
}

struct ItLayout
{
    size_t ctl, obs_base, pair_off, rec, idx0, idx1, id_at, key_start, key_ins, total;
};
ItLayout itab_layout(const int32_t n_samples, const int64_t expand_cap, const int64_t region_cap)
{
    ItLayout l;
    const size_t e = size_t(expand_cap);
    size_t at = 0;
    auto take = [&](const size_t bytes) {
        const size_t off = at;
        at += sk_align256(bytes + 16);
        return off;
    };
    l.ctl = take(8 * CTL_WORDS);
    l.obs_base = take(8 * (SK_MAX_SAMPLES + 1));
    l.pair_off = take(8 * (size_t(region_cap) * size_t(n_samples) + 1));
    l.rec = take(sizeof(ItRec) * e);
    l.idx0 = take(4 * e);
    l.idx1 = take(4 * e);
    l.id_at = take(8 * (e + 1));
    l.key_start = take(8 * (e + 1));
    l.key_ins = take(8 * (e + 1));
    l.total = at + 256; // (the base is rounded up to 256 bytes)
    return l;
}

const int64_t IT_MAX_EXPAND = int64_t(1) << 30; // (record indices are 32-bit, IT_NONE aside)

} // namespace

extern "C" {

int64_t sk_indel_table_key_bound(int64_t n_obs_total, int64_t n_allele_records_total)
{
    if (n_obs_total < 0 || n_allele_records_total < 0) return -1;
    return n_obs_total + n_allele_records_total;
}

int64_t sk_indel_table_id_bound(int64_t n_obs_total, int64_t n_expanded_support_total)
{
    if (n_obs_total < 0 || n_expanded_support_total < 0) return -1;
    return n_obs_total + n_expanded_support_total;
}

int64_t sk_indel_table_insert_bound(int64_t n_read_bases_total, int64_t n_allele_insert_bytes_total)
{
    if (n_read_bases_total < 0 || n_allele_insert_bytes_total < 0) return -1;
    return n_read_bases_total + n_allele_insert_bytes_total;
}

size_t sk_indel_table_scratch_bytes(int32_t n_samples, int64_t expand_cap, int64_t region_cap)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES || expand_cap < 0 || expand_cap > IT_MAX_EXPAND || region_cap < 0 || region_cap > INT32_MAX / 4) return 0;
    return itab_layout(n_samples, expand_cap, region_cap).total;
}

int sk_indel_table_dev(int32_t n_samples, const sk_indel_table_sample* samples, const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len,
                       const sk_active_region* dev_regions, const int32_t* dev_n_regions, int64_t region_cap, int32_t prev_end_in, int64_t expand_cap,
                       sk_indel_table_key* dev_keys, int64_t key_cap, sk_indel_table_sample_data* dev_data, uint32_t* dev_id_pool, int64_t id_cap,
                       uint8_t* dev_insert_pool, int64_t insert_cap, int64_t* dev_totals, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return sk_fail("sk_indel_table_dev: n_samples must be in 1..SK_MAX_SAMPLES");
    if (ref_len < 0 || region_cap < 0 || expand_cap < 0 || key_cap < 0 || id_cap < 0 || insert_cap < 0) return sk_fail("sk_indel_table_dev: negative size");
    if (expand_cap > IT_MAX_EXPAND || region_cap > INT32_MAX / 4) return sk_fail("sk_indel_table_dev: expand_cap or region_cap beyond the index range");
    if (!samples || !dev_n_regions || !dev_totals || (ref_len > 0 && !dev_ref_seq) || (region_cap > 0 && !dev_regions)) return sk_fail("sk_indel_table_dev: null argument");
    if ((key_cap > 0 && (!dev_keys || !dev_data)) || (id_cap > 0 && !dev_id_pool) || (insert_cap > 0 && !dev_insert_pool)) return sk_fail("sk_indel_table_dev: null argument");
    for (int s = 0; s < n_samples; ++s) {
        const sk_indel_table_sample& sm = samples[s];
        if (sm.n_reads < 0 || sm.obs_cap < 0 || sm.support_cap < 0 || sm.allele_cap < 0 || sm.insert_cap < 0) return sk_fail("sk_indel_table_dev: negative size");
        if (sm.n_reads > 0 && (!sm.read_off || !sm.read_code || !sm.obs_off || !sm.iat)) return sk_fail("sk_indel_table_dev: null argument");
        if ((sm.obs_cap > 0 && !sm.obs) || (sm.support_cap > 0 && !sm.support_pool) || (sm.allele_cap > 0 && !sm.alleles) || (sm.insert_cap > 0 && !sm.insert_pool) ||
            (region_cap > 0 && (!sm.hap_recs || !sm.recs)))
            return sk_fail("sk_indel_table_dev: null argument");
    }
    if (!dev_scratch || scratch_bytes < sk_indel_table_scratch_bytes(n_samples, expand_cap, region_cap))
        return sk_fail("sk_indel_table_dev: scratch is below sk_indel_table_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const ItLayout lay = itab_layout(n_samples, expand_cap, region_cap);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    ItArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_samples = n_samples;
    for (int s = 0; s < n_samples; ++s) a.s[s] = samples[s];
    a.ref = dev_ref_seq;
    a.ref_offset = ref_offset;
    a.ref_len = ref_len;
    a.regions = dev_regions;
    a.n_regions = dev_n_regions;
    a.region_cap = region_cap;
    a.prev_end_in = prev_end_in;
    a.expand_cap = expand_cap;
    a.key_cap = key_cap;
    a.id_cap = id_cap;
    a.insert_cap = insert_cap;
    a.keys = dev_keys;
    a.data = dev_data;
    a.id_pool = dev_id_pool;
    a.insert_pool = dev_insert_pool;
    a.totals = dev_totals;
    a.ctl = reinterpret_cast<int64_t*>(scratch + lay.ctl);
    a.obs_base = reinterpret_cast<int64_t*>(scratch + lay.obs_base);
    a.pair_off = reinterpret_cast<int64_t*>(scratch + lay.pair_off);
    a.rec = reinterpret_cast<ItRec*>(scratch + lay.rec);
    a.idx[0] = reinterpret_cast<uint32_t*>(scratch + lay.idx0);
    a.idx[1] = reinterpret_cast<uint32_t*>(scratch + lay.idx1);
    a.id_at = reinterpret_cast<int64_t*>(scratch + lay.id_at);
    a.key_start = reinterpret_cast<int64_t*>(scratch + lay.key_start);
    a.key_ins = reinterpret_cast<int64_t*>(scratch + lay.key_ins);
    a.err = sk_ctx().dev_error_flags;
    SK_LAUNCH(itab_plan_kernel, dim3(1), dim3(IT_SCAN_T), 0, st, a);
    int from = 0;
    if (expand_cap > 0) {
        const int64_t tiles = (expand_cap + IT_TILE - 1) / IT_TILE;
        const unsigned grid = unsigned(tiles < IT_GRID ? tiles : int64_t(IT_GRID));
        SK_LAUNCH(itab_expand_kernel, dim3(2 * (grid < 8u ? 8u : grid)), dim3(IT_SCAN_T), 0, st, a);
        SK_LAUNCH(itab_sort_tile_kernel, dim3(unsigned(tiles)), dim3(IT_TILE), 0, st, a);
        for (int64_t width = IT_TILE; width < expand_cap; width *= 2) { // (a number of passes fixed by expand_cap: the count is on the device)
            const int64_t blocks = (expand_cap + 255) / 256;
            SK_LAUNCH(itab_merge_kernel, dim3(unsigned(blocks < 4 * IT_GRID ? blocks : int64_t(4 * IT_GRID))), dim3(256), 0, st, a, from, width);
            from ^= 1;
        }
    }
    SK_LAUNCH(itab_heads_kernel, dim3(1), dim3(IT_SCAN_T), 0, st, a, from);
    if (expand_cap > 0 && key_cap > 0) {
        const int64_t grid = key_cap < expand_cap ? key_cap : expand_cap;
        SK_LAUNCH(itab_key_kernel, dim3(unsigned(grid < 4 * IT_GRID ? grid : int64_t(4 * IT_GRID))), dim3(64), 0, st, a, from);
    }
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_indel_table(int32_t n_samples, const sk_indel_table_sample* samples, const char* ref_seq, int32_t ref_offset, int32_t ref_len,
                   const sk_active_region* regions, int32_t n_regions, int32_t prev_end_in, sk_indel_table_key* keys, int64_t key_cap,
                   sk_indel_table_sample_data* data, uint32_t* id_pool, int64_t id_cap, uint8_t* insert_pool, int64_t insert_cap, int64_t* totals)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return sk_fail("sk_indel_table: n_samples must be in 1..SK_MAX_SAMPLES");
    if (ref_len < 0 || n_regions < 0 || key_cap < 0 || id_cap < 0 || insert_cap < 0) return sk_fail("sk_indel_table: negative size");
    if (!samples || !totals || (ref_len > 0 && !ref_seq) || (n_regions > 0 && !regions)) return sk_fail("sk_indel_table: null argument");
    // what the arrays hold, and rule 9
    int64_t n_obs_total = 0, n_records_total = 0, n_support_total = 0, n_bases_total = 0, n_ins_total = 0;
    struct Sizes
    {
        int64_t n_obs, n_bases, n_alleles, n_ins, n_support;
    } sz[SK_MAX_SAMPLES];
    for (int s = 0; s < n_samples; ++s) {
        const sk_indel_table_sample& sm = samples[s];
        const std::string where = "sk_indel_table: sample " + std::to_string(s) + ": ";
        if (sm.n_reads < 0 || sm.obs_cap < 0 || sm.support_cap < 0 || sm.allele_cap < 0 || sm.insert_cap < 0) return sk_fail(where + "negative size");
        if (sm.n_reads > 0 && (!sm.read_off || !sm.read_code || !sm.obs_off || !sm.iat)) return sk_fail(where + "null argument");
        if ((sm.obs_cap > 0 && !sm.obs) || (sm.support_cap > 0 && !sm.support_pool) || (sm.allele_cap > 0 && !sm.alleles) || (sm.insert_cap > 0 && !sm.insert_pool) ||
            (n_regions > 0 && (!sm.hap_recs || !sm.recs)))
            return sk_fail(where + "null argument");
        Sizes& z = sz[s];
        z.n_obs = sm.n_reads > 0 ? sm.obs_off[sm.n_reads] : 0;
        z.n_bases = sm.n_reads > 0 ? sm.read_off[sm.n_reads] : 0;
        if (z.n_obs < 0 || z.n_obs > sm.obs_cap || z.n_bases < 0) return sk_fail(where + "the observations lie outside obs_cap");
        if (sm.n_reads > 0 && (sm.obs_off[0] != 0 || sm.read_off[0] != 0)) return sk_fail(where + "obs_off and read_off must begin at 0");
        for (int32_t r = 0; r < sm.n_reads; ++r) {
            if (sm.iat[r] > SK_IAT_SUBMAP) return sk_fail(where + "read " + std::to_string(r) + ": an iat above 2");
            const int64_t o0 = sm.obs_off[r], o1 = sm.obs_off[r + 1], b0 = sm.read_off[r], b1 = sm.read_off[r + 1];
            if (o0 < 0 || o1 < o0 || o1 > z.n_obs || b0 < 0 || b1 < b0 || b1 > z.n_bases) return sk_fail(where + "read " + std::to_string(r) + ": offsets descend");
            for (int64_t j = o0; j < o1; ++j) {
                const sk_intake_obs& o = sm.obs[j];
                if (o.type != SK_INDEL_INDEL && o.type != SK_INDEL_BP_LEFT && o.type != SK_INDEL_BP_RIGHT)
                    return sk_fail(where + "observation " + std::to_string(j) + ": a type the intake does not make");
                if (int64_t(o.ins_begin) + o.ins_len > b1 - b0) return sk_fail(where + "observation " + std::to_string(j) + ": the insert lies outside its read");
            }
        }
        z.n_alleles = z.n_ins = z.n_support = 0;
        for (int32_t i = 0; i < n_regions; ++i) {
            const sk_region_haplotypes_rec& h = sm.hap_recs[i];
            const sk_region_alleles_rec& rc = sm.recs[i];
            const bool pending = h.status == SK_HAP_NO_READS || h.status == SK_HAP_TOO_FEW_COVERING || h.status == SK_HAP_DECLINED || rc.status == SK_HAP_DECLINED;
            if (pending || h.status == SK_HAP_BYPASSED) continue;
            const std::string at = where + "region " + std::to_string(i) + ": ";
            if (rc.allele_off < 0 || rc.allele_off + int64_t(rc.n_alleles) > sm.allele_cap) return sk_fail(at + "the records lie outside allele_cap");
            for (uint32_t k = 0; k < rc.n_alleles; ++k) {
                const sk_region_allele& al = sm.alleles[rc.allele_off + k];
                if (al.type != SK_INDEL_INDEL && al.type != SK_INDEL_MISMATCH) return sk_fail(at + "a record of a type sk_region_alleles does not make");
                if (al.ins_off < 0 || al.ins_off + int64_t(al.ins_len) > sm.insert_cap) return sk_fail(at + "a record's insert lies outside insert_cap");
                z.n_ins = std::max(z.n_ins, al.ins_off + int64_t(al.ins_len));
                if (!al.to_indel_buffer) continue;
                if (al.hap_slot < 0 || al.hap_slot >= SK_HAP_MAX_SELECTED || uint32_t(al.hap_slot) >= h.n_selected) return sk_fail(at + "a record names a haplotype its region did not select");
                const sk_selected_haplotype& hp = h.hap[al.hap_slot];
                if (hp.support_off < 0 || hp.support_off + int64_t(hp.count) > sm.support_cap) return sk_fail(at + "a support list lies outside support_cap");
                for (uint32_t q = 0; q < hp.count; ++q) {
                    const int32_t r = sm.support_pool[hp.support_off + q];
                    if (r < 0 || r >= sm.n_reads) return sk_fail(at + "a support list names a read outside the sample");
                }
                z.n_support += hp.count;
            }
            z.n_alleles = std::max(z.n_alleles, rc.allele_off + int64_t(rc.n_alleles));
        }
        n_obs_total += z.n_obs;
        n_records_total += z.n_alleles;
        n_support_total += z.n_support;
        n_bases_total += z.n_bases;
        n_ins_total += z.n_ins;
    }
    const int64_t key_bound = sk_indel_table_key_bound(n_obs_total, n_records_total), id_bound = sk_indel_table_id_bound(n_obs_total, n_support_total),
                  insert_bound = sk_indel_table_insert_bound(n_bases_total, n_ins_total);
    if (key_cap < key_bound) return sk_fail("sk_indel_table: key_cap is below sk_indel_table_key_bound");
    if (id_cap < id_bound) return sk_fail("sk_indel_table: id_cap is below sk_indel_table_id_bound");
    if (insert_cap < insert_bound) return sk_fail("sk_indel_table: insert_cap is below sk_indel_table_insert_bound");
    if ((key_bound > 0 && (!keys || !data)) || (id_bound > 0 && !id_pool) || (insert_bound > 0 && !insert_pool)) return sk_fail("sk_indel_table: null argument");
    const int64_t expand_cap = n_obs_total + n_records_total + n_support_total;
    if (expand_cap > IT_MAX_EXPAND) return sk_fail("sk_indel_table: more expanded records than the index range");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t ng = size_t(n_regions);
    const size_t scratch_bytes = sk_indel_table_scratch_bytes(n_samples, expand_cap, n_regions);
    struct
    {
        sk_indel_table_sample s[SK_MAX_SAMPLES];
        char* ref; sk_active_region* regions; int32_t* n_regions; sk_indel_table_key* keys; sk_indel_table_sample_data* data; uint32_t* ids; uint8_t* ins;
        int64_t* totals; char* scratch;
    } d;
    int rc = 0;
    // (+ 16 bytes and the like: kernels may read whole words past an array's end; a piece starts at a multiple of 256 bytes)
    if (sk_carve(d, [&](SkArena& ar) {
            decltype(d) o{};
            for (int s = 0; s < n_samples; ++s) {
                const sk_indel_table_sample& sm = samples[s];
                const size_t nr = size_t(sm.n_reads);
                sk_indel_table_sample t = sm;
                t.read_off = ar.up(sm.read_off, nr ? nr + 1 : 0, 1, st, rc);
                t.read_code = ar.up(sm.read_code, size_t(sz[s].n_bases), 16, st, rc);
                t.obs_off = ar.up(sm.obs_off, nr ? nr + 1 : 0, 1, st, rc);
                t.obs = ar.up(sm.obs, size_t(sz[s].n_obs), 1, st, rc);
                t.obs_cap = sz[s].n_obs;
                t.align_id = sm.align_id ? ar.up(sm.align_id, nr, 1, st, rc) : nullptr;
                t.iat = ar.up(sm.iat, nr, 16, st, rc);
                t.hap_recs = ar.up(sm.hap_recs, ng, 1, st, rc);
                t.support_pool = ar.up(sm.support_pool, size_t(sm.support_cap), 1, st, rc);
                t.recs = ar.up(sm.recs, ng, 1, st, rc);
                t.alleles = ar.up(sm.alleles, size_t(sm.allele_cap), 1, st, rc);
                t.insert_pool = ar.up(sm.insert_pool, size_t(sm.insert_cap), 16, st, rc);
                o.s[s] = t;
            }
            o.ref = ar.up(ref_seq, size_t(ref_len), 16, st, rc);
            o.regions = ar.up(regions, ng, 2, st, rc);
            o.n_regions = ar.up(&n_regions, 1, 0, st, rc);
            o.keys = ar.take<sk_indel_table_key>(size_t(key_bound) + 1);
            o.data = ar.take<sk_indel_table_sample_data>(size_t(key_bound) * size_t(n_samples) + 1);
            o.ids = ar.take<uint32_t>(size_t(id_bound) + 4);
            o.ins = ar.take<uint8_t>(size_t(insert_bound) + 16);
            o.totals = ar.take<int64_t>(4);
            o.scratch = ar.take<char>(scratch_bytes + 16);
            return o;
        }) || rc)
        return 1;
    if (sk_indel_table_dev(n_samples, d.s, d.ref, ref_offset, ref_len, d.regions, d.n_regions, n_regions, prev_end_in, expand_cap, d.keys, key_bound, d.data, d.ids, id_bound,
                           d.ins, insert_bound, d.totals, d.scratch, scratch_bytes + 16, st))
        return 1;
    int64_t t[4] = { 0, 0, 0, 0 };
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    if (t[0] < 0 || t[0] > key_bound || t[1] < 0 || t[1] > id_bound || t[2] < 0 || t[2] > insert_bound) return sk_fail("sk_indel_table: totals out of range");
    if (t[0] > 0) {
        SK_HIP(skrt::memcpyAsync(keys, d.keys, sizeof(sk_indel_table_key) * size_t(t[0]), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(data, d.data, sizeof(sk_indel_table_sample_data) * size_t(t[0]) * size_t(n_samples), hipMemcpyDeviceToHost, st));
    }
    if (t[1] > 0) SK_HIP(skrt::memcpyAsync(id_pool, d.ids, sizeof(uint32_t) * size_t(t[1]), hipMemcpyDeviceToHost, st));
    if (t[2] > 0) SK_HIP(skrt::memcpyAsync(insert_pool, d.ins, size_t(t[2]), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    for (int q = 0; q < 4; ++q) totals[q] = t[q];
    return 0;
}

} // extern "C"
