// realign_gate.hip -- from the indel table and its candidacy to what a realignment job is made of: per key the sk_indel_info fields, per
// read the alignment zone, the gate's verdict and the observed list.  The rules are numbered in the header's block and restated one
// function each in tests/realign_gate_model.py.
//
//   G0  gate_check_kernel      every output to zero; block 0: what the host entry refuses (the paths' place and segment types, read
//       lengths, the order of align_id, the key and id counts against their rooms, the id sets tiling the pool, observed_cap)
//   G1  gate_obs_count_kernel  rule G5, the count: one thread per id of the pool finds its (key, sample, set) by a binary search over the
//       sets' offsets, drops it when an earlier set of the same (key, sample) holds the id too, finds the read by a binary search over
//       align_id and takes a place in the read's list with an integer atomicAdd; (read, key, place) are kept for G4
//   G2  gate_key_kernel        rule G1 and the shared record: one thread per key; also the key as realign_core.h reads it
//   G3  gate_read_kernel       rules G2-G4: one wave per read
//   G4  gate_obs_fill_kernel   rule G5, the lists: one block per sample scans the counts (block_scan.h plus the carried prefix), puts every
//       kept id's key at its place, then a wave per read writes the list in ascending order -- up to SK_RGATE_SORT_CAP entries from the
//       wave's registers, a longer list in passes of 64 over global memory; never truncated
//
// Input the host entry refuses raises SK_DEVERR_REALIGN_GATE and leaves zeroed output.
#include "sk_common.h"

#include "block_scan.h"
#include "libm_dbl64.h"
#include "realign_core.h"

#include <algorithm>
#include <climits>

namespace
{

enum { GATE_T = 256, GATE_GRID = 1024, GATE_READ_T = 256, GATE_FILL_T = 1024 };
enum { GC_BAD = 0, GC_KEYS, GC_IDS, GC_WORDS = 8 };

struct GatePlus
{
    __device__ int64_t operator()(const int64_t a, const int64_t b) const { return a + b; }
};

struct GateSample
{
    int32_t n_reads;
    const int32_t* pos;
    const int64_t* path_off;
    const int32_t* n_seg;
    const sk_path_seg* path;
    int64_t path_cap;
    const int32_t* read_len;
    const uint32_t* align_id;
    const int32_t* realign_begin;
    const int32_t* realign_end;
    sk_realign_gate_read* reads;
    int64_t* observed_off;
    int32_t* observed;
    int64_t observed_cap;
};

struct GateArgs
{
    int32_t n_samples;
    int32_t max_indel_size;
    GateSample s[SK_MAX_SAMPLES];
    const sk_indel_table_key* keys;
    const sk_indel_table_sample_data* data;
    const uint32_t* id_pool;
    const int64_t* table_totals;
    int64_t key_cap, id_cap;
    const sk_indel_candidate* cand;
    const sk_indel_error_rates* rates;
    sk_realign_gate_key* keys_out;
    sk_realign_gate_log_rates* logs;
    int64_t* totals; // [2 + SK_MAX_SAMPLES]
    int64_t* ctl;    // [GC_WORDS]
    skcore::PIndel* tab;             // [key_cap] the keys as range_iter and range_intersect_indel_breakpoints read them
    int32_t *o_read, *o_flat, *o_slot; // [id_cap] per id: its read (-1: dropped), key * n_samples + sample, its place in the read's list
    int32_t* tmp;                    // [n_samples][id_cap] the lists in arrival order
    int exact_libm;
    unsigned* err;
};

__device__ __forceinline__ void gate_refuse(const GateArgs& a)
{
    a.ctl[GC_BAD] = 1; // (every writer writes 1)
    atomicOr(a.err, unsigned(SK_DEVERR_REALIGN_GATE));
}

// G0
__global__ __launch_bounds__(GATE_T) void gate_check_kernel(const GateArgs a)
{
    const int64_t stride = int64_t(gridDim.x) * GATE_T, first = int64_t(blockIdx.x) * GATE_T + threadIdx.x;
    for (int64_t k = first; k < a.key_cap; k += stride) a.keys_out[k] = sk_realign_gate_key{};
    for (int64_t k = first; k < a.key_cap * a.n_samples; k += stride) a.logs[k] = sk_realign_gate_log_rates{ 0., 0. };
    for (int s = 0; s < a.n_samples; ++s) {
        const GateSample& sm = a.s[s];
        for (int64_t r = first; r < sm.n_reads; r += stride) sm.reads[r] = sk_realign_gate_read{ 0, 0, 0, 0, 0 };
        for (int64_t r = first; r <= sm.n_reads; r += stride) sm.observed_off[r] = 0;
        for (int64_t i = first; i < sm.observed_cap; i += stride) sm.observed[i] = 0;
    }
    if (blockIdx.x != 0) return;
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    const int64_t n_keys = a.table_totals[0], n_ids = a.table_totals[1];
    const bool counts_ok = n_keys >= 0 && n_keys <= a.key_cap && n_ids >= 0 && n_ids <= a.id_cap;
    if (!counts_ok) bad = true;
    for (int s = 0; s < a.n_samples; ++s) {
        const GateSample& sm = a.s[s];
        if (counts_ok && sm.observed_cap < n_ids) bad = true;
        for (int64_t r = threadIdx.x; r < sm.n_reads; r += GATE_T) {
            const int64_t off = sm.path_off[r];
            const int32_t ns = sm.n_seg[r];
            if (ns < 0 || off < 0 || off > sm.path_cap || int64_t(ns) > sm.path_cap - off || sm.read_len[r] < 0) {
                bad = true;
                continue;
            }
            for (int32_t i = 0; i < ns; ++i)
                if (sm.path[off + i].type > uint32_t(SK_SEG_SEQ_MISMATCH)) bad = true;
            if (sm.align_id && r > 0 && !(sm.align_id[r - 1] < sm.align_id[r])) bad = true;
        }
    }
    if (counts_ok) { // the id sets tile [0, n_ids) in (key, sample, set) order: G1's search relies on it
        const int64_t n_rec = n_keys * a.n_samples;
        if (n_rec == 0 && n_ids != 0) bad = true;
        for (int64_t f = threadIdx.x; f < n_rec; f += GATE_T) {
            const sk_indel_table_sample_data& d = a.data[f];
            int64_t at = 0;
            if (f > 0) at = a.data[f - 1].off[SK_ITAB_N_SETS - 1] + int64_t(a.data[f - 1].count[SK_ITAB_N_SETS - 1]);
            for (int c = 0; c < SK_ITAB_N_SETS; ++c) {
                if (d.off[c] != at) bad = true;
                at = d.off[c] + int64_t(d.count[c]);
            }
            if (f == n_rec - 1 && at != n_ids) bad = true;
        }
    }
    if (bad) s_bad = 1; // (every writer writes 1)
    __syncthreads();
    if (threadIdx.x == 0) {
        a.ctl[GC_BAD] = s_bad;
        a.ctl[GC_KEYS] = s_bad ? 0 : n_keys;
        a.ctl[GC_IDS] = s_bad ? 0 : n_ids;
        for (int i = 0; i < 2 + SK_MAX_SAMPLES; ++i) a.totals[i] = 0;
        if (s_bad) atomicOr(a.err, unsigned(SK_DEVERR_REALIGN_GATE));
    }
}

__device__ __forceinline__ bool gate_set_holds(const uint32_t* ids, const uint32_t n, const uint32_t id)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && ids[lo] == id;
}

// G1 -- rule G5, the count
__global__ __launch_bounds__(GATE_T) void gate_obs_count_kernel(const GateArgs a)
{
    if (a.ctl[GC_BAD]) return;
    const int64_t n_ids = a.ctl[GC_IDS];
    const int64_t n_sets = a.ctl[GC_KEYS] * a.n_samples * SK_ITAB_N_SETS;
    const int64_t stride = int64_t(gridDim.x) * GATE_T;
    for (int64_t j = int64_t(blockIdx.x) * GATE_T + threadIdx.x; j < n_ids; j += stride) {
        int64_t lo = 0, hi = n_sets; // the last set whose offset is not behind j: the sets tile the pool (G0), so it holds j
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.data[mid >> 2].off[mid & 3] <= j) lo = mid + 1;
            else hi = mid;
        }
        const int64_t g = lo - 1, f = g >> 2;
        const int c = int(g & 3), s = int(f % a.n_samples);
        const sk_indel_table_sample_data& d = a.data[f];
        const uint32_t id = a.id_pool[j];
        a.o_read[j] = -1;
        bool repeat = false; // the read sits in an earlier set of this (key, sample) too: the index appears once
        for (int e = 0; e < c && !repeat; ++e) repeat = gate_set_holds(a.id_pool + d.off[e], d.count[e], id);
        if (repeat) continue;
        const GateSample& sm = a.s[s];
        int64_t r = -1;
        if (!sm.align_id) {
            if (id < uint32_t(sm.n_reads)) r = id;
        } else {
            int32_t b = 0, e = sm.n_reads;
            while (b < e) {
                const int32_t mid = (b + e) >> 1;
                if (sm.align_id[mid] < id) b = mid + 1;
                else e = mid;
            }
            if (b < sm.n_reads && sm.align_id[b] == id) r = b;
        }
        if (r < 0) { // an id that belongs to none of the sample's reads
            gate_refuse(a);
            continue;
        }
        a.o_slot[j] = int32_t(atomicAdd(reinterpret_cast<unsigned long long*>(sm.observed_off + r + 1), 1ull));
        a.o_flat[j] = int32_t(f);
        a.o_read[j] = int32_t(r);
    }
}

// G2 -- rule G1 and the shared record
__global__ __launch_bounds__(GATE_T) void gate_key_kernel(const GateArgs a)
{
    if (a.ctl[GC_BAD]) return;
    const SkLibmTables lt = sk_libm_tables_default();
    const int64_t n_keys = a.ctl[GC_KEYS];
    const int64_t stride = int64_t(gridDim.x) * GATE_T;
    for (int64_t k = int64_t(blockIdx.x) * GATE_T + threadIdx.x; k < n_keys; k += stride) {
        const sk_indel_table_key key = a.keys[k];
        const sk_indel_candidate cd = a.cand[k];
        sk_realign_gate_key o{};
        o.pos = key.pos;
        o.type = key.type;
        o.del_len = key.del_len;
        o.ins_len = key.ins_len;
        o.ins_off = key.ins_off;
        o.active_region_id = key.active_region_id;
        o.is_candidate = cd.is_candidate;
        o.undecided = cd.undecided;
        skcore::PIndel p{};
        p.pos = key.pos;
        p.del = key.del_len;
        p.ins_len = key.ins_len;
        p.arid = key.active_region_id;
        p.type = uint8_t(key.type);
        p.cand = cd.is_candidate;
#pragma unroll
        for (int s = 0; s < SK_MAX_SAMPLES; ++s) { // (unrolled: the records' per-sample arrays stay in registers)
            if (s >= a.n_samples) break;
            const sk_indel_table_sample_data& d = a.data[k * a.n_samples + s];
            o.haplotype_id[s] = p.hap[s] = int8_t(d.haplotype_id);
            o.is_haplotyping_bypassed[s] = p.bypass[s] = uint8_t(d.is_haplotyping_bypassed != 0);
            const sk_indel_error_rates& rt = a.rates[k * a.n_samples + s];
            a.logs[k * a.n_samples + s] = sk_realign_gate_log_rates{ sk_log(rt.ref_to_indel, a.exact_libm, lt), sk_log(rt.indel_to_ref, a.exact_libm, lt) }; // rule G1
        }
        a.keys_out[k] = o;
        a.tab[k] = p;
    }
}

__device__ __forceinline__ uint32_t gate_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int32_t gate_wave_min(int32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int32_t gate_wave_max(int32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// G3 -- rules G2, G3 and G4: a wave per read, four reads to a block (a one-wave block that waits on memory
// leaves its CU short of waves)
__global__ __launch_bounds__(GATE_READ_T) void gate_read_kernel(const GateArgs a)
{
    if (a.ctl[GC_BAD]) return;
    const GateSample& sm = a.s[blockIdx.y];
    const int lane = threadIdx.x & 63;
    skcore::PJob job{};
    job.tab = a.tab;
    job.n_tab = int32_t(a.ctl[GC_KEYS]);
    job.max_indel_size = a.max_indel_size;
    const int64_t stride = int64_t(gridDim.x) * (GATE_READ_T / 64);
    for (int64_t r = int64_t(blockIdx.x) * (GATE_READ_T / 64) + (threadIdx.x >> 6); r < sm.n_reads; r += stride) { // (wave-uniform)
        const sk_path_seg* path = sm.path + sm.path_off[r];
        const int32_t ns = sm.n_seg[r], pos = sm.pos[r], read_len = sm.read_len[r];
        // the path, reduced: reference length, the first and last segment that is no unaligned edge, over-max, spliced
        uint32_t ref_len = 0, flags = 0;
        int32_t first_al = ns, last_al = -1;
        for (int32_t i = lane; i < ns; i += 64) {
            const sk_path_seg sg = path[i];
            if (skcore::seg_ref_len(sg.type)) ref_len += sg.length;
            if (!skcore::seg_unaligned_edge(sg.type)) {
                first_al = min(first_al, i);
                last_al = max(last_al, i);
            }
            if (i != 0 && i + 1 != ns && (sg.type == SK_SEG_INSERT || sg.type == SK_SEG_DELETE) && sg.length > uint32_t(a.max_indel_size)) flags |= 1u; // is_overmax
            if (sg.type == SK_SEG_SKIP) flags |= 2u;
        }
        ref_len = gate_wave_sum(ref_len);
        first_al = gate_wave_min(first_al);
        last_al = gate_wave_max(last_al);
        flags = uint32_t(__ballot(flags & 1u) != 0) | (uint32_t(__ballot(flags & 2u) != 0) << 1);
        uint32_t prefix = 0, suffix = 0; // unalignedPrefixSize, unalignedSuffixSize (a path of unaligned edges only: both are all of it)
        for (int32_t i = lane; i < ns; i += 64) {
            const sk_path_seg sg = path[i];
            if (!skcore::seg_read_len(sg.type)) continue;
            if (i < first_al) prefix += sg.length;
            if (i > last_al) suffix += sg.length;
        }
        prefix = gate_wave_sum(prefix);
        suffix = gate_wave_sum(suffix);
        const int32_t b = int32_t(uint32_t(pos) - prefix), e = int32_t(uint32_t(pos) + ref_len + suffix);
        const int32_t zb = max(0, min(b, int32_t(uint32_t(e) - uint32_t(read_len)))), ze = max(e, int32_t(uint32_t(b) + uint32_t(read_len)));
        const skcore::PRange zone = skcore::mk_range(zb, ze);
        int status;
        bool asked_undecided = false;
        if (flags & 2u) status = SK_RGATE_SPLICED;
        else if (flags & 1u) status = SK_RGATE_OVERMAX;
        else if (!skcore::superset_of(skcore::mk_range(sm.realign_begin[r], sm.realign_end[r]), zone)) status = SK_RGATE_OUTSIDE_RANGE;
        else {
            int lo, hi;
            skcore::range_iter(job, zb, ze, lo, hi); // (the same two searches in every lane)
            bool passed = false, any_undecided = false;
            for (int base = lo; base < hi && !passed; base += 64) {
                const int k = base + lane;
                bool inter = false, cand = false, und = false;
                if (k < hi) {
                    inter = skcore::range_intersect_indel_breakpoints(zone, a.tab[k]);
                    cand = inter && a.tab[k].cand != 0;
                    und = inter && a.cand[k].undecided != 0;
                }
                const unsigned long long m_cand = __ballot(cand), m_inter = __ballot(inter);
                // the keys asked: the intersecting ones up to and with the FIRST decided candidate, where the reference's loop returns
                const unsigned long long upto = m_cand ? ((m_cand & (~m_cand + 1)) << 1) - 1 : ~0ull;
                const unsigned long long m_asked = m_inter & upto;
                if ((m_asked >> lane) & 1) a.keys_out[k].gate_consulted = 1; // rule G4: a byte store of 1
                if (__ballot(und && ((m_asked >> lane) & 1))) any_undecided = true;
                passed = m_cand != 0;
            }
            asked_undecided = any_undecided;
            status = passed ? SK_RGATE_PASS : (any_undecided ? SK_RGATE_UNDECIDED : SK_RGATE_NO_CANDIDATE);
        }
        if (lane == 0) {
            sm.reads[r] = sk_realign_gate_read{ zb, ze, uint8_t(status), uint8_t(asked_undecided ? 1 : 0), 0 };
            if (status == SK_RGATE_PASS) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), 1ull);
            if (status == SK_RGATE_UNDECIDED) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), 1ull);
        }
    }
}

// G4 -- rule G5, the lists: one block per sample
__global__ __launch_bounds__(GATE_FILL_T) void gate_obs_fill_kernel(const GateArgs a)
{
    __shared__ int64_t s_wave[16];
    __shared__ int64_t s_total;
    const int s = blockIdx.x;
    const GateSample& sm = a.s[s];
    if (a.ctl[GC_BAD]) { // G1 may have counted before it met the id that no read owns
        for (int64_t r = threadIdx.x; r <= sm.n_reads; r += GATE_FILL_T) sm.observed_off[r] = 0;
        return;
    }
    // the offsets: observed_off[r + 1] holds read r's count; the inclusive scan in chunks of 1 024, the carried prefix added
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < sm.n_reads; c0 += GATE_FILL_T) {
        const int64_t i = c0 + threadIdx.x;
        const int64_t v = block_scan_1024(i < sm.n_reads ? sm.observed_off[i + 1] : int64_t(0), GatePlus(), s_wave);
        if (i < sm.n_reads) sm.observed_off[i + 1] = carry + v;
        if (threadIdx.x == GATE_FILL_T - 1) s_total = v;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.totals[2 + s] = carry;
    __syncthreads();
    int32_t* tmp = a.tmp + int64_t(s) * a.id_cap;
    const int64_t n_ids = a.ctl[GC_IDS];
    for (int64_t j = threadIdx.x; j < n_ids; j += GATE_FILL_T) {
        const int32_t r = a.o_read[j];
        if (r < 0) continue;
        const int32_t f = a.o_flat[j];
        if (f % a.n_samples != s) continue;
        tmp[sm.observed_off[r] + a.o_slot[j]] = f / a.n_samples;
    }
    __syncthreads();
    // a wave per read: every entry goes to the place its rank gives it (the entries of one list are distinct), so the result does not
    // depend on the order of arrival
    const int lane = threadIdx.x & 63;
    for (int64_t r = threadIdx.x >> 6; r < sm.n_reads; r += GATE_FILL_T / 64) {
        const int64_t at = sm.observed_off[r], n = sm.observed_off[r + 1] - at;
        if (n <= SK_RGATE_SORT_CAP) {
            const int32_t v = lane < n ? tmp[at + lane] : INT_MAX;
            int rank = 0;
            for (int j = 0; j < int(n); ++j) rank += __shfl(v, j, 64) < v ? 1 : 0;
            if (lane < n) sm.observed[at + rank] = v;
        } else {
            for (int64_t i0 = 0; i0 < n; i0 += 64) { // a pass per 64 entries, each ranked against the whole list in global memory
                const int64_t i = i0 + lane;
                const int32_t v = i < n ? tmp[at + i] : INT_MAX;
                int64_t rank = 0;
                for (int64_t j = 0; j < n; ++j) rank += tmp[at + j] < v ? 1 : 0;
                if (i < n) sm.observed[at + rank] = v;
            }
        }
    }
}

struct GateLayout
{
    size_t ctl, tab, o_read, o_flat, o_slot, tmp, total;
};
GateLayout gate_layout(const int32_t n_samples, const int64_t key_cap, const int64_t id_cap)
{
    GateLayout l;
    l.ctl = 0;
    l.tab = 256;
    l.o_read = l.tab + sk_align256(sizeof(skcore::PIndel) * size_t(key_cap));
    l.o_flat = l.o_read + sk_align256(sizeof(int32_t) * size_t(id_cap));
    l.o_slot = l.o_flat + sk_align256(sizeof(int32_t) * size_t(id_cap));
    l.tmp = l.o_slot + sk_align256(sizeof(int32_t) * size_t(id_cap));
    l.total = l.tmp + sk_align256(sizeof(int32_t) * size_t(id_cap) * size_t(n_samples)) + 256; // (+ 256: the block is aligned here)
    return l;
}

enum : int64_t { GATE_MAX_KEYS = int64_t(1) << 26, GATE_MAX_IDS = int64_t(1) << 30 }; // key * n_samples + sample and an id's index stay int32

// what both entries refuse of the sizes and pointers the host can read
const char* gate_args_issue(const int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* outs, const int64_t n_keys, const int64_t n_ids)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return "n_samples must be in 1..SK_MAX_SAMPLES";
    if (n_keys < 0 || n_ids < 0) return "negative size";
    if (n_keys > GATE_MAX_KEYS || n_ids > GATE_MAX_IDS) return "more keys than 2^26 or more ids than 2^30";
    if (!samples || !outs) return "null argument";
    for (int s = 0; s < n_samples; ++s) {
        const sk_realign_gate_sample& sm = samples[s];
        if (sm.n_reads < 0 || sm.path_cap < 0 || outs[s].observed_cap < 0) return "negative size";
        if ((sm.n_reads > 0 && (!sm.pos || !sm.path_off || !sm.n_seg || !sm.read_len || !sm.realign_begin || !sm.realign_end || !outs[s].reads)) || (sm.path_cap > 0 && !sm.path) ||
            !outs[s].observed_off || (outs[s].observed_cap > 0 && !outs[s].observed))
            return "null argument";
    }
    return nullptr;
}

} // namespace

extern "C" {

int64_t sk_realign_gate_observed_bound(int64_t n_ids) { return n_ids < 0 ? -1 : n_ids; }

size_t sk_realign_gate_scratch_bytes(int32_t n_samples, int64_t key_cap, int64_t id_cap)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES || key_cap < 0 || id_cap < 0 || key_cap > GATE_MAX_KEYS || id_cap > GATE_MAX_IDS) return 0;
    return gate_layout(n_samples, key_cap, id_cap).total;
}

int sk_realign_gate_dev(int32_t n_samples, const sk_realign_gate_sample* samples, const sk_indel_table_key* dev_keys, const sk_indel_table_sample_data* dev_data,
                        const uint32_t* dev_id_pool, const int64_t* dev_table_totals, int64_t key_cap, int64_t id_cap, const sk_indel_candidate* dev_cand,
                        const sk_indel_error_rates* dev_rates, uint32_t max_indel_size, sk_realign_gate_key* dev_keys_out, sk_realign_gate_log_rates* dev_logs,
                        const sk_realign_gate_sample_out* outs, int64_t* dev_totals, void* dev_scratch, size_t scratch_bytes, void* hip_stream)
{
    if (const char* issue = gate_args_issue(n_samples, samples, outs, key_cap, id_cap)) return sk_fail(std::string("sk_realign_gate_dev: ") + issue);
    if (max_indel_size > uint32_t(INT32_MAX)) return sk_fail("sk_realign_gate_dev: max_indel_size above INT32_MAX");
    if (!dev_table_totals || !dev_totals || (key_cap > 0 && (!dev_keys || !dev_data || !dev_cand || !dev_rates || !dev_keys_out || !dev_logs)) || (id_cap > 0 && !dev_id_pool))
        return sk_fail("sk_realign_gate_dev: null argument");
    if (!dev_scratch || scratch_bytes < sk_realign_gate_scratch_bytes(n_samples, key_cap, id_cap)) return sk_fail("sk_realign_gate_dev: scratch is below sk_realign_gate_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const GateLayout lay = gate_layout(n_samples, key_cap, id_cap);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    GateArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_samples = n_samples;
    a.max_indel_size = int32_t(max_indel_size);
    int64_t zero_max = key_cap * n_samples;
    int32_t reads_max = 0;
    for (int s = 0; s < n_samples; ++s) {
        const sk_realign_gate_sample& sm = samples[s];
        a.s[s] = GateSample{ sm.n_reads, sm.pos, sm.path_off, sm.n_seg, sm.path, sm.path_cap, sm.read_len, sm.align_id, sm.realign_begin, sm.realign_end,
                             outs[s].reads, outs[s].observed_off, outs[s].observed, outs[s].observed_cap };
        if (sm.n_reads > reads_max) reads_max = sm.n_reads;
        if (int64_t(sm.n_reads) + 1 > zero_max) zero_max = int64_t(sm.n_reads) + 1;
        if (outs[s].observed_cap > zero_max) zero_max = outs[s].observed_cap;
    }
    a.keys = dev_keys;
    a.data = dev_data;
    a.id_pool = dev_id_pool;
    a.table_totals = dev_table_totals;
    a.key_cap = key_cap;
    a.id_cap = id_cap;
    a.cand = dev_cand;
    a.rates = dev_rates;
    a.keys_out = dev_keys_out;
    a.logs = dev_logs;
    a.totals = dev_totals;
    a.ctl = reinterpret_cast<int64_t*>(scratch + lay.ctl);
    a.tab = reinterpret_cast<skcore::PIndel*>(scratch + lay.tab);
    a.o_read = reinterpret_cast<int32_t*>(scratch + lay.o_read);
    a.o_flat = reinterpret_cast<int32_t*>(scratch + lay.o_flat);
    a.o_slot = reinterpret_cast<int32_t*>(scratch + lay.o_slot);
    a.tmp = reinterpret_cast<int32_t*>(scratch + lay.tmp);
    a.exact_libm = sk_ctx().libm_restated ? 1 : 0;
    a.err = sk_ctx().dev_error_flags;
    const auto grid_of = [](const int64_t n, const int64_t per_block) {
        const int64_t blocks = (n + per_block - 1) / per_block;
        return unsigned(blocks < 1 ? 1 : (blocks < GATE_GRID ? blocks : int64_t(GATE_GRID)));
    };
    // five launches, whatever the arrays hold
    SK_LAUNCH(gate_check_kernel, dim3(grid_of(zero_max, GATE_T)), dim3(GATE_T), 0, st, a);
    SK_LAUNCH(gate_obs_count_kernel, dim3(grid_of(id_cap, GATE_T)), dim3(GATE_T), 0, st, a);
    SK_LAUNCH(gate_key_kernel, dim3(grid_of(key_cap, GATE_T)), dim3(GATE_T), 0, st, a);
    SK_LAUNCH(gate_read_kernel, dim3(grid_of(reads_max, GATE_READ_T / 64), unsigned(n_samples)), dim3(GATE_READ_T), 0, st, a);
    SK_LAUNCH(gate_obs_fill_kernel, dim3(unsigned(n_samples)), dim3(GATE_FILL_T), 0, st, a);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_realign_gate(int32_t n_samples, const sk_realign_gate_sample* samples, const sk_indel_table_key* keys, const sk_indel_table_sample_data* data,
                    const uint32_t* id_pool, int64_t n_keys, int64_t n_ids, const sk_indel_candidate* cand, const sk_indel_error_rates* rates,
                    uint32_t max_indel_size, sk_realign_gate_key* keys_out, sk_realign_gate_log_rates* logs, const sk_realign_gate_sample_out* outs,
                    int64_t* totals)
{
    if (const char* issue = gate_args_issue(n_samples, samples, outs, n_keys, n_ids)) return sk_fail(std::string("sk_realign_gate: ") + issue);
    if (max_indel_size > uint32_t(INT32_MAX)) return sk_fail("sk_realign_gate: max_indel_size above INT32_MAX");
    if (!totals || (n_keys > 0 && (!keys || !data || !cand || !rates || !keys_out || !logs)) || (n_ids > 0 && !id_pool)) return sk_fail("sk_realign_gate: null argument");
    for (int s = 0; s < n_samples; ++s) {
        const sk_realign_gate_sample& sm = samples[s];
        if (outs[s].observed_cap < sk_realign_gate_observed_bound(n_ids))
            return sk_fail("sk_realign_gate: sample " + std::to_string(s) + ": observed_cap is below sk_realign_gate_observed_bound");
        for (int32_t r = 0; r < sm.n_reads; ++r) {
            const std::string where = "sk_realign_gate: sample " + std::to_string(s) + ": read " + std::to_string(r) + ": ";
            if (sm.n_seg[r] < 0) return sk_fail(where + "a negative n_seg");
            if (sm.read_len[r] < 0) return sk_fail(where + "a negative read_len");
            if (sm.path_off[r] < 0 || sm.path_off[r] > sm.path_cap || int64_t(sm.n_seg[r]) > sm.path_cap - sm.path_off[r]) return sk_fail(where + "the path lies outside path_cap");
            for (int32_t i = 0; i < sm.n_seg[r]; ++i)
                if (sm.path[sm.path_off[r] + i].type > uint32_t(SK_SEG_SEQ_MISMATCH)) return sk_fail(where + "a segment type above SK_SEG_SEQ_MISMATCH");
            if (sm.align_id && r > 0 && !(sm.align_id[r - 1] < sm.align_id[r])) return sk_fail(where + "align_id is not strictly ascending");
        }
    }
    int64_t at = 0;
    for (int64_t f = 0; f < n_keys * n_samples; ++f) {
        const int s = int(f % n_samples);
        const sk_realign_gate_sample& sm = samples[s];
        for (int c = 0; c < SK_ITAB_N_SETS; ++c) {
            if (data[f].off[c] != at || int64_t(data[f].count[c]) > n_ids - at)
                return sk_fail("sk_realign_gate: key " + std::to_string(f / n_samples) + ": the id sets do not tile id_pool in (key, sample, set) order");
            for (uint32_t i = 0; i < data[f].count[c]; ++i) {
                const uint32_t id = id_pool[at + i];
                const bool owned = sm.align_id ? std::binary_search(sm.align_id, sm.align_id + sm.n_reads, id) : id < uint32_t(sm.n_reads);
                if (!owned) return sk_fail("sk_realign_gate: key " + std::to_string(f / n_samples) + ": sample " + std::to_string(s) + ": an id that belongs to none of the sample's reads");
            }
            at += int64_t(data[f].count[c]);
        }
    }
    if (at != n_ids) return sk_fail("sk_realign_gate: the id sets do not tile id_pool in (key, sample, set) order");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nk = size_t(n_keys), ni = size_t(n_ids), ns = size_t(n_samples);
    const size_t scratch_bytes = sk_realign_gate_scratch_bytes(n_samples, n_keys, n_ids);
    const int64_t table_totals[4] = { n_keys, n_ids, 0, 0 };
    struct
    {
        sk_realign_gate_sample in[SK_MAX_SAMPLES];
        sk_realign_gate_sample_out out[SK_MAX_SAMPLES];
        sk_indel_table_key* keys; sk_indel_table_sample_data* data; uint32_t* id_pool; int64_t* table_totals; sk_indel_candidate* cand; sk_indel_error_rates* rates;
        sk_realign_gate_key* keys_out; sk_realign_gate_log_rates* logs; int64_t* totals; char* scratch;
    } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            decltype(d) o{};
            for (int s = 0; s < n_samples; ++s) {
                const sk_realign_gate_sample& sm = samples[s];
                const size_t nr = size_t(sm.n_reads);
                sk_realign_gate_sample t = sm;
                t.pos = ar.up(sm.pos, nr, 1, st, rc);
                t.path_off = ar.up(sm.path_off, nr, 1, st, rc);
                t.n_seg = ar.up(sm.n_seg, nr, 1, st, rc);
                t.path = ar.up(sm.path, size_t(sm.path_cap), 1, st, rc);
                t.read_len = ar.up(sm.read_len, nr, 1, st, rc);
                if (sm.align_id) t.align_id = ar.up(sm.align_id, nr, 1, st, rc);
                t.realign_begin = ar.up(sm.realign_begin, nr, 1, st, rc);
                t.realign_end = ar.up(sm.realign_end, nr, 1, st, rc);
                o.in[s] = t;
                o.out[s].reads = ar.take<sk_realign_gate_read>(nr + 1);
                o.out[s].observed_off = ar.take<int64_t>(nr + 1);
                o.out[s].observed = ar.take<int32_t>(ni + 1);
                o.out[s].observed_cap = n_ids;
            }
            o.keys = ar.up(keys, nk, 1, st, rc);
            o.data = ar.up(data, nk * ns, 1, st, rc);
            o.id_pool = ar.up(id_pool, ni, 1, st, rc);
            o.table_totals = ar.up(table_totals, 4, 0, st, rc);
            o.cand = ar.up(cand, nk, 1, st, rc);
            o.rates = ar.up(rates, nk * ns, 1, st, rc);
            o.keys_out = ar.take<sk_realign_gate_key>(nk + 1);
            o.logs = ar.take<sk_realign_gate_log_rates>(nk * ns + 1);
            o.totals = ar.take<int64_t>(2 + SK_MAX_SAMPLES);
            o.scratch = ar.take<char>(scratch_bytes + 16);
            return o;
        }) || rc)
        return 1;
    if (sk_realign_gate_dev(n_samples, d.in, d.keys, d.data, d.id_pool, d.table_totals, n_keys, n_ids, d.cand, d.rates, max_indel_size, d.keys_out, d.logs, d.out, d.totals,
                            d.scratch, scratch_bytes + 16, st))
        return 1;
    int64_t t[2 + SK_MAX_SAMPLES];
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st)); // (the observed entries to copy back are a count on the device)
    if (sk_check_device_errors()) return 1;
    if (n_keys > 0) {
        SK_HIP(skrt::memcpyAsync(keys_out, d.keys_out, sizeof(sk_realign_gate_key) * nk, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(logs, d.logs, sizeof(sk_realign_gate_log_rates) * nk * ns, hipMemcpyDeviceToHost, st));
    }
    for (int s = 0; s < n_samples; ++s) {
        const size_t nr = size_t(samples[s].n_reads);
        if (t[2 + s] < 0 || t[2 + s] > n_ids) return sk_fail("sk_realign_gate: the device left an observed count outside the pool");
        if (nr > 0) SK_HIP(skrt::memcpyAsync(outs[s].reads, d.out[s].reads, sizeof(sk_realign_gate_read) * nr, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(outs[s].observed_off, d.out[s].observed_off, sizeof(int64_t) * (nr + 1), hipMemcpyDeviceToHost, st));
        if (t[2 + s] > 0) SK_HIP(skrt::memcpyAsync(outs[s].observed, d.out[s].observed, sizeof(int32_t) * size_t(t[2 + s]), hipMemcpyDeviceToHost, st));
    }
    SK_HIP(skrt::streamSynchronize(st));
    for (int i = 0; i < 2 + SK_MAX_SAMPLES; ++i) totals[i] = t[i];
    return 0;
}

} // extern "C"
