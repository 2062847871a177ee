// realign_preamble.hip -- from the realignment gate's outputs to what the device realignment job starts from: one skcore::PRead per read
// that passed the gate, made by the rules P1-P5 of preamble_core.h (numbered in the header's block; the container-based statement in
// host/read_realign.cpp is the yardstick).
//
//   R0  pre_check_kernel    every output to zero; the keys as realign_core.h reads them; block 0: what the host entry refuses (the
//       paths' place and segment types, read lengths, the gate's status bytes, read_off, the observed lists, the keys' order and inserts)
//   R1  pre_slot_kernel     one block: the reads that passed the gate, counted in (sample, read) order (block_scan.h plus the carried
//       prefix); record_cap below the count is refused; each passing read gets a slot, every other read its status byte
//   R2  pre_read_kernel     rules P1-P5: one wave per slot.  Lane 0 walks the path (P1, P2, P4, P5); the keys of the exemplar range
//       are taken 64 to a turn, each lane tests adjacency, intersection and usability for its key, and a ballot and a prefix popcount
//       give the status map, which is ascending because the range is.  The record is built in LDS and leaves in 16-byte stores.
//   R3  pre_rank_kernel     one block: the slots whose status is SK_RPRE_OK, counted in order; source[] and the totals
//   R4  pre_copy_kernel     a wave per slot moves its record to its place
//
// Input the host entry refuses raises SK_DEVERR_REALIGN_PREAMBLE and leaves zeroed output.
#include "sk_common.h"

#include "block_scan.h"
#include "preamble_core.h"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

namespace
{

using skcore::PRead;

// sk_realign_prepared_read is skcore::PRead under its public name: the enumeration can take the array where it lies
#define PRE_SAME(pub, core) static_assert(offsetof(sk_realign_prepared_read, pub) == offsetof(PRead, core), "sk_realign_prepared_read." #pub)
static_assert(sizeof(sk_realign_prepared_read) == sizeof(PRead) && sizeof(PRead) == 784 && alignof(sk_realign_prepared_read) == alignof(PRead), "sk_realign_prepared_read");
PRE_SAME(realign_begin, realign_b);
PRE_SAME(realign_end, realign_e);
PRE_SAME(read_length, read_length);
PRE_SAME(sample, sample);
PRE_SAME(exemplar_range, exemplar_range);
PRE_SAME(alignment, cal);
PRE_SAME(status_map, sm);
PRE_SAME(order, order);
PRE_SAME(observed, observed);
PRE_SAME(n_status, n_sm);
PRE_SAME(n_order, n_order);
PRE_SAME(n_observed, n_observed);
PRE_SAME(clipped, clipped);
PRE_SAME(hc_lead, hc_lead);
PRE_SAME(hc_trail, hc_trail);
PRE_SAME(sc_lead, sc_lead);
PRE_SAME(sc_trail, sc_trail);
#undef PRE_SAME
#define PRE_SAME(pub_t, pub, core_t, core) static_assert(sizeof(pub_t) == sizeof(core_t) && offsetof(pub_t, pub) == offsetof(core_t, core), #pub_t "." #pub)
PRE_SAME(sk_realign_prepared_range, b, skcore::PRange, b);
PRE_SAME(sk_realign_prepared_range, e, skcore::PRange, e);
PRE_SAME(sk_realign_prepared_range, has_b, skcore::PRange, has_b);
PRE_SAME(sk_realign_prepared_range, has_e, skcore::PRange, has_e);
PRE_SAME(sk_realign_prepared_seg, type, skcore::PSeg, type);
PRE_SAME(sk_realign_prepared_seg, length, skcore::PSeg, length);
PRE_SAME(sk_realign_prepared_status, idx, skcore::PStatus, idx);
PRE_SAME(sk_realign_prepared_status, is_present, skcore::PStatus, is_present);
PRE_SAME(sk_realign_prepared_status, is_remove_only, skcore::PStatus, is_remove_only);
PRE_SAME(sk_realign_prepared_status, in_original, skcore::PStatus, in_original);
PRE_SAME(sk_realign_prepared_status, pad, skcore::PStatus, pad);
PRE_SAME(sk_realign_prepared_alignment, pos, skcore::PCal, pos);
PRE_SAME(sk_realign_prepared_alignment, lead, skcore::PCal, lead);
PRE_SAME(sk_realign_prepared_alignment, trail, skcore::PCal, trail);
PRE_SAME(sk_realign_prepared_alignment, is_fwd_strand, skcore::PCal, fwd);
PRE_SAME(sk_realign_prepared_alignment, n_seg, skcore::PCal, n_seg);
PRE_SAME(sk_realign_prepared_alignment, n_indels, skcore::PCal, n_indels);
PRE_SAME(sk_realign_prepared_alignment, pad, skcore::PCal, pad);
PRE_SAME(sk_realign_prepared_alignment, path, skcore::PCal, path);
PRE_SAME(sk_realign_prepared_alignment, indels, skcore::PCal, indels);
#undef PRE_SAME
static_assert(int(SK_RPRE_K) == int(skcore::Caps::K) && int(SK_RPRE_P) == int(skcore::Caps::P) && int(SK_RPRE_OBS) == int(skcore::Caps::OBS), "SK_RPRE_* capacities");

enum { PRE_T = 256, PRE_GRID = 1024, PRE_SCAN_T = 1024, PRE_REC_VEC = int(sizeof(PRead) / 16) };
enum { PC_BAD = 0, PC_KEYS, PC_HAS_MM, PC_PASS, PC_WORDS = 8 };
static_assert(sizeof(PRead) % 16 == 0 && PRE_REC_VEC <= 64, "a record leaves in one 16-byte store per lane");

struct PrePlus
{
    SKC_HD int64_t operator()(const int64_t a, const int64_t b) const { return a + b; }
};

struct PreSample
{
    int32_t n_reads;
    const int32_t* pos;
    const int64_t* path_off;
    const int32_t* n_seg;
    const sk_path_seg* path;
    int64_t path_cap;
    const int32_t* read_len;
    const int32_t* realign_begin;
    const int32_t* realign_end;
    const sk_realign_gate_read* gate;
    const int64_t* observed_off;
    const int32_t* observed;
    int64_t observed_cap;
    const uint8_t* code;
    const int64_t* read_off;
    int64_t code_cap;
    const uint8_t* fwd;
    uint8_t* status;
};

struct PreArgs // the one argument record: the kernels take it over device memory, the host hook over host memory
{
    int32_t n_samples;
    int32_t max_indel_size;
    PreSample s[SK_MAX_SAMPLES];
    const sk_realign_gate_key* keys;
    const int64_t* table_totals;
    int64_t key_cap;
    const uint8_t* ins_pool;
    int64_t ins_cap;
    const char* ref;
    int32_t ref_offset, ref_len;
    PRead* records;
    sk_realign_prepared_source* source;
    int64_t record_cap;
    uint8_t* consulted;
    int64_t* totals; // [SK_RPRE_N_TOTALS]
    int64_t* ctl;    // [PC_WORDS]
    skcore::PIndel* tab;                  // [key_cap]
    sk_realign_prepared_source* slot_src; // [record_cap] the passing reads in order
    int32_t* slot_status;                 // [record_cap] SK_RPRE_* of each
    int32_t* slot_dst;                    // [record_cap] its record's place, -1: none
    PRead* tmp;                           // [record_cap] the records by slot
    unsigned* err;
};

SKC_HD inline skcore::PIndel pre_tab_entry(const sk_realign_gate_key& k)
{
    skcore::PIndel p{};
    p.pos = k.pos;
    p.del = k.del_len;
    p.ins_len = k.ins_len;
    p.arid = k.active_region_id;
    p.type = uint8_t(k.type);
    p.cand = k.is_candidate;
    p.ins_off = uint32_t(k.ins_off);
    return p;
}
// what is refused of key k (the one before it is read too)
SKC_HD inline bool pre_key_bad(const PreArgs& a, const int64_t k)
{
    const sk_realign_gate_key& e = a.keys[k];
    if (e.type <= SK_INDEL_NONE || e.type > SK_INDEL_BP_RIGHT) return true;
    if (e.ins_off < 0 || e.ins_off > a.ins_cap || int64_t(e.ins_len) > a.ins_cap - e.ins_off) return true;
    return k > 0 && a.keys[k - 1].pos > e.pos;
}
// what is refused of read r of sample sm, given n_keys
SKC_HD inline bool pre_read_bad(const PreSample& sm, const int64_t r, const int64_t n_keys)
{
    const int64_t off = sm.path_off[r];
    const int32_t ns = sm.n_seg[r];
    if (ns < 0 || off < 0 || off > sm.path_cap || int64_t(ns) > sm.path_cap - off || sm.read_len[r] < 0) return true;
    for (int32_t i = 0; i < ns; ++i)
        if (sm.path[off + i].type > uint32_t(SK_SEG_SEQ_MISMATCH)) return true;
    if (sm.gate[r].status > uint8_t(SK_RGATE_SPLICED)) return true;
    const int64_t cb = sm.read_off[r], ce = sm.read_off[r + 1];
    if (cb < 0 || ce < cb || ce > sm.code_cap) return true;
    const int64_t ob = sm.observed_off[r], oe = sm.observed_off[r + 1];
    if (ob < 0 || oe < ob || oe > sm.observed_cap) return true;
    for (int64_t i = ob; i < oe; ++i)
        if (sm.observed[i] < 0 || sm.observed[i] >= n_keys || (i > ob && !(sm.observed[i - 1] < sm.observed[i]))) return true;
    return false;
}
SKC_HD inline skcore::PreRead pre_read_of(const PreSample& sm, const int32_t sample, const int64_t r)
{
    skcore::PreRead in;
    in.pos = sm.pos[r];
    in.n_seg = sm.n_seg[r];
    in.read_len = sm.read_len[r];
    in.sample = sample;
    in.realign_b = sm.realign_begin[r];
    in.realign_e = sm.realign_end[r];
    in.fwd = sm.fwd ? int32_t(sm.fwd[r] != 0) : 1;
    in.path = sm.path + sm.path_off[r];
    in.code = sm.code + sm.read_off[r];
    in.n_code = int32_t(sm.read_off[r + 1] - sm.read_off[r] < int64_t(INT32_MAX) ? sm.read_off[r + 1] - sm.read_off[r] : int64_t(INT32_MAX));
    in.observed = sm.observed + sm.observed_off[r];
    in.n_observed = int32_t(sm.observed_off[r + 1] - sm.observed_off[r]);
    return in;
}
SKC_HD inline skcore::PreTable pre_table_of(const PreArgs& a)
{
    skcore::PreTable t{};
    t.job.tab = a.tab;
    t.job.n_tab = int32_t(a.ctl[PC_KEYS]);
    t.job.max_indel_size = a.max_indel_size;
    t.ins_pool = a.ins_pool;
    t.has_mismatch_keys = int32_t(a.ctl[PC_HAS_MM]);
    t.ref = a.ref;
    t.ref_offset = a.ref_offset;
    t.ref_len = a.ref_len;
    t.consulted = a.consulted;
    return t;
}

// R0
__global__ __launch_bounds__(PRE_T) void pre_check_kernel(const PreArgs a)
{
    const int64_t stride = int64_t(gridDim.x) * PRE_T, first = int64_t(blockIdx.x) * PRE_T + threadIdx.x;
    uint4* const rec = reinterpret_cast<uint4*>(a.records);
    for (int64_t i = first; i < a.record_cap * PRE_REC_VEC; i += stride) rec[i] = uint4{ 0, 0, 0, 0 };
    for (int64_t i = first; i < a.record_cap; i += stride) a.source[i] = sk_realign_prepared_source{ 0, 0 };
    for (int64_t k = first; k < a.key_cap; k += stride) a.consulted[k] = 0;
    for (int s = 0; s < a.n_samples; ++s)
        for (int64_t r = first; r < a.s[s].n_reads; r += stride) a.s[s].status[r] = SK_RPRE_NONE;
    const int64_t n_keys = a.table_totals[0];
    const bool count_ok = n_keys >= 0 && n_keys <= a.key_cap;
    if (count_ok)
        for (int64_t k = first; k < n_keys; k += stride) a.tab[k] = pre_tab_entry(a.keys[k]);
    if (blockIdx.x != 0) return;
    __shared__ int s_bad, s_mm;
    if (threadIdx.x == 0) s_bad = s_mm = 0;
    __syncthreads();
    bool bad = !count_ok, mm = false;
    if (count_ok) {
        for (int64_t k = threadIdx.x; k < n_keys; k += PRE_T) {
            if (pre_key_bad(a, k)) bad = true;
            if (a.keys[k].type == SK_INDEL_MISMATCH) mm = true;
        }
        for (int s = 0; s < a.n_samples; ++s)
            for (int64_t r = threadIdx.x; r < a.s[s].n_reads; r += PRE_T)
                if (pre_read_bad(a.s[s], r, n_keys)) bad = true;
    }
    if (bad) s_bad = 1; // (every writer writes 1)
    if (mm) s_mm = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.ctl[PC_BAD] = s_bad;
        a.ctl[PC_KEYS] = s_bad ? 0 : n_keys;
        a.ctl[PC_HAS_MM] = s_mm;
        a.ctl[PC_PASS] = 0;
        for (int i = 0; i < SK_RPRE_N_TOTALS; ++i) a.totals[i] = 0;
        if (s_bad) atomicOr(a.err, unsigned(SK_DEVERR_REALIGN_PREAMBLE));
    }
}

// R1: one block
__global__ __launch_bounds__(PRE_SCAN_T) void pre_slot_kernel(const PreArgs a)
{
    __shared__ int64_t s_wave[16];
    __shared__ int64_t s_total;
    if (a.ctl[PC_BAD]) return;
    for (int pass = 0; pass < 2; ++pass) { // the count first: nothing is written for a record_cap that is refused
        int64_t carry = 0;
        for (int s = 0; s < a.n_samples; ++s) {
            const PreSample& sm = a.s[s];
            for (int64_t c0 = 0; c0 < sm.n_reads; c0 += PRE_SCAN_T) {
                const int64_t r = c0 + threadIdx.x;
                const bool passed = r < sm.n_reads && sm.gate[r].status == SK_RGATE_PASS;
                const int64_t v = block_scan_1024(int64_t(passed ? 1 : 0), PrePlus(), s_wave);
                if (pass == 1 && r < sm.n_reads) {
                    if (passed) a.slot_src[carry + v - 1] = sk_realign_prepared_source{ s, int32_t(r) };
                    else sm.status[r] = SK_RPRE_NOT_PASSED;
                }
                if (threadIdx.x == PRE_SCAN_T - 1) s_total = v;
                __syncthreads();
                carry += s_total;
                __syncthreads();
            }
        }
        if (pass == 0 && carry > a.record_cap) { // (the same in every thread)
            if (threadIdx.x == 0) {
                a.ctl[PC_BAD] = 1;
                atomicOr(a.err, unsigned(SK_DEVERR_REALIGN_PREAMBLE));
            }
            return;
        }
        if (pass == 1 && threadIdx.x == 0) a.ctl[PC_PASS] = carry;
    }
}

// R2 -- rules P1-P5: a wave per passing read.  A block is one wave: the waves of a block would wait for each other at every step, and a
// read's steps differ in length with its path and its range.
__global__ __launch_bounds__(64) void pre_read_kernel(const PreArgs a)
{
    __shared__ __align__(16) PRead s_rec;
    __shared__ int s_status;
    __shared__ skcore::PRange s_exemplar;
    if (a.ctl[PC_BAD]) return;
    const int lane = threadIdx.x;
    const int64_t n_pass = a.ctl[PC_PASS];
    const skcore::PreTable t = pre_table_of(a);
    for (int64_t slot = blockIdx.x; slot < n_pass; slot += gridDim.x) { // (block-uniform)
        const sk_realign_prepared_source src = a.slot_src[slot];
        const PreSample& sm = a.s[src.sample];
        const skcore::PreRead in = pre_read_of(sm, src.sample, src.read);
        if (lane < PRE_REC_VEC) reinterpret_cast<uint4*>(&s_rec)[lane] = uint4{ 0, 0, 0, 0 };
        __syncthreads();
        if (lane == 0) {
            skcore::PRange ex = skcore::mk_range(0, 0);
            s_status = skcore::pre_before_map(t, in, s_rec, ex);
            s_exemplar.b = ex.b;
            s_exemplar.e = ex.e;
        }
        __syncthreads();
        int status = s_status;
        if (status == SK_RPRE_OK) { // (wave-uniform)
            const skcore::PRange ex = skcore::mk_range(s_exemplar.b, s_exemplar.e);
            int lo, hi, n = 0;
            skcore::range_iter(t.job, ex.b, ex.e, lo, hi); // (the same two searches in every lane)
            for (int base = lo; base < hi; base += 64) {
                const int k = base + lane;
                const int state = k < hi ? skcore::pre_key_state(t, in, ex, k, true) : 0;
                const unsigned long long m = __ballot(state != 0);
                const int at = n + __popcll(m & ((1ull << lane) - 1));
                if (state && at < skcore::Caps::K) skcore::pre_put_status(s_rec, at, k, state);
                n += __popcll(m);
            }
            if (lane == 0) s_rec.n_sm = uint8_t(n < skcore::Caps::K ? n : int(skcore::Caps::K));
            __syncthreads();
            if (lane == 0) s_status = skcore::pre_after_map(t, in, ex, n <= skcore::Caps::K, s_rec);
            __syncthreads();
            status = s_status;
        }
        if (status == SK_RPRE_OK && lane < PRE_REC_VEC) reinterpret_cast<uint4*>(a.tmp + slot)[lane] = reinterpret_cast<const uint4*>(&s_rec)[lane];
        if (lane == 0) {
            a.slot_status[slot] = status;
            sm.status[src.read] = uint8_t(status);
        }
        __syncthreads(); // (the record is read before the next read clears it)
    }
}

// R3: one block
__global__ __launch_bounds__(PRE_SCAN_T) void pre_rank_kernel(const PreArgs a)
{
    __shared__ int64_t s_wave[16];
    __shared__ int64_t s_total;
    __shared__ unsigned s_count[SK_RPRE_N_STATUS];
    if (a.ctl[PC_BAD]) return;
    if (threadIdx.x < SK_RPRE_N_STATUS) s_count[threadIdx.x] = 0;
    __syncthreads();
    const int64_t n_pass = a.ctl[PC_PASS];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n_pass; c0 += PRE_SCAN_T) {
        const int64_t i = c0 + threadIdx.x;
        const int status = i < n_pass ? a.slot_status[i] : int(SK_RPRE_NONE);
        const int64_t v = block_scan_1024(int64_t(status == SK_RPRE_OK ? 1 : 0), PrePlus(), s_wave);
        if (i < n_pass) {
            a.slot_dst[i] = status == SK_RPRE_OK ? int32_t(carry + v - 1) : -1;
            if (status == SK_RPRE_OK) a.source[carry + v - 1] = a.slot_src[i];
            else atomicAdd(&s_count[status], 1u); // (the reads that are declined are few)
        }
        if (threadIdx.x == PRE_SCAN_T - 1) s_total = v;
        __syncthreads();
        carry += s_total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int64_t n_reads = 0;
        for (int s = 0; s < a.n_samples; ++s) n_reads += a.s[s].n_reads;
        a.totals[0] = carry;
        for (int i = 0; i < SK_RPRE_N_STATUS; ++i) a.totals[1 + i] = s_count[i];
        a.totals[1 + SK_RPRE_OK] = carry;
        a.totals[1 + SK_RPRE_NOT_PASSED] = n_reads - n_pass;
    }
}

// R4
__global__ __launch_bounds__(PRE_T) void pre_copy_kernel(const PreArgs a)
{
    if (a.ctl[PC_BAD]) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_pass = a.ctl[PC_PASS], stride = int64_t(gridDim.x) * (PRE_T / 64);
    for (int64_t slot = int64_t(blockIdx.x) * (PRE_T / 64) + (threadIdx.x >> 6); slot < n_pass; slot += stride) {
        const int32_t dst = a.slot_dst[slot];
        if (dst >= 0 && lane < PRE_REC_VEC) reinterpret_cast<uint4*>(a.records + dst)[lane] = reinterpret_cast<const uint4*>(a.tmp + slot)[lane];
    }
}

// the same five steps on the host, over host arrays: the test hook
void pre_run_host(const PreArgs& a)
{
    const int64_t n_keys = a.table_totals[0];
    for (int64_t k = 0; k < n_keys; ++k) a.tab[k] = pre_tab_entry(a.keys[k]);
    a.ctl[PC_BAD] = 0;
    a.ctl[PC_KEYS] = n_keys;
    a.ctl[PC_HAS_MM] = 0;
    for (int64_t k = 0; k < n_keys; ++k)
        if (a.keys[k].type == SK_INDEL_MISMATCH) a.ctl[PC_HAS_MM] = 1;
    const skcore::PreTable t = pre_table_of(a);
    int64_t n_rec = 0;
    for (int s = 0; s < a.n_samples; ++s) {
        const PreSample& sm = a.s[s];
        for (int32_t r = 0; r < sm.n_reads; ++r) {
            int status = SK_RPRE_NOT_PASSED;
            if (sm.gate[r].status == SK_RGATE_PASS) {
                PRead rec;
                std::memset(&rec, 0, sizeof(rec));
                status = skcore::preamble_read(t, pre_read_of(sm, s, r), rec);
                if (status == SK_RPRE_OK) {
                    a.records[n_rec] = rec;
                    a.source[n_rec++] = sk_realign_prepared_source{ s, r };
                }
            }
            sm.status[r] = uint8_t(status);
            a.totals[1 + status]++;
        }
    }
    a.totals[0] = n_rec;
}

struct PreLayout
{
    size_t ctl, tab, slot_src, slot_status, slot_dst, tmp, total;
};
PreLayout pre_layout(const int64_t key_cap, const int64_t record_cap)
{
    PreLayout l;
    l.ctl = 0;
    l.tab = 256;
    l.slot_src = l.tab + sk_align256(sizeof(skcore::PIndel) * size_t(key_cap));
    l.slot_status = l.slot_src + sk_align256(sizeof(sk_realign_prepared_source) * size_t(record_cap));
    l.slot_dst = l.slot_status + sk_align256(sizeof(int32_t) * size_t(record_cap));
    l.tmp = l.slot_dst + sk_align256(sizeof(int32_t) * size_t(record_cap));
    l.total = l.tmp + sk_align256(sizeof(PRead) * size_t(record_cap)) + 256; // (+ 256: the block is aligned here)
    return l;
}

enum : int64_t { PRE_MAX_KEYS = int64_t(1) << 26, PRE_MAX_RECORDS = int64_t(1) << 24 };

// what every entry refuses of the sizes and pointers the host can read
const char* pre_args_issue(const int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* gate, const sk_realign_preamble_sample* pre,
                           const int64_t n_keys, const int64_t ins_len, const int32_t ref_len, const uint32_t max_indel_size, const int64_t record_cap, const void* keys,
                           const void* ins_pool, const void* ref, const void* records, const void* source, const void* consulted, const void* totals)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return "n_samples must be in 1..SK_MAX_SAMPLES";
    if (n_keys < 0 || ins_len < 0 || ref_len < 0 || record_cap < 0) return "negative size";
    if (n_keys > PRE_MAX_KEYS || record_cap > PRE_MAX_RECORDS || ins_len > int64_t(UINT32_MAX)) return "more keys than 2^26, more records than 2^24 or an insert pool above 2^32 - 1 bytes";
    if (max_indel_size > uint32_t(INT32_MAX)) return "max_indel_size above INT32_MAX";
    if (!samples || !gate || !pre || !totals || (n_keys > 0 && (!keys || !consulted)) || (ins_len > 0 && !ins_pool) || (ref_len > 0 && !ref) ||
        (record_cap > 0 && (!records || !source)))
        return "null argument";
    for (int s = 0; s < n_samples; ++s) {
        const sk_realign_gate_sample& sm = samples[s];
        if (sm.n_reads < 0 || sm.path_cap < 0 || gate[s].observed_cap < 0 || pre[s].code_cap < 0) return "negative size";
        if ((sm.n_reads > 0 && (!sm.pos || !sm.path_off || !sm.n_seg || !sm.read_len || !sm.realign_begin || !sm.realign_end || !gate[s].reads || !pre[s].status)) ||
            (sm.path_cap > 0 && !sm.path) || !gate[s].observed_off || (gate[s].observed_cap > 0 && !gate[s].observed) || !pre[s].read_off ||
            (pre[s].code_cap > 0 && !pre[s].read_code))
            return "null argument";
    }
    return nullptr;
}

void pre_fill_samples(PreArgs& a, const int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* gate, const sk_realign_preamble_sample* pre)
{
    a.n_samples = n_samples;
    for (int s = 0; s < n_samples; ++s) {
        const sk_realign_gate_sample& sm = samples[s];
        a.s[s] = PreSample{ sm.n_reads, sm.pos, sm.path_off, sm.n_seg, sm.path, sm.path_cap, sm.read_len, sm.realign_begin, sm.realign_end, gate[s].reads,
                            gate[s].observed_off, gate[s].observed, gate[s].observed_cap, pre[s].read_code, pre[s].read_off, pre[s].code_cap, pre[s].is_fwd_strand,
                            pre[s].status };
    }
}

// what the host entry and the hook refuse of the arrays' contents: "" = nothing
std::string pre_content_issue(const PreArgs& a, const int64_t n_keys)
{
    for (int64_t k = 0; k < n_keys; ++k)
        if (pre_key_bad(a, k)) return "key " + std::to_string(k) + ": a type outside SK_INDEL_INDEL..SK_INDEL_BP_RIGHT, an insert outside the pool, or a position before the previous key's";
    int64_t n_pass = 0;
    for (int s = 0; s < a.n_samples; ++s)
        for (int32_t r = 0; r < a.s[s].n_reads; ++r) {
            const PreSample& sm = a.s[s];
            const std::string where = "sample " + std::to_string(s) + ": read " + std::to_string(r) + ": ";
            if (sm.n_seg[r] < 0) return where + "a negative n_seg";
            if (sm.read_len[r] < 0) return where + "a negative read_len";
            if (sm.path_off[r] < 0 || sm.path_off[r] > sm.path_cap || int64_t(sm.n_seg[r]) > sm.path_cap - sm.path_off[r]) return where + "the path lies outside path_cap";
            if (sm.gate[r].status > uint8_t(SK_RGATE_SPLICED)) return where + "a gate status above SK_RGATE_SPLICED";
            if (sm.read_off[r] < 0 || sm.read_off[r + 1] < sm.read_off[r] || sm.read_off[r + 1] > sm.code_cap) return where + "read_off descends or leaves code_cap";
            if (sm.observed_off[r] < 0 || sm.observed_off[r + 1] < sm.observed_off[r] || sm.observed_off[r + 1] > sm.observed_cap) return where + "observed_off descends or leaves observed_cap";
            if (pre_read_bad(sm, r, n_keys)) return where + "a segment type above SK_SEG_SEQ_MISMATCH, or an observed list that is not strictly ascending or holds an index outside the table";
            n_pass += sm.gate[r].status == SK_RGATE_PASS;
        }
    if (n_pass > a.record_cap) return "record_cap is below the " + std::to_string(n_pass) + " reads that pass the gate";
    return "";
}

} // namespace

extern "C" {

size_t sk_realign_preamble_scratch_bytes(int32_t n_samples, int64_t key_cap, int64_t record_cap)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES || key_cap < 0 || record_cap < 0 || key_cap > PRE_MAX_KEYS || record_cap > PRE_MAX_RECORDS) return 0;
    return pre_layout(key_cap, record_cap).total;
}

int sk_realign_preamble_dev(int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* gate, const sk_realign_preamble_sample* pre,
                            const sk_realign_gate_key* dev_keys, const int64_t* dev_table_totals, int64_t key_cap, const uint8_t* dev_insert_pool, int64_t insert_cap,
                            const char* dev_ref, int32_t ref_offset, int32_t ref_len, uint32_t max_indel_size, sk_realign_prepared_read* dev_records,
                            sk_realign_prepared_source* dev_source, int64_t record_cap, uint8_t* dev_preamble_consulted, int64_t* dev_totals, void* dev_scratch,
                            size_t scratch_bytes, void* hip_stream)
{
    if (const char* issue = pre_args_issue(n_samples, samples, gate, pre, key_cap, insert_cap, ref_len, max_indel_size, record_cap, dev_keys, dev_insert_pool, dev_ref, dev_records,
                                           dev_source, dev_preamble_consulted, dev_totals))
        return sk_fail(std::string("sk_realign_preamble_dev: ") + issue);
    if (!dev_table_totals) return sk_fail("sk_realign_preamble_dev: null argument");
    if (reinterpret_cast<uintptr_t>(dev_records) & 15) return sk_fail("sk_realign_preamble_dev: dev_records is not aligned to 16 bytes");
    if (!dev_scratch || scratch_bytes < sk_realign_preamble_scratch_bytes(n_samples, key_cap, record_cap))
        return sk_fail("sk_realign_preamble_dev: scratch is below sk_realign_preamble_scratch_bytes");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const PreLayout lay = pre_layout(key_cap, record_cap);
    char* scratch = static_cast<char*>(dev_scratch);
    scratch += (256 - (reinterpret_cast<uintptr_t>(scratch) & 255)) & 255;
    PreArgs a;
    std::memset(&a, 0, sizeof(a));
    pre_fill_samples(a, n_samples, samples, gate, pre);
    a.max_indel_size = int32_t(max_indel_size);
    a.keys = dev_keys;
    a.table_totals = dev_table_totals;
    a.key_cap = key_cap;
    a.ins_pool = dev_insert_pool;
    a.ins_cap = insert_cap;
    a.ref = dev_ref;
    a.ref_offset = ref_offset;
    a.ref_len = ref_len;
    a.records = reinterpret_cast<PRead*>(dev_records);
    a.source = dev_source;
    a.record_cap = record_cap;
    a.consulted = dev_preamble_consulted;
    a.totals = dev_totals;
    a.ctl = reinterpret_cast<int64_t*>(scratch + lay.ctl);
    a.tab = reinterpret_cast<skcore::PIndel*>(scratch + lay.tab);
    a.slot_src = reinterpret_cast<sk_realign_prepared_source*>(scratch + lay.slot_src);
    a.slot_status = reinterpret_cast<int32_t*>(scratch + lay.slot_status);
    a.slot_dst = reinterpret_cast<int32_t*>(scratch + lay.slot_dst);
    a.tmp = reinterpret_cast<PRead*>(scratch + lay.tmp);
    a.err = sk_ctx().dev_error_flags;
    int64_t zero_max = std::max(record_cap * PRE_REC_VEC, key_cap);
    for (int s = 0; s < n_samples; ++s) zero_max = std::max(zero_max, int64_t(samples[s].n_reads));
    const auto grid_of = [](const int64_t n, const int64_t per_block, const int64_t most) {
        const int64_t blocks = (n + per_block - 1) / per_block;
        return unsigned(blocks < 1 ? 1 : (blocks < most ? blocks : most));
    };
    // five launches, whatever the arrays hold
    SK_LAUNCH(pre_check_kernel, dim3(grid_of(zero_max, PRE_T, PRE_GRID)), dim3(PRE_T), 0, st, a);
    SK_LAUNCH(pre_slot_kernel, dim3(1), dim3(PRE_SCAN_T), 0, st, a);
    SK_LAUNCH(pre_read_kernel, dim3(grid_of(record_cap, 1, 8 * PRE_GRID)), dim3(64), 0, st, a);
    SK_LAUNCH(pre_rank_kernel, dim3(1), dim3(PRE_SCAN_T), 0, st, a);
    SK_LAUNCH(pre_copy_kernel, dim3(grid_of(record_cap, PRE_T / 64, PRE_GRID)), dim3(PRE_T), 0, st, a);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_debug_realign_preamble_host(int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* gate, const sk_realign_preamble_sample* pre,
                                   const sk_realign_gate_key* keys, int64_t n_keys, const uint8_t* insert_pool, int64_t insert_len, const char* ref, int32_t ref_offset,
                                   int32_t ref_len, uint32_t max_indel_size, sk_realign_prepared_read* records, sk_realign_prepared_source* source, int64_t record_cap,
                                   uint8_t* preamble_consulted, int64_t* totals)
{
    if (const char* issue = pre_args_issue(n_samples, samples, gate, pre, n_keys, insert_len, ref_len, max_indel_size, record_cap, keys, insert_pool, ref, records, source,
                                           preamble_consulted, totals))
        return sk_fail(std::string("sk_debug_realign_preamble_host: ") + issue);
    const int64_t table_totals[4] = { n_keys, 0, 0, 0 };
    int64_t ctl[PC_WORDS] = {};
    std::vector<skcore::PIndel> tab(size_t(n_keys) + 1);
    PreArgs a;
    std::memset(&a, 0, sizeof(a));
    pre_fill_samples(a, n_samples, samples, gate, pre);
    a.max_indel_size = int32_t(max_indel_size);
    a.keys = keys;
    a.table_totals = table_totals;
    a.key_cap = n_keys;
    a.ins_pool = insert_pool;
    a.ins_cap = insert_len;
    a.ref = ref;
    a.ref_offset = ref_offset;
    a.ref_len = ref_len;
    a.records = reinterpret_cast<PRead*>(records);
    a.source = source;
    a.record_cap = record_cap;
    a.consulted = preamble_consulted;
    a.totals = totals;
    a.ctl = ctl;
    a.tab = tab.data();
    const std::string issue = pre_content_issue(a, n_keys);
    if (!issue.empty()) return sk_fail("sk_debug_realign_preamble_host: " + issue);
    if (record_cap > 0) std::memset(records, 0, sizeof(PRead) * size_t(record_cap));
    for (int64_t i = 0; i < record_cap; ++i) source[i] = sk_realign_prepared_source{ 0, 0 };
    for (int64_t k = 0; k < n_keys; ++k) preamble_consulted[k] = 0;
    for (int i = 0; i < SK_RPRE_N_TOTALS; ++i) totals[i] = 0;
    pre_run_host(a);
    return 0;
}

int sk_realign_preamble(int32_t n_samples, const sk_realign_gate_sample* samples, const sk_realign_gate_sample_out* gate, const sk_realign_preamble_sample* pre,
                        const sk_realign_gate_key* keys, int64_t n_keys, const uint8_t* insert_pool, int64_t insert_len, const char* ref, int32_t ref_offset,
                        int32_t ref_len, uint32_t max_indel_size, sk_realign_prepared_read* records, sk_realign_prepared_source* source, int64_t record_cap,
                        uint8_t* preamble_consulted, int64_t* totals)
{
    if (const char* issue = pre_args_issue(n_samples, samples, gate, pre, n_keys, insert_len, ref_len, max_indel_size, record_cap, keys, insert_pool, ref, records, source,
                                           preamble_consulted, totals))
        return sk_fail(std::string("sk_realign_preamble: ") + issue);
    {
        PreArgs h;
        std::memset(&h, 0, sizeof(h));
        pre_fill_samples(h, n_samples, samples, gate, pre);
        h.keys = keys;
        h.ins_cap = insert_len;
        h.record_cap = record_cap;
        const std::string issue = pre_content_issue(h, n_keys);
        if (!issue.empty()) return sk_fail("sk_realign_preamble: " + issue);
    }
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t nk = size_t(n_keys), nrec = size_t(record_cap);
    const size_t scratch_bytes = sk_realign_preamble_scratch_bytes(n_samples, n_keys, record_cap);
    const int64_t table_totals[4] = { n_keys, 0, 0, 0 };
    struct
    {
        sk_realign_gate_sample in[SK_MAX_SAMPLES];
        sk_realign_gate_sample_out gate[SK_MAX_SAMPLES];
        sk_realign_preamble_sample pre[SK_MAX_SAMPLES];
        sk_realign_gate_key* keys; int64_t* table_totals; uint8_t* ins_pool; char* ref; sk_realign_prepared_read* records; sk_realign_prepared_source* source;
        uint8_t* consulted; int64_t* totals; char* scratch;
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
                t.align_id = nullptr;
                t.realign_begin = ar.up(sm.realign_begin, nr, 1, st, rc);
                t.realign_end = ar.up(sm.realign_end, nr, 1, st, rc);
                o.in[s] = t;
                o.gate[s].reads = ar.up(gate[s].reads, nr, 1, st, rc);
                o.gate[s].observed_off = ar.up(gate[s].observed_off, nr + 1, 0, st, rc);
                o.gate[s].observed = ar.up(gate[s].observed, size_t(gate[s].observed_cap), 1, st, rc);
                o.gate[s].observed_cap = gate[s].observed_cap;
                o.pre[s].read_code = ar.up(pre[s].read_code, size_t(pre[s].code_cap), 1, st, rc);
                o.pre[s].read_off = ar.up(pre[s].read_off, nr + 1, 0, st, rc);
                o.pre[s].code_cap = pre[s].code_cap;
                o.pre[s].is_fwd_strand = pre[s].is_fwd_strand ? ar.up(pre[s].is_fwd_strand, nr, 1, st, rc) : nullptr;
                o.pre[s].status = ar.take<uint8_t>(nr + 1);
            }
            o.keys = ar.up(keys, nk, 1, st, rc);
            o.table_totals = ar.up(table_totals, 4, 0, st, rc);
            o.ins_pool = ar.up(insert_pool, size_t(insert_len), 1, st, rc);
            o.ref = ar.up(ref, size_t(ref_len), 1, st, rc);
            o.records = ar.take<sk_realign_prepared_read>(nrec + 1);
            o.source = ar.take<sk_realign_prepared_source>(nrec + 1);
            o.consulted = ar.take<uint8_t>(nk + 1);
            o.totals = ar.take<int64_t>(SK_RPRE_N_TOTALS);
            o.scratch = ar.take<char>(scratch_bytes + 16);
            return o;
        }) || rc)
        return 1;
    if (sk_realign_preamble_dev(n_samples, d.in, d.gate, d.pre, d.keys, d.table_totals, n_keys, d.ins_pool, insert_len, d.ref, ref_offset, ref_len, max_indel_size, d.records,
                                d.source, record_cap, d.consulted, d.totals, d.scratch, scratch_bytes + 16, st))
        return 1;
    int64_t t[SK_RPRE_N_TOTALS];
    SK_HIP(skrt::memcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1;
    if (t[0] < 0 || t[0] > record_cap) return sk_fail("sk_realign_preamble: the device left a record count outside record_cap");
    if (nrec > 0) { // (the whole room: what lies past the count is zero, and says so)
        SK_HIP(skrt::memcpyAsync(records, d.records, sizeof(sk_realign_prepared_read) * nrec, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(source, d.source, sizeof(sk_realign_prepared_source) * nrec, hipMemcpyDeviceToHost, st));
    }
    if (nk > 0) SK_HIP(skrt::memcpyAsync(preamble_consulted, d.consulted, nk, hipMemcpyDeviceToHost, st));
    for (int s = 0; s < n_samples; ++s)
        if (samples[s].n_reads > 0) SK_HIP(skrt::memcpyAsync(pre[s].status, d.pre[s].status, size_t(samples[s].n_reads), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    for (int i = 0; i < SK_RPRE_N_TOTALS; ++i) totals[i] = t[i];
    return 0;
}

} // extern "C"
