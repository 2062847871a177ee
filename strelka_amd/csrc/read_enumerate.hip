// read_enumerate.hip -- candidate-alignment enumeration, flattening and scoring of a realignment job on the device
// (sk_realign_options.enumeration == 2).
//
//   E1  root_kernel, level_kernel x depth   candidate_alignment_search (csrc/realign_core.h, the statement of
//                          L/starling_common/starling_read_align.cpp:857-1277 shared with the host), level by level: one thread
//                          per call of the reference's recursion, all reads of the job at once
//   E2  group/dedupe/rank  the leaves of each read -> its std::set<CandidateAlignment>: duplicates dropped, set order
//   L1  pool_bounds/layout  reference window and insert sequences of each read's haplotype pool
//   L2  op_count_kernel    one thread per candidate alignment: ops it flattens to
//   F1  pool_fill_kernel   one wave per read: the pool's bytes
//   F2  flatten_kernel     one thread per candidate alignment: the walk of scoreCandidateAlignment
//                          (starling_read_align_score.cpp:286-493) emitting scoring ops (host/align_flatten.cpp holds the host form)
//   F3  entries_kernel     one thread per candidate alignment: the transition entries and event masks kernel A1 reads
//                          (csrc/align_entry.h) -- so neither sk_align_builder nor sk_align_prepare runs on the host for these reads
//   A1  score_wave_per_read (score_alignments.hip) on the batch E3 left in HBM
//
// All of this is integer/byte work; it has to reproduce the host stages exactly (tests/test_device_enumeration.py).  A read that
// exceeds a capacity of the core, or that the host code would have thrown on, is reported (status != ST_OK) and redone by the
// container-based host code, which then produces either the result or the reference's error text -- nothing is truncated.

#include "sk_common.h"

#include "align_entry.h"
#include "read_enumerate.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace skcore;

int sk_score_alignments_launch_hostleg(const sk_align_batch* b, double* dev_out_lnp, void* hip_stream); // score_alignments.hip

namespace
{

static_assert(sizeof(PFrame) % 4 == 0 && sizeof(PCal) % 4 == 0, "frames move through LDS as 32-bit words");

// ---------------------------------------------------------------------------------------------------------------------
// E1: the search, level by level.  The reference's recursion passes its whole state by value, so the calls at one depth are
// independent of each other (they share the set the leaves go into and two warning flags): level d of ALL reads of the job is
// one launch, one thread per call, the frames of the level in one array and the children appended to the next level's array.
// A thread's frame is staged into LDS first (the 64 frames of a workgroup are contiguous in HBM): expanding a call is a long
// chain of dependent accesses to its frame, and LDS is an order of magnitude closer than HBM.

struct EnumArgs
{
    PJob job; // device pointers
    const PRead* reads;
    int32_t n_reads;
    PFrame* level_in;
    PFrame* level_out;
    int32_t frame_cap;
    int32_t* level_count; // [Caps::K + 3]
    int32_t depth;
    PCal* pool; // leaves, as found (duplicates included)
    int32_t* leaf_read;
    uint32_t* leaf_hash;
    int32_t pool_cap;
    int32_t* n_leaves;
    int32_t* n_raw;  // [n_reads] leaves found
    int32_t* status; // [n_reads] max over the read's calls
    int32_t* warn;   // [n_reads] bit 0 origin, bit 1 toggle depth
    unsigned long long* n_nodes;
    // null, or per read cells that start at INT_MAX (win_begin, ins_lo) / INT_MIN (win_end, ins_hi): the root launch sets them when the
    // job runs as one fixed sequence (no fills of their own)
    int32_t* min_cells_a;
    int32_t* min_cells_b;
    int32_t* max_cells_a;
    int32_t* max_cells_b;
};

__device__ inline uint32_t cal_hash(const PCal& c)
{
    uint32_t h = 2166136261u;
    auto mix = [&](const uint32_t v) { h = (h ^ v) * 16777619u; };
    mix(uint32_t(c.pos));
    mix(uint32_t(c.fwd) | (uint32_t(c.n_seg) << 8) | (uint32_t(c.n_indels) << 16));
    mix(uint32_t(uint16_t(c.lead)) | (uint32_t(uint16_t(c.trail)) << 16));
    for (int i = 0; i < c.n_seg; ++i) mix(uint32_t(c.path[i].type) | (uint32_t(c.path[i].length) << 16));
    for (int i = 0; i < c.n_indels; ++i) mix(uint32_t(uint16_t(c.indels[i])));
    return h;
}

struct LeafSink // a leaf: the read's clips back on (clip_adder :508-542), dropped when outside the realign range (:1981-1993)
{
    const EnumArgs* a;
    const PRead* r;
    int32_t read_id;
    __device__ bool operator()(PCal& leaf)
    {
        if (r->clipped && !clip_adder(leaf, r->hc_lead, r->hc_trail, r->sc_lead, r->sc_trail)) return false;
        if (!superset_of(mk_range(r->realign_b, r->realign_e), strict_range(leaf))) return true;
        const int slot = atomicAdd(a->n_leaves, 1);
        if (slot >= a->pool_cap) return false;
        copy_cal(a->pool[slot], leaf);
        a->leaf_read[slot] = read_id;
        a->leaf_hash[slot] = cal_hash(leaf);
        atomicAdd(&a->n_raw[read_id], 1);
        return true;
    }
};

struct LevelAlloc
{
    const EnumArgs* a;
    __device__ PFrame* operator()()
    {
        const int slot = atomicAdd(&a->level_count[a->depth + 1], 1);
        if (slot >= a->frame_cap) return nullptr;
        return &a->level_out[slot];
    }
};

__global__ __launch_bounds__(64) void root_kernel(const EnumArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    if (r == 0) a.level_count[0] = a.n_reads;
    if (a.min_cells_a) {
        a.min_cells_a[r] = a.min_cells_b[r] = INT_MAX;
        a.max_cells_a[r] = a.max_cells_b[r] = INT_MIN;
    }
    PFrame& f = a.level_out[r];
    root_frame(a.job, a.reads[r], f);
    f.read_id = r;
}

enum { FRAME_WORDS = sizeof(PFrame) / 4 };

__global__ __launch_bounds__(64) void level_kernel(const EnumArgs a)
{
    extern __shared__ __align__(16) uint32_t lds_words[];
    PFrame* frames = reinterpret_cast<PFrame*>(lds_words);
    const int n_in = min(a.level_count[a.depth], a.frame_cap);
    for (int base = blockIdx.x * 64; base < n_in; base += gridDim.x * 64) {
        const int n_here = min(64, n_in - base);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.level_in + base);
        for (int w = threadIdx.x; w < n_here * FRAME_WORDS; w += 64) lds_words[w] = src[w];
        __syncthreads();
        if (int(threadIdx.x) < n_here) {
            PFrame& f = frames[threadIdx.x];
            const int r = f.read_id;
            if (f.stage != 0xffff && a.status[r] == ST_OK) {
                SearchOut so;
                so.status = ST_OK;
                so.warn_origin = so.warn_toggle = 0;
                so.nodes = 0;
                LeafSink sink{ &a, &a.reads[r], r };
                LevelAlloc alloc{ &a };
                expand_node(a.job, a.reads[r], f, alloc, &f.cal, sink, so); // (a leaf is completed in place: the frame is done with)
                if (so.status != ST_OK) atomicMax(&a.status[r], so.status);
                if (so.warn_origin | so.warn_toggle) atomicOr(&a.warn[r], (so.warn_origin ? 1 : 0) | (so.warn_toggle ? 2 : 0));
            }
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.n_nodes) atomicAdd(a.n_nodes, (unsigned long long)n_in);
}

// ---------------------------------------------------------------------------------------------------------------------
// E2: the leaves of each read -> a std::set<CandidateAlignment>: grouped by read, duplicates dropped, ordered

struct SetArgs
{
    const PCal* pool;
    const int32_t* leaf_read;
    const uint32_t* leaf_hash;
    const int32_t* status;
    int32_t n_reads, n_leaves;
    const int32_t* raw_off; // [n_reads+1] (reads that failed: empty)
    int32_t* fill;          // [n_reads] zeroed
    int32_t* grouped;       // [raw_off[n_reads]] leaf slots, read by read
    uint32_t* ghash;        // [raw_off[n_reads]] their hashes
    ulonglong2* gkey;       // [raw_off[n_reads]] their keys (leaf_key)
    uint8_t* dup;           // [raw_off[n_reads]]
    int32_t* n_uniq;        // [n_reads] zeroed
    const int32_t* cal_off; // [n_reads+1]
    int32_t* sorted;        // [cal_off[n_reads]] leaf slots in set order
    const int32_t* n_leaves_dev; // null, or where the search counted its leaves: the job runs as one fixed sequence, the host has not
                                 // seen the count (n_leaves is then the pool's capacity)
};

__device__ inline int group_of(const int32_t* off, const int n, const int g) // last r with off[r] <= g
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// The first fields cal_compare looks at (position, strand, number of segments, the first four segments), packed so that comparing
// the two words as numbers is comparing those fields in cal_compare's order: most pairs of leaves are told apart by the key alone,
// read from one contiguous array instead of from two 300-byte records
__device__ inline ulonglong2 leaf_key(const PCal& c)
{
    auto seg = [&](const int i) -> unsigned long long { // 20 bits: type, length
        return i < c.n_seg ? ((unsigned long long)(c.path[i].type & 0xfu) << 16) | c.path[i].length : 0ull;
    };
    ulonglong2 k;
    k.x = ((unsigned long long)(uint32_t(c.pos) ^ 0x80000000u) << 32) | ((unsigned long long)(c.fwd ? 1 : 0) << 31) |
          ((unsigned long long)(c.n_seg & 0x7fu) << 24) | (seg(0) << 4) | (seg(1) >> 16);
    k.y = ((seg(1) & 0xffffull) << 48) | (seg(2) << 28) | (seg(3) << 8);
    return k;
}
__global__ __launch_bounds__(256) void group_kernel(const SetArgs a)
{
    const int n_leaves = a.n_leaves_dev ? min(*a.n_leaves_dev, a.n_leaves) : a.n_leaves;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n_leaves; s += gridDim.x * blockDim.x) {
        const int r = a.leaf_read[s];
        if (a.status[r] != ST_OK) continue;
        const int g = a.raw_off[r] + atomicAdd(&a.fill[r], 1);
        a.grouped[g] = s;
        a.ghash[g] = a.leaf_hash[s];
        a.gkey[g] = leaf_key(a.pool[s]);
    }
}

// a leaf is a duplicate when an equal leaf stands before it in its read's group (which of the equal ones stands first differs
// from run to run; they are equal).  The scan over the group is a plain comparison of hashes with nothing in the loop that waits
// for a load (reads with thousands of leaves make it long); the records are compared only where a hash is met again.
__global__ __launch_bounds__(256) void dedupe_kernel(const SetArgs a)
{
    const int n_grouped = a.raw_off[a.n_reads];
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n_grouped; g += gridDim.x * blockDim.x) {
    const int r = group_of(a.raw_off, a.n_reads, g);
    const uint32_t h = a.ghash[g];
    const int q0 = a.raw_off[r];
    bool dup = false;
    for (int from = q0; from < g && !dup;) {
        int first = g; // the first leaf at or after `from` with this hash
        int q = from;
        for (; q + 8 <= g; q += 8) {
            uint32_t v[8];
            for (int z = 0; z < 8; ++z) v[z] = a.ghash[q + z];
            for (int z = 7; z >= 0; --z) first = (v[z] == h && q + z < first) ? q + z : first;
            if (first < g) break;
        }
        if (first == g)
            for (; q < g; ++q)
                if (a.ghash[q] == h) {
                    first = q;
                    break;
                }
        if (first >= g) break;
        if (cal_compare(a.pool[a.grouped[first]], a.pool[a.grouped[g]]) == 0) dup = true;
        from = first + 1;
    }
    a.dup[g] = dup ? 1 : 0;
    if (!dup) atomicAdd(&a.n_uniq[r], 1);
    }
}

// the rank of a kept leaf in the set order of its read (CandidateAlignment.hh:37-48, alignment.hh:72-90: cal_compare): the keys
// decide for almost every pair, without a branch; pairs with equal keys (their number is counted on the way) get the full comparison
__global__ __launch_bounds__(256) void rank_kernel(const SetArgs a)
{
    const int n_grouped = a.raw_off[a.n_reads];
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n_grouped; g += gridDim.x * blockDim.x) {
    if (a.dup[g]) continue;
    const int r = group_of(a.raw_off, a.n_reads, g);
    const ulonglong2 kmine = a.gkey[g];
    const int q0 = a.raw_off[r], q1 = a.raw_off[r + 1];
    int rank = 0, n_equal = 0;
    auto count = [&](const ulonglong2 k, const uint8_t dup) {
        const bool kept = dup == 0;
        const bool lower = (k.x < kmine.x) || (k.x == kmine.x && k.y < kmine.y);
        const bool equal = (k.x == kmine.x) && (k.y == kmine.y);
        rank += (kept && lower) ? 1 : 0;
        n_equal += (kept && equal) ? 1 : 0;
    };
    int q = q0;
    for (; q + 8 <= q1; q += 8) { // (eight keys in flight: one at a time the loop is a chain of load latencies, 120 us per 4 096 reads x 88)
        ulonglong2 k[8];
        uint8_t d[8];
#pragma unroll
        for (int z = 0; z < 8; ++z) {
            k[z] = a.gkey[q + z];
            d[z] = a.dup[q + z];
        }
#pragma unroll
        for (int z = 0; z < 8; ++z) count(k[z], d[z]);
    }
    for (; q < q1; ++q) count(a.gkey[q], a.dup[q]);
    if (n_equal > 1) { // (itself and others)
        const PCal& mine = a.pool[a.grouped[g]];
        for (int q = q0; q < q1; ++q) {
            if (q == g || a.dup[q]) continue;
            const ulonglong2 k = a.gkey[q];
            if (k.x == kmine.x && k.y == kmine.y && cal_compare(a.pool[a.grouped[q]], mine) < 0) ++rank;
        }
    }
    a.sorted[a.cal_off[r] + rank] = a.grouped[g];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The job as ONE fixed sequence of launches (no host decision between the upload and the results): the two prefix sums the host used to
// make between waits -- leaves per read -> raw_off, unique alignments per read -> cal_off -- are made here, by one workgroup (a job has at
// most a few ten thousand reads: a thread a run of consecutive reads, one block-wide scan of the runs' sums), together with what else
// the host derived from them: the totals, stage 3's two read lists, and the conditions under which the sequence's assumptions do not
// hold (then the host runs the job again the staged way: sk_enum_device_run).

enum { DYN_N_GROUPED = 0, DYN_N_CALS, DYN_N_LIGHT, DYN_N_HEAVY, DYN_FLAGS, DYN_MAX_CALS, DYN_REF_OUTSIDE, DYN_COUNT = 8 };
enum { DYNF_DEEPER = 1,    // calls were left at the first level the sequence did not launch
       DYNF_POOL_FULL = 2 }; // more leaves than the sequence's pool holds
// the job's counters: 32-bit slots at the head of the zero arena (EnumBuffers::counters), all zero when a job starts
enum { SEARCH_LEVELS = Caps::K + 2,       // level launches after which no search has a call left
       CNT_LEVELS = 0,                    // [SEARCH_LEVELS + 1] calls made at each depth (EnumArgs::level_count)
       CNT_LEAVES = Caps::K + 3,          // leaves found
       CNT_NODES = (Caps::K + 5) & ~1,    // calls made: 64 bit, so at the first even slot past the leaves (two slots)
       CNT_UNHANDLED = Caps::K + 7,       // reads F5 turned down
       CNT_DYN = Caps::K + 8,             // [DYN_COUNT] the scans' results
       CNT_QUEUE = CNT_DYN + DYN_COUNT,   // [2] F5's read queue (FusedScoreArgs::queue)
       CNT_SHARED = CNT_QUEUE + 2,        // F5's rounds scored by a wave other than their read's owner (FusedScoreArgs::shared_rounds)
       N_COUNTERS = CNT_SHARED + 2 };     // ([CNT_SHARED + 1]: rounds after a read's first that turned the read down)
static_assert(CNT_LEVELS + SEARCH_LEVELS + 1 == CNT_LEAVES && CNT_NODES > CNT_LEAVES && CNT_NODES + 2 <= CNT_UNHANDLED, "the counters' slots overlap");

template <typename V> // (int; unsigned long long: two 32-bit counts scanned as one value, tail_order_kernel)
__device__ inline V block_exclusive_scan(const V v, V* wave_sums /* LDS [blockDim.x / 64 + 1] */, V* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    V x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const V y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads(); // (wave_sums may still be read from a previous scan)
    if (lane == 63) wave_sums[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        V run = 0;
        for (int w = 0; w < n_waves; ++w) {
            const V t = wave_sums[w];
            wave_sums[w] = run;
            run += t;
        }
        wave_sums[n_waves] = run;
    }
    __syncthreads();
    *total = wave_sums[n_waves];
    return wave_sums[wave] + x - v;
}

struct ScanArgs
{
    int32_t n_reads;
    const int32_t* status;
    const int32_t* count;   // [n_reads] n_raw (scan 1) / n_uniq (scan 2)
    int32_t* off;           // [n_reads + 1] raw_off / cal_off
    int32_t* dyn;           // [DYN_COUNT]
    // scan 1
    const int32_t* level_count;
    int32_t first_level_not_launched; // (or -1: every level went out)
    const int32_t* n_leaves;
    int32_t pool_cap;
    // scan 2
    int32_t* list;          // [n_reads] stage 3: reads with at most light_cals alignments from the front, the others from the back
    int32_t light_cals;
};

// The job's way in and out as kernels: the packed input arena is read from the caller's page-locked mirror and the zero arena filled by
// one launch, the results (the zero arena, stage 3's records) are written to their page-locked mirrors by another.  The copy and fill
// calls they replace go through the runtime's copy engines, which eight caller processes sharing a GPU queue up for (a job's two copies
// in cost 0.16 ms of host time there against 0.015 ms alone: profiles/r05_enum_job_history.txt); a launch is a packet in the process's
// own queue.
__global__ __launch_bounds__(256) void job_stage_in_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const uint32_t n_in, uint4* __restrict__ zero,
                                                          const uint32_t n_zero)
{
    const uint32_t i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (uint32_t i = i0; i < n_in; i += step) dst[i] = src[i];
    const uint4 z = { 0, 0, 0, 0 };
    for (uint32_t i = i0; i < n_zero; i += step) zero[i] = z;
}
__global__ __launch_bounds__(256) void job_stage_out_kernel(const uint4* __restrict__ a, uint4* __restrict__ host_a, const uint32_t n_a, const uint4* __restrict__ b,
                                                           uint4* __restrict__ host_b, const uint32_t n_b)
{
    const uint32_t i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (uint32_t i = i0; i < n_a; i += step) host_a[i] = a[i];
    for (uint32_t i = i0; i < n_b; i += step) host_b[i] = b[i];
}

template <bool SECOND>
__global__ __launch_bounds__(1024) void job_scan_kernel(const ScanArgs a)
{
    __shared__ int wave_sums[17];
    const int n = a.n_reads, t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int r0 = min(n, t * per), r1 = min(n, r0 + per);
    int sum = 0, n_light = 0, n_heavy = 0, max_cals = 0;
    for (int r = r0; r < r1; ++r) {
        const int k = (a.status[r] == ST_OK) ? a.count[r] : 0;
        sum += k;
        if (SECOND) {
            if (k <= a.light_cals) ++n_light; else ++n_heavy;
            max_cals = max(max_cals, k);
        }
    }
    int total = 0;
    int at = block_exclusive_scan(sum, wave_sums, &total);
    for (int r = r0; r < r1; ++r) {
        a.off[r] = at;
        at += (a.status[r] == ST_OK) ? a.count[r] : 0;
    }
    if (t == 0) a.off[n] = total;
    if (!SECOND) {
        if (t == 0) {
            a.dyn[DYN_N_GROUPED] = total;
            int flags = 0;
            if (a.first_level_not_launched >= 0 && a.level_count[a.first_level_not_launched] != 0) flags |= DYNF_DEEPER;
            if (*a.n_leaves >= a.pool_cap) flags |= DYNF_POOL_FULL;
            a.dyn[DYN_FLAGS] = flags;
        }
    } else {
        int tot_light = 0, tot_heavy = 0;
        int lat = block_exclusive_scan(n_light, wave_sums, &tot_light);
        int hat = block_exclusive_scan(n_heavy, wave_sums, &tot_heavy);
        for (int r = r0; r < r1; ++r) {
            const int k = (a.status[r] == ST_OK) ? a.count[r] : 0;
            if (k <= a.light_cals) a.list[lat++] = r; else a.list[n - 1 - hat++] = r;
        }
        atomicMax(&a.dyn[DYN_MAX_CALS], max_cals);
        if (t == 0) {
            a.dyn[DYN_N_CALS] = total;
            a.dyn[DYN_N_LIGHT] = tot_light;
            a.dyn[DYN_N_HEAVY] = tot_heavy;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// flattening

__device__ inline uint8_t code_of(const char c) // get_bam_seq_code, L/htsapi/bam_seq.hh:73-92
{
    switch (c) {
    case '=': return SK_BAM_REF;
    case 'A': return SK_BAM_A;
    case 'C': return SK_BAM_C;
    case 'G': return SK_BAM_G;
    case 'T': return SK_BAM_T;
    default: return SK_BAM_ANY;
    }
}
// the same on the host, as a table: the job's code images (FlatArgs::ref_code, ins_code) are made with it
constexpr int F5_CODE_PAD = 1024; // bytes of SK_BAM_ANY on either side of the reference's codes
struct CodeLut
{
    uint8_t code[256];
    CodeLut()
    {
        std::memset(code, SK_BAM_ANY, sizeof(code));
        code[uint8_t('=')] = SK_BAM_REF;
        code[uint8_t('A')] = SK_BAM_A;
        code[uint8_t('C')] = SK_BAM_C;
        code[uint8_t('G')] = SK_BAM_G;
        code[uint8_t('T')] = SK_BAM_T;
    }
};
inline const CodeLut& code_lut()
{
    static const CodeLut l;
    return l;
}

struct FlatArgs
{
    PJob job;
    const char* ins_pool;
    const char* ref;
    // the job's code images (F5 reads these; the staged chain keeps reading the characters): code_of() of every reference character
    // with F5_CODE_PAD bytes of SK_BAM_ANY before and after it (ref_code points at the reference's first base: a window that leaves
    // the reference reads pad), and of every character of the insert pool
    const uint8_t* ref_code;
    const uint8_t* ins_code;
    int32_t ref_offset, ref_len;
    int32_t n_reads, n_cals;
    const PCal* pool;
    const int32_t* list; // [n_cals] leaf slots, each read's in set order
    int32_t* status;
    const int64_t* read_off;
    const uint8_t* read_code;
    const int32_t* cal_off;
    // per-read layout of the haplotype pool (L1 out)
    int32_t* win_begin; // (L1a: min over the read's candidate alignments, cells start at INT_MAX)
    int32_t* win_end;   // (cells start at INT_MIN)
    int32_t* ins_lo;    // lowest / highest table index of an indel with an insert sequence
    int32_t* ins_hi;
    uint8_t* n_seg8;    // [n_cals] path segments of each candidate alignment (capped at 255), set order: F5 orders a read's alignments by it
    int32_t* win_len;
    int32_t* hap_len;
    int32_t* n_ins;
    int16_t* ins_idx; // [n_reads][INS_CAP] table indices whose insert sequence is in the pool
    int32_t* ins_off; // [n_reads][INS_CAP] where
    // per candidate alignment
    int32_t* n_ops; // (L2 out)
    const int64_t* hap_off;
    PCal* cals;
    uint8_t* hap_code;
    const int64_t* op_off; // [n_cals + 1]
    sk_score_op* ops;
    uint32_t* entries;
    uint32_t* evmask;
    int32_t evmask_words, max_read_len;
    // the column form (strelka_amd.h, sk_align_batch::colmat)
    uint8_t* colmat; // (bytes of the words; pre-filled with the 0.0 column)
    const int64_t* colmat_off;
    uint32_t* addmask;
    int32_t* ref_outside;     // counts the window bytes that lie outside the job's reference segment (they read as N)
    int32_t n_cals_on_device; // the job runs as one fixed sequence: the number of candidate alignments is cal_off[n_reads], the host has not seen it
};
enum { INS_CAP = Caps::K + 2 };

__device__ inline int read_of_cal(const FlatArgs& a, const int c) // last r with cal_off[r] <= c
{
    int lo = 0, hi = a.n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.cal_off[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// L1: the layout of each read's haplotype pool -- its reference window (the union of the reference spans of the match segments
// of all its candidate alignments), then the insert sequences of the table indels between the lowest and the highest one any of
// its candidate alignments holds, in table order.  (The host builder appends the insert sequences its ops use in order of first
// use and shares equal sequences; the layout is private to the read's batch entry and the scores do not depend on it.)
//   L1a  one thread per candidate alignment: window and indel-index bounds into the read's cells (atomicMin / atomicMax)
//   L1b  one thread per read: offsets
__global__ __launch_bounds__(256) void pool_bounds_kernel(const FlatArgs a)
{
    const int n_cals = a.n_cals_on_device ? a.cal_off[a.n_reads] : a.n_cals;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cals; c += gridDim.x * blockDim.x) {
    const int r = read_of_cal(a, c);
    const PCal& cal = a.pool[a.list[c]];
    a.n_seg8[c] = uint8_t(min(int(cal.n_seg), 255));
    int32_t wb = INT_MAX, we = INT_MIN, pos = cal.pos;
    for (int i = 0; i < cal.n_seg; ++i) {
        const PSeg s = cal.path[i];
        if (seg_align_match(s.type)) {
            wb = min(wb, pos);
            we = max(we, pos + int32_t(s.length));
            pos += int32_t(s.length);
        } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
            pos += int32_t(s.length);
        }
    }
    if (wb <= we) {
        atomicMin(&a.win_begin[r], wb);
        atomicMax(&a.win_end[r], we);
    }
    int lo = INT_MAX, hi = INT_MIN;
    auto add = [&](const int t) {
        if (t < 0 || a.job.tab[t].ins_len == 0) return;
        lo = min(lo, t);
        hi = max(hi, t);
    };
    for (int i = 0; i < cal.n_indels; ++i) add(cal.indels[i]);
    add(cal.lead);
    add(cal.trail);
    if (lo <= hi) {
        atomicMin(&a.ins_lo[r], lo);
        atomicMax(&a.ins_hi[r], hi);
    }
    }
}

__global__ __launch_bounds__(64) void pool_layout_kernel(const FlatArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    const int nc = a.cal_off[r + 1] - a.cal_off[r];
    a.n_ins[r] = 0;
    a.win_len[r] = 0;
    a.hap_len[r] = 0;
    if (nc == 0) return;
    int32_t wb = a.win_begin[r], we = a.win_end[r];
    if (wb > we) wb = we = 0;
    a.win_begin[r] = wb;
    int32_t len = we - wb;
    a.win_len[r] = len;
    int16_t* idx = a.ins_idx + size_t(r) * INS_CAP;
    int32_t* off = a.ins_off + size_t(r) * INS_CAP;
    int n = 0;
    for (int t = a.ins_lo[r]; t <= a.ins_hi[r]; ++t) {
        const uint32_t il = a.job.tab[t].ins_len;
        if (il == 0) continue;
        if (n >= INS_CAP) { // more insert sequences than this form holds: the host flattens this read
            a.status[r] = ST_OVERFLOW;
            n = 0;
            break;
        }
        idx[n] = int16_t(t);
        off[n] = len;
        len += int32_t(il);
        ++n;
    }
    a.n_ins[r] = n;
    a.hap_len[r] = max(len, 1);
}

// getMatchingIndelKey, starling_read_align_score.cpp:177-228: table index, -1 = no key, -2 = inconsistent
__device__ int matching_indel(const PJob& j, const PCal& c, const int32_t ref_head_pos, const unsigned del_len, const unsigned ins_len,
                              const int ends_first, const int ends_second, const int path_index)
{
    if (path_index < ends_first) return c.lead;
    if (path_index > ends_second) return c.trail;
    int found = -1;
    for (int k = 0; k < c.n_indels; ++k) {
        const PIndel& ci = j.tab[c.indels[k]];
        if (ci.pos == ref_head_pos && (ci.type == SK_INDEL_INDEL || ci.type == SK_INDEL_MISMATCH) && ci.del == del_len &&
            ci.ins_len == ins_len) {
            if (found >= 0) return -2;
            found = c.indels[k];
        } else if (ci.pos > ref_head_pos) {
            break;
        }
    }
    return found >= 0 ? found : -2;
}

// one candidate alignment -> ops (the walk of scoreCandidateAlignment :286-493 as host/align_flatten.cpp states it); returns the
// op count, -1 = leave this read to the host (it throws the reference's error, or handles what this form does not hold).
// WRITE = false only counts.
struct NoOpSink
{
    __device__ __forceinline__ void operator()(uint8_t, uint32_t, int32_t, bool) const {}
};

// SINK: called for every op in path order (kind, length, source offset, non-candidate penalty) -- the fused flatten + score kernel
// (F5) scores the op on the spot instead of storing it
template <bool WRITE, typename SINK = NoOpSink>
__device__ int flatten_cal(const FlatArgs& a, const int r, const PCal& c, const int32_t read_len, sk_score_op* ops, SINK&& sink = SINK())
{
    const int aps = c.n_seg;
    const int32_t win_begin = a.win_begin[r];
    const int n_ins = a.n_ins[r];
    const int16_t* ins_idx = a.ins_idx + size_t(r) * INS_CAP;
    const int32_t* ins_off = a.ins_off + size_t(r) * INS_CAP;
    unsigned read_offset = 0;
    int32_t ref_head_pos = c.pos;
    int ends_first = aps, ends_second = aps; // get_match_edge_segments, align_path.cpp:735-752
    {
        bool is_first_match = false;
        for (int i = 0; i < aps; ++i)
            if (seg_align_match(c.path[i].type)) {
                if (!is_first_match) ends_first = i;
                is_first_match = true;
                ends_second = i;
            }
    }
    int n = 0;
    auto emit = [&](const uint8_t kind, const uint32_t len, const int32_t src, const bool penalty) {
        if (kind == SK_OP_NOBASE && !penalty) return;
        sink(kind, len, src, penalty);
        if (WRITE) {
            sk_score_op op;
            op.length = uint16_t(len);
            op.kind = kind;
            op.flags = uint8_t(penalty ? SK_OPFLAG_NONCANDIDATE_PENALTY : 0);
            op.src = src;
            ops[n] = op;
        }
        ++n;
    };
    // offset of insert bases [head, head+len) of table indel `idx` in the pool, -1 = not representable here
    auto insert_src = [&](const int idx, const int32_t head, const uint32_t len) -> int32_t {
        const PIndel& k = a.job.tab[idx];
        if (head < 0 || uint32_t(head) + len > k.ins_len) return -1;
        for (int i = 0; i < n_ins; ++i)
            if (ins_idx[i] == idx) return ins_off[i] + head;
        return -1;
    };
    auto is_cand = [&](const int idx) -> bool { return job_cand(a.job, idx); };

    int path_index = 0;
    while (path_index < aps) {
        bool is_swap_start = false; // is_segment_swap_start, align_path.cpp:868-895
        {
            bool is_insert = false, is_delete = false;
            for (int i = path_index; i < aps; ++i) {
                if (c.path[i].type == SK_SEG_INSERT) is_insert = true;
                else if (c.path[i].type == SK_SEG_DELETE) is_delete = true;
                else break;
            }
            is_swap_start = is_insert && is_delete;
        }
        unsigned n_seg = 1;
        const PSeg ps = c.path[path_index];
        if (is_swap_start || ps.type == SK_SEG_SEQ_MISMATCH) {
            unsigned del_len, ins_len;
            if (ps.type == SK_SEG_SEQ_MISMATCH) {
                del_len = ins_len = ps.length;
            } else { // swap_info, align_path_util.hh:75-106
                int k = path_index;
                del_len = ins_len = 0;
                for (; k < aps && (c.path[k].type == SK_SEG_INSERT || c.path[k].type == SK_SEG_DELETE); ++k) {
                    if (c.path[k].type == SK_SEG_INSERT) ins_len += c.path[k].length;
                    else del_len += c.path[k].length;
                }
                n_seg = unsigned(k - path_index);
            }
            const int key = matching_indel(a.job, c, ref_head_pos, del_len, ins_len, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            int32_t head = 0;
            if (path_index < ends_first) head = int32_t(a.job.tab[key].ins_len) - int32_t(ps.length);
            const bool pen = !is_cand(key);
            if (ins_len > 0) {
                if (ins_len > 0xffffu) return -1;
                const int32_t src = insert_src(key, head, ins_len);
                if (src < 0) return -1;
                emit(SK_OP_BASES, ins_len, src, pen);
            } else {
                emit(SK_OP_NOBASE, 0, 0, pen);
            }
        } else if (seg_align_match(ps.type)) {
            emit(SK_OP_BASES, ps.length, ref_head_pos - win_begin, false);
        } else if (ps.type == SK_SEG_INSERT) {
            const int key = matching_indel(a.job, c, ref_head_pos, 0, ps.length, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            int32_t head = 0;
            if (path_index < ends_first) head = int32_t(a.job.tab[key].ins_len) - int32_t(ps.length);
            const int32_t src = insert_src(key, head, ps.length);
            if (src < 0) return -1;
            emit(SK_OP_BASES, ps.length, src, !is_cand(key));
        } else if (ps.type == SK_SEG_DELETE) {
            const int key = matching_indel(a.job, c, ref_head_pos, ps.length, 0, ends_first, ends_second, path_index);
            if (key < 0) return -1;
            emit(SK_OP_NOBASE, 0, 0, !is_cand(key));
        } else if (ps.type == SK_SEG_SKIP || ps.type == SK_SEG_HARD_CLIP) {
            // nothing
        } else if (ps.type == SK_SEG_SOFT_CLIP) {
            emit(SK_OP_SOFT_CLIP, ps.length, 0, false);
        } else {
            return -1;
        }
        for (unsigned i = 0; i < n_seg; ++i) { // increment_path, align_path_util.hh:38-68
            const PSeg s = c.path[path_index];
            if (seg_align_match(s.type)) {
                read_offset += s.length;
                ref_head_pos += int32_t(s.length);
            } else if (s.type == SK_SEG_DELETE || s.type == SK_SEG_SKIP) {
                ref_head_pos += int32_t(s.length);
            } else if (s.type == SK_SEG_INSERT || s.type == SK_SEG_SOFT_CLIP) {
                read_offset += s.length;
            }
            path_index++;
        }
    }
    if (int64_t(read_offset) != int64_t(read_len)) return -1;
    return n;
}

// L2, one thread per candidate alignment: how many ops it flattens to
__global__ __launch_bounds__(64) void op_count_kernel(const FlatArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cals) return;
    const int r = read_of_cal(a, c);
    const PCal& cal = a.pool[a.list[c]];
    const int n = flatten_cal<false>(a, r, cal, int32_t(a.read_off[r + 1] - a.read_off[r]), nullptr);
    if (n < 0) a.status[r] = ST_FAIL;
    a.n_ops[c] = n < 0 ? 0 : n;
}

// F1, one wave per read: the bytes of its haplotype pool
__global__ __launch_bounds__(64) void pool_fill_kernel(const FlatArgs a)
{
    const int r = blockIdx.x;
    if (a.cal_off[r + 1] == a.cal_off[r]) return;
    uint8_t* hap = a.hap_code + a.hap_off[r];
    const int32_t P = int32_t(a.hap_off[r + 1] - a.hap_off[r]);
    const int32_t wb = a.win_begin[r];
    const int n_ins = a.n_ins[r];
    const int16_t* idx = a.ins_idx + size_t(r) * INS_CAP;
    const int32_t* off = a.ins_off + size_t(r) * INS_CAP;
    const int32_t win_len = a.win_len[r];
    for (int32_t i = threadIdx.x; i < P; i += 64) {
        uint8_t v = SK_BAM_ANY;
        if (i < win_len) {
            const int32_t p = wb + i; // reference_contig_segment::get_base :46-51
            const bool outside = (p < a.ref_offset || p >= a.ref_offset + a.ref_len);
            if (outside && a.ref_outside) atomicAdd(a.ref_outside, 1);
            v = outside ? uint8_t(SK_BAM_ANY) : code_of(a.ref[p - a.ref_offset]);
        }
        for (int k = 0; k < n_ins; ++k) {
            const PIndel& d = a.job.tab[idx[k]];
            if (i >= off[k] && i < off[k] + int32_t(d.ins_len)) v = code_of(a.ins_pool[d.ins_off + uint32_t(i - off[k])]);
        }
        hap[i] = v;
    }
}

// F2, one thread per candidate alignment: the alignment itself (for the host), its ops, and the candidate-status lookups the
// host form performs for every indel of the alignment (cal_to_c)
__global__ __launch_bounds__(64) void flatten_kernel(const FlatArgs a)
{
    // The wave's 64 records travel pool -> LDS -> cals as rows of consecutive dwords: a lane copying its own 288-byte record field
    // by field made every load and store a scatter over 64 records (1.4 GB of traffic for 360 000 candidate alignments,
    // profiles/r03_v20_pmc_traffic.json); the lanes then read their record from LDS (stride 73 dwords: odd, conflict-free).
    constexpr int REC_DW = int(sizeof(PCal) / 4), REC_STRIDE = REC_DW | 1;
    static_assert(sizeof(PCal) % 4 == 0 && REC_DW <= 128, "a record is at most two dwords per lane");
    __shared__ uint32_t s_cal[64 * REC_STRIDE];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * blockDim.x;
    const int c = c0 + lane;
    const int nc = min(64, a.n_cals - c0);
    const int src_k = (lane < nc) ? a.list[c0 + lane] : 0;
    for (int k = 0; k < nc; ++k) {
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.pool + __shfl(src_k, k));
        uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(a.cals + (c0 + k));
        for (int j = lane; j < REC_DW; j += 64) {
            const uint32_t v = src[j];
            s_cal[k * REC_STRIDE + j] = v;
            dst[j] = v;
        }
    }
    __syncthreads();
    if (c >= a.n_cals) return;
    const int r = read_of_cal(a, c);
    const PCal& cal = *reinterpret_cast<const PCal*>(s_cal + lane * REC_STRIDE);
    if (a.status[r] != ST_OK) return; // (its op range is empty)
    (void)flatten_cal<true>(a, r, cal, int32_t(a.read_off[r + 1] - a.read_off[r]), a.ops + a.op_off[c]);
    for (int i = 0; i < cal.n_indels; ++i) (void)job_cand(a.job, cal.indels[i]);
    if (cal.lead >= 0) (void)job_cand(a.job, cal.lead);
    if (cal.trail >= 0) (void)job_cand(a.job, cal.trail);
}

// ---------------------------------------------------------------------------------------------------------------------
// F5, one wave per read: flattening AND scoring in one kernel -- scoreCandidateAlignment (starling_read_align_score.cpp:261-499) as the
// reference has it, one function from the alignment to its double.  F1-F3 + A1c stage the same work through HBM (the pool's bytes, 8-byte
// ops, transition entries, masks, column words: 6.8 x the algorithmic bytes, profiles/r03_v24_pmc_traffic.json) and wait on dependent
// global loads lane by lane (a wave of entries_wave_kernel took ~200 us per read); here the read (codes, the two terms of every position),
// its haplotype pool and the wave's 64 candidate-alignment records sit in LDS, every lane walks its alignment's path with flatten_cal and
// adds each op's terms as they come -- bases in read order, then the op's penalty, a soft clip's length x ln 0.25: the order of
// score_one_generic (score_alignments.hip), which A1 / A1c reproduce.  Nothing but the scores (and, while stage 3 reads them there, the
// records' copy in set order) goes back to HBM.
// A read this form does not hold (longer than F5_MAX_READ bases, pool over F5_MAX_POOL bytes) is counted in *n_unhandled: the caller
// then runs F1-F3 + A1c over the job.
constexpr int F5_MAX_READ = 256;  // (as F3's wave form; longer reads and larger pools take the staged chain)
constexpr int ONE_WAIT_MAX_READS = 16384; // reads of a job that runs as one fixed sequence (its buffers are sized by capacities: 256 leaves per read)
constexpr int F5_MAX_POOL = 768;
#ifndef F5_SORT
#define F5_SORT 1 // experiments: 0 = the set's order
#endif
constexpr int F5_TAB = 32;       // span of table indices the indels of one round's candidate alignments may cover (and the width of the
                                 // mask the round's consulted entries are gathered in: 32 bits, a bit an entry of the copy)

static_assert(F5_TAB <= 32, "the table copy is a lane an entry, the consulted mask a bit an entry");

struct FusedScoreArgs
{
    FlatArgs f;
    const uint8_t* read_qual;
    const SkTables* tab;
    double* scores;
    unsigned* err;         // SkContext::dev_error_flags (a quality above 70)
    int32_t* n_unhandled;  // reads left to the staged kernels
    int32_t write_cals;    // the records' copy in set order (stage 3 and sk_enum_device_fetch_cals read it)
    unsigned long long* dbg; // diagnostics ($SK_F5_TIMING): per read F5_STAMPS cycle stamps, or null
    unsigned* queue;       // [2] the launch's read queue: next read, waves that have left (both 0 between launches: the last wave out zeroes them)
    // the order of the launch's last hand-outs (tail_order_kernel): hand-out h in [tail_first, tail_first + tail_n) is read
    // tail_order[h - tail_first], every other hand-out h is read h; tail_n = 0: the job's own order throughout
    const int32_t* tail_order;
    uint32_t tail_first, tail_n;
    // round sharing (flatten_score_kernel): off with 0 ($SK_F5_SHARE); the rounds scored by a wave other than their read's owner
    int32_t share;
    unsigned* shared_rounds; // [2]: the helped rounds that were scored; the rounds after a read's first that turned their read down
                             // (sk_debug_f5_late_turn_downs: what tests look for a case by)
};

// a candidate alignment's slot in LDS: the walk's output -- up to F5_SEGS + 1 transitions, one per op that covers read positions and
// one for the read's end (start position | penalties that precede the op's terms << 9 | soft clip << 15 | (pool offset - position + 256)
// << 16).  The record's header, path and indel indices are in the lane's registers (F5Rec).  17 words a lane instead of round 3's 39:
// with the table entries cut to the five words the walk reads and the rows of terms sized for the job's longest read, a wave's LDS
// goes from 17.8 KB to under 10 KB and a CU holds 16 of them instead of 9 (profiles/r04_a5_history.txt: a wave alone on a CU takes as
// long as nine sharing it; with sixteen the vector unit is ~85 % busy, profiles/r05_f5_history.txt).
constexpr int F5_SEGS = 16, F5_INDELS = 8;
constexpr int F5_STAMPS = 11; // $SK_F5_TIMING: a read's stamps (f5_prologue, f5_round; the ninth is the cycles of the draw that handed
                              // it out, the tenth the 100 MHz counter at the read's start: where the read lies in the launch, the
                              // eleventh the rounds its owner scored itself)
constexpr int F5_SLOT = (F5_SEGS + 1) | 1; // (odd stride: conflict-free)
__device__ __forceinline__ int f5_ent_word(const int k) { return k; }
// doubles per read position: agree, 0.0, differ -- the read's own cases folded in (a '=' base: differ = agree; an N base and the pad
// rows past the read: both +0.0), so that phase B only asks whether the read byte and the pool byte differ, and a position past the
// op's end reads its row's 0.0: byte offset 0 = agree, 8 = past the op, 16 = differ
constexpr int F5_ROW = 3;

struct F5Tab // what the walk reads of a table entry
{
    int32_t pos;
    uint32_t del, ins_len;
    uint32_t type_cand; // type | cand << 8
    int32_t ins_at;     // where the entry's insert sequence starts in the read's pool, -1 = it is not there (ins_idx / ins_off by entry)
};

template <int MAXR>
struct F5Lds
{
    // (phase B fetches a position's eight bytes as the three aligned words that hold them: up to 11 bytes past the last position;
    // the two byte arrays first, where their words' offsets fit the immediate of a two-word LDS read)
    uint8_t read[MAXR + 12];
    uint8_t hap[F5_MAX_POOL + 12];
    double row[(MAXR + 8) * F5_ROW];
    uint32_t slot[64 * F5_SLOT]; // (phase B reads word F5_SLOT of a lane's slot too: the next lane's, or for lane 63 the table copy)
    // what the walk looks up per path segment (a chain of dependent look-ups: from HBM / L2 they cost a wave ~100 us per round)
    F5Tab tab[F5_TAB];
};
// (the CU hands LDS out in 1 280-byte pieces: 10 240 bytes are sixteen waves to a CU, one byte more fourteen; the 256-base form,
// ~12.4 KB, still fits three four-wave blocks)
constexpr int F5_Q_TERMS = 2 * (SK_NQ + 1); // the block's copy of q2lncompe and q2mis
constexpr size_t F5_SHARE_BYTES = 36; // a wave's claim word and descriptor (F5Share), and 8 bytes a block for its count of busy waves
constexpr size_t f5_block_granules(const size_t lds_object, const int waves) // a block's LDS in the CU's 1 280-byte pieces (128 to a CU)
{
    return ((lds_object + F5_SHARE_BYTES) * size_t(waves) + 8 * size_t(F5_Q_TERMS) + 8 + 1279) / 1280;
}
static_assert(sizeof(F5Lds<152>) <= 10240 && 2 * f5_block_granules(sizeof(F5Lds<152>), 8) <= 128, "two eight-wave blocks of the short-read form to a CU");
static_assert(3 * f5_block_granules(sizeof(F5Lds<F5_MAX_READ>), 4) <= 128, "three four-wave blocks of the long-read form to a CU");
static_assert((152 + 12) % 4 == 0 && (F5_MAX_READ + 12) % 4 == 0 && (F5_MAX_POOL + 12) % 4 == 0, "the byte arrays' words stay aligned");
static_assert(INS_CAP <= 64, "a lane an insert");
static_assert(F5_CODE_PAD >= F5_MAX_POOL + 16 && F5_CODE_PAD % 4 == 0, "a window that leaves the reference stays inside the pad");

// A compact record's path in the lane's registers: the walk looks at a segment's type up to a dozen times per turn (the edge
// segments, the look-ahead for swaps, the step to the next segment) and every look from LDS is a round trip on the lane's chain.  The
// sixteen types are 4 bits each in one 64-bit value, the sixteen lengths 16 bits each in four; segment i is a shift by i (the lengths:
// a select among the four values first).  The indel indices are 6 bits each relative to the round's table copy (tab_lo: every index
// of the round lies in [tab_lo, tab_lo + F5_TAB)), the eight of them in one 64-bit value.
struct F5Rec
{
    uint32_t w0, w1, w2;  // pos; lead | trail << 16; fwd | n_seg << 8 | n_indels << 16
    uint64_t types;       // segment i: bits [4i, 4i + 4)
    uint64_t l0, l1, l2, l3; // segment i: bits [16 (i & 3), + 16) of l(i >> 2)  (four values, not an array: an array indexed per lane
                          // goes to scratch memory)
    uint64_t ind;         // indel k: bits [6k, 6k + 6), its table index - ind_lo
    int ind_lo;
    __device__ __forceinline__ int32_t pos() const { return int32_t(w0); }
    __device__ __forceinline__ int lead() const { return int(int16_t(w1 & 0xffffu)); }
    __device__ __forceinline__ int trail() const { return int(int16_t(w1 >> 16)); }
    __device__ __forceinline__ int n_seg() const { return int((w2 >> 8) & 0xffu); }
    __device__ __forceinline__ int n_indels() const { return int((w2 >> 16) & 0xffu); }
    __device__ __forceinline__ int indel(const int k) const { return ind_lo + int(unsigned(ind >> (6 * k)) & 63u); }
};
static_assert(6 * F5_INDELS <= 64, "an indel index in 6 bits, eight in one value");

// flatten_cal over a compact record, every look-up from the block's LDS copies: the walk of scoreCandidateAlignment :286-493 as
// host/align_flatten.cpp states it, as ONE loop of selects.  Written with the reference's four branches (swap, sequence mismatch, insert,
// delete; match; soft clip; skip / hard clip) a turn is ~1 000 instructions, two thirds of them the scalar unit's mask bookkeeping, and
// the lanes of a wave take the branches in turn (round 4's form, profiles/r05_f5_history.txt).  Here what the branches have in common is
// computed once for every lane and selected: the segment kinds as bit sets over the path (one bit per 4-bit type: a run of insert /
// delete segments, the first and last match segment are shifts and bit counts, not loops), getMatchingIndelKey over packed entries
// (position; del << 16 | ins) up to the largest count in the wave, the insert's place in the pool from the table copy (F5Tab::ins_at).
// Only a swap (insert + delete run: rare) keeps a branch of its own.  The walk writes the alignment's transitions into its slot:
// one word per op that covers read positions and one for the read's end; returns their number, -1 = leave the read to the host form.
template <typename LDS>
__device__ __forceinline__ int f5_walk_selects(LDS& S, const F5Rec c, const bool has, const int tab_lo, const int32_t win_begin, uint32_t& consulted,
                                               const int32_t L, const int32_t P, uint32_t* const myslot)
{
    constexpr uint64_t N1 = 0x1111111111111111ull;
    const uint64_t types = c.types, p_l0 = c.l0, p_l1 = c.l1, p_l2 = c.l2, p_l3 = c.l3;
    const int aps = has ? c.n_seg() : 0;
    auto eq4 = [=](const unsigned v) -> uint64_t { // bit 4 i: segment i is of type v
        uint64_t x = types ^ (N1 * v);
        x |= x >> 1;
        x |= x >> 2;
        return ~x & N1;
    };
    auto seg_len = [=](const int i) -> unsigned {
        const uint64_t lo = (i & 4) ? p_l1 : p_l0, hi = (i & 4) ? p_l3 : p_l2;
        return unsigned(((i & 8) ? hi : lo) >> (16 * (i & 3))) & 0xffffu;
    };
    const uint64_t in_path = (aps >= 16) ? N1 : (((1ull << (4 * aps)) - 1ull) & N1);
    const uint64_t M4 = (eq4(SK_SEG_MATCH) | eq4(SK_SEG_SEQ_MATCH) | eq4(SK_SEG_SEQ_MISMATCH)) & in_path;
    const uint64_t I4 = eq4(SK_SEG_INSERT) & in_path, D4 = eq4(SK_SEG_DELETE) & in_path;
    // get_match_edge_segments, align_path.cpp:735-752
    const int ends_first = M4 ? (__builtin_ctzll(M4) >> 2) : aps, ends_second = M4 ? ((63 - __builtin_clzll(M4)) >> 2) : aps;
    // the alignment's indels, read once: position and the two lengths as one word (del << 16 | ins; an entry that is a breakpoint, or no
    // entry, holds a word no segment asks for); lengths of 0xffff and more are left to the host form
    const int ni = c.n_indels();
    int ni_wave = 0; // (the most indels any of the wave's alignments holds: the entries past it are not looked at)
#pragma unroll
    for (int k = 1; k <= F5_INDELS; ++k) ni_wave = __any(ni >= k) ? k : ni_wave;
    int32_t k_pos[F5_INDELS];
    uint32_t k_pack[F5_INDELS];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < F5_INDELS; ++k) {
        k_pos[k] = INT_MIN;
        k_pack[k] = 0xffffffffu;
        if (k < ni_wave) {
            const F5Tab& ci = S.tab[((k < ni) ? c.indel(k) : tab_lo) - tab_lo];
            const unsigned ty = ci.type_cand & 0xffu;
            const bool kind = (ty == SK_INDEL_INDEL || ty == SK_INDEL_MISMATCH);
            if (k < ni) {
                k_pos[k] = ci.pos;
                if (kind) {
                    k_pack[k] = (ci.del << 16) | ci.ins_len;
                    bad = bad || ci.del >= 0xffffu || ci.ins_len >= 0xffffu;
                }
            }
        }
    }
    int pi = 0, n_ent = 0;
    int32_t pos = 0, ref_head_pos = c.pos(); // (read_offset of the reference's walk)
    unsigned npen = 0;
    for (;;) {
        const bool live = pi < aps && !bad;
        if (!__any(live)) break;
        const int sh = 4 * (pi & 15);
        const unsigned ty = unsigned(types >> sh) & 15u, ln = seg_len(pi & 15);
        // the run of insert / delete segments that starts here (is_segment_swap_start, align_path.cpp:868-895: a swap = both kinds in it)
        const uint64_t not_run = ~((I4 | D4) >> sh) & N1;
        const int run4 = not_run ? __builtin_ctzll(not_run) : 64;
        const uint64_t run_set = (run4 >= 64) ? ~0ull : ((1ull << run4) - 1ull);
        const bool is_swap = live && ((I4 >> sh) & run_set) != 0ull && ((D4 >> sh) & run_set) != 0ull;
        const bool is_match = (ty == SK_SEG_MATCH || ty == SK_SEG_SEQ_MATCH), is_clip = (ty == SK_SEG_SOFT_CLIP);
        const bool is_indel_seg = is_swap || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_INSERT || ty == SK_SEG_DELETE;
        unsigned del_len = (ty == SK_SEG_INSERT) ? 0u : ln, ins_len = (ty == SK_SEG_DELETE) ? 0u : ln;
        int n_seg = 1;
        unsigned read_step = (is_match || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_INSERT || is_clip) ? ln : 0u; // increment_path, align_path_util.hh:38-68
        unsigned ref_step = (is_match || ty == SK_SEG_SEQ_MISMATCH || ty == SK_SEG_DELETE || ty == SK_SEG_SKIP) ? ln : 0u;
        if (is_swap) { // swap_info, align_path_util.hh:75-106
            n_seg = run4 >> 2;
            del_len = ins_len = 0;
            for (int k = 0; k < n_seg; ++k) {
                const unsigned l = seg_len((pi + k) & 15);
                if ((I4 >> (4 * ((pi + k) & 15))) & 1ull) ins_len += l;
                else del_len += l;
            }
            read_step = ins_len;
            ref_step = del_len;
        }
        // getMatchingIndelKey, starling_read_align_score.cpp:177-228: the edge indels outside the match segments; between them the one
        // entry of the alignment's that is this indel -- the reference stops at a second match and at the first entry past the position
        const unsigned asked = (del_len << 16) | ins_len;
        const bool askable = del_len < 0xffffu && ins_len < 0xffffu;
        int k_found = 0, n_found = 0;
        bool open = true;
#pragma unroll
        for (int k = 0; k < F5_INDELS; ++k) {
            if (k < ni_wave) {
                const bool m = open && k_pos[k] == ref_head_pos && k_pack[k] == asked;
                k_found = m ? k : k_found;
                n_found += m ? 1 : 0;
                open = open && (m || k_pos[k] <= ref_head_pos);
            }
        }
        int key = (n_found == 1) ? c.indel(k_found) : -2;
        key = (pi < ends_first) ? c.lead() : (pi > ends_second) ? c.trail() : key;
        const bool key_ok = key >= 0;
        const F5Tab te = S.tab[(key_ok ? key : tab_lo) - tab_lo];
        const bool indel_ok = live && is_indel_seg && key_ok;
        consulted |= indel_ok ? (1u << ((key - tab_lo) & 31)) : 0u; // job_cand: bit key - tab_lo (the copy holds F5_TAB <= 32 entries)
        const bool pen = is_indel_seg && (te.type_cand >> 8) == 0u;
        const int32_t head = (pi < ends_first) ? int32_t(te.ins_len) - int32_t(ln) : 0;
        // the op: bases of the pool (a match segment's window bytes, an indel's insert sequence), a soft clip, or a penalty alone
        const bool ins_bases = is_indel_seg && ins_len > 0u;
        const bool ins_ok = ins_len <= 0xffffu && head >= 0 && uint32_t(head) + ins_len <= te.ins_len && te.ins_at >= 0;
        const bool bases = ins_bases || is_match;
        const int32_t src = ins_bases ? te.ins_at + head : ref_head_pos - win_begin;
        const unsigned len = ins_bases ? ins_len : ln;
        const bool known = is_indel_seg || is_match || is_clip || ty == SK_SEG_SKIP || ty == SK_SEG_HARD_CLIP;
        bool fail = !known || (is_indel_seg && (!key_ok || !askable)) || (ins_bases && !ins_ok);
        const bool entry = (bases || (is_clip && !is_indel_seg)) && len > 0u;
        if (entry) {
            fail = fail || pos + int32_t(len) > L || (bases && (src < 0 || int64_t(src) + int64_t(len) > int64_t(P)));
            const int hidx = bases ? int(src) - pos : 0;
            fail = fail || n_ent > F5_SEGS || npen > 4u || hidx < -256 || hidx > 3839;
            if (live && !fail) myslot[f5_ent_word(n_ent)] = unsigned(pos) | (npen << 9) | (bases ? 0u : 1u << 15) | (unsigned(hidx + 256) << 16);
        }
        if (live) {
            bad = fail;
            n_ent += entry ? 1 : 0;
            npen = entry ? (pen ? 1u : 0u) : npen + (pen ? 1u : 0u);
            pos += int32_t(read_step);
            ref_head_pos += int32_t(ref_step);
            pi += n_seg;
        }
    }
    if (!has) return 0;
    if (bad || pos != L || n_ent > F5_SEGS || npen > 4u) return -1;
    myslot[f5_ent_word(n_ent)] = unsigned(L) | (npen << 9) | (256u << 16); // trailing penalties
    return n_ent + 1;
}

// Phase B of F5, a lane its alignment, in path order (the order of score_one_generic): entering an op, the penalties that precede its
// terms, then a soft clip's length x ln 0.25; inside an op of bases, eight positions per turn -- eight read codes against the eight pool
// bytes they face (SWAR), each position's address: its row's agree or differ term, or the row's 0.0 past the op's end (the rows already
// hold what a '=' or an N read base adds) -- eight reads, eight adds.  ONE loop per lane (eight bases and the step to the next op in the
// same turn), so that the turns a wave makes are the longest lane's, not the sum over ops of the longest op.  What is rare for a whole
// wave -- a penalty, a soft clip -- sits behind a vote.
template <typename LDS>
__device__ __forceinline__ double f5_sum(LDS& S, const uint32_t* const myslot, const int n_ent, const double ln_noncand, const double ln_quarter)
{
    double lnp = 0.0;
    const unsigned char* rows = reinterpret_cast<const unsigned char*>(S.row);
    int e = 0, p = 0, stop = 0, hidx = 0;
    // the current op's transition and the next one stay in registers: a turn reads one slot word, the one after them (word e + 1 <=
    // n_ent <= F5_SLOT: past the read's end it is a word of the LDS object that nothing looks at)
    uint32_t cur = myslot[f5_ent_word(0)], nxt = myslot[f5_ent_word(1)];
    // the step to the next op, by selects (the loop has one back edge); true: the read's end
    auto next_op = [&]() -> bool {
        const bool adv = (p >= stop);
        const int start = int(cur & 0x1ffu), next_start = int(nxt & 0x1ffu);
        const unsigned np = adv ? ((cur >> 9) & 63u) : 0u; // (at most 4: the walk hands anything longer to the host form)
        const bool clip = adv && (cur & (1u << 15)) != 0u; // (never the read's end: its word holds no soft clip)
        if (__builtin_amdgcn_ballot_w64(np != 0u || clip) != 0ull) { // (both rare: one vote)
            const double l1 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 1u) ? l1 : lnp;
            const double l2 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 2u) ? l2 : lnp;
            const double l3 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 3u) ? l3 : lnp;
            const double l4 = __dadd_rn(lnp, ln_noncand);
            lnp = (np >= 4u) ? l4 : lnp;
            const double lc = __dadd_rn(lnp, __dmul_rn(double(unsigned(next_start - start)), ln_quarter));
            lnp = clip ? lc : lnp;
        }
        if (adv && e + 1 >= n_ent) return true;
        p = adv ? (clip ? next_start : start) : p;
        stop = adv ? next_start : stop;
        hidx = adv ? int(cur >> 16) - 256 : hidx;
        e = adv ? e + 1 : e;
        cur = adv ? nxt : cur;
        nxt = myslot[f5_ent_word(e + 1)];
        return false;
    };
    if (next_op()) return lnp; // (the first op: no bases before it)
    for (;;) {
        {
            const int m = stop - p;          // bases of the current op still to add (0: a soft clip just stepped over)
            const int mm = (m > 8) ? 8 : m;
            // the eight read codes at p and the eight pool bytes they face, each from the three aligned words that hold them (a byte
            // address read as one 8-byte word is an unaligned LDS access: replayed); 32-bit halves, positions 0-3 and 4-7
            const int ph = p + hidx;
            const uint32_t* const rw = reinterpret_cast<const uint32_t*>(S.read + (p & ~3));
            const uint32_t* const hw = reinterpret_cast<const uint32_t*>(S.hap + (ph & ~3));
            const uint32_t r0 = rw[0], r1 = rw[1], r2 = rw[2], h0 = hw[0], h1 = hw[1], h2 = hw[2];
            const uint32_t R[2] = {__builtin_amdgcn_alignbyte(r1, r0, unsigned(p)), __builtin_amdgcn_alignbyte(r2, r1, unsigned(p))};
            const uint32_t H[2] = {__builtin_amdgcn_alignbyte(h1, h0, unsigned(ph)), __builtin_amdgcn_alignbyte(h2, h1, unsigned(ph))};
            // 0x18 in the bytes of the positions past the op's end (a suffix of the eight)
            const uint64_t past = (mm >= 8) ? 0ull : (0x1818181818181818ull << (8 * mm));
            constexpr uint32_t B0F = 0x0f0f0f0fu, B10 = 0x10101010u;
            uint32_t sel[2]; // per byte the offset in the position's row: 0 agree, 8 past the op's end (0.0), 16 differ
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // (the codes are 4-bit: x ^ y + 15 sets bit 4 of a byte exactly when the two differ; a byte past the op may carry into
                // the next one, which is past the op too, and the select drops both: bit 4 from the compare where the position is the
                // op's, bit 3 = past the op)
                const uint32_t x = (R[h] ^ H[h]) + B0F;
                uint32_t pm = uint32_t(past >> (32 * h));
                // (no known bits for the compiler to act on: the select stays one three-input bit op, the bytes' extraction below the
                // byte-select operands of the adds)
                __asm__("" : "+v"(pm));
                sel[h] = (B10 & ~pm & x) | (~B10 & pm);
                __asm__("" : "+v"(sel[h]));
            }
            const unsigned base = __umul24(unsigned(8 * F5_ROW), unsigned(p));
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned at = base + unsigned(8 * F5_ROW * u) + ((sel[u >> 2] >> (8 * (u & 3))) & 0xffu);
                v[u] = *reinterpret_cast<const double*>(rows + at);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) lnp = __dadd_rn(lnp, v[u]);
            p += mm;
        }
        if (next_op()) break;
    }
    return lnp;
}

// TIMING: the cycle stamps of $SK_F5_TIMING (fa.dbg); without it the stamps are constants and their s_memtime + waits are gone
// a block is F5_WAVES waves, each with a read and an LDS object of its own: what orders a wave's LDS accesses is the wave (its LDS
// instructions complete in order), so the points where the lanes exchange data through LDS need the compiler's and the counters'
// attention, not a workgroup barrier
__device__ __forceinline__ void f5_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a record as it is loaded: header + F5_SEGS path segments (five 16-byte loads) + F5_INDELS indel indices, all in flight at once
struct F5Raw
{
    uint4 q0, q1, q2, q3, q4;
    uint32_t i0, i1, i2, i3;
};
__device__ __forceinline__ F5Raw f5_load_raw(const PCal* src)
{
    F5Raw w;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    w.q0 = s4[0], w.q1 = s4[1], w.q2 = s4[2], w.q3 = s4[3], w.q4 = s4[4];
    const uint32_t* si = reinterpret_cast<const uint32_t*>(src->indels);
    w.i0 = si[0], w.i1 = si[1], w.i2 = si[2], w.i3 = si[3];
    return w;
}

constexpr int F5_INS_REG = 4;  // inserts of up to 64 bases each whose bytes the prologue holds in registers (a lane a base)

// The prologue's global loads go out as GROUPS, each waited for once (a wave that asks for one value at a time waits ~1 us for each:
// the prologue and the staging were 46k of a read's 122k cycles, nearly all of it such waits -- profiles/r08_f5_history.txt):
//   group 1  what is indexed by the read alone (cal_off, status, read_off, hap_len, win_begin, n_ins, win_len): uniform loads, above
//            the early return -- every index is in range for r < n_reads
//   group 2  what group 1 addresses: list[] of the first round, the job's table (when it fits the copy: one copy per
//            read, tab_lo = 0), ins_idx / ins_off, the window's codes (words of the job's code image: the pad answers for a window
//            that leaves the reference), the read's codes and qualities, n_seg8
//   group 3  what group 2 addresses: the first round's records (where the set's order is kept) and the inserts' bytes (up to
//            F5_INS_REG inserts of up to 64 bases in registers, written in table order; more or longer ones: the loop)
// With the draw from the queue that is four waits for a read of one round (counted in the assembly, profiles/r08_f5_history.txt); a
// later round waits for its records only (its list[] entry is asked for a round ahead).  The two terms of a quality come from the
// block's copy in LDS (q_terms: q2lncompe, then q2mis).  Not built: the read's codes and qualities as words and S.read written with
// word stores -- they are loaded and stored a byte a lane (up to three of each in flight at once, no wait between them).
//
// A read is scored in two parts.  f5_prologue is its owner's alone: everything up to the first round -- the loads above, the read, the
// pool, the rows of terms, the order and (where the job's table fits it) the table copy written into the owner's LDS object, which
// nothing writes again until the owner's next read.  f5_round is one round of up to 64 candidate alignments: staging, walk, sums, the
// consulted marks, the scores' store.  It reads the read's data through a pointer and writes the EXECUTING wave's slots only, so that
// a wave other than the owner can run it (flatten_score_kernel); what it needs of the read beyond the LDS object is in F5Desc.
struct F5Desc // a read's uniforms, as a round needs them
{
    int32_t r, c0, ncr, L, P, win_begin, sorted_order;
};
// what the owner carries from the prologue into its rounds and from a round into its next one
struct F5Own
{
    int32_t slot_next;      // where the lane's record of the owner's coming round is (list[] a round ahead)
    F5Raw raw0;             // round 0's records, asked for in group 3
    int my_ins_idx;         // lane k < n_ins: the read's insert k (a job whose table does not fit the copy places it per round)
    int32_t my_ins_off;
    unsigned long long stamp[F5_STAMPS], wall0; // $SK_F5_TIMING
};
// a wave's published read, in the block's LDS (flatten_score_kernel: round sharing)
struct F5Share
{
    uint32_t claim; // the next round nobody has claimed | the read's rounds << 16; 0: nothing open
    F5Desc d;
    uint32_t dry_at; // the wave has drawn dry: the 100 MHz counter's low word then, | 1 (0: not yet)
};
static_assert(sizeof(F5Share) == F5_SHARE_BYTES, "f5_block_granules counts the claim words and descriptors");

template <int MAXR, bool TIMING>
__device__ __forceinline__ bool f5_prologue(const FusedScoreArgs& fa, const int r, F5Lds<MAXR>& S, const double* const q_terms, F5Desc& desc,
                                            F5Own& own) // false: the read has nothing to score here
{
    auto now = [&]() -> unsigned long long { return TIMING ? (unsigned long long)clock64() : 0ull; };
    const FlatArgs& a = fa.f;
    unsigned long long(&stamp)[F5_STAMPS] = own.stamp;
    // (the lane as a value of this read's: what is computed from it -- addresses of the loads below -- is computed here, not once
    // per kernel and kept in scratch memory, whose reload is one more wait in the middle of a group)
    int lane_of_read = threadIdx.x & 63;
    __asm__ volatile("" : "+v"(lane_of_read));
    const int lane = lane_of_read;
    stamp[0] = now(); // (before group 1: the prologue's figure holds every trip of the read but the draw, as it did)
    own.wall0 = TIMING ? (unsigned long long)wall_clock64() : 0ull; // (the constant 100 MHz counter: the block's life in time)
    // ---- group 1 (the empty statement keeps the loads together above the early return: every value is asked for before the first
    // is looked at; they are the same in every lane)
    int g1_c0 = a.cal_off[r], g1_c1 = a.cal_off[r + 1];
    int32_t g1_status = a.status[r];
    int64_t g1_ro = a.read_off[r], g1_ro1 = a.read_off[r + 1];
    int32_t g1_P = a.hap_len[r], g1_win_begin = a.win_begin[r], g1_n_ins = a.n_ins[r], g1_win_len = a.win_len[r];
    __asm__ volatile("" : "+v"(g1_c0), "+v"(g1_c1), "+v"(g1_status), "+v"(g1_ro), "+v"(g1_ro1), "+v"(g1_P), "+v"(g1_win_begin), "+v"(g1_n_ins), "+v"(g1_win_len));
    auto uniform64 = [](const int64_t v) -> int64_t {
        return int64_t(uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uint64_t(v)))))) |
                       (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(uint64_t(v) >> 32))))) << 32));
    };
    const int c0 = __builtin_amdgcn_readfirstlane(g1_c0), c1 = __builtin_amdgcn_readfirstlane(g1_c1);
    const int32_t status_r = __builtin_amdgcn_readfirstlane(g1_status);
    const int64_t ro = uniform64(g1_ro), ro1 = uniform64(g1_ro1);
    const int32_t P = __builtin_amdgcn_readfirstlane(g1_P);
    const int32_t win_begin = __builtin_amdgcn_readfirstlane(g1_win_begin);
    const int n_ins = __builtin_amdgcn_readfirstlane(g1_n_ins);
    const int32_t win_len = __builtin_amdgcn_readfirstlane(g1_win_len);
    const int ncr = c1 - c0;
    if (ncr == 0 || status_r != ST_OK) return false;
    for (int i = 1; i < F5_STAMPS; ++i) stamp[i] = 0;
    const int32_t L = int32_t(ro1 - ro);
    if (L > MAXR || P > F5_MAX_POOL) {
        if (lane == 0) atomicAdd(fa.n_unhandled, 1);
        return false;
    }
    // the job's table fits the copy: one copy per read, every index relative to entry 0
    const int job_n_tab = a.job.n_tab;
    const bool whole_tab = job_n_tab <= F5_TAB;
    uint8_t* const order = S.hap + ((P + 8 + 3) & ~3);
    const bool sorted_order = (F5_SORT != 0) && ncr > 64 && ncr <= 256 && ((P + 8 + 3) & ~3) + ncr <= int(sizeof(S.hap));
    // ---- group 2, every load issued before the first use
    // where the lane's record of the coming round is: list[] a round ahead (the first round's here, where the lanes take the read's
    // alignments in the set's order, or after the sort; the next round's while this round's sums run), so that a round waits for its
    // records only
    int32_t slot_next = 0;
    if (!sorted_order && lane < ncr) slot_next = a.list[c0 + lane];
    int32_t lst[4]; // (a read whose alignments are put in order first: list[] of all of them)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lst[k] = 0;
        if (sorted_order && lane + 64 * k < ncr) lst[k] = a.list[c0 + lane + 64 * k];
    }
    F5Tab g; // lane t: entry t of the job's table (whole_tab)
    g.pos = 0, g.del = 0, g.ins_len = 0, g.type_cand = 0, g.ins_at = -1;
    uint32_t g_ins_off = 0;
    if (whole_tab && lane < job_n_tab) {
        const PIndel& e = a.job.tab[lane];
        g.pos = e.pos;
        g.del = e.del;
        g.ins_len = e.ins_len;
        g.type_cand = unsigned(e.type) | (unsigned(e.cand) << 8);
        g_ins_off = e.ins_off;
    }
    int my_ins_idx = -1;    // lane k < n_ins: the table index of the read's insert k and where its sequence starts in the pool
    int32_t my_ins_off = 0;
    if (lane < n_ins) {
        my_ins_idx = a.ins_idx[size_t(r) * INS_CAP + lane];
        my_ins_off = a.ins_off[size_t(r) * INS_CAP + lane];
    }
    // the window's codes, a lane a word of the pool: bytes [win_len, P + 8) stay SK_BAM_ANY
    constexpr int HAP_WORDS = int(sizeof(S.hap)) / 4, HAP_K = (HAP_WORDS + 63) / 64;
    constexpr uint32_t ANY4 = 0x01010101u * uint32_t(SK_BAM_ANY);
    uint32_t hw[HAP_K];
    {
        // (32-bit from here: a window that begins further out than the pad reads pad all the same)
        const int32_t p_max = int32_t(min(int64_t(a.ref_len) + F5_CODE_PAD - 4, int64_t(INT_MAX - 2 * F5_CODE_PAD)));
        const int32_t wbase = int32_t(min(max(int64_t(win_begin) - int64_t(a.ref_offset), int64_t(-2 * F5_CODE_PAD)), int64_t(p_max) + F5_CODE_PAD));
#pragma unroll
        for (int k = 0; k < HAP_K; ++k) {
            const int w = lane + 64 * k;
            hw[k] = ANY4;
            if (4 * w < win_len) {
                // (a word that lies beyond the pad on either side holds positions outside the reference only, as the pad does)
                const int32_t p = min(max(wbase + 4 * w, -F5_CODE_PAD), p_max);
                uint32_t v;
                __builtin_memcpy(&v, a.ref_code + p, 4);
                hw[k] = v;
            }
        }
    }
    constexpr int READ_K = (MAXR + 12 + 63) / 64;
    uint8_t rc[READ_K], rq[READ_K];
#pragma unroll
    for (int k = 0; k < READ_K; ++k) {
        const int i = lane + 64 * k;
        rc[k] = SK_BAM_ANY;
        rq[k] = 0;
        if (i < L) {
            rc[k] = a.read_code[ro + i];
            rq[k] = fa.read_qual[ro + i];
        }
    }
    uint8_t seg8[4]; // (left by pool_bounds_kernel, which reads every record anyway; looked at after the pool is placed)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        seg8[k] = 0;
        if (sorted_order && lane + 64 * k < ncr) seg8[k] = a.n_seg8[c0 + lane + 64 * k];
    }
    // The read's candidate alignments in order of path length, longest first (a counting sort over the segment counts, the order in the
    // unused tail of the pool's bytes): a wave's walk lasts as long as its longest path, so a round of like paths wastes fewer turns
    // and the last, partly filled round gets the short ones.  Reads with more than 256 candidate alignments keep the set's order.
    // Done before the pool is placed: the order lies past the pool's bytes, and the first round's records can go out at once.  list[] of
    // all the read's alignments, up to 256, is parked in the slots meanwhile (the first round's walk is the first to write there).
    if (sorted_order) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < ncr) S.slot[lane + 64 * k] = uint32_t(lst[k]);
        int seg_of[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) seg_of[k] = (lane + 64 * k < ncr) ? min(int(seg8[k]), F5_SEGS + 1) : -1;
        // (only the segment counts that occur: a read's alignments have a handful of distinct ones -- the loop over all eighteen was ~650
        // of a read's ~7 800 instructions)
        unsigned present = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) present |= (seg_of[k] >= 0) ? (1u << seg_of[k]) : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) present |= unsigned(__shfl_xor(int(present), d));
        present = unsigned(__builtin_amdgcn_readfirstlane(int(present)));
        int at = 0; // alignments placed so far
        while (present != 0u) { // descending, as the loop over every count was
            const int v = 31 - __builtin_clz(present);
            present &= ~(1u << v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t m = __ballot(seg_of[k] == v);
                if (seg_of[k] == v) order[at + __popcll(m & ((1ull << lane) - 1ull))] = uint8_t(lane + 64 * k);
                at += __popcll(m);
            }
        }
        f5_wave_sync(); // (the order written)
        slot_next = int32_t(S.slot[order[lane]]); // (more than 64 alignments: every lane has one)
    }
    // ---- group 3: the inserts' bytes, then the first round's records -- all issued before either is looked at
    // (insert k's length and source stay in lane k's registers; its table index and offset go into the table copy, F5Tab::ins_at)
    int32_t my_ins_len = 0;
    uint32_t my_ins_src = 0;
    if (whole_tab) {
        const int32_t len_t = __shfl(int32_t(g.ins_len), my_ins_idx & 63);
        const uint32_t src_t = uint32_t(__shfl(int(g_ins_off), my_ins_idx & 63));
        if (lane < n_ins) {
            my_ins_len = len_t;
            my_ins_src = src_t;
        }
    } else if (lane < n_ins) {
        my_ins_len = int32_t(a.job.tab[my_ins_idx].ins_len);
        my_ins_src = a.job.tab[my_ins_idx].ins_off;
    }
    const bool ins_in_regs = n_ins <= F5_INS_REG && !__any(my_ins_len > 64);
    uint32_t ib[F5_INS_REG]; // (a register each: bytes packed into one would be waited for one by one)
    int32_t ib_n[F5_INS_REG];
    uint32_t ib_src[F5_INS_REG];
#pragma unroll
    for (int k = 0; k < F5_INS_REG; ++k) { // (lengths and sources first: the one wait for them stands before the first insert's load)
        ib_n[k] = ins_in_regs ? __builtin_amdgcn_readlane(my_ins_len, k) : 0; // (a lane that is no insert holds 0)
        ib_src[k] = uint32_t(__builtin_amdgcn_readlane(int(my_ins_src), k));
    }
#pragma unroll
    for (int k = 0; k < F5_INS_REG; ++k) {
        ib[k] = SK_BAM_ANY;
        if (lane < ib_n[k]) ib[k] = a.ins_code[ib_src[k] + uint32_t(lane)];
    }
    // (every lane loads -- one without an alignment the record its slot_next names, 0 or a former round's, which nothing looks at:
    // a load that some lanes skip is merged with the registers' former values, and that merge waits for the load where it is issued)
    own.raw0 = f5_load_raw(a.pool + slot_next);
    // ---- the pool's bytes (as pool_fill_kernel), the read, its rows of terms, the pool's layout
    if (a.ref_outside && lane == 0) { // (the window's positions that lie outside the job's reference segment: they read as N)
        const int64_t b = max(int64_t(win_begin), int64_t(a.ref_offset));
        const int64_t e = min(int64_t(win_begin) + int64_t(win_len), int64_t(a.ref_offset) + int64_t(a.ref_len));
        const int32_t outside = win_len - int32_t(max(e - b, int64_t(0)));
        if (outside > 0) atomicAdd(a.ref_outside, outside);
    }
    {
        uint32_t* const hap_w = reinterpret_cast<uint32_t*>(S.hap);
        const int n_words = (P + 8 + 3) >> 2; // (at most HAP_WORDS - 1: the array holds F5_MAX_POOL + 12 bytes)
#pragma unroll
        for (int k = 0; k < HAP_K; ++k) {
            const int w = lane + 64 * k;
            const int keep = win_len - 4 * w; // bytes of the word that are the window's
            const uint32_t m = (keep >= 4) ? 0xffffffffu : (keep <= 0) ? 0u : ((1u << (8 * keep)) - 1u);
            if (w < n_words) hap_w[w] = (hw[k] & m) | (ANY4 & ~m);
        }
    }
    if (whole_tab) {
        if (lane < job_n_tab) S.tab[lane] = g;
        f5_wave_sync();
        // (the read's inserts are distinct table indices, pool_layout_kernel: a lane an insert, no two write the same entry)
        if (lane < n_ins && my_ins_idx < job_n_tab) S.tab[my_ins_idx].ins_at = my_ins_off;
    }
    f5_wave_sync();
    // the insert sequences, in table order (a later one overwrites an earlier one, as pool_fill_kernel)
    if (ins_in_regs) {
#pragma unroll
        for (int k = 0; k < F5_INS_REG; ++k) {
            if (k < n_ins) {
                const int32_t o = __builtin_amdgcn_readlane(my_ins_off, k), n = __builtin_amdgcn_readlane(my_ins_len, k);
                if (lane < n && o + lane < P) S.hap[o + lane] = uint8_t(ib[k]);
            }
        }
    } else {
        for (int k = 0; k < n_ins; ++k) {
            const int32_t o = __builtin_amdgcn_readlane(my_ins_off, k), n = __builtin_amdgcn_readlane(my_ins_len, k);
            const uint32_t src = uint32_t(__builtin_amdgcn_readlane(int(my_ins_src), k));
            for (int32_t i = lane; i < n; i += 64)
                if (o + i < P) S.hap[o + i] = a.ins_code[src + uint32_t(i)];
        }
    }
#pragma unroll
    for (int k = 0; k < READ_K; ++k) {
        const int32_t i = lane + 64 * k;
        if (i < L + 12) {
            unsigned q = rq[k];
            const uint8_t code = rc[k];
            if (q > 70u) { // the reference throws (qscore_cache.cpp:53-75): flagged, sk_check_device_errors reports it
                atomicOr(fa.err, unsigned(SK_DEVERR_QSCORE));
                q = 70u;
            }
            S.read[i] = code & 15u;
            if (i < L + 8) { // (the row of a '=' base adds its agree term either way, an N base and a pad row +0.0)
                const unsigned c = code & 15u;
                const bool adds = i < L && c != 15u;
                const double agree = adds ? q_terms[q] : 0.0;
                S.row[F5_ROW * i] = agree;
                S.row[F5_ROW * i + 1] = 0.0;
                S.row[F5_ROW * i + 2] = !adds ? 0.0 : (c == 0u) ? agree : q_terms[SK_NQ + 1 + q];
            }
        }
    }
    desc.r = r, desc.c0 = c0, desc.ncr = ncr, desc.L = L, desc.P = P, desc.win_begin = win_begin, desc.sorted_order = sorted_order ? 1 : 0;
    own.slot_next = slot_next;
    own.my_ins_idx = my_ins_idx;
    own.my_ins_off = my_ins_off;
    return true;
}

// the place of alignment 64 j + lane of the read in list[] (a round's lanes take the read's alignments in the set's order, or after the
// sort: the order's bytes lie past the pool's in the read's LDS object)
template <typename LDS>
__device__ __forceinline__ int f5_list_index(const LDS& D, const F5Desc& d, const int at)
{
    const uint8_t* const order = D.hap + ((d.P + 8 + 3) & ~3);
    return d.c0 + (d.sorted_order ? int(order[at]) : at);
}

// One round: alignments [64 j, 64 j + 64) of the read d, whose data the prologue left in D.  `mine`: the executing wave is the read's
// owner (D is its own LDS object); else it is a helper -- it reads D, writes its own slots (myslot), and has loaded own.slot_next at the
// round's start.  The owner's round 0 finds its records asked for by the prologue; every other round asks for them here.  `next_j` (the
// owner's): called between the walk and the sums, it names the owner's next round or -1, so that list[] of that round is asked for
// behind the sums.  Returns false where the round ends the read for this form (a record beyond the compact form, an index outside the
// table: counted in *n_unhandled, the staged chain takes the job).
template <int MAXR, bool TIMING, typename NextRound>
__device__ __forceinline__ bool f5_round(const FusedScoreArgs& fa, F5Lds<MAXR>& D, uint32_t* const slots, const F5Desc& d, const int j, const bool mine,
                                         F5Own& own, NextRound next_j, int& j_next)
{
    auto now = [&]() -> unsigned long long { return TIMING ? (unsigned long long)clock64() : 0ull; };
    const FlatArgs& a = fa.f;
    unsigned long long(&stamp)[F5_STAMPS] = own.stamp; // (a helper's rounds are not stamped: the stamps are a read's, stored by its owner)
    F5Lds<MAXR>& S = D;
    F5Raw& raw0 = own.raw0;
    int32_t& slot_next = own.slot_next;
    const int lane = threadIdx.x & 63;
    const int r = d.r, c0 = d.c0, ncr = d.ncr, job_n_tab = a.job.n_tab;
    const int32_t L = d.L, P = d.P, win_begin = d.win_begin;
    const int my_ins_idx = own.my_ins_idx;
    const int32_t my_ins_off = own.my_ins_off;
    const double ln_quarter = fa.tab->ln_quarter, ln_noncand = fa.tab->ln_noncand; // (asked for here, looked at by the sums)
    {
        const int j0 = 64 * j;
        const int nc = min(64, ncr - j0);
        f5_wave_sync(); // (pool and read complete; the previous round's slots read; the order written)
        const unsigned long long ta = now();
        if (mine && j0 == 0) stamp[1] = ta; // prologue done
        // ---- the round's records, a lane its own: header + F5_SEGS path segments (five 16-byte loads) + F5_INDELS indel indices, all in
        // flight at once; a record with more of either is left to the staged chain
        const bool has = lane < nc;
        uint32_t* const myslot = slots + lane * F5_SLOT;
        const bool whole_tab = job_n_tab <= F5_TAB; // (a helper's read is of such a job: only those are published)
        bool fits = true;
        const int my_j = has ? f5_list_index(S, d, j0 + lane) - c0 : 0; // the lane's alignment among the read's
        F5Rec rec;
        rec.w0 = rec.w1 = rec.w2 = 0;
        rec.types = 0;
        rec.l0 = rec.l1 = rec.l2 = rec.l3 = 0;
        rec.ind = 0;
        rec.ind_lo = 0;
        uint64_t ind_raw0 = 0, ind_raw1 = 0; // the record's eight 16-bit indel indices, until the round's table copy is placed
        if (!mine || j0 > 0) raw0 = f5_load_raw(a.pool + slot_next);
        if (has) {
            const F5Raw w = raw0;
            const uint4 q0 = w.q0, q1 = w.q1, q2 = w.q2, q3 = w.q3, q4 = w.q4;
            ind_raw0 = uint64_t(w.i0) | (uint64_t(w.i1) << 32);
            ind_raw1 = uint64_t(w.i2) | (uint64_t(w.i3) << 32);
            rec.w0 = q0.x;
            rec.w1 = q0.y;
            rec.w2 = q0.z;
            const unsigned nseg = (q0.z >> 8) & 0xffu, nind = (q0.z >> 16) & 0xffu;
            fits = (nseg <= unsigned(F5_SEGS) && nind <= unsigned(F5_INDELS));
            uint64_t types = 0;
            bool odd_type = false; // (not a segment type: the staged chain reports it)
            auto pack4 = [&](const uint32_t a0, const uint32_t a1, const uint32_t a2, const uint32_t a3, const int first) -> uint64_t {
                types |= (uint64_t(a0 & 15u) | (uint64_t(a1 & 15u) << 4) | (uint64_t(a2 & 15u) << 8) | (uint64_t(a3 & 15u) << 12)) << (4 * first);
                odd_type = odd_type || (unsigned(first) < nseg && (a0 & 0xffffu) > 15u) || (unsigned(first + 1) < nseg && (a1 & 0xffffu) > 15u) ||
                           (unsigned(first + 2) < nseg && (a2 & 0xffffu) > 15u) || (unsigned(first + 3) < nseg && (a3 & 0xffffu) > 15u);
                return uint64_t(a0 >> 16) | (uint64_t(a1 >> 16) << 16) | (uint64_t(a2 >> 16) << 32) | (uint64_t(a3 >> 16) << 48);
            };
            rec.l0 = pack4(q0.w, q1.x, q1.y, q1.z, 0);
            rec.l1 = pack4(q1.w, q2.x, q2.y, q2.z, 4);
            rec.l2 = pack4(q2.w, q3.x, q3.y, q3.z, 8);
            rec.l3 = pack4(q3.w, q4.x, q4.y, q4.z, 12);
            rec.types = types;
            fits = fits && !odd_type;
        }
        // the table entries this round's alignments name
        auto raw_indel = [&](const int k) -> int { return int(int16_t(((k & 4) ? ind_raw1 : ind_raw0) >> (16 * (k & 3)))); };
        int tab_lo = 0;
        if (whole_tab) {
            // the prologue's copy holds the job's table: tab_lo = 0, nothing to place per round
            bool out_of_table = false;
            if (has && fits) {
                auto check = [&](const int i) { out_of_table = out_of_table || i < 0 || i >= job_n_tab; };
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) check(raw_indel(i));
                if (rec.lead() >= 0) check(rec.lead());
                if (rec.trail() >= 0) check(rec.trail());
            }
            // (a record beyond the compact form, an index that is none of the table's: the staged chain takes the job)
            if (__any((has && !fits) || out_of_table)) {
                if (lane == 0) {
                    atomicAdd(fa.n_unhandled, 1);
                    if (j > 0) atomicAdd(fa.shared_rounds + 1, 1u); // (diagnostics: a round after the read's first turned it down)
                }
                return false;
            }
            uint64_t ind = 0;
#pragma unroll
            for (int k = 0; k < F5_INDELS; ++k) ind |= uint64_t(unsigned(raw_indel(k)) & 63u) << (6 * k);
            rec.ind = ind;
            rec.ind_lo = 0;
        } else {
            int lo = INT_MAX, hi = INT_MIN;
            if (has && fits) {
                auto add = [&](const int i) {
                    lo = min(lo, i);
                    hi = max(hi, i);
                };
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) add(raw_indel(i));
                if (rec.lead() >= 0) add(rec.lead());
                if (rec.trail() >= 0) add(rec.trail());
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                lo = min(lo, __shfl_xor(lo, d));
                hi = max(hi, __shfl_xor(hi, d));
            }
            const int n_tab = (lo <= hi) ? hi - lo + 1 : 0;
            // (a record beyond the compact form, indices further apart than the copy holds: the staged chain takes the job)
            if (__any(has && !fits) || (n_tab > 0 && lo < 0) || n_tab > F5_TAB) {
                if (lane == 0) {
                    atomicAdd(fa.n_unhandled, 1);
                    if (j > 0) atomicAdd(fa.shared_rounds + 1, 1u); // (diagnostics: a round after the read's first turned it down)
                }
                return false;
            }
            tab_lo = n_tab ? lo : 0;
            // (every index of the round's records lies in [tab_lo, tab_lo + n_tab), n_tab <= F5_TAB: 6 bits relative to tab_lo)
            uint64_t ind = 0;
#pragma unroll
            for (int k = 0; k < F5_INDELS; ++k) ind |= uint64_t(unsigned(raw_indel(k) - tab_lo) & 63u) << (6 * k);
            rec.ind = ind;
            rec.ind_lo = tab_lo;
            if (lane < n_tab) { // (n_tab <= F5_TAB <= 32: a lane an entry)
                const PIndel& g = a.job.tab[tab_lo + lane];
                F5Tab e;
                e.pos = g.pos;
                e.del = g.del;
                e.ins_len = g.ins_len;
                e.type_cand = unsigned(g.type) | (unsigned(g.cand) << 8);
                e.ins_at = -1;
                S.tab[lane] = e;
            }
            f5_wave_sync();
            // (the read's inserts are distinct table indices, pool_layout_kernel: a lane an insert, no two write the same entry)
            if (my_ins_idx >= tab_lo && my_ins_idx < tab_lo + n_tab) S.tab[my_ins_idx - tab_lo].ins_at = my_ins_off;
        }
        f5_wave_sync();
        const unsigned long long tc = now();
        stamp[2] += tc - ta; // staging + table copy
        // ---- phase A, a lane per candidate alignment: the walk of its path leaves the alignment's TRANSITIONS in its slot: one word per
        // op that covers read positions, and one for the read's end
        int n_ent = 0;
        bool bad = false;
        bool cons_mine = false;
        uint8_t cons_seen = 1;
        {
            const unsigned long long tA0 = now();
            uint32_t cons = 0; // the table entries whose candidate status this lane's alignment consults: bit index - tab_lo
            n_ent = f5_walk_selects(S, rec, has, tab_lo, win_begin, cons, L, P, myslot);
            const unsigned long long tA1 = now();
            stamp[7] += tA1 - tA0; // the walk
            bad = n_ent < 0;
            if (has) {
                // the candidate-status lookups the host form performs for every indel of the alignment (cal_to_c)
                const int ni = rec.n_indels();
                for (int i = 0; i < ni; ++i) cons |= 1u << ((rec.indel(i) - tab_lo) & 31);
                if (rec.lead() >= 0) cons |= 1u << ((rec.lead() - tab_lo) & 31);
                if (rec.trail() >= 0) cons |= 1u << ((rec.trail() - tab_lo) & 31);
                if (bad) a.status[r] = ST_FAIL;
            }
            // the round's entries: one OR over the wave, lane t looks at entry tab_lo + t and marks it where it reads 0 (a stale 0 costs a
            // store of the 1 that is there already) -- a byte store per lane per indel stood in front of the next round's record loads
            if (a.job.consulted) {
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) cons |= uint32_t(__shfl_xor(int(cons), d));
                cons_mine = lane < 32 && ((cons >> lane) & 1u) != 0u;
                if (cons_mine) cons_seen = a.job.consulted[tab_lo + lane];
            }
            (void)tA1;
        }
        // (the owner's next round, named before the sums: its list[] entries travel while they run)
        j_next = mine ? next_j() : -1;
        if (j_next >= 0 && 64 * j_next + lane < ncr) slot_next = a.list[f5_list_index(S, d, 64 * j_next + lane)];
        __builtin_amdgcn_wave_barrier();
        const unsigned long long td = now();
        stamp[4] += td - tc; // phase A
        // ---- phase B, a lane its alignment: the terms in path order (f5_sum)
        if (has && !bad) {
            const double lnp = f5_sum(S, myslot, n_ent, ln_noncand, ln_quarter);
            fa.scores[c0 + my_j] = lnp;
        }
        if (cons_mine && cons_seen == 0) a.job.consulted[tab_lo + lane] = 1;
        // (the record's registers are the next round's to load: nothing of them lives through the walk and the sums)
        raw0.q0 = raw0.q1 = raw0.q2 = raw0.q3 = raw0.q4 = make_uint4(0, 0, 0, 0);
        raw0.i0 = raw0.i1 = raw0.i2 = raw0.i3 = 0;
        stamp[5] += now() - td; // phase B
        if (mine) stamp[10] += 1; // (rounds the owner scored itself)
    }
    return true;
}

// $SK_F5_TIMING: the owner's last rounds are over -- the read's stamps go out (a round a helper still runs ends later: the stamps
// are the owner's time on the read)
template <bool TIMING>
__device__ __forceinline__ void f5_store_stamps(const FusedScoreArgs& fa, const int r, F5Own& own, const unsigned long long draw_cycles)
{
    if (TIMING && fa.dbg && (threadIdx.x & 63) == 0) { // (the build without the stamps has no store of them either)
        unsigned long long(&stamp)[F5_STAMPS] = own.stamp;
        stamp[6] = (unsigned long long)clock64();
        stamp[3] = (unsigned long long)wall_clock64() - own.wall0;
        stamp[8] = draw_cycles; // the draw that handed this read out, from before the atomic to its value in a scalar register (0: the
                                // wave's first read, which is not drawn)
        stamp[9] = own.wall0;
        for (int i = 0; i < F5_STAMPS; ++i) fa.dbg[size_t(r) * F5_STAMPS + i] = stamp[i];
    }
}

// A wave per read, WAVES waves to a block (each wave with an LDS object of its own, which it alone writes; at the launch's end a
// block-mate may read it: ROUND SHARING below).  With a block per
// read the kernel was bound by the rate at which the dispatcher places workgroups (65 536 one-wave blocks went out at ~30 per us, a block
// lives ~58 us: ~7 of a CU's 16 slots filled); eight waves to a block: 2.23 -> 1.67 ms per 65 536 reads (profiles/r05_f5_history.txt).
// The waves TAKE their reads from a queue (one counter, one atomic per read; a grid of the blocks the device holds at a time).  With read r
// bound to wave r a block lived as long as its heaviest read -- a read's work goes with its candidate alignments, a round of the wave per
// 64 -- and its other seven slots stood empty meanwhile: 7.5 waves to a CU on average (SQ_WAVE_CYCLES, profiles/r06_v28_pmc_traffic.json)
// where two such blocks, 16 waves, are resident (tools/diag/lds_residency.hip).  1.67 -> 1.23 ms.  Round 5's persistent grid (reads r, r + 4 096, ... to wave r: slower) had the
// same binding, only longer.  The queue's order is the job's: taking the heavy reads first, or the light ones last (lists by rounds of 64
// candidate alignments, filled by pool_layout_kernel), was tried against the launch's tail and is SLOWER (1.33-1.37 ms: reads of one kind
// side by side keep their waves in step -- all in their prologues, all in their walks -- where the job's own order mixes them;
// profiles/r06_f5_history.txt).  A wave's FIRST read is not drawn: wave g of the grid takes read g, and a draw hands out
// gridDim.x * WAVES + the counter's value.  All the grid's waves used to make their first draw on the one word within the ~15 us it takes
// to place the blocks, and a head word answers ~88 such atomics per us: the last of that burst waited ~45 us for its first read
// (1.025 -> 0.981 ms, profiles/r09_f5_history.txt; a later draw costs a wave 3 700 - 4 600 cycles at this load, the `draw` figure of
// $SK_F5_TIMING).  What is handed out is a number h; it names read h except among the launch's last hand-outs, whose reads are taken
// from a table in which the reads of several rounds stand earlier than in the job (tail_order_kernel, below).  A wave whose number is
// past the last read makes no draw.  The last wave to leave puts the queue back to zero -- every wave counts itself out after
// its last draw, whether it drew or not -- so that the next launch, the same buffers, the same stream, finds it as this one did.
//
// ROUND SHARING.  The launch used to end a heavy read's life after its last hand-out (~135 us of ~0.92 ms, profiles/r10_f5_history.txt): a
// read of three or four rounds drawn late keeps one wave busy while its block-mates have left.  Now a wave that has drawn DRY does not
// leave: it takes whole rounds of reads owned by waves of its own block.  The owner's prologue has left the read, the pool, the order, the
// rows of terms and the table copy in its LDS object, which nothing writes again before the owner's next prologue; the helper reads them
// where they lie and writes its own slots, so no second prologue runs and nothing but the round's own records is read from HBM.
//   publication  A read of more than one round in a job whose table fits the copy (whole_tab: else the table copy is written per round
//                and the read is not shared) is published after the prologue's last LDS write: a workgroup release fence by every
//                lane (each wrote part of the data), then lane 0's descriptor stores, its release fence, and one atomic store of
//                the wave's claim word {next round = 1 | rounds << 16}.
//   claims       A round is claimed by an LDS atomic add of 1 on the claim word; the old value names the round if its low half is below
//                the high half.  The owner claims the same way, between a round's walk and its sums (list[] of its next round
//                travels behind the sums, as before); round 0 is always its own (its records are asked for in the prologue, and the
//                list[] entries parked in its slots die with its first walk).  A helper reads the word first and adds only where a
//                round is open, so a word over-counts by at most the block's waves (rounds < 2^15: the halves do not meet).  After a
//                claim the helper makes an acquire fence, reads the descriptor, asks for list[] of the round and then its records.
//   helpers      `busy` counts the block's waves that have not drawn dry.  A dry wave polls its block-mates' claim words -- never its
//                own -- with s_sleep F5_HELP_NAP between looks, and leaves when busy == 0 (an owner draws dry only after every round
//                of its read is claimed, or its word is closed: nothing is open then) or F5_HELP_CAP ticks of the constant 100 MHz
//                counter (20 ms) after it drew dry.
//   closing      A word is open only while its read is the one in the owner's LDS object.  A read that goes through uses its word
//                up (the owner's last claim finds no round left).  An owner that leaves a published read EARLY -- a round of its
//                own turned the read down -- stores 0 into its word before it draws: left open, the word would outlive a draw
//                that hands out a read, and a wave that drew dry later would score the dead read's rounds over the new read's data.
// NO WAVE EVER WAITS FOR ANOTHER TO DO SOMETHING.  An owner does not wait for helpers: it claims until its word is used up, scores what
// it claimed, and goes on to draw.  A helper may leave at any moment: what nobody claimed the owner scores.  A helper's reads of an
// owner's LDS object are safe without any wait, because the queue's counter only grows: once any wave of the launch has drawn dry
// (n_waves + counter >= n_reads; a wave whose own number is past the last read implies n_waves >= n_reads), every later draw is dry
// too -- the helper's dry draw returned before it claimed, the owner's next draw is issued after its own last claim or after it closed
// its word -- so an owner never runs another prologue while a helper that claimed from its word can be reading its object, and after
// that draw the word gives nothing out; and a block's LDS lives until its last wave leaves, after the helper.  There is no waiting across blocks, no barrier after the first, no spin without the cap.  What ends a round early (a
// record outside the compact form: *n_unhandled, which the drivers test for > 0) or marks the read (ST_FAIL) a helper records as the
// owner would, and goes on polling.  Rounds a helper SCORED (not those it was turned down in) are counted in *shared_rounds, one
// atomic each (the tail pays it).
// $SK_F5_SHARE=0 (FusedScoreArgs::share = 0): nothing is published, a dry wave leaves at once, the kernel runs as it did.
constexpr int F5_HELP_NAP = 64; // s_sleep between a dry wave's looks: ~4 000 cycles, under 2 us -- a fifth of a round
constexpr unsigned F5_HELP_CAP = 2000000u; // ticks of the 100 MHz counter a dry wave stays at most: 20 ms
template <int MAXR, bool TIMING, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4, 4))) void flatten_score_kernel(const FusedScoreArgs fa, const int n_reads)
{
    __shared__ __attribute__((aligned(16))) F5Lds<MAXR> S[WAVES];
    // the two terms of every quality, once per block (every wave reaches the barrier: it stands before the first draw)
    __shared__ double q_terms[F5_Q_TERMS];
    __shared__ F5Share share[WAVES];
    __shared__ unsigned busy;
    for (int i = threadIdx.x; i < F5_Q_TERMS; i += 64 * WAVES) q_terms[i] = (i <= SK_NQ) ? fa.tab->q2lncompe[i] : fa.tab->q2mis[i - (SK_NQ + 1)];
    if (threadIdx.x < unsigned(WAVES)) share[threadIdx.x].claim = 0u, share[threadIdx.x].dry_at = 0u; // (nothing open, nobody dry)
    if (threadIdx.x == 0) busy = unsigned(WAVES);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned n_waves = gridDim.x * unsigned(WAVES);
    // a read of `ncr` candidate alignments is published: sharing is on, the job's table fits the copy, more than one round
    auto published = [&](const int ncr) -> bool { return WAVES > 1 && fa.share != 0 && fa.f.job.n_tab <= F5_TAB && ncr > 64 && ncr < (0x8000 << 6); };
    // the first hand-out: the wave's own number, no draw
    unsigned h = unsigned(__builtin_amdgcn_readfirstlane(int(blockIdx.x * unsigned(WAVES) + unsigned(wave))));
    unsigned long long draw_cycles = 0;
    auto draw = [&]() {
        f5_wave_sync(); // (the wave's LDS object is the next read's)
        const unsigned long long t0 = TIMING ? (unsigned long long)clock64() : 0ull;
        unsigned got = 0;
        if (lane == 0) got = atomicAdd(&fa.queue[0], 1u);
        int drawn = __builtin_amdgcn_readfirstlane(int(got));
        if (TIMING) __asm__ volatile("" : "+s"(drawn)); // (the second stamp stands after the value has arrived)
        h = n_waves + unsigned(drawn);
        draw_cycles = TIMING ? (unsigned long long)clock64() - t0 : 0ull;
    };
    F5Desc d; // the read whose round comes next: the wave's own, or a block-mate's
    F5Own own;
    d.r = d.c0 = d.ncr = d.L = d.P = d.win_begin = d.sorted_order = 0;
    int j = -1, src = wave; // the round to run (-1: none); the wave whose LDS object holds the read (the wave's own: it is the owner)
    for (;;) {
        if (j < 0 && h < unsigned(n_reads)) { // ---- the owner's next read
            // hand-out h is read h, except among the launch's last tail_n hand-outs, which go through the table (the same for the whole
            // wave; one more dependent load, paid by those hand-outs only)
            unsigned r = h;
            if (h - fa.tail_first < fa.tail_n) r = unsigned(__builtin_amdgcn_readfirstlane(fa.tail_order[h - fa.tail_first]));
            if (!f5_prologue<MAXR, TIMING>(fa, int(r), S[wave], q_terms, d, own)) {
                draw();
                continue;
            }
            j = 0;
            if (published(d.ncr)) {
                // (every lane wrote part of the prologue's data: every lane releases its stores, before lane 0 alone writes the
                // descriptor and, behind a release of its own, the word)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) {
                    share[wave].d = d;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __hip_atomic_store(&share[wave].claim, 1u | (unsigned((d.ncr + 63) >> 6) << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        } else if (j < 0) { // ---- a dry wave (h is past the last read and stays there: no further draw): a round of a block-mate's read
            // (when it drew dry is kept in LDS, and the lane is taken anew: neither is a register's through the owners' rounds)
            unsigned dry_at = unsigned(__builtin_amdgcn_readfirstlane(int(share[wave].dry_at)));
            if (dry_at == 0u) {
                if (lane == 0) __hip_atomic_fetch_add(&busy, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (!(WAVES > 1 && fa.share != 0)) break;
                dry_at = unsigned(wall_clock64()) | 1u;
                if (lane == 0) share[wave].dry_at = dry_at;
            }
            int look = threadIdx.x & 63;
            __asm__ volatile("" : "+v"(look));
            unsigned w = 0;
            if (look < WAVES && look != wave) w = __hip_atomic_load(&share[look].claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // (never its own)
            const unsigned long long open = __ballot((w & 0xffffu) < (w >> 16));
            if (open == 0ull) {
                const unsigned left = __hip_atomic_load(&busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (__builtin_amdgcn_readfirstlane(int(left)) == 0 || unsigned(wall_clock64()) - dry_at > F5_HELP_CAP) break;
                __builtin_amdgcn_s_sleep(F5_HELP_NAP);
                continue;
            }
            const int o = __builtin_amdgcn_readfirstlane(__builtin_ctzll(open)); // (< WAVES: only those lanes looked)
            unsigned old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(&share[o].claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            old = unsigned(__builtin_amdgcn_readfirstlane(int(old)));
            if ((old & 0xffffu) >= (old >> 16)) continue; // (taken meanwhile: look again)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const F5Desc& p = share[o].d;
            d.r = __builtin_amdgcn_readfirstlane(p.r), d.c0 = __builtin_amdgcn_readfirstlane(p.c0), d.ncr = __builtin_amdgcn_readfirstlane(p.ncr);
            d.L = __builtin_amdgcn_readfirstlane(p.L), d.P = __builtin_amdgcn_readfirstlane(p.P);
            d.win_begin = __builtin_amdgcn_readfirstlane(p.win_begin), d.sorted_order = __builtin_amdgcn_readfirstlane(p.sorted_order);
            j = int(old & 0xffffu), src = o;
            // (what the owner gets a round ahead: list[] of the round; a lane without an alignment names record 0, which nothing looks at)
            own.slot_next = (64 * j + lane < d.ncr) ? fa.f.list[f5_list_index(S[src], d, 64 * j + lane)] : 0;
            own.my_ins_idx = -1, own.my_ins_off = 0;
        }
        const bool mine = src == wave;
        int j_next = -1;
        const bool went = f5_round<MAXR, TIMING>(
            fa, S[src], S[wave].slot, d, j, mine, own,
            [&]() -> int { // the owner's next round: the one after this, or, of a published read, the next that nobody has claimed
                int nj = j + 1;
                if (published(d.ncr)) {
                    unsigned old = 0;
                    if (lane == 0) old = __hip_atomic_fetch_add(&share[wave].claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    nj = __builtin_amdgcn_readfirstlane(int(old)) & 0xffff;
                }
                return 64 * nj < d.ncr ? nj : -1;
            },
            j_next);
        if (!mine && went && lane == 0) atomicAdd(fa.shared_rounds, 1u); // (a helped round that was scored)
        j = (mine && went) ? j_next : -1;
        if (mine && j < 0) { // (the owner's last round, or the round that left the read to the staged chain)
            if (went) f5_store_stamps<TIMING>(fa, d.r, own, draw_cycles);
            // The owner leaves a published read EARLY: it closes its word before it draws.  A round claimed before the store is a
            // helper's, and a helper has drawn dry, so the draw below is dry too (the argument above); after the store nothing can be
            // claimed, and if the draw hands out a read, its prologue writes an object that no word points at.  (A read that went
            // through needs no store: its word is used up, the owner's last claim found it so.)
            else if (published(d.ncr) && lane == 0) __hip_atomic_store(&share[wave].claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            draw();
        }
    }
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(&fa.queue[1], 1u) == gridDim.x * unsigned(WAVES) - 1u) { // (every wave has made its last draw)
            fa.queue[0] = 0u;
            fa.queue[1] = 0u;
        }
    }
}

// the rows of terms sized for the job's longest read: with 150-base reads a wave's LDS is 10 KB, sixteen waves to a CU (the 256-base
// form: twelve)
// eight waves to a block where their LDS leaves room for two blocks to a CU (the short-read form: 76.7 KB), four with the long form
// the launch's shape, computed in one place for the launch and for the table of its last hand-outs: the waves of a block and the
// blocks of the grid.  waves() is W, the reads handed out without a draw.
struct F5Grid
{
    int wpb, blocks;
    int waves() const { return wpb * blocks; }
};
template <int MAXR>
static F5Grid f5_grid_t(const int n_reads)
{
    static const int waves = [] { const char* e = std::getenv("SK_F5_WAVES"); return e ? std::atoi(e) : 0; }(); // (experiments: 1, 2, 4, 8, 16; 0 = the default)
    constexpr int DEFAULT_WAVES = (sizeof(F5Lds<MAXR>) * 16 <= 160 * 1024) ? 8 : 4;
    const int w = waves > 0 ? waves : DEFAULT_WAVES;
    const int wpb = (w == 16 && MAXR <= 152) ? 16 : w >= 8 ? 8 : w == 4 ? 4 : w == 2 ? 2 : 1; // (the instantiations there are)
    // the blocks the device holds at a time (256 CUs; by LDS: 16 waves of the short-read form to a CU, 14 of the long one; a grid larger
    // than that only queues blocks that find the read queue empty, a smaller one leaves slots unused): $SK_F5_GRID = blocks, experiments
    static const int grid_env = [] { const char* e = std::getenv("SK_F5_GRID"); return e ? std::atoi(e) : 0; }();
    constexpr int WAVES_PER_CU = int((160 * 1024) / sizeof(F5Lds<MAXR>)) >= 16 ? 16 : int((160 * 1024) / sizeof(F5Lds<MAXR>));
    const int resident = grid_env > 0 ? grid_env : 256 * std::max(1, WAVES_PER_CU / wpb);
    return { wpb, std::max(1, std::min(resident, (n_reads + wpb - 1) / wpb)) };
}
static F5Grid f5_grid(const int n_reads, const int max_read_len) // (the form launch_flatten_score takes for the job)
{
    return max_read_len <= 152 ? f5_grid_t<152>(n_reads) : f5_grid_t<F5_MAX_READ>(n_reads);
}

template <int MAXR, bool TIMING>
static void launch_flatten_score_t(const int n_reads, hipStream_t st, const FusedScoreArgs& fs)
{
    const F5Grid g = f5_grid_t<MAXR>(n_reads);
    const dim3 grid(unsigned(g.blocks)), block(unsigned(64 * g.wpb));
    if (g.wpb == 16) SK_LAUNCH((flatten_score_kernel<152, TIMING, 16>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 8) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 8>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 4) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 4>), grid, block, 0, st, fs, n_reads);
    else if (g.wpb == 2) SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 2>), grid, block, 0, st, fs, n_reads);
    else SK_LAUNCH((flatten_score_kernel<MAXR, TIMING, 1>), grid, block, 0, st, fs, n_reads);
}

// ---- the order of the launch's last hand-outs.  A read makes a round per 64 candidate alignments, and a read of four rounds drawn just
// before the queue runs dry holds the launch open for its whole life while the other waves leave.  The job's order stays as it is (it
// mixes the kinds of reads: see above) except in a window of the last T = min(n_reads, W + 6 s) hand-outs, W the grid's waves: there a
// read of c rounds (1-5; a read without candidate alignments counts as 1) moves up by (c - 1) s places -- window position i gets the
// key i - (c - 1) s, and the window is put in ascending key order, ties to the lower position.  Each kind keeps its own order, nothing
// is clumped at the launch's start, and the launch's last hand-outs are one-round reads where the window holds enough of them.  No
// sort is needed: a position's place is the number of positions before it in that order, a sum over the five kinds of counts below an
// index -- kind q's positions j with j < i + (q - c) s, and j = i + (q - c) s too where q < c.  A block per 1 024 positions.  EVERY block
// reads the kinds of the whole window (4 bytes a read, a wave 64 consecutive positions, eight loads in flight) and keeps them in LDS as
// one 64-bit mask per kind 2-5 and 64 positions (kind 1 is the rest), with the kinds' counts before each 64 positions from one
// block-wide scan of two packed values; a count below an index is then a scan entry plus a population count, and a position looks its
// five up without leaving the CU.  (As one block that kept the counts per position in HBM the kernel took 77 us for 16 384 positions,
// a fifth of F5's time on a job of that size: profiles/r10_f5_history.txt.)  No atomics: the table is the same on every run.
constexpr int F5_TAIL_KINDS = 5;
constexpr int F5_TAIL_MAX = 65536; // positions of a window: what tail_order_kernel's LDS holds (a larger shift is cut down to fit)
struct TailArgs
{
    const int32_t* cal_off; // [n_reads + 1]
    int32_t first, n;       // the window: hand-outs [first, first + n), n <= F5_TAIL_MAX
    int32_t shift;          // s
    int32_t* order;         // [n] the table: the read of hand-out first + k
};
__global__ __launch_bounds__(1024) void tail_order_kernel(const TailArgs a)
{
    constexpr int MAX_CHUNKS = F5_TAIL_MAX / 64, AHEAD = 8;
    __shared__ unsigned long long mask[MAX_CHUNKS + 1][F5_TAIL_KINDS - 1]; // [chunk][q - 2]: the chunk's positions of kind q
    __shared__ uint4 before[MAX_CHUNKS + 1];                               // the positions of kind 2, 3, 4, 5 before the chunk
    __shared__ unsigned long long wave_sums[17];
    const int T = a.n, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_chunks = (T + 63) >> 6; // (<= 1 024: a thread a chunk in the scan)
    for (int c0 = wave; c0 < n_chunks; c0 += 16 * AHEAD) {
        int lo[AHEAD], hi[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int i = (c0 + 16 * u) * 64 + lane;
            lo[u] = i < T ? a.cal_off[a.first + i] : 0;
            hi[u] = i < T ? a.cal_off[a.first + i + 1] : 0;
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int chunk = c0 + 16 * u; // (the same for the wave)
            if (chunk >= n_chunks) break;
            const int kind = (chunk * 64 + lane < T) ? min(max((hi[u] - lo[u] + 63) >> 6, 1), F5_TAIL_KINDS) : 0;
#pragma unroll
            for (int q = 2; q <= F5_TAIL_KINDS; ++q) {
                const unsigned long long m = __ballot(kind == q);
                if (lane == 0) mask[chunk][q - 2] = m;
            }
        }
    }
    if (t < F5_TAIL_KINDS - 1) mask[n_chunks][t] = 0; // (an index of T itself, where T is a multiple of 64)
    __syncthreads();
    unsigned cnt[F5_TAIL_KINDS - 1] = { 0, 0, 0, 0 };
    if (t < n_chunks) {
#pragma unroll
        for (int q = 0; q < F5_TAIL_KINDS - 1; ++q) cnt[q] = unsigned(__popcll(mask[t][q]));
    }
    unsigned long long tot23 = 0, tot45 = 0;
    const unsigned long long at23 = block_exclusive_scan<unsigned long long>(cnt[0] | (unsigned long long)cnt[1] << 32, wave_sums, &tot23);
    const unsigned long long at45 = block_exclusive_scan<unsigned long long>(cnt[2] | (unsigned long long)cnt[3] << 32, wave_sums, &tot45);
    if (t < n_chunks) before[t] = make_uint4(unsigned(at23), unsigned(at23 >> 32), unsigned(at45), unsigned(at45 >> 32));
    if (t == 0) before[n_chunks] = make_uint4(unsigned(tot23), unsigned(tot23 >> 32), unsigned(tot45), unsigned(tot45 >> 32));
    __syncthreads();
    for (int i = blockIdx.x * 1024 + t; i < T; i += gridDim.x * 1024) {
        int c = 1;
#pragma unroll
        for (int q = 2; q <= F5_TAIL_KINDS; ++q)
            if ((mask[i >> 6][q - 2] >> (i & 63)) & 1ull) c = q;
        int place = 0;
#pragma unroll
        for (int q = 1; q <= F5_TAIL_KINDS; ++q) {
            const long long x = (long long)i + (long long)(q - c) * a.shift + (q < c ? 1 : 0);
            const int below = int(min(max(x, 0ll), (long long)T)); // kind q's positions [0, below) come before position i
            const uint4 p = before[below >> 6];
            const unsigned long long bits = (1ull << (below & 63)) - 1ull;
            const unsigned long long* const m = mask[below >> 6];
            const unsigned n2 = p.x + unsigned(__popcll(m[0] & bits)), n3 = p.y + unsigned(__popcll(m[1] & bits));
            const unsigned n4 = p.z + unsigned(__popcll(m[2] & bits)), n5 = p.w + unsigned(__popcll(m[3] & bits));
            place += int(q == 1 ? unsigned(below) - (n2 + n3 + n4 + n5) : q == 2 ? n2 : q == 3 ? n3 : q == 4 ? n4 : n5);
        }
        if (unsigned(place) < unsigned(T)) a.order[place] = a.first + i; // (a position's place is its own: the order is total)
    }
}
static void launch_tail_order(hipStream_t st, const TailArgs& ta) { SK_LAUNCH(tail_order_kernel, dim3(unsigned(ta.n + 1023) / 1024), dim3(1024), 0, st, ta); }
// $SK_F5_TAIL_SHIFT = s in hand-outs (experiments and tests; 0 = the job's own order to the end); the default is the grid's waves: of W / 4,
// W / 2, W, 1.5 W, 2 W and 2.5 W it is the fastest on a job of 65 536 reads and on one of 16 384 (profiles/r10_f5_history.txt: the
// launch gets shorter up to W and longer again beyond it, as more of the job is put in order of work).  Cut down so that the window fits
// the table kernel.
static int f5_tail_shift(const int W)
{
    static const int env = [] { const char* e = std::getenv("SK_F5_TAIL_SHIFT"); return e ? std::max(0, std::atoi(e)) : -1; }();
    return std::min(env >= 0 ? env : W, std::max(0, (F5_TAIL_MAX - W) / 6));
}
// the window for a launch over n_reads with W waves: its length T (0: the launch draws nothing, or the shift is off -- no table)
static int f5_tail_window(const int n_reads, const int W, const int shift)
{
    if (n_reads <= W || shift <= 0) return 0;
    return int(std::min<int64_t>(n_reads, int64_t(W) + 6 * int64_t(shift)));
}

static void launch_flatten_score(const int n_reads, hipStream_t st, const FusedScoreArgs& fs)
{
    const bool short_reads = fs.f.max_read_len <= 152, timing = fs.dbg != nullptr;
    if (short_reads && !timing) launch_flatten_score_t<152, false>(n_reads, st, fs);
    else if (short_reads) launch_flatten_score_t<152, true>(n_reads, st, fs);
    else if (!timing) launch_flatten_score_t<F5_MAX_READ, false>(n_reads, st, fs);
    else launch_flatten_score_t<F5_MAX_READ, true>(n_reads, st, fs);
}

// the records in set order, for the host (sk_enum_device_fetch_cals; a job whose stage 3 runs on the host): pool[list[c]] -> cals[c], a wave
// per 64 records, rows of consecutive dwords
__global__ __launch_bounds__(64) void gather_cals_kernel(const PCal* __restrict__ pool, const int32_t* __restrict__ list, const int32_t n_cals,
                                                         PCal* __restrict__ cals)
{
    constexpr int REC_DW = int(sizeof(PCal) / 4);
    const int lane = threadIdx.x;
    const int c0 = blockIdx.x * 64;
    const int nc = min(64, n_cals - c0);
    const int src_k = (lane < nc) ? list[c0 + lane] : 0;
    for (int k0 = 0; k0 < nc; k0 += 16) {
        uint32_t v0[16], v1[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = k0 + u;
            const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(pool + __shfl(src_k, (k < nc) ? k : 0));
            v0[u] = (k < nc) ? src[lane] : 0u;
            v1[u] = (k < nc && lane + 64 < REC_DW) ? src[lane + 64] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = k0 + u;
            if (k < nc) {
                uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(cals + (c0 + k));
                dst[lane] = v0[u];
                if (lane + 64 < REC_DW) dst[lane + 64] = v1[u];
            }
        }
    }
}

// F3: ops -> transition entries + the read's event mask (host form: align_prepare in host/align_flatten.cpp; layout
// csrc/align_entry.h), then the column form (host form: sk_align_prepare_cols).  Two kernels produce the same bytes:
//   entries_kernel       one THREAD per candidate alignment walks its ops and then every read position (a dependent byte load of
//                        the haplotype pool per position);
//   entries_wave_kernel  one WAVE per read: the lanes emit the entries of their candidate alignments, the base comparisons are
//                        made once per distinct (haplotype offset, read position) -- a read's candidates face the pool at a
//                        handful of offsets, one per combination of indels before a position -- as packed 8-position words in
//                        LDS, and a lane assembles its alignment's column words from those with masks.

// the entries of candidate alignment c (slots ent[0 .. nslots)); returns true if the alignment is left to the generic routine
// ("complex"), in which case its column words stay as preset.  `hap`: the read's pool (P bytes).  n_ent: entries written.
__device__ inline bool f3_emit_entries(const FlatArgs& a, const int c, const int r, const uint8_t* hap, const int32_t L, const int32_t P,
                                       uint32_t* ent, int& n_ent)
{
    const int W = a.evmask_words;
    uint32_t* mask = a.evmask + int64_t(r) * W;
    const bool read_ok = (L >= 0 && L <= SK_ENT_MAX_READ_LEN && L <= a.max_read_len && P >= 0 && P <= SK_ENT_MAX_POOL);
    auto col_at = [&](const int idx) -> unsigned { return (idx >= 0 && idx < P) ? sk_ent_col_index(hap[idx]) : unsigned(SK_ENT_ZERO_COL); };
    const int64_t k0 = a.op_off[c], k1 = a.op_off[c + 1];
    const int nslots = int(k1 - k0) + 2;
    for (int i = 0; i < nslots; ++i) ent[i] = SK_ENT_END;
    bool complex_cal = !read_ok;
    int e = 0, pos = 0;
    unsigned npen = 0;
    auto emit = [&](const unsigned np, const bool clip, const int hidx) {
        if (np > 7u || hidx + SK_ENT_HIDX_BIAS < 0 || hidx + SK_ENT_HIDX_BIAS > 2047) complex_cal = true;
        if (complex_cal) return;
        ent[e++] = unsigned(pos) | (np << 10) | (clip ? 1u << 13 : 0u) | (col_at(hidx + pos) << 15) | (col_at(hidx + pos + 1) << 18) |
                   (unsigned(hidx + SK_ENT_HIDX_BIAS) << 21);
        if (pos > 0 && pos <= L) atomicOr(&mask[pos >> 5], 1u << (pos & 31));
    };
    for (int64_t kk = k0; kk < k1 && !complex_cal; ++kk) {
        const sk_score_op op = a.ops[kk];
        const int len = int(op.length);
        const unsigned pen = op.flags & SK_OPFLAG_NONCANDIDATE_PENALTY;
        if ((op.kind == SK_OP_BASES || op.kind == SK_OP_SOFT_CLIP) && len > 0) {
            if (pos >= int(SK_ENT_END)) {
                complex_cal = true;
                break;
            }
            const bool bases = (op.kind == SK_OP_BASES);
            if (bases && (op.src < 0 || int64_t(op.src) + len > P)) complex_cal = true;
            emit(npen, !bases, bases ? int(op.src) - pos : P - pos);
            pos += len;
            npen = pen;
        } else {
            npen += pen;
        }
    }
    if (!complex_cal) {
        if (pos != L || pos >= int(SK_ENT_END)) complex_cal = true;
        else emit(npen, false, P - pos);
    }
    if (complex_cal) {
        for (int i = 0; i < nslots; ++i) ent[i] = SK_ENT_END;
        ent[0] = SK_ENT_COMPLEX;
        atomicOr(&a.addmask[int64_t(r) * W + (W - 1)], 1u << 31);
        n_ent = 0;
        return true;
    }
    // where entries add terms
    uint32_t* am = a.addmask + int64_t(r) * W;
    for (int i = 0; i < e; ++i)
        if (ent[i] & SK_ENT_ADD_BITS) {
            const unsigned p = ent[i] & SK_ENT_POS_MASK;
            atomicOr(&am[p >> 5], 1u << (p & 31));
        }
    n_ent = e;
    return false;
}

// the column words of candidate alignment c, position by position (the serial form)
__device__ inline void f3_columns_serial(const FlatArgs& a, const int c, const int r, const uint8_t* hap, const int32_t L, const int32_t P,
                                         const uint32_t* ent, const int e)
{
    const int W = a.evmask_words;
    auto col_at = [&](const int idx) -> unsigned { return (idx >= 0 && idx < P) ? sk_ent_col_index(hap[idx]) : unsigned(SK_ENT_ZERO_COL); };
    const int64_t k0 = a.op_off[c], k1 = a.op_off[c + 1];
    // one word (eight read positions) at a time: assembled in a register, stored once
    const int ncr = a.cal_off[r + 1] - a.cal_off[r], j = c - a.cal_off[r];
    uint32_t* cm = reinterpret_cast<uint32_t*>(a.colmat) + a.colmat_off[r] + j;
    const uint8_t* read = a.read_code + a.read_off[r];
    constexpr uint32_t NONE_WORD = 0x11111111u * SK_SEL_NONE;
    uint32_t word = NONE_WORD;
    int wk = 0; // index of the word being assembled
    int pos = 0;
    const int nch = (L + 7) >> 3;
    int ei = 0; // next entry that adds terms (entries and positions both ascend)
    bool needs_entries = false;
    // an entry adding exactly one penalty at position i becomes bit 2 of that position's nibble; anything else leaves the read to
    // its entries (host form and rationale: sk_align_prepare_cols)
    auto flag_at = [&](const int i) -> unsigned {
        while (ei < e && int(ent[ei] & SK_ENT_POS_MASK) < i) ++ei;
        if (ei < e && int(ent[ei] & SK_ENT_POS_MASK) == i && (ent[ei] & SK_ENT_ADD_BITS)) {
            const bool simple = ((ent[ei] >> 10) & 7u) == 1u && !(ent[ei] & (1u << 13)) && i < 8 * nch;
            if (simple) return 4u;
            needs_entries = true;
        }
        return 0u;
    };
    auto put = [&](const int i, const unsigned sel) {
        const int k8 = i >> 3;
        if (k8 != wk) {
            cm[int64_t(wk) * ncr] = word;
            for (int q = wk + 1; q < k8; ++q) cm[int64_t(q) * ncr] = NONE_WORD; // (words a soft clip spans)
            word = NONE_WORD;
            wk = k8;
        }
        const unsigned shift = 8u * (unsigned(i) & 3u) + ((i & 4) ? 4u : 0u);
        word = (word & ~(0xfu << shift)) | (sel << shift);
    };
    for (int64_t kk = k0; kk < k1; ++kk) {
        const sk_score_op op = a.ops[kk];
        const int len = int(op.length);
        if (!((op.kind == SK_OP_BASES || op.kind == SK_OP_SOFT_CLIP) && len > 0)) continue;
        if (op.kind == SK_OP_BASES) {
            for (int t = 0; t < len && pos + t < L; ++t)
                put(pos + t, sk_col_selector(col_at(int(op.src) + t), read[pos + t]) | flag_at(pos + t));
        } else if (flag_at(pos)) { // (a soft clip's entry is never the simple kind; flag_at notes that the entries are needed)
        }
        pos += len;
    }
    {
        const unsigned f = flag_at(L); // trailing penalties: the nibble after the last base, where the last word has one
        if (f) put(L, SK_SEL_NONE | f);
    }
    for (; ei < e; ++ei) // (entries no position above stood for)
        if ((ent[ei] & SK_ENT_ADD_BITS) && int(ent[ei] & SK_ENT_POS_MASK) > L) needs_entries = true;
    if (needs_entries) atomicOr(&a.addmask[int64_t(r) * W + (W - 1)], 1u << 30);
    if (wk < nch) cm[int64_t(wk) * ncr] = word;
    for (int q = wk + 1; q < nch; ++q) cm[int64_t(q) * ncr] = NONE_WORD;
}

__global__ __launch_bounds__(64) void entries_kernel(const FlatArgs a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cals) return;
    const int r = read_of_cal(a, c);
    const int32_t L = int32_t(a.read_off[r + 1] - a.read_off[r]);
    const int32_t P = int32_t(a.hap_off[r + 1] - a.hap_off[r]);
    const uint8_t* hap = a.hap_code + a.hap_off[r];
    uint32_t* ent = a.entries + a.op_off[c] + 2 * int64_t(c);
    int e = 0;
    if (f3_emit_entries(a, c, r, hap, L, P, ent, e)) return;
    f3_columns_serial(a, c, r, hap, L, P, ent, e);
}

constexpr int F3W_MAX_D = 64;    // distinct haplotype offsets of a read's candidate alignments the wave form holds
constexpr int F3W_MAX_NCH = 32;  // reads of up to 256 bases
constexpr int F3W_MAX_POOL = 1024;

struct F3wLds
{
    uint8_t hap[F3W_MAX_POOL];
    uint8_t read[8 * F3W_MAX_NCH];
    uint8_t slot_of[2048];           // haplotype offset + SK_ENT_HIDX_BIAS -> its slot in M
    uint32_t delta_bits[64];         // which of the 2048 offsets occur
    int32_t n_slots;
    int16_t delta_of[F3W_MAX_D];     // slot -> haplotype offset
    uint32_t M[F3W_MAX_D][F3W_MAX_NCH];  // the column word of (offset, 8 read positions)
    uint32_t tile[F3W_MAX_NCH][64];      // the column words of 64 candidate alignments
};

// positions [0, x) of an 8-position column word (position i sits at bit 8 (i & 3) + 4 (i >> 2 & 1))
__device__ __forceinline__ uint32_t f3w_below(const int x)
{
    const uint32_t lo = (x >= 4) ? 0x0f0f0f0fu : (uint32_t((1ull << (8 * x)) - 1ull) & 0x0f0f0f0fu);
    const uint32_t hi = (x <= 4) ? 0u : (x >= 8 ? 0xf0f0f0f0u : (uint32_t((1ull << (8 * (x - 4))) - 1ull) & 0xf0f0f0f0u));
    return lo | hi;
}

__global__ __launch_bounds__(64) void entries_wave_kernel(const FlatArgs a)
{
    __shared__ F3wLds S;
    const int r = blockIdx.x;
    const int lane = threadIdx.x;
    const int c0 = a.cal_off[r], c1 = a.cal_off[r + 1];
    const int ncr = c1 - c0;
    if (ncr == 0) return;
    const int32_t L = int32_t(a.read_off[r + 1] - a.read_off[r]);
    const int32_t P = int32_t(a.hap_off[r + 1] - a.hap_off[r]);
    const uint8_t* ghap = a.hap_code + a.hap_off[r];
    const uint8_t* gread = a.read_code + a.read_off[r];
    const int nch = (L + 7) >> 3;
    const bool fits = (L >= 0 && nch <= F3W_MAX_NCH && P >= 0 && P <= F3W_MAX_POOL);
    if (fits) {
        for (int i = lane; i < P; i += 64) S.hap[i] = ghap[i];
        for (int i = lane; i < 8 * nch; i += 64) S.read[i] = (i < L) ? gread[i] : uint8_t(15);
    }
    S.delta_bits[lane] = 0;
    if (lane == 0) S.n_slots = 0;
    __syncthreads();
    const uint8_t* hap = fits ? S.hap : ghap;

    // ---- the entries of every candidate alignment; the haplotype offsets their base ops use
    for (int c = c0 + lane; c < c1; c += 64) {
        uint32_t* ent = a.entries + a.op_off[c] + 2 * int64_t(c);
        int e = 0;
        const bool complex_cal = f3_emit_entries(a, c, r, hap, L, P, ent, e);
        if (complex_cal) continue;
        if (!fits) { // (a read the LDS form does not hold: position by position, as the thread-per-alignment kernel)
            f3_columns_serial(a, c, r, hap, L, P, ent, e);
            continue;
        }
        int pos = 0;
        for (int64_t kk = a.op_off[c]; kk < a.op_off[c + 1]; ++kk) {
            const sk_score_op op = a.ops[kk];
            const int len = int(op.length);
            if (!((op.kind == SK_OP_BASES || op.kind == SK_OP_SOFT_CLIP) && len > 0)) continue;
            if (op.kind == SK_OP_BASES) {
                const int d = int(op.src) - pos + SK_ENT_HIDX_BIAS; // (0..2047: f3_emit_entries turned anything else down)
                atomicOr(&S.delta_bits[d >> 5], 1u << (d & 31));
            }
            pos += len;
        }
    }
    if (!fits) return;
    __syncthreads();
    // ---- a slot per distinct offset (ascending)
    {
        const uint32_t w = S.delta_bits[lane];
        int n = __popc(w), before = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(before, d, 64);
            if (lane >= d) before += up;
        }
        const int total = __shfl(before, 63, 64);
        before -= n;
        if (lane == 0) S.n_slots = total;
        if (total <= F3W_MAX_D) {
            uint32_t ww = w;
            int slot = before;
            while (ww) {
                const int b = __ffs(int(ww)) - 1;
                ww &= ww - 1u;
                S.delta_of[slot] = int16_t(32 * lane + b - SK_ENT_HIDX_BIAS);
                S.slot_of[32 * lane + b] = uint8_t(slot++);
            }
        }
    }
    __syncthreads();
    const int D = S.n_slots;
    if (D > F3W_MAX_D) { // (more offsets than the table holds: the serial form for this read)
        for (int c = c0 + lane; c < c1; c += 64) {
            const uint32_t* ent = a.entries + a.op_off[c] + 2 * int64_t(c);
            if (ent[0] == SK_ENT_COMPLEX) continue;
            int e = 0;
            while ((ent[e] & SK_ENT_POS_MASK) != SK_ENT_END) ++e;
            f3_columns_serial(a, c, r, hap, L, P, ent, e);
        }
        return;
    }
    // ---- M: every (offset, 8 positions) once
    constexpr uint32_t NONE_WORD = 0x11111111u * SK_SEL_NONE;
    for (int t = lane; t < D * nch; t += 64) {
        const int slot = t / nch, k = t - slot * nch;
        const int delta = S.delta_of[slot];
        uint32_t word = NONE_WORD;
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8) {
            const int p = 8 * k + t8;
            if (p < L) {
                const int idx = p + delta;
                const unsigned col = (idx >= 0 && idx < P) ? sk_ent_col_index(S.hap[idx]) : unsigned(SK_ENT_ZERO_COL);
                const unsigned sel = sk_col_selector(col, S.read[p]);
                const unsigned shift = 8u * (unsigned(t8) & 3u) + ((t8 & 4) ? 4u : 0u);
                word = (word & ~(0xfu << shift)) | (sel << shift);
            }
        }
        S.M[slot][k] = word;
    }
    __syncthreads();
    // ---- the column words of the candidate alignments, 64 at a time
    const int W = a.evmask_words;
    uint32_t* cm_base = reinterpret_cast<uint32_t*>(a.colmat) + a.colmat_off[r];
    for (int j0 = 0; j0 < ncr; j0 += 64) {
        const int j = j0 + lane;
        for (int k = 0; k < nch; ++k) S.tile[k][lane] = NONE_WORD;
        if (j < ncr) {
            const int c = c0 + j;
            const uint32_t* ent = a.entries + a.op_off[c] + 2 * int64_t(c);
            if (ent[0] != SK_ENT_COMPLEX) {
                int pos = 0;
                for (int64_t kk = a.op_off[c]; kk < a.op_off[c + 1]; ++kk) {
                    const sk_score_op op = a.ops[kk];
                    const int len = int(op.length);
                    if (!((op.kind == SK_OP_BASES || op.kind == SK_OP_SOFT_CLIP) && len > 0)) continue;
                    if (op.kind == SK_OP_BASES) {
                        const int slot = S.slot_of[int(op.src) - pos + SK_ENT_HIDX_BIAS];
                        const int p0 = pos, p1 = min(pos + len, int(L));
                        for (int k = p0 >> 3; p0 < p1 && k <= (p1 - 1) >> 3; ++k) {
                            const int lo = max(p0, 8 * k) - 8 * k, hi = min(p1, 8 * k + 8) - 8 * k;
                            const uint32_t m = f3w_below(hi) & ~f3w_below(lo);
                            S.tile[k][lane] = (S.tile[k][lane] & ~m) | (S.M[slot][k] & m);
                        }
                    }
                    pos += len;
                }
                // an entry adding exactly one penalty becomes bit 2 of its position's nibble; anything else leaves the read to its
                // entries (f3_columns_serial's flag_at: every entry sits at the start of a base op, of a soft clip, or at L)
                bool needs_entries = false;
                for (int ei = 0; (ent[ei] & SK_ENT_POS_MASK) != SK_ENT_END; ++ei) {
                    if (!(ent[ei] & SK_ENT_ADD_BITS)) continue;
                    const int i = int(ent[ei] & SK_ENT_POS_MASK);
                    const bool simple = ((ent[ei] >> 10) & 7u) == 1u && !(ent[ei] & (1u << 13)) && i < 8 * nch && i <= L;
                    if (simple) {
                        const unsigned shift = 8u * (unsigned(i) & 3u) + ((i & 4) ? 4u : 0u);
                        S.tile[i >> 3][lane] |= 4u << shift;
                    } else {
                        needs_entries = true;
                    }
                }
                if (needs_entries) atomicOr(&a.addmask[int64_t(r) * W + (W - 1)], 1u << 30);
            }
        }
        // (a lane reads and writes only its own column of the tile)
        if (j < ncr)
            for (int k = 0; k < nch; ++k) cm_base[int64_t(k) * ncr + j] = S.tile[k][lane];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// S3: stage 3 (csrc/stage3_core.h) -- the max / smooth candidate alignment, the realigned alignment clipped where the smooth
// pool disagrees, the late normalisation filter and score_indels -- one wavefront per read over the read's candidate alignments and
// scores where the scoring kernel left them: the loops over alignments are spread over the 64 lanes, lane 0 takes the decisions the
// reference defines by iteration order (see the header).  What leaves the device is a fixed-size record per read.
enum { S3_LIGHT_CALS = 256, S3_LDS_CALS = 1580 }; // (1580 alignments: 53 KB; with the shared state that stays under 64 KB per workgroup)

struct WaveLanes // the lanes of a workgroup: one wavefront for most reads, four for reads with many candidate alignments
{
    int id, width;
    __device__ void sync() const { __syncthreads(); }
    __device__ void max_i64(long long* p, const long long v) const { atomicMax(p, v); }
};

struct Stage3Args
{
    sk3::Tab tab;
    sk3::Opt opt;
    int32_t n_reads;
    const int32_t* status;
    const int32_t* cal_off;
    const PCal* cals;    // the records in set order -- or, with `slot`, the pool the search left its leaves in
    const int32_t* slot; // null, or [n_cals] the pool slot of every alignment in set order
    const double* scores;
    const int64_t* read_off;
    const uint8_t* read_code;
    const int32_t* map_level;
    int32_t* order;
    double* smooth;
    uint8_t* flag;
    uint32_t* key;
    double* sorted_score;
    uint32_t* sorted_hash;
    int32_t* next_same;
    int32_t* range_end;
    uint8_t* removed;
    uint8_t* rm_type;
    int32_t* rm_pos;
    sk3::Out* out;
    const int32_t* list; // the reads of this launch
    int32_t lds_cals;
    // the job as one fixed sequence: the launch has a block per read of the JOB, the number of reads on this launch's list is on the
    // device (n_list; the heavy list is filled from the back: list_step = -1), and nothing runs when F5 turned a read down (skip_if:
    // the scores are then incomplete -- the host runs the job again through the staged chain)
    const int32_t* n_list;
    int32_t list_step;
    const int32_t* skip_if;
};

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void stage3_kernel(const Stage3Args a)
{
    constexpr int T = 64 * WAVES;
    __shared__ sk3::Shared sh;
    extern __shared__ double s3_lds[]; // the per-alignment arrays of the selection and the late normalisation filter, for a read with at most a.lds_cals candidate alignments
    if (a.skip_if && *a.skip_if > 0) return;
    if (a.n_list && int(blockIdx.x) >= *a.n_list) return;
    const int r = a.list[int(blockIdx.x) * (a.n_list ? a.list_step : 1)];
    sk3::Out& o = a.out[r];
    const int32_t c0 = a.cal_off[r], c1 = a.cal_off[r + 1];
    if (a.status[r] != ST_OK || c1 == c0) {
        if (threadIdx.x == 0) o.status = sk3::S3_CAPACITY;
        return;
    }
    const int64_t b0 = a.read_off[r], b1 = a.read_off[r + 1];
    sk3::Read rd;
    rd.cals = a.slot ? sk3::CalView{ a.cals, a.slot + c0 } : sk3::CalView{ a.cals + c0, nullptr };
    rd.scores = a.scores + c0;
    rd.scores_select = rd.scores;
    rd.n_cals = c1 - c0;
    rd.map_level = a.map_level[r];
    rd.read_length = int32_t(b1 - b0);
    if (threadIdx.x == 0) sh.ne = 0; // (borrowed as the counter of bases that are not N)
    __syncthreads();
    {
        int na = 0;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += T) na += (a.read_code[i] != SK_BAM_ANY) ? 1 : 0;
        for (int d = 32; d > 0; d >>= 1) na += __shfl_xor(na, d);
        if ((threadIdx.x & 63) == 0) atomicAdd(&sh.ne, na);
    }
    __syncthreads();
    rd.non_ambig = sh.ne;
    __syncthreads();
    sk3::Scratch w;
    w.order = a.order + c0;
    w.smooth = a.smooth + c0;
    w.flag = a.flag + c0;
    w.key = a.key + 4 * size_t(c0);
    w.sorted_score = a.sorted_score + c0;
    w.sorted_hash = a.sorted_hash + c0;
    w.next_same = a.next_same + c0;
    w.range_end = a.range_end + c0;
    w.removed = a.removed + c0;
    w.rm_type = a.rm_type + b0;
    w.rm_pos = a.rm_pos + b0;
    if (rd.n_cals <= a.lds_cals) {
        // what lane 0's scans and the ordering walk over and over sits in LDS (the accesses are chains of dependent loads)
        double* sc = s3_lds; // the scores for the selection, later the smoothed scores by place
        double* ssc = sc + a.lds_cals;
        int32_t* ord = reinterpret_cast<int32_t*>(ssc + a.lds_cals);
        uint32_t* shs = reinterpret_cast<uint32_t*>(ord + a.lds_cals);
        int32_t* nxt = reinterpret_cast<int32_t*>(shs + a.lds_cals);
        int32_t* rend = nxt + a.lds_cals;
        uint8_t* fl = reinterpret_cast<uint8_t*>(rend + a.lds_cals);
        uint8_t* rem = fl + a.lds_cals;
        for (int i = threadIdx.x; i < rd.n_cals; i += T) sc[i] = rd.scores[i];
        __syncthreads();
        rd.scores_select = sc;
        w.smooth = sc;
        w.sorted_score = ssc;
        w.sorted_hash = shs;
        w.next_same = nxt;
        w.range_end = rend;
        w.order = ord;
        w.flag = fl;
        w.removed = rem;
    }
    WaveLanes ln;
    ln.id = int(threadIdx.x);
    ln.width = T;
    sk3::finish_read(ln, a.tab, a.opt, rd, w, sh, o);
}

// ---------------------------------------------------------------------------------------------------------------------
// buffers: grown on demand, kept for the life of the process (one job after the other reuses them)

struct View // a piece of one of the arenas below
{
    void* p = nullptr;
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The job's small arrays live in a few arenas so that a job is a handful of copies and fills, not dozens (each one costs 4-5 us on
// the stream whatever its size): everything that goes up before the search in `in_arena` (packed in a pinned mirror, one copy), every
// array that starts at zero in `zero_arena` (one fill; the parts the host reads come back in one copy per synchronisation point)
struct EnumBuffers
{
    SkDevBuf in_arena, zero_arena, minmax_arena, mask_arena;
    SkPinBuf h_in_arena, h_zero_arena;
    View tab, ins, toggle, ref, ref_code, ins_code, reads, read_off, read_code, read_qual, r2i, i2r, orig, map_level;
    View counters, status, warn, n_raw, hap_len, fill, n_uniq, consulted;
    View win_begin, ins_lo, win_end, ins_hi, evmask, addmask;
    View h_counters, h_status, h_warn, h_n_raw, h_hap_len, h_n_uniq, h_consulted;
    View cal_off_z, h_cal_off_z;
    SkDevBuf level_a, level_b, pool, leaf_read, leaf_hash;
    SkDevBuf raw_off, grouped, ghash, gkey, dup, sorted;
    SkDevBuf n_ops, win_len, n_ins, ins_idx, ins_off, n_seg8;
    SkDevBuf cal_off, hap_off, cals, hap_code, op_off, ops, entries, scores, colmat, colmat_off;
    SkDevBuf s3_order, s3_smooth, s3_flag, s3_rm_type, s3_rm_pos, s3_key, s3_sorted_score, s3_sorted_hash, s3_next_same, s3_range_end, s3_removed, s3_out, s3_list;
    SkDevBuf tail_order; // F5's last hand-outs (tail_order_kernel)
    SkPinBuf h_s3_out, h_s3_list;
    SkPinBuf h_raw_off, h_n_ops, h_cal_off, h_hap_off, h_op_off, h_cals, h_scores, h_colmat_off;
    void drop() // every block above, then the views into them
    {
        for (SkDevBuf* b : { &in_arena, &zero_arena, &minmax_arena, &mask_arena, &level_a, &level_b, &pool, &leaf_read, &leaf_hash, &raw_off, &grouped, &ghash,
                             &gkey, &dup, &sorted, &n_ops, &win_len, &n_ins, &ins_idx, &ins_off, &n_seg8, &cal_off, &hap_off, &cals, &hap_code, &op_off, &ops,
                             &entries, &scores, &colmat, &colmat_off, &s3_order, &s3_smooth, &s3_flag, &s3_rm_type, &s3_rm_pos, &s3_key, &s3_sorted_score,
                             &s3_sorted_hash, &s3_next_same, &s3_range_end, &s3_removed, &s3_out, &s3_list, &tail_order })
            b->drop();
        for (SkPinBuf* b : { &h_in_arena, &h_zero_arena, &h_s3_out, &h_s3_list, &h_raw_off, &h_n_ops, &h_cal_off, &h_hap_off, &h_op_off, &h_cals, &h_scores,
                             &h_colmat_off })
            b->drop();
        *this = EnumBuffers();
    }
};
EnumBuffers& bufs()
{
    static EnumBuffers b;
    return b;
}

// a job's reservations, as tables: a device buffer holds at least 256 bytes (an empty array still has an address), a pinned one 64 bytes
// more than asked for (job_stage_out_kernel writes whole 16-byte words)
int reserve_dev(std::initializer_list<std::pair<SkDevBuf&, size_t>> wants) // { buffer, bytes }, ...
{
    for (const auto& w : wants)
        if (w.first.reserve(std::max<size_t>(w.second, 256))) return 1;
    return 0;
}
int reserve_pinned(std::initializer_list<std::pair<SkPinBuf&, size_t>> wants)
{
    for (const auto& w : wants)
        if (w.first.reserve(w.second + 64)) return 1;
    return 0;
}
// copies on the job's stream; nothing is submitted for zero bytes
int copy_up(hipStream_t st, const SkDevBuf& dst, const void* src, const size_t bytes)
{
    if (bytes > 0) SK_HIP(skrt::memcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}
int copy_down(hipStream_t st, const SkPinBuf& dst, const SkDevBuf& src, const size_t bytes)
{
    if (bytes > 0) SK_HIP(skrt::memcpyAsync(dst.p, src.p, bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

} // namespace

extern "C" int sk_enum_device_available(void) { return sk_ctx().ready ? 1 : 0; } // (host stages alone run without a device)

namespace
{
uint64_t g_generation = 0; // of the run whose candidate alignments the buffers hold
int32_t g_n_cals = 0;
bool g_cals_gathered = false; // bufs().cals holds the run's records in set order (else: pool + list, gathered when the host asks)
const PCal* g_cals_pool = nullptr;
const int32_t* g_cals_list = nullptr;
const double* g_scores = nullptr; // the run's scores, where the scoring kernel left them

// what sk_enum_device_rescore needs to run F1-F3 + the scoring kernel again on the candidate alignments of the last run
struct LastFlat
{
    bool valid = false;
    bool fused = false; // the last run scored with F5 (fs), else with the staged chain (fa, d)
    FusedScoreArgs fs;
    FlatArgs fa;
    sk_align_batch d;
    int32_t n = 0, n_cals = 0;
    int64_t cells = 0;
    size_t mask_bytes = 0, colmat_bytes = 0;
    double* scores = nullptr;
} g_last;
} // namespace

// (the generation counter stays: a caller that kept a generation from before sk_shutdown is refused, not served from another run's memory)
void sk_enum_reset()
{
    bufs().drop();
    g_n_cals = 0;
    g_scores = nullptr;
    g_cals_pool = nullptr;
    g_cals_list = nullptr;
    g_cals_gathered = false;
    g_last.valid = false;
}

extern "C" uint64_t sk_enum_device_generation(void) { return g_generation; }

extern "C" int sk_enum_device_fetch_scores(const uint64_t generation, const int32_t first, const int32_t count, double* dst)
{
    if (generation != g_generation || first < 0 || count < 0 || first + count > g_n_cals || !g_scores) return 1;
    if (count == 0) return 0;
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    SK_HIP(skrt::memcpyAsync(dst, g_scores + first, 8 * size_t(count), hipMemcpyDeviceToHost, ctx.stream));
    SK_HIP(skrt::streamSynchronize(ctx.stream));
    return 0;
}

extern "C" int sk_enum_device_fetch_cals(const uint64_t generation, const int32_t first, const int32_t count, PCal* dst)
{
    if (generation != g_generation || first < 0 || count < 0 || first + count > g_n_cals) return 1;
    if (count == 0) return 0;
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    if (!g_cals_gathered) { // (F5 left the records where the search put them: in set order on demand, once per run)
        if (bufs().cals.reserve(sizeof(PCal) * size_t(g_n_cals))) return 1;
        SK_LAUNCH(gather_cals_kernel, dim3((g_n_cals + 63) / 64), dim3(64), 0, ctx.stream, g_cals_pool, g_cals_list, g_n_cals, bufs().cals.as<PCal>());
        SK_HIP(skrt::getLastError());
        g_cals_gathered = true;
    }
    SK_HIP(skrt::memcpyAsync(dst, bufs().cals.as<PCal>() + first, sizeof(PCal) * size_t(count), hipMemcpyDeviceToHost, ctx.stream));
    SK_HIP(skrt::streamSynchronize(ctx.stream));
    return 0;
}

namespace
{
// statistics of the process: jobs run as one fixed sequence (one wait), and those of them the host ran again the staged way because
// an assumption of the sequence did not hold (deeper levels than launched, a full leaf pool, a read outside F5's form)
int64_t g_jobs_one_wait = 0, g_jobs_one_wait_redone = 0, g_jobs_staged = 0;
int64_t g_tail_launches = 0; // launches of tail_order_kernel by the job drivers (sk_debug_f5_tail_launches)
int64_t g_late_turn_downs = 0; // F5's rounds after a read's first that left the read to the staged chain, over the drivers' F5 launches
int64_t g_shared_rounds = 0; // F5's rounds scored by a wave other than their read's owner, over the drivers' jobs (sk_debug_f5_shared_rounds)
// diagnostics ($SK_ENUM_JOB_SECONDS): where a one-sequence job's wall time goes -- buffers + packing, submissions, the wait -- on stderr at exit
struct JobSeconds
{
    double setup = 0, submit = 0, wait = 0, after = 0;
    ~JobSeconds()
    {
        if (std::getenv("SK_ENUM_JOB_SECONDS"))
            std::fprintf(stderr, "strelka_amd enum job seconds: jobs=%lld setup=%.4f submit=%.4f wait=%.4f after=%.4f\n", (long long)g_jobs_one_wait, setup, submit,
                         wait, after);
    }
} g_job_seconds;
}
extern "C" void sk_enum_device_job_counts(int64_t* one_wait, int64_t* one_wait_redone, int64_t* staged)
{
    if (one_wait) *one_wait = g_jobs_one_wait;
    if (one_wait_redone) *one_wait_redone = g_jobs_one_wait_redone;
    if (staged) *staged = g_jobs_staged;
}

// test hooks (include/strelka_amd.h): the table kernel over a host-given cal_off with the grid's waves and the shift given, in buffers of
// its own (the last job's stay as they are); and how often the job drivers launched it
extern "C" int sk_debug_f5_tail_order(const int32_t* cal_off, const int32_t n_reads, const int32_t waves, const int32_t shift, int32_t* first, int32_t* n,
                                      int32_t* order_out)
{
    SK_REQUIRE_INIT();
    if (!cal_off || n_reads < 0 || waves <= 0 || !first || !n) return sk_fail("sk_debug_f5_tail_order: bad argument");
    const int T = f5_tail_window(n_reads, waves, shift);
    *first = T ? n_reads - T : 0;
    *n = T;
    if (T == 0) return 0; // (no launch: what the drivers do for such a job)
    if (T > F5_TAIL_MAX) return sk_fail("sk_debug_f5_tail_order: a window of more than 65536 hand-outs (the drivers cut the shift down)");
    if (!order_out) return sk_fail("sk_debug_f5_tail_order: no room for the table");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    int32_t *d_off = nullptr, *d_order = nullptr;
    int rc = 0;
    auto run = [&]() -> int {
        SK_HIP(skrt::malloc_(&d_off, 4 * (size_t(n_reads) + 1)));
        SK_HIP(skrt::malloc_(&d_order, 4 * size_t(T)));
        SK_HIP(skrt::memcpyAsync(d_off, cal_off, 4 * (size_t(n_reads) + 1), hipMemcpyHostToDevice, st));
        SK_HIP(skrt::memsetAsync(d_order, 0xff, 4 * size_t(T), st)); // (an entry the kernel left out shows as -1)
        launch_tail_order(st, TailArgs{ d_off, n_reads - T, T, shift, d_order });
        SK_HIP(skrt::getLastError());
        SK_HIP(skrt::memcpyAsync(order_out, d_order, 4 * size_t(T), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::streamSynchronize(st));
        return 0;
    };
    rc = run();
    if (d_off) (void)skrt::free_(d_off);
    if (d_order) (void)skrt::free_(d_order);
    return rc;
}
extern "C" int64_t sk_debug_f5_tail_launches(void) { return g_tail_launches; }
extern "C" int64_t sk_debug_f5_shared_rounds(void) { return g_shared_rounds; }
extern "C" int64_t sk_debug_f5_late_turn_downs(void) { return g_late_turn_downs; }

// ---------------------------------------------------------------------------------------------------------------------
// the job driver.  A job is prepared once (start_job, plan_job: capacities, the arenas' layout, reservations, the packed input on its way up)
// and then run either as ONE fixed sequence of submissions with one host wait (run_one_wait) or the staged way, with a wait after the
// search, one after the sets and one at the end (run_staged).  One builder per kernel argument struct: its parameters are what differs
// between the two runs.
namespace
{
struct JobPlan
{
    const SkEnumInput* in = nullptr;
    EnumBuffers& B = bufs();
    hipStream_t st = nullptr;
    bool one_wait = false, with_stage3 = false;
    int n = 0;
    int64_t n_bases = 0, frame_cap = 0, pool_cap = 0; // capacities: calls in flight at one depth, leaves found (before duplicates are dropped)
    int W = 0;                                        // words of a read's event mask
    int max_order = 0;                                // the deepest indel order a read of the job arrives with
    size_t in_bytes = 0, zero_bytes = 0, minmax_bytes = 0, mask_bytes = 0; // the arenas
    size_t minmax_split = 0;                                               // win_begin, ins_lo before it; win_end, ins_hi from it on
    PJob dj;
    // stage 3: a read with at most light_cals candidate alignments is the first launch's; a block keeps up to lds_cals of them in LDS
    int light_cals = S3_LIGHT_CALS, lds_cals = S3_LDS_CALS;
    bool timing = false; // $SK_ENUM_TIMING
    std::chrono::steady_clock::time_point t_begin;

    void lap(const char* what) const
    {
        if (!timing) return;
        (void)skrt::streamSynchronize(st);
        std::fprintf(stderr, "[enum-dev] %-28s t=%.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    }
};

struct Piece // of an arena, at a 256-byte offset
{
    View* view;
    const void* src; // in_arena: where the bytes come from
    size_t bytes, off;
};
size_t lay_out(Piece* pc, const int n_pieces)
{
    size_t at = 0;
    for (int i = 0; i < n_pieces; ++i) {
        pc[i].off = at;
        at += (pc[i].bytes + 255) & ~size_t(255);
    }
    return at;
}

// everything about a job that is known before its first submission.  one_wait: the buffers between the search and stage 3 will be sized
// by the pool's capacity, and cal_off is made on the device (a piece of the zero arena)
int plan_job(const SkEnumInput* in, const bool one_wait, JobPlan& p)
{
    EnumBuffers& B = p.B;
    p.in = in;
    p.st = sk_ctx().stream;
    p.one_wait = one_wait;
    const int n = p.n = in->n_reads;
    const int64_t n_bases = p.n_bases = n ? in->read_off[n] : 0;
    // capacities: calls in flight at one depth and leaves found (before duplicates are dropped), for the whole job; a job that
    // needs more has the reads that did not fit enumerated on the host
    // (sized by the job; the ceilings -- two level buffers of 2^23 frames, 2^25 leaves: ~21 GB in all -- are a fraction of 288 GB of HBM
    // and let a job of 2^16 reads with ~90 candidate alignments each run whole)
    p.frame_cap = std::min<int64_t>(std::max<int64_t>(int64_t(n) * 128, 1 << 18), 1 << 23);
    p.pool_cap = std::min<int64_t>(std::max<int64_t>(int64_t(n) * 512, 1 << 19), int64_t(32) << 20);
    const char* const test_caps = std::getenv("SK_ENUM_TEST_CAPS"); // tests: small capacities, so that the overflow paths run
    if (test_caps) {
        long long fc = 0, pc = 0;
        if (std::sscanf(test_caps, "%lld,%lld", &fc, &pc) == 2 && fc > 0 && pc > 0) {
            p.frame_cap = std::max<int64_t>(fc, n);
            p.pool_cap = pc;
        }
    }
    // one sequence: the buffers between the search and stage 3 are sized by the pool's capacity instead of by counts the host would have
    // to wait for -- 256 leaves per read (at least 2^17) cover every WGS-like job; one that needs more is run again the staged way
    if (one_wait && !(test_caps && test_caps[0])) p.pool_cap = std::min<int64_t>(p.pool_cap, std::max<int64_t>(int64_t(n) * 256, 1 << 17));
    const bool s3 = p.with_stage3 = in->want_scores && in->want_stage3;
    const int W = p.W = sk_ent_evmask_words(std::max(in->max_read_len, 0));
    for (int r = 0; r < n; ++r) p.max_order = std::max(p.max_order, int(in->reads[r].n_order));
    if (const char* e = std::getenv("SK_STAGE3_TEST_LDS_CALS")) { // tests: small capacities, so that the second launch and the HBM arrays run
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b >= a && b <= S3_LDS_CALS) {
            p.light_cals = a;
            p.lds_cals = b;
        }
    }
    if (reserve_dev({ { B.level_a, sizeof(PFrame) * size_t(p.frame_cap) }, { B.level_b, sizeof(PFrame) * size_t(p.frame_cap) },
                      { B.pool, sizeof(PCal) * size_t(p.pool_cap) }, { B.leaf_read, 4 * size_t(p.pool_cap) }, { B.leaf_hash, 4 * size_t(p.pool_cap) },
                      { B.raw_off, 4 * size_t(n + 1) }, { B.win_len, 4 * size_t(n) }, { B.n_ins, 4 * size_t(n) },
                      { B.ins_idx, 2 * size_t(n) * INS_CAP }, { B.ins_off, 4 * size_t(n) * INS_CAP },
                      { B.cal_off, 4 * size_t(n + 1) }, { B.hap_off, 8 * size_t(n + 1) },
                      { B.tail_order, 4 * size_t(std::min(n, F5_TAIL_MAX)) } }) || // (F5's last hand-outs: a window is at most this, plan_tail)
        reserve_pinned({ { B.h_raw_off, 4 * size_t(n + 1) }, { B.h_cal_off, 4 * size_t(n + 1) }, { B.h_hap_off, 8 * size_t(n + 1) } }))
        return 1;
    // ---- the arenas: pieces at 256-byte offsets
    Piece ins_p[] = {
        { &B.tab, in->tab, sizeof(PIndel) * size_t(in->n_tab), 0 },
        { &B.ins, in->ins_pool, size_t(in->ins_pool_len), 0 },
        { &B.toggle, in->max_toggle, sizeof(uint32_t) * size_t(in->n_max_toggle), 0 },
        { &B.ref, in->ref, size_t(std::max(in->ref_len, 0)), 0 },
        { &B.reads, in->reads, sizeof(PRead) * size_t(n), 0 },
        { &B.read_off, in->read_off, sizeof(int64_t) * size_t(n + 1), 0 },
        { &B.read_code, in->read_code, size_t(n_bases), 0 },
        { &B.read_qual, in->read_qual, size_t(n_bases), 0 },
        { &B.r2i, in->r2i, s3 ? 8 * size_t(in->n_tab) : 0, 0 },
        { &B.i2r, in->i2r, s3 ? 8 * size_t(in->n_tab) : 0, 0 },
        { &B.orig, in->orig, s3 ? 4 * size_t(in->n_tab) : 0, 0 },
        { &B.map_level, in->map_level, s3 ? 4 * size_t(n) : 0, 0 },
        // (no source: the code images are written into the mirror below)
        { &B.ref_code, nullptr, size_t(std::max(in->ref_len, 0)) + 2 * size_t(F5_CODE_PAD), 0 },
        { &B.ins_code, nullptr, size_t(in->ins_pool_len), 0 },
    };
    const int n_ins_p = int(sizeof(ins_p) / sizeof(ins_p[0]));
    p.in_bytes = lay_out(ins_p, n_ins_p);
    // (the order matters: what the host reads after the search is one run, what it reads after the layout another)
    Piece zero_p[] = {
        { &B.counters, nullptr, 4 * size_t(N_COUNTERS), 0 }, { &B.warn, nullptr, 4 * size_t(n), 0 },    { &B.n_raw, nullptr, 4 * size_t(n), 0 },
        { &B.status, nullptr, 4 * size_t(n), 0 },            { &B.hap_len, nullptr, 4 * size_t(n), 0 }, { &B.fill, nullptr, 4 * size_t(n), 0 },
        { &B.n_uniq, nullptr, 4 * size_t(n), 0 },            { &B.consulted, nullptr, size_t(in->n_tab) + 1, 0 },
        { &B.cal_off_z, nullptr, one_wait ? 4 * size_t(n + 1) : 0, 0 }, // (one sequence: cal_off is made on the device and comes back with the arena)
    };
    View* zero_host[] = { &B.h_counters, &B.h_warn, &B.h_n_raw, &B.h_status, &B.h_hap_len, nullptr, &B.h_n_uniq, &B.h_consulted, &B.h_cal_off_z };
    const int n_zero_p = int(sizeof(zero_p) / sizeof(zero_p[0]));
    p.zero_bytes = lay_out(zero_p, n_zero_p);
    Piece minmax_p[] = { { &B.win_begin, nullptr, 4 * size_t(n), 0 }, { &B.ins_lo, nullptr, 4 * size_t(n), 0 },
                         { &B.win_end, nullptr, 4 * size_t(n), 0 },   { &B.ins_hi, nullptr, 4 * size_t(n), 0 } };
    p.minmax_bytes = lay_out(minmax_p, 4);
    p.minmax_split = minmax_p[2].off;
    Piece mask_p[] = { { &B.evmask, nullptr, 4 * (size_t(n) * size_t(W) + 1), 0 }, { &B.addmask, nullptr, 4 * (size_t(n) * size_t(W) + 1), 0 } };
    p.mask_bytes = lay_out(mask_p, 2);
    if (reserve_dev({ { B.in_arena, p.in_bytes }, { B.zero_arena, p.zero_bytes }, { B.minmax_arena, p.minmax_bytes }, { B.mask_arena, p.mask_bytes } })) return 1;
    if (reserve_pinned({ { B.h_in_arena, p.in_bytes }, { B.h_zero_arena, p.zero_bytes } })) return 1;
    for (int i = 0; i < n_ins_p; ++i) {
        ins_p[i].view->p = static_cast<char*>(B.in_arena.p) + ins_p[i].off;
        if (ins_p[i].bytes && ins_p[i].src) std::memcpy(static_cast<char*>(B.h_in_arena.p) + ins_p[i].off, ins_p[i].src, ins_p[i].bytes);
    }
    { // the job's code images, made once where its reference and its insert pool go up
        const CodeLut& lut = code_lut();
        const size_t ref_n = size_t(std::max(in->ref_len, 0));
        uint8_t* rc = static_cast<uint8_t*>(B.h_in_arena.p) + size_t(static_cast<char*>(B.ref_code.p) - static_cast<char*>(B.in_arena.p));
        std::memset(rc, SK_BAM_ANY, size_t(F5_CODE_PAD));
        for (size_t i = 0; i < ref_n; ++i) rc[size_t(F5_CODE_PAD) + i] = lut.code[uint8_t(in->ref[i])];
        std::memset(rc + size_t(F5_CODE_PAD) + ref_n, SK_BAM_ANY, size_t(F5_CODE_PAD));
        uint8_t* ic = static_cast<uint8_t*>(B.h_in_arena.p) + size_t(static_cast<char*>(B.ins_code.p) - static_cast<char*>(B.in_arena.p));
        for (size_t i = 0; i < size_t(in->ins_pool_len); ++i) ic[i] = lut.code[uint8_t(in->ins_pool[i])];
    }
    for (int i = 0; i < n_zero_p; ++i) {
        zero_p[i].view->p = static_cast<char*>(B.zero_arena.p) + zero_p[i].off;
        if (zero_host[i]) zero_host[i]->p = static_cast<char*>(B.h_zero_arena.p) + zero_p[i].off;
    }
    for (int i = 0; i < 4; ++i) minmax_p[i].view->p = static_cast<char*>(B.minmax_arena.p) + minmax_p[i].off;
    for (int i = 0; i < 2; ++i) mask_p[i].view->p = static_cast<char*>(B.mask_arena.p) + mask_p[i].off;

    p.dj.tab = B.tab.as<PIndel>();
    p.dj.n_tab = in->n_tab;
    p.dj.max_toggle = B.toggle.as<uint32_t>();
    p.dj.n_max_toggle = in->n_max_toggle;
    p.dj.sample_count = in->sample_count;
    p.dj.max_read_indel_toggle = in->max_read_indel_toggle;
    p.dj.max_candidate_indel_density = in->max_candidate_indel_density;
    p.dj.is_haplotyping_enabled = in->is_haplotyping_enabled;
    p.dj.max_indel_size = in->max_indel_size;
    p.dj.consulted = B.consulted.as<uint8_t>();
    p.dj.max_nodes = 0;
    return 0;
}

// the copy / fill calls instead of the job_stage_*_kernel launches of a one-sequence run ($SK_ENUM_STAGE_COPIES, for A-B runs)
bool stage_by_kernel()
{
    static const bool by_kernel = std::getenv("SK_ENUM_STAGE_COPIES") == nullptr;
    return by_kernel;
}

// the job's way in: the packed input up, the zero arena zeroed
int stage_in(const JobPlan& p)
{
    EnumBuffers& B = p.B;
    if (p.one_wait && stage_by_kernel()) {
        const uint32_t n_in16 = uint32_t(p.in_bytes / 16), n_zero16 = uint32_t(p.zero_bytes / 16); // (pieces sit at 256-byte offsets)
        const int blocks = int(std::min<size_t>(std::max<size_t>((std::max(p.in_bytes, p.zero_bytes) / 16 + 255) / 256, 1), 256));
        SK_LAUNCH(job_stage_in_kernel, dim3(blocks), dim3(256), 0, p.st, static_cast<const uint4*>(B.h_in_arena.p), static_cast<uint4*>(B.in_arena.p), n_in16,
                  static_cast<uint4*>(B.zero_arena.p), n_zero16);
    } else {
        if (copy_up(p.st, B.in_arena, B.h_in_arena.p, p.in_bytes)) return 1;
        SK_HIP(skrt::memsetAsync(B.zero_arena.p, 0, p.zero_bytes, p.st));
    }
    return 0;
}

// a run of the zero arena, device -> its pinned mirror
int fetch_zero(const JobPlan& p, const View& first, const View& last, const size_t last_bytes)
{
    char* const dev = static_cast<char*>(p.B.zero_arena.p);
    const size_t a0 = size_t(static_cast<char*>(first.p) - dev);
    const size_t a1 = size_t(static_cast<char*>(last.p) - dev) + last_bytes;
    SK_HIP(skrt::memcpyAsync(static_cast<char*>(p.B.h_zero_arena.p) + a0, dev + a0, a1 - a0, hipMemcpyDeviceToHost, p.st));
    return 0;
}

// a new generation of results, the plan, the input on its way; a job without reads is complete after this
int start_job(const SkEnumInput* in, SkEnumOutput* out, const bool one_wait, JobPlan& p)
{
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    if (!in || !out) return sk_fail("sk_enum_device_run: null argument");
    std::memset(out, 0, sizeof(*out));
    out->generation = ++g_generation;
    g_n_cals = 0;
    g_scores = nullptr;
    g_cals_gathered = false;
    g_last.valid = false;
    if (in->n_reads < 0 || in->n_tab < 0) return sk_fail("sk_enum_device_run: negative count");
    SK_HIP(skrt::setDevice(sk_ctx().device));
    p.timing = std::getenv("SK_ENUM_TIMING") != nullptr;
    p.t_begin = std::chrono::steady_clock::now();
    if (plan_job(in, one_wait, p) || stage_in(p)) return 1;
    EnumBuffers& B = p.B;
    B.h_cal_off.as<int32_t>()[0] = 0;
    out->status = B.h_status.as<int32_t>();
    out->cal_off = B.h_cal_off.as<int32_t>();
    out->consulted = B.h_consulted.as<uint8_t>();
    if (p.n == 0) {
        std::memset(B.h_consulted.p, 0, size_t(in->n_tab));
        return 0;
    }
    if (p.n > p.frame_cap) return sk_fail("sk_enum_device_run: more reads in one job than the device pipeline holds");
    p.lap("H2D");
    return 0;
}

// ---- the kernels' arguments

// root_sets_minmax: the root launch initialises the four minmax arrays (else they are filled before pool_bounds_kernel)
EnumArgs enum_args(const JobPlan& p, const bool root_sets_minmax)
{
    EnumBuffers& B = p.B;
    int32_t* const counters = B.counters.as<int32_t>();
    EnumArgs ea{}; // (level_in, level_out, depth: launch_search)
    ea.job = p.dj;
    ea.reads = B.reads.as<PRead>();
    ea.n_reads = p.n;
    ea.frame_cap = int32_t(p.frame_cap);
    ea.level_count = counters + CNT_LEVELS;
    ea.pool = B.pool.as<PCal>();
    ea.leaf_read = B.leaf_read.as<int32_t>();
    ea.leaf_hash = B.leaf_hash.as<uint32_t>();
    ea.pool_cap = int32_t(p.pool_cap);
    ea.n_leaves = counters + CNT_LEAVES;
    ea.n_nodes = reinterpret_cast<unsigned long long*>(counters + CNT_NODES);
    ea.n_raw = B.n_raw.as<int32_t>();
    ea.status = B.status.as<int32_t>();
    ea.warn = B.warn.as<int32_t>();
    ea.min_cells_a = root_sets_minmax ? B.win_begin.as<int32_t>() : nullptr;
    ea.min_cells_b = root_sets_minmax ? B.ins_lo.as<int32_t>() : nullptr;
    ea.max_cells_a = root_sets_minmax ? B.win_end.as<int32_t>() : nullptr;
    ea.max_cells_b = root_sets_minmax ? B.ins_hi.as<int32_t>() : nullptr;
    return ea;
}

// E1: the launches of depths [d0, d1) -- depth -1 is the root launch --, the two level buffers taking turns
void launch_search(const JobPlan& p, EnumArgs ea, const int d0, const int d1, const int level_blocks)
{
    PFrame* const buf[2] = { p.B.level_a.as<PFrame>(), p.B.level_b.as<PFrame>() };
    for (int d = d0; d < d1; ++d) {
        ea.level_in = (d < 0) ? nullptr : buf[d & 1];
        ea.level_out = buf[(d + 1) & 1];
        ea.depth = d;
        if (d < 0) SK_LAUNCH(root_kernel, dim3((p.n + 63) / 64), dim3(64), 0, p.st, ea);
        else SK_LAUNCH(level_kernel, dim3(level_blocks), dim3(64), 64 * sizeof(PFrame), p.st, ea);
    }
}

// n_leaves_dev: null, or where the search counted its leaves (n_leaves is then the pool's capacity)
SetArgs set_args(const JobPlan& p, const int32_t n_leaves, const int32_t* n_leaves_dev, const int32_t* cal_off)
{
    EnumBuffers& B = p.B;
    SetArgs sa{};
    sa.pool = B.pool.as<PCal>();
    sa.leaf_read = B.leaf_read.as<int32_t>();
    sa.leaf_hash = B.leaf_hash.as<uint32_t>();
    sa.status = B.status.as<int32_t>();
    sa.n_reads = p.n;
    sa.n_leaves = n_leaves;
    sa.n_leaves_dev = n_leaves_dev;
    sa.raw_off = B.raw_off.as<int32_t>();
    sa.fill = B.fill.as<int32_t>();
    sa.grouped = B.grouped.as<int32_t>();
    sa.ghash = B.ghash.as<uint32_t>();
    sa.gkey = B.gkey.as<ulonglong2>();
    sa.dup = B.dup.as<uint8_t>();
    sa.n_uniq = B.n_uniq.as<int32_t>();
    sa.cal_off = cal_off;
    sa.sorted = B.sorted.as<int32_t>();
    return sa;
}

// n_cals_on_device: the count is cal_off[n] (n_cals is then a capacity); n_ops: null unless L2 runs; chain: with the arrays of the
// staged chain (F1-F3 + A1c), which are reserved once the layout pass has come back
FlatArgs flat_args(const JobPlan& p, const int32_t n_cals, const bool n_cals_on_device, const int32_t* cal_off, int32_t* n_ops, const bool chain)
{
    EnumBuffers& B = p.B;
    FlatArgs fa{};
    fa.job = p.dj;
    fa.ins_pool = B.ins.as<char>();
    fa.ref = B.ref.as<char>();
    fa.ref_code = B.ref_code.as<uint8_t>() + F5_CODE_PAD;
    fa.ins_code = B.ins_code.as<uint8_t>();
    fa.ref_offset = p.in->ref_offset;
    fa.ref_len = p.in->ref_len;
    fa.n_reads = p.n;
    fa.n_cals = n_cals;
    fa.n_cals_on_device = n_cals_on_device ? 1 : 0;
    fa.pool = B.pool.as<PCal>();
    fa.list = B.sorted.as<int32_t>();
    fa.status = B.status.as<int32_t>();
    fa.read_off = B.read_off.as<int64_t>();
    fa.read_code = B.read_code.as<uint8_t>();
    fa.cal_off = cal_off;
    fa.win_begin = B.win_begin.as<int32_t>();
    fa.win_len = B.win_len.as<int32_t>();
    fa.hap_len = B.hap_len.as<int32_t>();
    fa.n_ins = B.n_ins.as<int32_t>();
    fa.ins_idx = B.ins_idx.as<int16_t>();
    fa.ins_off = B.ins_off.as<int32_t>();
    fa.n_ops = n_ops;
    fa.win_end = B.win_end.as<int32_t>();
    fa.ins_lo = B.ins_lo.as<int32_t>();
    fa.ins_hi = B.ins_hi.as<int32_t>();
    fa.n_seg8 = B.n_seg8.as<uint8_t>();
    fa.max_read_len = p.in->max_read_len;
    fa.ref_outside = B.counters.as<int32_t>() + CNT_DYN + DYN_REF_OUTSIDE;
    if (chain) {
        fa.cals = B.cals.as<PCal>();
        fa.hap_off = B.hap_off.as<int64_t>();
        fa.op_off = B.op_off.as<int64_t>();
        fa.hap_code = B.hap_code.as<uint8_t>();
        fa.ops = B.ops.as<sk_score_op>();
        fa.entries = B.entries.as<uint32_t>();
        fa.evmask = B.evmask.as<uint32_t>();
        fa.evmask_words = p.W;
        fa.colmat = B.colmat.as<uint8_t>();
        fa.colmat_off = B.colmat_off.as<int64_t>();
        fa.addmask = B.addmask.as<uint32_t>();
    }
    return fa;
}

FusedScoreArgs fused_args(const JobPlan& p, const FlatArgs& fa)
{
    EnumBuffers& B = p.B;
    FusedScoreArgs fs;
    fs.f = fa;
    fs.read_qual = B.read_qual.as<uint8_t>();
    fs.tab = sk_ctx().dev_tables;
    fs.scores = B.scores.as<double>();
    fs.err = sk_ctx().dev_error_flags;
    fs.n_unhandled = B.counters.as<int32_t>() + CNT_UNHANDLED;
    fs.queue = B.counters.as<unsigned>() + CNT_QUEUE;
    fs.write_cals = 0;
    fs.dbg = nullptr;
    fs.tail_order = nullptr; // (plan_tail)
    fs.tail_first = fs.tail_n = 0;
    // $SK_F5_SHARE = 0: no round sharing (experiments and tests; read once)
    static const bool share = [] { const char* e = std::getenv("SK_F5_SHARE"); return !(e && std::strcmp(e, "0") == 0); }();
    fs.share = share ? 1 : 0;
    fs.shared_rounds = B.counters.as<unsigned>() + CNT_SHARED;
    return fs;
}

// the table of F5's last hand-outs, built on the job's stream from cal_off (after pool_layout_kernel, before F5) and named in the launch's
// arguments.  A job that fits the grid makes no draw and gets no launch here; nor does any job with the shift off.  The table's buffer
// is reserved with the job's others (plan_job): nothing is allocated between the submissions of a sequence.
void plan_tail(const JobPlan& p, FusedScoreArgs& fs)
{
    EnumBuffers& B = p.B;
    const int W = f5_grid(p.n, fs.f.max_read_len).waves();
    const int shift = f5_tail_shift(W), T = f5_tail_window(p.n, W, shift); // (T <= min(n, F5_TAIL_MAX): f5_tail_shift)
    if (T == 0) return;
    launch_tail_order(p.st, TailArgs{ fs.f.cal_off, p.n - T, T, shift, B.tail_order.as<int32_t>() });
    ++g_tail_launches;
    fs.tail_order = B.tail_order.as<int32_t>();
    fs.tail_first = uint32_t(p.n - T);
    fs.tail_n = uint32_t(T);
}

// stage 3's arrays: per candidate alignment (n_cals: the count, or a capacity), per base, a record per read
int reserve_stage3(EnumBuffers& B, const int n, const int64_t n_bases, const int32_t n_cals)
{
    if (reserve_dev({ { B.s3_order, 4 * size_t(n_cals) }, { B.s3_smooth, 8 * size_t(n_cals) }, { B.s3_flag, size_t(n_cals) },
                      { B.s3_rm_type, size_t(n_bases) }, { B.s3_rm_pos, 4 * size_t(n_bases) }, { B.s3_key, 16 * size_t(n_cals) },
                      { B.s3_sorted_score, 8 * size_t(n_cals) }, { B.s3_sorted_hash, 4 * size_t(n_cals) }, { B.s3_next_same, 4 * size_t(n_cals) },
                      { B.s3_removed, size_t(n_cals) }, { B.s3_range_end, 4 * size_t(n_cals) }, { B.s3_out, sizeof(sk3::Out) * size_t(n) } }))
        return 1;
    return reserve_pinned({ { B.h_s3_out, sizeof(sk3::Out) * size_t(n) } });
}

// cals, slot: the records in set order and null -- or the pool the search left its leaves in and each alignment's slot there;
// skip_if: null, or F5's count of the reads it turned down (nothing runs when it is not zero: the scores are incomplete).
// What is a launch's own (its list, the capacity in LDS) is launch_stage3's
Stage3Args stage3_args(const JobPlan& p, const FlatArgs& fa, const PCal* cals, const int32_t* slot, const int32_t* skip_if)
{
    EnumBuffers& B = p.B;
    Stage3Args s3{};
    s3.tab.tab = p.dj.tab;
    s3.tab.r2i = B.r2i.as<double>();
    s3.tab.i2r = B.i2r.as<double>();
    s3.tab.orig = B.orig.as<int32_t>();
    s3.tab.n_tab = p.in->n_tab;
    s3.tab.max_indel_size = p.in->max_indel_size;
    s3.tab.consulted = p.dj.consulted;
    s3.opt = p.in->stage3_opt;
    s3.n_reads = p.n;
    s3.status = fa.status;
    s3.cal_off = fa.cal_off;
    s3.cals = cals;
    s3.slot = slot;
    s3.scores = B.scores.as<double>();
    s3.read_off = fa.read_off;
    s3.read_code = fa.read_code;
    s3.map_level = B.map_level.as<int32_t>();
    s3.order = B.s3_order.as<int32_t>();
    s3.smooth = B.s3_smooth.as<double>();
    s3.flag = B.s3_flag.as<uint8_t>();
    s3.rm_type = B.s3_rm_type.as<uint8_t>();
    s3.rm_pos = B.s3_rm_pos.as<int32_t>();
    s3.key = B.s3_key.as<uint32_t>();
    s3.sorted_score = B.s3_sorted_score.as<double>();
    s3.sorted_hash = B.s3_sorted_hash.as<uint32_t>();
    s3.next_same = B.s3_next_same.as<int32_t>();
    s3.removed = B.s3_removed.as<uint8_t>();
    s3.range_end = B.s3_range_end.as<int32_t>();
    s3.out = B.s3_out.as<sk3::Out>();
    s3.skip_if = skip_if;
    return s3;
}

// one of stage 3's two launches, WAVES wavefronts a read: `blocks` reads of `list` (n_list null), or a block per read of the job with the
// list's length on the device (n_list; list_step -1: the list is filled from the back)
template <int WAVES>
void launch_stage3(hipStream_t st, Stage3Args s3, const int blocks, const int32_t* list, const int32_t* n_list, const int list_step, const int lds_cals)
{
    s3.list = list;
    s3.n_list = n_list;
    s3.list_step = list_step;
    s3.lds_cals = lds_cals;
    SK_LAUNCH(stage3_kernel<WAVES>, dim3(blocks), dim3(64 * WAVES), size_t(lds_cals) * (8 + 8 + 4 + 4 + 4 + 4 + 1 + 1) + 8, st, s3);
}

// warn as the caller reads it: a byte per read, made in place (byte r is written after int r was read)
const uint8_t* narrow_warn(EnumBuffers& B, const int n)
{
    uint8_t* w8 = reinterpret_cast<uint8_t*>(B.h_warn.p);
    const int32_t* w32 = B.h_warn.as<int32_t>();
    for (int r = 0; r < n; ++r) w8[r] = uint8_t(w32[r]);
    return w8;
}

// ---- what sk_enum_device_rescore replays
int64_t job_cells(const SkEnumInput* in, const int32_t* h_cal_off)
{
    int64_t cells = 0;
    for (int r = 0; r < in->n_reads; ++r) cells += (in->read_off[r + 1] - in->read_off[r]) * int64_t(h_cal_off[r + 1] - h_cal_off[r]);
    return cells;
}
void remember_fused(const JobPlan& p, const FusedScoreArgs& fs, const int32_t n_cals)
{
    g_last.fused = true;
    g_last.fs = fs;
    g_last.fs.f.n_cals = n_cals;       // (the count, where the run knew a capacity)
    g_last.fs.f.ref_outside = nullptr; // (a repeat for the clock counts nothing)
    g_last.n = p.n;
    g_last.n_cals = n_cals;
    g_last.scores = fs.scores;
    g_last.cells = job_cells(p.in, p.B.h_cal_off.as<int32_t>());
    g_last.valid = true;
}
void remember_staged(const JobPlan& p, const FlatArgs& fa, const sk_align_batch& d, const size_t colmat_bytes)
{
    g_last.fused = false;
    g_last.fa = fa;
    g_last.fa.ref_outside = nullptr;
    g_last.d = d;
    g_last.mask_bytes = p.mask_bytes;
    g_last.colmat_bytes = colmat_bytes;
    g_last.n = p.n;
    g_last.n_cals = fa.n_cals;
    g_last.scores = p.B.scores.as<double>();
    g_last.cells = job_cells(p.in, p.B.h_cal_off.as<int32_t>());
    g_last.valid = true;
}

// ---- the job as one fixed sequence: ~20 submissions, no host decision between them, ONE wait.  Everything the host computes between the
// staged run's waits is computed by job_scan_kernel; every buffer is sized by a capacity known now; launches whose size the host does
// not know cover the capacity with a grid-stride loop (or a block per read of the job that leaves at once).
// *redo is set when the sequence's assumptions did not hold for this job and nothing of `out` is valid: the caller runs it again the staged way
int run_one_wait(const JobPlan& p, SkEnumOutput* out, bool* redo)
{
    const auto t_setup = std::chrono::steady_clock::now();
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    const int32_t n_cap = int32_t(p.pool_cap); // leaves, grouped leaves and candidate alignments are all at most this many
    if (reserve_dev({ { B.grouped, 4 * size_t(n_cap) }, { B.ghash, 4 * size_t(n_cap) }, { B.gkey, 16 * size_t(n_cap) }, { B.dup, size_t(n_cap) },
                      { B.sorted, 4 * size_t(n_cap) }, { B.n_seg8, size_t(n_cap) }, { B.scores, 8 * size_t(n_cap) }, { B.s3_list, 4 * size_t(n) } }) ||
        reserve_stage3(B, n, p.n_bases, n_cap))
        return 1;
    int32_t* const dyn = B.counters.as<int32_t>() + CNT_DYN;

    // E1: root + the levels up to the deepest order of the job (+ 2: indels that join an order on the way); whether calls were left
    // for a deeper level is looked at on the device (scan 1) and reported with the results
    const EnumArgs ea = enum_args(p, true);
    int n_levels = std::min(p.max_order + 3, int(SEARCH_LEVELS));
    if (const char* e = std::getenv("SK_ENUM_TEST_LEVELS")) // tests: too few levels, so that the device reports it and the job runs again
        if (std::atoi(e) > 0) n_levels = std::min(n_levels, std::atoi(e));
    // (a level of this job has at most a few frames per read: blocks beyond that would only read the count and leave)
    launch_search(p, ea, -1, n_levels, int(std::min<int64_t>(std::min<int64_t>((p.frame_cap + 63) / 64, 1024), std::max<int64_t>(n, 16))));
    // scan 1: raw_off
    ScanArgs sc{};
    sc.n_reads = n;
    sc.status = ea.status;
    sc.count = ea.n_raw;
    sc.off = B.raw_off.as<int32_t>();
    sc.dyn = dyn;
    sc.level_count = ea.level_count;
    sc.first_level_not_launched = (n_levels >= SEARCH_LEVELS) ? -1 : n_levels;
    sc.n_leaves = ea.n_leaves;
    sc.pool_cap = n_cap;
    SK_LAUNCH(job_scan_kernel<false>, dim3(1), dim3(1024), 0, st, sc);
    // E2
    const SetArgs sa = set_args(p, n_cap, ea.n_leaves, B.cal_off_z.as<int32_t>());
    // (grids for counts the host has not seen: enough blocks for ~64 leaves per read, the loops cover the rest)
    const int e2_blocks = int(std::min<int64_t>(std::max<int64_t>((int64_t(n) * 64 + 255) / 256, 8), 2048));
    SK_LAUNCH(group_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    SK_LAUNCH(dedupe_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    // scan 2: cal_off, stage 3's lists
    sc.count = B.n_uniq.as<int32_t>();
    sc.off = B.cal_off_z.as<int32_t>();
    sc.list = B.s3_list.as<int32_t>();
    sc.light_cals = p.light_cals;
    SK_LAUNCH(job_scan_kernel<true>, dim3(1), dim3(1024), 0, st, sc);
    SK_LAUNCH(rank_kernel, dim3(e2_blocks), dim3(256), 0, st, sa);
    // L1
    const FlatArgs fa = flat_args(p, n_cap, true, B.cal_off_z.as<int32_t>(), nullptr, false);
    SK_LAUNCH(pool_bounds_kernel, dim3(e2_blocks), dim3(256), 0, st, fa);
    SK_LAUNCH(pool_layout_kernel, dim3((n + 63) / 64), dim3(64), 0, st, fa);
    // F5, the table of its last hand-outs first
    FusedScoreArgs fs = fused_args(p, fa);
    plan_tail(p, fs);
    launch_flatten_score(n, st, fs);
    // S3: a block per read of the job in either launch; the blocks past a list's length leave at once
    // (the largest read of the heavy list is not known here: LDS for the most a block holds)
    const Stage3Args s3 = stage3_args(p, fa, fa.pool, fa.list, fs.n_unhandled);
    launch_stage3<1>(st, s3, n, B.s3_list.as<int32_t>(), dyn + DYN_N_LIGHT, 1, p.light_cals);
    launch_stage3<4>(st, s3, n, B.s3_list.as<int32_t>() + (n - 1), dyn + DYN_N_HEAVY, -1, p.lds_cals);
    SK_HIP(skrt::getLastError());
    // the results: the zero arena whole (counters + the scans' numbers, warn, n_raw, status, ..., consulted, cal_off) and stage 3's records
    const size_t out_bytes = sizeof(sk3::Out) * size_t(n);
    if (stage_by_kernel()) {
        const uint32_t n_a = uint32_t(p.zero_bytes / 16), n_b = uint32_t((out_bytes + 15) / 16); // (buffers are reserved with slack)
        const int blocks = int(std::min<size_t>(std::max<size_t>((std::max(p.zero_bytes, out_bytes) / 16 + 255) / 256, 1), 256));
        SK_LAUNCH(job_stage_out_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint4*>(B.zero_arena.p), static_cast<uint4*>(B.h_zero_arena.p), n_a,
                  static_cast<const uint4*>(B.s3_out.p), static_cast<uint4*>(B.h_s3_out.p), n_b);
        SK_HIP(skrt::getLastError());
    } else {
        if (copy_down(st, B.h_zero_arena, B.zero_arena, p.zero_bytes) || copy_down(st, B.h_s3_out, B.s3_out, out_bytes)) return 1;
    }
    const auto t_submitted = std::chrono::steady_clock::now();
    SK_HIP(skrt::streamSynchronize(st));
    const auto t_waited = std::chrono::steady_clock::now();
    g_job_seconds.setup += std::chrono::duration<double>(t_setup - p.t_begin).count();
    g_job_seconds.submit += std::chrono::duration<double>(t_submitted - t_setup).count();
    g_job_seconds.wait += std::chrono::duration<double>(t_waited - t_submitted).count();
    p.lap("one sequence");
    const int32_t* h_counters = B.h_counters.as<int32_t>();
    const int32_t* const h_dyn = h_counters + CNT_DYN;
    g_shared_rounds += h_counters[CNT_SHARED]; // (of this launch, whether the job is run again or not)
    g_late_turn_downs += h_counters[CNT_SHARED + 1];
    if (h_dyn[DYN_FLAGS] != 0 || h_counters[CNT_UNHANDLED] > 0) {
        if (p.timing)
            std::fprintf(stderr, "[enum-dev] one sequence: flags %d, reads outside F5's form %d -> the staged chain\n", h_dyn[DYN_FLAGS], h_counters[CNT_UNHANDLED]);
        *redo = true;
        return 0;
    }
    ++g_jobs_one_wait;
    out->warn = narrow_warn(B, n);
    int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    std::memcpy(h_cal_off, B.h_cal_off_z.p, 4 * size_t(n + 1));
    const int32_t n_cals = h_cal_off[n];
    g_n_cals = n_cals;
    g_cals_pool = fa.pool;
    g_cals_list = fa.list;
    g_scores = B.scores.as<double>();
    out->cals = nullptr;   // (in the pool: sk_enum_device_fetch_cals)
    out->scores = nullptr; // (on the device: sk_enum_device_fetch_scores -- the host needs them only for a read stage 3 turned down)
    out->stage3 = B.h_s3_out.as<sk3::Out>();
    out->ref_reads_outside = h_dyn[DYN_REF_OUTSIDE];
    remember_fused(p, fs, n_cals);
    if (p.timing)
        std::fprintf(stderr, "[enum-dev] one sequence: %d reads, %d levels launched, %d leaves, %d candidate alignments, stage 3 lists %d + %d\n", n, n_levels,
                     h_counters[CNT_LEAVES], n_cals, h_dyn[DYN_N_LIGHT], h_dyn[DYN_N_HEAVY]);
    return 0;
}

// ---- the staged run

// what follows the scores in either chain: the scores' way back, stage 3 (lists made here: the host has the counts).  cals_in_set_order:
// the staged chain left the records in B.cals (flatten_kernel); else they are where the search put them, and F5 counted the reads it turned
// down: stage 3 then has nothing to work on -- the staged chain scores the job and this runs again
int after_scores(const JobPlan& p, SkEnumOutput* out, const FlatArgs& fa, const bool cals_in_set_order)
{
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    if (copy_down(st, B.h_scores, B.scores, 8 * size_t(fa.n_cals))) return 1;
    out->scores = B.h_scores.as<double>();
    if (!p.in->want_stage3) return 0;
    if (reserve_stage3(B, n, p.n_bases, fa.n_cals)) return 1;
    const Stage3Args s3 = cals_in_set_order ? stage3_args(p, fa, fa.cals, nullptr, nullptr)
                                            : stage3_args(p, fa, fa.pool, fa.list, B.counters.as<int32_t>() + CNT_UNHANDLED);
    // two launches: reads with few candidate alignments (small LDS, many wavefronts per CU) and the others
    if (reserve_dev({ { B.s3_list, 4 * size_t(n) } }) || reserve_pinned({ { B.h_s3_list, 4 * size_t(n) } })) return 1;
    int32_t* h_list = B.h_s3_list.as<int32_t>();
    const int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    int n_light = 0, n_heavy = 0, max_cals = 0;
    for (int r = 0; r < n; ++r) {
        const int k = h_cal_off[r + 1] - h_cal_off[r];
        if (k <= p.light_cals) h_list[n_light++] = r;
        else {
            h_list[n - 1 - n_heavy++] = r;
            max_cals = std::max(max_cals, k);
        }
    }
    if (copy_up(st, B.s3_list, h_list, 4 * size_t(n))) return 1;
    if (n_light > 0) launch_stage3<1>(st, s3, n_light, B.s3_list.as<int32_t>(), nullptr, 1, p.light_cals);
    if (n_heavy > 0) {
        const int32_t* heavy = B.s3_list.as<int32_t>() + (n - n_heavy);
        const int lds_cals = std::min(max_cals, p.lds_cals); // (a read with more uses the arrays in HBM)
        // four wavefronts per read: the loops over the read's alignments go four times as wide, lane 0's share stays
        static const bool one_wave = std::getenv("SK_STAGE3_ONE_WAVE") != nullptr; // (diagnostics)
        if (one_wave) launch_stage3<1>(st, s3, n_heavy, heavy, nullptr, 1, lds_cals);
        else launch_stage3<4>(st, s3, n_heavy, heavy, nullptr, 1, lds_cals);
    }
    if (p.timing)
        std::fprintf(stderr, "[enum-dev] stage 3: %d reads with at most %d candidate alignments, %d with more (up to %d)\n", n_light, p.light_cals, n_heavy, max_cals);
    SK_HIP(skrt::getLastError());
    if (copy_down(st, B.h_s3_out, B.s3_out, sizeof(sk3::Out) * size_t(n))) return 1;
    out->stage3 = B.h_s3_out.as<sk3::Out>();
    p.lap("S3 stage 3");
    return 0;
}

// the staged chain's flattening and scoring (L2, F1-F3, A1c: ops, entries, column words through HBM) and, with scores, what follows them.
// It leaves the records in set order in B.cals.  layout: the job's FlatArgs as L1 ran with them
int run_chain(const JobPlan& p, SkEnumOutput* out, const FlatArgs& layout)
{
    const SkEnumInput* in = p.in;
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    const int32_t n_cals = layout.n_cals;
    const int32_t* h_status = B.h_status.as<int32_t>();
    const int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    if (reserve_dev({ { B.cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
    g_cals_gathered = true; // (flatten_kernel below writes them)
    if (n_cals > 0) {
        SK_LAUNCH(op_count_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, layout);
        SK_HIP(skrt::getLastError());
    }
    if (fetch_zero(p, B.status, B.hap_len, 4 * size_t(n))) return 1; // status, hap_len (the host has made bytes of its copy of warn)
    if (copy_down(st, B.h_n_ops, B.n_ops, 4 * size_t(n_cals))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    p.lap("L1+L2 layout");

    const int32_t* h_hap_len = B.h_hap_len.as<int32_t>();
    const int32_t* h_n_ops = B.h_n_ops.as<int32_t>();
    int64_t* h_hap_off = B.h_hap_off.as<int64_t>();
    int64_t* h_op_off = B.h_op_off.as<int64_t>();
    h_hap_off[0] = 0;
    h_op_off[0] = 0;
    int32_t max_hap = 1;
    for (int r = 0; r < n; ++r) {
        const int32_t c0 = h_cal_off[r], c1 = h_cal_off[r + 1];
        h_hap_off[r + 1] = h_hap_off[r] + ((c1 > c0) ? h_hap_len[r] : 0);
        if (c1 > c0) max_hap = std::max(max_hap, h_hap_len[r]);
        const bool ok = (h_status[r] == ST_OK); // (a read turned down by L1/L2 keeps its slots in the batch, with no ops)
        for (int32_t c = c0; c < c1; ++c) h_op_off[c + 1] = h_op_off[c] + (ok ? h_n_ops[c] : 0);
    }
    const int64_t n_hap = h_hap_off[n], ops_total = h_op_off[n_cals];

    if (reserve_dev({ { B.hap_code, size_t(n_hap) + 16 }, { B.ops, sizeof(sk_score_op) * size_t(ops_total) }, { B.entries, 4 * (size_t(ops_total) + 2 * size_t(n_cals) + 1) } }) ||
        reserve_pinned({ { B.h_colmat_off, 8 * size_t(n + 1) } }))
        return 1;
    int64_t* h_colmat_off = B.h_colmat_off.as<int64_t>();
    h_colmat_off[0] = 0;
    for (int r = 0; r < n; ++r)
        h_colmat_off[r + 1] = h_colmat_off[r] + ((in->read_off[r + 1] - in->read_off[r] + 7) / 8) * int64_t(h_cal_off[r + 1] - h_cal_off[r]);
    const size_t colmat_bytes = 4 * size_t(h_colmat_off[n]) + 16;
    if (reserve_dev({ { B.colmat, colmat_bytes }, { B.colmat_off, 8 * size_t(n + 1) } })) return 1;
    if (n_cals == 0) return 0;

    if (copy_up(st, B.hap_off, h_hap_off, 8 * size_t(n + 1)) || copy_up(st, B.op_off, h_op_off, 8 * size_t(n_cals + 1))) return 1;
    SK_HIP(skrt::memsetAsync(B.mask_arena.p, 0, p.mask_bytes, st)); // evmask, addmask
    SK_HIP(skrt::memsetAsync(B.colmat.p, SK_SEL_NONE | (SK_SEL_NONE << 4), colmat_bytes, st));
    if (copy_up(st, B.colmat_off, h_colmat_off, 8 * size_t(n + 1))) return 1;
    const FlatArgs fa = flat_args(p, n_cals, false, layout.cal_off, layout.n_ops, true);
    SK_LAUNCH(pool_fill_kernel, dim3(n), dim3(64), 0, st, fa);
    SK_LAUNCH(flatten_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, fa);
    SK_HIP(skrt::getLastError());
    if (p.with_stage3) out->cals = nullptr; // (they stay here: sk_enum_device_fetch_cals)
    else if (copy_down(st, B.h_cals, B.cals, sizeof(PCal) * size_t(n_cals))) return 1;
    if (!in->want_scores) return 0;
    // F3: a wave per read ($SK_F3_KERNEL = thread pins the thread-per-alignment form; the tests run both)
    const bool f3_thread = (std::getenv("SK_F3_KERNEL") != nullptr && std::strcmp(std::getenv("SK_F3_KERNEL"), "thread") == 0);
    if (f3_thread) SK_LAUNCH(entries_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, fa);
    else SK_LAUNCH(entries_wave_kernel, dim3(n), dim3(64), 0, st, fa);
    SK_HIP(skrt::getLastError());
    p.lap("F1-F3 flatten");
    sk_align_batch d{};
    d.n_reads = n;
    d.n_cals = n_cals;
    d.n_ops = ops_total;
    d.read_off = B.read_off.as<int64_t>();
    d.read_code = B.read_code.as<uint8_t>();
    d.read_qual = B.read_qual.as<uint8_t>();
    d.hap_off = fa.hap_off;
    d.hap_code = fa.hap_code;
    d.cal_off = fa.cal_off;
    d.op_off = fa.op_off;
    d.ops = fa.ops;
    d.max_read_len = in->max_read_len;
    d.max_hap_len = max_hap;
    d.entries = fa.entries;
    d.evmask = fa.evmask;
    d.evmask_words = p.W;
    d.colmat = B.colmat.as<uint32_t>();
    d.colmat_off = fa.colmat_off;
    d.addmask = fa.addmask;
    if (sk_score_alignments_launch_hostleg(&d, B.scores.as<double>(), st)) return 1;
    p.lap("A1 score");
    remember_staged(p, fa, d, colmat_bytes);
    return after_scores(p, out, fa, true);
}

// a wait after the search, one after the sets and one at the end; buffers sized by the counts that came back.  The scores come from F5
// or, when the job holds a read F5 turns down, when the host wants the alignments without scores and with $SK_A5_FUSED=0 (tests: both
// chains), from the staged chain
int run_staged(const JobPlan& p, SkEnumOutput* out)
{
    const SkEnumInput* in = p.in;
    EnumBuffers& B = p.B;
    hipStream_t st = p.st;
    const int n = p.n;
    ++g_jobs_staged;
    // ---- E1: the search, one launch per depth.  A call at depth d expands indel order[d]; a call at depth n_order is a leaf.  A read's
    // order as it arrives says how deep its search goes unless an alignment reaches indels beyond the read's first range (they join the
    // order): the levels up to the deepest order of the job (+1) go out at once, the level counts that come back with the results say
    // whether more are needed
    const EnumArgs ea = enum_args(p, false);
    const int level_blocks = int(std::min<int64_t>((p.frame_cap + 63) / 64, 1024));
    launch_search(p, ea, -1, 0, level_blocks);
    for (int done = 0, batch = std::min(std::max(p.max_order + 2, 3), int(SEARCH_LEVELS));; batch = 4) {
        const int upto = std::min(done + batch, int(SEARCH_LEVELS));
        launch_search(p, ea, done, upto, level_blocks);
        done = upto;
        SK_HIP(skrt::getLastError());
        if (fetch_zero(p, B.counters, B.status, 4 * size_t(n))) return 1; // counters, warn, n_raw, status
        SK_HIP(skrt::streamSynchronize(st));
        if (done >= SEARCH_LEVELS || B.h_counters.as<int32_t>()[CNT_LEVELS + done] == 0) break;
    }
    p.lap("E1 search (all depths)");
    const int32_t* h_status = B.h_status.as<int32_t>();
    const int32_t* h_counters = B.h_counters.as<int32_t>();
    const int32_t n_leaves = std::min<int32_t>(h_counters[CNT_LEAVES], int32_t(p.pool_cap));
    if (p.timing) {
        long long calls = 0;
        int deepest = 0;
        for (int d = 0; d <= SEARCH_LEVELS; ++d) {
            calls += h_counters[CNT_LEVELS + d];
            if (h_counters[CNT_LEVELS + d]) deepest = d;
        }
        std::fprintf(stderr, "[enum-dev] search calls %lld, deepest level %d, leaves found %d\n", calls, deepest, n_leaves);
    }
    out->warn = narrow_warn(B, n);

    // ---- E2: leaves -> each read's set
    const int32_t* h_n_raw = B.h_n_raw.as<int32_t>();
    int32_t* h_raw_off = B.h_raw_off.as<int32_t>();
    h_raw_off[0] = 0;
    for (int r = 0; r < n; ++r) h_raw_off[r + 1] = h_raw_off[r] + ((h_status[r] == ST_OK) ? h_n_raw[r] : 0);
    const int32_t n_grouped = h_raw_off[n];
    if (reserve_dev({ { B.grouped, 4 * size_t(n_grouped) }, { B.ghash, 4 * size_t(n_grouped) }, { B.gkey, 16 * size_t(n_grouped) }, { B.dup, size_t(n_grouped) },
                      { B.sorted, 4 * size_t(n_grouped) } }))
        return 1;
    const SetArgs sa = set_args(p, n_leaves, nullptr, B.cal_off.as<int32_t>());
    if (copy_up(st, B.raw_off, h_raw_off, 4 * size_t(n + 1))) return 1;
    if (n_grouped > 0) {
        SK_LAUNCH(group_kernel, dim3((n_leaves + 255) / 256), dim3(256), 0, st, sa);
        SK_LAUNCH(dedupe_kernel, dim3((n_grouped + 255) / 256), dim3(256), 0, st, sa);
        SK_HIP(skrt::getLastError());
    }
    if (fetch_zero(p, B.n_uniq, B.n_uniq, 4 * size_t(n))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    const int32_t* h_n_uniq = B.h_n_uniq.as<int32_t>();
    int32_t* h_cal_off = B.h_cal_off.as<int32_t>();
    for (int r = 0; r < n; ++r) h_cal_off[r + 1] = h_cal_off[r] + ((h_status[r] == ST_OK) ? h_n_uniq[r] : 0);
    const int32_t n_cals = h_cal_off[n];
    if (copy_up(st, B.cal_off, h_cal_off, 4 * size_t(n + 1))) return 1;
    if (n_grouped > 0) {
        SK_LAUNCH(rank_kernel, dim3((n_grouped + 255) / 256), dim3(256), 0, st, sa);
        SK_HIP(skrt::getLastError());
    }
    p.lap("E2 sets");

    // ---- L1: layout of the batch
    if (reserve_dev({ { B.n_ops, 4 * size_t(n_cals) }, { B.op_off, 8 * size_t(n_cals + 1) }, { B.n_seg8, size_t(n_cals) }, { B.scores, 8 * size_t(n_cals) } }) ||
        reserve_pinned({ { B.h_n_ops, 4 * size_t(n_cals) }, { B.h_op_off, 8 * size_t(n_cals + 1) }, { B.h_scores, 8 * size_t(n_cals) } }))
        return 1;
    if (!p.with_stage3 && reserve_pinned({ { B.h_cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
    const FlatArgs fa = flat_args(p, n_cals, false, B.cal_off.as<int32_t>(), B.n_ops.as<int32_t>(), false);
    // (byte patterns: 0x7f7f7f7f is large enough to stand for "no lower bound yet", 0x80808080 is below any position / index)
    SK_HIP(skrt::memsetAsync(B.minmax_arena.p, 0x7f, p.minmax_split, st));                                                                // win_begin, ins_lo
    SK_HIP(skrt::memsetAsync(static_cast<char*>(B.minmax_arena.p) + p.minmax_split, 0x80, p.minmax_bytes - p.minmax_split, st)); // win_end, ins_hi
    if (n_cals > 0) SK_LAUNCH(pool_bounds_kernel, dim3((n_cals + 255) / 256), dim3(256), 0, st, fa);
    SK_LAUNCH(pool_layout_kernel, dim3((n + 63) / 64), dim3(64), 0, st, fa);
    SK_HIP(skrt::getLastError());
    out->cals = B.h_cals.as<PCal>();
    g_n_cals = n_cals;
    g_cals_pool = fa.pool;
    g_cals_list = fa.list;

    // ---- flattening + scoring.  The default is F5 (flatten_score_kernel): one launch from the records to the scores, no layout pass
    // and no host wait before stage 3; it reads the records where the search left them
    const bool fused_enabled = !(std::getenv("SK_A5_FUSED") != nullptr && std::strcmp(std::getenv("SK_A5_FUSED"), "0") == 0);
    bool chain = !(fused_enabled && in->want_scores && n_cals > 0);
    if (!chain) {
        FusedScoreArgs fs = fused_args(p, fa);
        plan_tail(p, fs); // (the table of F5's last hand-outs)
        launch_flatten_score(n, st, fs);
        SK_HIP(skrt::getLastError());
        p.lap("F5 flatten + score");
        if (in->want_stage3) {
            out->cals = nullptr; // (they stay here, in the pool: sk_enum_device_fetch_cals gathers them when the host asks)
        } else {
            if (reserve_dev({ { B.cals, sizeof(PCal) * size_t(n_cals) } })) return 1;
            SK_LAUNCH(gather_cals_kernel, dim3((n_cals + 63) / 64), dim3(64), 0, st, fa.pool, fa.list, n_cals, B.cals.as<PCal>());
            SK_HIP(skrt::getLastError());
            g_cals_gathered = true;
            if (copy_down(st, B.h_cals, B.cals, sizeof(PCal) * size_t(n_cals))) return 1;
        }
        remember_fused(p, fs, n_cals);
        if (after_scores(p, out, fa, false)) return 1;
        if (fetch_zero(p, B.counters, B.counters, 4 * size_t(N_COUNTERS))) return 1; // (n_unhandled)
        if (fetch_zero(p, B.status, B.status, 4 * size_t(n))) return 1;             // (F5 may have turned reads down: ST_FAIL)
        SK_HIP(skrt::streamSynchronize(st));
        chain = B.h_counters.as<int32_t>()[CNT_UNHANDLED] > 0; // a read outside F5's form: the staged chain over the job
    }
    if (chain && run_chain(p, out, fa)) return 1;
    if (fetch_zero(p, B.consulted, B.consulted, size_t(in->n_tab))) return 1;
    if (fetch_zero(p, B.counters, B.counters, 4 * size_t(N_COUNTERS))) return 1;
    SK_HIP(skrt::streamSynchronize(st));
    // (when F5 turned a read down both chains filled the pools: the count may be double -- what matters to the caller is zero or not)
    out->ref_reads_outside = B.h_counters.as<int32_t>()[CNT_DYN + DYN_REF_OUTSIDE];
    g_shared_rounds += B.h_counters.as<int32_t>()[CNT_SHARED]; // (the job's one F5 launch, if it had one: the counters' last fetch)
    g_late_turn_downs += B.h_counters.as<int32_t>()[CNT_SHARED + 1];
    p.lap("done");
    return 0;
}
} // namespace

// A job with the whole read path on the device (scores + stage 3) and F5 enabled runs as one fixed sequence with one wait; a job for
// which the sequence's assumptions do not hold (reported by the device with the results), one too large for capacity-sized buffers, and
// a caller that wants the alignments or the scores on the host run the staged way (a wait after the search, one after the sets, one at
// the end).  $SK_ENUM_ONE_WAIT = 0 pins the staged way (tests run both).
extern "C" int sk_enum_device_run(const SkEnumInput* in, SkEnumOutput* out)
{
    const bool enabled = !(std::getenv("SK_ENUM_ONE_WAIT") != nullptr && std::strcmp(std::getenv("SK_ENUM_ONE_WAIT"), "0") == 0);
    const bool fused_enabled = !(std::getenv("SK_A5_FUSED") != nullptr && std::strcmp(std::getenv("SK_A5_FUSED"), "0") == 0);
    if (enabled && fused_enabled && in && in->want_scores && in->want_stage3 && in->n_reads > 0 && in->n_reads <= ONE_WAIT_MAX_READS &&
        in->max_read_len <= F5_MAX_READ) {
        JobPlan p;
        bool redo = false;
        const int rc = start_job(in, out, true, p) || run_one_wait(p, out, &redo);
        if (rc != 0 || !redo) return rc;
        ++g_jobs_one_wait_redone;
    }
    JobPlan p; // (a job run again is prepared again from the start: a new generation, another layout of the zero arena)
    if (start_job(in, out, false, p)) return 1;
    return p.n == 0 ? 0 : run_staged(p, out);
}

// diagnostics ($SK_F5_TIMING): where a wave of F5 spends its cycles on the last run's job, and how the kernel's time grows with the grid
static int f5_timing_report(hipStream_t st)
{
    FusedScoreArgs fs = g_last.fs;
    const size_t nb = size_t(g_last.n) * F5_STAMPS;
    SkDevBuf dbg; // (this report's own: dropped below)
    if (dbg.reserve(nb * 8)) return 1;
    unsigned long long* d = dbg.as<unsigned long long>();
    SK_HIP(skrt::memsetAsync(d, 0, nb * 8, st));
    fs.dbg = d;
    unsigned helped[2] = { 0, 0 }; // the job's count of helped rounds before and after this launch
    SK_HIP(skrt::memcpyAsync(&helped[0], fs.shared_rounds, 4, hipMemcpyDeviceToHost, st));
    launch_flatten_score(g_last.n, st, fs);
    SK_HIP(skrt::memcpyAsync(&helped[1], fs.shared_rounds, 4, hipMemcpyDeviceToHost, st));
    std::vector<unsigned long long> h(nb);
    SK_HIP(skrt::memcpyAsync(h.data(), d, nb * 8, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    dbg.drop();
    { // the rounds of the reads that were scored (a stamped read: its owner went through all it claimed), by who scored them
        const int32_t* const cal_off = bufs().h_cal_off.as<int32_t>();
        long long by_owner = 0, implied = 0;
        for (int r = 0; r < g_last.n; ++r) {
            const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
            if (s[6] == 0) continue;
            by_owner += (long long)s[10];
            implied += (cal_off[r + 1] - cal_off[r] + 63) / 64;
        }
        std::fprintf(stderr, "[f5-timing] rounds: %lld scored by their owners + %u by helpers = %lld; cal_off implies %lld (sharing %s)\n", by_owner,
                     helped[1] - helped[0], by_owner + (long long)(helped[1] - helped[0]), implied, fs.share ? "on" : "off");
    }
    double sum[F5_STAMPS] = { 0 };
    unsigned long long first = ~0ull, last = 0;
    int nblk = 0, ndrawn = 0;
    for (int r = 0; r < g_last.n; ++r) {
        const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
        if (s[6] == 0) continue;
        ++nblk;
        first = std::min(first, s[0]);
        last = std::max(last, s[6]);
        sum[0] += double(s[1] - s[0]);
        for (int i = 2; i <= 5; ++i) sum[i] += double(s[i]);
        sum[7] += double(s[7]);
        sum[6] += double(s[6] - s[0]);
        sum[8] += double(s[8]);
        ndrawn += s[8] != 0;
    }
    for (const int grid : { 64, 256, 512, 1024, 1792, 2048, 4096 }) { // how the kernel's time grows with the blocks in flight
        if (grid > g_last.n) break;
        hipEvent_t a0, a1;
        SK_HIP(hipEventCreate(&a0));
        SK_HIP(hipEventCreate(&a1));
        FusedScoreArgs f2 = g_last.fs;
        f2.tail_n = 0; // (the table is the whole job's: these launches end before its window)
        launch_flatten_score(grid, st, f2);
        SK_HIP(hipEventRecord(a0, st));
        for (int k = 0; k < 5; ++k) launch_flatten_score(grid, st, f2);
        SK_HIP(hipEventRecord(a1, st));
        SK_HIP(hipEventSynchronize(a1));
        float ms = 0;
        SK_HIP(hipEventElapsedTime(&ms, a0, a1));
        std::fprintf(stderr, "[f5-timing] grid %d blocks: %.1f us per launch\n", grid, ms * 1000.f / 5.f);
        (void)hipEventDestroy(a0);
        (void)hipEventDestroy(a1);
    }
    if (nblk)
        std::fprintf(stderr, "[f5-timing] blocks %d: cycles per block: draw %.0f (%d drawn: %.0f each) prologue %.0f staging %.0f phaseA %.0f (walk %.0f) phaseB %.0f total %.0f = %.1f us by the 100 MHz counter (%.0f MHz); kernel span %llu cycles => %.1f blocks in flight\n",
                     nblk, sum[8] / nblk, ndrawn, sum[8] / std::max(1, ndrawn), sum[0] / nblk, sum[2] / nblk, sum[4] / nblk, sum[7] / nblk, sum[5] / nblk, sum[6] / nblk, sum[3] / nblk / 100.0,
                     sum[6] / std::max(1.0, sum[3]) * 100.0, last - first,
                     sum[6] / double(last - first));
    // the drain, by the 100 MHz counter (a read's start is its tenth stamp, its duration the fourth): when the last read was handed
    // out, when the launch's last read ended, and how long a slot stood empty at the end -- over the W reads that started last (the
    // last read of each of the grid's W waves, or nearly), the mean of (the launch's end - the read's end)
    std::vector<std::pair<unsigned long long, unsigned long long>> span; // (start, end) of every stamped read
    for (int r = 0; r < g_last.n; ++r) {
        const unsigned long long* s = &h[size_t(r) * F5_STAMPS];
        if (s[6] != 0) span.emplace_back(s[9], s[9] + s[3]);
    }
    if (!span.empty()) {
        std::sort(span.begin(), span.end());
        const unsigned long long w0 = span.front().first;
        unsigned long long w1 = 0;
        for (const auto& x : span) w1 = std::max(w1, x.second);
        const size_t W = size_t(f5_grid(g_last.n, fs.f.max_read_len).waves()), n_last = std::min(W, span.size());
        double idle = 0;
        for (size_t i = span.size() - n_last; i < span.size(); ++i) idle += double(w1 - span[i].second);
        std::fprintf(stderr, "[f5-timing] drain: tail window %u hand-outs; last read handed out at %.1f us, last read ended at %.1f us; over the %zu reads that started last a slot stood empty for %.1f us on average\n",
                     fs.tail_n, double(span.back().first - w0) / 100.0, double(w1 - w0) / 100.0, n_last, idle / double(n_last) / 100.0);
    }
    return 0;
}

// Measurement entry (bench.py's a5 leg): flattening AND scoring of the candidate alignments the last run left on the device, the way
// that run did it -- F5 (one launch from the records to the scores), or, for a job scored by the staged chain, pool bytes, ops,
// transition entries, masks and column words rebuilt from the PCal records (F1-F3), then the scoring kernel over them --
// `reps` times, timed with events on the library's stream.  This is what sk_enum_device_run does between the sets (E2) and stage 3,
// minus the layout pass (L1/L2: per-read pool bounds and op counts, whose results -- offsets -- a steady state already has).
extern "C" int sk_enum_device_rescore(const int32_t reps, float* out_ms, int32_t* out_n_reads, int32_t* out_n_cals, int64_t* out_cells)
{
    SK_REQUIRE_INIT();
    if (!g_last.valid) return sk_fail("sk_enum_device_rescore: no device run with scores to repeat");
    if (reps <= 0 || !out_ms) return sk_fail("sk_enum_device_rescore: bad argument");
    if (skrt::remote()) return sk_fail("sk_enum_device_rescore: a timing entry point (events); not carried by the broker -- unset STRELKA_AMD_BROKER");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    EnumBuffers& B = bufs();
    const FlatArgs& fa = g_last.fa;
    hipEvent_t e0, e1;
    SK_HIP(hipEventCreate(&e0));
    SK_HIP(hipEventCreate(&e1));
    SK_HIP(hipEventRecord(e0, st));
    if (g_last.fused && std::getenv("SK_F5_TIMING") && f5_timing_report(st)) return 1;
    for (int i = 0; i < reps; ++i) {
        if (g_last.fused) { // F5: the records -> the scores in one launch
            launch_flatten_score(g_last.n, st, g_last.fs);
            continue;
        }
        SK_HIP(skrt::memsetAsync(B.mask_arena.p, 0, g_last.mask_bytes, st));
        SK_HIP(skrt::memsetAsync(B.colmat.p, SK_SEL_NONE | (SK_SEL_NONE << 4), g_last.colmat_bytes, st));
        SK_LAUNCH(pool_fill_kernel, dim3(g_last.n), dim3(64), 0, st, fa);
        SK_LAUNCH(flatten_kernel, dim3((g_last.n_cals + 63) / 64), dim3(64), 0, st, fa);
        const bool f3_thread = (std::getenv("SK_F3_KERNEL") != nullptr && std::strcmp(std::getenv("SK_F3_KERNEL"), "thread") == 0);
        if (f3_thread) SK_LAUNCH(entries_kernel, dim3((g_last.n_cals + 63) / 64), dim3(64), 0, st, fa);
        else SK_LAUNCH(entries_wave_kernel, dim3(g_last.n), dim3(64), 0, st, fa);
        if (sk_score_alignments_launch_hostleg(&g_last.d, g_last.scores, st)) return 1;
    }
    SK_HIP(hipEventRecord(e1, st));
    SK_HIP(hipEventSynchronize(e1));
    SK_HIP(skrt::getLastError());
    SK_HIP(hipEventElapsedTime(out_ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (out_n_reads) *out_n_reads = g_last.n;
    if (out_n_cals) *out_n_cals = g_last.n_cals;
    if (out_cells) *out_cells = g_last.cells;
    return 0;
}
