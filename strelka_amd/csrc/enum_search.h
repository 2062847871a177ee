// enum_search.h -- a section of read_enumerate.hip: E1 (the search, level by level), E2 (each read's set of candidate alignments),
// the job's counter slots, the block scan, and the staging and scan kernels of a job run as one fixed sequence.
// Part of that one translation unit (its first section; the kernels live in its anonymous namespace), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "read_enumerate.h"

using namespace skcore;

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

} // namespace
