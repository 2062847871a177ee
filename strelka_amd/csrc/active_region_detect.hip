// active_region_detect.hip -- from the read intake's per-position arrays to the list of active regions: the reference's repeat finder
// (ReferenceRepeatFinder::updateRepeatSpan / initRepeatSpan, L/starling_common/ReferenceRepeatFinder.cpp:26-80, driven by
// ActiveRegionReadBuffer::setEndPos, ActiveRegionReadBuffer.cpp:173-189) and the detector's per-position walk
// (SampleActiveRegionDetector::updateEndPosition, L/starling_common/ActiveRegionDetector.cpp:336-409, createActiveRegion :314-328).
//
// The finder, with match_u(q) <=> base(q-u) != 'N' && base(q) == base(q-u) and span_u(q) = match_u(q) ? span_u(q-1) + 1 : u:
//   general rule   p is NOT an anchor <=> some u in 1..50 and q in [p, p+99] have span_u(q) >= 2u, span_u(q) >= 3 and either q == p or
//                  (span_u(q) == 2u || span_u(q) == 3) && q - span_u(q) < p.  span_u(m-1), m = max(init_pos - 99, ref_offset), is an
//                  INPUT: initRepeatSpan writes span_u(m) = u and updateRepeatSpan(m) overwrites it from the ring's stale slot.
//   tract form     100 and more past m: per u, a maximal run [a, b] of match_u of at least max(u, 3-u) makes [a-u, b] non-anchor.
//
//   AR1h ar_anchor_head_kernel  the first AR_HEAD positions from m, one wave: lane u-1 walks span_u from init_span as the reference does
//        (the back-unsets are idempotent stores of 0 into an LDS row, so the lanes need no order among them)
//   AR1  ar_anchor_tile_kernel  a tile of 1 024 positions per workgroup, tract form: the bases with their halo in LDS, one 64-bit match
//        mask per (u, word) by ballot, runs of at least max(u, 3-u) by shift-and-AND doubling, spread u + run - 1 to the left by
//        shift-and-OR doubling, OR-ed over u
//   AR1s ar_span_kernel         a wave per queried position, lane u-1 walking back to its run's start (or to m)
//   AR2  ar_walk_kernel         one workgroup: every wave turns 64 positions' flags into three mask words in LDS (16 384 positions a
//        turn), then one lane walks the words.  While no region is open (num_variants == 0 with an anchor after the last variant) a plain
//        anchor only moves the start and the previous anchor, so the lane jumps to the word's next candidate; otherwise it takes the
//        events (candidate or anchor) one by one through the reference's own statements.
#include "sk_common.h"

#include <climits>

namespace
{

typedef unsigned long long u64;

enum { AR_MAX_UNIT = SK_REPEAT_MAX_UNIT, AR_MIN_SPAN = 3, AR_AHEAD = 2 * AR_MAX_UNIT }; // ActiveRegionReadBuffer.hh:72-74
enum { AR_MAX_DIST = 13, AR_MIN_VARIANTS = 2 };                                         // ActiveRegionDetector.hh:141-144
enum {
    AR_THREADS = 256,
    AR_TILE_WORDS = 16,
    AR_TILE = 64 * AR_TILE_WORDS,
    AR_MWORDS = AR_TILE_WORDS + 3,                       // match words: one before the tile (a run may begin 49 back), two after
    AR_EWORDS = AR_TILE_WORDS + 2,                       // run-end words: two after the tile (the spread looks 99 ahead)
    AR_BASE_BEFORE = 64 + AR_MAX_UNIT,                   // bases before the tile: the word before it and its q - u
    AR_NBASES = AR_BASE_BEFORE + 64 * (AR_TILE_WORDS + 2)
};
enum { AR_HEAD = 210, AR_HEAD_Q = AR_HEAD + AR_AHEAD + 1 }; // positions the head kernel answers, positions its walk visits
enum { AR_WALK_THREADS = 1024, AR_WALK_WAVES = AR_WALK_THREADS / 64, AR_WALK_WORDS = 256, AR_WALK_CHUNK = 64 * AR_WALK_WORDS };

struct InitSpan
{
    uint32_t v[AR_MAX_UNIT];
};

// reference_contig_segment::get_base
__device__ __forceinline__ uint32_t ar_base(const char* ref, const int32_t ref_offset, const int32_t ref_len, const int64_t p)
{
    const int64_t k = p - ref_offset;
    return (k < 0 || k >= ref_len) ? uint32_t('N') : uint32_t(uint8_t(ref[k]));
}

// AR1h: is_anchor of [win_begin, head_end), head_end <= m + AR_HEAD, by the reference's own walk from m through head_end + 100
__global__ __launch_bounds__(64) void ar_anchor_head_kernel(const char* ref, const int32_t ref_offset, const int32_t ref_len, const int32_t m, const InitSpan init,
                                                            const int32_t win_begin, const int32_t head_end, uint8_t* is_anchor)
{
    __shared__ uint8_t bases[AR_MAX_UNIT + AR_HEAD_Q];
    __shared__ uint8_t anchor[AR_HEAD_Q];
    const int lane = threadIdx.x;
    const int n_q = (head_end - m) + AR_AHEAD + 1; // q = m .. head_end - 1 + 101
    for (int k = lane; k < AR_MAX_UNIT + n_q; k += 64) bases[k] = uint8_t(ar_base(ref, ref_offset, ref_len, int64_t(m) - AR_MAX_UNIT + k));
    for (int k = lane; k < n_q; k += 64) anchor[k] = 1; // (:32; in a row without the ring's wrap nothing unsets q before its own turn)
    __syncthreads();
    if (lane < AR_MAX_UNIT) {
        const uint32_t u = uint32_t(lane) + 1u;
        uint32_t span = init.v[lane]; // _repeatSpan[(m - 1) % 1000][u - 1] as updateRepeatSpan(m) finds it
        for (int qi = 0; qi < n_q; ++qi) {
            const uint32_t b = bases[AR_MAX_UNIT + qi], pb = bases[AR_MAX_UNIT + qi - int(u)];
            span = (pb != uint32_t('N') && b == pb) ? span + 1u : u; // :38-41
            if (span >= 2u * u && span >= uint32_t(AR_MIN_SPAN)) {   // :43
                if (span == 2u * u || span == uint32_t(AR_MIN_SPAN)) { // :46-53
                    int lo = qi - int(span) + 1;
                    if (lo < 0) lo = 0; // (positions before m are not answered)
                    for (int k = qi - 1; k >= lo; --k) anchor[k] = 0;
                }
                anchor[qi] = 0; // :55
            }
        }
    }
    __syncthreads();
    const int first = win_begin - m;
    for (int i = lane; i < head_end - win_begin; i += 64) is_anchor[i] = anchor[first + i];
}

// AR1: is_anchor of [begin, end) in tiles, begin >= m + 100
__global__ __launch_bounds__(AR_THREADS) void ar_anchor_tile_kernel(const char* ref, const int32_t ref_offset, const int32_t ref_len, const int32_t begin, const int32_t end,
                                                                   const int32_t win_begin, uint8_t* is_anchor)
{
    __shared__ uint8_t bases[AR_NBASES];        // positions t0 - AR_BASE_BEFORE ..
    __shared__ u64 mword[AR_MAX_UNIT][AR_MWORDS]; // match_u of positions t0 + 64 (k - 1) ..
    __shared__ u64 eword[AR_MAX_UNIT][AR_EWORDS]; // "a run of the wanted length ends here" of positions t0 + 64 j ..
    __shared__ u64 non_anchor[AR_TILE_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = int64_t(begin) + int64_t(blockIdx.x) * AR_TILE;
    for (int k = tid; k < AR_NBASES; k += AR_THREADS) bases[k] = uint8_t(ar_base(ref, ref_offset, ref_len, t0 - AR_BASE_BEFORE + k));
    if (tid < AR_TILE_WORDS) non_anchor[tid] = 0;
    __syncthreads();
    for (int item = wave; item < AR_MAX_UNIT * AR_MWORDS; item += AR_THREADS / 64) {
        const int u = item / AR_MWORDS + 1, k = item % AR_MWORDS;
        const int at = AR_MAX_UNIT + 64 * k + lane;
        const uint32_t b = bases[at], pb = bases[at - u];
        const u64 w = __ballot(pb != uint32_t('N') && b == pb);
        if (lane == 0) mword[u - 1][k] = w;
    }
    __syncthreads();
    for (int item = tid; item < AR_MAX_UNIT * AR_EWORDS; item += AR_THREADS) {
        const int u = item / AR_EWORDS + 1, j = item % AR_EWORDS;
        const int run = u == 1 ? 2 : u; // max(u, 3 - u)
        u64 lo = mword[u - 1][j], hi = mword[u - 1][j + 1];
        for (int have = 1; have < run;) { // after the step: bit q <=> match_u on [q - have + 1, q]
            const int s = min(have, run - have);
            const u64 shi = (hi << s) | (lo >> (64 - s)), slo = lo << s;
            hi &= shi;
            lo &= slo;
            have += s;
        }
        eword[u - 1][j] = hi;
    }
    __syncthreads();
    for (int item = tid; item < AR_MAX_UNIT * AR_TILE_WORDS; item += AR_THREADS) {
        const int u = item / AR_TILE_WORDS + 1, j = item % AR_TILE_WORDS;
        const int need = (u == 1 ? 2 : u) + u; // p is covered by a run end at q in [p, p + run - 1 + u]
        u64 a0 = eword[u - 1][j], a1 = eword[u - 1][j + 1], a2 = eword[u - 1][j + 2];
        if ((a0 | a1 | a2) == 0) continue;
        for (int have = 1; have < need;) { // after the step: bit p <=> a run end in [p, p + have - 1]
            const int s = min(have, need - have);
            const u64 b0 = (a0 >> s) | (a1 << (64 - s)), b1 = (a1 >> s) | (a2 << (64 - s)), b2 = a2 >> s;
            a0 |= b0;
            a1 |= b1;
            a2 |= b2;
            have += s;
        }
        if (a0) atomicOr(&non_anchor[j], a0);
    }
    __syncthreads();
    for (int i = tid; i < AR_TILE; i += AR_THREADS) {
        const int64_t p = t0 + i;
        if (p < end) is_anchor[p - win_begin] = ((non_anchor[i >> 6] >> (i & 63)) & 1ull) ? 0 : 1;
    }
}

// AR1s: the _repeatSpan row of position span_pos[block] (:38-42 unrolled back to the run's start)
__global__ __launch_bounds__(64) void ar_span_kernel(const char* ref, const int32_t ref_offset, const int32_t ref_len, const int32_t m, const InitSpan init,
                                                     const int32_t* span_pos, uint32_t* span_out, unsigned* err)
{
    const int lane = threadIdx.x;
    if (lane >= AR_MAX_UNIT) return;
    const int32_t s = span_pos[blockIdx.x];
    uint32_t* row = span_out + size_t(blockIdx.x) * AR_MAX_UNIT;
    if (s < m) { // the host entry refuses this
        if (lane == 0) atomicOr(err, unsigned(SK_DEVERR_ACTIVE_REGION));
        row[lane] = 0;
        return;
    }
    const uint32_t u = uint32_t(lane) + 1u;
    uint32_t count = 0;
    int64_t q = s;
    while (q >= m) {
        const uint32_t b = ar_base(ref, ref_offset, ref_len, q), pb = ar_base(ref, ref_offset, ref_len, q - int64_t(u));
        if (!(pb != uint32_t('N') && b == pb)) break;
        ++count;
        --q;
    }
    row[lane] = (q < m ? init.v[lane] : u) + count;
}

// SampleActiveRegionDetector::updateEndPosition(x + 1) from :353 on; false where createActiveRegion's assertion (:318) fails
__device__ __forceinline__ bool ar_step(sk_ar_state& s, const int32_t x, bool cand, const bool depth_zero, const bool ring_anchor, bool& made, sk_active_region& region)
{
    if (depth_zero && s.num_variants == 0u) cand = false; // :357-360
    const bool anchor = ring_anchor && !cand;             // :362
    if (!cand && !anchor) return true;
    const uint32_t distance = uint32_t(x) - uint32_t(s.prev_variant_pos); // :368
    if (distance > uint32_t(AR_MAX_DIST) && s.anchor_pos_following_prev_variant >= 0) {
        if (s.num_variants >= uint32_t(AR_MIN_VARIANTS)) {
            if (!(s.active_region_start_pos < s.anchor_pos_following_prev_variant)) return false;
            region.begin = s.active_region_start_pos;
            region.end = s.anchor_pos_following_prev_variant + 1; // :327
            region.made_at = x + 1;
            made = true;
            s.active_region_start_pos = 0; // :325
        }
        s.num_variants = 0;
    }
    if (anchor) {
        if (s.num_variants == 0u) s.active_region_start_pos = x;
        if (s.anchor_pos_following_prev_variant < 0) s.anchor_pos_following_prev_variant = x;
        s.prev_anchor_pos = x;
    }
    if (cand) {
        if (!s.active_region_start_pos) s.active_region_start_pos = s.prev_anchor_pos; // :400: start position 0 reads as unset
        ++s.num_variants;
        s.prev_variant_pos = x;
        s.anchor_pos_following_prev_variant = -1;
    }
    return true;
}

// AR2
__global__ __launch_bounds__(AR_WALK_THREADS) void ar_walk_kernel(const int32_t win_begin, const int32_t n_pos, const sk_intake_site* sites, const uint8_t* is_candidate,
                                                                 const uint8_t* is_anchor, const sk_ar_state* state_in, sk_ar_state* state_out,
                                                                 sk_active_region* regions, const int64_t region_cap, int32_t* n_regions, unsigned* err)
{
    __shared__ u64 cand_w[AR_WALK_WORDS], zero_w[AR_WALK_WORDS], anchor_w[AR_WALK_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    sk_ar_state s = {}, s_in = {};
    int64_t n_out = 0;
    bool bad = false;
    if (tid == 0) {
        s_in = *state_in;
        s = s_in;
        if (n_pos > 0 && s.is_beginning) { // :341-347, at the first call, pos = win_begin + 1
            s.active_region_start_pos = s.anchor_pos_following_prev_variant = s.prev_anchor_pos = win_begin + 1;
            s.is_beginning = 0;
        }
    }
    for (int64_t c0 = 0; c0 < n_pos; c0 += AR_WALK_CHUNK) {
        const int n_here = int(min(int64_t(AR_WALK_CHUNK), int64_t(n_pos) - c0));
        const int words = (n_here + 63) / 64;
#pragma unroll 4
        for (int k = 0; k < AR_WALK_WORDS / AR_WALK_WAVES; ++k) { // (w < words is the same for a whole wave)
            const int w = wave + AR_WALK_WAVES * k;
            if (w >= words) continue;
            const int64_t i = c0 + 64 * int64_t(w) + lane;
            bool c = false, z = false, a = false;
            if (i < n_pos) {
                c = is_candidate[i] != 0;
                z = sites[i].depth == 0u;
                a = is_anchor[i] != 0;
            }
            const u64 cw = __ballot(c), zw = __ballot(z), aw = __ballot(a);
            if (lane == 0) {
                cand_w[w] = cw;
                zero_w[w] = zw;
                anchor_w[w] = aw;
            }
        }
        __syncthreads();
        if (tid == 0 && !bad) {
            for (int w = 0; w < words && !bad; ++w) {
                const u64 C = cand_w[w], Z = zero_w[w], A = anchor_w[w];
                const int32_t base = int32_t(int64_t(win_begin) + c0 + 64 * int64_t(w));
                u64 pending = ~0ull;
                while (pending) {
                    int bit;
                    if (s.num_variants == 0u && s.anchor_pos_following_prev_variant >= 0) {
                        // no region open: a depth-zero candidate is none (:357-360), and a plain anchor only moves the start and the
                        // previous anchor (:385-395; :370-381 changes nothing at num_variants == 0) -- the last one before the next candidate counts
                        const u64 real = C & ~Z;
                        const u64 next = real & pending;
                        const u64 before = next ? ((next & (~next + 1ull)) - 1ull) : ~0ull;
                        const u64 plain = A & ~real & pending & before;
                        if (plain) s.active_region_start_pos = s.prev_anchor_pos = base + (63 - __clzll(plain));
                        if (!next) break;
                        bit = __ffsll(next) - 1;
                    } else {
                        const u64 events = (C | A) & pending;
                        if (!events) break;
                        bit = __ffsll(events) - 1;
                    }
                    bool made = false;
                    sk_active_region region = {};
                    if (!ar_step(s, base + bit, (C >> bit) & 1ull, (Z >> bit) & 1ull, (A >> bit) & 1ull, made, region)) {
                        bad = true;
                        break;
                    }
                    if (made) {
                        if (n_out < region_cap) regions[n_out] = region;
                        else bad = true; // (the host entry refuses a cap below the bound)
                        ++n_out;
                    }
                    pending = bit == 63 ? 0ull : (~0ull << (bit + 1));
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (bad) {
            atomicOr(err, unsigned(SK_DEVERR_ACTIVE_REGION));
            *n_regions = 0;
            *state_out = s_in;
        } else {
            *n_regions = int32_t(n_out);
            *state_out = s;
        }
    }
}

// ---- the multi-sample synchroniser (ActiveRegionDetector, .cpp:77-154, :203-293) -----------------------------------------------------------------

enum { AR_SYNC_WORDS = 64, AR_SYNC_CHUNK = 64 * AR_SYNC_WORDS }; // (2 * SK_MAX_SAMPLES + 1) * 64 words: 8 704 bytes of LDS beside AR2's 6 144
enum { AR_SYNC_PADDING = 9 };                                    // ActiveRegionReadBuffer::MaxAssemblyPadding
enum { AR_SYNC_ID_THREADS = 256 };

struct SyncArgs
{
    int32_t n_samples, win_begin, n_pos;
    const sk_intake_site* sites; // [n_samples][n_pos]
    const uint8_t* is_candidate; // [n_samples][n_pos]
    const uint8_t* is_anchor;    // [n_pos]
    const int32_t* mark_off;     // [n_samples + 1]
    const sk_ploidy_mark* marks;
    int32_t default_ploidy;
    const sk_sync_state* state_in;
    sk_sync_state* state_out;
    int32_t do_clear;
    int32_t buf_begin[SK_MAX_SAMPLES], buf_end[SK_MAX_SAMPLES];
    sk_sync_region* regions;
    int64_t region_cap;
    int32_t* n_regions;
    unsigned* err;
};

// SampleActiveRegionDetector::getPloidy(pos) (:280-284) over the sorted marks of one sample
__device__ __forceinline__ int32_t ar_ploidy_at(const sk_ploidy_mark* marks, int32_t lo, int32_t hi, const int32_t default_ploidy, const int32_t pos)
{
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const int32_t p = marks[mid].pos;
        if (p == pos) return marks[mid].ploidy;
        if (p < pos) lo = mid + 1;
        else hi = mid;
    }
    return default_ploidy;
}

// AR3: one workgroup, AR2's shape.  Every wave turns 64 positions' flags into mask words in LDS -- a candidate word and a depth-zero word per
// sample and one anchor word, the samples' finders being one -- 4 096 positions a turn; then one lane walks the words for all samples at once.
// A sample's detector reads nothing of the others, and the synchroniser only reads the samples' start positions, so between two positions at
// which some sample's coordinates change the close test (:137-153) gives one answer: the lane visits those positions only and closes the region
// at the first call >= end + 9 since the last visit whose test passes.  While no synchronised region is open nobody reads the start positions
// and AR2's shortcut holds per sample (a plain anchor only moves the start and the previous anchor); while one is open every anchor is visited.
__global__ __launch_bounds__(AR_WALK_THREADS) void ar_sync_walk_kernel(const SyncArgs a)
{
    __shared__ u64 cand_w[SK_MAX_SAMPLES][AR_SYNC_WORDS], zero_w[SK_MAX_SAMPLES][AR_SYNC_WORDS], anchor_w[AR_SYNC_WORDS];
    __shared__ sk_sync_state s_in, s;
    __shared__ int bad_marks, failed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.n_samples;
    if (tid == 0) bad_marks = 0;
    for (int k = tid; k < int(sizeof(sk_sync_state) / 4); k += AR_WALK_THREADS) { // (state_out may be state_in: read whole before anything is written)
        const int32_t v = reinterpret_cast<const int32_t*>(a.state_in)[k];
        reinterpret_cast<int32_t*>(&s_in)[k] = v;
        reinterpret_cast<int32_t*>(&s)[k] = v;
    }
    __syncthreads();
    // the marks: ascending positions per sample, ploidy 1 or 2 (the host entry refuses others with a message)
    for (int smp = 0; smp < S; ++smp) {
        const int32_t lo = a.mark_off[smp], hi = a.mark_off[smp + 1];
        if (tid == 0 && (lo < 0 || hi < lo)) bad_marks = 1;
        for (int64_t k = int64_t(lo) + tid; k < hi; k += AR_WALK_THREADS) {
            const sk_ploidy_mark m = a.marks[k];
            if ((m.ploidy != 1 && m.ploidy != 2) || (k + 1 < hi && !(m.pos < a.marks[k + 1].pos))) bad_marks = 1;
        }
    }
    if (tid == 0 && a.default_ploidy != 1 && a.default_ploidy != 2) bad_marks = 1;
    __syncthreads();

    // the walking lane's own: the synchronised region, the first call whose close test has not been answered yet
    int64_t n_out = 0, t_from = int64_t(a.win_begin) + 1;
    bool bad = bad_marks != 0;

    // no sample's unclosed start lies inside the region (:141-149)
    const auto can_close = [&]() {
        for (int smp = 0; smp < S; ++smp) {
            const int32_t start = s.sample[smp].active_region_start_pos;
            if (start >= 0 && start < s.sync_end - 1) return false;
        }
        return true;
    };
    // closeActiveRegion (:203-250) for the call closed_at
    const auto close_region = [&](const int32_t closed_at) {
        if (!(int64_t(s.sync_end) - s.sync_begin > 0)) { // :206
            bad = true;
            return;
        }
        if (n_out < a.region_cap) {
            sk_sync_region* r = a.regions + n_out;
            const int32_t begin = s.sync_begin, end = s.sync_end;
            r->begin = begin;
            r->end = end;
            r->closed_at = closed_at;
            r->prev_end = s.prev_end;
            for (int smp = 0; smp < SK_MAX_SAMPLES; ++smp) r->ploidy[smp] = 0;
            for (int smp = 0; smp < S; ++smp) {
                const int32_t lo = a.mark_off[smp], hi = a.mark_off[smp + 1];
                const int32_t left = ar_ploidy_at(a.marks, lo, hi, a.default_ploidy, begin), right = ar_ploidy_at(a.marks, lo, hi, a.default_ploidy, end - 1);
                r->ploidy[smp] = uint8_t(left > right ? left : right); // :286-293
            }
            r->sample_mask = s.sample_mask;
            r->pad = 0;
        } else {
            bad = true; // (the host entry refuses a cap below the bound)
        }
        ++n_out;
        s.prev_end = s.sync_end;         // :248
        s.sync_begin = s.sync_end = 0;   // :249
        s.sample_mask = 0;
    };
    // processExistingActiveRegion (:133-154) for every call from t_from through upto, between which no sample's coordinates change
    const auto close_through = [&](const int64_t upto) {
        if (s.sync_end == 0 || !can_close()) return;
        const int64_t first = int64_t(s.sync_end) + AR_SYNC_PADDING;
        const int64_t at = first > t_from ? first : t_from;
        if (at <= upto) close_region(int32_t(at));
    };
    // updateActiveRegionRange (:119-131)
    const auto merge = [&](const int32_t begin, const int32_t end, const int smp) {
        if (s.sync_end) {
            if (begin < s.sync_begin) s.sync_begin = begin;
            if (end > s.sync_end) s.sync_end = end;
        } else {
            s.sync_begin = begin;
            s.sync_end = end;
        }
        s.sample_mask |= 1u << smp;
    };

    if (tid == 0 && !bad && a.n_pos > 0) {
        close_through(t_from); // the first call's test reads the starts as they came in, before :341-347
        t_from += 1;
        for (int smp = 0; smp < S; ++smp) {
            sk_ar_state& d = s.sample[smp];
            if (d.is_beginning) { // :341-347, at the first call, pos = win_begin + 1
                d.active_region_start_pos = d.anchor_pos_following_prev_variant = d.prev_anchor_pos = a.win_begin + 1;
                d.is_beginning = 0;
            }
        }
    }
    for (int64_t c0 = 0; c0 < a.n_pos; c0 += AR_SYNC_CHUNK) {
        const int n_here = int(min(int64_t(AR_SYNC_CHUNK), int64_t(a.n_pos) - c0));
        const int words = (n_here + 63) / 64;
        for (int item = wave; item < (S + 1) * words; item += AR_WALK_WAVES) { // (the same for a whole wave)
            const int smp = item / words, w = item - smp * words;
            const int64_t i = c0 + 64 * int64_t(w) + lane;
            if (smp < S) {
                bool c = false, z = false;
                if (i < a.n_pos) {
                    const int64_t at = int64_t(smp) * a.n_pos + i;
                    c = a.is_candidate[at] != 0;
                    z = a.sites[at].depth == 0u;
                }
                const u64 cw = __ballot(c), zw = __ballot(z);
                if (lane == 0) {
                    cand_w[smp][w] = cw;
                    zero_w[smp][w] = zw;
                }
            } else {
                const u64 aw = __ballot(i < a.n_pos && a.is_anchor[i] != 0);
                if (lane == 0) anchor_w[w] = aw;
            }
        }
        __syncthreads();
        if (tid == 0 && !bad) {
            for (int w = 0; w < words && !bad; ++w) {
                const u64 A = anchor_w[w];
                u64 any_c = 0;
                for (int smp = 0; smp < S; ++smp) any_c |= cand_w[smp][w];
                const int32_t base = int32_t(int64_t(a.win_begin) + c0 + 64 * int64_t(w));
                u64 pending = ~0ull;
                while (pending && !bad) {
                    // the positions to visit: with a region open every event of any sample; otherwise per sample what AR2 visits
                    u64 visit = 0, jumping = 0;
                    if (s.sync_end != 0) {
                        visit = any_c | A;
                    } else {
                        for (int smp = 0; smp < S; ++smp) {
                            const sk_ar_state& d = s.sample[smp];
                            const u64 C = cand_w[smp][w];
                            if (d.num_variants == 0u && d.anchor_pos_following_prev_variant >= 0) {
                                visit |= C & ~zero_w[smp][w];
                                jumping |= 1ull << smp;
                            } else {
                                visit |= C | A;
                            }
                        }
                    }
                    visit &= pending;
                    // the plain anchors before it: the last one counts (:385-395), for the samples that skip them
                    const u64 before = visit ? ((visit & (~visit + 1ull)) - 1ull) : ~0ull;
                    const u64 plain = A & pending & before;
                    if (plain && jumping) {
                        const int32_t at = base + (63 - __clzll(plain));
                        for (int smp = 0; smp < S; ++smp)
                            if ((jumping >> smp) & 1ull) s.sample[smp].active_region_start_pos = s.sample[smp].prev_anchor_pos = at;
                    }
                    if (!visit) break;
                    const int bit = __ffsll(visit) - 1;
                    const int32_t x = base + bit;
                    close_through(int64_t(x) + 1); // the calls up to this one: the test comes before the samples' steps (:80)
                    const bool ring = (A >> bit) & 1ull;
                    for (int smp = 0; smp < S && !bad; ++smp) {
                        const bool c = (cand_w[smp][w] >> bit) & 1ull;
                        if (!c && !ring) continue; // (no event for this sample, :364)
                        sk_ar_state d = s.sample[smp];
                        bool made = false;
                        sk_active_region region = {};
                        if (!ar_step(d, x, c, (zero_w[smp][w] >> bit) & 1ull, ring, made, region)) {
                            bad = true;
                            break;
                        }
                        s.sample[smp] = d;
                        if (made) merge(region.begin, region.end, smp);
                    }
                    t_from = int64_t(x) + 2;
                    pending = bit == 63 ? 0ull : (~0ull << (bit + 1));
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (!bad) close_through(int64_t(a.win_begin) + a.n_pos);
        if (!bad && a.do_clear) { // clear() (:98-111) over closeActiveRegionDetector (:413-440)
            for (int smp = 0; smp < S && !bad; ++smp) {
                sk_ar_state& d = s.sample[smp];
                if (d.is_beginning) continue;
                if (d.num_variants >= uint32_t(AR_MIN_VARIANTS)) {
                    const bool no_start = d.active_region_start_pos < 0, no_end = d.anchor_pos_following_prev_variant < 0;
                    if (!no_start || !no_end || a.buf_begin[smp] < a.buf_end[smp]) {
                        if (no_start) d.active_region_start_pos = a.buf_begin[smp];
                        if (no_end) d.anchor_pos_following_prev_variant = a.buf_end[smp] - 1;
                        if (!(d.active_region_start_pos < d.anchor_pos_following_prev_variant)) { // :318
                            bad = true;
                            break;
                        }
                        merge(d.active_region_start_pos, d.anchor_pos_following_prev_variant + 1, smp);
                    }
                }
                d.prev_anchor_pos = d.active_region_start_pos = d.anchor_pos_following_prev_variant = d.prev_variant_pos = -1; // clearCoordinates, is_beginning as it was
                d.num_variants = 0;
            }
            if (!bad && s.sync_end) close_region(SK_SYNC_CLOSED_AT_CLEAR);
        }
        if (bad) atomicOr(a.err, unsigned(SK_DEVERR_SYNC_REGIONS));
        *a.n_regions = bad ? 0 : int32_t(n_out);
        failed = bad ? 1 : 0;
    }
    __syncthreads();
    const sk_sync_state& out = failed ? s_in : s;
    for (int k = tid; k < int(sizeof(sk_sync_state) / 4); k += AR_WALK_THREADS) reinterpret_cast<int32_t*>(a.state_out)[k] = reinterpret_cast<const int32_t*>(&out)[k];
}

// AR3i: region_id of the window's positions from the closed regions (setPosToActiveRegionIdMap, :267-278): the last region of at most 250
// positions that covers the position
__global__ __launch_bounds__(AR_SYNC_ID_THREADS) void ar_sync_region_id_kernel(const int32_t win_begin, const int32_t n_pos, const sk_sync_region* regions, const int32_t* n_regions,
                                                                               const int64_t region_cap, int32_t* region_id)
{
    const int64_t i = int64_t(blockIdx.x) * AR_SYNC_ID_THREADS + threadIdx.x;
    if (i >= n_pos) return;
    int64_t n = *n_regions;
    if (n > region_cap) n = region_cap;
    const int64_t p = int64_t(win_begin) + i;
    int32_t id = -1;
    for (int64_t r = n - 1; r >= 0; --r) {
        const int32_t begin = regions[r].begin, end = regions[r].end;
        if (p >= begin && p < end && int64_t(end) - begin <= SK_HAP_MAX_REF_SPAN) {
            id = begin;
            break;
        }
    }
    region_id[i] = id;
}

// AR3p: one sample's sk_region_params and sk_active_region records from the synchronised list
__global__ __launch_bounds__(256) void ar_sync_params_kernel(const sk_sync_region* sync, const int32_t* n_regions, const int64_t region_cap, const int32_t sample,
                                                             const int32_t buf_begin, const int32_t buf_end_at_clear, sk_active_region* regions, sk_region_params* params)
{
    const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
    int64_t n = *n_regions;
    if (n > region_cap) n = region_cap;
    if (r >= n) return;
    const int32_t closed_at = sync[r].closed_at;
    if (regions) {
        sk_active_region out;
        out.begin = sync[r].begin;
        out.end = sync[r].end;
        out.made_at = closed_at;
        regions[r] = out;
    }
    sk_region_params p;
    p.buf_begin = buf_begin;
    p.buf_end = closed_at == SK_SYNC_CLOSED_AT_CLEAR ? buf_end_at_clear : closed_at;
    p.ploidy = sync[r].ploidy[sample];
    p.pad = 0;
    params[r] = p;
}

const char* ar_sync_issue(const int32_t n_samples, const int32_t win_begin, const int32_t n_pos, const int32_t default_ploidy, const int64_t region_cap)
{
    if (n_samples < 1 || n_samples > SK_MAX_SAMPLES) return "n_samples outside 1..SK_MAX_SAMPLES";
    if (n_pos < 0 || region_cap < 0) return "negative size";
    if (win_begin < 0) return "win_begin below zero";
    if (int64_t(win_begin) + n_pos + 1 > INT32_MAX) return "the window ends beyond int32";
    if (default_ploidy != 1 && default_ploidy != 2) return "default_ploidy must be 1 or 2";
    if (region_cap < int64_t(n_pos) + 1) return "region_cap is below sk_sync_regions_bound";
    return nullptr;
}

// m of initRepeatSpan(init_pos) (:62-64)
int32_t ar_min_pos(const int32_t init_pos, const int32_t ref_offset)
{
    const int64_t m = int64_t(init_pos) - AR_AHEAD + 1;
    return m < ref_offset ? ref_offset : int32_t(m);
}

const char* ar_anchor_issue(const int32_t ref_offset, const int32_t ref_len, const int32_t init_pos, const int32_t win_begin, const int32_t n_pos, const int32_t n_span_pos)
{
    if (ref_len < 0 || n_pos < 0 || n_span_pos < 0) return "negative size";
    if (ref_offset < 0) return "negative ref_offset";
    if (int64_t(ref_offset) + ref_len > INT32_MAX) return "the reference segment ends beyond int32";
    if (int64_t(init_pos) - AR_AHEAD + 1 < INT32_MIN || int64_t(init_pos) + AR_AHEAD > INT32_MAX) return "init_pos beyond int32's reach of the finder's arithmetic";
    if (int64_t(win_begin) + n_pos + AR_AHEAD + 1 > INT32_MAX) return "the window ends beyond int32's reach of the finder's arithmetic";
    if (win_begin < ar_min_pos(init_pos, ref_offset)) return "win_begin is before the first position initRepeatSpan(init_pos) updates";
    return nullptr;
}

} // namespace

extern "C" {

void sk_ar_state_initial(sk_ar_state* s)
{
    s->is_beginning = 1; // ActiveRegionDetector.hh:157
    s->active_region_start_pos = s->anchor_pos_following_prev_variant = s->prev_anchor_pos = s->prev_variant_pos = -1; // clearCoordinates, .cpp:296-303
    s->num_variants = 0;
}

int64_t sk_active_regions_bound(int32_t n_pos)
{
    if (n_pos < 0) return -1;
    return int64_t(n_pos) / 2 + 1; // a region takes two variants; one more may be carried in by state_in
}

int sk_ref_anchors_dev(const char* dev_ref_seq, int32_t ref_offset, int32_t ref_len, int32_t init_pos, const uint32_t* init_span, int32_t win_begin, int32_t n_pos,
                       uint8_t* dev_is_anchor, int32_t n_span_pos, const int32_t* dev_span_pos, uint32_t* dev_span_out, void* hip_stream)
{
    if (const char* why = ar_anchor_issue(ref_offset, ref_len, init_pos, win_begin, n_pos, n_span_pos)) return sk_fail(std::string("sk_ref_anchors_dev: ") + why);
    if ((ref_len > 0 && !dev_ref_seq) || (n_pos > 0 && !dev_is_anchor) || (n_span_pos > 0 && (!dev_span_pos || !dev_span_out)))
        return sk_fail("sk_ref_anchors_dev: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    InitSpan init;
    for (int u = 0; u < AR_MAX_UNIT; ++u) init.v[u] = init_span ? init_span[u] : 0u;
    const int32_t m = ar_min_pos(init_pos, ref_offset);
    const int64_t win_end = int64_t(win_begin) + n_pos;
    const int64_t head_end = win_end < int64_t(m) + AR_HEAD ? win_end : int64_t(m) + AR_HEAD;
    if (head_end > win_begin) SK_LAUNCH(ar_anchor_head_kernel, dim3(1), dim3(64), 0, st, dev_ref_seq, ref_offset, ref_len, m, init, win_begin, int32_t(head_end), dev_is_anchor);
    const int64_t tile_begin = head_end > win_begin ? head_end : int64_t(win_begin);
    if (win_end > tile_begin) {
        const int64_t tiles = (win_end - tile_begin + AR_TILE - 1) / AR_TILE;
        SK_LAUNCH(ar_anchor_tile_kernel, dim3(unsigned(tiles)), dim3(AR_THREADS), 0, st, dev_ref_seq, ref_offset, ref_len, int32_t(tile_begin), int32_t(win_end), win_begin,
                  dev_is_anchor);
    }
    if (n_span_pos > 0)
        SK_LAUNCH(ar_span_kernel, dim3(unsigned(n_span_pos)), dim3(64), 0, st, dev_ref_seq, ref_offset, ref_len, m, init, dev_span_pos, dev_span_out, sk_ctx().dev_error_flags);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_ref_anchors(const char* ref_seq, int32_t ref_offset, int32_t ref_len, int32_t init_pos, const uint32_t* init_span, int32_t win_begin, int32_t n_pos,
                   uint8_t* is_anchor, int32_t n_span_pos, const int32_t* span_pos, uint32_t* span_out)
{
    if (const char* why = ar_anchor_issue(ref_offset, ref_len, init_pos, win_begin, n_pos, n_span_pos)) return sk_fail(std::string("sk_ref_anchors: ") + why);
    if ((ref_len > 0 && !ref_seq) || (n_pos > 0 && !is_anchor) || (n_span_pos > 0 && (!span_pos || !span_out))) return sk_fail("sk_ref_anchors: null argument");
    const int32_t m = ar_min_pos(init_pos, ref_offset);
    for (int32_t i = 0; i < n_span_pos; ++i)
        if (span_pos[i] < m) return sk_fail("sk_ref_anchors: span_pos[" + std::to_string(i) + "] is before the first position initRepeatSpan(init_pos) updates");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t n_span = size_t(AR_MAX_UNIT) * size_t(n_span_pos);
    struct { char* ref; uint8_t* anchor; int32_t* span_pos; uint32_t* span_out; } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(ref_seq, size_t(ref_len), 16, st, rc), ar.take<uint8_t>(size_t(n_pos) + 16), ar.up(span_pos, size_t(n_span_pos), 4, st, rc),
                                ar.take<uint32_t>(n_span + 4) };
        }) || rc)
        return 1;
    if (sk_ref_anchors_dev(d.ref, ref_offset, ref_len, init_pos, init_span, win_begin, n_pos, d.anchor, n_span_pos, d.span_pos, d.span_out, st)) return 1;
    if (n_pos > 0) SK_HIP(skrt::memcpyAsync(is_anchor, d.anchor, size_t(n_pos), hipMemcpyDeviceToHost, st));
    if (n_span_pos > 0) SK_HIP(skrt::memcpyAsync(span_out, d.span_out, sizeof(uint32_t) * n_span, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    return 0;
}

int sk_active_regions_dev(int32_t win_begin, int32_t n_pos, const sk_intake_site* dev_sites, const uint8_t* dev_is_candidate, const uint8_t* dev_is_anchor,
                          const sk_ar_state* dev_state_in, sk_ar_state* dev_state_out, sk_active_region* dev_regions, int64_t region_cap, int32_t* dev_n_regions,
                          void* hip_stream)
{
    if (n_pos < 0 || region_cap < 0) return sk_fail("sk_active_regions_dev: negative size");
    if (win_begin < 0) return sk_fail("sk_active_regions_dev: win_begin below zero");
    if (int64_t(win_begin) + n_pos + 1 > INT32_MAX) return sk_fail("sk_active_regions_dev: the window ends beyond int32");
    if (region_cap < sk_active_regions_bound(n_pos)) return sk_fail("sk_active_regions_dev: region_cap is below sk_active_regions_bound");
    if (!dev_state_in || !dev_state_out || !dev_regions || !dev_n_regions || (n_pos > 0 && (!dev_sites || !dev_is_candidate || !dev_is_anchor)))
        return sk_fail("sk_active_regions_dev: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    SK_LAUNCH(ar_walk_kernel, dim3(1), dim3(AR_WALK_THREADS), 0, st, win_begin, n_pos, dev_sites, dev_is_candidate, dev_is_anchor, dev_state_in, dev_state_out, dev_regions,
              region_cap, dev_n_regions, sk_ctx().dev_error_flags);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_active_regions(int32_t win_begin, int32_t n_pos, const sk_intake_site* sites, const uint8_t* is_candidate, const uint8_t* is_anchor, const sk_ar_state* state_in,
                      sk_ar_state* state_out, sk_active_region* regions, int64_t region_cap, int32_t* n_regions)
{
    if (n_pos < 0 || region_cap < 0) return sk_fail("sk_active_regions: negative size");
    if (win_begin < 0) return sk_fail("sk_active_regions: win_begin below zero");
    if (int64_t(win_begin) + n_pos + 1 > INT32_MAX) return sk_fail("sk_active_regions: the window ends beyond int32");
    const int64_t bound = sk_active_regions_bound(n_pos);
    if (region_cap < bound) return sk_fail("sk_active_regions: region_cap is below sk_active_regions_bound");
    if (!state_in || !state_out || !regions || !n_regions || (n_pos > 0 && (!sites || !is_candidate || !is_anchor))) return sk_fail("sk_active_regions: null argument");
    if (state_in->num_variants >= uint32_t(AR_MIN_VARIANTS) && state_in->anchor_pos_following_prev_variant >= 0 &&
        !(state_in->active_region_start_pos < state_in->anchor_pos_following_prev_variant))
        return sk_fail("sk_active_regions: state_in holds a region whose start is not before its end anchor (createActiveRegion's assertion)");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t np = size_t(n_pos);
    // (state_in, state_out and n_regions each in a 256-byte piece of their own; the sticky error flag is the _dev entry's)
    struct { sk_intake_site* sites; uint8_t* cand; uint8_t* anchor; sk_active_region* regions; sk_ar_state* state_in; sk_ar_state* state_out; int32_t* n; } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(sites, np, 2, st, rc), ar.up(is_candidate, np, 16, st, rc), ar.up(is_anchor, np, 16, st, rc),
                                ar.take<sk_active_region>(size_t(bound) + 2), ar.up(state_in, 1, 0, st, rc), ar.take<sk_ar_state>(1), ar.take<int32_t>(1) };
        }) || rc)
        return 1;
    if (sk_active_regions_dev(win_begin, n_pos, d.sites, d.cand, d.anchor, d.state_in, d.state_out, d.regions, bound, d.n, st)) return 1;
    sk_ar_state out;
    int32_t n = 0;
    SK_HIP(skrt::memcpyAsync(&out, d.state_out, sizeof(sk_ar_state), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::memcpyAsync(&n, d.n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1; // the assertion failed mid-window: nothing is emitted
    if (n < 0 || n > bound) return sk_fail("sk_active_regions: region count out of range");
    if (n > 0) {
        SK_HIP(skrt::memcpyAsync(regions, d.regions, sizeof(sk_active_region) * size_t(n), hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::streamSynchronize(st));
    }
    *state_out = out;
    *n_regions = n;
    return 0;
}

void sk_sync_state_initial(sk_sync_state* s)
{
    for (int k = 0; k < SK_MAX_SAMPLES; ++k) sk_ar_state_initial(&s->sample[k]);
    s->sync_begin = s->sync_end = 0; // known_pos_range2::clear
    s->prev_end = -1;                // ActiveRegionDetector.hh:117
    s->sample_mask = 0;
}

int64_t sk_sync_regions_bound(int32_t n_pos)
{
    if (n_pos < 0) return -1;
    return int64_t(n_pos) + 1; // one close per call at most (processExistingActiveRegion runs once in it), and one in clear()
}

int sk_sync_active_regions_dev(int32_t n_samples, int32_t win_begin, int32_t n_pos, const sk_intake_site* dev_sites, const uint8_t* dev_is_candidate,
                               const uint8_t* dev_is_anchor, const int32_t* dev_mark_off, const sk_ploidy_mark* dev_marks, int32_t default_ploidy,
                               const sk_sync_state* dev_state_in, sk_sync_state* dev_state_out, int32_t do_clear, const int32_t* buf_begin,
                               const int32_t* buf_end, sk_sync_region* dev_regions, int64_t region_cap, int32_t* dev_n_regions, int32_t* dev_region_id,
                               void* hip_stream)
{
    if (const char* why = ar_sync_issue(n_samples, win_begin, n_pos, default_ploidy, region_cap)) return sk_fail(std::string("sk_sync_active_regions_dev: ") + why);
    if (!dev_mark_off || !dev_state_in || !dev_state_out || !dev_regions || !dev_n_regions || (n_pos > 0 && (!dev_sites || !dev_is_candidate || !dev_is_anchor)) ||
        (do_clear && (!buf_begin || !buf_end)))
        return sk_fail("sk_sync_active_regions_dev: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    SyncArgs a = {};
    a.n_samples = n_samples;
    a.win_begin = win_begin;
    a.n_pos = n_pos;
    a.sites = dev_sites;
    a.is_candidate = dev_is_candidate;
    a.is_anchor = dev_is_anchor;
    a.mark_off = dev_mark_off;
    a.marks = dev_marks;
    a.default_ploidy = default_ploidy;
    a.state_in = dev_state_in;
    a.state_out = dev_state_out;
    a.do_clear = do_clear ? 1 : 0;
    for (int s = 0; s < n_samples && do_clear; ++s) {
        a.buf_begin[s] = buf_begin[s];
        a.buf_end[s] = buf_end[s];
    }
    a.regions = dev_regions;
    a.region_cap = region_cap;
    a.n_regions = dev_n_regions;
    a.err = sk_ctx().dev_error_flags;
    SK_LAUNCH(ar_sync_walk_kernel, dim3(1), dim3(AR_WALK_THREADS), 0, st, a);
    if (dev_region_id && n_pos > 0)
        SK_LAUNCH(ar_sync_region_id_kernel, dim3(unsigned((n_pos + AR_SYNC_ID_THREADS - 1) / AR_SYNC_ID_THREADS)), dim3(AR_SYNC_ID_THREADS), 0, st, win_begin, n_pos, dev_regions,
                  dev_n_regions, region_cap, dev_region_id);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_sync_active_regions(int32_t n_samples, int32_t win_begin, int32_t n_pos, const sk_intake_site* sites, const uint8_t* is_candidate,
                           const uint8_t* is_anchor, const int32_t* mark_off, const sk_ploidy_mark* marks, int32_t default_ploidy,
                           const sk_sync_state* state_in, sk_sync_state* state_out, int32_t do_clear, const int32_t* buf_begin, const int32_t* buf_end,
                           sk_sync_region* regions, int64_t region_cap, int32_t* n_regions, int32_t* region_id)
{
    if (const char* why = ar_sync_issue(n_samples, win_begin, n_pos, default_ploidy, region_cap)) return sk_fail(std::string("sk_sync_active_regions: ") + why);
    if (!mark_off || !state_in || !state_out || !regions || !n_regions || (n_pos > 0 && (!sites || !is_candidate || !is_anchor)) || (do_clear && (!buf_begin || !buf_end)))
        return sk_fail("sk_sync_active_regions: null argument");
    if (mark_off[0] < 0) return sk_fail("sk_sync_active_regions: negative size (mark_off[0] below zero)");
    for (int32_t s = 0; s < n_samples; ++s) {
        if (mark_off[s + 1] < mark_off[s]) return sk_fail("sk_sync_active_regions: negative size (mark_off is not ascending)");
        if (mark_off[s + 1] > mark_off[s] && !marks) return sk_fail("sk_sync_active_regions: null argument");
        for (int32_t k = mark_off[s]; k < mark_off[s + 1]; ++k) {
            if (marks[k].ploidy != 1 && marks[k].ploidy != 2)
                return sk_fail("sk_sync_active_regions: sample " + std::to_string(s) + ": the mark at " + std::to_string(marks[k].pos) + " holds a ploidy other than 1 or 2");
            if (k + 1 < mark_off[s + 1] && !(marks[k].pos < marks[k + 1].pos))
                return sk_fail("sk_sync_active_regions: sample " + std::to_string(s) + ": the ploidy marks are not in ascending order of position");
        }
    }
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t np = size_t(n_pos), ns = size_t(n_samples), n_marks = size_t(mark_off[n_samples]);
    const int64_t bound = sk_sync_regions_bound(n_pos);
    struct { sk_intake_site* sites; uint8_t* cand; uint8_t* anchor; int32_t* mark_off; sk_ploidy_mark* marks; sk_sync_state* state_in; sk_sync_state* state_out;
             sk_sync_region* regions; int32_t* n; int32_t* region_id; } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(sites, ns * np, 2, st, rc), ar.up(is_candidate, ns * np, 16, st, rc), ar.up(is_anchor, np, 16, st, rc), ar.up(mark_off, ns + 1, 1, st, rc),
                                ar.up(marks, n_marks, 2, st, rc), ar.up(state_in, 1, 0, st, rc), ar.take<sk_sync_state>(1), ar.take<sk_sync_region>(size_t(bound) + 1),
                                ar.take<int32_t>(1), ar.take<int32_t>(np + 4) };
        }) || rc)
        return 1;
    if (sk_sync_active_regions_dev(n_samples, win_begin, n_pos, d.sites, d.cand, d.anchor, d.mark_off, d.marks, default_ploidy, d.state_in, d.state_out, do_clear, buf_begin,
                                   buf_end, d.regions, bound, d.n, region_id ? d.region_id : nullptr, st))
        return 1;
    sk_sync_state out;
    int32_t n = 0;
    SK_HIP(skrt::memcpyAsync(&out, d.state_out, sizeof(sk_sync_state), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::memcpyAsync(&n, d.n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    if (sk_check_device_errors()) return 1; // an assertion would have fired: nothing is emitted
    if (n < 0 || n > bound) return sk_fail("sk_sync_active_regions: region count out of range");
    if (n > 0) SK_HIP(skrt::memcpyAsync(regions, d.regions, sizeof(sk_sync_region) * size_t(n), hipMemcpyDeviceToHost, st));
    if (region_id && n_pos > 0) SK_HIP(skrt::memcpyAsync(region_id, d.region_id, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st));
    SK_HIP(skrt::streamSynchronize(st));
    *state_out = out;
    *n_regions = n;
    return 0;
}

int sk_sync_region_params_dev(const sk_sync_region* dev_sync_regions, const int32_t* dev_n_regions, int64_t region_cap, int32_t sample, int32_t buf_begin,
                              int32_t buf_end_at_clear, sk_active_region* dev_regions, sk_region_params* dev_params, void* hip_stream)
{
    if (region_cap < 0) return sk_fail("sk_sync_region_params_dev: negative size");
    if (region_cap > INT32_MAX) return sk_fail("sk_sync_region_params_dev: region_cap beyond int32");
    if (sample < 0 || sample >= SK_MAX_SAMPLES) return sk_fail("sk_sync_region_params_dev: sample outside 0..SK_MAX_SAMPLES - 1");
    if (!dev_n_regions || (region_cap > 0 && (!dev_sync_regions || !dev_params))) return sk_fail("sk_sync_region_params_dev: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (region_cap > 0)
        SK_LAUNCH(ar_sync_params_kernel, dim3(unsigned((region_cap + 255) / 256)), dim3(256), 0, st, dev_sync_regions, dev_n_regions, region_cap, sample, buf_begin, buf_end_at_clear,
                  dev_regions, dev_params);
    SK_HIP(skrt::getLastError());
    return 0;
}

int sk_sync_region_params(const sk_sync_region* sync_regions, int32_t n_regions, int32_t sample, int32_t buf_begin, int32_t buf_end_at_clear,
                          sk_active_region* regions, sk_region_params* params)
{
    if (n_regions < 0) return sk_fail("sk_sync_region_params: negative size");
    if (sample < 0 || sample >= SK_MAX_SAMPLES) return sk_fail("sk_sync_region_params: sample outside 0..SK_MAX_SAMPLES - 1");
    if (n_regions > 0 && (!sync_regions || !params)) return sk_fail("sk_sync_region_params: null argument");
    SK_REQUIRE_INIT();
    skrt::wakeHint();
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    hipStream_t st = ctx.stream;
    const size_t ng = size_t(n_regions);
    struct { sk_sync_region* sync; int32_t* n; sk_active_region* regions; sk_region_params* params; } d;
    int rc = 0;
    if (sk_carve(d, [&](SkArena& ar) {
            return decltype(d){ ar.up(sync_regions, ng, 1, st, rc), ar.up(&n_regions, 1, 0, st, rc), ar.take<sk_active_region>(ng + 2), ar.take<sk_region_params>(ng + 1) };
        }) || rc)
        return 1;
    if (sk_sync_region_params_dev(d.sync, d.n, n_regions, sample, buf_begin, buf_end_at_clear, d.regions, d.params, st)) return 1;
    if (n_regions > 0) {
        if (regions) SK_HIP(skrt::memcpyAsync(regions, d.regions, sizeof(sk_active_region) * ng, hipMemcpyDeviceToHost, st));
        SK_HIP(skrt::memcpyAsync(params, d.params, sizeof(sk_region_params) * ng, hipMemcpyDeviceToHost, st));
    }
    SK_HIP(skrt::streamSynchronize(st));
    return 0;
}

} // extern "C"
