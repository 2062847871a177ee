// pileup_column.h -- a section of pileup.hip: P2, `pileup_column_kernel_t`: 64 loci to a block, a lane a locus, the reads' records
// walked in read order into one column or, in the three-column form, the stream's columns and the MAPQ tracker.  Part of that one
// translation unit (after pileup_read.h), not a reusable interface.
#pragma once

#include "pileup_read.h"

namespace
{

// does a record belong to the requested column?  `part` = 1 selects the second half of SK_PILEUP_CLEAN_TIER2
__device__ __forceinline__ bool rec_selected(const unsigned rec, const int mode, const int part)
{
    if (!(rec & REC_EMIT)) return false;
    const bool t2 = rec & REC_TIER2, filt = rec & (1u << 12), tscf = rec & (1u << 13);
    switch (mode) {
    case SK_PILEUP_RAW_TIER1: return !t2;
    case SK_PILEUP_RAW_TIER2: return t2;
    case SK_PILEUP_CLEAN_TIER1: return !t2 && !filt;
    default: return part == 0 ? (!t2 && (!filt || tscf)) : (t2 && !filt); // PileupCleaner.cpp:43-64
    }
}

// P2: 64 loci to a block, a lane a locus.  THREE = false: the column of a.mode; THREE = true: the raw tier1, raw tier2 and cleaned tier1
// columns (count3 / call_off3 / calls3, in that order) and the MAPQ tracker in the same walk over the records.
// A block is P2_WAVES waves that SHARE the walk: a wave takes one run of the reads that reach the block's loci (the reads [lo, hi) in
// P2_WAVES consecutive pieces), so a locus' column is its lanes' pieces one after the other -- the count pass adds the waves' counts up,
// the store pass counts its piece first (the same walk, nothing stored), starts its cursors behind the earlier waves' pieces and walks
// again.  With one wave a window's two passes took 2 x 64 us of a push's 310 us on the device: a wave per 64 loci is 128 waves for a
// window, each a chain of ~60 dependent record loads (profiles/r06_v49_stream_window_kernel_stats.csv).
// A launch that fills the device anyway (the one-shot entry point at bench size: 61 000 blocks) keeps one wave to a block: the pieces'
// extra quarter walk and the four searches are then work the device has no idle waves for (2.34 -> 2.90 ms with four).
#ifndef SK_P2_WAVES
#define SK_P2_WAVES 4 // (experiments: 2, 8)
#endif
constexpr int P2_WAVES_MAX = SK_P2_WAVES;
constexpr int P2_SPLIT_BELOW_BLOCKS = 2048; // (8 waves to each of 256 CUs)
template <bool THREE, bool SOM = false, bool EVS = false, int P2_WAVES = P2_WAVES_MAX>
__global__ __launch_bounds__(WAVE* P2_WAVES) void pileup_column_kernel_t(const PileupArgs a)
{
    static_assert(THREE || !(SOM || EVS), "the somatic / EVS columns extend the three-column form");
    const int lane = threadIdx.x & (WAVE - 1);
    const int sub = __builtin_amdgcn_readfirstlane(int(threadIdx.x) / WAVE); // the wave's piece of the reads
    const int l0 = blockIdx.x * WAVE;
    const int l = l0 + lane;
    const int p0 = a.o.report_begin + l0;
    const int p = p0 + lane;
    const int n = a.b.n_reads;
    // reads [lo, hi): lo = first read whose prefix-max end exceeds p0; hi = first read from which every begin >= p0+64
    // 64-ary searches: the lanes probe 64 evenly spaced elements per step, so a range of 2^20 reads takes 4 dependent
    // loads instead of the 20 of a binary search (those 2 x 20 round trips were most of this kernel's time)
    auto first_true = [&](int x, int y, auto&& pred) { // first index in [x, y) with pred, y if none; pred is monotone
        while (x < y) {
            const int span = y - x;
            const int step = (span + WAVE - 1) / WAVE;
            const int m = x + lane * step;
            const bool valid = (m < y);
            const bool v = valid ? pred(m) : true;
            const unsigned long long hit = __ballot(v);                 // lanes past the range report true
            const int f = hit ? __ffsll((long long)hit) - 1 : WAVE;    // first true probe; WAVE: every probe was false
            const int mf = x + f * step;
            if (step == 1) return (mf < y) ? mf : y;
            const int nx = (f == 0) ? x : x + (f - 1) * step + 1;
            y = (mf < y) ? mf : y;
            x = nx;
        }
        return y;
    };
    const int lo_all = first_true(0, n, [&](const int m) { return a.maxend[m] > p0; });
    const int hi_all = first_true(lo_all, n, [&](const int m) { return a.minbegin[m] >= p0 + WAVE; });
    unsigned cnt = 0, cnt2 = 0, cnt3 = 0, cnt4a = 0, cnt4b = 0;
    unsigned mq_n = 0, mq_zero = 0;
    unsigned long long mq_sq = 0;
    const int64_t* __restrict__ off_a = THREE ? a.call_off3[0] : a.call_off;
    uint16_t* __restrict__ calls_a = THREE ? a.calls3[0] : a.calls;
    const int64_t base = (a.store && l < a.n_loci) ? off_a[l] : 0;
    const int64_t base2 = (THREE && a.store && l < a.n_loci) ? a.call_off3[1][l] : 0;
    const int64_t base3 = (THREE && a.store && l < a.n_loci) ? a.call_off3[2][l] : 0;
    const int64_t base4a = (SOM && a.store && l < a.n_loci) ? a.call_off4[l] : 0;
    const int64_t base4b = (SOM && a.store && l < a.n_loci) ? base4a + int64_t(a.count4a[l]) : 0;
    const int64_t base_e = (EVS && a.store && l < a.n_loci) ? a.evs_off[l] : 0;
    unsigned cnt_e = 0;
    const int parts = (!THREE && a.mode == SK_PILEUP_CLEAN_TIER2) ? 2 : 1;
    // (the two-part column -- every read's first-part calls, then every read's second-part calls -- stays one wave's walk)
    const int piece = (parts == 2) ? (hi_all - lo_all) : (hi_all - lo_all + P2_WAVES - 1) / P2_WAVES;
    const int lo = (parts == 2) ? (sub == 0 ? lo_all : hi_all) : min(hi_all, lo_all + sub * piece);
    const int hi = (parts == 2) ? hi_all : min(hi_all, lo + piece);
    const bool live = (l < a.n_loci);
    // store pass: the wave's 64 columns are one contiguous span of `calls`; it is assembled in LDS and written out with
    // consecutive stores (a lane storing 2 bytes every ~80 bytes costs a 32-byte memory transaction per call)
    __shared__ uint16_t s_col[COL_STAGE];
    __shared__ uint16_t s_col3[THREE ? COL_STAGE : 1];
    int64_t span0 = 0, span0c = 0;
    int span_n = 0, span_nc = 0;
    bool staged = false;
    if (a.store) {
        span0 = off_a[min(l0, a.n_loci)];
        const int64_t tot = off_a[min(l0 + WAVE, a.n_loci)] - span0;
        staged = (tot <= COL_STAGE); // (the cleaned column is a subset of the raw tier1 one: it fits whenever that does)
        span_n = staged ? int(tot) : 0;
        if (THREE) {
            span0c = a.call_off3[2][min(l0, a.n_loci)];
            span_nc = staged ? int(a.call_off3[2][min(l0 + WAVE, a.n_loci)] - span0c) : 0;
        }
    }
    const unsigned lbase = unsigned(base - span0);
    const unsigned lbase3 = unsigned(base3 - span0c);
    // Index of the record read k of the batch contributes to this lane's locus (-1: none).  A locus lies in at most one
    // match segment of a read.  The segments of reads with up to three segments were decoded by the lane that fetched the
    // read (mb/me/mr: reference begin / end and read begin of its match segments, empty ranges otherwise), so per read
    // the wave only broadcasts nine integers and does three range tests; longer paths are walked segment by segment.
    auto locate = [&](const int2 sp, const int64_t ro_k, const int64_t so_k, const int nseg_k, const int (&mb)[3], const int (&me)[3],
                      const int (&mr)[3], const int k) -> int64_t {
        const int sx = __builtin_amdgcn_readlane(sp.x, k), sy = __builtin_amdgcn_readlane(sp.y, k);
        if (sy <= p0 || sx >= p0 + WAVE) return -1;
        const int64_t ro = (int64_t(__builtin_amdgcn_readlane(int(ro_k >> 32), k)) << 32) |
                           uint32_t(__builtin_amdgcn_readlane(int(ro_k & 0xffffffff), k));
        const int nseg = __builtin_amdgcn_readlane(nseg_k, k);
        int off = -1;
        if (nseg <= 3) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int b = __builtin_amdgcn_readlane(mb[i], k), e = __builtin_amdgcn_readlane(me[i], k);
                const int r = __builtin_amdgcn_readlane(mr[i], k);
                off = (p >= b && p < e) ? r + (p - b) : off;
            }
        } else {
            const int64_t so = (int64_t(__builtin_amdgcn_readlane(int(so_k >> 32), k)) << 32) |
                               uint32_t(__builtin_amdgcn_readlane(int(so_k & 0xffffffff), k));
            int read_head = 0, ref_head = sx;
            for (int i = 0; i < nseg; ++i) {
                const uint32_t t = a.b.path[so + i].type;
                const int len = int(a.b.path[so + i].length);
                if (seg_match(t) && p >= ref_head && p < ref_head + len) off = read_head + (p - ref_head);
                if (seg_read_len(t)) read_head += len;
                if (seg_ref_len(t)) ref_head += len;
                if (ref_head >= p0 + WAVE) break;
            }
        }
        return (live && off >= 0) ? ro + off : int64_t(-1);
    };
    constexpr int RU = 8; // reads whose record loads are in flight together
    // the wave's walk over its piece of the reads; store = false: only the counters move
    auto walk = [&](const bool store) {
    for (int part = 0; part < parts; ++part) {
        for (int rb = lo; rb < hi; rb += WAVE) {
            // the lanes fetch the geometry of 64 reads at once (one memory round trip instead of one per read); the
            // loops below read it back lane by lane into scalar registers
            const int rk = rb + lane;
            const bool have = (rk < hi);
            const int2 sp = have ? a.span[rk] : make_int2(INT_MAX, INT_MIN);
            const int64_t ro_k = have ? a.b.read_off[rk] : 0;
            const int64_t so_k = have ? a.b.path_off[rk] : 0;
            const int nseg_k = have ? int(a.b.path_off[rk + 1] - so_k) : 0;
            const int mapq_k = (THREE && have) ? int(a.b.mapq[rk]) : 0;
            const int len_k = ((SOM || EVS) && have) ? int(a.b.read_off[rk + 1] - ro_k) : 0;
            sk_path_seg g0 = { 0u, 0u }, g1 = { 0u, 0u }, g2 = { 0u, 0u };
            if (nseg_k >= 1) g0 = a.b.path[so_k];
            if (nseg_k >= 2) g1 = a.b.path[so_k + 1];
            if (nseg_k >= 3) g2 = a.b.path[so_k + 2];
            int mb[3], me[3], mr[3];
            {
                int read_head = 0, ref_head = sp.x;
                const sk_path_seg gs[3] = { g0, g1, g2 };
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const uint32_t t = gs[i].type;
                    const int len = int(gs[i].length);
                    const bool is_m = (i < nseg_k) && seg_match(t);
                    mb[i] = is_m ? ref_head : INT_MAX;
                    me[i] = is_m ? ref_head + len : INT_MIN;
                    mr[i] = read_head;
                    if (i < nseg_k && seg_read_len(t)) read_head += len;
                    if (i < nseg_k && seg_ref_len(t)) ref_head += len;
                }
            }
            const int nk = min(WAVE, hi - rb);
            // RU reads at a time: all their record loads are issued before the first is consumed (one dependent load per
            // read was the whole cost of this kernel); the calls are still appended in read order
            for (int k0 = 0; k0 < nk; k0 += RU) {
                int64_t idx[RU];
#pragma unroll
                for (int u = 0; u < RU; ++u) idx[u] = (k0 + u < nk) ? locate(sp, ro_k, so_k, nseg_k, mb, me, mr, k0 + u) : -1;
                unsigned rec[RU];
#pragma unroll
                for (int u = 0; u < RU; ++u) rec[u] = (idx[u] >= 0) ? unsigned(a.rec[idx[u]]) : 0u;
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    if (THREE) {
                        if (idx[u] < 0) continue;
                        const unsigned rc = rec[u];
                        const uint16_t call = uint16_t(rc & 0x3fffu);
                        if (rc & REC_EMIT) {
                            if (rc & REC_TIER2) {
                                if (store) a.calls3[1][base2 + cnt2] = call;
                                ++cnt2;
                            } else {
                                if (store) {
                                    if (staged) s_col[lbase + cnt] = call;
                                    else calls_a[base + cnt] = call;
                                    if (SOM && a.read_pos) {
                                        const int64_t ro_u = (int64_t(__builtin_amdgcn_readlane(int(ro_k >> 32), k0 + u)) << 32) |
                                                             uint32_t(__builtin_amdgcn_readlane(int(ro_k & 0xffffffff), k0 + u));
                                        const unsigned len_u = unsigned(__builtin_amdgcn_readlane(len_k, k0 + u));
                                        a.read_pos[base + cnt] = unsigned(idx[u] - ro_u) | (len_u << 16);
                                    }
                                }
                                ++cnt;
                                if (!(rc & (1u << 12))) {
                                    if (store) {
                                        if (staged) s_col3[lbase3 + cnt3] = call;
                                        else a.calls3[2][base3 + cnt3] = call;
                                    }
                                    ++cnt3;
                                }
                            }
                            if (SOM) { // the fourth column's two parts
                                const bool t2 = rc & REC_TIER2, filt = rc & (1u << 12), tscf = rc & (1u << 13);
                                if (!t2 && (!filt || tscf)) {
                                    if (store) a.calls4[base4a + cnt4a] = call;
                                    ++cnt4a;
                                } else if (t2 && !filt) {
                                    if (store) a.calls4[base4b + cnt4b] = call;
                                    ++cnt4b;
                                }
                            }
                        }
                        if (EVS && store && ((rc & REC_EMIT) || rc == REC_SUBLIVE)) {
                            const int64_t ro_u = (int64_t(__builtin_amdgcn_readlane(int(ro_k >> 32), k0 + u)) << 32) |
                                                 uint32_t(__builtin_amdgcn_readlane(int(ro_k & 0xffffffff), k0 + u));
                            const unsigned len_u = unsigned(__builtin_amdgcn_readlane(len_k, k0 + u));
                            const unsigned mq = unsigned(__builtin_amdgcn_readlane(mapq_k, k0 + u));
                            const unsigned rp = unsigned(idx[u] - ro_u);
                            const unsigned code = a.b.read_code[idx[u]];
                            const unsigned id = code == SK_BAM_A ? 0u : code == SK_BAM_C ? 1u : code == SK_BAM_G ? 2u : code == SK_BAM_T ? 3u : 4u;
                            const unsigned q0 = a.b.read_qual[idx[u]];
                            const unsigned adj = mq < 5u ? 5u : mq; // pileup_read_segment :1181-1184
                            const bool mapq_adjust = a.o.is_mapq_adjust && (adj <= 80u);
                            const unsigned q = mapq_adjust ? unsigned(a.tab->mappedq[adj][q0 > 70u ? 70u : q0]) : q0;
                            const bool sub = (rc == REC_SUBLIVE);
                            const bool fwd = (rc >> 10) & 1u; // (a submapped position has no strand in its record; its cycle is never read)
                            const unsigned cycle = fwd ? rp : (len_u - (rp + 1u));
                            const unsigned edge = min(min(rp, len_u - (rp + 1u)), 20u);
                            // (a submapped position only feeds the MAPQ rank sum: its other fields are left 0)
                            a.evs_words[base_e + cnt_e] =
                                sub ? ((unsigned long long)id | ((unsigned long long)mq << 3) | (1ull << 34))
                                    : ((unsigned long long)id | ((unsigned long long)mq << 3) | ((unsigned long long)q << 11) |
                                       ((unsigned long long)cycle << 18) | ((unsigned long long)edge << 29));
                            ++cnt_e;
                        }
                        if (!store && ((rc & REC_EMIT) || rc == REC_SUBLIVE)) { // MapqTracker::add (L/blt_common/MapqTracker.hh:36-42)
                            const unsigned mq = unsigned(__builtin_amdgcn_readlane(mapq_k, k0 + u));
                            ++mq_n;
                            mq_sq += (unsigned long long)(mq * mq);
                            mq_zero += (mq == 0u) ? 1u : 0u;
                        }
                    } else if (idx[u] >= 0 && rec_selected(rec[u], a.mode, part)) {
                        if (store) {
                            if (staged) s_col[lbase + cnt] = uint16_t(rec[u] & 0x3fffu);
                            else calls_a[base + cnt] = uint16_t(rec[u] & 0x3fffu);
                        }
                        ++cnt;
                    }
                }
            }
        }
    }
    };
    // the waves' counts meet in LDS: [counter][wave][lane]
    __shared__ unsigned s_part[8][P2_WAVES][WAVE];
    __shared__ unsigned long long s_part_sq[P2_WAVES][WAVE];
    auto publish = [&]() {
        s_part[0][sub][lane] = cnt; s_part[1][sub][lane] = cnt2; s_part[2][sub][lane] = cnt3; s_part[3][sub][lane] = cnt4a;
        s_part[4][sub][lane] = cnt4b; s_part[5][sub][lane] = cnt_e; s_part[6][sub][lane] = mq_n; s_part[7][sub][lane] = mq_zero;
        s_part_sq[sub][lane] = mq_sq;
        __syncthreads();
    };
    if (P2_WAVES == 1) {
        walk(a.store != 0);
    } else if (!a.store) {
        walk(false);
        publish();
        if (sub != 0) return;
        cnt = cnt2 = cnt3 = cnt4a = cnt4b = cnt_e = mq_n = mq_zero = 0;
        mq_sq = 0;
#pragma unroll
        for (int w = 0; w < P2_WAVES; ++w) {
            cnt += s_part[0][w][lane]; cnt2 += s_part[1][w][lane]; cnt3 += s_part[2][w][lane]; cnt4a += s_part[3][w][lane];
            cnt4b += s_part[4][w][lane]; cnt_e += s_part[5][w][lane]; mq_n += s_part[6][w][lane]; mq_zero += s_part[7][w][lane];
            mq_sq += s_part_sq[w][lane];
        }
    } else {
        // where this wave's piece of every column starts: behind the pieces of the waves before it
        walk(false);
        publish();
        cnt = cnt2 = cnt3 = cnt4a = cnt4b = cnt_e = 0;
#pragma unroll
        for (int w = 0; w < P2_WAVES; ++w) {
            if (w < sub) {
                cnt += s_part[0][w][lane]; cnt2 += s_part[1][w][lane]; cnt3 += s_part[2][w][lane]; cnt4a += s_part[3][w][lane];
                cnt4b += s_part[4][w][lane];
                cnt_e += s_part[6][w][lane]; // (a locus has one EVS word per MAPQ-tracker entry: counted as mq_n when nothing is stored)
            }
        }
        walk(true);
    }
    if (!a.store && l <= a.n_loci) {
        if (THREE) {
            a.count3[0][l] = (l < a.n_loci) ? cnt : 0u;
            a.count3[1][l] = (l < a.n_loci) ? cnt2 : 0u;
            a.count3[2][l] = (l < a.n_loci) ? cnt3 : 0u;
            if (SOM) {
                a.count4[l] = (l < a.n_loci) ? cnt4a + cnt4b : 0u;
                a.count4a[l] = (l < a.n_loci) ? cnt4a : 0u;
            }
            if (l < a.n_loci) {
                a.mapq_count[l] = mq_n;
                a.mapq_zero[l] = mq_zero;
                a.mapq_sumsq[l] = mq_sq;
            } else {
                a.mapq_count[l] = 0; // (entry n_loci of the counts, as the columns' have)
            }
        } else {
            a.count[l] = (l < a.n_loci) ? cnt : 0u;
        }
    }
    if (a.store && staged) { // (`staged` is the block's: every wave comes here)
        __syncthreads();
        uint16_t* __restrict__ dst = calls_a + span0;
        for (int i = int(threadIdx.x); i < span_n; i += WAVE * P2_WAVES) dst[i] = s_col[i];
        if (THREE) {
            uint16_t* __restrict__ dst3 = a.calls3[2] + span0c;
            for (int i = int(threadIdx.x); i < span_nc; i += WAVE * P2_WAVES) dst3[i] = s_col3[i];
        }
    }
}

} // namespace
