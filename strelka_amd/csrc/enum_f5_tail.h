// enum_f5_tail.h -- a section of read_enumerate.hip: the order of an F5 launch's last hand-outs -- tail_order_kernel, its launcher, and
// the window's shift and length (f5_tail_shift, f5_tail_window), which the driver names in the launch's arguments (plan_tail).
// Part of that one translation unit (after enum_f5.h, before enum_entries.h), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "enum_search.h"

#include <algorithm>
#include <cstdlib>

namespace
{

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

} // namespace
