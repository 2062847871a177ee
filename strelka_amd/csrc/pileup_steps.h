// pileup_steps.h -- a section of pileup.hip: the small launches around P1 and P2 -- the span split of the one-shot entry, the stream's
// carry copies, span bounds and column offsets, the reference base ids.  Part of that one translation unit (its last device section:
// ref_base_id_kernel is the unit's last kernel), not a reusable interface.
#pragma once

#include "sk_common.h"

#include "block_scan.h"

#include <climits>

namespace
{

__global__ void span_split_kernel(const int2* span, int* begin, int* end, const int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        begin[i] = span[i].x;
        end[i] = span[i].y;
    }
}

struct MaxOp
{
    __host__ __device__ int operator()(const int a, const int b) const { return a > b ? a : b; }
};
struct MinOp
{
    __host__ __device__ int operator()(const int a, const int b) const { return a < b ? a : b; }
};

// ---- the stream's small steps as three launches.  A window's push used to be ~30 submissions -- five device-to-device copies of the
// carried tail, the span split, two rocPRIM scans over the reads and three to five over the loci (two launches each), four copies of
// counters into the output block -- around the four kernels that do the work.  Here: one launch copies every carried piece, one makes
// both running bounds of the reads' spans, one makes every column's offsets and moves the counters: ~12 submissions per push.  (It
// is 4 % of a window's 0.45 ms, not more: what a push waits for is P1's latency on 2 200 reads -- 0.11 ms, a chain of dependent loads
// per read -- and the 2.5 MB of columns and records going back to the host.)
struct CopySeg
{
    const char* src;
    char* dst;
    int64_t bytes;
};
struct CopyArgs
{
    CopySeg seg[6];
    int n;
};
// blockIdx.y = the piece, grid-stride over it in 16-byte words where both ends allow
__global__ __launch_bounds__(256) void copy_segments_kernel(const CopyArgs a)
{
    const CopySeg s = a.seg[blockIdx.y];
    const int64_t tid = int64_t(blockIdx.x) * 256 + threadIdx.x, stride = int64_t(gridDim.x) * 256;
    if (((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 15u) == 0) {
        const int64_t words = s.bytes / 16;
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(s.src);
        uint4* __restrict__ dst = reinterpret_cast<uint4*>(s.dst);
        for (int64_t i = tid; i < words; i += stride) dst[i] = src[i];
        for (int64_t i = words * 16 + tid; i < s.bytes; i += stride) s.dst[i] = s.src[i];
    } else {
        for (int64_t i = tid; i < s.bytes; i += stride) s.dst[i] = s.src[i];
    }
}

// block 0: maxend[i] = max of the spans' ends up to read i; block 1: minbegin[i] = min of the spans' begins from read i on
__global__ __launch_bounds__(1024) void span_bounds_kernel(const int2* __restrict__ span, int* __restrict__ maxend, int* __restrict__ minbegin, const int n)
{
    __shared__ int s_wave[16];
    __shared__ int s_carry;
    const bool fwd = (blockIdx.x == 0);
    if (threadIdx.x == 0) s_carry = fwd ? INT_MIN : INT_MAX;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int k = base + int(threadIdx.x);           // position in scan order
        const int i = fwd ? k : n - 1 - k;               // the read
        int v = fwd ? INT_MIN : INT_MAX;
        if (k < n) v = fwd ? span[i].y : span[i].x;
        v = fwd ? block_scan_1024(v, MaxOp(), s_wave) : block_scan_1024(v, MinOp(), s_wave);
        const int carry = s_carry;
        v = fwd ? max(v, carry) : min(v, carry);
        if (k < n) (fwd ? maxend : minbegin)[i] = v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = v;
        __syncthreads();
    }
}

struct OffsetsArgs
{
    const uint32_t* count[5]; // per-locus counts, n + 1 entries each (the last is not read)
    int64_t* off[5];          // exclusive sums, n + 1 entries: off[n] = the total
    int n_scans;
    int n;                    // loci
    CopySeg copy[4];          // counters to move into the output block, a block each
    int n_copies;
};
struct PlusOp
{
    __device__ int64_t operator()(const int64_t a, const int64_t b) const { return a + b; }
};
__global__ __launch_bounds__(1024) void column_offsets_kernel(const OffsetsArgs a)
{
    __shared__ int64_t s_wave[16];
    __shared__ int64_t s_carry;
    if (int(blockIdx.x) >= a.n_scans) {
        const CopySeg s = a.copy[int(blockIdx.x) - a.n_scans];
        for (int64_t i = threadIdx.x; i < s.bytes; i += 1024) s.dst[i] = s.src[i];
        return;
    }
    const uint32_t* __restrict__ cnt = a.count[blockIdx.x];
    int64_t* __restrict__ off = a.off[blockIdx.x];
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base <= a.n; base += 1024) {
        const int i = base + int(threadIdx.x);
        const int64_t c = (i < a.n) ? int64_t(cnt[i]) : 0;
        const int64_t incl = block_scan_1024(c, PlusOp(), s_wave) + s_carry;
        if (i <= a.n) off[i] = incl - c;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = incl;
        __syncthreads();
    }
}

__global__ void ref_base_id_kernel(const char* ref_seq, const int ref_offset, const int ref_len, const int begin, const int n,
                                   uint8_t* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = begin + i - ref_offset;
    uint8_t id = 4;
    if (p >= 0 && p < ref_len) {
        const char c = ref_seq[p];
        id = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
    }
    out[i] = id;
}

} // namespace
