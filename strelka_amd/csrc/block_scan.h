// block_scan.h -- the one block-wide scan the small planning kernels share (pileup_steps.h's column offsets and span bounds,
// indel_table.hip's offsets).  Device code only; include inside a translation unit that has the HIP runtime header.
#pragma once

namespace
{

// a block's inclusive scan of one value per thread (1 024 threads), `op` associative; a caller that scans in chunks joins the chunks'
// carry itself
template <typename T, typename OP>
__device__ __forceinline__ T block_scan_1024(T v, const OP op, T* s_wave /*[16]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d, 64);
        if (lane >= d) v = op(up, v);
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    if (wave > 0) {
        T pre = s_wave[0];
        for (int w = 1; w < wave; ++w) pre = op(pre, s_wave[w]);
        v = op(pre, v);
    }
    __syncthreads();
    return v;
}

} // namespace
