// libm_probe.h -- the kernel skeleton of sk_debug_libm_eval (libm_probe.hip), shared with libm_probe_germline.hip.
//
// Two sources because the germline and the somatic callers each state error_prob_to_qphred_d (germline_common.h: sk_log10 inlined;
// somatic_common.h: the out-of-line twin sk_log10_call) under the same name, so one translation unit cannot see both.  Each source
// includes the header of the kernels it stands for and calls those functions, never a copy.
#pragma once

#include "sk_common.h"
#include "libm_dbl64.h"

struct SkLibmProbeArgs
{
    int64_t n;
    const void* a;
    const void* b;     // second argument of the two-argument functions, else nullptr
    void* out;
    uint8_t* restated; // or nullptr
    int exact_libm;    // the context's, as every kernel takes it
    float ln10f;       // GermlineDerived::ln10f (SK_LIBM_LN_QPHRED_F)
};

enum { SK_LIBM_PROBE_THREADS = 256, SK_LIBM_PROBE_MAX_BLOCKS = 1024 };

template <typename T> __device__ __forceinline__ T probe_ld(const void* p, const int64_t i) { return static_cast<const T*>(p)[i]; }
template <typename T> __device__ __forceinline__ void probe_st(void* p, const int64_t i, const T v) { static_cast<T*>(p)[i] = v; }

// One element per thread, grid-stride.  EVAL::at(p, i, lt) reads a[i] (b[i]), writes out[i] (restated[i]), i < p.n.
// VARIANT 1: the tables are the block's LDS copy; anything else: constant memory.
template <typename EVAL, int VARIANT> __global__ void __launch_bounds__(SK_LIBM_PROBE_THREADS) libm_probe_kernel(const SkLibmProbeArgs p)
{
    __shared__ uint64_t s_tab[VARIANT == 1 ? 512 : 1];
    SkLibmTables lt = sk_libm_tables_default();
    if (VARIANT == 1) {
        lt = sk_libm_tables_to_lds(s_tab, int(threadIdx.x), int(blockDim.x));
        __syncthreads();
    }
    const int64_t stride = int64_t(gridDim.x) * SK_LIBM_PROBE_THREADS;
    for (int64_t i = int64_t(blockIdx.x) * SK_LIBM_PROBE_THREADS + threadIdx.x; i < p.n; i += stride) EVAL::at(p, i, lt);
}

template <typename EVAL, int VARIANT> inline void libm_probe_launch(const SkLibmProbeArgs& p, hipStream_t st)
{
    const int64_t blocks = (p.n + SK_LIBM_PROBE_THREADS - 1) / SK_LIBM_PROBE_THREADS;
    const unsigned grid = unsigned(blocks < SK_LIBM_PROBE_MAX_BLOCKS ? blocks : SK_LIBM_PROBE_MAX_BLOCKS);
    auto kernel = libm_probe_kernel<EVAL, VARIANT>;
    SK_LAUNCH(kernel, dim3(grid), dim3(SK_LIBM_PROBE_THREADS), 0, st, p);
}

/// libm_probe_germline.hip: LOGF_REF, DEPENDENT_EPROB, LN_QPHRED_F (variant 0) and QPHRED_D (variants 0, 1) as germline_common.h
/// states them; fills p.ln10f itself.  false: not one of these.
bool sk_libm_probe_germline(int fn, int variant, SkLibmProbeArgs p, hipStream_t st);
