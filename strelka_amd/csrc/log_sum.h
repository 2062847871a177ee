// log_sum.h -- the reference's two-term log-sums, float (somatic_site.hip: the strand states) and double (indel_lhood.hip: every
// read's term), in one place so that the libm probe (libm_probe.hip, sk_debug_libm_eval) calls the very functions the kernels call.
#pragma once

#include "libm_dbl64.h"

#include <cmath>

namespace
{

// getLogSum<float>, L/blt_util/logSumUtil.hh:33-41 with log1p_switch<float>, L/blt_util/math_util.hh:33-48: the reference's
// expf / log1pf / logf are the host libm's, restated for the device in libm_flt32.h; the device library's double-precision
// functions rounded once stand in when the host libm is another implementation (sk_libm_restated() == 0)
__device__ __forceinline__ float log_sum2f(float x1, float x2, const int exact_libm)
{
    if (x1 < x2) {
        const float t = x1;
        x1 = x2;
        x2 = t;
    }
    const float d = __fsub_rn(x2, x1);
    float e, l;
    if (!(exact_libm && sk_libm::expf_glibc(d, e))) e = static_cast<float>(exp(static_cast<double>(d)));
    if (fabsf(e) < 0.01f) {
        if (!(exact_libm && sk_libm::log1pf_glibc(e, l))) l = static_cast<float>(log1p(static_cast<double>(e)));
    } else {
        const float one_e = __fadd_rn(1.f, e);
        if (!(exact_libm && sk_libm::logf_glibc(one_e, l))) l = static_cast<float>(log(static_cast<double>(one_e)));
    }
    return __fadd_rn(x1, l);
}

// log1p_switch / getLogSum, L/blt_util/math_util.hh:33-48, L/blt_util/logSumUtil.hh:33-41 (double)
__device__ __forceinline__ double log1p_switch_d(const double x, const int ex, const SkLibmTables& lt)
{
    return (fabs(x) < 0.01) ? sk_log1p(x, ex) : sk_log(__dadd_rn(1., x), ex, lt);
}
__device__ __forceinline__ double log_sum2(double x1, double x2, const int ex, const SkLibmTables& lt)
{
    if (x1 < x2) {
        const double t = x1;
        x1 = x2;
        x2 = t;
    }
    return __dadd_rn(x1, log1p_switch_d(sk_exp(__dsub_rn(x2, x1), ex, lt), ex, lt));
}

} // namespace
