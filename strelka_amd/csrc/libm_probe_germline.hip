// libm_probe_germline.hip -- sk_debug_libm_eval's functions of the germline kernels (germline_common.h): see libm_probe.h.
#include "libm_probe.h"
#pragma clang diagnostic ignored "-Wunused-function" // (the site kernels' functions of germline_common.h: not called from here)
#include "germline_common.h"

namespace
{

struct EvLogfRef
{
    static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables&)
    {
        probe_st<float>(p.out, i, logf_ref(probe_ld<float>(p.a, i), p.exact_libm));
        if (p.restated) p.restated[i] = 0;
    }
};
struct EvDependentEprob
{
    static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables&)
    {
        probe_st<float>(p.out, i, get_dependent_eprob(probe_ld<float>(p.a, i), probe_ld<float>(p.b, i), p.exact_libm));
        if (p.restated) p.restated[i] = 0;
    }
};
struct EvLnQphredF
{
    static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables&)
    {
        probe_st<int32_t>(p.out, i, ln_error_prob_to_qphred_f(probe_ld<float>(p.a, i), p.ln10f));
        if (p.restated) p.restated[i] = 0;
    }
};
struct EvQphredD
{
    static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables& lt)
    {
        probe_st<int32_t>(p.out, i, error_prob_to_qphred_d(probe_ld<double>(p.a, i), p.exact_libm, lt));
        if (p.restated) p.restated[i] = 0;
    }
};

} // namespace

bool sk_libm_probe_germline(const int fn, const int variant, SkLibmProbeArgs p, hipStream_t st)
{
    if (fn == SK_LIBM_LOGF_REF && variant == 0) libm_probe_launch<EvLogfRef, 0>(p, st);
    else if (fn == SK_LIBM_DEPENDENT_EPROB && variant == 0) libm_probe_launch<EvDependentEprob, 0>(p, st);
    else if (fn == SK_LIBM_LN_QPHRED_F && variant == 0) {
        // ln10f the way the germline kernels take it: GermlineDerived, from the host libm
        sk_germline_options opt;
        sk_germline_options_default(&opt);
        GermlineDerived d;
        derive(opt, d);
        p.ln10f = d.ln10f;
        libm_probe_launch<EvLnQphredF, 0>(p, st);
    } else if (fn == SK_LIBM_QPHRED_D && variant == 0) libm_probe_launch<EvQphredD, 0>(p, st);
    else if (fn == SK_LIBM_QPHRED_D && variant == 1) libm_probe_launch<EvQphredD, 1>(p, st);
    else return false;
    return true;
}
