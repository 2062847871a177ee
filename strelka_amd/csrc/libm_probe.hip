// libm_probe.hip -- sk_debug_libm_eval: the device's evaluation of the restated libm routines (libm_flt32.h, libm_dbl64.h) and of the
// scalar functions the kernels build on them, element by element, for tests/test_libm_device.py.  Adds no work to any other kernel.
//
// Every function evaluated here is the one the kernels call, reached through the header that states it: the raw routines and the
// sk_* wrappers from libm_dbl64.h, the log-sums from log_sum.h, the somatic callers' error_prob_to_qphred_d from somatic_common.h;
// the germline kernels' functions live in libm_probe_germline.hip (libm_probe.h says why).
#include "libm_probe.h"
#include "somatic_common.h"
#include "log_sum.h"

namespace
{

// ---- the eight raw routines: out = the result or zero bits, restated = the return value
#define SK_PROBE_RAW1(NAME, T, CALL)                                                                           \
    struct NAME                                                                                                \
    {                                                                                                          \
        static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables& lt) \
        {                                                                                                      \
            const T x = probe_ld<T>(p.a, i);                                                                   \
            T r = T(0);                                                                                        \
            const bool ok = CALL;                                                                              \
            probe_st<T>(p.out, i, ok ? r : T(0));                                                              \
            if (p.restated) p.restated[i] = ok ? 1 : 0;                                                        \
            (void)lt;                                                                                          \
        }                                                                                                      \
    }
SK_PROBE_RAW1(EvLogf, float, sk_libm::logf_glibc(x, r));
SK_PROBE_RAW1(EvExpf, float, sk_libm::expf_glibc(x, r));
SK_PROBE_RAW1(EvLog1pf, float, sk_libm::log1pf_glibc(x, r));
SK_PROBE_RAW1(EvExp, double, sk_libm::exp_glibc(x, r, lt.exp_t));
SK_PROBE_RAW1(EvLog, double, sk_libm::log_glibc(x, r, lt.log_t));
SK_PROBE_RAW1(EvLog10, double, sk_libm::log10_glibc(x, r, lt.log_t));
SK_PROBE_RAW1(EvLog1p, double, sk_libm::log1p_glibc(x, r));
SK_PROBE_RAW1(EvPowf, float, sk_libm::powf_glibc(x, probe_ld<float>(p.b, i), r));
#undef SK_PROBE_RAW1

// ---- what the kernels call: the context's exact_libm, restated = 0
#define SK_PROBE_FN(NAME, TIN, TOUT, EXPR)                                                                     \
    struct NAME                                                                                                \
    {                                                                                                          \
        static __device__ __forceinline__ void at(const SkLibmProbeArgs& p, const int64_t i, const SkLibmTables& lt) \
        {                                                                                                      \
            const TIN x = probe_ld<TIN>(p.a, i);                                                               \
            const int ex = p.exact_libm;                                                                       \
            probe_st<TOUT>(p.out, i, EXPR);                                                                    \
            if (p.restated) p.restated[i] = 0;                                                                 \
            (void)lt;                                                                                          \
            (void)ex;                                                                                          \
        }                                                                                                      \
    }
SK_PROBE_FN(EvSkExp, double, double, sk_exp(x, ex, lt));
SK_PROBE_FN(EvSkLog, double, double, sk_log(x, ex, lt));
SK_PROBE_FN(EvSkLog10, double, double, sk_log10(x, ex, lt));
SK_PROBE_FN(EvSkLog1p, double, double, sk_log1p(x, ex));
SK_PROBE_FN(EvSkExpCall, double, double, sk_exp_call(x, ex, lt));
SK_PROBE_FN(EvSkLogCall, double, double, sk_log_call(x, ex, lt));
SK_PROBE_FN(EvSkLog10Call, double, double, sk_log10_call(x, ex, lt));
SK_PROBE_FN(EvQphredDCall, double, int32_t, error_prob_to_qphred_d(x, ex, lt)); // somatic_common.h: through sk_log10_call
SK_PROBE_FN(EvLog1pSwitchD, double, double, log1p_switch_d(x, ex, lt));
SK_PROBE_FN(EvLogSum2, double, double, log_sum2(x, probe_ld<double>(p.b, i), ex, lt));
SK_PROBE_FN(EvLogSum2f, float, float, log_sum2f(x, probe_ld<float>(p.b, i), ex));
#undef SK_PROBE_FN

struct FnShape
{
    int in_size, out_size; // bytes per element
    bool two_args, takes_tables, has_twin;
};
// indexed by SK_LIBM_*
constexpr FnShape SHAPE[SK_LIBM_FN_COUNT] = {
    { 4, 4, false, false, false }, // LOGF
    { 4, 4, true, false, false },  // POWF
    { 4, 4, false, false, false }, // EXPF
    { 4, 4, false, false, false }, // LOG1PF
    { 8, 8, false, true, false },  // EXP
    { 8, 8, false, true, false },  // LOG
    { 8, 8, false, true, false },  // LOG10
    { 8, 8, false, false, false }, // LOG1P
    { 8, 8, false, true, true },   // SK_EXP
    { 8, 8, false, true, true },   // SK_LOG
    { 8, 8, false, true, true },   // SK_LOG10
    { 8, 8, false, false, false }, // SK_LOG1P
    { 4, 4, false, false, false }, // LOGF_REF
    { 4, 4, true, false, false },  // DEPENDENT_EPROB
    { 4, 4, false, false, false }, // LN_QPHRED_F
    { 8, 4, false, true, true },   // QPHRED_D
    { 8, 8, false, true, false },  // LOG1P_SWITCH_D
    { 8, 8, true, true, false },   // LOG_SUM2
    { 4, 4, true, false, false },  // LOG_SUM2F
};

template <typename EV> void launch01(const int variant, const SkLibmProbeArgs& p, hipStream_t st)
{
    if (variant == 1) libm_probe_launch<EV, 1>(p, st);
    else libm_probe_launch<EV, 0>(p, st);
}

} // namespace

extern "C" int sk_debug_libm_eval(const int fn, const int variant, const int64_t n, const void* a, const void* b, void* out, uint8_t* restated)
{
    SK_REQUIRE_INIT();
    if (fn < 0 || fn >= SK_LIBM_FN_COUNT) {
        sk_fail("sk_debug_libm_eval: no such function");
        return -1;
    }
    const FnShape& sh = SHAPE[fn];
    if (!(variant == 0 || (variant == 1 && sh.takes_tables) || (variant == 2 && sh.has_twin))) {
        sk_fail("sk_debug_libm_eval: this function has no such variant (1: functions that take tables; 2: sk_exp, sk_log, sk_log10, error_prob_to_qphred_d)");
        return -1;
    }
    if (n < 0 || n > (int64_t(1) << 24)) return sk_fail("sk_debug_libm_eval: n out of range");
    if (n == 0) return 0;
    if (!a || !out || (sh.two_args && !b)) return sk_fail("sk_debug_libm_eval: null argument");
    SkContext& ctx = sk_ctx();
    SK_HIP(skrt::setDevice(ctx.device));
    SkStage sg;
    const size_t in_bytes = size_t(n) * sh.in_size, out_bytes = size_t(n) * sh.out_size;
    if (sg.begin(in_bytes * (sh.two_args ? 2 : 1), out_bytes + size_t(n), 0, 4)) return 1;
    SkLibmProbeArgs p;
    p.n = n;
    p.a = sg.put(static_cast<const char*>(a), in_bytes);
    p.b = sh.two_args ? sg.put(static_cast<const char*>(b), in_bytes) : nullptr;
    char* dout = sg.out<char>(out_bytes);
    uint8_t* dres = sg.out<uint8_t>(size_t(n));
    p.out = dout;
    p.restated = restated ? dres : nullptr;
    p.exact_libm = ctx.libm_restated ? 1 : 0;
    p.ln10f = 0.f;
    if (sg.upload(ctx.stream)) return 1;
    hipStream_t st = ctx.stream;
    if (!sk_libm_probe_germline(fn, variant, p, st)) {
        switch (fn) {
        case SK_LIBM_LOGF: libm_probe_launch<EvLogf, 0>(p, st); break;
        case SK_LIBM_POWF: libm_probe_launch<EvPowf, 0>(p, st); break;
        case SK_LIBM_EXPF: libm_probe_launch<EvExpf, 0>(p, st); break;
        case SK_LIBM_LOG1PF: libm_probe_launch<EvLog1pf, 0>(p, st); break;
        case SK_LIBM_EXP: launch01<EvExp>(variant, p, st); break;
        case SK_LIBM_LOG: launch01<EvLog>(variant, p, st); break;
        case SK_LIBM_LOG10: launch01<EvLog10>(variant, p, st); break;
        case SK_LIBM_LOG1P: libm_probe_launch<EvLog1p, 0>(p, st); break;
        case SK_LIBM_SK_EXP:
            if (variant == 2) libm_probe_launch<EvSkExpCall, 2>(p, st);
            else launch01<EvSkExp>(variant, p, st);
            break;
        case SK_LIBM_SK_LOG:
            if (variant == 2) libm_probe_launch<EvSkLogCall, 2>(p, st);
            else launch01<EvSkLog>(variant, p, st);
            break;
        case SK_LIBM_SK_LOG10:
            if (variant == 2) libm_probe_launch<EvSkLog10Call, 2>(p, st);
            else launch01<EvSkLog10>(variant, p, st);
            break;
        case SK_LIBM_SK_LOG1P: libm_probe_launch<EvSkLog1p, 0>(p, st); break;
        case SK_LIBM_QPHRED_D: libm_probe_launch<EvQphredDCall, 2>(p, st); break; // (variants 0 and 1: the germline statement)
        case SK_LIBM_LOG1P_SWITCH_D: launch01<EvLog1pSwitchD>(variant, p, st); break;
        case SK_LIBM_LOG_SUM2: launch01<EvLogSum2>(variant, p, st); break;
        case SK_LIBM_LOG_SUM2F: libm_probe_launch<EvLogSum2f, 0>(p, st); break;
        default: return sk_fail("sk_debug_libm_eval: function not handled");
        }
    }
    if (sg.download_and_wait(ctx.stream)) return 1;
    sg.fetch(static_cast<char*>(out), dout, out_bytes);
    if (restated) sg.fetch(restated, dres, size_t(n));
    return 0;
}
