// libm_header_eval.cpp -- TEST INFRASTRUCTURE: strelka_amd/csrc/libm_flt32.h and libm_dbl64.h compiled for the HOST (as
// libm_check.cpp does, -ffp-contract=off) and evaluated over arrays: sko_libm_header_eval of strelka_oracle.h.  The tests use it to
// show that their case sets are ones on which the restatement agrees with the host libm, and for the expected `restated` flags
// of the device (tests/test_libm_restatement.py, tests/test_libm_device.py).
#include "../strelka_amd/csrc/libm_dbl64.h"
#include "strelka_oracle.h"

using namespace sk_libm;

extern "C" int sko_libm_header_eval(int fn, int64_t n, const void* a, const void* b, void* out, uint8_t* restated)
{
    const volatile float* af = static_cast<const volatile float*>(a);
    const volatile float* bf = static_cast<const volatile float*>(b);
    const volatile double* ad = static_cast<const volatile double*>(a);
    float* of = static_cast<float*>(out);
    double* od = static_cast<double*>(out);
    if (fn < 0 || fn > 7) return 1;
    for (int64_t i = 0; i < n; ++i) {
        bool ok = false;
        if (fn < 4) {
            float r = 0.f;
            const float x = af[i];
            switch (fn) {
            case 0: ok = logf_glibc(x, r); break;
            case 1: ok = powf_glibc(x, bf[i], r); break;
            case 2: ok = expf_glibc(x, r); break;
            default: ok = log1pf_glibc(x, r); break;
            }
            of[i] = ok ? r : 0.f;
        } else {
            double r = 0.;
            const double x = ad[i];
            switch (fn) {
            case 4: ok = exp_glibc(x, r); break;
            case 5: ok = log_glibc(x, r); break;
            case 6: ok = log10_glibc(x, r); break;
            default: ok = log1p_glibc(x, r); break;
            }
            od[i] = ok ? r : 0.;
        }
        if (restated) restated[i] = ok ? 1 : 0;
    }
    return 0;
}
