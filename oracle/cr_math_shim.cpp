// oracle/cr_math_shim.cpp -- TEST INFRASTRUCTURE.  The device's own elementary functions, compiled for the host, behind C names: what
// libkr_oracle_cr.so (kr_oracle.c built with -DKRO_CR_MATH) calls where the plain oracle calls the C library.  Nothing is restated here: the two
// headers ARE the device code (they compile as host C++ so that tests/sincos_check.cpp and tests/crmath_check.cpp can measure them), so the
// correctly rounded oracle and a strict device trace evaluate the same operations in the same order -- built, like the oracle, without contraction.
#include <stdint.h>

#include "../raytrace_cpu_amd/csrc/kr_crmath.hpp"

extern "C" {

// kr_arith.hpp's kr_sin / kr_cos: one half of kr_sincos_f64's pair
double kro_cr_sin(double x) { double s, c; kr_sincos_f64(x, s, c); return s; }
double kro_cr_cos(double x) { double s, c; kr_sincos_f64(x, s, c); return c; }
double kro_cr_acos(double x) { return krcr::kr_acos_cr(x); }
double kro_cr_asin(double x) { return krcr::kr_asin_cr(x); }
double kro_cr_atan2(double y, double x) { return krcr::kr_atan2_cr(y, x); }
double kro_cr_tan(double x) { return krcr::kr_tan_cr(x); }

// the same over arrays, for the tests (op: 0 sin, 1 cos, 2 acos, 3 asin, 4 atan2(a, b), 5 tan); returns 0, or -1 for an unknown op
int kro_cr_apply(int op, const double* a, const double* b, double* out, int64_t n)
{
    if (op < 0 || op > 5) return -1;
    for (int64_t i = 0; i < n; i++) {
        switch (op) {
            case 0: out[i] = kro_cr_sin(a[i]); break;
            case 1: out[i] = kro_cr_cos(a[i]); break;
            case 2: out[i] = kro_cr_acos(a[i]); break;
            case 3: out[i] = kro_cr_asin(a[i]); break;
            case 4: out[i] = kro_cr_atan2(a[i], b[i]); break;
            case 5: out[i] = kro_cr_tan(a[i]); break;
        }
    }
    return 0;
}

}  // extern "C"
