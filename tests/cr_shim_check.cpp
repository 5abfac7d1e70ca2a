// TEST INFRASTRUCTURE: csrc/kr_sincos.hpp and csrc/kr_crmath.hpp compiled for the host DIRECTLY (no shim, no shared library), applied to a file of
// arguments: tests/test_oracle_cr.py compares the bits with what oracle/cr_math_shim.cpp's entry points return for the same arguments.
// usage: cr_shim_check OP IN OUT   -- OP: 0 sin, 1 cos, 2 acos, 3 asin, 4 atan2(a, b), 5 tan; IN: raw doubles, a[n] (op 4: a[n] then b[n]); OUT: raw doubles
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../raytrace_cpu_amd/csrc/kr_crmath.hpp"

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int op = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> in(bytes / sizeof(double));
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 4;
    fclose(f);
    const size_t n = op == 4 ? in.size() / 2 : in.size();
    std::vector<double> out(n);
    for (size_t i = 0; i < n; i++) {
        const double x = in[i];
        double s, c;
        switch (op) {
            case 0: kr_sincos_f64(x, s, c); out[i] = s; break;
            case 1: kr_sincos_f64(x, s, c); out[i] = c; break;
            case 2: out[i] = krcr::kr_acos_cr(x); break;
            case 3: out[i] = krcr::kr_asin_cr(x); break;
            case 4: out[i] = krcr::kr_atan2_cr(x, in[n + i]); break;
            case 5: out[i] = krcr::kr_tan_cr(x); break;
            default: return 5;
        }
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), sizeof(double), n, f) != n) return 6;
    fclose(f);
    return 0;
}
