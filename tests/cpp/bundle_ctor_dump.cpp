// tests/cpp/bundle_ctor_dump.cpp -- writes the rays of the host mirror's ImagePlaneBundles<double> constructor (raytrace_cpu_amd/host/raytracer/
// imageplane_bundles.h) to a file: int32 count, then count 144-byte records.  Constructing the object makes no GPU call.  Compiled by the tests that
// use it (tests/test_caustic_rules.py, tests/test_gpu_caustic.py) into their temporary directory, with the flags of tests/cpp/Makefile's host_ctor_dump.
//   bundle_ctor_dump <outfile> dist incl x0 xmax dx y0 ymax dy spin phi0 eps_frac
#include <cstdio>
#include <cstdlib>

#include "raytracer/imageplane_bundles.h"

int main(int argc, char** argv)
{
    if (argc != 2 + 11) {
        std::fprintf(stderr, "usage: %s outfile dist incl x0 xmax dx y0 ymax dy spin phi0 eps_frac\n", argv[0]);
        return 2;
    }
    auto arg = [&](int i) { return std::strtod(argv[2 + i], nullptr); };
    ImagePlaneBundles<double> s(arg(0), arg(1), arg(2), arg(3), arg(4), arg(5), arg(6), arg(7), arg(8), arg(9), PRECISION, arg(10));
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    const int n = s.get_count();
    const bool ok = std::fwrite(&n, 4, 1, f) == 1 && std::fwrite(s.rays, sizeof(Ray<double>), n, f) == (size_t) n;
    return std::fclose(f) == 0 && ok ? 0 : 4;
}
