// tests/cpp/vel_tetrad_check.cpp -- the host tetrad of the point source with any four-velocity (raytrace_cpu_amd/csrc/kr_vel_tetrad.hpp) in a
// stand-alone program, for a sanitizer build on the CPU:
//   g++ -O1 -g -std=c++14 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o vel_tetrad_check vel_tetrad_check.cpp
// usage: vel_tetrad_check t r theta phi ut ur utheta uphi spin  ->  one line of 16 + 4 + 1 hexadecimal doubles: the tetrad [leg][component], u / sqrt(g(u, u)),
// g(u, u).  Exit 2 when a leg's norm is off by more than 1e-12 of the sum of its absolute terms (the tests compare the printed bits themselves).
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../raytrace_cpu_amd/csrc/kr_vel_tetrad.hpp"

int main(int argc, char** argv)
{
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s t r theta phi ut ur utheta uphi spin\n", argv[0]);
        return 1;
    }
    double pos[4], u[4];
    for (int i = 0; i < 4; i++) {
        pos[i] = std::strtod(argv[1 + i], nullptr);
        u[i] = std::strtod(argv[5 + i], nullptr);
    }
    const double spin = std::strtod(argv[9], nullptr);
    krvel::Frame f;
    krvel::solve_tetrad(pos, u, spin, &f);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) std::printf("%a ", f.tetrad[i][j]);
    for (int j = 0; j < 4; j++) std::printf("%a ", f.un[j]);
    std::printf("%a\n", f.norm_u);
    const double g[4][4] = {{f.g00, 0, 0, f.g03}, {0, f.g11, 0, 0}, {0, 0, f.g22, 0}, {f.g03, 0, 0, f.g33}};
    for (int i = 0; i < 4; i++) {
        double norm = 0, scale = 0;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                norm += g[a][b] * f.tetrad[i][a] * f.tetrad[i][b];
                scale += std::fabs(g[a][b] * f.tetrad[i][a] * f.tetrad[i][b]);
            }
        if (!(std::fabs(norm - (i == 0 ? 1 : -1)) <= 1e-12 * scale)) return 2;
    }
    return 0;
}
