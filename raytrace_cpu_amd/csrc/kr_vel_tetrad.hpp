// kr_vel_tetrad.hpp -- the rest frame of an emitter with an arbitrary timelike four-velocity: PointSourceVel::SolveTetrad (pointsource_vel.cpp:113-260)
// restated operation for operation in plain C++ (no HIP), once for the device source (kr_source_vel.hip computes it on the host, per launch, and hands
// it to the kernel by value), for the host class mirror (host/raytracer/pointsource_vel.h) and for the stand-alone check tests/cpp/vel_tetrad_check.cpp.
// Every line is one IEEE operation in the reference's association (compile with -ffp-contract=off); sin / cos / tan are the C library's.
//   metric     rhosq, delta, sigmasq, e2nu, e2psi, omega as everywhere;  g00 = e2nu - omega omega e2psi, g03 = g30 = omega e2psi, g11 = -rhosq / delta,
//              g22 = -rhosq, g33 = -e2psi
//   start      v0 = u (as given, NOT normalised), v1 = d_r, v2 = d_theta, v3 = d_phi
//   orthogonal e_i = v_i - sum_{j < i} (g(v_i, e_j) / g(e_j, e_j)) e_j, classical Gram-Schmidt: the projections are of v_i, not of the running e_i, and
//              are subtracted in the order j = 0, 1, 2.  g(x, y) = sum over all sixteen (a, b), row-major, zeros included, of (g_ab x^a) y^b
//   normalise  e_i /= sqrt(|g(e_i, e_i)|), each component its own division
//   permute    leg 0 = e_0, leg 3 = e_1 (r), leg 1 = e_2 (theta), leg 2 = e_3 (phi)
//   signs      leg 1 negated if its theta component < 0, leg 2 if its phi component < 0, leg 3 if its r component < 0
// Besides the tetrad the frame carries what the emitted energy needs: g(u, u) of the input, u / sqrt(g(u, u)) (four divisions), the five metric components.
#pragma once

#include <cmath>

namespace krvel {

struct Frame {
    double tetrad[4][4];                 // [leg][t, r, theta, phi]
    double un[4];                        // u[a] / sqrt(norm_u)
    double g00, g03, g11, g22, g33;
    double norm_u;                       // g(u, u) of the input u: > 0 for a timelike u
    double sin_th, cos_th, tan_th;       // of pos[2], from the C library
};

inline void solve_tetrad(const double* pos, const double* vel, double spin, Frame* f)
{
    double g[4][4];
    double v[4][4];
    double e[4][4];

    const double r = pos[1];
    const double theta = pos[2];
    const double st = std::sin(theta), ct = std::cos(theta);

    const double rhosq = r * r + (spin * ct) * (spin * ct);
    const double delta = r * r - 2 * r + spin * spin;
    const double sigmasq = (r * r + spin * spin) * (r * r + spin * spin) - spin * spin * delta * st * st;

    const double e2nu = rhosq * delta / sigmasq;
    const double e2psi = sigmasq * st * st / rhosq;
    const double omega = 2 * spin * r / sigmasq;

    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            g[i][j] = 0;
            v[i][j] = 0;
            e[i][j] = 0;
        }

    g[0][0] = e2nu - omega * omega * e2psi;
    g[0][3] = omega * e2psi;
    g[3][0] = g[0][3];
    g[1][1] = -rhosq / delta;
    g[2][2] = -rhosq;
    g[3][3] = -e2psi;

    v[0][0] = vel[0];
    v[0][1] = vel[1];
    v[0][2] = vel[2];
    v[0][3] = vel[3];
    v[1][1] = 1;
    v[2][2] = 1;
    v[3][3] = 1;

    for (int a = 0; a < 4; a++) e[0][a] = v[0][a];

    for (int i = 1; i < 4; i++) {
        for (int a = 0; a < 4; a++) e[i][a] = v[i][a];
        for (int j = 0; j < i; j++) {
            double dotprod = 0;
            double enorm = 0;
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    dotprod += g[a][b] * v[i][a] * e[j][b];
                    enorm += g[a][b] * e[j][a] * e[j][b];
                }
            for (int a = 0; a < 4; a++) e[i][a] -= (dotprod / enorm) * e[j][a];
        }
    }

    for (int i = 0; i < 4; i++) {
        double enorm = 0;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) enorm += g[a][b] * e[i][a] * e[i][b];
        if (i == 0) {
            // the emitter's own four-velocity for the emitted energy: the INPUT u over sqrt(g(u, u)), before e[0] is divided (by sqrt(|g(u, u)|))
            f->norm_u = enorm;
            for (int a = 0; a < 4; a++) f->un[a] = vel[a] / std::sqrt(enorm);
        }
        for (int a = 0; a < 4; a++) e[i][a] /= std::sqrt(std::fabs(enorm));
    }

    static const int leg_of[4] = {0, 3, 1, 2};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) f->tetrad[leg_of[i]][j] = e[i][j];

    if (f->tetrad[1][2] < 0)
        for (int i = 0; i < 4; i++) f->tetrad[1][i] *= -1;
    if (f->tetrad[2][3] < 0)
        for (int i = 0; i < 4; i++) f->tetrad[2][i] *= -1;
    if (f->tetrad[3][1] < 0)
        for (int i = 0; i < 4; i++) f->tetrad[3][i] *= -1;

    f->g00 = g[0][0]; f->g03 = g[0][3]; f->g11 = g[1][1]; f->g22 = g[2][2]; f->g33 = g[3][3];
    f->sin_th = st; f->cos_th = ct; f->tan_th = std::tan(theta);
}

}  // namespace krvel
