// raytracer/pointsource_vel.h -- point source whose emitter has an arbitrary timelike four-velocity.
//
// API contract of the reference's src/raytracer/pointsource_vel.h: PointSourceVel<T>(pos, u, spin, tol, dcosalpha, dbeta, cosalpha0, cosalphamax,
// beta0, betamax, E) with u the contravariant four-velocity (u^t, u^r, u^theta, u^phi), not necessarily normalised, and the two redshift conveniences
// (here in the mirror's lower-case spelling, as PointSource has them).  The reference's class is written against ray arrays that its Raytracer no
// longer has; this one fills the live rays[] with the rule that include/kr_trace.h states under kr_pointsource_vel_spec -- the tetrad of
// csrc/kr_vel_tetrad.hpp (SolveTetrad operation for operation: the one definition the device source uses too) and InitPointSourceVel step by step --
// the rule kr_pointsource_vel_init_dev_f64 follows.  The constructor runs on the host with the C library (build with -ffp-contract=off, like the
// rest of the mirror: its acos / sin / cos may differ from the device's correctly rounded ones in a last bit); run_raytrace() then takes the base
// class's path to the GPU.  The tetrad is solved in double; only PointSourceVel<double> is supported.
//
// Two deliberate differences.  An out-of-range grid point marks only its own ray (steps = -1, the PointSource rule) where the reference returns from
// the whole constructor (pointsource_vel.cpp:50).  redshift_start() takes the emitted energy in the EMITTER'S frame, g_ab u^a p^b with
// u = u_in / sqrt(g(u_in, u_in)) and the momentum the tetrad launched; the reference's RedshiftStart() (:263-269) takes the frame of an orbit of angular
// velocity `velocity`, a member it never sets.
#ifndef POINTSOURCE_VEL_H_
#define POINTSOURCE_VEL_H_

#include <stdexcept>
#include <string>
#include <type_traits>

#include "raytracer.h"
#include "../../../include/kr_trace.h"
#include "../../csrc/kr_vel_tetrad.hpp"

template <typename T>
class PointSourceVel : public Raytracer<T> {
    static_assert(std::is_same<T, double>::value, "PointSourceVel: the tetrad is solved in double; only PointSourceVel<double> exists");

public:
    PointSourceVel(T* pos, T* V, T spin, T tol, T dcosalpha, T dbeta, T cosalpha0 = -0.999999, T cosalphamax = 0.995, T beta0 = -0.995 * M_PI, T betamax = M_PI,
                   T E = 1)
        : Raytracer<T>(checked_rays(pos, V, spin, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax), spin, tol), energy(E)
    {
        n_cosalpha = ((cosalphamax - cosalpha0) / dcosalpha) + 1;
        n_beta = ((betamax - beta0) / dbeta) + 1;
        krvel::solve_tetrad(pos, V, spin, &frame);
        init_pointsource_vel(pos, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax);
    }

    void init_pointsource_vel(T* pos, T dcosalpha, T dbeta, T cosalpha0, T cosalphamax, T beta0, T betamax)
    {
        Ray<T>* rays = Raytracer<T>::rays;
        const T r = pos[1], a = Raytracer<T>::spin;
        const T st = frame.sin_th, ct = frame.cos_th, tt = frame.tan_th;
        const T rhosq = r * r + (a * ct) * (a * ct);
        for (int i = 0; i < n_cosalpha; i++)
            for (int j = 0; j < n_beta; j++) {
                const int ix = i * n_beta + j;
                if (ix >= Raytracer<T>::nRays) continue;
                Ray<T>& R = rays[ix];
                const T cosalpha = cosalpha0 + i * dcosalpha;
                const T beta = beta0 + j * dbeta;
                if (cosalpha >= cosalphamax || beta >= betamax) {
                    R.steps = -1;
                    continue;
                }
                R.alpha = cosalpha;
                R.beta = beta;
                const T alpha = acos(cosalpha);
                R.t = pos[0]; R.r = pos[1]; R.theta = pos[2]; R.phi = pos[3];
                R.pt = R.pr = R.ptheta = R.pphi = 0;
                R.steps = 0;
                T p[4];
                launched(alpha, beta, p);
                const T tdot = p[0], rdot = p[1], thetadot = p[2], phidot = p[3];
                const T k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot;
                T h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st);
                h = h - 2 * a * r * k * st * st;
                h = h / (r * r + a * a * ct * ct - 2 * r);
                R.k = k;
                R.h = h;
                R.Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt);
                R.rdot_sign = (rdot > 0) ? 1 : -1;
                R.thetadot_sign = (thetadot > 0) ? 1 : -1;
            }
    }

    // the emitter's tetrad, [leg][t, r, theta, phi]
    const double (&tetrad() const)[4][4] { return frame.tetrad; }

    // emitted energies in the emitter's own frame: E to rounding on every ray
    void redshift_start()
    {
        Ray<T>* rays = Raytracer<T>::rays;
        const double g[16] = {frame.g00, 0, 0, frame.g03, 0, frame.g11, 0, 0, 0, 0, frame.g22, 0, frame.g03, 0, 0, frame.g33};
        for (int ix = 0; ix < Raytracer<T>::nRays; ix++) {
            Ray<T>& R = rays[ix];
            if (R.steps == -1) continue;
            T p[4];
            launched(acos(R.alpha), R.beta, p);
            T e = 0;
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) e += g[a * 4 + b] * frame.un[a] * p[b];
            R.emit = e;
        }
    }

    // received / emitted ratio for material orbiting at V (-1: Keplerian at the ray's end point)
    void redshift(T V) { Raytracer<T>::redshift(V); }
    using Raytracer<T>::redshift;

private:
    T energy;
    int n_cosalpha, n_beta;
    krvel::Frame frame;

    // (tdot, rdot, thetadot, phidot) of the photon emitted at polar angles alpha, beta of the emitter's frame (pointsource_vel.cpp:86-91)
    void launched(T alpha, T beta, T* p) const
    {
        const T rp[4] = {energy, energy * sin(alpha) * cos(beta), energy * sin(alpha) * sin(beta), energy * cos(alpha)};
        for (int c = 0; c < 4; c++) p[c] = rp[0] * frame.tetrad[0][c] + rp[1] * frame.tetrad[1][c] + rp[2] * frame.tetrad[2][c] + rp[3] * frame.tetrad[3][c];
    }

    // the reference's ray count, after the checks the library makes of the same arguments (include/kr_trace.h, kr_pointsource_vel_spec)
    static int checked_rays(const T* pos, const T* u, T spin, T dcosalpha, T dbeta, T cosalpha0, T cosalphamax, T beta0, T betamax)
    {
        kr_pointsource_vel_spec s;
        for (int c = 0; c < 4; c++) { s.pos[c] = pos[c]; s.u[c] = u[c]; }
        s.spin = spin; s.tol = 0; s.E = 1;
        s.dcosalpha = dcosalpha; s.dbeta = dbeta; s.cosalpha0 = cosalpha0; s.cosalphamax = cosalphamax; s.beta0 = beta0; s.betamax = betamax;
        double t16[16];
        if (kr_pointsource_vel_tetrad(&s, t16) != KR_OK) throw std::invalid_argument(std::string("PointSourceVel: ") + kr_last_error());
        return (int) kr_pointsource_vel_count(&s, nullptr, nullptr);
    }
};

#endif /* POINTSOURCE_VEL_H_ */
