// raytracer/healpix_pointsource.h -- point source whose sky is sampled by the pixels of a HEALPix sphere, orbiting or moving radially.
//
// API contract of the reference's src/raytracer/healpix_pointsource.h: HealpixPointSource<T>(pos, V, spin, order, motion, basis, tol), five rays
// per pixel (ray 5 pix + i: corners i = 0..3, centre i = 4), get_num_pix(), set_disc_source(), redshift_start(reverse), redshift(V, reverse).  The reference's class is
// written against ray arrays that its Raytracer no longer has and does not compile; this one fills the live rays[] with the rule that
// include/kr_trace.h states under kr_healpix_source (pixel geometry of healpix.h with its quirks -- csrc/kr_healpix_geom.hpp, the one definition
// the device source uses too -- and the constants of calc_consts_from_vector operation for operation) -- the rule kr_healpix_init_dev_f64 follows.  The constructor runs on the host with the C library (build with
// -ffp-contract=off, like the rest of the mirror); run_raytrace() then takes the base class's path to the GPU.
//
// Deliberate difference: redshift_start() takes the emitted energy in the frame the photons were launched in.  For motion 1 that is the radially
// moving source, u = (u_t, V u_t, 0, 0); the reference takes the orbital frame for both motions, which spreads the "emitted" energy of a source
// moving at dr/dt = 0.3 over 0.587 ... 1.704 E.  That energy is g_ij u^i p^j with the momentum the tetrad launched the photon with, not with the one
// rebuilt from k, h, Q: the rebuilding takes p^r from the null condition, and the un-normalised centre vector is not null.
#ifndef HEALPIX_POINTSOURCE_H_
#define HEALPIX_POINTSOURCE_H_

#include <stdexcept>

#include "raytracer.h"
#include "../../csrc/kr_healpix_geom.hpp"

namespace krhost_healpix {

// the C library's sin and cos for the shared pixel geometry (csrc/kr_healpix_geom.hpp)
template <typename T>
struct HostMath {
    static void sincos(T x, T& s, T& c) { s = sin(x); c = cos(x); }
};

// four corners (12 values) and their un-normalised average
template <typename T>
void pixel_vectors(int order, int pix, T* corners, T* centre)
{
    T v[15];
    krhpx::pixel_vectors<HostMath<T>, T>(order, pix, 0, v);
    for (int c = 0; c < 12; c++) corners[c] = v[c];
    for (int c = 0; c < 3; c++) centre[c] = v[12 + c];
}

}  // namespace krhost_healpix

template <typename T>
class HealpixPointSource : public Raytracer<T> {
public:
    HealpixPointSource(T* pos, T V, T spin, int order, int motion = 0, int basis = 0, T tol = TOL)
        : Raytracer<T>(checked_rays(order, motion, basis), spin, tol), velocity(V), source_motion(motion), source_order(order)
    {
        for (int c = 0; c < 4; c++) source_pos[c] = pos[c];
        nside = 1 << order;
        npix = 12 * nside * nside;
        init_healpix_pointsource(pos, order, motion, basis);
    }

    int get_num_pix() { return npix; }

    // a source on the disc: the rays that start towards increasing theta, into the disc under it, become unused slots
    void set_disc_source()
    {
        Ray<T>* rays = Raytracer<T>::rays;
        for (int i = 0; i < Raytracer<T>::nRays; i++)
            if (rays[i].thetadot_sign > 0) rays[i].steps = -1;
    }

    void init_healpix_pointsource(T* pos, int order, int motion, int basis)
    {
        Ray<T>* rays = Raytracer<T>::rays;
#pragma omp parallel for schedule(static) num_threads(kr_host_threads())
        for (int pix = 0; pix < npix; pix++) {
            T vec[15];
            krhost_healpix::pixel_vectors<T>(order, pix, vec, vec + 12);
            for (int i = 0; i < 5; i++) {
                Ray<T>& R = rays[5 * pix + i];
                R.t = pos[0]; R.r = pos[1]; R.theta = pos[2]; R.phi = pos[3];
                R.pt = R.pr = R.ptheta = R.pphi = 0;
                R.steps = 0;
                R.alpha = vec[3 * i + 2];
                R.beta = atan2(vec[3 * i + 1], vec[3 * i]);
                constants_from_vector(R, T(1), &vec[3 * i], velocity, Raytracer<T>::spin, motion, basis);
            }
        }
    }

    // emitted energies in the frame of the source, orbiting or moving radially
    void redshift_start(bool reverse = false)
    {
        if (source_motion == 0) {
            Raytracer<T>::redshift_start(velocity, reverse);
            return;
        }
        Ray<T>* rays = Raytracer<T>::rays;
        const T a = reverse ? -1 * Raytracer<T>::spin : Raytracer<T>::spin, V = velocity;
        const T flip = reverse ? -1 : 1;
#pragma omp parallel for schedule(static) num_threads(kr_host_threads())
        for (int pix = 0; pix < npix; pix++) {
            T vec[15];
            krhost_healpix::pixel_vectors<T>(source_order, pix, vec, vec + 12);
            for (int i = 0; i < 5; i++) {
                Ray<T>& R = rays[5 * pix + i];
                Ray<T> at_source = R;
                at_source.r = source_pos[1]; at_source.theta = source_pos[2];
                T p[4];
                constants_from_vector(at_source, T(1), &vec[3 * i], V, Raytracer<T>::spin, 1, 0, p);
                const T r = at_source.r, st = sin(at_source.theta), ct = cos(at_source.theta);
                const T rhosq = r * r + (a * ct) * (a * ct);
                const T delta = r * r - 2 * r + a * a;
                const T sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st;
                const T e2nu = rhosq * delta / sigmasq;
                const T e2psi = sigmasq * st * st / rhosq;
                const T omega = 2 * a * r / sigmasq;
                const T g00 = e2nu - omega * omega * e2psi, g03 = omega * e2psi, g11 = -rhosq / delta;
                const T ut = 1 / sqrt(g00 + g11 * V * V), ur = V * ut;
                R.emit = g00 * ut * p[0] + g03 * ut * (flip * p[3]) + g11 * ur * (flip * p[1]);
            }
        }
    }

    // received / emitted ratio for material orbiting at V (-1: Keplerian at the ray's end point)
    void redshift(T V, bool reverse = false) { Raytracer<T>::redshift(V, reverse); }
    using Raytracer<T>::redshift;

private:
    int nside, npix;
    T velocity;
    int source_motion, source_order;
    T source_pos[4];

    static int checked_rays(int order, int motion, int basis)
    {
        if (order < 0 || order > 13) throw std::invalid_argument("HealpixPointSource: order must be 0 ... 13");
        if ((motion != 0 && motion != 1) || (basis != 0 && basis != 1) || (motion == 1 && basis == 1))
            throw std::invalid_argument("HealpixPointSource: motion 0 with basis 0 or 1, or motion 1 with basis 0");
        if (order > 12) throw std::invalid_argument("HealpixPointSource: five rays per pixel beyond order 12 do not fit the class API's int ray count");
        return 5 * 12 * (1 << order) * (1 << order);
    }

    // k, h, Q and the two signs of a ray leaving the source along `vec` in the source's frame
    // (p, when given: the momentum the photon is launched with, tdot, rdot, thetadot, phidot)
    static void constants_from_vector(Ray<T>& R, T E, const T* vec, T V, T a, int motion, int basis, T* p = nullptr)
    {
        const T r = R.r, st = sin(R.theta), ct = cos(R.theta), tt = tan(R.theta);
        const T rhosq = r * r + (a * ct) * (a * ct);
        const T delta = r * r - 2 * r + a * a;
        const T sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st;
        const T e2nu = rhosq * delta / sigmasq;
        const T e2psi = sigmasq * st * st / rhosq;
        const T omega = 2 * a * r / sigmasq;
        const T g00 = e2nu - omega * omega * e2psi;
        const T g03 = omega * e2psi;
        const T g11 = -rhosq / delta;
        const T g33 = -e2psi;

        const T rp0 = E, rp1 = E * vec[0], rp2 = E * vec[1], rp3 = E * vec[2];
        T tdot, rdot, thetadot, phidot;
        if (motion == 0) {
            const T et0 = (1 / sqrt(e2nu)) / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
            const T et3 = (1 / sqrt(e2nu)) * V / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
            const T e10 = (V - omega) * sqrt(e2psi / e2nu) / sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
            const T e13 = (1 / sqrt(e2nu * e2psi)) * (e2nu + V * omega * e2psi - omega * omega * e2psi) / sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
            tdot = rp0 * et0 + rp1 * e10;
            phidot = rp0 * et3 + rp1 * e13;
            if (basis == 0) {
                const T e22 = -1 / sqrt(rhosq);
                const T e31 = sqrt(delta / rhosq);
                rdot = rp3 * e31;
                thetadot = rp2 * e22;
            } else {
                const T e32 = -1 / sqrt(rhosq);
                const T e21 = -1 * sqrt(delta / rhosq);
                rdot = rp2 * e21;
                thetadot = rp3 * e32;
            }
        } else {
            const T et0 = 1 / sqrt(g00 + g11 * V * V);
            const T et1 = V * et0;
            const T e12 = 1 / sqrt(rhosq);
            const T e23 = sqrt(g00 / (g03 * g03 - g00 * g33));
            const T e20 = -(g03 / g00) * e23;
            const T e30 = sqrt(-g11 / g00) * V / sqrt(g00 + g11 * V * V);
            const T e31 = sqrt(-g00 / g11) / sqrt(g00 + g11 * V * V);
            tdot = rp0 * et0 + rp1 * e20 + rp3 * e30;
            phidot = rp1 * e23;
            rdot = rp0 * et1 + rp3 * e31;
            thetadot = rp2 * e12;
        }
        const T k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot;
        T h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st);
        h = h - 2 * a * r * k * st * st;
        h = h / (r * r + a * a * ct * ct - 2 * r);
        R.k = k;
        R.h = h;
        R.Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt);
        R.rdot_sign = (rdot > 0) ? 1 : -1;
        R.thetadot_sign = (thetadot > 0) ? 1 : -1;
        if (p) { p[0] = tdot; p[1] = rdot; p[2] = thetadot; p[3] = phidot; }
    }
};

#endif /* HEALPIX_POINTSOURCE_H_ */
