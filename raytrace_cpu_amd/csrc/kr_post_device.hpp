// kr_post_device.hpp -- the per-ray device functions of the O(N) passes either side of the trace (ray sources, redshift_start, redshift,
// range_phi, the emissivity reducer's accumulation), applied by the streaming kernels of kr_post.hip to 144-byte records in HBM; the fused and the
// separate passes share one definition each, so both routes produce the same per-ray bits.  Reference lines cited per function.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "kr_device.hpp"
#include "kr_crmath.hpp"

namespace kr {

// Kerr metric in the (e2nu, e2psi, omega) form used throughout the reference
// (raytracer.cpp:370-388, :491-509, :564-582, :632-639).  Everything up to calculate_momentum below is a template over
// the ray record R (kr_ray_f64 / kr_ray_f32) and computes in the record's scalar type, like the reference's
// Raytracer<double> / Raytracer<float> instantiations of the same source lines.
template <typename T>
struct Metric {
    T rhosq, delta, sigmasq, e2nu, e2psi, omega;
    T g00, g03, g11, g22, g33;
};

template <typename R> struct ScalarOf;
template <> struct ScalarOf<kr_ray_f64> { using type = double; };
template <> struct ScalarOf<kr_ray_f32> { using type = float; };

template <typename T>
KR_DEV Metric<T> kerr_metric(T r, T theta, T a)
{
    Metric<T> m;
    const T st = kr_sin(theta), ct = kr_cos(theta);
    m.rhosq = r * r + (a * ct) * (a * ct);
    m.delta = r * r - 2 * r + a * a;
    m.sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * m.delta * st * st;
    m.e2nu = m.rhosq * m.delta / m.sigmasq;
    m.e2psi = m.sigmasq * st * st / m.rhosq;
    m.omega = 2 * a * r / m.sigmasq;
    m.g00 = m.e2nu - m.omega * m.omega * m.e2psi;
    m.g03 = m.omega * m.e2psi;
    m.g11 = -m.rhosq / m.delta;
    m.g22 = -m.rhosq;
    m.g33 = -m.e2psi;
    return m;
}

// sum_ij g[i][j] * et[i] * p[j] over all 16 entries in row-major order, zeros included, exactly like the
// reference loops (raytracer.cpp:412-415, :547-550): a 0 * inf or 0 * NaN term must poison the sum the same way.
template <typename T>
KR_DEV T energy_dot(const Metric<T>& m, const T* et, const T* p)
{
    const T g[16] = {m.g00, 0, 0, m.g03, 0, m.g11, 0, 0, 0, 0, m.g22, 0, m.g03, 0, 0, m.g33};
    T e = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) e += g[i * 4 + j] * et[i] * p[j];
    return e;
}

template <typename T>
KR_DEV T keplerian_V(T a, T r, T theta, bool projradius)
{
    if (projradius) return 1 / (a + r * kr_sin(theta) * kr_sqrt(r * kr_sin(theta)));
    return 1 / (a + r * kr_sqrt(r));
}

// ---- redshift_start (raytracer.cpp:342-417) ------------------------------------------------------------
// V is a by-value parameter that the reference's loop overwrites when it equals -1, so the orbital velocity
// computed at the FIRST record (index 0, valid or not) is used for every ray.
template <typename R, typename T = typename ScalarOf<R>::type>
KR_DEV T emit_value(const R& ray, T spin, T a, T V, int reverse)
{
    const T r = ray.r, theta = ray.theta;
    const Metric<T> m = kerr_metric<T>(r, theta, a);
    const T et[4] = {(1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu), 0, 0,
                     (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu)};
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    return energy_dot<T>(m, et, p);
}

// ---- redshift(V, ...) (raytracer.cpp:420-447, :480-553) ----------------------------------------------
template <typename R, typename T = typename ScalarOf<R>::type>
KR_DEV T redshift_value(const R& ray, T spin, T V_in, int reverse, int projradius, int motion)
{
    const T a = reverse ? -1 * spin : spin;
    const T r = ray.r, theta = ray.theta;
    const Metric<T> m = kerr_metric<T>(r, theta, a);
    T V = V_in;
    T et[4] = {0, 0, 0, 0};
    if (motion == 0) {
        if (V == -1) V = keplerian_V<T>(a, r, theta, projradius != 0);
        et[0] = (1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu);
        et[3] = (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu);
    } else if (motion == 1) {
        if (V < 0) V = kr_abs(V) * (r * r - 2 * r + spin + spin) / (r * r + spin * spin);   // sic, :531
        et[0] = (T) (1. / kr_sqrt(m.g00 + m.g11 * V * V));                                  // (a double division in the float build too, :533)
        et[1] = V * et[0];
    }
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    const T recv = energy_dot<T>(m, et, p);
    return reverse ? recv / ray.emit : ray.emit / recv;
}

// ---- the photon in the rest frame of the orbiting observer of redshift(V, ..., motion = 0): its momentum on the four legs of the reference's
//      Tetrad (kerr.h:127-170: e_t, e1 along phi, e2 along theta, e3 along r), each by the reference's DotProduct (energy_dot above).  E is the
//      `recv` of redshift_value -- the same metric, e_t and momentum expressions, hence the same bits -- and frame_redshift turns it into that
//      function's return value; P_r = -g(p, e3), P_th = -g(p, e2), P_phi = -g(p, e1).  include/kr_trace.h (kr_angles_dev_f64) has the rule. ----
struct Frame { double E, P_r, P_th, P_phi; };

KR_DEV Frame frame_value(const kr_ray_f64& ray, double spin, double V_in, int reverse, int projradius)
{
    using T = double;
    const T a = reverse ? -1 * spin : spin;
    const T r = ray.r, theta = ray.theta;
    const Metric<T> m = kerr_metric<T>(r, theta, a);
    T V = V_in;
    if (V == -1) V = keplerian_V<T>(a, r, theta, projradius != 0);
    const T et[4] = {(1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu), 0, 0,
                     (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu)};
    const T e1[4] = {(V - m.omega) * kr_sqrt(m.e2psi / m.e2nu) / kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi), 0, 0,
                     (1 / kr_sqrt(m.e2nu * m.e2psi)) * (m.e2nu + V * m.omega * m.e2psi - m.omega * m.omega * m.e2psi) /
                         kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi)};
    const T e2[4] = {0, 0, 1 / kr_sqrt(m.rhosq), 0};
    const T e3[4] = {0, kr_sqrt(m.delta / m.rhosq), 0, 0};
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    Frame f;
    f.E = energy_dot<T>(m, et, p);
    f.P_phi = -1 * energy_dot<T>(m, e1, p);
    f.P_th = -1 * energy_dot<T>(m, e2, p);
    f.P_r = -1 * energy_dot<T>(m, e3, p);
    return f;
}

// ---- the disc flow "Keplerian, plunging inside the ISCO" (include/kr_trace.h, KR_V_PLUNGE; a compile-time parameter of the kernels that evaluate a
//      frame or a redshift, so that the instance of every other V is the code it was).  DiscFlow<false> carries nothing; DiscFlow<true> the ISCO of the
//      metric's a and the energy and angular momentum of its circular orbit, computed once per launch on the host (plunge_flow, kr_pass.hpp).  At
//      r >= r_ms the plunge instance runs the expressions of frame_value / redshift_value with V = -1, operation for operation; at r < r_ms the gas is
//      on the equatorial geodesic with those constants (host/include/disc.h plunge_velocity, in double), e_t = u, e2 stays, and e3 (r-like), e1
//      (phi-like) come from Gram-Schmidt against the metric seeded with d/dr, then d/dphi, oriented e3^r > 0, e1^phi > 0
//      (host/include/gramschmidt_basis.h).  Both sides share one metric and one momentum evaluation. ----
template <bool PLUNGE> struct DiscFlow {};
template <> struct DiscFlow<true> { double r_ms, E_ms, L_ms; };

// a four-vector in named scalars: the two sides of the per-lane r < r_ms branch hand whole vectors on, and both stay in registers (the plunge
// instances take the 32 bytes of scratch per lane that every kernel of these files takes, -Rpass-analysis=kernel-resource-usage, and no more)
struct Vec4 { double t, r, th, ph; };

// energy_dot on two Vec4: the same sixteen terms in the same order
KR_DEV double vec_dot(const Metric<double>& m, const Vec4& x, const Vec4& y)
{
    const double xa[4] = {x.t, x.r, x.th, x.ph}, ya[4] = {y.t, y.r, y.th, y.ph};
    return energy_dot<double>(m, xa, ya);
}

KR_DEV Vec4 plunge_velocity(const DiscFlow<true>& fl, double r, double a)
{
    const double delta = r * r - 2 * r + a * a;
    const double k = fl.E_ms, h = fl.L_ms;
    const double rad = k * k - 1 + 2 / r + (a * a * (k * k - 1) - h * h) / (r * r) + 2 * (h - a * k) * (h - a * k) / (r * r * r);
    Vec4 u;
    u.t = ((r * r + a * a + 2 * a * a / r) * k - 2 * a * h / r) / delta;
    u.r = -1 * kr_sqrt(rad > 0 ? rad : 0.0);
    u.th = 0;
    u.ph = (2 * a * k / r + (1 - 2 / r) * h) / delta;
    return u;
}

// the r-like and phi-like legs of the observer u by Gram-Schmidt: projections removed leg by leg before any leg is normalised, as the host class does
KR_DEV void plunge_legs(const Metric<double>& m, const Vec4& u, Vec4* e1, Vec4* e3)
{
    const Vec4 seed_r = {0, 1, 0, 0}, seed_phi = {0, 0, 0, 1};
    const double uu = vec_dot(m, u, u);
    const double c3 = vec_dot(m, seed_r, u) / uu;
    const Vec4 v3 = {seed_r.t - c3 * u.t, seed_r.r - c3 * u.r, seed_r.th - c3 * u.th, seed_r.ph - c3 * u.ph};
    const double n3 = vec_dot(m, v3, v3);
    const double c1 = vec_dot(m, seed_phi, u) / uu, c13 = vec_dot(m, seed_phi, v3) / n3;
    const Vec4 v1 = {(seed_phi.t - c1 * u.t) - c13 * v3.t, (seed_phi.r - c1 * u.r) - c13 * v3.r, (seed_phi.th - c1 * u.th) - c13 * v3.th,
                     (seed_phi.ph - c1 * u.ph) - c13 * v3.ph};
    const double n1 = vec_dot(m, v1, v1);
    const double l3 = (v3.r < 0 ? -1 : 1) * kr_sqrt(kr_abs(n3)), l1 = (v1.ph < 0 ? -1 : 1) * kr_sqrt(kr_abs(n1));
    *e3 = Vec4{v3.t / l3, v3.r / l3, v3.th / l3, v3.ph / l3};
    *e1 = Vec4{v1.t / l1, v1.r / l1, v1.th / l1, v1.ph / l1};
}

// e_t of the flow at (r, theta): the plunging gas inside r_ms, the circular orbit of V = -1 (redshift_value's expressions) from r_ms on
KR_DEV Vec4 flow_et(const DiscFlow<true>& fl, const Metric<double>& m, double r, double theta, double a, int projradius, bool inside)
{
    if (inside) return plunge_velocity(fl, r, a);
    const double V = keplerian_V<double>(a, r, theta, projradius != 0);
    return Vec4{(1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu), 0, 0,
                (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu)};
}

template <bool PLUNGE>
KR_DEV Frame frame_value(const kr_ray_f64& ray, double spin, double V_in, int reverse, int projradius, const DiscFlow<PLUNGE>& fl)
{
    if constexpr (!PLUNGE) {
        return frame_value(ray, spin, V_in, reverse, projradius);
    } else {
        using T = double;
        const T a = reverse ? -1 * spin : spin;
        const T r = ray.r, theta = ray.theta;
        const Metric<T> m = kerr_metric<T>(r, theta, a);
        const bool inside = r < fl.r_ms;
        const Vec4 et = flow_et(fl, m, r, theta, a, projradius, inside);
        Vec4 e1, e3;
        if (inside) {
            plunge_legs(m, et, &e1, &e3);
        } else {
            const T V = keplerian_V<T>(a, r, theta, projradius != 0);
            e1 = Vec4{(V - m.omega) * kr_sqrt(m.e2psi / m.e2nu) / kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi), 0, 0,
                      (1 / kr_sqrt(m.e2nu * m.e2psi)) * (m.e2nu + V * m.omega * m.e2psi - m.omega * m.omega * m.e2psi) /
                          kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi)};
            e3 = Vec4{0, kr_sqrt(m.delta / m.rhosq), 0, 0};
        }
        const Vec4 e2 = {0, 0, 1 / kr_sqrt(m.rhosq), 0};
        Vec4 p;
        momentum<T>(p.t, p.r, p.th, p.ph, ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
        if (reverse) { p.r *= -1; p.th *= -1; p.ph *= -1; }
        Frame f;
        f.E = vec_dot(m, et, p);
        f.P_phi = -1 * vec_dot(m, e1, p);
        f.P_th = -1 * vec_dot(m, e2, p);
        f.P_r = -1 * vec_dot(m, e3, p);
        return f;
    }
}

// redshift_value for the flow: only e_t is evaluated.  (R, T stay template parameters so that the f32 kernels name the same function; the plunge
// instance exists for f64 records alone.)
template <bool PLUNGE, typename R, typename T = typename ScalarOf<R>::type>
KR_DEV T redshift_value(const R& ray, T spin, T V_in, int reverse, int projradius, int motion, const DiscFlow<PLUNGE>& fl)
{
    if constexpr (!PLUNGE) {
        return redshift_value(ray, spin, V_in, reverse, projradius, motion);
    } else {
        const T a = reverse ? -1 * spin : spin;
        const T r = ray.r, theta = ray.theta;
        const Metric<T> m = kerr_metric<T>(r, theta, a);
        const Vec4 et = flow_et(fl, m, r, theta, a, projradius, r < fl.r_ms);
        Vec4 p;
        momentum<T>(p.t, p.r, p.th, p.ph, ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
        if (reverse) { p.r *= -1; p.th *= -1; p.ph *= -1; }
        const T recv = vec_dot(m, et, p);
        return reverse ? recv / ray.emit : ray.emit / recv;
    }
}

KR_DEV double frame_redshift(const Frame& f, double emit, int reverse) { return reverse ? f.E / emit : emit / f.E; }

// mu = |P_th| / E, the cosine of the angle to the disc normal; chi = atan2(P_phi, P_r), the azimuth about it (0 radially outward, +pi/2 along
// the orbital motion).  A record is bad-angle when mu is not finite, mu > 1 or E <= 0: a ray the integrator stepped past a radial turning point
// has rdot^2 < 0 under the sqrt(|.|) of the momentum, and its state is not a null vector.
KR_DEV double frame_mu(const Frame& f) { return kr_abs(f.P_th) / f.E; }
KR_DEV double frame_chi(const Frame& f) { return atan2(f.P_phi, f.P_r); }
KR_DEV bool frame_bad_angle(const Frame& f, double mu) { return !__builtin_isfinite(mu) || mu > 1 || !(f.E > 0); }

// the limb law of kr_limb_law at mu (law validated on the host: 0, 1 or 2)
KR_DEV double limb_weight(int law, double coeff, double mu)
{
    if (law == 1) return 1 + coeff * mu;
    if (law == 2) return kr_log(1 + 1 / mu);
    return 1;
}

// ---- frame_value with the sine and cosine of theta and the two metric coefficients that the normal of a disc SURFACE needs (DiscSurface,
//      kr_disc_pass.hpp), from the one metric evaluation: expression for expression frame_value, so E keeps redshift_value's bits ----
struct FrameCoef { double sn, cs, delta, rhosq; };

KR_DEV Frame frame_value_coef(const kr_ray_f64& ray, double spin, double V_in, int reverse, int projradius, FrameCoef* mc)
{
    using T = double;
    const T a = reverse ? -1 * spin : spin;
    const T r = ray.r, theta = ray.theta;
    const Metric<T> m = kerr_metric<T>(r, theta, a);
    kr_sincos(theta, mc->sn, mc->cs);            // (kerr_metric's own pair: one evaluation after inlining)
    mc->delta = m.delta;
    mc->rhosq = m.rhosq;
    T V = V_in;
    if (V == -1) V = keplerian_V<T>(a, r, theta, projradius != 0);
    const T et[4] = {(1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu), 0, 0,
                     (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu)};
    const T e1[4] = {(V - m.omega) * kr_sqrt(m.e2psi / m.e2nu) / kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi), 0, 0,
                     (1 / kr_sqrt(m.e2nu * m.e2psi)) * (m.e2nu + V * m.omega * m.e2psi - m.omega * m.omega * m.e2psi) /
                         kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi)};
    const T e2[4] = {0, 0, 1 / kr_sqrt(m.rhosq), 0};
    const T e3[4] = {0, kr_sqrt(m.delta / m.rhosq), 0, 0};
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    Frame f;
    f.E = energy_dot<T>(m, et, p);
    f.P_phi = -1 * energy_dot<T>(m, e1, p);
    f.P_th = -1 * energy_dot<T>(m, e2, p);
    f.P_r = -1 * energy_dot<T>(m, e3, p);
    return f;
}

// ---- the polarisation of disc emission carried to a distant image plane (include/kr_trace.h, kr_polarisation_dev_f64).  The frame is frame_value's,
//      expression for expression -- E and mu keep its bits, so `redshift` is redshift_value's return value -- and the legs e1, e3 and the momentum p it
//      is built from go on into the emitted polarisation vector f = (P_phi e3 - P_r e1) / nrm and the Walker-Penrose constant
//      kappa = (A - iB)(r - i a cos theta), which is inverted at the observer with the ray's own image-plane coordinates (alpha, beta) and the sine of
//      the plane's inclination.  c2, s2 = cos, sin of twice the polarisation angle, from the image's x axis towards its y axis. ----
struct Polar {
    Frame f;
    double redshift, mu, kappa1, kappa2, c2, s2;
    bool bad;           // bad-pol: bad-angle, nrm == 0, or a kappa1, kappa2, c2, s2 that is not finite
};

KR_DEV Polar polar_value(const kr_ray_f64& ray, double spin, double V_in, int reverse, int projradius, double sin_incl)
{
    using T = double;
    const T a = reverse ? -1 * spin : spin;
    const T r = ray.r, theta = ray.theta;
    const Metric<T> m = kerr_metric<T>(r, theta, a);
    T V = V_in;
    if (V == -1) V = keplerian_V<T>(a, r, theta, projradius != 0);
    const T et[4] = {(1 / kr_sqrt(m.e2nu)) / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu), 0, 0,
                     (1 / kr_sqrt(m.e2nu)) * V / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu)};
    const T e1[4] = {(V - m.omega) * kr_sqrt(m.e2psi / m.e2nu) / kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi), 0, 0,
                     (1 / kr_sqrt(m.e2nu * m.e2psi)) * (m.e2nu + V * m.omega * m.e2psi - m.omega * m.omega * m.e2psi) /
                         kr_sqrt(m.e2nu - (V - m.omega) * (V - m.omega) * m.e2psi)};
    const T e2[4] = {0, 0, 1 / kr_sqrt(m.rhosq), 0};
    const T e3[4] = {0, kr_sqrt(m.delta / m.rhosq), 0, 0};
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], ray.k, ray.h, ray.Q, ray.rdot_sign, ray.thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    Polar q;
    q.f.E = energy_dot<T>(m, et, p);
    q.f.P_phi = -1 * energy_dot<T>(m, e1, p);
    q.f.P_th = -1 * energy_dot<T>(m, e2, p);
    q.f.P_r = -1 * energy_dot<T>(m, e3, p);
    q.redshift = frame_redshift(q.f, ray.emit, reverse);
    q.mu = frame_mu(q.f);

    // f in coordinates (f^theta = 0): g(f, p) = 0 and g(f, f) = -1 by construction
    const T nrm = kr_sqrt(q.f.P_r * q.f.P_r + q.f.P_phi * q.f.P_phi);
    const T f_t = -1 * q.f.P_r * e1[0] / nrm, f_r = q.f.P_phi * e3[1] / nrm, f_th = 0, f_phi = -1 * q.f.P_r * e1[3] / nrm;
    const T s = kr_sin(theta), c = kr_cos(theta);
    const T A = (p[0] * f_r - p[1] * f_t) + a * s * s * (p[1] * f_phi - p[3] * f_r);
    const T B = ((r * r + a * a) * (p[3] * f_th - p[2] * f_phi) - a * (p[0] * f_th - p[2] * f_t)) * s;     // the zero terms stay: 0 * inf poisons as in the rule
    q.kappa1 = r * A - a * c * B;
    q.kappa2 = -1 * (r * B + a * c * A);

    // the observer: pixel (x, y) = (alpha, beta) has the impact parameters (-x, -y)
    const T al = -1 * ray.alpha, be = -1 * ray.beta;
    const T nu = -1 * (al + a * sin_incl);
    const T d = nu * nu + be * be;
    const T f_al = (be * q.kappa2 - nu * q.kappa1) / d, f_be = (be * q.kappa1 + nu * q.kappa2) / d;
    const T n2 = f_al * f_al + f_be * f_be;
    q.c2 = (f_al * f_al - f_be * f_be) / n2;
    q.s2 = 2 * f_al * f_be / n2;
    q.bad = frame_bad_angle(q.f, q.mu) || nrm == 0 || !__builtin_isfinite(q.kappa1) || !__builtin_isfinite(q.kappa2) || !__builtin_isfinite(q.c2) ||
            !__builtin_isfinite(q.s2);
    return q;
}

// the degree law of kr_pol_law at mu (law validated on the host: 0 or 1)
KR_DEV double pol_degree(int law, double coeff, double mu)
{
    if (law == 1) return coeff * (1 - mu) / (1 + 3.582 * mu);
    return coeff;
}

// the geodesic, `emit` and the image-plane coordinates that polar_value reads, copied out of a record that the pass goes on to write to
KR_DEV kr_ray_f64 polar_record_of(const kr_ray_f64* ray)
{
    kr_ray_f64 v;
    v.r = ray->r; v.theta = ray->theta; v.k = ray->k; v.h = ray->h; v.Q = ray->Q; v.rdot_sign = ray->rdot_sign; v.thetadot_sign = ray->thetadot_sign;
    v.emit = ray->emit; v.alpha = ray->alpha; v.beta = ray->beta;
    return v;
}

// ---- range_phi (raytracer.cpp:603-622): repeated +-2pi like the reference, so the result is bit-identical.  2 * M_PI is a double:
//      in the float build each `phi -= 2 * M_PI` is a double subtraction rounded back to float, here as there. ----
template <typename T>
KR_DEV T range_phi_value(T phi, int steps, T lo, T hi)
{
    if (kr_abs(phi) > 1000 || phi != phi || !(steps > 0)) return phi;
    while (phi >= hi) phi -= 2 * kPi;
    while (phi < lo) phi += 2 * kPi;
    return phi;
}

// ---- PointSource ctor: Raytracer ctor (steps=-1, status=0, raytracer.cpp:45-49) + init_pointsource
//      (pointsource.cpp:30-64) + calculate_constants (raytracer.cpp:625-676).  Fields the reference leaves
//      indeterminate are zeroed. ------------------------------------------------------------------------
// The constructor's transcendental values, tabulated ON THE HOST with the C library the reference itself calls: alpha = acos(cos alpha) takes
// only n_cosalpha distinct values over the whole grid, beta n_beta, and the source position is one point -- so sin(alpha_i), cos(alpha_i), sin(beta_j),
// cos(beta_j) (two small device arrays: 100 KB at 1e7 rays) and sin / cos / tan of the source's polar angle (three scalars) carry glibc's bits
// and everything that is left for the device is + - x / sqrt, which is IEEE on both sides: k, h, Q of EVERY device-built ray are the reference
// constructor's, bit for bit (with the device library's acos 5 % of the rays differed in the last bit of h and Q, and on chaotic rays that is
// another bin).  kr_post.hip::source_tables builds the arrays once per (device, grid) in the device table store (TablePins, kr_common.hpp).
struct SourceTables {
    const double2* alpha_sc;     // [n_cosalpha]  (sin, cos) of acos(cosalpha0 + i dcosalpha)     pointsource.cpp:38,46; raytracer.cpp:653
    const double2* beta_sc;      // [n_beta]      (sin, cos) of beta0 + j dbeta                   pointsource.cpp:39;    raytracer.cpp:653
    double sin_th, cos_th, tan_th;   // of pos[2]                                                 raytracer.cpp:631-672
};

KR_DEV kr_ray_f64 pointsource_ray(const kr_pointsource& s, const SourceTables& tb, long long n_grid, int n_beta, long long ix)
{
    kr_ray_f64 ray;
        memset(&ray, 0, sizeof(ray));
        ray.steps = -1;
        if (ix < n_grid) {
            const int i = (int) (ix / n_beta), j = (int) (ix % n_beta);
            const double cosalpha = s.cosalpha0 + i * s.dcosalpha;
            const double beta = s.beta0 + j * s.dbeta;
            if (!(cosalpha >= s.cosalphamax || beta >= s.betamax)) {
                const double2 a_sc = tb.alpha_sc[i], b_sc = tb.beta_sc[j];
                const double sin_alpha = a_sc.x, cos_alpha = a_sc.y, sin_beta = b_sc.x, cos_beta = b_sc.y;
                ray.alpha = cosalpha;      // sic: cos(alpha), pointsource.cpp:48
                ray.beta = beta;
                ray.t = s.pos[0]; ray.r = s.pos[1]; ray.theta = s.pos[2]; ray.phi = s.pos[3];
                ray.steps = 0;

                const double spin = s.spin, V = s.V, E = s.E;
                const double r = ray.r;
                const double st = tb.sin_th, ct = tb.cos_th;
                const double rhosq = r * r + (spin * ct) * (spin * ct);
                const double delta = r * r - 2 * r + spin * spin;
                const double sigmasq = (r * r + spin * spin) * (r * r + spin * spin) - spin * spin * delta * st * st;
                const double e2nu = rhosq * delta / sigmasq;
                const double e2psi = sigmasq * st * st / rhosq;
                const double omega = 2 * spin * r / sigmasq;

                const double et0 = (1 / kr_sqrt(e2nu)) / kr_sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
                const double et3 = (1 / kr_sqrt(e2nu)) * V / kr_sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
                const double e10 = (V - omega) * kr_sqrt(e2psi / e2nu) / kr_sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
                const double e13 = (1 / kr_sqrt(e2nu * e2psi)) * (e2nu + V * omega * e2psi - omega * omega * e2psi) /
                                   kr_sqrt(e2nu - (V - omega) * (V - omega) * e2psi);
                const double e22 = -1 / kr_sqrt(rhosq);
                const double e31 = kr_sqrt(delta / rhosq);

                const double rp0 = E, rp1 = E * sin_alpha * cos_beta, rp2 = E * sin_alpha * sin_beta, rp3 = E * cos_alpha;
                const double tdot = rp0 * et0 + rp1 * e10;
                const double phidot = rp0 * et3 + rp1 * e13;
                const double rdot = rp3 * e31;
                const double thetadot = rp2 * e22;

                ray.k = (1 - 2 * r / rhosq) * tdot + (2 * spin * r * st * st / rhosq) * phidot;
                double h = phidot * ((r * r + spin * spin) * (r * r + spin * spin * ct * ct - 2 * r) * st * st + 2 * spin * spin * r * st * st * st * st);
                h = h - 2 * spin * r * ray.k * st * st;
                h = h / (r * r + spin * spin * ct * ct - 2 * r);
                ray.h = h;
                const double tt = tb.tan_th;
                ray.Q = rhosq * rhosq * thetadot * thetadot - (spin * ray.k * ct + h / tt) * (spin * ray.k * ct - h / tt);
                ray.rdot_sign = (rdot >= 0) ? 1 : -1;
                ray.thetadot_sign = (thetadot > 0) ? 1 : -1;
            }
        }
    return ray;
}

// ---- redshift(RayDestination*, ...) with the default four_velocity (raytracer.cpp:450-477, :556-600; ray_destination.h:59-78): the energy ratio
//      of one record against the equatorial Keplerian flow at its end point.  kr_post.hip::redshift_dest_kernel and the caustic epilogue
//      (kr_caustic.hip) share it. -----------------------------------------------------------------------------------------------------
template <typename T>
KR_DEV T redshift_dest_value(T r, T theta, T k, T h, T Q, int rdot_sign, int thetadot_sign, T emit, T spin, int reverse)
{
    const Metric<T> m = kerr_metric<T>(r, theta, spin);
    const T V = 1 / (spin + r * kr_sqrt(r));
    const T gamma_factor = 1 / kr_sqrt(1 - (V - m.omega) * (V - m.omega) * m.e2psi / m.e2nu);
    const T et[4] = {gamma_factor / kr_sqrt(m.e2nu), 0, 0, gamma_factor * V / kr_sqrt(m.e2nu)};
    T p[4];
    momentum<T>(p[0], p[1], p[2], p[3], k, h, Q, rdot_sign, thetadot_sign, r, theta, spin);
    if (reverse) { p[1] *= -1; p[2] *= -1; p[3] *= -1; }
    const T recv = energy_dot<T>(m, et, p);
    return reverse ? recv / emit : emit / recv;
}

// ---- the camera ray through one point (x, y) of a distant image plane (imageplane.cpp:45-113, imageplane_bundles.h:123-196; the host mirror's
//      host/raytracer/image_ray.h::camera_ray): ImagePlane takes it at the grid points, ImagePlaneBundles at the bundle centres and their four
//      satellites.  sin / cos of the inclination come from the host's C library (one angle per plane: PlaneTrig); the per-ray acos, atan2, asin and
//      tan -- N^2 distinct arguments, nothing to tabulate -- are kr_crmath.hpp's correctly rounded routines, sin / cos kr_sincos.hpp's: a device-built
//      ray then differs from the reference constructor's only where the host library itself is not correctly rounded (~1e-3 of the rays in some last
//      bit; the device library's 1-2 ulp routines left 21-25 % of the rays with another phi and 4-7 % with another theta or Q).
//      GUARD_CENTRE: beta = 0 at the point x = y = 0 instead of asin(0 / 0) (the bundles; ImagePlane keeps the reference's NaN there). ----------
struct PlaneTrig { double sin_incl, cos_incl; };

// a slot beyond the source's grid: the Raytracer ctor's record (steps = -1, raytracer.cpp:45-49), the rest zeroed
KR_DEV kr_ray_f64 dead_ray()
{
    kr_ray_f64 ray;
    memset(&ray, 0, sizeof(ray));
    ray.steps = -1;
    return ray;
}

template <bool GUARD_CENTRE>
KR_DEV kr_ray_f64 camera_ray(const PlaneTrig& pt_, double a, double D, double phi0, double x, double y)
{
    kr_ray_f64 ray;
    memset(&ray, 0, sizeof(ray));
    const double si = pt_.sin_incl, ci = pt_.cos_incl;

    const double r = kr_sqrt(D * D + x * x + y * y);
    const double theta = krcr::kr_acos_cr((D * ci + y * si) / r);
    const double phi = phi0 + krcr::kr_atan2_cr(x, D * si - y * ci);

    const double pr = D / r;
    const double ptheta = kr_sin(krcr::kr_acos_cr(D / r)) / r;
    const double pphi = x * si / (x * x + (D * si - y * ci) * (D * si - y * ci));

    const double st = kr_sin(theta), ct = kr_cos(theta);
    const double rhosq = r * r + (a * ct) * (a * ct);
    const double delta = r * r - 2 * r + a * a;
    const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st;
    const double e2nu = rhosq * delta / sigmasq;
    const double e2psi = sigmasq * st * st / rhosq;
    const double omega = 2 * a * r / sigmasq;
    const double g00 = e2nu - omega * omega * e2psi, g03 = omega * e2psi, g11 = -rhosq / delta, g22 = -rhosq, g33 = -e2psi;

    const double A = g00, B = 2 * g03 * pphi;
    const double Cq = g11 * pr * pr + g22 * ptheta * ptheta + g33 * pphi * pphi;
    double pt = (-B + kr_sqrt(B * B - 4 * A * Cq)) / (2 * A);
    if (pt < 0) pt = (-B - kr_sqrt(B * B - 4 * A * Cq)) / (2 * A);

    ray.t = 0; ray.r = r; ray.theta = theta; ray.phi = phi;
    ray.pt = pt; ray.pr = pr; ray.ptheta = ptheta; ray.pphi = pphi;
    ray.rdot_sign = -1;
    ray.k = 1;                                   // calculate_constants_from_p's k/h/Q are overwritten, :100-113

    const double b = kr_sqrt(x * x + y * y);
    double beta = (GUARD_CENTRE && !(b > 0)) ? 0.0 : krcr::kr_asin_cr(y / b);
    if (x < 0) beta = kPi - beta;
    const double h = -1. * b * si * kr_cos(beta);
    const double ltheta = b * kr_sin(beta);
    const double tt = krcr::kr_tan_cr(theta);
    ray.h = h;
    ray.Q = (ltheta * ltheta) - (a * ct) * (a * ct) + ((h / tt)) * ((h / tt));
    ray.thetadot_sign = (ltheta >= 0) ? 1 : -1;
    ray.steps = 0;
    ray.alpha = x;
    ray.beta = y;
    return ray;
}

// ---- powerlaw3 emissivity (imageplane_disc_image.cpp:20-28): the image reducer (kr_post.hip) and the line reducer (kr_line.hip) ----
KR_DEV double powerlaw3(double r, double q1, double rb1, double q2, double rb2, double q3)
{
    if (r < rb1) return kr_pow(r, -1 * q1);
    else if (r < rb2) return kr_pow(rb1, q2 - q1) * kr_pow(r, -1 * q2);
    else return kr_pow(rb1, q2 - q1) * kr_pow(rb2, q3 - q2) * kr_pow(r, -1 * q3);
}

// d_hist layout: [count(nr) | flux(nr) | emis(nr) | sum_redshift(nr) | sum_time(nr) | disc_count(1)], doubles.
// LDS holds one private copy per workgroup when it fits (5*nr+1 doubles); flushed with global f64 atomics.
constexpr int kMaxLdsBins = 1024;

// one ray's contribution to the radial histogram (emissivity.cpp:96-126); acc: LDS copy or the global histogram
KR_DEV void emissivity_accumulate(double* acc, const kr_emis_bins& b, double log_dr, int steps, double r, double theta, double g, double t)
{
    if (!(steps > 0)) return;
    const int nr = b.nr;
    const double z = r * kr_cos(theta);         // cartesian(), kerr.h:55
    if (z < 1E-2 && g > 0 && r >= b.r_isco) {
        // the index rule of kr_emis_bins, decided on the floating quotient BEFORE the conversion (as kr_line.hip does): -1 < q < nr is what the
        // reference's `(int) q` followed by 0 <= ir < nr keeps on the CPU -- the band (-1, 0] truncates to 0 -- and a NaN, infinite or out-of-int-range
        // q fails it, where v_cvt_i32_f64 would saturate and turn NaN into 0, i.e. into bin 0
        const double q = b.logbin ? kr_log(r / b.r_min) / log_dr : (r - b.r_min) / b.dr;
        if (q > -1 && q < nr) {
            const int ir = (int) q;
            atomicAdd(&acc[ir], 1.0);
            atomicAdd(&acc[nr + ir], 1 / (b.num_primary_rays * kr_pow(g, 1.0)));
            atomicAdd(&acc[2 * nr + ir], 1 / kr_pow(g, b.gamma));
            atomicAdd(&acc[3 * nr + ir], g);
            atomicAdd(&acc[4 * nr + ir], t);
        }
        atomicAdd(&acc[5 * nr], 1.0);
    }
}

}  // namespace kr
