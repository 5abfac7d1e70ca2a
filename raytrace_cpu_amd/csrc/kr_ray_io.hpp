// kr_ray_io.hpp -- what every kernel that integrates rays shares besides the step functions of kr_device.hpp: the AoS record <-> registers
// moves and the launch constants made from a kr_params.  Used by kr_trace.hip (the trace) and kr_paths.hip (the recording trace), so that
// both read, integrate and write back a ray the same way.
#pragma once

#include <cmath>
#include <cstring>
#include <limits>

#include "kr_device.hpp"

namespace kr {

// ---- AoS record <-> registers -----------------------------------------------------------------
KR_DEV void load_ray(const kr_ray_f64* p, Lane<double>& s)
{
    const double2* d = reinterpret_cast<const double2*>(p);      // 144-B records, 16-B aligned
    const double2 a0 = d[0], a1 = d[1], a2 = d[2], a3 = d[3], a4 = d[4];
    s.t = a0.x; s.r = a0.y; s.theta = a1.x; s.phi = a1.y;
    s.pt = a2.x; s.pr = a2.y; s.ptheta = a3.x; s.pphi = a3.y;
    s.k = a4.x; s.h = a4.y;
    s.Q = p->Q;
    const int2* iv = reinterpret_cast<const int2*>(&p->steps);
    const int2 i0 = iv[0], i1 = iv[1], i2 = iv[2];
    s.steps0 = i0.x; s.status = i0.y; s.rdot_sign = i1.x; s.thetadot_sign = i1.y; s.rdot_flips = i2.x; s.eq_cross = i2.y;
}

KR_DEV void store_ray(kr_ray_f64* p, const Lane<double>& s, int32_t out_steps)
{
    double2* d = reinterpret_cast<double2*>(p);
    d[0] = make_double2(s.t, s.r);
    d[1] = make_double2(s.theta, s.phi);
    d[2] = make_double2(s.pt, s.pr);
    d[3] = make_double2(s.ptheta, s.pphi);
    int2* iv = reinterpret_cast<int2*>(&p->steps);
    iv[0] = make_int2(out_steps, s.status);
    iv[1] = make_int2(s.rdot_sign, s.thetadot_sign);
    iv[2] = make_int2(s.rdot_flips, s.eq_cross);
}

KR_DEV void load_ray(const kr_ray_f32* p, Lane<float>& s)
{
    s.t = p->t; s.r = p->r; s.theta = p->theta; s.phi = p->phi;
    s.pt = p->pt; s.pr = p->pr; s.ptheta = p->ptheta; s.pphi = p->pphi;
    s.k = p->k; s.h = p->h; s.Q = p->Q;
    s.steps0 = p->steps; s.status = p->status; s.rdot_sign = p->rdot_sign; s.thetadot_sign = p->thetadot_sign;
    s.rdot_flips = p->rdot_flips; s.eq_cross = p->equatorial_crossings;
}

KR_DEV void store_ray(kr_ray_f32* p, const Lane<float>& s, int32_t out_steps)
{
    p->t = s.t; p->r = s.r; p->theta = s.theta; p->phi = s.phi;
    p->pt = s.pt; p->pr = s.pr; p->ptheta = s.ptheta; p->pphi = s.pphi;
    p->steps = out_steps; p->status = s.status; p->rdot_sign = s.rdot_sign; p->thetadot_sign = s.thetadot_sign;
    p->rdot_flips = s.rdot_flips; p->equatorial_crossings = s.eq_cross;
}

// ---- launch constants (host) --------------------------------------------------------------------
template <typename T>
TraceConsts<T> make_consts(const kr_params* p, int steplim)
{
    TraceConsts<T> c;
    c.a = (T) p->spin; c.horizon = (T) p->horizon; c.rlim = (T) p->r_max; c.thetalim = (T) p->theta_max;
    c.precision = (T) p->precision; c.theta_precision = (T) p->theta_precision;
    c.max_tstep = (T) p->max_tstep;
    const T maxtstep_rlim = (T) p->maxtstep_rlim, max_phistep = (T) p->max_phistep;
    c.tol = (T) p->rk45_tol;
    c.sp0 = (T) p->stop_params[0]; c.sp1 = (T) p->stop_params[1]; c.sp2 = (T) p->stop_params[2]; c.sp3 = (T) p->stop_params[3];
    c.inv_precision = (T) (1.0 / p->precision);
    c.inv_theta_precision = (T) (1.0 / p->theta_precision);
    c.rk45_extrapolate = !(p->flags & KR_FLAG_RK45_ITERATE_ALL);
    {
        // div_by_uniform (kr_device.hpp) needs a finite, normal divisor with a normal reciprocal and a significand that is not all ones
        auto qualifies = [](double b) {
            if (!(std::fabs(b) >= 1e-300 && std::fabs(b) <= 1e300)) return false;
            int e;
            const double m = std::frexp(std::fabs(b), &e);          // m in [0.5, 1)
            return m != 1.0 - std::ldexp(1.0, -53);
        };
        c.inv_ok = qualifies(p->precision) && qualifies(p->theta_precision);
    }
    c.steplim = steplim;
    c.stop_kind = p->stop_kind;
    const T inf = std::numeric_limits<T>::infinity();
    set_theta_limits(c);
    c.tstep_rlim_eff = c.max_tstep > 0 ? maxtstep_rlim : -inf;
    {
        unsigned long long bits;
        const double mt = (double) p->max_tstep;
        std::memcpy(&bits, &mt, sizeof bits);
        c.tstep_lo = (uint32_t) bits; c.tstep_on_hi = (uint32_t) (bits >> 32); c.tstep_off_hi = 0x7FE00000u;
    }
    c.phistep_eff = max_phistep > 0 ? max_phistep : inf;
    return c;
}

// effective_steplim, raytracer.cpp:80
inline int effective_steplim(const kr_params* p)
{
    return (p->steplim > 0) ? p->steplim : (p->integrator == KR_RK45) ? KR_RK45_STEPLIM : KR_STEPLIM;
}

}  // namespace kr
